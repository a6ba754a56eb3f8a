"""Multi-LoRA on the GPU: shrink/expand HIP kernels vs the fp32 reference,
and adapters through the engine (hipGraph vs eager, mixed batches,
fp8 bases, slot eviction between graph replays)."""
import pytest
import torch

import helix_amd.ops as ops
import helix_amd.ops.reference as ref
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models import lora as L
from helix_amd.models.llama import PRESETS

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 3
CYCLE = [-1, 0, 2, 1, S, -1]

# T, K, slice widths, Rmax, adapter rank, first index into CYCLE
CASES = [
    (1, 256, (512, 128, 128), 8, 8, 1),
    (3, 256, (512, 128, 128), 16, 8, 0),
    (67, 4096, (4096,), 64, 64, 0),
    (5, 14336, (4096,), 16, 16, 1),
    (33, 512, (1024, 1024), 32, 32, 0),
]


def _bf16(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("T,K,widths,Rmax,rank,start", CASES)
def test_shrink_expand_vs_reference(T, K, widths, Rmax, rank, start):
    g = torch.Generator().manual_seed(T * 1000 + K)
    ns, N = len(widths), sum(widths)
    n_off = [0]
    for w in widths:
        n_off.append(n_off[-1] + w)
    x = _bf16(torch.randn(T, K, generator=g))
    base = _bf16(torch.randn(T, N, generator=g))
    # compact rank-`rank` adapters, zero-padded into Rmax-wide stacks
    Ac = _bf16(torch.randn(S, ns, rank, K, generator=g) / K ** 0.5)
    Bc = _bf16(torch.randn(S, N, rank, generator=g) / Rmax ** 0.5)
    A = torch.zeros(S, ns, Rmax, K, dtype=torch.bfloat16)
    A[:, :, :rank] = Ac
    A = A.view(S, ns * Rmax, K)
    B = torch.zeros(S, N, Rmax, dtype=torch.bfloat16)
    B[:, :, :rank] = Bc
    scale = torch.tensor([0.5, 2.0, 0.5])
    slot = torch.tensor([CYCLE[(start + t) % len(CYCLE)] for t in range(T)],
                        dtype=torch.int32)

    # fp32 CPU reference from the compact (unpadded) adapter
    y_ref = torch.zeros(T, ns * rank)
    ref.lora_shrink(y_ref, x.float(), Ac.view(S, ns * rank, K).float(), slot)
    want = ref.lora_expand(base.float().clone(), y_ref, Bc.float(), slot,
                           scale, n_off)

    y = torch.full((T, ns * Rmax), float("nan"), device=DEV)
    out = base.to(DEV).clone()
    slot_d = slot.to(DEV)
    ops.lora_shrink(y, x.to(DEV), A.to(DEV), slot_d)
    ops.lora_expand(out, y, B.to(DEV), slot_d, scale.to(DEV), n_off)
    torch.cuda.synchronize()

    valid = (slot >= 0) & (slot < S)
    assert valid.any()
    out = out.cpu()
    # rows with no adapter: bit-equal to base, and y never written
    assert torch.equal(out[~valid].view(torch.int16),
                       base[~valid].view(torch.int16))
    assert y.cpu()[~valid].isnan().all()
    assert not out.float().isnan().any()
    yv = y.cpu()[valid].view(-1, ns, Rmax)
    torch.testing.assert_close(yv[:, :, :rank],
                               y_ref[valid].view(-1, ns, rank),
                               atol=2e-2, rtol=2e-2)
    assert not yv[:, :, rank:].any()
    # base and delta are both O(1): a wrong slot/slice/scale is an O(1) miss
    assert (want[valid] - base.float()[valid]).abs().mean() > 0.2
    torch.testing.assert_close(out.float(), want, atol=2e-2, rtol=2e-2)


def test_host_checks_reject_bad_arguments():
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=DEV)
    A = torch.zeros(S, 16, 64, dtype=torch.bfloat16, device=DEV)
    B = torch.zeros(S, 32, 16, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(2, 16, device=DEV)
    out = torch.zeros(2, 32, dtype=torch.bfloat16, device=DEV)
    slot = torch.zeros(2, dtype=torch.int32, device=DEV)
    scale = torch.ones(S, device=DEV)
    with pytest.raises(RuntimeError):
        ops.lora_shrink(y, x, A, slot.long())
    with pytest.raises(RuntimeError):
        ops.lora_shrink(y, x[:, :60].contiguous(), A[:, :, :60].contiguous(),
                        slot)
    with pytest.raises(RuntimeError):
        ops.lora_shrink(y[:, :8].contiguous(), x, A, slot)
    with pytest.raises(RuntimeError):
        # two slices need a 32-wide y
        ops.lora_expand(out, y, B, slot, scale, [0, 16, 32])
    with pytest.raises(RuntimeError):
        ops.lora_expand(out, y, B, slot, scale, [0, 16])       # != N
    with pytest.raises(RuntimeError):
        ops.lora_expand(out, y, B[:, :, :4].contiguous(), slot, scale,
                        [0, 32])                               # Rmax 4
    with pytest.raises(RuntimeError):
        ops.lora_expand(out, y, B, slot, scale.double(), [0, 32])


# ---------------------------------------------------------------------------
# Engine
# ---------------------------------------------------------------------------
CFG = PRESETS["tiny-gqa"]
SP = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
PROMPTS = [[(7 * i + 3) % 1000 + 1 for i in range(19)],
           [(11 * i + 5) % 1000 + 1 for i in range(33)],
           [(13 * i + 2) % 1000 + 1 for i in range(8)],
           [(11 * i + 5) % 1000 + 1 for i in range(33)]]
NAMES = [None, "a1", "a2", "a1"]


@pytest.fixture(scope="module")
def adapter_dirs(tmp_path_factory):
    d = tmp_path_factory.mktemp("loras")
    out = {}
    for seed, (name, zero) in enumerate(
            [("a1", False), ("a2", False), ("zero", True)], start=1):
        t = L.random_adapter_tensors(CFG, 16, seed=seed, b_std=0.05,
                                     zero_b=zero)
        out[name] = L.save_peft_adapter(str(d / name), t, r=16,
                                        lora_alpha=64)
    return out


def make_engine(adapter_dirs, max_loras, names=(), **kw):
    eng = LLMEngine(EngineConfig(
        model="tiny-gqa", max_model_len=256, max_num_seqs=8,
        kv_cache_blocks=256, eos_token_id=-1, max_loras=max_loras,
        max_lora_rank=16, **kw), device=DEV)
    for n in names:
        eng.add_lora(n, adapter_dirs[n])
    return eng


@pytest.fixture(scope="module")
def mixed_outputs(adapter_dirs):
    """The [None, a1, a2, a1] batch on a graph engine, an eager engine and
    a max_loras=0 graph engine (computed once, read by several tests)."""
    graph = make_engine(adapter_dirs, 2, ("a1", "a2"))
    assert graph.graph_runner is not None
    eager = make_engine(adapter_dirs, 2, ("a1", "a2"), enforce_eager=True)
    base = make_engine(adapter_dirs, 0)
    res = {"graph": graph.generate(PROMPTS, SP, loras=NAMES),
           "eager": eager.generate(PROMPTS, SP, loras=NAMES),
           "base": base.generate(PROMPTS, SP),
           "free": [e.num_free_blocks() for e in (graph, eager, base)]}
    return res


def test_engine_graph_equals_eager(mixed_outputs):
    assert mixed_outputs["graph"] == mixed_outputs["eager"]
    assert mixed_outputs["free"] == [256, 256, 256]


def test_engine_no_leak_into_base_row(mixed_outputs):
    assert mixed_outputs["graph"][0] == mixed_outputs["base"][0]


def test_engine_adapter_rows_differ_from_base(mixed_outputs):
    got, base = mixed_outputs["graph"], mixed_outputs["base"]
    assert got[1] != base[1] and got[2] != base[2] and got[3] != base[3]
    assert got[1] == got[3]


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_engine_zero_b_adapter_equals_base(adapter_dirs, quant):
    eng = make_engine(adapter_dirs, 2, ("zero",), quantization=quant)
    base = make_engine(adapter_dirs, 0, quantization=quant)
    assert eng.generate(PROMPTS, SP, loras=["zero"] * 4) == \
        base.generate(PROMPTS, SP)
    assert eng.num_free_blocks() == 256


def test_engine_eviction_between_graph_replays(adapter_dirs):
    eng = make_engine(adapter_dirs, 1, ("a1", "a2"))
    assert eng.graph_runner is not None
    first = eng.generate(PROMPTS[:1], SP, loras=["a1"])
    second = eng.generate(PROMPTS[:1], SP, loras=["a2"])
    third = eng.generate(PROMPTS[:1], SP, loras=["a1"])
    assert eng.lora.slots == ["a1"]
    assert third == first and second != first
    assert eng.num_free_blocks() == 256
