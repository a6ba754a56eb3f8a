"""Segment-tiled multi-LoRA kernels (lora_sgmv.hip) through
ops.lora_apply(groups=...): against fp64, row independence, host checks,
and the engine above the LORA_SGMV_MIN_T cutoff."""
import pytest
import torch

import helix_amd.ops as ops
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models import lora as L
from helix_amd.models.llama import PRESETS
from wq_oracle import wq_error

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 3
CYCLE = [-1, 0, 2, 1, S, -1]
RUNS = [(1, 21), (-1, 3), (0, 37), (2, 11)]      # run ends never on 16
COLS = 256                                       # expand column block

# K, slice widths, Rmax, adapter rank
CASES = [
    (288, (48, 16, 16), 8, 8),
    (256, (32,), 8, 8),
    (2080, (1024, 1024), 32, 32),
    (512, (COLS + 16,), 64, 64),
    (4096, (512, 128, 128), 16, 8),
]
TS = [1, 15, 16, 17, 65, 130]

# 4 x the worst wq_error, over TS x PATTERNS x CASES, of emulate() below: a
# CPU computation that rounds where the kernels round (fp32 y, fp32 delta,
# one rounding of out to bf16). That worst error is 3.79e-3 (docs/KERNELS.md,
# "lora_sgmv.hip"): the one bf16 rounding of an O(1) output, relative to the
# row's largest value.
TOL = 4 * 3.79e-3


def slots_for(pattern, T):
    if pattern == "cycle":
        s = [CYCLE[(1 + t) % len(CYCLE)] for t in range(T)]
    elif pattern == "runs":
        s = [v for _ in range(T // 72 + 1) for v, n in RUNS for _ in range(n)]
    else:
        s = [2] * T
    return torch.tensor(s[:T], dtype=torch.int32)


def make_case(T, K, widths, Rmax, rank, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + T * 1000 + K)
    ns, N = len(widths), sum(widths)
    n_off = [0]
    for w in widths:
        n_off.append(n_off[-1] + w)
    bf = lambda t: t.to(torch.bfloat16)            # noqa: E731
    x = bf(torch.randn(T, K, generator=g))
    base = bf(torch.randn(T, N, generator=g))
    Ac = bf(torch.randn(S, ns, rank, K, generator=g) / K ** 0.5)
    Bc = bf(torch.randn(S, N, rank, generator=g) / rank ** 0.5)
    A = torch.zeros(S, ns, Rmax, K, dtype=torch.bfloat16)
    A[:, :, :rank] = Ac
    B = torch.zeros(S, N, Rmax, dtype=torch.bfloat16)
    B[:, :, :rank] = Bc
    scale = torch.tensor([0.5, 2.0, 0.5])
    return x, base, Ac, Bc, A.view(S, ns * Rmax, K), B, scale, n_off


def reference(x, base, Ac, Bc, scale, n_off, slot, dtype):
    """Shrink + expand on the compact adapter in `dtype`, not rounded."""
    want = base.to(dtype).clone()
    for t in range(x.shape[0]):
        s = int(slot[t])
        if 0 <= s < S:
            for i in range(len(n_off) - 1):
                y = Ac[s, i].to(dtype) @ x[t].to(dtype)
                want[t, n_off[i]:n_off[i + 1]] += scale[s].to(dtype) * (
                    Bc[s, n_off[i]:n_off[i + 1]].to(dtype) @ y)
    return want


def emulate(x, base, Ac, Bc, scale, n_off, slot):
    return reference(x, base, Ac, Bc, scale, n_off, slot,
                     torch.float32).to(torch.bfloat16)


def run_gpu(x, base, A, B, scale, n_off, slot):
    out = base.to(DEV).clone()
    slot_d = slot.to(DEV)
    ops.lora_apply(out, x.to(DEV), A.to(DEV), B.to(DEV), slot_d,
                   scale.to(DEV), n_off, groups=ops.lora_group(slot_d, S))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("K,widths,Rmax,rank", CASES)
@pytest.mark.parametrize("pattern", ["cycle", "runs", "one"])
@pytest.mark.parametrize("T", TS)
def test_apply_vs_fp64(T, pattern, K, widths, Rmax, rank):
    x, base, Ac, Bc, A, B, scale, n_off = make_case(T, K, widths, Rmax, rank)
    slot = slots_for(pattern, T)
    valid = (slot >= 0) & (slot < S)
    assert valid.any()
    want = reference(x, base, Ac, Bc, scale, n_off, slot, torch.float64)
    # base and delta are both O(1): a wrong slot/slice/scale is an O(1) miss
    assert (want[valid] - base.double()[valid]).abs().mean() > 0.2

    out = run_gpu(x, base, A, B, scale, n_off, slot)
    assert torch.equal(out[~valid].view(torch.int16),
                       base[~valid].view(torch.int16))
    assert not out.float().isnan().any()
    emu = float(wq_error(emulate(x, base, Ac, Bc, scale, n_off, slot)[valid],
                         want[valid]).max())
    err = float(wq_error(out[valid], want[valid]).max())
    print(f"T={T} {pattern} K={K} R={Rmax}: err {err:.3e} emulation {emu:.3e}")
    assert err <= TOL


def test_y_not_written_for_rows_without_adapter():
    x, base, Ac, Bc, A, B, scale, n_off = make_case(17, *CASES[0])
    slot = slots_for("cycle", 17).to(DEV)
    y = torch.full((17, A.shape[1]), float("nan"), device=DEV)
    ops.lora_sgmv_shrink(y, x.to(DEV), A.to(DEV), ops.lora_group(slot, S))
    valid = ((slot >= 0) & (slot < S)).cpu()
    assert y.cpu()[~valid].isnan().all() and not y.cpu()[valid].isnan().any()


@pytest.mark.parametrize("K,widths,Rmax,rank", [CASES[0], CASES[4]])
def test_row_bits_do_not_depend_on_batch(K, widths, Rmax, rank):
    """One row and slot at T = 1, 17, 65, 130 (MT changes above 64): other
    neighbours, other places in its list, the same bits."""
    N = sum(widths)
    _, _, Ac, Bc, A, B, scale, n_off = make_case(1, K, widths, Rmax, rank)
    g = torch.Generator().manual_seed(5)
    xr = torch.randn(K, generator=g).to(torch.bfloat16)
    br = torch.randn(N, generator=g).to(torch.bfloat16)
    got = []
    for T, at, pattern in [(1, 0, "one"), (17, 16, "cycle"), (65, 40, "runs"),
                           (130, 129, "one")]:
        x, base = make_case(T, K, widths, Rmax, rank, seed=T)[:2]
        slot = slots_for(pattern, T)
        x[at], base[at], slot[at] = xr, br, 1
        got.append(run_gpu(x, base, A, B, scale, n_off, slot)[at])
    assert not torch.equal(got[0], br)
    for o in got[1:]:
        assert torch.equal(o.view(torch.int16), got[0].view(torch.int16))


def test_host_checks_reject_bad_arguments():
    T, K, N, R = 4, 64, 32, 16
    x = torch.zeros(T, K, dtype=torch.bfloat16, device=DEV)
    A = torch.zeros(S, R, K, dtype=torch.bfloat16, device=DEV)
    B = torch.zeros(S, N, R, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(T, R, device=DEV)
    out = torch.zeros(T, N, dtype=torch.bfloat16, device=DEV)
    scale = torch.ones(S, device=DEV)
    slot = torch.zeros(T, dtype=torch.int32, device=DEV)
    off, rows = ops.lora_group(slot, S)
    ops.lora_sgmv_shrink(y, x, A, (off, rows))               # the good call
    ops.lora_sgmv_expand(out, y, B, (off, rows), scale, [0, N])
    with pytest.raises(ValueError):
        ops.lora_group(slot, 257)
    big = torch.zeros(258, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):                        # S = 257
        ops.lora_sgmv_shrink(y, x, A.new_zeros(257, R, K), (big, rows))
    with pytest.raises(RuntimeError):                        # K % 32
        ops.lora_sgmv_shrink(y, x.new_zeros(T, 48), A.new_zeros(S, R, 48),
                             (off, rows))
    with pytest.raises(RuntimeError):                        # boundary % 16
        ops.lora_sgmv_expand(out, y.new_zeros(T, 2 * R), B, (off, rows),
                             scale, [0, 8, N])
    for bad in [(off.long(), rows), (off, rows.long()), (off[:S], rows),
                (off, rows[:T - 1]), (off, big[1:T + 1])]:   # dtype/shape/align
        with pytest.raises(RuntimeError):
            ops.lora_sgmv_shrink(y, x, A, bad)
        with pytest.raises(RuntimeError):
            ops.lora_sgmv_expand(out, y, B, bad, scale, [0, N])
    with pytest.raises(RuntimeError):                        # strided out
        ops.lora_sgmv_expand(out.new_zeros(T, 2 * N)[:, :N], y, B,
                             (off, rows), scale, [0, N])


# ---------------------------------------------------------------------------
# Engine: prompts longer than the cutoff, more running sequences than it
# ---------------------------------------------------------------------------
CFG = PRESETS["tiny-gqa"]
SP = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
NSEQ = ops.LORA_SGMV_MIN_T + 3
PROMPTS = [[(7 * i + 3 * s) % 1000 + 1
            for i in range(ops.LORA_SGMV_MIN_T + 9 if s < 2 else 5 + s % 4)]
           for s in range(NSEQ)]
NAMES = [[None, "a1", "a2"][s % 3] for s in range(NSEQ)]


def make_engine(dirs, max_loras, names=(), **kw):
    eng = LLMEngine(EngineConfig(
        model="tiny-gqa", max_model_len=1024, max_num_seqs=NSEQ,
        kv_cache_blocks=2048, max_prefill_tokens=2048, eos_token_id=-1, max_loras=max_loras,
        max_lora_rank=16, **kw), device=DEV)
    for n in names:
        eng.add_lora(n, dirs[n])
    return eng


@pytest.fixture(scope="module")
def engine_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("loras")
    dirs = {}
    for seed, (name, zero) in enumerate(
            [("a1", False), ("a2", False), ("zero", True)], start=1):
        t = L.random_adapter_tensors(CFG, 16, seed=seed, b_std=0.05,
                                     zero_b=zero)
        dirs[name] = L.save_peft_adapter(str(d / name), t, r=16,
                                         lora_alpha=64)
    graph = make_engine(dirs, 2, ("a1", "a2"))
    assert graph.graph_runner is not None
    eager = make_engine(dirs, 2, ("a1", "a2"), enforce_eager=True)
    return {"graph": graph.generate(PROMPTS, SP, loras=NAMES),
            "eager": eager.generate(PROMPTS, SP, loras=NAMES),
            "zero": make_engine(dirs, 2, ("zero",)).generate(
                PROMPTS, SP, loras=["zero"] * NSEQ),
            "base": make_engine(dirs, 0).generate(PROMPTS, SP)}


def test_engine_graph_equals_eager(engine_outputs):
    assert engine_outputs["graph"] == engine_outputs["eager"]


def test_engine_base_rows_and_zero_adapter_equal_base(engine_outputs):
    got, base = engine_outputs["graph"], engine_outputs["base"]
    assert got[0::3] == base[0::3]
    assert engine_outputs["zero"] == base


def test_engine_adapter_rows_differ_from_base(engine_outputs):
    got, base = engine_outputs["graph"], engine_outputs["base"]
    assert got[1] != base[1] and got[2] != base[2]
