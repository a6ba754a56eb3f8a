"""Qwen3 on the GPU, QK-norm weights randomised. The tiny-qwen3 engine
(head_dim 128): hipGraph decode against eager, chunked prefill and
prefix-cache hits against a cold prefill, the e4m3 KV cache, a resident
Q4_K_M file. Prefill logits against the CPU model, for tiny-qwen3 and for
test_qwen3_cpu's Qwen3-MoE config (head_dim 64, 128 experts, top-8; a model,
not a served preset). The routed expert GEMMs at E = 128, k = 8."""
import copy

import pytest
import torch
import torch.nn.functional as F

import helix_amd.ops as ops
import moe_oracle as mo
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import (PRESETS, LlamaForCausalLM, MoEMLP,
                                    PrefillMeta)
from helix_amd.engine.kv_cache import KVCache
from test_qwen3_cpu import CONFIGS, randomize_qk_norms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TINY = ("tiny-qwen3",)


def _mk(preset, seed=7, **kw):
    cfg = EngineConfig(model=preset, max_model_len=512, max_num_seqs=8,
                       kv_cache_blocks=256, eos_token_id=-1, seed=seed, **kw)
    eng = LLMEngine(cfg, device=DEV)
    randomize_qk_norms(eng.model)
    a = eng.model.layers[0].attn
    assert a.q_norm_w.dtype == torch.bfloat16 and a.q_norm_w.is_cuda
    assert not bool((a.q_norm_w == 1).all())
    return eng


@pytest.mark.parametrize("preset", TINY)
def test_graph_matches_eager_greedy(preset):
    """Batch 3 replays the bucket-4 graph, whose pad row has slot -1."""
    prompts = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11], [12] * 33]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    out_eager = _mk(preset, enforce_eager=True).generate(prompts, sp)
    eng = _mk(preset)
    assert eng.graph_runner is not None
    out_graph = eng.generate(prompts, sp)
    assert out_eager == out_graph
    assert all(len(o) == 24 for o in out_graph)


@pytest.mark.parametrize("preset", TINY)
def test_chunked_prefill_matches_single_prefill(preset):
    prompt = [((i * 37) % 500) + 1 for i in range(200)]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)

    def run(budget):
        return _mk(preset, seed=9, enforce_eager=True,
                   max_prefill_tokens=budget).generate([prompt], sp)[0]

    assert run(64) == run(8192)


@pytest.mark.parametrize("preset", TINY)
def test_prefix_cache_hit_matches_cold_prefill(preset):
    """The second request reads the first one's cached K: it must be the
    normed, roped K."""
    system = list(range(1, 49))
    p1 = system + [100, 101, 102]
    p2 = system + [200, 201]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)

    def run(prefix_caching):
        eng = _mk(preset, seed=11, enable_prefix_caching=prefix_caching)
        o1 = eng.generate([p1], sp)[0]
        eng.add_request("r2", p2, sp)
        eng.step()
        cached = eng.seqs["r2"].cached_prefix
        while eng.has_work:
            eng.step()
        return o1, eng.seqs["r2"].output_ids, cached

    o1a, o2a, cached_a = run(True)
    o1b, o2b, cached_b = run(False)
    assert cached_a == 48 and cached_b == 0
    assert o1a == o1b
    assert o2a == o2b


@pytest.mark.parametrize("preset", TINY)
def test_fp8_kv_cache(preset):
    """What tests/test_fp8_kv.py asks of its tiny model, with its prompt and
    seed: at least 6 of 12 greedy tokens agree with the bf16 cache; and
    graph == eager, as tests/test_engine_gpu.py asks of the fp8 cache."""
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    prompts = [[1, 2, 3, 4, 5]]
    want = _mk(preset, seed=5, enforce_eager=True).generate(prompts, sp)[0]
    e8 = _mk(preset, seed=5, enforce_eager=True, kv_cache_dtype="fp8")
    assert e8.kv.caches[0][0].dtype == torch.uint8
    eager = e8.generate(prompts, sp)[0]
    graph = _mk(preset, seed=5, kv_cache_dtype="fp8").generate(prompts, sp)[0]
    assert eager == graph
    assert len(eager) == 12
    agree = sum(a == b for a, b in zip(eager, want))
    print(f"{preset}: fp8 KV agrees with bf16 KV on {agree} of 12 tokens")
    assert agree >= 6, f"fp8-KV diverged early: {eager} vs {want}"


def test_resident_q4_k_m_file_serves(tmp_path):
    """`export-gguf --preset tiny-qwen3 --quant q4_k_m`, loaded with
    keep_quantized: KQLinear projections, bf16 norm weights, and the decode
    hipGraph gives the eager tokens."""
    from helix_amd.engine.gguf import export_model_gguf, load_gguf_weights
    from helix_amd.models.quant import KQLinear
    cfg = PRESETS["tiny-qwen3"]
    src = randomize_qk_norms(LlamaForCausalLM(cfg).init_random(3))
    path = str(tmp_path / "tiny-qwen3-q4_k_m.gguf")
    export_model_gguf(src, path, quant="q4_k_m")

    def engine(eager):
        m = LlamaForCausalLM(cfg)
        load_gguf_weights(m, path, keep_quantized=True)
        m = m.to(torch.bfloat16).to(DEV)
        a = m.layers[0].attn
        assert isinstance(a.qkv_proj, KQLinear)
        assert a.q_norm_w.dtype == torch.bfloat16
        assert torch.equal(a.q_norm_w.cpu(), src.layers[0].attn.q_norm_w
                           .to(torch.bfloat16))
        return LLMEngine(EngineConfig(model="tiny-qwen3", max_model_len=512,
                                      max_num_seqs=8, kv_cache_blocks=256,
                                      eos_token_id=-1, enforce_eager=eager),
                         device=DEV, model=m)

    prompts = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11]]
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    want = engine(True).generate(prompts, sp)
    eng = engine(False)
    assert eng.graph_runner is not None
    assert eng.generate(prompts, sp) == want
    assert all(len(o) == 12 for o in want)


# -- logits against the CPU model ---------------------------------------------

ROUTE_MARGIN = 0.005


def _prefill_logits(model, caches, ids, device, margins=None):
    T = len(ids)
    meta = PrefillMeta(
        cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device=device),
        max_seqlen=T,
        slot_mapping=torch.arange(T, dtype=torch.int64, device=device),
        positions=torch.arange(T, dtype=torch.int64, device=device))
    hooks = []
    if margins is not None:
        def pre(mod, args):
            lg = F.linear(args[0], mod.router_w).float()
            top = lg.sort(dim=-1, descending=True).values
            margins.append(top[:, mod.k - 1] - top[:, mod.k])
        hooks = [m.register_forward_pre_hook(pre) for m in model.modules()
                 if isinstance(m, MoEMLP)]
    with torch.inference_mode():
        h = model(torch.tensor(ids, dtype=torch.int64, device=device),
                  caches, meta)
        out = model.compute_logits(h).float().cpu()
    for hk in hooks:
        hk.remove()
    return out


@pytest.mark.parametrize("preset", tuple(CONFIGS))
def test_prefill_logits_match_the_cpu_model(preset):
    """The same bf16 weights on both sides. Each of the ~12 bf16 roundings
    per layer can fall the other way (2^-9 relative per element, random
    sign): over 2 layers and the head that is ~sqrt(25) * 2^-9 / sqrt(3) =
    0.006 of a row's norm per side, 0.012 for the difference; the bound is
    0.03 of the row's norm. The mixture of experts adds a discrete choice:
    a row whose 8th and 9th router logits are closer than ROUTE_MARGIN in a
    layer (about 3 sigma of a logit's rounding error, 0.0016) may route
    differently and is left out; most rows stay in."""
    cfg = CONFIGS[preset]
    cpu = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(5)
    randomize_qk_norms(cpu)
    gpu = copy.deepcopy(cpu).to(DEV)
    ids = [((i * 53) % 500) + 1 for i in range(40)]
    margins = []

    def caches(device):
        return KVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim, 16, 8,
                       torch.device(device), dtype=torch.bfloat16).caches
    want = _prefill_logits(cpu, caches("cpu"), ids, "cpu", margins)
    got = _prefill_logits(gpu, caches(DEV), ids, DEV)
    keep = torch.ones(len(ids), dtype=torch.bool)
    for m in margins:
        keep &= m >= ROUTE_MARGIN
    assert int(keep.sum()) >= len(ids) // 3, int(keep.sum())
    rel = (got - want).norm(dim=-1) / want.norm(dim=-1)
    print(f"{preset}: rows kept {int(keep.sum())}/{len(ids)}, worst kept "
          f"{float(rel[keep].max()):.4f}, worst of all {float(rel.max()):.4f}")
    assert torch.isfinite(got).all()
    assert float(rel[keep].max()) <= 0.03


# -- routed expert GEMMs at a small Qwen3-MoE's size ---------------------------

E128 = [mo.Case(128, 8, 256, 64, T, fam) for T in (1, 17, 130)
        for fam in mo.FAMILIES]


@pytest.mark.parametrize("case", E128, ids=lambda c: c.id)
def test_routed_gemm_e128_k8(case):
    """E = 128, k = 8: at T = 1, 120 of the 128 expert lists are empty."""
    b = mo.build(case)
    if case.T == 1:
        assert int((b.counts == 0).sum()) == 120
    w13, w2 = (t.to(DEV) for t in mo.weights(case.E, case.H, case.I))
    for fused in (True, False):
        out = ops.moe_forward(b.x.to(DEV), b.logits.to(DEV), w13, w2, case.k,
                              fused=fused)
        torch.cuda.synchronize()
        err = float(mo.wq_error(out.cpu(), b.want).max())
        print(f"{case.id}: fused={fused} {err:.5f}, tol {mo.TOL_MOE}")
        mo.assert_wq_close(out.cpu(), b.want, mo.TOL_MOE,
                           f"{case.id} fused={fused}")
