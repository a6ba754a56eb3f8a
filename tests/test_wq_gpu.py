"""Q4_0/Q8_0 weight-only GEMM on the GPU (ops/hip/gemm_wq.hip): exact
one-hot probes of every nibble position and block index, the oracle cases
of tests/wq_oracle.py (tests/test_wq_cpu.py shows on the same inputs that
these assertions can fail), row independence, the fallback boundary, the
host guards and the engine.
"""
import pytest
import torch

import wq_oracle as wo
import helix_amd.ops as ops
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 3          # NaN rows in front of and behind the output


def _dev(t):
    return None if t is None else t.to(DEV)


def _guarded_gemm(x, qs, d, fmt, bias):
    """Run the fused kernel into the middle of a NaN-filled buffer; returns
    (out, guard rows before, guard rows after)."""
    M, N = x.shape[0], qs.shape[0]
    buf = torch.full((M + 2 * GUARD, N), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    out = buf[GUARD:GUARD + M]
    ops._native().gemm_wq(out, x, qs, d, bias, ops.wq_bits(fmt))
    return out, buf[:GUARD], buf[GUARD + M:]


# -- one-hot exactness ----------------------------------------------------

@pytest.mark.parametrize("fmt", wo.FMTS)
@pytest.mark.parametrize("K", [32, 160])
def test_one_hot_exact(fmt, K):
    N, nblk = 32, K // 32
    g = torch.Generator().manual_seed(K)
    n = torch.arange(N)[:, None]
    b = torch.arange(nblk)[None, :]
    # distinct scale per (row, block): a wrong one is off by at least 2x
    scale = (2.0 ** ((n + 3 * b) % 7).float()) * 0.01
    w = torch.randn(N, nblk, 32, generator=g) * scale[..., None]
    qs, d = ops.quantize_wq(w.reshape(N, K), fmt)
    want = ops.dequantize_wq(qs, d, fmt, torch.bfloat16)       # [N, K]
    if fmt == "q4_0":       # every nibble value occurs
        assert len(torch.unique(torch.cat([qs & 15, qs >> 4]))) == 16
    eye = torch.eye(K, dtype=torch.bfloat16)
    qs_d, d_d = qs.to(DEV), d.to(DEV)
    for k0 in range(0, K, 16):
        out = ops.gemm_wq(eye[k0:k0 + 16].to(DEV), qs_d, d_d, fmt)
        assert torch.equal(out.cpu(), want[:, k0:k0 + 16].t()), (fmt, K, k0)


# -- oracle cases ---------------------------------------------------------

@pytest.mark.parametrize("case", wo.CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    assert case.M <= ops._C.WQ_KERNEL_MAX_M
    b = wo.build(case)
    out, before, after = _guarded_gemm(_dev(b.x), _dev(b.qs), _dev(b.d),
                                       case.fmt, _dev(b.bias))
    e = wo.assert_wq_close(out.cpu(), b.want, wo.TOL_WQ, case.id)
    print(f"{case.id}: error {e:.5f} (tol {wo.TOL_WQ})")
    assert torch.isnan(before).all() and torch.isnan(after).all(), \
        "the kernel wrote outside its [M, N] output"
    # the public op: the same kernel up to the cutoff, the library path above
    got = ops.gemm_wq(_dev(b.x), _dev(b.qs), _dev(b.d), case.fmt,
                      _dev(b.bias))
    if case.M <= ops.WQ_FUSED_MAX_M:
        assert torch.equal(got, out)
    else:
        wo.assert_wq_close(got.cpu(), b.want, wo.TOL_WQ, case.id + " (op)")


@pytest.mark.parametrize("fmt", wo.FMTS)
def test_row_independence(fmt):
    """out[m, :] of the fused kernel does not depend on M or on the other
    rows, over the kernel's whole range (graph replay pads the batch to a
    bucket)."""
    def run(x, qs, d, bias):
        out = torch.empty(x.shape[0], qs.shape[0], dtype=torch.bfloat16,
                          device=DEV)
        ops._native().gemm_wq(out, x, qs, d, bias, ops.wq_bits(fmt))
        return out

    for N, K in ((512, 256), (256, 4128), (32, 2080)):
        b = wo.build(wo.Case(fmt, 64, N, K, True, "randn"))
        x, qs, d, bias = _dev(b.x), _dev(b.qs), _dev(b.d), _dev(b.bias)
        full = run(x, qs, d, bias)
        for m in (0, 15, 16, 37, 63):
            one = run(x[m:m + 1].contiguous(), qs, d, bias)
            assert torch.equal(one[0], full[m]), (N, K, m)
        for M in (17, 33):
            part = run(x[:M].contiguous(), qs, d, bias)
            assert torch.equal(part, full[:M]), (N, K, M)


# -- fallback boundary ----------------------------------------------------

@pytest.mark.parametrize("fmt", wo.FMTS)
def test_dequant_exact(fmt):
    for N, K in ((48, 160), (256, 4128)):
        b = wo.build(wo.Case(fmt, 1, N, K, False, "needle"))
        want = ops.dequantize_wq(b.qs, b.d, fmt, torch.bfloat16)
        buf = torch.full((N * K + 64,), float("nan"), dtype=torch.bfloat16,
                         device=DEV)
        got = ops.dequant_wq(_dev(b.qs), _dev(b.d), fmt, out=buf)
        assert got.data_ptr() == buf.data_ptr()
        assert torch.equal(got.cpu(), want)
        assert torch.isnan(buf[N * K:]).all()
        assert torch.equal(ops.dequant_wq(_dev(b.qs), _dev(b.d), fmt).cpu(),
                           want)


@pytest.mark.parametrize("case", wo.FALLBACK_CASES, ids=lambda c: c.id)
def test_fallback_case(case):
    assert case.M > ops.WQ_FUSED_MAX_M
    b = wo.build(case)
    scratch = torch.empty(case.N * case.K, dtype=torch.bfloat16, device=DEV)
    out = ops.gemm_wq(_dev(b.x), _dev(b.qs), _dev(b.d), case.fmt,
                      _dev(b.bias), scratch=scratch)
    e = wo.assert_wq_close(out.cpu(), b.want, wo.TOL_WQ, case.id)
    print(f"{case.id}: error {e:.5f} (tol {wo.TOL_WQ})")


# -- host guards ----------------------------------------------------------

def test_host_guards():
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    qs = torch.zeros(32, 32, dtype=torch.uint8, device=DEV)
    d = torch.zeros(32, 2, dtype=torch.float16, device=DEV)
    assert not ops.gemm_wq(x, qs, d, "q4_0").any()         # the good call
    bad = [
        ("K % 32", x[:, :48].contiguous(), qs[:, :24].contiguous(), d),
        ("N % 16", x, qs[:24].contiguous(), d[:24].contiguous()),
        ("qs strided", x, torch.zeros(32, 64, dtype=torch.uint8,
                                      device=DEV)[:, ::2], d),
        ("d shape", x, qs, torch.zeros(32, 3, dtype=torch.float16,
                                       device=DEV)),
        ("d dtype", x, qs, d.float()),
        ("qs dtype", x, qs.view(torch.int8), d),
        ("x K", x[:, :32].contiguous(), qs, d),
        ("x dtype", x.float(), qs, d),
    ]
    for what, bx, bqs, bd in bad:
        with pytest.raises(RuntimeError):
            ops.gemm_wq(bx, bqs, bd, "q4_0")
            pytest.fail(f"{what}: accepted")
        if not what.startswith("x "):              # the planes are at fault
            with pytest.raises(RuntimeError):
                ops.dequant_wq(bqs, bd, "q4_0")
    out = torch.zeros(65, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):                      # M past the kernel
        ops._native().gemm_wq(out, torch.zeros(65, 64, dtype=torch.bfloat16,
                                               device=DEV), qs, d, None, 4)
    with pytest.raises(ValueError):
        ops.gemm_wq(x, qs, d, "q5_0")


# -- engine ---------------------------------------------------------------

BASE = dict(model="tiny-gqa", max_model_len=512, max_num_seqs=8,
            kv_cache_blocks=256, eos_token_id=-1, seed=7)
SP = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
PROMPTS = [[1, 2, 3, 4, 5], [7, 8]]


@pytest.fixture(scope="module")
def q4_eager_tokens():
    return LLMEngine(EngineConfig(**BASE, enforce_eager=True,
                                  quantization="q4_0"),
                     device=DEV).generate(PROMPTS, SP)


def test_q4_engine_gpu(q4_eager_tokens):
    """Mirror of test_fp8_quantized_engine_gpu: eager == graph, and both
    agree with an eager bf16 engine carrying the dequantized weights on at
    least 6 of the first 12 tokens (seed 7; the CPU run of the same pair,
    tests/test_wq_cpu.py, is exact)."""
    from helix_amd.models.quant import WQLinear
    ref = LLMEngine(EngineConfig(**BASE, enforce_eager=True), device=DEV)
    for layer in ref.model.layers:
        for lin in (layer.attn.qkv_proj, layer.attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            lin.weight.data.copy_(ops.dequantize_wq(
                *ops.quantize_wq(lin.weight.data, "q4_0"), "q4_0"))
    want = ref.generate(PROMPTS, SP)
    graph = LLMEngine(EngineConfig(**BASE, quantization="q4_0"), device=DEV)
    assert graph.graph_runner is not None
    assert isinstance(graph.model.layers[0].mlp.down_proj, WQLinear)
    got_graph = graph.generate(PROMPTS, SP)
    assert q4_eager_tokens == got_graph                  # capture-safe
    for g, w in zip(got_graph, want):
        assert len(g) == 12
        agree = sum(a == b for a, b in zip(g, w))
        assert agree >= 6, f"q4_0 diverged early: {g} vs {w}"


def test_q4_engine_zero_lora_equals_base(tmp_path, q4_eager_tokens):
    import helix_amd.models.lora as L
    from helix_amd.models.llama import PRESETS
    t = L.random_adapter_tensors(PRESETS["tiny-gqa"], 16, seed=3, b_std=0.05,
                                 zero_b=True)
    path = L.save_peft_adapter(str(tmp_path / "zero"), t, r=16, lora_alpha=64)
    eng = LLMEngine(EngineConfig(**BASE, enforce_eager=True,
                                 quantization="q4_0", max_loras=2,
                                 max_lora_rank=16), device=DEV)
    eng.add_lora("zero", path)
    assert eng.generate(PROMPTS, SP, loras=["zero"] * 2) == q4_eager_tokens


# -- the large-M path inside an engine --------------------------------------

WIDE = dict(BASE, max_num_seqs=32)
WIDE_PROMPTS = [[(7 * i + j) % 900 + 1 for j in range(5)] for i in range(32)]


def test_q4_engine_fallback_path_gpu():
    """32 busy sequences: the 160-token prefill and every decode step (M =
    32, bucket 32) are above WQ_FUSED_MAX_M, so every projection takes
    dequant_wq + library GEMM into the model's scratch, eagerly and under
    graph capture. Eager and graph see the same M and must agree exactly;
    against the bf16 engine carrying the dequantized weights the bar is the
    engine tests' 6 of the first 12 tokens per sequence."""
    assert ops.WQ_FUSED_MAX_M < 32
    eager = LLMEngine(EngineConfig(**WIDE, enforce_eager=True,
                                   quantization="q4_0"), device=DEV)
    assert eager.model.layers[0].mlp.down_proj.scratch is not None
    got_eager = eager.generate(WIDE_PROMPTS, SP)
    graph = LLMEngine(EngineConfig(**WIDE, quantization="q4_0"), device=DEV)
    assert graph.graph_runner is not None
    got_graph = graph.generate(WIDE_PROMPTS, SP)
    assert got_eager == got_graph
    ref = LLMEngine(EngineConfig(**WIDE, enforce_eager=True), device=DEV)
    for layer in ref.model.layers:
        for lin in (layer.attn.qkv_proj, layer.attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            lin.weight.data.copy_(ops.dequantize_wq(
                *ops.quantize_wq(lin.weight.data, "q4_0"), "q4_0"))
    want = ref.generate(WIDE_PROMPTS, SP)
    print("sequences identical to the bf16 reference:",
          sum(g == w for g, w in zip(got_eager, want)), "of", len(want))
    for g, w in zip(got_eager, want):
        assert len(g) == 12
        assert sum(a == b for a, b in zip(g, w)) >= 6, (g, w)


def test_scratch_is_owned_by_the_model():
    """The large-M path is two launches (dequantize, GEMM); two models on
    one GPU run on two threads, so they must not share the buffer between
    those launches. Layers of one model run in sequence and do share it."""
    from helix_amd.models.llama import LlamaForCausalLM, PRESETS
    from helix_amd.models.quant import (WQLinear, attach_wq_scratch,
                                        quantize_model_wq)

    def wq_modules(m):
        return [x for x in m.modules() if isinstance(x, WQLinear)]

    models = []
    for seed in (0, 1):
        m = LlamaForCausalLM(PRESETS["tiny-gqa"]).to(torch.bfloat16).to(DEV)
        m.init_random(seed)
        quantize_model_wq(m, "q4_0")
        models.append(m)
    bufs = []
    for m in models:
        mods = wq_modules(m)
        assert mods and all(x.scratch is mods[0].scratch for x in mods)
        assert mods[0].scratch.device == mods[0].qs.device
        assert mods[0].scratch.numel() == max(
            x.in_features * x.out_features for x in mods)
        bufs.append(mods[0].scratch)
    assert bufs[0].untyped_storage().data_ptr() != \
        bufs[1].untyped_storage().data_ptr()
    # a model quantized on the CPU and moved afterwards gets its buffer when
    # an engine takes it, and keeps it (captured graphs point into it)
    m = LlamaForCausalLM(PRESETS["tiny-gqa"]).to(torch.bfloat16)
    m.init_random(2)
    quantize_model_wq(m, "q8_0")
    assert all(x.scratch is None for x in wq_modules(m))
    m.to(DEV)
    eng = LLMEngine(EngineConfig(**BASE, enforce_eager=True), device=DEV,
                    model=m)
    mine = wq_modules(eng.model)[0].scratch
    assert mine is not None and mine.is_cuda
    assert all(x.d.dtype == torch.float16 for x in wq_modules(eng.model))
    attach_wq_scratch(eng.model)
    assert wq_modules(eng.model)[0].scratch is mine
    assert mine.untyped_storage().data_ptr() not in (
        bufs[0].untyped_storage().data_ptr(),
        bufs[1].untyped_storage().data_ptr())
    assert len(eng.generate(PROMPTS, SP)[0]) == 12
