"""Q4_K/Q6_K weight-only GEMM on the GPU (ops/hip/gemm_kq.hip): exact
one-hot probes of every element position and sub-block, the oracle cases of
tests/kq_oracle.py (tests/test_kq_cpu.py shows on the same inputs that these
assertions can fail), segment-by-segment launches into one output, row
independence, the fallback boundary, the host guards and the engine.
"""
import pytest
import torch

import kq_oracle as ko
import helix_amd.ops as ops
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.quant import KQLinear

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 3          # NaN rows in front of and behind the output


def _dev(t):
    if t is None:
        return None
    if isinstance(t, (tuple, list)):
        return tuple(p.to(DEV) for p in t)
    return t.to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def _guarded_gemm(x, planes, fmt, bias):
    """Run the fused kernel into the middle of a NaN-filled buffer; returns
    (out, guard rows before, guard rows after)."""
    M, N = x.shape[0], planes[0].shape[0]
    buf = _nan(M + 2 * GUARD, N)
    out = buf[GUARD:GUARD + M]
    ops._native().gemm_kq(out, 0, x, list(planes), bias, fmt)
    return out, buf[:GUARD], buf[GUARD + M:]


def test_kernel_limits_and_k_splits():
    assert ops._C.KQ_KERNEL_MAX_M == ko.KQ_KERNEL_MAX_M
    assert ops.KQ_FUSED_MAX_M <= ops._C.KQ_KERNEL_MAX_M
    assert max(ko.MS) == ops._C.KQ_KERNEL_MAX_M
    # the oracle shapes take every K-split factor the kernel is built for
    assert {ops.kq_waves(n, k) for n, k in ko.NKS} == {4, 8, 16}


# -- one-hot exactness ----------------------------------------------------

@pytest.mark.parametrize("fmt", ko.FMTS)
@pytest.mark.parametrize("K", [256, 768, 2304, 4352])
def test_one_hot_exact(fmt, K):
    """Identity rows of x: out[k, n] is the bf16 rounding of element k of
    channel n, for every element position of every super-block (the four K
    take the 4-, 4-, 8- and 16-wave kernels)."""
    N = 32
    planes = ops.quantize_kq(ko.make_weight(fmt, N, K, "needle", salt=9), fmt)
    want = ops.dequantize_kq(planes, fmt, torch.bfloat16)       # [N, K]
    if fmt == "q4_k":       # every nibble value occurs
        assert len(torch.unique(torch.cat([planes[0] & 15,
                                           planes[0] >> 4]))) == 16
    eye = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    pd = _dev(planes)
    got = torch.cat([ops.gemm_kq(eye[k0:k0 + 16], pd, fmt)
                     for k0 in range(0, K, 16)])                 # [K, N]
    assert torch.equal(got.cpu(), want.t())


# -- oracle cases ---------------------------------------------------------

@pytest.mark.parametrize("case", ko.CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    assert case.M <= ops._C.KQ_KERNEL_MAX_M
    b = ko.build(case)
    x, planes, bias = _dev(b.x), _dev(b.planes), _dev(b.bias)
    out, before, after = _guarded_gemm(x, planes, case.fmt, bias)
    e = ko.assert_wq_close(out.cpu(), b.want, ko.TOL_KQ, case.id)
    print(f"{case.id}: error {e:.5f} (tol {ko.TOL_KQ})")
    assert torch.isnan(before).all() and torch.isnan(after).all(), \
        "the kernel wrote outside its [M, N] output"
    # the public op: the same kernel up to the cutoff, the library path above
    got = ops.gemm_kq(x, planes, case.fmt, bias)
    if case.M <= ops.KQ_FUSED_MAX_M:
        assert torch.equal(got, out)
    else:
        ko.assert_wq_close(got.cpu(), b.want, ko.TOL_KQ, case.id + " (op)")


# -- segments -------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 16, 17, 32])
@pytest.mark.parametrize("bias", [False, True])
def test_three_segments_one_output(M, bias):
    """16 q4_k | 16 q4_k | 32 q6_k at K = 768, launched segment by segment
    into a NaN-filled [M, 64]: each launch writes only its own columns, and
    the whole is the oracle of the concatenated weight."""
    x, segs, b, want = ko.build_mixed(M, bias)
    x, b = _dev(x), _dev(b)
    buf = _nan(M + 2 * GUARD, 64)
    out = buf[GUARD:GUARD + M]
    col, written = 0, torch.zeros(64, dtype=torch.bool)
    for fmt, planes in segs:
        n = planes[0].shape[0]
        ops._native().gemm_kq(out, col, x, list(_dev(planes)), b, fmt)
        written[col:col + n] = True
        cpu = out.cpu()
        assert torch.isfinite(cpu[:, written].float()).all()
        assert torch.isnan(cpu[:, ~written]).all(), \
            f"the {fmt} launch at column {col} wrote outside its columns"
        col += n
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + M:]).all()
    ko.assert_wq_close(out.cpu(), want, ko.TOL_KQ, f"mixed M={M}")
    # a segment alone computes the same bits as inside the shared output
    fmt, planes = segs[2]
    alone = torch.empty(M, 32, dtype=torch.bfloat16, device=DEV)
    ops._native().gemm_kq(alone, 0, x, list(_dev(planes)),
                          None if b is None else b[32:].contiguous(), fmt)
    assert torch.equal(alone, out[:, 32:])
    if M <= ops.KQ_FUSED_MAX_M:
        mod = KQLinear(segs, None if b is None else b.cpu()).to(DEV)
        assert torch.equal(mod(x), out)


@pytest.mark.parametrize("fmt", ko.FMTS)
def test_row_independence(fmt):
    """out[m, :] of the fused kernel does not depend on M or on the other
    rows, over the kernel's whole range (graph replay pads the batch to a
    bucket)."""
    def run(x, planes, bias):
        out = torch.empty(x.shape[0], planes[0].shape[0],
                          dtype=torch.bfloat16, device=DEV)
        ops._native().gemm_kq(out, 0, x, list(planes), bias, fmt)
        return out

    top = ops._C.KQ_KERNEL_MAX_M
    for N, K in ((512, 512), (256, 4352), (32, 2304)):
        b = ko.build(ko.Case(fmt, top, N, K, True, "randn"))
        x, planes, bias = _dev(b.x), _dev(b.planes), _dev(b.bias)
        full = run(x, planes, bias)
        for m in (0, 15, 16, 23, top - 1):
            one = run(x[m:m + 1].contiguous(), planes, bias)
            assert torch.equal(one[0], full[m]), (N, K, m)
        for M in (2, 16, 17):
            part = run(x[:M].contiguous(), planes, bias)
            assert torch.equal(part, full[:M]), (N, K, M)


# -- fallback boundary ----------------------------------------------------

@pytest.mark.parametrize("fmt", ko.FMTS)
def test_dequant_exact(fmt):
    for N, K in ((48, 768), (256, 4352)):
        b = ko.build(ko.Case(fmt, 1, N, K, False, "needle"))
        want = ops.dequantize_kq(b.planes, fmt, torch.bfloat16)
        buf = _nan(N * K + 64)
        got = ops.dequant_kq(_dev(b.planes), fmt, out=buf)
        assert got.data_ptr() == buf.data_ptr()
        assert torch.equal(got.cpu(), want)
        assert torch.isnan(buf[N * K:]).all()
        assert torch.equal(ops.dequant_kq(_dev(b.planes), fmt).cpu(), want)


@pytest.mark.parametrize("M", ko.FALLBACK_MS)
@pytest.mark.parametrize("bias", [False, True])
def test_fallback_mixed_module(M, bias):
    """Above the cutoff a mixed KQLinear dequantizes every segment into its
    row range of the scratch and runs one library GEMM."""
    assert M > ops.KQ_FUSED_MAX_M
    x, segs, b, want = ko.build_mixed(M, bias)
    mod = KQLinear(segs, b).to(DEV)
    scratch = _nan(64 * ko.MIXED_K + 32)
    mod.scratch = scratch
    out = mod(_dev(x))
    e = ko.assert_wq_close(out.cpu(), want, ko.TOL_KQ, f"fallback M={M}")
    print(f"mixed fallback M={M}: error {e:.5f} (tol {ko.TOL_KQ})")
    w = torch.cat([ops.dequantize_kq(p, f, torch.bfloat16) for f, p in segs])
    assert torch.equal(scratch[:64 * ko.MIXED_K].view(64, -1).cpu(), w)
    assert torch.isnan(scratch[64 * ko.MIXED_K:]).all()
    # the op alone, one segment
    fmt, planes = segs[2]
    got = ops.gemm_kq(_dev(x), _dev(planes), fmt,
                      None if b is None else _dev(b[32:].contiguous()))
    ko.assert_wq_close(got.cpu(), want[:, 32:], ko.TOL_KQ, "fallback op")


# -- host guards ----------------------------------------------------------

def test_host_guards():
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    x = z(4, 512, dt=torch.bfloat16)
    q4 = (z(32, 256), z(32, 2, 16))
    q6 = (z(32, 256), z(32, 128), z(32, 32, dt=torch.int8),
          z(32, 2, dt=torch.float16))
    assert not ops.gemm_kq(x, q4, "q4_k").any()            # the good calls
    assert not ops.gemm_kq(x, q6, "q6_k").any()
    off = z(32 * 256 + 1)[1:].view(32, 256)                # 1 byte off
    bad = [
        ("K % 256", "q4_k", (z(32, 192), z(32, 1, 16))),
        ("N % 16", "q4_k", (z(24, 256), z(24, 2, 16))),
        ("qs strided", "q4_k", (z(32, 512)[:, ::2], q4[1])),
        ("qs dtype", "q4_k", (q4[0].view(torch.int8), q4[1])),
        ("qs unaligned", "q4_k", (off, q4[1])),
        ("hdr shape", "q4_k", (q4[0], z(32, 2, 12))),
        ("hdr dtype", "q4_k", (q4[0], z(32, 2, 16, dt=torch.int8))),
        ("hdr on the CPU", "q4_k", (q4[0], q4[1].cpu())),
        ("plane count", "q4_k", q4 + (q4[1],)),
        ("plane count", "q6_k", q6[:3]),
        ("ql unaligned", "q6_k", (off,) + q6[1:]),
        ("qh shape", "q6_k", (q6[0], z(32, 64), q6[2], q6[3])),
        ("qh strided", "q6_k", (q6[0], z(32, 256)[:, ::2], q6[2], q6[3])),
        ("sc dtype", "q6_k", (q6[0], q6[1], q6[2].view(torch.uint8), q6[3])),
        ("sc shape", "q6_k", (q6[0], q6[1], z(32, 16, dt=torch.int8), q6[3])),
        ("d dtype", "q6_k", q6[:3] + (q6[3].float(),)),
        ("d shape", "q6_k", q6[:3] + (z(32, 1, dt=torch.float16),)),
    ]
    for what, fmt, planes in bad:
        xk = z(4, planes[0].shape[1] * 2, dt=torch.bfloat16)
        with pytest.raises(RuntimeError):
            ops.gemm_kq(xk, planes, fmt)
            pytest.fail(f"{what}: accepted by gemm_kq")
        with pytest.raises(RuntimeError):
            ops.dequant_kq(planes, fmt)
            pytest.fail(f"{what}: accepted by dequant_kq")
    C = ops._native()
    out = z(4, 64, dt=torch.bfloat16)
    C.gemm_kq(out, 32, x, list(q4), None, "q4_k")          # the good call
    calls = [
        ("col_off % 4", out, 2, x, None),
        ("col_off < 0", out, -4, x, None),
        ("ldo < col_off + N", out, 36, x, None),
        ("ldo % 4", z(4, 66, dt=torch.bfloat16), 32, x, None),
        ("out rows", z(5, 64, dt=torch.bfloat16), 32, x, None),
        ("out dtype", out.float(), 32, x, None),
        ("out strided", z(4, 128, dt=torch.bfloat16)[:, ::2], 32, x, None),
        ("x K", out, 32, x[:, :256].contiguous(), None),
        ("x dtype", out, 32, x.float(), None),
        ("bias short", out, 32, x, z(32, dt=torch.bfloat16)),
        ("bias dtype", out, 32, x, z(64, dt=torch.float32)),
    ]
    for what, o, col, xx, bias in calls:
        with pytest.raises(RuntimeError):
            C.gemm_kq(o, col, xx, list(q4), bias, "q4_k")
            pytest.fail(f"{what}: accepted")
    top = ops._C.KQ_KERNEL_MAX_M
    with pytest.raises(RuntimeError):                      # M past the kernel
        C.gemm_kq(z(top + 1, 32, dt=torch.bfloat16), 0,
                  z(top + 1, 512, dt=torch.bfloat16), list(q4), None, "q4_k")
    with pytest.raises(RuntimeError):                      # unknown format
        C.gemm_kq(out, 0, x, list(q4), None, "q5_k")
    with pytest.raises(RuntimeError):
        C.dequant_kq(z(32, 512, dt=torch.bfloat16), list(q4), "q4_0")
    with pytest.raises(ValueError):
        ops.gemm_kq(x, q4, "q5_k")
    with pytest.raises(ValueError):
        ops.dequant_kq(q4, "q5_k")
    assert not out.any()


# -- engine ---------------------------------------------------------------

BASE = dict(model="tiny-gqa", max_model_len=512, max_num_seqs=8,
            kv_cache_blocks=256, eos_token_id=-1, seed=7)
SP = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
PROMPTS = [[1, 2, 3, 4, 5], [7, 8]]


def _dequantized_reference(cfg_kwargs, fmt):
    """An eager bf16 engine carrying the dequantized weights."""
    ref = LLMEngine(EngineConfig(**cfg_kwargs, enforce_eager=True),
                    device=DEV)
    for layer in ref.model.layers:
        for lin in (layer.attn.qkv_proj, layer.attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            lin.weight.data.copy_(ops.dequantize_kq(
                ops.quantize_kq(lin.weight.data, fmt), fmt))
    return ref


def test_q4_k_engine_gpu():
    """Mirror of test_q4_engine_gpu: eager == graph, and both agree with an
    eager bf16 engine carrying the dequantized weights on at least 6 of the
    first 12 tokens (seed 7; the CPU run of the same pair,
    tests/test_kq_cpu.py, is exact)."""
    eager = LLMEngine(EngineConfig(**BASE, enforce_eager=True,
                                   quantization="q4_k"), device=DEV)
    got_eager = eager.generate(PROMPTS, SP)
    want = _dequantized_reference(BASE, "q4_k").generate(PROMPTS, SP)
    graph = LLMEngine(EngineConfig(**BASE, quantization="q4_k"), device=DEV)
    assert graph.graph_runner is not None
    assert isinstance(graph.model.layers[0].mlp.down_proj, KQLinear)
    got_graph = graph.generate(PROMPTS, SP)
    assert got_eager == got_graph                        # capture-safe
    for g, w in zip(got_graph, want):
        assert len(g) == 12
        agree = sum(a == b for a, b in zip(g, w))
        assert agree >= 6, f"q4_k diverged early: {g} vs {w}"


WIDE = dict(BASE, max_num_seqs=32)
WIDE_PROMPTS = [[(7 * i + j) % 900 + 1 for j in range(5)] for i in range(32)]


def test_q4_k_engine_fallback_path_gpu():
    """32 busy sequences: the 160-token prefill and every decode step (M =
    32, bucket 32) take dequant_kq + library GEMM into the model's scratch
    when the cutoff is below 32, eagerly and under graph capture. Eager and
    graph see the same M and must agree exactly; against the bf16 engine
    carrying the dequantized weights the bar is 6 of the first 12 tokens
    per sequence."""
    eager = LLMEngine(EngineConfig(**WIDE, enforce_eager=True,
                                   quantization="q4_k"), device=DEV)
    mods = [m for m in eager.model.modules() if isinstance(m, KQLinear)]
    assert mods and mods[0].scratch is not None
    assert all(m.scratch is mods[0].scratch for m in mods)
    assert mods[0].scratch.numel() == max(
        m.in_features * m.out_features for m in mods)
    got_eager = eager.generate(WIDE_PROMPTS, SP)
    graph = LLMEngine(EngineConfig(**WIDE, quantization="q4_k"), device=DEV)
    assert graph.graph_runner is not None
    got_graph = graph.generate(WIDE_PROMPTS, SP)
    assert got_eager == got_graph
    want = _dequantized_reference(WIDE, "q4_k").generate(WIDE_PROMPTS, SP)
    print("sequences identical to the bf16 reference:",
          sum(g == w for g, w in zip(got_eager, want)), "of", len(want))
    for g, w in zip(got_eager, want):
        assert len(g) == 12
        assert sum(a == b for a, b in zip(g, w)) >= 6, (g, w)
