"""LDS-tiled split-K Q4_0/Q8_0 GEMM (ops/hip/gemm_wq_tiled.hip) against the
fp64 oracle of tests/wq_oracle.py, plus one-hot exactness, row
independence, the three-way dispatch of ops.gemm_wq, the host guards and
the engine.
"""
import pytest
import torch

import wq_oracle as wo
import helix_amd.ops as ops
from helix_amd.engine.graph_runner import BATCH_BUCKETS

DEV = "cuda:0"
GUARD = 3          # NaN rows in front of and behind the output
# 4 x the worst error of wo.emulate (weight to bf16, fp32 accumulate, bf16
# out) against the fp64 oracle over exactly the cases below, measured on the
# CPU: 0.00726, the same when the fp32 partials are summed split by split.
# The smallest mutant of wo.mutant_outputs on these inputs is offset_7 at
# 0.38 = 13 x tol, then drop_last_k_block at 0.72.
TOL_WQ_TILED = 0.0290
# (N, K) per value of wq_tiled_splits: the smallest step count that selects
# it plus one step that is a single 32-element block (uneven last split, K
# no multiple of 128); (48, 160) has a partial 64-channel group.
NKS = ((48, 160), (64, 128), (192, 512), (64, 2080), (128, 4128), (64, 8224))
MS = (17, 33, 128, 129, 260)    # tile edges of MT = 2 / 4 / 8, three M tiles
CASES = [wo.Case(f, m, n, k, b, fam) for f in wo.FMTS for (n, k) in NKS
         for m in MS for b in (False, True) for fam in wo.FAMILIES]


def _dev(t):
    return None if t is None else t.to(DEV)


def _tiled(x, qs, d, fmt, bias, slack=64):
    """The kernel into the middle of a NaN-guarded output, with a NaN-filled
    workspace `slack` elements longer than needed; returns (buf, ws, used)."""
    M, N = x.shape[0], qs.shape[0]
    KS = ops.wq_tiled_splits(N, x.shape[1])
    used = KS * M * N if KS > 1 else 0
    ws = torch.full((used + slack,), float("nan"), device=DEV)
    buf = torch.full((M + 2 * GUARD, N), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    ops._C.gemm_wq_tiled(buf[GUARD:GUARD + M], x, qs, d, bias,
                         ops.wq_bits(fmt), ws)
    return buf, ws, used


def _run(b, fmt, rows=slice(None)):
    x = _dev(b.x[rows].contiguous())
    buf, _, _ = _tiled(x, _dev(b.qs), _dev(b.d), fmt, _dev(b.bias))
    return buf[GUARD:-GUARD]


@pytest.mark.gpu
def test_every_split_factor_is_hit():
    assert {ops.wq_tiled_splits(n, k) for n, k in NKS} == {1, 2, 4, 8}
    assert [ops.wq_tiled_splits(n, k) for n, k in NKS] == [1, 1, 1, 2, 4, 8]
    for n, k in ((4096, 4096), (6144, 4096), (4096, 14336)):
        assert ops.wq_tiled_splits(n, k) == 4
    assert ops.wq_tiled_splits(28672, 4096) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    b = wo.build(case)
    buf, ws, used = _tiled(_dev(b.x), _dev(b.qs), _dev(b.d), case.fmt,
                           _dev(b.bias))
    e = wo.assert_wq_close(buf[GUARD:-GUARD].cpu(), b.want, TOL_WQ_TILED,
                           case.id)
    print(f"{case.id}: error {e:.5f} (tol {TOL_WQ_TILED})")
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), \
        "the kernel wrote outside its [M, N] output"
    assert torch.isnan(ws[used:]).all(), "the kernel wrote past KS*M*N of ws"
    assert not torch.isnan(ws[:used]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", wo.FMTS)
@pytest.mark.parametrize("K", [160, 2080])
def test_one_hot_exact(fmt, K):
    b = wo.build(wo.Case(fmt, 1, 48, K, False, "needle"))
    want = ops.dequantize_wq(b.qs, b.d, fmt, torch.bfloat16)       # [N, K]
    eye = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    buf, _, _ = _tiled(eye, _dev(b.qs), _dev(b.d), fmt, None)
    assert torch.equal(buf[GUARD:-GUARD].cpu(), want.t())


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", wo.FMTS)
@pytest.mark.parametrize("N,K", [(192, 512), (128, 4128), (64, 8224)])
def test_row_independence(fmt, N, K):
    """out[m, :] does not depend on M or on the other rows (graph replay
    pads the batch to a bucket), and the kernel is deterministic."""
    b = wo.build(wo.Case(fmt, 260, N, K, True, "randn"))
    full = _run(b, fmt)
    assert torch.equal(_run(b, fmt), full)
    for m in (0, 16, 127, 128, 259):
        assert torch.equal(_run(b, fmt, slice(m, m + 1))[0], full[m]), m
    for M in (17, 129):
        assert torch.equal(_run(b, fmt, slice(0, M)), full[:M]), M


def test_cutoff_is_a_bucket():
    assert ops.WQ_TILED_MAX_M in BATCH_BUCKETS
    assert ops.WQ_TILED_MAX_M > ops.WQ_FUSED_MAX_M


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", wo.FMTS)
def test_dispatch(fmt, monkeypatch):
    N, K = 128, 4128                                   # KS = 4
    top = ops.WQ_TILED_MAX_M
    b = wo.build(wo.Case(fmt, top + 1, N, K, True, "randn"))
    x, qs, d, bias = _dev(b.x), _dev(b.qs), _dev(b.d), _dev(b.bias)
    full = _run(b, fmt)
    model_scratch = torch.empty(N * K, dtype=torch.bfloat16, device=DEV)
    for M in (17, top):
        for scratch in (None, model_scratch):
            got = ops.gemm_wq(x[:M].contiguous(), qs, d, fmt, bias, scratch)
            assert torch.equal(got, full[:M]), (M, scratch is None)
    got = ops.gemm_wq(x, qs, d, fmt, bias, model_scratch)
    wo.assert_wq_close(got.cpu(), b.want, TOL_WQ_TILED, "above the cutoff")
    # the partial sums of M rows do not fit a scratch of N*K bf16 once
    # 2*KS*M > K: the dequant path, which leaves the bf16 weight there
    monkeypatch.setattr(ops, "WQ_TILED_MAX_M", 1024)
    N, K, M = 64, 2080, 521                            # KS = 2
    b = wo.build(wo.Case(fmt, M, N, K, True, "randn"))
    small = torch.zeros(N * K, dtype=torch.bfloat16, device=DEV)
    got = ops.gemm_wq(_dev(b.x), _dev(b.qs), _dev(b.d), fmt, _dev(b.bias),
                      small)
    wo.assert_wq_close(got.cpu(), b.want, TOL_WQ_TILED, "scratch too small")
    assert torch.equal(small.view(N, K).cpu(),
                       ops.dequantize_wq(b.qs, b.d, fmt, torch.bfloat16))


@pytest.mark.gpu
def test_host_guards():
    N, K, M = 64, 2080, 17                             # KS = 2
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    qs = torch.zeros(N, K // 2, dtype=torch.uint8, device=DEV)
    d = torch.zeros(N, K // 32, dtype=torch.float16, device=DEV)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ws = torch.zeros(2 * M * N + 4, device=DEV)
    ops._C.gemm_wq_tiled(out, x, qs, d, None, 4, ws)   # the good call
    assert not out.any()
    bad = {
        "ws missing": (out, x, qs, d, None, 4, None),
        "ws too small": (out, x, qs, d, None, 4, ws[:2 * M * N - 1]),
        "ws dtype": (out, x, qs, d, None, 4, ws.double()),
        "ws device": (out, x, qs, d, None, 4, ws.cpu()),
        "ws misaligned": (out, x, qs, d, None, 4, ws[1:]),
        "x K": (out, x[:, :2048].contiguous(), qs, d, None, 4, ws),
        "out shape": (out[:, :48].contiguous(), x, qs, d, None, 4, ws),
        "bits": (out, x, qs, d, None, 5, ws),
        "M = 0": (out[:0], x[:0], qs, d, None, 4, ws),
    }
    out.fill_(float("nan"))
    for what, args in bad.items():
        with pytest.raises(RuntimeError):
            ops._C.gemm_wq_tiled(*args)
            pytest.fail(f"{what}: accepted")
    assert torch.isnan(out).all(), "a refused call launched"


@pytest.mark.gpu
def test_q8_engine_tiled_path_gpu():
    """32 busy sequences: the 160-token prefill and every decode step (M =
    32, bucket 32) are above WQ_FUSED_MAX_M. Eager and graph see the same M
    and must agree exactly; against the bf16 engine carrying the dequantized
    weights the bar is the engine tests' 6 of the first 12 tokens."""
    from helix_amd.engine.engine import EngineConfig, LLMEngine
    from helix_amd.engine.sampling_params import SamplingParams
    cfg = dict(model="tiny-gqa", max_model_len=512, max_num_seqs=32,
               kv_cache_blocks=256, eos_token_id=-1, seed=7)
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    prompts = [[(7 * i + j) % 900 + 1 for j in range(5)] for i in range(32)]
    assert 32 <= ops.WQ_TILED_MAX_M
    got_eager = LLMEngine(EngineConfig(**cfg, enforce_eager=True,
                                       quantization="q8_0"),
                          device=DEV).generate(prompts, sp)
    graph = LLMEngine(EngineConfig(**cfg, quantization="q8_0"), device=DEV)
    assert graph.graph_runner is not None
    assert graph.generate(prompts, sp) == got_eager
    ref = LLMEngine(EngineConfig(**cfg, enforce_eager=True), device=DEV)
    for layer in ref.model.layers:
        for lin in (layer.attn.qkv_proj, layer.attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            lin.weight.data.copy_(ops.dequantize_wq(
                *ops.quantize_wq(lin.weight.data, "q8_0"), "q8_0"))
    for g, w in zip(got_eager, ref.generate(prompts, sp)):
        assert len(g) == 12
        assert sum(a == b for a, b in zip(g, w)) >= 6, (g, w)
