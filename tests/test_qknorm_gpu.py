"""QK-norm + rope HIP kernel (ops/hip/rope_qkv_norm.hip) on the GPU: every
oracle case with and without compact K/V and a paged cache, a sentinel cache
with pad rows, a strided qkv, the e4m3 cache, host-check refusals and
hipGraph replay."""
import functools

import pytest
import torch

import helix_amd.ops as ops
import qknorm_oracle as qo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A         # bytes that no output test relies on


@functools.lru_cache(maxsize=None)
def _cs(D):
    return qo.cos_sin(D).to(DEV)


def _cache(case, b, dtype):
    """A sentinel-filled (k_cache, v_cache) pair."""
    shape = (b.nblocks, case.Hkv, qo.BLOCK, case.D)
    n = shape[0] * shape[1] * shape[2] * shape[3] * \
        (1 if dtype == torch.uint8 else 2)
    assert n % 8 == 0

    def one():
        raw = torch.full((n // 8,), SENTINEL, dtype=torch.int64, device=DEV)
        return raw.view(dtype).view(shape)
    return one(), one()


def _run(case, b, qkv=None, cache_dtype=None, want_kv=False):
    kv = _cache(case, b, cache_dtype) if cache_dtype is not None else None
    q, k, v = ops.rope_qkv_cache(
        b.positions.to(DEV), b.qkv.to(DEV) if qkv is None else qkv,
        _cs(case.D), case.Hq, case.Hkv, case.D, kv_cache=kv,
        slot_mapping=b.slots.to(DEV) if kv is not None else None,
        want_kv=want_kv, q_norm_w=b.wq.to(DEV), k_norm_w=b.wk.to(DEV),
        eps=qo.EPS)
    torch.cuda.synchronize()
    return q, k, v, kv


def _v_in(case, b):
    return b.qkv[:, (case.Hq + case.Hkv) * case.D:].view(
        case.T, case.Hkv, case.D)


def _check_cache(case, b, kv, k_bits=None):
    """Written slots hold the oracle's K (bitwise k_bits when given) and the
    input's V; every other byte is the sentinel."""
    kc, vc = (t.cpu() for t in kv)
    fp8 = kc.dtype == torch.uint8
    rows, blk, off = qo.written_rows(b)
    gk, gv = kc[blk, :, off], vc[blk, :, off]          # [n, Hkv, D]
    want = b.want_k.view(case.T, case.Hkv, case.D)[rows].reshape(-1, case.D)
    vin = _v_in(case, b)[rows]
    if fp8:
        qo.assert_wq_close(ops.kv_fp8_dequant(gk, torch.float32)
                           .reshape(-1, case.D), want, qo.TOL_QKNORM_FP8,
                           case.id + " fp8 k cache")
        assert torch.equal(gv, ops.kv_fp8_quant(vin))
    else:
        qo.assert_wq_close(gk.reshape(-1, case.D), want, qo.TOL_QKNORM,
                           case.id + " k cache")
        assert torch.equal(gv, vin)
        if k_bits is not None:
            assert torch.equal(gk, k_bits.cpu()[rows])
    mask = torch.ones(b.nblocks, qo.BLOCK, dtype=torch.bool)
    mask[blk, off] = False
    sent = torch.full((1,), SENTINEL, dtype=torch.int64).view(kc.dtype)[0]
    for c in (kc, vc):
        assert bool((c.permute(0, 2, 1, 3)[mask] == sent).all()), \
            case.id + ": a byte outside the written slots changed"


@pytest.mark.parametrize("cache", [False, True], ids=["nocache", "cache"])
@pytest.mark.parametrize("want_kv", [False, True], ids=["q", "qkv"])
@pytest.mark.parametrize("case", qo.CASES, ids=lambda c: c.id)
def test_oracle_case(case, want_kv, cache):
    b = qo.build(case)
    q, k, v, kv = _run(case, b, cache_dtype=torch.bfloat16 if cache else None,
                       want_kv=want_kv)
    assert q.dtype == torch.bfloat16 and q.shape == (case.T, case.Hq, case.D)
    qo.assert_wq_close(q.cpu().reshape(-1, case.D), b.want_q, qo.TOL_QKNORM,
                       case.id + " q")
    if want_kv:
        qo.assert_wq_close(k.cpu().reshape(-1, case.D), b.want_k,
                           qo.TOL_QKNORM, case.id + " k")
        assert torch.equal(v.cpu(), _v_in(case, b))
    else:
        assert k is None and v is None
    if cache:
        _check_cache(case, b, kv, k if want_kv else None)


@pytest.mark.parametrize("shape", qo.SHAPES, ids=str)
def test_q_is_bitwise_equal_with_and_without_cache(shape):
    for T in qo.TS:
        case = qo.Case(*shape, T, "randn")
        b = qo.build(case)
        q0, k0, _, _ = _run(case, b, want_kv=True)
        q1, k1, _, _ = _run(case, b, cache_dtype=torch.bfloat16, want_kv=True)
        q2, _, _, _ = _run(case, b, cache_dtype=torch.uint8)
        assert torch.equal(q0, q1) and torch.equal(q0, q2), case.id
        assert torch.equal(k0, k1), case.id


@pytest.mark.parametrize("case", [c for c in qo.CASES if c.T in (3, 130)],
                         ids=lambda c: c.id)
def test_fp8_cache(case):
    b = qo.build(case)
    q, k, v, kv = _run(case, b, cache_dtype=torch.uint8, want_kv=True)
    assert kv[0].dtype == torch.uint8
    qo.assert_wq_close(q.cpu().reshape(-1, case.D), b.want_q, qo.TOL_QKNORM,
                       case.id + " q")
    qo.assert_wq_close(k.cpu().reshape(-1, case.D), b.want_k, qo.TOL_QKNORM,
                       case.id + " k")
    _check_cache(case, b, kv)


@pytest.mark.parametrize("shape", qo.SHAPES, ids=str)
def test_strided_qkv(shape):
    """qkv is a column slice of a wider tensor: row stride > width."""
    case = qo.Case(*shape, 17, "randn")
    b = qo.build(case)
    wide = torch.full((case.T, case.width + 192), float("nan"),
                      dtype=torch.bfloat16, device=DEV)
    wide[:, 64:64 + case.width] = b.qkv.to(DEV)
    view = wide[:, 64:64 + case.width]
    assert view.stride(0) > case.width and not view.is_contiguous()
    q, k, v, kv = _run(case, b, qkv=view, cache_dtype=torch.bfloat16,
                       want_kv=True)
    q0, k0, v0, _ = _run(case, b, want_kv=True)
    assert torch.equal(q, q0) and torch.equal(k, k0) and torch.equal(v, v0)
    _check_cache(case, b, kv, k)


def test_empty_batch_returns():
    case = qo.Case(4, 2, 128, 1, "randn")
    b = qo.build(case)
    q, k, v = ops.rope_qkv_cache(
        torch.zeros(0, dtype=torch.int64, device=DEV),
        torch.zeros(0, case.width, dtype=torch.bfloat16, device=DEV),
        _cs(case.D), case.Hq, case.Hkv, case.D, want_kv=True,
        q_norm_w=b.wq.to(DEV), k_norm_w=b.wk.to(DEV), eps=qo.EPS)
    torch.cuda.synchronize()
    assert q.shape == (0, case.Hq, case.D) and k.shape == (0, case.Hkv, case.D)


def test_host_checks_refuse_before_any_launch():
    case = qo.Case(4, 2, 128, 3, "randn")
    b = qo.build(case)
    pos, qkv = b.positions.to(DEV), b.qkv.to(DEV)
    wq, wk = b.wq.to(DEV), b.wk.to(DEV)
    cs = _cs(case.D)
    C = ops._native()

    def native(q_out, **kw):
        a = dict(positions=pos, qkv=qkv, cos_sin=cs, Hq=case.Hq,
                 Hkv=case.Hkv, D=case.D, wq=wq, wk=wk, eps=qo.EPS)
        a.update(kw)
        C.rope_qkv_norm_cache(a["positions"], a["qkv"], q_out, None, None,
                              None, None, None, a["cos_sin"], a["Hq"],
                              a["Hkv"], a["D"], a["wq"], a["wk"], a["eps"])

    q_out = torch.full((case.T, case.Hq * case.D), float("nan"),
                       dtype=torch.bfloat16, device=DEV)
    cs96 = torch.zeros(qo.MAX_POS, 96, dtype=torch.float32, device=DEV)
    w96 = torch.ones(96, dtype=torch.bfloat16, device=DEV)
    bad = (
        # D = 96: 4 + 2*2 heads of 96 = 768 columns
        dict(D=96, qkv=qkv[:, :768].contiguous(), cos_sin=cs96, wq=w96,
             wk=w96),
        dict(wq=wq.float()), dict(wk=wk.float()),        # fp32 weights
        dict(wq=wq[:64].contiguous()),                   # wrong length
        dict(wk=torch.cat([wk, wk])),
        dict(wq=torch.cat([wq, wq])[::2]),               # not contiguous
        dict(wq=wq.cpu()),                               # another device
        dict(eps=0.0), dict(eps=-1e-6),
        dict(positions=pos.int()), dict(cos_sin=cs.double()),
    )
    for kw in bad:
        with pytest.raises(RuntimeError):
            native(q_out, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(q_out).all()), "a refused call launched"
    # one weight missing is refused by the dispatch, with either one
    for kw in (dict(q_norm_w=wq), dict(k_norm_w=wk)):
        with pytest.raises(ValueError):
            ops.rope_qkv_cache(pos, qkv, cs, case.Hq, case.Hkv, case.D,
                               eps=qo.EPS, **kw)
    # through the dispatch too
    with pytest.raises(RuntimeError):
        ops.rope_qkv_cache(pos, qkv, cs, case.Hq, case.Hkv, case.D,
                           q_norm_w=wq, k_norm_w=wk, eps=0.0)
    # the same call is accepted once it is right
    native(q_out)
    torch.cuda.synchronize()
    qo.assert_wq_close(q_out.cpu().reshape(-1, case.D), b.want_q,
                       qo.TOL_QKNORM)


def test_without_weights_the_unnormed_kernel_runs():
    """No weights: the dispatch calls the un-normed binding, bit for bit."""
    case = qo.Case(4, 2, 128, 17, "randn")
    b = qo.build(case)
    pos, qkv = b.positions.to(DEV), b.qkv.to(DEV)
    cs = _cs(case.D)
    q, k, v = ops.rope_qkv_cache(pos, qkv, cs, case.Hq, case.Hkv, case.D,
                                 want_kv=True)
    q_out = torch.empty(case.T, case.Hq * case.D, dtype=torch.bfloat16,
                        device=DEV)
    k_out = torch.empty(case.T, case.Hkv * case.D, dtype=torch.bfloat16,
                        device=DEV)
    v_out = torch.empty_like(k_out)
    ops._native().rope_qkv_cache(pos, qkv, q_out, None, None, None, k_out,
                                 v_out, cs, case.Hq, case.Hkv, case.D)
    assert torch.equal(q.reshape(case.T, -1), q_out)
    assert torch.equal(k.reshape(case.T, -1), k_out)


@pytest.mark.parametrize("shape", [(4, 2, 128), (8, 2, 64)], ids=str)
def test_graph_replay_equals_eager(shape):
    """Captured once, replayed twice with other input contents (positions,
    slots with a pad row, qkv): each replay equals the eager call."""
    T = 17
    cases = [qo.Case(*shape, T, fam) for fam in qo.FAMILIES]
    bs = [qo.build(c) for c in cases]
    case, b0 = cases[0], bs[0]
    cs = _cs(case.D)
    wq, wk = b0.wq.to(DEV), b0.wk.to(DEV)
    s_pos = b0.positions.to(DEV).clone()
    s_qkv = b0.qkv.to(DEV).clone()
    s_slots = b0.slots.to(DEV).clone()
    kv = _cache(case, b0, torch.bfloat16)

    def call(pos, qkv, slots, cache):
        return ops.rope_qkv_cache(pos, qkv, cs, case.Hq, case.Hkv, case.D,
                                  kv_cache=cache, slot_mapping=slots,
                                  want_kv=True, q_norm_w=wq, k_norm_w=wk,
                                  eps=qo.EPS)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(s_pos, s_qkv, s_slots, kv)                  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = call(s_pos, s_qkv, s_slots, kv)
    for c, b in zip(cases[1:], bs[1:]):
        s_pos.copy_(b.positions.to(DEV))
        s_qkv.copy_(b.qkv.to(DEV))
        s_slots.copy_(b.slots.to(DEV))
        for t in kv:
            t.view(torch.int16).fill_(0x5A5A)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in g_out] + [t.clone() for t in kv]
        ekv = _cache(c, b, torch.bfloat16)
        want = list(call(b.positions.to(DEV), b.qkv.to(DEV),
                         b.slots.to(DEV), ekv)) + list(ekv)
        torch.cuda.synchronize()
        for g_t, w_t in zip(got, want):
            assert torch.equal(g_t, w_t), c.id
        qo.assert_wq_close(got[0].cpu().reshape(-1, c.D), b.want_q,
                           qo.TOL_QKNORM, c.id + " replay q")
