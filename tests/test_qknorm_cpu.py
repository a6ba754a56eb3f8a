"""QK-norm + rope on CPU: the test oracle itself (tolerances, mutants) and
ops.rope_qkv_cache's CPU branch with norm weights against the fp64 oracle."""
import functools
from collections import defaultdict

import pytest
import torch

import helix_amd.ops as ops
import qknorm_oracle as qo


@functools.lru_cache(maxsize=None)
def _result(case):
    """(bf16 emulation error, fp8 K error, HF-order error, {mutant: error}),
    each the worst head row of the case."""
    b = qo.build(case)
    q, k, k8 = qo.emulate(b, case)
    err = max(float(qo.wq_error(q, b.want_q).max()),
              float(qo.wq_error(k, b.want_k).max()))
    err8 = float(qo.wq_error(k8, b.want_k).max())
    hq, hk = qo.emulate_hf(b, case)
    hf = max(float(qo.wq_error(hq, b.want_q).max()),
             float(qo.wq_error(hk, b.want_k).max()))
    muts = {m: qo.mutant_error(case, b, m) for m in qo.MUTANTS}
    return err, err8, hf, muts


def test_tolerance():
    """TOL_QKNORM and TOL_QKNORM_FP8 = 4 x the worst emulation error over
    all cases (within rounding of the constants); HF's rounding order passes
    too; every mutant misses the tolerance on at least one family of every
    shape. Prints the numbers and the mutant table."""
    res = {c: _result(c) for c in qo.CASES}
    worst, wcase = max(((r[0], c) for c, r in res.items()),
                       key=lambda p: p[0])
    worst8, wcase8 = max(((r[1], c) for c, r in res.items()),
                         key=lambda p: p[0])
    hf = max(r[2] for r in res.values())
    print(f"worst emulation error {worst:.5f} ({wcase.id}), "
          f"TOL_QKNORM {qo.TOL_QKNORM}")
    print(f"worst e4m3 K emulation error {worst8:.5f} ({wcase8.id}), "
          f"TOL_QKNORM_FP8 {qo.TOL_QKNORM_FP8}")
    print(f"HF rounding order (norm, weight, rope each rounded): {hf:.5f}")
    for D in (64, 128):
        w = max(r[0] for c, r in res.items() if c.D == D)
        print(f"  D = {D}: worst emulation error {w:.5f}")
    assert 4 * worst <= qo.TOL_QKNORM * 1.02, worst
    assert qo.TOL_QKNORM <= 4 * worst * 1.10, worst
    assert 4 * worst8 <= qo.TOL_QKNORM_FP8 * 1.02, worst8
    assert qo.TOL_QKNORM_FP8 <= 4 * worst8 * 1.10, worst8
    assert hf <= qo.TOL_QKNORM
    # mutant -> shape -> family -> worst error over T
    table = defaultdict(lambda: defaultdict(lambda: defaultdict(float)))
    for c, r in res.items():
        for m, v in r[3].items():
            fam = table[m][(c.Hq, c.Hkv, c.D)]
            fam[c.family] = max(fam[c.family], v)
    print(f"{'mutant':18s} {'shape':14s} " +
          " ".join(f"{f:>9s}" for f in qo.FAMILIES))
    for m in qo.MUTANTS:
        for shape in qo.SHAPES:
            fam = table[m][shape]
            print(f"{m:18s} {str(shape):14s} " +
                  " ".join(f"{fam[f]:9.4f}" for f in qo.FAMILIES))
            assert max(fam.values()) > qo.TOL_QKNORM, (m, shape, dict(fam))
    # eps is seen by `small` alone
    for m in ("eps0", "eps1e-5"):
        for shape in qo.SHAPES:
            fam = table[m][shape]
            assert fam["small"] > 10 * qo.TOL_QKNORM
            assert fam["randn"] <= qo.TOL_QKNORM
            assert fam["outlier"] <= qo.TOL_QKNORM


def test_mutant_fails_the_assertion():
    """The mutants fail assert_wq_close itself, the assertion the GPU tests
    use, on a `small` case, which every mutant shows on."""
    case = qo.Case(4, 2, 128, 17, "small")
    b = qo.build(case)
    q, k, k8 = qo.emulate(b, case)
    qo.assert_wq_close(q, b.want_q, qo.TOL_QKNORM)
    qo.assert_wq_close(k, b.want_k, qo.TOL_QKNORM)
    qo.assert_wq_close(k8, b.want_k, qo.TOL_QKNORM_FP8)
    for m in qo.MUTANTS:
        mq, mk, _ = qo.emulate(b, case, m)
        # every mutant changes Q (K's weight on Q changes nothing else)
        with pytest.raises(AssertionError, match="error"):
            qo.assert_wq_close(mq, b.want_q, qo.TOL_QKNORM, m)
        if m != "k_weight_on_q":
            with pytest.raises(AssertionError, match="error"):
                qo.assert_wq_close(mk, b.want_k, qo.TOL_QKNORM, m)


def test_case_inputs_are_what_they_promise():
    for c in qo.CASES:
        b = qo.build(c)
        assert int(b.positions.max()) == qo.MAX_POS - 1
        live = b.slots[b.slots >= 0]
        assert live.numel() >= 1 and live.unique().numel() == live.numel()
        assert int(live.max()) < b.nblocks * qo.BLOCK
        if c.T >= 3:
            assert int((b.slots < 0).sum()) >= 1
        assert float((b.wq.float() - 1).abs().min()) >= 0 and \
            float((b.wq.float() - 1).abs().max()) > 0.3
    assert len(qo.CASES) == len(qo.SHAPES) * len(qo.TS) * len(qo.FAMILIES)


def _call(case, b, cache_dtype=None, want_kv=True, **kw):
    kv_cache = None
    if cache_dtype is not None:
        shape = (b.nblocks, case.Hkv, qo.BLOCK, case.D)
        kv_cache = (torch.zeros(shape, dtype=cache_dtype),
                    torch.zeros(shape, dtype=cache_dtype))
    out = ops.rope_qkv_cache(
        b.positions, b.qkv, qo.cos_sin(case.D), case.Hq, case.Hkv, case.D,
        kv_cache=kv_cache, slot_mapping=b.slots, want_kv=want_kv,
        q_norm_w=b.wq, k_norm_w=b.wk, eps=qo.EPS, **kw)
    return out, kv_cache


CPU_CASES = [c for c in qo.CASES if c.T in (1, 17)]


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_ops_cpu_match_oracle(case):
    b = qo.build(case)
    (q, k, v), (kc, vc) = _call(case, b, torch.bfloat16)
    assert q.dtype == torch.bfloat16 and q.shape == (case.T, case.Hq, case.D)
    qo.assert_wq_close(q.reshape(-1, case.D), b.want_q, qo.TOL_QKNORM,
                       case.id + " q")
    qo.assert_wq_close(k.reshape(-1, case.D), b.want_k, qo.TOL_QKNORM,
                       case.id + " k")
    vin = b.qkv[:, (case.Hq + case.Hkv) * case.D:].view(case.T, case.Hkv,
                                                        case.D)
    assert torch.equal(v, vin)
    rows, blk, off = qo.written_rows(b)
    assert torch.equal(kc[blk, :, off], k[rows])
    assert torch.equal(vc[blk, :, off], vin[rows])
    # nothing else was written
    mask = torch.ones(b.nblocks, qo.BLOCK, dtype=torch.bool)
    mask[blk, off] = False
    assert not kc.permute(0, 2, 1, 3)[mask].any()
    # no compact K/V unless asked; q does not depend on the cache
    (q2, k2, v2), _ = _call(case, b, None, want_kv=False)
    assert k2 is None and v2 is None and torch.equal(q2, q)


def test_ops_cpu_fp8_cache():
    case = qo.Case(4, 2, 128, 17, "randn")
    b = qo.build(case)
    (q, k, v), (kc, vc) = _call(case, b, torch.uint8)
    rows, blk, off = qo.written_rows(b)
    got = ops.kv_fp8_dequant(kc[blk, :, off], torch.float32)
    want = b.want_k.view(case.T, case.Hkv, case.D)[rows]
    qo.assert_wq_close(got.reshape(-1, case.D), want.reshape(-1, case.D),
                       qo.TOL_QKNORM_FP8, "fp8 k cache")


def test_one_weight_alone_is_refused():
    case = qo.Case(4, 2, 128, 3, "randn")
    b = qo.build(case)
    for kw in (dict(q_norm_w=b.wq), dict(k_norm_w=b.wk)):
        with pytest.raises(ValueError, match="go together"):
            ops.rope_qkv_cache(b.positions, b.qkv, qo.cos_sin(case.D),
                               case.Hq, case.Hkv, case.D, eps=qo.EPS, **kw)


def test_without_weights_nothing_changes():
    """Neither weight: the un-normed composition, bit for bit."""
    case = qo.Case(4, 2, 128, 17, "randn")
    b = qo.build(case)
    cs = qo.cos_sin(case.D)
    q, k, v = ops.rope_qkv_cache(b.positions, b.qkv, cs, case.Hq, case.Hkv,
                                 case.D, want_kv=True)
    qs, ks = case.Hq * case.D, case.Hkv * case.D
    qr, kr = ops.reference.rotary_embedding(
        b.positions, b.qkv[:, :qs].contiguous(),
        b.qkv[:, qs:qs + ks].contiguous(), cs, case.D)
    assert torch.equal(q.reshape(case.T, -1), qr)
    assert torch.equal(k.reshape(case.T, -1), kr)


def test_ref_qk_rms_norm_is_per_head():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 3 * 64, generator=g).to(torch.bfloat16)
    w = (0.5 + torch.rand(64, generator=g)).to(torch.bfloat16)
    y = ops.reference.qk_rms_norm(x, w, 1e-6, 64)
    assert y.dtype == torch.float32 and y.shape == x.shape
    for h in range(3):
        xh = x[:, 64 * h:64 * (h + 1)].double()
        want = xh / (xh.pow(2).mean(-1, keepdim=True) + 1e-6).sqrt() \
            * w.double()
        assert torch.allclose(y[:, 64 * h:64 * (h + 1)].double(), want,
                              rtol=1e-5, atol=1e-6)
