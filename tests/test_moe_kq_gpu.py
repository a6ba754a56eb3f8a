"""Routed expert GEMMs over Q4_K/Q6_K experts (ops/hip/moe_kq.hip) and the
tiny-qwen3-moe engine with K-quant experts on the GPU: every kernel the
dispatch can select, exact fragment mapping of both kernels, every oracle
case on both paths, the library path's dequantiser, row independence, host
guards, hipGraph serving, resident Q4_K_M GGUF serving."""
import functools

import pytest
import torch

import helix_amd.ops as ops
import moe_kq_oracle as mq
import moe_oracle as mo
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
FMTS = ("q4_k", "q6_k")
DEEP_GATED = mq.SHAPES[4]            # 8 waves in the gated GEMM
DEEP_DOWN8 = mq.SHAPES[5]            # 8 waves in the down GEMM
DEEP_DOWN16 = mq.SHAPES[6]           # 16


@functools.lru_cache(maxsize=None)
def _gpu_stack(fmt, which, E, H, I):
    return tuple(t.to(DEV) for t in mq.stack_planes(fmt, which, E, H, I))


def _mt(T):
    return 1 if T <= 16 else 2 if T <= 32 else 4


def test_waves_cover_every_kernel():
    """The oracle's mirror of the K split is the host's function, and the
    oracle cases reach every (waves, token tiles) pair the dispatch can
    select: 4 and 8 waves gated, 4, 8 and 16 down, each with MT = 1, 2, 4."""
    assert ops.MOE_KQ_FUSED_MAX_T >= 1
    for N in (16, 256, 768, 2048, 4096, 14336, 65536):
        for K in range(256, 256 * 40, 256):
            for gated in (True, False):
                assert ops.moe_kq_waves(N, K, gated) == mq.waves(N, K, gated)
    gated = {(ops.moe_kq_waves(c.I, c.H, True), _mt(c.T)) for c in mq.CASES}
    down = {(ops.moe_kq_waves(c.H, c.I, False), _mt(c.T)) for c in mq.CASES}
    assert gated == {(w, m) for w in (4, 8) for m in (1, 2, 4)}
    assert down == {(w, m) for w in (4, 8, 16) for m in (1, 2, 4)}
    # no shape can select anything else
    assert {mq.waves(N, K, g) for N in (16, 65536) for K in (256, 256 * 64)
            for g in (True, False)} <= {4, 8, 16}
    # and the shapes this feature is for: Qwen3-30B-A3B, Mixtral
    assert ops.moe_kq_waves(768, 2048, True) == 8
    assert ops.moe_kq_waves(2048, 768, False) == 4
    assert ops.moe_kq_waves(14336, 4096, True) == 8
    assert ops.moe_kq_waves(4096, 14336, False) == 16


# -- exact fragment mapping -------------------------------------------------

_Q4_SC = (4, 12, 20, 40, 24, 48, 36, 60)          # <= 4 significant bits
_Q4_C = (3, 5, 2, 6, 1, 4, 7, 2)                  # min = c scale steps
_Q6_SC = (1, -3, 5, -7, 2, -6, 10, -14, 4, -12, 20, -28, 8, -24, 40, -56)


def _integer_stack(fmt, E, rows, K, positive=False):
    """Planes with an asymmetric integer payload, distinct scale codes in
    every sub-block (rotated by row and super-block, the codes of sub-blocks
    4..7 using their high bits) and power-of-two d, and the bf16-exact
    weight [E, rows, K] they dequantise to.
    q4_k: dmin = 4d and m = sc*c/4, so w = d*sc*(nib - c).
    q6_k: w = d*sc*(u - 32), |sc| = (odd < 8) * 2^s.
    positive: every weight is >= 32 (see test_one_hot_gated_exact)."""
    N, nb = E * rows, K // 256
    row = torch.arange(N)
    e_, r_ = row // rows, row % rows
    sb = torch.arange(nb)
    rot = (r_[:, None] + sb[None, :]) % 8                       # [N, nb]
    dexp = (r_[:, None] * 3 + sb[None, :] * 5 + e_[:, None]) % 5
    k_ = torch.arange(K)
    pat = (r_[:, None] * 7 + k_[None, :] * 3 + e_[:, None] * 11)    # [N, K]
    if fmt == "q4_k":
        j = (torch.arange(8)[None, None, :] + rot[..., None]) % 8   # [N,nb,8]
        sc = torch.tensor(_Q4_SC)[j]
        c = torch.tensor(_Q4_C)[j]
        m = sc * c // 4
        assert int(m.max()) <= 63 and int((sc * c % 4).abs().max()) == 0
        d = 2.0 ** (dexp.float() + (3 if positive else -8))
        cc = c[..., None].expand(N, nb, 8, 32).reshape(N, K)
        if positive:
            nib = cc + 1 + pat % (15 - cc)                       # c < nib <= 15
        else:
            nib = pat % 16
        nib = nib.to(torch.uint8).reshape(N, nb, 4, 2, 32)
        qs = (nib[..., 0, :] | (nib[..., 1, :] << 4)).reshape(N, K // 2)
        scu, mu = sc.to(torch.uint8), m.to(torch.uint8)
        scales = torch.cat([
            scu[..., :4] | ((scu[..., 4:] >> 4) << 6),
            mu[..., :4] | ((mu[..., 4:] >> 4) << 6),
            (scu[..., 4:] & 0xF) | ((mu[..., 4:] & 0xF) << 4)], -1)
        d16 = d.to(torch.float16)[..., None]
        hdr = torch.cat([d16.view(torch.uint8),
                         (4 * d16).view(torch.uint8), scales], -1)
        planes = (qs.contiguous(), hdr.contiguous())
        nibf = nib.reshape(N, nb, 8, 32).float()       # sub-block 2c + j
        w = (d[..., None, None] * sc[..., None].float()
             * (nibf - c[..., None].float())).reshape(N, K)
    else:
        j = (torch.arange(16)[None, None, :] + 2 * rot[..., None]) % 16
        sc = torch.tensor(_Q6_SC)[j]                             # [N, nb, 16]
        if positive:
            sc = sc.abs()
            u = 33 + pat % 31                                    # q in [1, 31]
        else:
            u = pat % 64
        d = 2.0 ** (dexp.float() + (5 if positive else -8))
        u8 = u.to(torch.uint8).reshape(N, nb, 2, 4, 32)          # half, g, l
        lo4, hi2 = u8 & 0x0F, u8 >> 4
        ql = (lo4[..., :2, :] | (lo4[..., 2:, :] << 4)).reshape(N, K // 2)
        qh = (hi2[..., 0, :] | (hi2[..., 1, :] << 2) | (hi2[..., 2, :] << 4)
              | (hi2[..., 3, :] << 6)).reshape(N, K // 4)
        planes = (ql.contiguous(), qh.contiguous(),
                  sc.to(torch.int8).reshape(N, K // 16).contiguous(),
                  d.to(torch.float16).contiguous())
        s = (d[..., None] * sc.float()).reshape(N, nb, 2, 4, 2, 1)
        w = (s * (u.reshape(N, nb, 2, 4, 2, 16).float() - 32)).reshape(N, K)
    # the project's reference dequantiser reads the planes the same way
    assert torch.equal(ops.dequantize_kq(planes, fmt), w)
    assert torch.equal(w.to(torch.bfloat16).float(), w)      # exact in bf16
    assert not positive or float(w.min()) >= 32
    w = w.view(E, rows, K)
    assert not torch.equal(w[0, :32, :32], w[0, :32, :32].t())
    return tuple(p.view(E, rows, *p.shape[1:]) for p in planes), w


def _const_stack(fmt, E, rows, K, value):
    """Planes of the constant weight `value` (a power of two)."""
    N, nb = E * rows, K // 256
    d = torch.full((N, nb), float(value), dtype=torch.float16)
    if fmt == "q4_k":
        hdr = torch.zeros(N, nb, 16, dtype=torch.uint8)
        hdr[..., 0:2] = d[..., None].view(torch.uint8)
        hdr[..., 4:8] = 1                    # sc 1 for sub-blocks 0..3
        hdr[..., 12:16] = 1                  # and 4..7 (low nibble), m = 0
        planes = (torch.full((N, K // 2), 0x11, dtype=torch.uint8), hdr)
    else:
        planes = (torch.full((N, K // 2), 0x11, dtype=torch.uint8),   # u = 33
                  torch.full((N, K // 4), 0xAA, dtype=torch.uint8),
                  torch.ones(N, K // 16, dtype=torch.int8), d)
    assert torch.equal(ops.dequantize_kq(planes, fmt),
                       torch.full((N, K), float(value)))
    return tuple(p.view(E, rows, *p.shape[1:]) for p in planes)


def _one_hot_tokens(E, K, seed):
    """T = E*K tokens, token t the one-hot row `pos` of expert `e`."""
    T = E * K
    order = torch.randperm(T, generator=torch.Generator().manual_seed(seed))
    ids = (order // K).to(torch.int32).view(T, 1)
    rows = torch.zeros(T, K, dtype=torch.bfloat16)
    rows[torch.arange(T), order % K] = 1.0
    return ids, rows, order // K, order % K


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("E, H, I", [(4, 32, 768), (2, 32, DEEP_DOWN8[3]),
                                     (2, 32, DEEP_DOWN16[3])])
def test_one_hot_down_exact(E, H, I, fmt):
    """The down GEMM with topk_w = 1, k = 1 and one-hot activation rows
    returns the dequantised weight transposed, bit for bit, for every K
    position and every expert (4-, 8- and 16-wave kernels)."""
    assert ops.moe_kq_waves(H, I, False) == {768: 4, DEEP_DOWN8[3]: 8,
                                             DEEP_DOWN16[3]: 16}[I]
    C = ops._native()
    planes, w = _integer_stack(fmt, E, H, I)
    ids, act, ex, pos = _one_hot_tokens(E, I, E + I)
    T = E * I
    want = w[ex, :, pos]                                     # [T, H]
    off, pairs = ops.moe_align(ids.to(DEV), E)
    ypair = torch.full((T, H), NAN, dtype=torch.float32, device=DEV)
    C.moe_gemm_down_kq(ypair, act.to(DEV), [p.to(DEV) for p in planes], fmt,
                       torch.ones(T, 1, dtype=torch.float32, device=DEV),
                       off, pairs)
    assert torch.equal(ypair.cpu(), want)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("E, H, I", [(4, 768, 32), (2, DEEP_GATED[2], 32)])
def test_one_hot_gated_exact(E, H, I, fmt):
    """The gated GEMM on one-hot x rows, one side at a time (4- and 8-wave
    kernels). Every driven weight is >= 32, where silu(g) = g exactly in
    fp32 whatever the exponential's last bit is (e^-32 < 2^-24), and the
    other side is the constant 1 resp. 64 (silu(64) = 64):
    gate driven: act = bf16(silu(g) * 1) = g; up driven: act = 64 * u."""
    assert ops.moe_kq_waves(I, H, True) == (4 if H == 768 else 8)
    C = ops._native()
    T = E * H
    ids, x, ex, pos = _one_hot_tokens(E, H, E + H)
    off, pairs = ops.moe_align(ids.to(DEV), E)
    planes, w = _integer_stack(fmt, E, I, H, positive=True)
    for side in ("gate", "up"):
        const = _const_stack(fmt, E, I, H, 1.0 if side == "gate" else 64.0)
        halves = (planes, const) if side == "gate" else (const, planes)
        w13 = [torch.cat([a, b], dim=1).contiguous().to(DEV)
               for a, b in zip(*halves)]
        want = w[ex, :, pos] * (1.0 if side == "gate" else 64.0)   # [T, I]
        assert torch.equal(want.to(torch.bfloat16).float(), want)
        act = torch.full((T, I), NAN, dtype=torch.bfloat16, device=DEV)
        C.moe_gemm_gated_kq(act, x.to(DEV), w13, fmt, off, pairs, 1)
        assert torch.equal(act.cpu().float(), want), side


# -- oracle cases -----------------------------------------------------------

def _run(b, case, fused):
    """moe_experts_kq on the GPU with NaN-filled act / ypair and NaN guard
    rows around out. Returns out (on the CPU)."""
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    p13 = _gpu_stack(case.f13, "w13", E, H, I)
    p2 = _gpu_stack(case.f2, "w2", E, H, I)
    ids, w = ops.moe_route(b.logits.to(DEV), k)
    big = torch.full((T + 2, H), NAN, dtype=torch.bfloat16, device=DEV)
    act = torch.full((T * k, I), NAN, dtype=torch.bfloat16, device=DEV)
    ypair = torch.full((T * k, H), NAN, dtype=torch.float32, device=DEV)
    out = ops.moe_experts_kq(b.x.to(DEV), p13, p2, case.fmt, ids, w,
                             fused=fused, out=big[1:T + 1], act=act,
                             ypair=ypair)
    assert out.data_ptr() == big[1].data_ptr()
    assert torch.isnan(big[0]).all() and torch.isnan(big[T + 1]).all()
    assert torch.isfinite(act.float()).all()
    assert torch.isfinite(ypair).all()
    return out.cpu()


@pytest.mark.parametrize("case", mq.CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    """Fused kernels and the library path against the fp64 oracle."""
    b = mq.build(case)
    got = _run(b, case, True)
    err = float(mq.wq_error(got, b.want).max())
    lib = _run(b, case, False)
    err_lib = float(mq.wq_error(lib, b.want).max())
    print(f"{case.id}: fused {err:.5f}, library {err_lib:.5f}, "
          f"tol {mq.TOL_MOE_KQ}")
    mq.assert_wq_close(got, b.want, mq.TOL_MOE_KQ, case.id + " fused")
    mq.assert_wq_close(lib, b.want, mq.TOL_MOE_KQ, case.id + " library")


@pytest.mark.parametrize("fmt", FMTS)
def test_library_dequant_of_a_stack_slice_is_exact(fmt):
    """The library path's weight: dequant_kq of one expert's slices of the
    planes equals the CPU dequantisation (what the fused kernel's registers
    hold), bit for bit, also through a shared scratch."""
    E, _, H, I = DEEP_DOWN8
    p13 = _gpu_stack(fmt, "w13", E, H, I)
    p2 = _gpu_stack(fmt, "w2", E, H, I)
    w13 = mq.dense_stack(fmt, "w13", E, H, I)
    w2 = mq.dense_stack(fmt, "w2", E, H, I)
    c13 = mq.stack_planes(fmt, "w13", E, H, I)
    assert torch.equal(ops.dequantize_experts_kq(c13, fmt), w13)
    scratch = torch.empty(2 * I * H + 64, dtype=torch.bfloat16, device=DEV)
    for e in range(E):
        got = ops.dequant_kq([p[e] for p in p13], fmt, out=scratch)
        assert got.data_ptr() == scratch.data_ptr()
        assert torch.equal(got.cpu(), w13[e])
        got = ops.dequant_kq([p[e] for p in p2], fmt, out=scratch)
        assert torch.equal(got.cpu(), w2[e])
        assert torch.equal(ops.dequant_kq([p[e] for p in p2], fmt).cpu(),
                           w2[e])


@pytest.mark.parametrize("fmt", FMTS)
def test_default_path_follows_the_cutoff(monkeypatch, fmt):
    """fused=None: the fused kernels up to MOE_KQ_FUSED_MAX_T tokens, the
    library path above (told apart by the library path's host sync); the
    cutoff is read at call time."""
    E, k, H, I = 8, 2, 256, 256
    p13 = _gpu_stack(fmt, "w13", E, H, I)
    p2 = _gpu_stack(fmt, "w2", E, H, I)
    c13 = mq.stack_planes(fmt, "w13", E, H, I)
    c2 = mq.stack_planes(fmt, "w2", E, H, I)
    synced = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist",
                        lambda t: synced.append(1) or real(t))
    for cutoff in (ops.MOE_KQ_FUSED_MAX_T, 5):
        monkeypatch.setattr(ops, "MOE_KQ_FUSED_MAX_T", cutoff)
        for T in (cutoff, cutoff + 1):
            g = torch.Generator().manual_seed(T)
            x = torch.randn(T, H, generator=g).to(torch.bfloat16).to(DEV)
            logits = torch.randn(T, E, generator=g).to(torch.bfloat16).to(DEV)
            synced.clear()
            out = ops.moe_forward_kq(x, logits, p13, p2, fmt, k)
            assert bool(synced) == (T > cutoff)
            ref = ops.moe_forward_kq(x.cpu(), logits.cpu(), c13, c2, fmt, k)
            mq.assert_wq_close(out.cpu(), ref.double(), 2 * mq.TOL_MOE_KQ,
                               f"T={T}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", [(8, 2, 256, 256), (4, 2, 256, 768),
                                   DEEP_GATED, DEEP_DOWN16], ids=str)
def test_row_independence(shape, fmt):
    """One token row (its x and its logits) gives the same bits whatever
    T is, wherever it sits, whoever its neighbours are (crowding its experts
    or avoiding them) and however many zero pad rows follow."""
    E, k, H, I = shape
    p13 = _gpu_stack(fmt, "w13", E, H, I)
    p2 = _gpu_stack(fmt, "w2", E, H, I)
    g = torch.Generator().manual_seed(17 + H)
    x0 = (torch.randn(H, generator=g) + 1.0).to(torch.bfloat16)
    l0, _ = mo.make_logits(E, k, 1, "uniform", g)
    mine = mo.route_ref(l0, k)[0][0].tolist()

    def neighbours(T, how):
        x = torch.randn(T, H, generator=g).to(torch.bfloat16)
        lg, perm = mo.make_logits(E, k, T, "uniform", g)
        if how == "crowd":                       # everyone wants my experts
            lg = l0.expand(T, E).clone()
        elif how == "avoid":                     # nobody does
            lg[:, mine] = -30.0
        return x, lg

    def run(T, pos, how, pad=0):
        x, lg = neighbours(T, how)
        x[pos], lg[pos] = x0, l0[0]
        if pad:
            x = torch.cat([x, torch.zeros(pad, H, dtype=x.dtype)])
            lg = torch.cat([lg, torch.zeros(pad, E, dtype=lg.dtype)])
        ids = mo.route_ref(lg, k)[0]
        n_mine = int((ids == mine[0]).sum())
        out = ops.moe_forward_kq(x.to(DEV), lg.to(DEV), p13, p2, fmt, k,
                                 fused=True)
        assert torch.isfinite(out.float()).all()
        return out[pos].cpu(), n_mine

    base, _ = run(1, 0, "uniform")
    assert float(base.float().abs().max()) > 0
    seen = []
    for T, pos, how, pad in ((17, 5, "uniform", 0), (64, 63, "crowd", 0),
                             (130, 100, "crowd", 0), (130, 100, "avoid", 0),
                             (64, 0, "avoid", 0), (3, 2, "uniform", 1),
                             (17, 16, "uniform", 15), (65, 64, "crowd", 63)):
        got, n_mine = run(T, pos, how, pad)
        seen.append(n_mine)
        assert torch.equal(got, base), (T, pos, how, pad)
    assert max(seen) >= 128 and min(seen) == 1    # both extremes were run


_PLANE_NAMES = {"q4_k": ("qs", "hdr"), "q6_k": ("ql", "qh", "sc", "d")}


def test_host_guards():
    """Each rejected input raises before any launch: the NaN-filled outputs
    stay untouched."""
    C = ops._native()
    E, k, H, I, T = 8, 2, 256, 256, 5
    P = T * k

    def stack(fmt, E, rows, K):
        if fmt == "q4_k":
            return [torch.zeros(E, rows, K // 2, dtype=torch.uint8,
                                device=DEV),
                    torch.zeros(E, rows, K // 256, 16, dtype=torch.uint8,
                                device=DEV)]
        return [torch.zeros(E, rows, K // 2, dtype=torch.uint8, device=DEV),
                torch.zeros(E, rows, K // 4, dtype=torch.uint8, device=DEV),
                torch.zeros(E, rows, K // 16, dtype=torch.int8, device=DEV),
                torch.zeros(E, rows, K // 256, dtype=torch.float16,
                            device=DEV)]

    def fresh(E=E, k=k, H=H, I=I, T=T, fmt="q4_k"):
        P = T * k
        return dict(
            fmt=fmt,
            x=torch.zeros(T, H, dtype=torch.bfloat16, device=DEV),
            w13=stack(fmt, E, 2 * I, H), w2=stack(fmt, E, H, I),
            tw=torch.ones(T, k, dtype=torch.float32, device=DEV),
            off=torch.zeros(E + 1, dtype=torch.int32, device=DEV),
            pairs=torch.zeros(P, dtype=torch.int32, device=DEV),
            act=torch.full((P, I), NAN, dtype=torch.bfloat16, device=DEV),
            ypair=torch.full((P, H), NAN, dtype=torch.float32, device=DEV))

    def gated(d, k=k):
        C.moe_gemm_gated_kq(d["act"], d["x"], d["w13"], d["fmt"], d["off"],
                            d["pairs"], k)

    def down(d):
        C.moe_gemm_down_kq(d["ypair"], d["act"], d["w2"], d["fmt"], d["tw"],
                           d["off"], d["pairs"])

    def misaligned(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        return buf[1:].view(t.shape)

    def strided(t):
        buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype,
                          device=DEV)
        return buf[..., :t.shape[-1]]

    def bad(change, call=None, **shape):
        d = fresh(**shape)
        change(d)
        for fn in ([call] if call else [gated, down]):
            with pytest.raises(RuntimeError):
                fn(d)
        torch.cuda.synchronize()
        for n in ("act", "ypair"):               # still all NaN
            assert bool(torch.isnan(d[n].float()).all()), n

    def plane(w, i, f):
        def change(d):
            d[w][i] = f(d[w][i])
        return change

    # the good calls run, both formats (an empty offset table: nothing is
    # written), and so does T = 0
    for fmt in FMTS:
        d = fresh(fmt=fmt)
        gated(d), down(d)
        torch.cuda.synchronize()
        assert bool(torch.isnan(d["ypair"]).all())
        d = fresh(fmt=fmt, T=0)
        gated(d), down(d)

    has_two = torch.cuda.device_count() > 1
    for w, call in (("w13", gated), ("w2", down)):
        for fmt in FMTS:
            n = len(_PLANE_NAMES[fmt])
            # plane count
            bad(lambda d: d.update({w: d[w][:-1]}), call, fmt=fmt)
            bad(lambda d: d.update({w: d[w] + d[w][:1]}), call, fmt=fmt)
            bad(lambda d: d.update({w: []}), call, fmt=fmt)
            for i in range(n):
                # dtype, rank, shape, alignment, layout, device
                bad(plane(w, i, lambda t: t.view(
                    {torch.uint8: torch.int8, torch.int8: torch.uint8,
                     torch.float16: torch.bfloat16}[t.dtype])), call, fmt=fmt)
                bad(plane(w, i, lambda t: t.to(torch.int32)), call, fmt=fmt)
                bad(plane(w, i, lambda t: t[0]), call, fmt=fmt)
                bad(plane(w, i, lambda t: t.reshape(-1, *t.shape[2:])), call,
                    fmt=fmt)
                bad(plane(w, i, lambda t: t[:-1].contiguous()), call, fmt=fmt)
                bad(plane(w, i, lambda t: t[:, :-1].contiguous()), call,
                    fmt=fmt)
                bad(plane(w, i, lambda t: t[:, :, :-1].contiguous()), call,
                    fmt=fmt)
                bad(plane(w, i, misaligned), call, fmt=fmt)
                bad(plane(w, i, strided), call, fmt=fmt)
                bad(plane(w, i, lambda t: t.cpu()), call, fmt=fmt)
                if has_two and i > 0:
                    bad(plane(w, i, lambda t: t.to("cuda:1")), call, fmt=fmt)
            if has_two:
                bad(lambda d: d.update({w: [t.to("cuda:1") for t in d[w]]}),
                    call, fmt=fmt)
        # format names; q6_k planes named q4_k and the reverse
        for name in ("q4_0", "q5_k", "", "Q4_K"):
            bad(lambda d: d.update(fmt=name), call)
        bad(lambda d: d.update(fmt="q6_k"), call)
        bad(lambda d: d.update(fmt="q4_k"), call, fmt="q6_k")
    # K % 256, N % 16, rows == 2I
    for fmt in FMTS:
        bad(lambda d: None, gated, H=128, fmt=fmt)   # K of gated
        bad(lambda d: None, gated, H=384, fmt=fmt)
        bad(lambda d: None, gated, H=288, fmt=fmt)
        bad(lambda d: None, down, I=128, fmt=fmt)    # K of down
        bad(lambda d: None, down, I=288, fmt=fmt)
        bad(lambda d: d.update(w13=stack(fmt, E, 2 * 24, H),
                               act=torch.full((P, 24), NAN, device=DEV,
                                              dtype=torch.bfloat16)),
            gated, fmt=fmt)                          # N of gated
        bad(lambda d: d.update(w2=stack(fmt, E, 40, I),
                               ypair=torch.full((P, 40), NAN, device=DEV)),
            down, fmt=fmt)                           # N of down
    # x / act / ypair / topk_w
    bad(lambda d: d.update(x=d["x"].half()), gated)
    bad(lambda d: d.update(x=d["x"].cpu()), gated)
    bad(lambda d: d.update(x=strided(d["x"])), gated)
    bad(lambda d: d.update(x=misaligned(d["x"])), gated)
    bad(lambda d: d.update(x=d["x"][:, :128].contiguous()), gated)
    bad(lambda d: d.update(x=d["x"][:T - 1]), gated)
    bad(lambda d: d.update(act=d["act"][:P - 1]), gated)
    bad(lambda d: d.update(act=d["act"].float()), gated)
    bad(lambda d: d.update(ypair=d["ypair"].bfloat16()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:, :128].contiguous()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:P - 1]), down)
    bad(lambda d: d.update(act=d["act"][:P - 1]), down)
    bad(lambda d: d.update(tw=d["tw"].double()), down)
    bad(lambda d: d.update(tw=d["tw"][:, :1].contiguous()), down)
    # lists, E and k: as the bf16 entry points
    bad(lambda d: d.update(off=d["off"].long()))
    bad(lambda d: d.update(off=d["off"][:E]))
    bad(lambda d: d.update(pairs=d["pairs"][:P - 1]))
    bad(lambda d: d.update(pairs=d["pairs"].long()))
    bad(lambda d: None, E=257, H=256, I=256)
    bad(lambda d: None, lambda d: gated(d, k=9), k=9, E=16)
    bad(lambda d: None, down, k=9, E=16)
    bad(lambda d: None, E=1, k=2)
    bad(lambda d: None, lambda d: gated(d, k=0))
    # the op-level wrapper refuses what the library path cannot take
    d = fresh()
    ids = torch.zeros(T, k, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.moe_experts_kq(d["x"], d["w13"], d["w2"], "q4_k", ids,
                           d["tw"][:, :1], fused=False)
    with pytest.raises(ValueError):
        ops.moe_experts_kq(d["x"], d["w13"], d["w2"], "q4_0", ids, d["tw"])
    with pytest.raises(ValueError):
        ops.moe_experts_kq(d["x"], d["w13"], d["w2"], "q6_k", ids, d["tw"])


# -- engine -----------------------------------------------------------------

def _model(seed, fmt=None):
    """tiny-qwen3-moe on the CPU from `seed`, its experts quantised there
    (ops.quantize_kq's argmax over equal magnitudes is not promised to agree
    across devices)."""
    from helix_amd.models.llama import LlamaForCausalLM, get_preset
    from helix_amd.models.quant import quantize_model_experts_kq
    m = LlamaForCausalLM(get_preset("tiny-qwen3-moe")).to(torch.bfloat16) \
        .init_random(seed)
    if fmt is not None:
        assert quantize_model_experts_kq(m, fmt) == 2
    return m


def _mk(enforce_eager: bool, model, seed=7):
    cfg = EngineConfig(model="tiny-qwen3-moe", max_model_len=512,
                       max_num_seqs=8, kv_cache_blocks=256, eos_token_id=-1,
                       seed=seed, enforce_eager=enforce_eager)
    return LLMEngine(cfg, device=DEV, model=model.to(DEV))


def test_kquant_experts_graph_matches_eager_greedy():
    """q4_k gate/up with q6_k down (a Q4_K_M layer): batch 3 replays the
    bucket-4 graph and equals eager greedy token for token; the model owns
    one dequant scratch and its Q6_K `d` planes stay fp16."""
    prompts = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11], [12] * 33]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    fmt = ("q4_k", "q6_k")
    eager = _mk(True, _model(11, fmt))
    mlps = [l.mlp for l in eager.model.layers]
    assert all(m.expert_fmt == fmt for m in mlps)
    assert all(m.w2_d.dtype == torch.float16 and m.w13_qs.is_cuda
               for m in mlps)
    assert mlps[0].scratch is not None
    assert all(m.scratch is mlps[0].scratch for m in mlps)
    cfg = eager.model_cfg
    assert mlps[0].scratch.numel() >= \
        2 * cfg.intermediate_size * cfg.hidden_size
    out_eager = eager.generate(prompts, sp)
    eng = _mk(False, _model(11, fmt))
    assert eng.graph_runner is not None
    out_graph = eng.generate(prompts, sp)
    assert out_eager == out_graph
    assert all(len(o) == 24 for o in out_graph)
    # and the experts matter: bf16 experts decode something else
    assert out_graph != _mk(False, _model(11)).generate(prompts, sp)


def test_kquant_experts_continuous_batching():
    """Mixed prompt lengths joined mid-flight match one-by-one generation."""
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    prompts = {"a": [1, 2, 3], "b": [4, 5, 6, 7] * 9, "c": [8] * 17}
    eng = _mk(False, _model(11, "q6_k"))
    eng.add_request("a", prompts["a"], sp)
    eng.step()
    eng.add_request("b", prompts["b"], sp)
    eng.step()
    eng.add_request("c", prompts["c"], sp)
    while eng.has_work:
        eng.step()
    assert eng.num_free_blocks() == 256
    solo = _mk(False, _model(11, "q6_k"))
    for name, p in prompts.items():
        assert eng.seqs[name].output_ids == solo.generate([p], sp)[0], name


def test_resident_q4_k_m_gguf_serves_what_dequantised_experts_serve(tmp_path):
    """A q4_k_m-expert GGUF of tiny-qwen3-moe, loaded resident, decodes
    inside the hipGraph the tokens of the bf16 engine that carries the same
    experts dequantised (attention left bf16 in both)."""
    from helix_amd.engine.gguf import export_model_gguf, load_gguf_weights
    src = _model(11)
    path = str(tmp_path / "qwen3moe-q4_k_m.gguf")
    export_model_gguf(src, path, expert_quant="q4_k_m")
    dst = _model(12)
    load_gguf_weights(dst, path, keep_quantized=True)
    assert [l.mlp.expert_fmt for l in dst.layers] == \
        [("q4_k", "q4_k"), ("q4_k", "q6_k")]
    dense = _model(13)
    load_gguf_weights(dense, path)
    for a, b in zip(dst.layers, dense.layers):
        assert b.mlp.expert_fmt is None
        assert torch.equal(
            b.mlp.w2.data, ops.dequantize_experts_kq(a.mlp.expert_planes("w2"),
                                                     a.mlp.expert_fmt[1]))
    prompts = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11]]
    sp = SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True)
    eng = _mk(False, dst)
    assert eng.graph_runner is not None
    got = eng.generate(prompts, sp)
    assert all(len(o) == 16 for o in got)
    assert got == _mk(False, dense).generate(prompts, sp)
