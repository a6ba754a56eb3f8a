"""Shared inputs, fp64 oracle, rounding emulation, mutants and metric for
the Q4_K/Q6_K weight-only GEMM tests (test_kq_cpu.py, test_kq_gpu.py).

Every GPU oracle case is built here, on the CPU, from a seed, so that the
CPU file can show on the very same inputs that the emulation of the
kernel's rounding passes and that each mutant fails. The metric and the
assertion are wq_oracle's.
"""
import functools
from dataclasses import dataclass

import torch

import helix_amd.ops as ops
from wq_oracle import assert_wq_close, emulate, oracle, wq_error  # noqa: F401

# tol = 4 x the worst error of the rounding emulation against the fp64 oracle
# over all cases; test_kq_cpu.py::test_tolerance shows that worst error is
# within the Q4_0/Q8_0 tests' 0.0068, so their tolerance carries over.
TOL_KQ = 0.027

KQ_KERNEL_MAX_M = 32          # gemm_kq.hip KQ_MAX_M; the GPU file holds it
FMTS = ("q4_k", "q6_k")
MS = tuple(m for m in (1, 2, 15, 16, 17, 32) if m <= KQ_KERNEL_MAX_M)
# (16, 256) is the smallest legal weight; (48, 768) has three super-blocks,
# fewer than any K split, so some waves have no work; the last two take the
# 16- and 8-wave kernels, the first three the 4-wave one.
NKS = ((16, 256), (48, 768), (512, 512), (256, 4352), (32, 2304))
FAMILIES = ("needle", "randn")
FALLBACK_MS = (ops.KQ_FUSED_MAX_M + 1, 128)
# the mixed projection of the segment and fallback tests
MIXED_K = 768
MIXED_SEGS = (("q4_k", 16), ("q4_k", 16), ("q6_k", 32))


@dataclass(frozen=True)
class Case:
    fmt: str
    M: int
    N: int
    K: int
    bias: bool
    family: str

    @property
    def id(self):
        return (f"{self.fmt}-M{self.M}-N{self.N}-K{self.K}-"
                f"{'bias' if self.bias else 'nobias'}-{self.family}")


CASES = [Case(f, m, n, k, b, fam) for f in FMTS for (n, k) in NKS
         for m in MS for b in (False, True) for fam in FAMILIES]


@dataclass
class Built:
    x: torch.Tensor          # [M, K] bf16
    planes: tuple
    bias: torch.Tensor       # [N] bf16 or None
    want: torch.Tensor       # [M, N] fp64


def make_weight(fmt, N, K, family, salt=0):
    g = torch.Generator().manual_seed(
        1000 * N + K + (7 if fmt == "q6_k" else 0) + 100003 * salt)
    w = torch.randn(N, K, generator=g)
    if family == "needle":
        # neighbouring 32-element sub-blocks and neighbouring rows differ by
        # at least 2x in scale, so a scale taken from the wrong one shows
        nblk = K // 32
        e = (torch.arange(N)[:, None] + 3 * torch.arange(nblk)[None, :]) % 7
        w = (w.view(N, nblk, 32) * (2.0 ** e.float())[..., None] * 0.01)
        w = w.reshape(N, K)
    return w


@functools.lru_cache(maxsize=None)
def _weight(fmt, N, K, family):
    return ops.quantize_kq(make_weight(fmt, N, K, family), fmt)


def make_x(M, K, family, g):
    x = torch.randn(M, K, generator=g)
    if family == "needle":
        # exactly wq_oracle's: one dominant activation per token, in the
        # LAST super-block, at a position that walks over the 32 slots of
        # its last sub-block (M <= 32: every slot is used once)
        m = torch.arange(M)
        x[m, K - 1 - (m % 32)] = 24.0
    else:
        # unit mean: a constant added to every weight of a sub-block (a
        # wrong min or offset) is invisible to activations that sum to 0
        x = x + 1.0
    return x.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def build(case: Case) -> Built:
    planes = _weight(case.fmt, case.N, case.K, case.family)
    g = torch.Generator().manual_seed(case.M * 131 + case.K)
    x = make_x(case.M, case.K, case.family, g)
    bias = None
    if case.bias:
        bias = torch.randn(case.N, generator=g).to(torch.bfloat16)
    want = oracle(x, ops.dequantize_kq(planes, case.fmt), bias)
    return Built(x, planes, bias, want)


@functools.lru_cache(maxsize=None)
def build_mixed(M: int, bias: bool):
    """The three-segment projection 16 q4_k | 16 q4_k | 32 q6_k at K = 768:
    (x, [(fmt, planes)], bias [64] or None, fp64 oracle of the whole)."""
    segs = [(fmt, ops.quantize_kq(
        make_weight(fmt, n, MIXED_K, "needle", salt=i + 1), fmt))
        for i, (fmt, n) in enumerate(MIXED_SEGS)]
    g = torch.Generator().manual_seed(M * 131 + MIXED_K + 5)
    x = make_x(M, MIXED_K, "needle", g)
    b = torch.randn(64, generator=g).to(torch.bfloat16) if bias else None
    w = torch.cat([ops.dequantize_kq(p, f) for f, p in segs], dim=0)
    return x, segs, b, oracle(x, w, b)


# -- mutants: a dequantizer with one deliberate error --------------------

def _q4k_fields(planes):
    """(d, dmin [N,nb,1]; sc, m [N,nb,8] fp32; lo, hi nibbles [N,nb,4,32])."""
    qs, hdr = planes
    N, nb = hdr.shape[:2]
    d = hdr[..., 0:2].contiguous().view(torch.float16).float()
    dmin = hdr[..., 2:4].contiguous().view(torch.float16).float()
    s = hdr[..., 4:16].to(torch.int32)
    sc = torch.cat([s[..., 0:4] & 63,
                    (s[..., 8:12] & 0xF) | ((s[..., 0:4] >> 6) << 4)], -1)
    m = torch.cat([s[..., 4:8] & 63,
                   (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], -1)
    b = qs.reshape(N, nb, 4, 32)
    return d, dmin, sc.float(), m.float(), (b & 0x0F).float(), \
        (b >> 4).float()


def _q4k_value(d, dmin, sc, m, lo, hi):
    N, nb = sc.shape[:2]
    nib = torch.stack([lo, hi], dim=3).reshape(N, nb, 8, 32)
    y = (d * sc)[..., None] * nib - (dmin * m)[..., None]
    return y.reshape(N, nb * 256)


def _q6k_fields(planes):
    """(low4 [N,nb,2,4,32] int, qh [N,nb,2,1,32] uint8, sc [N,nb,16] int8,
    d [N,nb,1] fp32)."""
    ql, qh, sc, d = planes
    N, nb = d.shape
    b = ql.reshape(N, nb, 2, 2, 32)
    low = torch.cat([b & 0x0F, b >> 4], dim=3).to(torch.int32)
    return low, qh.reshape(N, nb, 2, 1, 32), sc.reshape(N, nb, 16), \
        d.float().reshape(N, nb, 1)


def _q6k_value(low, high, scales, d, offset=32):
    """scales: fp32 [N, nb, 16] as the kernel would have read them."""
    N, nb = d.shape[:2]
    q = (low | (high << 4)) - offset
    s = (d * scales).reshape(N, nb, 2, 4, 2, 1)
    y = s * q.reshape(N, nb, 2, 4, 2, 16).float()
    return y.reshape(N, nb * 256)


_SHIFTS = torch.tensor([0, 2, 4, 6], dtype=torch.uint8).view(4, 1)


def mutant_weights(planes, fmt):
    """{name: fp32 [N, K] weight a broken kernel would have used}."""
    good = ops.dequantize_kq(planes, fmt)
    out = {}
    if fmt == "q4_k":
        d, dmin, sc, m, lo, hi = _q4k_fields(planes)
        assert torch.equal(_q4k_value(d, dmin, sc, m, lo, hi), good)
        out["min_ignored"] = _q4k_value(d, dmin, sc, m * 0, lo, hi)
        out["sc_m_swapped"] = _q4k_value(d, dmin, m, sc, lo, hi)
        out["d_dmin_swapped"] = _q4k_value(dmin, d, sc, m, lo, hi)
        # the j >= 4 codes without the two bits kept in scales[j-4], [j]
        sc2, m2 = sc.clone(), m.clone()
        sc2[..., 4:] = sc[..., 4:].to(torch.int32) & 0xF
        m2[..., 4:] = m[..., 4:].to(torch.int32) & 0xF
        out["upper_scale_bits_dropped"] = _q4k_value(d, dmin, sc2, m2, lo, hi)
        out["nibble_pair_swapped"] = _q4k_value(d, dmin, sc, m, hi, lo)
        out["scale_next_sub_block"] = _q4k_value(
            d, dmin, sc.roll(-1, -1), m.roll(-1, -1), lo, hi)
    else:
        low, qh, sc, d = _q6k_fields(planes)
        high = ((qh >> _SHIFTS) & 3).to(torch.int32)
        scf = sc.float()
        assert torch.equal(_q6k_value(low, high, scf, d), good)
        out["qh_ignored"] = _q6k_value(low, high * 0, scf, d)
        out["qh_shift_off_by_one_group"] = _q6k_value(
            low, high.roll(-1, 3), scf, d)
        out["scales_unsigned"] = _q6k_value(
            low, high, sc.view(torch.uint8).float(), d)
        out["scale_next"] = _q6k_value(low, high, scf.roll(-1, -1), d)
        out["offset_31"] = _q6k_value(low, high, scf, d, offset=31)
    w = good.clone()
    w[:, -256:] = 0
    out["drop_last_super_block"] = w
    w = good.clone()
    w[:, -32:] = 0
    out["drop_last_32"] = w
    w = good.clone()
    w[-16:] = 0
    out["drop_last_channel_tile"] = w
    return out


MUTANTS_Q4K = {"min_ignored", "sc_m_swapped", "d_dmin_swapped",
               "upper_scale_bits_dropped", "nibble_pair_swapped",
               "scale_next_sub_block"}
MUTANTS_Q6K = {"qh_ignored", "qh_shift_off_by_one_group", "scales_unsigned",
               "scale_next", "offset_31"}
MUTANTS_BOTH = {"drop_last_super_block", "drop_last_32",
                "drop_last_channel_tile", "zeros"}


def mutant_outputs(case: Case, b: Built):
    outs = {}
    for name, w in mutant_weights(b.planes, case.fmt).items():
        bias = b.bias
        if name == "drop_last_channel_tile" and bias is not None:
            bias = bias.clone()
            bias[-16:] = 0              # the tile is not written at all
        outs[name] = emulate(b.x, w, bias)
    outs["zeros"] = torch.zeros_like(outs["drop_last_32"])
    return outs
