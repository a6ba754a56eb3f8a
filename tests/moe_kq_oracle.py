"""Shared inputs, fp64 oracle, rounding emulation, mutants and metric for
the K-quant mixture-of-experts tests (test_moe_kq_cpu.py,
test_moe_kq_gpu.py).

moe_oracle's routing families, ladder logits and metric; the expert weights
are quantised by ops.quantize_kq. The fp64 oracle runs on the EXACTLY
dequantised weights ((d*sc)*nib - dmin*m resp. (d*sc)*(u - 32), evaluated in
fp64, where every product and the difference are exact), so quantisation
error is not in the metric; the emulation rounds where the kernels round:
the exact weight to fp32 and then to bf16, fp32 accumulation, act to bf16,
ypair in fp32, out to bf16.

Weight pattern, per stack and in the granularity of its format's scales (32
for q4_k, 16 for q6_k): run b of row n (n counted within the gate half and
the up half separately, plus one in the up half) is scaled by 2^((n + b) % 3),
so neighbouring sub-blocks, neighbouring rows and a gate row and its up row
never share a scale. Every 32-element sub-block has a mean of +-0.5 sigma,
the sign alternating with sub-block, row and expert: a Q4_K sub-block's min
is then far from a fixed multiple of its scale, so dmin*m matters and cannot
be traded against d*sc, while a row's sum stays near zero (a common mean
would swamp what tells two experts apart). The last super-block of the down
weights is four times larger: with 17 super-blocks (I = 4352) a dropped last
one of plain weights is 1/17 of the energy.
x has mean 1: a constant added to every weight of a sub-block (a dropped
min, offset 31 for 32) cannot hide behind activations that sum to zero.

Shapes: the smallest at which each thing can go wrong, then one deep shape
per further wave count of the K split (`waves`, a mirror of the host's
moe_kq_waves that test_moe_kq_gpu.py holds to the native function): the
smallest number of super-blocks that selects the count, plus one, so the
waves' shares are uneven.
"""
import functools
from dataclasses import dataclass

import torch

import helix_amd.ops as ops
from moe_oracle import (FAMILIES, align_ref, make_logits,  # noqa: F401
                        route_ref)
from wq_oracle import assert_wq_close, wq_error  # noqa: F401

# tol = 4 x the worst error of the rounding emulation against the fp64 oracle
# over all cases (test_moe_kq_cpu.py::test_tolerance re-derives it and prints
# both numbers; docs/KERNELS.md records them).
TOL_MOE_KQ = 0.0382

FMT_PAIRS = (("q4_k", "q4_k"), ("q4_k", "q6_k"), ("q6_k", "q6_k"))
TS = (1, 16, 17, 65, 130)


def waves(N, K, gated):
    """Mirror of moe_kq.hip's moe_kq_waves_host."""
    w, cap = 4, 8 if gated else 16
    while w < cap and (N // 16) * w < 4096 and K // 256 >= 2 * w:
        w *= 2
    return w


def _deep_k(N, gated, want):
    """K of the smallest super-block count that selects `want` waves for an
    [N, K] weight, plus one super-block."""
    nsb = next(n for n in range(1, 65) if waves(N, 256 * n, gated) == want)
    assert waves(N, 256 * (nsb + 1), gated) == want
    return 256 * (nsb + 1)


# (E, k, H, I): one super-block in both GEMMs (most waves idle); three in
# the gated GEMM; three in the down GEMM (Qwen3's I); empty lists and k = 8;
# then the deep ones
SHAPES = ((8, 2, 256, 256), (8, 2, 768, 256), (4, 2, 256, 768),
          (64, 8, 256, 256),
          (4, 2, _deep_k(256, True, 8), 256),
          (4, 2, 256, _deep_k(256, False, 8)),
          (4, 2, 256, _deep_k(256, False, 16)))


@dataclass(frozen=True)
class Case:
    f13: str
    f2: str
    E: int
    k: int
    H: int
    I: int
    T: int
    family: str

    @property
    def fmt(self):
        return (self.f13, self.f2)

    @property
    def id(self):
        return (f"{self.f13}+{self.f2}-E{self.E}k{self.k}-H{self.H}-"
                f"I{self.I}-T{self.T}-{self.family}")


CASES = [Case(f13, f2, E, k, H, I, T, fam) for (f13, f2) in FMT_PAIRS
         for (E, k, H, I) in SHAPES for T in TS for fam in FAMILIES]


@dataclass
class Built:
    x: torch.Tensor          # [T, H] bf16
    logits: torch.Tensor     # [T, E] bf16
    w13: tuple               # planes [E, 2I, ...] of format f13
    w2: tuple                # planes [E, H, ...] of format f2
    ids: torch.Tensor        # [T, k] int64, the stable-sort routing
    counts: torch.Tensor     # [E] list lengths
    want: torch.Tensor       # [T, H] fp64


def _stack_dims(which, E, H, I):
    return (E, 2 * I, H, I) if which == "w13" else (E, H, I, H)


@functools.lru_cache(maxsize=None)
def stack_planes(fmt, which, E, H, I):
    """Planes [E, rows, ...] of stack `which` ("w13" / "w2") in `fmt`."""
    E, rows, K, half = _stack_dims(which, E, H, I)
    g = torch.Generator().manual_seed(
        7 * E + 13 * H + I + (5 if fmt == "q6_k" else 0)
        + (101 if which == "w2" else 0))
    w = torch.randn(E, rows, K, generator=g)
    n = torch.arange(rows) % half + (torch.arange(rows) >= half).long()
    sign = 1.0 - 2.0 * ((torch.arange(E)[:, None, None] + n[None, :, None]
                         + torch.arange(K // 32)[None, None, :]) % 2)
    w = (w.view(E, rows, K // 32, 32) + 0.5 * sign[..., None]) \
        .reshape(E, rows, K)
    run = 32 if fmt == "q4_k" else 16
    e = (n[:, None] + torch.arange(K // run)[None, :]) % 3
    w = (w.view(E, rows, K // run, run) * (2.0 ** e.float())[None, :, :, None]
         ).reshape(E, rows, K) / K ** 0.5
    if which == "w2":
        w[:, :, -256:] *= 4.0
    planes = ops.quantize_kq(w.view(E * rows, K), fmt)
    return tuple(p.view(E, rows, *p.shape[1:]) for p in planes)


def planes(f13, f2, E, H, I):
    return stack_planes(f13, "w13", E, H, I), stack_planes(f2, "w2", E, H, I)


# -- dequantisers: the right one and one deliberate error each -------------

W_MUTANTS_Q4 = ("q4k_min_dropped", "q4k_d_dmin_swapped")
W_MUTANTS_Q6 = ("q6k_high_bits_dropped", "q6k_offset_31")
MUTANTS = W_MUTANTS_Q4 + W_MUTANTS_Q6 + (
    "scale_next_subblock", "gate_up_headers_swapped", "expert_plus1",
    "drop_last_superblock_down", "nibble_groups_swapped")


def _swap_halves(t):
    h = t.shape[1] // 2
    return torch.cat([t[:, h:], t[:, :h]], dim=1)


def _roll_flat(t):
    """The value one past the right one in the flat plane."""
    return t.reshape(-1).roll(-1).reshape(t.shape)


def dequant_stack(stack, fmt, mutant=None, gated=False):
    """fp64 [E, rows, K] of a stack, exact. `mutant` names one deliberate
    decoding error; one that belongs to the other format or (the header swap)
    to the other stack is ignored."""
    swap = mutant == "gate_up_headers_swapped" and gated
    if fmt == "q4_k":
        qs, hdr = stack
        E, rows, nb = hdr.shape[:3]
        if swap:
            hdr = _swap_halves(hdr)
        d = hdr[..., 0:2].contiguous().view(torch.float16).double()
        dmin = hdr[..., 2:4].contiguous().view(torch.float16).double()
        if mutant == "q4k_d_dmin_swapped":
            d, dmin = dmin, d
        s = hdr[..., 4:16].to(torch.int32)
        sc = torch.cat([s[..., 0:4] & 63,
                        (s[..., 8:12] & 0xF) | ((s[..., 0:4] >> 6) << 4)], -1)
        m = torch.cat([s[..., 4:8] & 63,
                       (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], -1)
        ds, dm = d * sc.double(), dmin * m.double()          # [E, rows, nb, 8]
        if mutant == "scale_next_subblock":
            ds, dm = _roll_flat(ds), _roll_flat(dm)
        if mutant == "q4k_min_dropped":
            dm = torch.zeros_like(dm)
        b = qs.reshape(E, rows, nb, 4, 1, 32)
        lo, hi = b & 0x0F, b >> 4
        if mutant == "nibble_groups_swapped":
            lo, hi = hi, lo
        nib = torch.cat([lo, hi], dim=4).reshape(E, rows, nb, 8, 32)
        y = ds[..., None] * nib.double() - dm[..., None]
    else:
        ql, qh, sc, d = stack
        E, rows, nb = d.shape
        if swap:
            sc, d = _swap_halves(sc), _swap_halves(d)
        b = ql.reshape(E, rows, nb, 2, 2, 32)                 # half, g&1, l
        lo, hi = b & 0x0F, b >> 4
        if mutant == "nibble_groups_swapped":
            lo, hi = hi, lo
        low = torch.cat([lo, hi], dim=4)                      # half, g, l
        h = qh.reshape(E, rows, nb, 2, 1, 32)
        shift = torch.tensor([0, 2, 4, 6], dtype=torch.uint8).view(4, 1)
        high = (h >> shift) & 3
        if mutant == "q6k_high_bits_dropped":
            high = torch.zeros_like(high)
        off = 31 if mutant == "q6k_offset_31" else 32
        q = (low | (high << 4)).to(torch.int32) - off         # [E,rows,nb,2,4,32]
        scf = sc.reshape(E, rows, nb, 16).double()
        if mutant == "scale_next_subblock":
            scf = _roll_flat(scf)
        s = (d.double().reshape(E, rows, nb, 1) * scf) \
            .reshape(E, rows, nb, 2, 4, 2, 1)                 # 8h + 2g + l/16
        y = s * q.reshape(E, rows, nb, 2, 4, 2, 16).double()
    w = y.reshape(E, rows, -1)
    if mutant == "expert_plus1":
        w = w.roll(-1, dims=0)
    return w


# one shape's weights at a time: the cases of a shape follow each other, a
# deep stack is 9 M elements, and there are eleven versions of it
@functools.lru_cache(maxsize=24)
def _stack_as(fmt, which, E, H, I, dtype, rounded, mutant):
    w = dequant_stack(stack_planes(fmt, which, E, H, I), fmt, mutant,
                      gated=which == "w13")
    if rounded:
        w = w.float().to(torch.bfloat16)
    return w.to(dtype)


def _stack_mutant(fmt, mutant):
    """What of `mutant` a stack of format `fmt` sees."""
    if mutant in W_MUTANTS_Q4 and fmt != "q4_k":
        return None
    if mutant in W_MUTANTS_Q6 and fmt != "q6_k":
        return None
    return None if mutant == "drop_last_superblock_down" else mutant


def mutant_applies(name: str, case: Case) -> bool:
    if name in W_MUTANTS_Q4:
        return "q4_k" in case.fmt
    if name in W_MUTANTS_Q6:
        return "q6_k" in case.fmt
    return True


def forward(case: Case, x, logits, dtype, rounded, mutant=None):
    """moe_forward_kq in `dtype`. rounded: round where the kernels round
    (weights to fp32 then bf16, act to bf16, ypair kept in `dtype` = fp32,
    out to bf16). mutant: one deliberate error."""
    E, k, H, I = case.E, case.k, case.H, case.I
    T = x.shape[0]
    w13d = _stack_as(case.f13, "w13", E, H, I, dtype, rounded,
                     _stack_mutant(case.f13, mutant))
    w2d = _stack_as(case.f2, "w2", E, H, I, dtype, rounded,
                    _stack_mutant(case.f2, mutant))
    ids, w = route_ref(logits, k, dtype)
    lists = align_ref(ids, E)
    xd = x.to(dtype)
    wflat = w.reshape(-1)
    ypair = torch.zeros(T * k, H, dtype=dtype)
    for e, p in enumerate(lists):
        if p.numel() == 0:
            continue
        gu = xd[p // k] @ w13d[e].t()
        act = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
        if rounded:
            act = act.to(torch.bfloat16).to(dtype)
        if mutant == "drop_last_superblock_down":
            act = act.clone()
            act[:, -256:] = 0
        ypair[p] = (act @ w2d[e].t()) * wflat[p, None]
    y = ypair.view(T, k, H)
    out = torch.zeros(T, H, dtype=dtype)
    for j in range(k):
        out = out + y[:, j]
    return out.to(torch.bfloat16) if rounded else out


def emulate(case: Case, b: Built, mutant=None):
    return forward(case, b.x, b.logits, torch.float32, True, mutant)


@functools.lru_cache(maxsize=None)
def inputs(E, k, H, T, family):
    """(x, logits, ids, counts): shared by the format pairs and by the shapes
    that differ in I alone."""
    g = torch.Generator().manual_seed(
        1013 * T + 29 * E + H + 100003 * FAMILIES.index(family))
    x = (torch.randn(T, H, generator=g) + 1.0).to(torch.bfloat16)
    logits, _ = make_logits(E, k, T, family, g)
    ids, _ = route_ref(logits, k)
    counts = torch.bincount(ids.reshape(-1), minlength=E)
    assert int(counts.sum()) == T * k
    return x, logits, ids, counts


@functools.lru_cache(maxsize=None)
def build(case: Case) -> Built:
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    p13, p2 = planes(case.f13, case.f2, E, H, I)
    x, logits, ids, counts = inputs(E, k, H, T, case.family)
    want = forward(case, x, logits, torch.float64, False)
    return Built(x, logits, p13, p2, ids, counts, want)


def mutant_outputs(case: Case, b: Built):
    return {m: emulate(case, b, m) for m in MUTANTS
            if mutant_applies(m, case)}


def dense_stack(fmt, which, E, H, I):
    """bf16 [E, rows, K]: what the kernels dequantise the stack to."""
    return _stack_as(fmt, which, E, H, I, torch.bfloat16, True, None)
