"""Shared inputs, fp64 oracle, rounding emulation, mutants and metric for
the quantised mixture-of-experts tests (test_moe_wq_cpu.py,
test_moe_wq_gpu.py).

moe_oracle's shapes, routing families, ladder logits and metric; the expert
weights are randn with a per-block power-of-two pattern, quantised by
ops.quantize_wq. The fp64 oracle runs on the EXACTLY dequantised weights
(d * q is exact in fp32), so quantisation error is not in the metric; the
emulation rounds where the kernels round: d * q to bf16, fp32 accumulation,
act to bf16, ypair in fp32, out to bf16.

Weight pattern: block b of row n (n counted within the gate half and the up
half separately) is scaled by 2^((n + b + up) % 3), so neighbouring blocks,
neighbouring rows and a gate row and its up row never share a scale: a
scale from the wrong block or the wrong half shows. The last K block of the
down weights is four times larger again: with 129 blocks (I = 4128) a
dropped last block of plain randn weights is 1/129 of the energy, a 0.044
error next to a tolerance of 0.043.
x has mean 1: a constant added to every weight of a block (the offset-7
mutant) cannot hide behind activations that sum to zero.
"""
import functools
from dataclasses import dataclass

import torch

import helix_amd.ops as ops
from moe_oracle import (FAMILIES, SHAPES, align_ref, make_logits,  # noqa: F401
                        route_ref)
from wq_oracle import assert_wq_close, wq_error  # noqa: F401

# tol = 4 x the worst error of the rounding emulation against the fp64 oracle
# over all cases (test_moe_wq_cpu.py::test_tolerance re-derives it and prints
# both numbers; docs/KERNELS.md records them).
TOL_MOE_WQ = 0.0428

FMTS = ("q4_0", "q8_0")
TS = (1, 16, 17, 65, 130)


@dataclass(frozen=True)
class Case:
    fmt: str
    E: int
    k: int
    H: int
    I: int
    T: int
    family: str

    @property
    def id(self):
        return (f"{self.fmt}-E{self.E}k{self.k}-H{self.H}-I{self.I}-"
                f"T{self.T}-{self.family}")


CASES = [Case(f, E, k, H, I, T, fam) for f in FMTS for (E, k, H, I) in SHAPES
         for T in TS for fam in FAMILIES]


@dataclass
class Built:
    x: torch.Tensor          # [T, H] bf16
    logits: torch.Tensor     # [T, E] bf16
    w13: tuple               # (qs [E, 2I, ...], d [E, 2I, H/32])
    w2: tuple                # (qs [E, H, ...], d [E, H, I/32])
    ids: torch.Tensor        # [T, k] int64, the stable-sort routing
    counts: torch.Tensor     # [E] list lengths
    want: torch.Tensor       # [T, H] fp64


def _pattern(E, rows, K, half):
    n = torch.arange(rows) % half + (torch.arange(rows) >= half).long()
    e = (n[:, None] + torch.arange(K // 32)[None, :]) % 3
    return (2.0 ** e.float())[None, :, :, None].expand(E, rows, K // 32, 1)


@functools.lru_cache(maxsize=None)
def planes(fmt, E, H, I):
    """((w13_qs, w13_d), (w2_qs, w2_d)) of the shape's quantised experts."""
    g = torch.Generator().manual_seed(7 * E + 13 * H + I
                                      + (5 if fmt == "q8_0" else 0))
    w13 = torch.randn(E, 2 * I, H, generator=g) / H ** 0.5
    w2 = torch.randn(E, H, I, generator=g) / I ** 0.5
    w13 = (w13.view(E, 2 * I, H // 32, 32) * _pattern(E, 2 * I, H, I)) \
        .reshape(E, 2 * I, H)
    w2 = (w2.view(E, H, I // 32, 32) * _pattern(E, H, I, H)).reshape(E, H, I)
    w2[:, :, -32:] *= 4.0
    out = []
    for w in (w13, w2):
        e, rows, K = w.shape
        qs, d = ops.quantize_wq(w.view(e * rows, K), fmt)
        out.append((qs.view(e, rows, -1), d.view(e, rows, K // 32)))
    return tuple(out)


# -- dequantisers: the right one and one deliberate error each -------------

W_MUTANTS_Q4 = ("nibbles_swapped", "offset_7")
W_MUTANTS_Q8 = ("q8_unsigned",)
MUTANTS = W_MUTANTS_Q4 + W_MUTANTS_Q8 + (
    "scale_next_block", "expert_plus1", "gate_up_scales_swapped",
    "drop_last_k_down")


def dequant_stack(qs, d, fmt, mutant=None, gated=False):
    """fp32 [E, rows, K] of a stack, exact (d * q is exact in fp32)."""
    E, rows, nblk = d.shape
    df = d.float()
    if mutant == "scale_next_block":
        # the scale one past the right one in the flat plane
        df = df.reshape(-1).roll(-1).reshape(E, rows, nblk)
    elif mutant == "gate_up_scales_swapped" and gated:
        df = torch.cat([df[:, rows // 2:], df[:, :rows // 2]], dim=1)
    if fmt == "q4_0":
        b = qs.reshape(E, rows, nblk, 16)
        lo, hi = b & 0x0F, b >> 4
        if mutant == "nibbles_swapped":
            lo, hi = hi, lo
        q = torch.cat([lo, hi], -1).float() - \
            (7.0 if mutant == "offset_7" else 8.0)
    else:
        q8 = qs.reshape(E, rows, nblk, 32)
        q = q8.view(torch.uint8).float() if mutant == "q8_unsigned" \
            else q8.float()
    w = (df[..., None] * q).reshape(E, rows, nblk * 32)
    if mutant == "expert_plus1":
        w = w.roll(-1, dims=0)
    return w


@functools.lru_cache(maxsize=None)
def _weights_as(fmt, E, H, I, dtype, rounded, mutant):
    p13, p2 = planes(fmt, E, H, I)
    out = []
    for (qs, d), gated in ((p13, True), (p2, False)):
        w = dequant_stack(qs, d, fmt, mutant, gated)
        if rounded:
            w = w.to(torch.bfloat16)
        out.append(w.to(dtype))
    return tuple(out)


def mutant_applies(name: str, case: Case) -> bool:
    if name in W_MUTANTS_Q4:
        return case.fmt == "q4_0"
    if name in W_MUTANTS_Q8:
        return case.fmt == "q8_0"
    return True


def forward(case: Case, x, logits, dtype, rounded, mutant=None):
    """moe_forward_wq in `dtype`. rounded: round where the kernels round
    (weights to bf16, act to bf16, ypair kept in `dtype` = fp32, out to
    bf16). mutant: one deliberate error."""
    E, k, H, I = case.E, case.k, case.H, case.I
    T = x.shape[0]
    wmut = mutant if mutant not in (None, "drop_last_k_down") else None
    w13d, w2d = _weights_as(case.fmt, E, H, I, dtype, rounded, wmut)
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
        if mutant == "drop_last_k_down":
            act = act.clone()
            act[:, -32:] = 0
        ypair[p] = (act @ w2d[e].t()) * wflat[p, None]
    y = ypair.view(T, k, H)
    out = torch.zeros(T, H, dtype=dtype)
    for j in range(k):
        out = out + y[:, j]
    return out.to(torch.bfloat16) if rounded else out


def emulate(case: Case, b: Built, mutant=None):
    return forward(case, b.x, b.logits, torch.float32, True, mutant)


@functools.lru_cache(maxsize=None)
def build(case: Case) -> Built:
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    p13, p2 = planes(case.fmt, E, H, I)
    g = torch.Generator().manual_seed(
        1013 * T + 29 * E + H + I + 100003 * FAMILIES.index(case.family))
    x = (torch.randn(T, H, generator=g) + 1.0).to(torch.bfloat16)
    logits, _ = make_logits(E, k, T, case.family, g)
    ids, _ = route_ref(logits, k)
    counts = torch.bincount(ids.reshape(-1), minlength=E)
    assert int(counts.sum()) == T * k
    want = forward(case, x, logits, torch.float64, False)
    return Built(x, logits, p13, p2, ids, counts, want)


def mutant_outputs(case: Case, b: Built):
    return {m: emulate(case, b, m) for m in MUTANTS
            if mutant_applies(m, case)}


def dense_weights(fmt, E, H, I):
    """bf16 (w13, w2): what the kernels dequantise to."""
    return _weights_as(fmt, E, H, I, torch.bfloat16, True, None)
