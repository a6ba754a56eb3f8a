"""Shared inputs, fp64 oracle, rounding emulation, mutants and metric for
the Q4_0/Q8_0 weight-only GEMM tests (test_wq_cpu.py, test_wq_gpu.py).

Every GPU oracle case is built here, on the CPU, from a seed, so that the
CPU file can show on the very same inputs that the emulation of the
kernel's rounding passes and that each mutant fails.
"""
import functools
import math
from dataclasses import dataclass

import torch

import helix_amd.ops as ops

# tol = 4 x the worst error of the rounding emulation against the fp64 oracle
# over all cases (test_wq_cpu.py::test_tolerance re-derives it and prints
# both numbers; docs/KERNELS.md records them). The factor 4 is the margin
# the attention tests give for accumulation order.
TOL_WQ = 0.027

FMTS = ("q4_0", "q8_0")
MS = (1, 2, 15, 16, 17, 33, 64)
# K = 160 and 4128 are no multiple of a wave's K stride, N = 48 is no
# multiple of a 4-channel-tile workgroup; (32, 2080) is added because the
# three K-split factors of the kernel (4, 8, 16 waves, chosen from the
# weight's shape) are 4 for the first three shapes, 16 for K = 4128, 8 here.
NKS = ((16, 32), (48, 160), (512, 256), (256, 4096 + 32), (32, 2048 + 32))
FAMILIES = ("needle", "randn")
FALLBACK_MS = (ops.WQ_FUSED_MAX_M + 1, 128)


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
FALLBACK_CASES = [Case(f, m, 48, 160, b, "needle") for f in FMTS
                  for m in FALLBACK_MS for b in (False, True)]


@dataclass
class Built:
    x: torch.Tensor          # [M, K] bf16
    qs: torch.Tensor
    d: torch.Tensor
    bias: torch.Tensor       # [N] bf16 or None
    want: torch.Tensor       # [M, N] fp64


@functools.lru_cache(maxsize=None)
def _weight(fmt, N, K, family):
    g = torch.Generator().manual_seed(1000 * N + K + (7 if fmt == "q8_0" else 0))
    w = torch.randn(N, K, generator=g)
    if family == "needle":
        # neighbouring blocks and neighbouring rows differ by at least 2x in
        # scale, so a scale taken from the wrong block shows
        nblk = K // 32
        e = (torch.arange(N)[:, None] + 3 * torch.arange(nblk)[None, :]) % 7
        w = (w.view(N, nblk, 32) * (2.0 ** e.float())[..., None] * 0.01)
        w = w.reshape(N, K)
    qs, d = ops.quantize_wq(w, fmt)
    return qs, d


@functools.lru_cache(maxsize=None)
def build(case: Case) -> Built:
    qs, d = _weight(case.fmt, case.N, case.K, case.family)
    g = torch.Generator().manual_seed(case.M * 131 + case.K)
    x = torch.randn(case.M, case.K, generator=g)
    if case.family == "needle":
        # one dominant activation per token, in the LAST K block and at a
        # position that walks over all 32 slots of it
        m = torch.arange(case.M)
        x[m, case.K - 1 - (m % 32)] = 24.0
    else:
        # unit mean: a constant added to every weight of a block (the
        # offset-7 mutant) is invisible to a token whose activations sum to 0
        x = x + 1.0
    x = x.to(torch.bfloat16)
    bias = None
    if case.bias:
        bias = torch.randn(case.N, generator=g).to(torch.bfloat16)
    want = oracle(x, ops.dequantize_wq(qs, d, case.fmt), bias)
    return Built(x, qs, d, bias, want)


def oracle(x, w32, bias):
    out = x.double() @ w32.double().t()
    if bias is not None:
        out = out + bias.double()
    return out


def emulate(x, w32, bias):
    """Round where the kernels round: weight to bf16, fp32 accumulate,
    fp32 bias add, bf16 out."""
    out = x.float() @ w32.to(torch.bfloat16).float().t()
    if bias is not None:
        out = out + bias.float()
    return out.to(torch.bfloat16)


# -- mutants: a dequantizer with one deliberate error --------------------

def _planes(qs, d, fmt):
    N, nblk = d.shape
    if fmt == "q4_0":
        b = qs.reshape(N, nblk, 16)
        return b & 0x0F, b >> 4
    return qs.reshape(N, nblk, 32), None


def mutant_weights(qs, d, fmt):
    """{name: fp32 [N, K] weight a broken kernel would have used}."""
    N, nblk = d.shape
    df = d.float()[..., None]
    good = ops.dequantize_wq(qs, d, fmt)
    out = {}
    if fmt == "q4_0":
        lo, hi = _planes(qs, d, fmt)
        out["nibbles_swapped"] = (
            df * (torch.cat([hi, lo], -1).float() - 8)).reshape(N, -1)
        out["offset_7"] = (
            df * (torch.cat([lo, hi], -1).float() - 7)).reshape(N, -1)
        q = torch.cat([lo, hi], -1).float() - 8
    else:
        q8, _ = _planes(qs, d, fmt)
        q = q8.float()
        out["q8_unsigned"] = (
            df * q8.view(torch.uint8).float()).reshape(N, -1)
    # the scale one past the right one in the flat [N, K/32] plane
    nxt = d.float().reshape(-1).roll(-1).reshape(N, nblk)[..., None]
    out["scale_next_block"] = (nxt * q).reshape(N, -1)
    as_bf16 = d.view(torch.bfloat16).float()[..., None]
    out["scale_as_bf16"] = (as_bf16 * q).reshape(N, -1)
    w = good.clone()
    w[:, -32:] = 0
    out["drop_last_k_block"] = w
    w = good.clone()
    w[-16:] = 0
    out["drop_last_channel_tile"] = w
    return out


MUTANTS_Q4 = {"nibbles_swapped", "offset_7", "scale_next_block",
              "scale_as_bf16", "drop_last_k_block", "drop_last_channel_tile",
              "zeros"}
MUTANTS_Q8 = {"q8_unsigned", "scale_next_block", "scale_as_bf16",
              "drop_last_k_block", "drop_last_channel_tile", "zeros"}


def mutant_outputs(case: Case, b: Built):
    outs = {}
    for name, w in mutant_weights(b.qs, b.d, case.fmt).items():
        bias = b.bias
        if name == "drop_last_channel_tile" and bias is not None:
            bias = bias.clone()
            bias[-16:] = 0              # the tile is not written at all
        outs[name] = emulate(b.x, w, bias)
    outs["zeros"] = torch.zeros_like(outs["scale_as_bf16"])
    return outs


# -- metric ---------------------------------------------------------------

def wq_error(got, want64):
    """Per output row: max of |got-want|_2 / |want|_2 and
    max|got-want| / max|want|. Returns a [M] fp64 tensor."""
    g = got.detach().double().cpu()
    diff = g - want64
    l2 = diff.norm(dim=-1) / want64.norm(dim=-1)
    mx = diff.abs().amax(-1) / want64.abs().amax(-1)
    err = torch.maximum(l2, mx)
    return torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)


def assert_wq_close(got, want64, tol, what=""):
    assert tuple(got.shape) == tuple(want64.shape), (got.shape, want64.shape)
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    err = wq_error(got, want64)
    worst = float(err.max())
    if worst <= tol:
        return worst
    row = int(err.argmax())
    dd = (got.detach().double().cpu() - want64)[row].abs()
    pos = int(dd.argmax())
    raise AssertionError(
        f"{what}: error {worst:.4g} > tol {tol:.4g} at row {row} (worst "
        f"channel {pos}: got {float(got[row, pos]):.6g}, want "
        f"{float(want64[row, pos]):.6g}); {int((err > tol).sum())} of "
        f"{err.numel()} rows fail")
