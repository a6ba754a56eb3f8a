"""Shared inputs, fp64 oracle, rounding emulation, mutants and metric for
the QK-norm + rope tests (test_qknorm_cpu.py, test_qknorm_gpu.py).

Every GPU oracle case is built here, on the CPU, from a seed, so that the
CPU file can show on the very same inputs that the emulation of the kernel's
rounding passes and that each mutant fails. The metric and the assertion are
wq_oracle's, applied per head row: q is judged as [T*Hq, D], k as [T*Hkv, D].

The fp32 cos/sin table is an input of the kernel, so the oracle takes the
table's values (widened to fp64), not cosines of its own.

Norm weights are drawn in [0.5, 1.5], separately for Q and for K, never ones:
with unit weights norm-before-rope and norm-after-rope are the same function
(a rotation keeps the norm), and Q's and K's weights could be swapped unseen.
"""
import functools
from dataclasses import dataclass

import torch

from helix_amd.ops.reference import make_cos_sin_cache
from wq_oracle import assert_wq_close, wq_error  # noqa: F401

# tol = 4 x the worst error of the rounding emulation against the fp64 oracle
# over all cases (test_qknorm_cpu.py::test_tolerance re-derives both and
# prints the numbers; docs/KERNELS.md records them). The emulation rounds
# once, to bf16; for the e4m3 K cache once, to fp8.
TOL_QKNORM = 0.0155
TOL_QKNORM_FP8 = 0.2353

EPS = 1e-6                    # Qwen3's rms_norm_eps
MAX_POS = 40960               # Qwen3's max_position
ROPE_BASE = 1e6
BLOCK = 16                    # paged-cache block size

# (Hq, Hkv, D): the two tiny presets' heads, a head count that is no multiple
# of the four waves, and qwen3-8b's
SHAPES = ((4, 2, 128), (8, 2, 64), (5, 1, 128), (32, 8, 128))
TS = (1, 3, 17, 130)
# small: rows scaled by 1e-3, so mean(x^2) ~ eps: the only family that sees
# eps. outlier: element OUT_COL of every head x 40, so one element carries
# most of a head's mean square and the heads' means differ widely.
FAMILIES = ("randn", "small", "outlier")
OUT_COL = 5


@dataclass(frozen=True)
class Case:
    Hq: int
    Hkv: int
    D: int
    T: int
    family: str

    @property
    def id(self):
        return f"q{self.Hq}kv{self.Hkv}-D{self.D}-T{self.T}-{self.family}"

    @property
    def width(self):
        return (self.Hq + 2 * self.Hkv) * self.D


CASES = [Case(Hq, Hkv, D, T, fam) for (Hq, Hkv, D) in SHAPES for T in TS
         for fam in FAMILIES]


@dataclass
class Built:
    qkv: torch.Tensor         # [T, width] bf16
    wq: torch.Tensor          # [D] bf16
    wk: torch.Tensor          # [D] bf16
    positions: torch.Tensor   # [T] int64, non-monotonic, up to MAX_POS - 1
    slots: torch.Tensor       # [T] int64, distinct, some -1
    nblocks: int
    want_q: torch.Tensor      # [T*Hq, D] fp64
    want_k: torch.Tensor      # [T*Hkv, D] fp64


@functools.lru_cache(maxsize=None)
def cos_sin(D):
    """The model's table for head_dim D: [MAX_POS, D] fp32."""
    return make_cos_sin_cache(D, MAX_POS, ROPE_BASE)


def norm_weights(D):
    g = torch.Generator().manual_seed(977 + D)
    wq = (0.5 + torch.rand(D, generator=g)).to(torch.bfloat16)
    wk = (0.5 + torch.rand(D, generator=g)).to(torch.bfloat16)
    assert not torch.equal(wq, wk)
    return wq, wk


def _rope(y, cs, D, dtype):
    """y [T, H, D], cs [T, D] table rows."""
    half = D // 2
    c = cs[:, None, :half].to(dtype)
    s = cs[:, None, half:].to(dtype)
    y1, y2 = y[..., :half], y[..., half:]
    return torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], dim=-1)


def _norm(x, w, eps, dtype, mutant):
    """x [T, H, D] in dtype."""
    if mutant == "no_norm":
        return x
    if mutant == "mean_all_heads":
        var = x.pow(2).mean(dim=(-2, -1), keepdim=True)
    else:
        var = x.pow(2).mean(-1, keepdim=True)
    if mutant == "eps0":
        eps = 0.0
    elif mutant == "eps1e-5":
        eps = 1e-5
    y = x * torch.rsqrt(var + eps)
    return y if mutant == "no_weight" else y * w.to(dtype)


def forward(qkv, wq, wk, positions, case, dtype, mutant=None, eps=EPS):
    """(q [T*Hq, D], k [T*Hkv, D]) in `dtype`, unrounded."""
    Hq, Hkv, D, T = case.Hq, case.Hkv, case.D, qkv.shape[0]
    cs = cos_sin(D)[positions]
    x = qkv.to(dtype)
    q = x[:, :Hq * D].reshape(T, Hq, D)
    k = x[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)
    wq_used = wk if mutant == "k_weight_on_q" else wq
    if mutant == "norm_after_rope":
        q = _norm(_rope(q, cs, D, dtype), wq_used, eps, dtype, None)
        k = _norm(_rope(k, cs, D, dtype), wk, eps, dtype, None)
    else:
        q = _rope(_norm(q, wq_used, eps, dtype, mutant), cs, D, dtype)
        k = _rope(_norm(k, wk, eps, dtype, mutant), cs, D, dtype)
    return q.reshape(T * Hq, D), k.reshape(T * Hkv, D)


def oracle(b: Built, case):
    return forward(b.qkv, b.wq, b.wk, b.positions, case, torch.float64)


def fp8_round(t):
    """fp32 -> OCP e4m3 -> fp32 (one rounding, as the kernel's cache write)."""
    return t.float().to(torch.float8_e4m3fn).float()


def emulate(b: Built, case, mutant=None):
    """fp32 from the load to one rounding. (q bf16, k bf16, k e4m3-as-fp32)."""
    q, k = forward(b.qkv, b.wq, b.wk, b.positions, case, torch.float32, mutant)
    return q.to(torch.bfloat16), k.to(torch.bfloat16), fp8_round(k)


def emulate_hf(b: Built, case):
    """HF's order: round to bf16 after the norm, after the weight and after
    the rope. Reported next to the emulation; not what the kernel does."""
    Hq, Hkv, D, T = case.Hq, case.Hkv, case.D, b.qkv.shape[0]
    cs = cos_sin(D)[b.positions]
    outs = []
    for lo, H, w in ((0, Hq, b.wq), (Hq * D, Hkv, b.wk)):
        x = b.qkv[:, lo:lo + H * D].reshape(T, H, D).float()
        y = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)) \
            .to(torch.bfloat16)
        y = (w * y).float()
        outs.append(_rope(y, cs, D, torch.float32).to(torch.bfloat16)
                    .reshape(T * H, D))
    return outs


def make_qkv(case: Case, g):
    x = torch.randn(case.T, case.width, generator=g)
    if case.family == "small":
        x = x * 1e-3
    elif case.family == "outlier":
        x.view(case.T, -1, case.D)[:, :, OUT_COL] *= 40.0
    return x.to(torch.bfloat16)


def make_positions(T, g):
    pos = torch.randint(0, MAX_POS, (T,), generator=g, dtype=torch.int64)
    pos[0] = MAX_POS - 1
    if T > 1:
        pos[-1] = 0
    if T > 2:
        pos[1] = 1
        assert not torch.equal(pos, pos.sort().values)
    return pos


def make_slots(T, g):
    """Distinct slots scattered over the blocks; every third row of T >= 3
    is a pad row (slot -1). Returns (slots, nblocks)."""
    nblocks = (T + BLOCK - 1) // BLOCK + 2
    slots = torch.randperm(nblocks * BLOCK, generator=g)[:T].to(torch.int64)
    if T >= 3:
        slots[1::3] = -1
    return slots, nblocks


@functools.lru_cache(maxsize=None)
def build(case: Case) -> Built:
    g = torch.Generator().manual_seed(
        1009 * case.T + 31 * case.Hq + 7 * case.Hkv + case.D
        + 100003 * FAMILIES.index(case.family))
    qkv = make_qkv(case, g)
    wq, wk = norm_weights(case.D)
    pos = make_positions(case.T, g)
    slots, nblocks = make_slots(case.T, g)
    b = Built(qkv, wq, wk, pos, slots, nblocks, None, None)
    b.want_q, b.want_k = oracle(b, case)
    if case.family == "small":
        # what the family promises: eps matters
        ms = qkv.float().view(case.T, -1, case.D).pow(2).mean(-1)
        assert 0.2 * EPS < float(ms.median()) < 5 * EPS
    return b


# -- mutants --------------------------------------------------------------

MUTANTS = ("no_norm", "no_weight", "k_weight_on_q", "norm_after_rope",
           "eps0", "eps1e-5", "mean_all_heads")


def mutant_error(case: Case, b: Built, name: str) -> float:
    """Worst head-row error of the mutant's bf16 outputs, over q and k."""
    q, k, _ = emulate(b, case, name)
    return max(float(wq_error(q, b.want_q).max()),
               float(wq_error(k, b.want_k).max()))


def written_rows(b: Built):
    """Token rows with a cache slot, and their (block, offset)."""
    rows = (b.slots >= 0).nonzero().flatten()
    s = b.slots[rows]
    return rows, s // BLOCK, s % BLOCK
