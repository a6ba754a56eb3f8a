"""Shared inputs, fp64 oracle, rounding emulation, mutants and metric for
the mixture-of-experts tests (test_moe_cpu.py, test_moe_gpu.py).

Every GPU oracle case is built here, on the CPU, from a seed, so that the
CPU file can show on the very same inputs that the emulation of the
kernels' rounding passes and that each mutant fails. The metric and the
assertion are wq_oracle's.

Router logits are a per-token permuted ladder: the expert of rank r gets
base_t - 0.25 r (exact in bf16), so the builder decides every list. The
oracle and the code under test take the same logits tensor and the same tie
rule (stable descending sort: equal logits go to the lower expert), so no
case needs a routing-margin exclusion.
"""
import functools
from dataclasses import dataclass

import torch

from wq_oracle import assert_wq_close, wq_error  # noqa: F401

# tol = 4 x the worst error of the rounding emulation against the fp64 oracle
# over all cases (test_moe_cpu.py::test_tolerance re-derives it and prints
# both numbers; docs/KERNELS.md records them).
TOL_MOE = 0.0242

# (E, k, H, I). (8, 2, 160, 96): K is no multiple of a wave's 128-element
# step in either GEMM. The last three are the deep ones: at H = 2080 the
# gated GEMM takes its 8-wave kernel, at I = 2080 and 4128 the down GEMM its
# 8- and 16-wave ones; everything else runs 4 waves. Three small shapes
# instead of one with every depth, whose weights would be 100 M elements.
SHAPES = ((8, 2, 256, 256), (8, 2, 160, 96), (4, 1, 256, 256),
          (64, 8, 256, 64), (4, 2, 2080, 32), (4, 2, 32, 2080),
          (4, 2, 32, 4128))
TS = (1, 2, 15, 16, 17, 64, 65, 130)
FAMILIES = ("uniform", "skewed", "sparse", "tied")
STEP = 0.25                   # ladder spacing
SKEW_EXPERT = 1               # every token's first choice in `skewed`


@dataclass(frozen=True)
class Case:
    E: int
    k: int
    H: int
    I: int
    T: int
    family: str

    @property
    def id(self):
        return f"E{self.E}k{self.k}-H{self.H}-I{self.I}-T{self.T}-{self.family}"


CASES = [Case(E, k, H, I, T, fam) for (E, k, H, I) in SHAPES for T in TS
         for fam in FAMILIES]


@dataclass
class Built:
    x: torch.Tensor          # [T, H] bf16
    logits: torch.Tensor     # [T, E] bf16
    w13: torch.Tensor        # [E, 2I, H] bf16
    w2: torch.Tensor         # [E, H, I] bf16
    ids: torch.Tensor        # [T, k] int64, the stable-sort routing
    counts: torch.Tensor     # [E] list lengths
    want: torch.Tensor       # [T, H] fp64


@functools.lru_cache(maxsize=None)
def weights(E, H, I):
    g = torch.Generator().manual_seed(7 * E + 13 * H + I)
    w13 = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    w2 = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(torch.bfloat16)
    return w13, w2


@functools.lru_cache(maxsize=None)
def _weights_as(E, H, I, dtype):
    w13, w2 = weights(E, H, I)
    return w13.to(dtype), w2.to(dtype)


def make_logits(E, k, T, family, g):
    """[T, E] bf16 ladder logits of the family, and the rank -> expert
    permutation [T, E] that produced them."""
    perm = torch.stack([torch.randperm(E, generator=g) for _ in range(T)])
    if family == "skewed":
        for t in range(T):
            j = int((perm[t] == SKEW_EXPERT).nonzero())
            perm[t, [0, j]] = perm[t, [j, 0]]
    elif family == "sparse":
        # the top k ranks come from the first max(k, E/2) experts only
        S = max(k, E // 2)
        for t in range(T):
            head = torch.randperm(S, generator=g)
            rest = [e for e in perm[t].tolist() if e >= S]
            perm[t] = torch.tensor(head.tolist() + rest)
    rank_val = -STEP * torch.arange(E, dtype=torch.float32)
    if family == "tied":
        # ranks k-1 .. k+1 share one value: a tie across the k-th place
        hi = min(k + 1, E - 1)
        rank_val[k - 1:hi + 1] = rank_val[k - 1]
    base = 0.5 * (torch.arange(T) % 5).float()
    logits = torch.empty(T, E)
    logits.scatter_(1, perm, (base[:, None] + rank_val[None, :]))
    lb = logits.to(torch.bfloat16)
    assert torch.equal(lb.float(), logits)        # the ladder is exact
    return lb, perm


def route_ref(logits, k, dtype=torch.float64, mutant=None):
    """Stable-sort routing. (ids [T, k] int64, w [T, k] dtype)."""
    lf = logits.to(dtype)
    order = torch.sort(lf, dim=-1, descending=True, stable=True).indices
    ids = order[:, :k].clone()
    if mutant == "kplus1_expert":
        ids[:, k - 1] = order[:, k]
    p = torch.softmax(lf, dim=-1).gather(-1, ids)
    w = p if mutant == "no_renorm" else p / p.sum(-1, keepdim=True)
    if mutant == "swap_w01":
        w = w.clone()
        w[:, [0, 1]] = w[:, [1, 0]]
    return ids, w


def align_ref(ids, E):
    """expert -> ascending pair indices."""
    flat = ids.reshape(-1)
    return [(flat == e).nonzero().flatten() for e in range(E)]


def forward(x, logits, w13, w2, k, dtype, rounded, mutant=None):
    """moe_forward in `dtype`. rounded: round where the kernels round (act
    to bf16, ypair kept in fp32, out to bf16). mutant: one deliberate error."""
    E, I2, H = w13.shape
    I = I2 // 2
    T = x.shape[0]
    if mutant == "zeros":
        return torch.zeros(T, H, dtype=torch.bfloat16 if rounded else dtype)
    ids, w = route_ref(logits, k, dtype, mutant)
    lists = align_ref(ids, E)
    if mutant == "drop_last_of_longest":
        e = max(range(E), key=lambda i: lists[i].numel())
        lists[e] = lists[e][:-1]
    elif mutant == "drop_past_64":
        lists = [p[:64] for p in lists]
    w13d, w2d = _weights_as(E, H, I, dtype)
    xd = x.to(dtype)
    wflat = w.reshape(-1)
    ypair = torch.zeros(T * k, H, dtype=dtype)
    for e, p in enumerate(lists):
        if p.numel() == 0:
            continue
        ee = (e + 1) % E if mutant == "expert_plus1" else e
        xs = xd[p // k]
        if mutant == "drop_last_k_gated":
            xs = xs.clone()
            xs[:, -32:] = 0
        gu = xs @ w13d[ee].t()
        gate, up = gu[:, :I], gu[:, I:]
        if mutant == "gate_up_swapped":
            gate, up = up, gate
        act = torch.nn.functional.silu(gate) * up
        if rounded:
            act = act.to(torch.bfloat16).to(dtype)
        if mutant == "drop_last_k_down":
            act = act.clone()
            act[:, -32:] = 0
        ypair[p] = (act @ w2d[ee].t()) * wflat[p, None]
    y = ypair.view(T, k, H)
    kk = k - 1 if mutant == "combine_omits_last" else k
    out = torch.zeros(T, H, dtype=dtype)
    for j in range(kk):
        out = out + y[:, j]
    return out.to(torch.bfloat16) if rounded else out


def oracle(b: Built, k):
    return forward(b.x, b.logits, b.w13, b.w2, k, torch.float64, False)


def emulate(b: Built, k, mutant=None):
    return forward(b.x, b.logits, b.w13, b.w2, k, torch.float32, True, mutant)


@functools.lru_cache(maxsize=None)
def build(case: Case) -> Built:
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    w13, w2 = weights(E, H, I)
    g = torch.Generator().manual_seed(
        1009 * T + 31 * E + H + I + 100003 * FAMILIES.index(case.family))
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    logits, perm = make_logits(E, k, T, case.family, g)
    ids, _ = route_ref(logits, k)
    counts = torch.bincount(ids.reshape(-1), minlength=E)
    # what the family promises
    assert int(counts.sum()) == T * k
    if case.family == "skewed":
        assert int(counts[SKEW_EXPERT]) == T
        assert torch.equal(ids[:, 0], torch.full((T,), SKEW_EXPERT))
    elif case.family == "sparse":
        assert int((counts == 0).sum()) * 2 >= E
    elif case.family == "tied":
        hi = min(k + 1, E - 1)
        group = perm[:, k - 1:hi + 1]
        assert group.shape[1] >= 2
        # slot k-1 went to the lowest expert index of the tied group
        assert torch.equal(ids[:, k - 1], group.min(dim=1).values)
        assert torch.equal(ids[:, :k - 1], perm[:, :k - 1])
    else:
        assert torch.equal(ids, perm[:, :k])
    b = Built(x, logits, w13, w2, ids, counts, None)
    b.want = oracle(b, k)
    return b


# -- mutants --------------------------------------------------------------

MUTANTS = ("expert_plus1", "no_renorm", "swap_w01", "drop_last_of_longest",
           "drop_past_64", "gate_up_swapped", "drop_last_k_gated",
           "drop_last_k_down", "kplus1_expert", "combine_omits_last", "zeros")


def mutant_applies(name: str, case: Case, b: Built) -> bool:
    if name == "swap_w01":
        return case.k >= 2
    if name == "drop_past_64":
        return int(b.counts.max()) > 64
    if name == "kplus1_expert":
        return case.E > case.k
    return True


def mutant_outputs(case: Case, b: Built):
    return {m: emulate(b, case.k, m) for m in MUTANTS
            if mutant_applies(m, case, b)}
