"""fp64 oracle, adversarial inputs and mutants for the two attention kernels.

Shared by tests/test_attn_oracle_cpu.py (proves on the CPU that every case
below can fail), tests/test_attn_gpu.py and tests/test_ops_gpu.py.

What is here
  * decode_ref64 / prefill_ref64: fp64 references with explicit masks
    (causal, window, ctx = klen - qlen, hkv = hq // G, block-table gather),
    written independently of helix_amd/ops/reference.py.
  * decode_emulation / prefill_emulation: CPU emulations that round where
    the kernels round: bf16 (or fp8) inputs, fp32 scores and accumulation,
    P rounded to bf16 before PV for prefill only, bf16 output.
  * assert_attn_close: for every (row, head),
        |got - want|_2 <= tol * |want|_2   and
        max|got - want| <= tol * max|want|.
  * build_decode / build_prefill: inputs of two families. "randn" is plain
    noise. "needle" puts loud keys on the edges the kernels can get wrong
    and loud, finite poison in every slot a row must not read.
  * decode_mutants / prefill_mutants: the reference with one deliberate
    error each.

How a needle is built.  Every q head h has a fixed unit direction u_h,
orthonormal within its kv group.  A query is q = c * u_h + r with r random
and orthogonal to the group's directions; a needle key of kv head j is
A * sum_g u_(j*G+g), the sum of the group's queries' shared parts.  Its
score is scale * A * c for every head of the group, independent of r, so c
plays the part of the per-head alpha: it is solved per (row, head) on the
fp64 softmax of the values as stored (bf16 or e4m3) so that the visible
needles together hold half of the mass.  The builder then asserts on the
fp64 softmax of the final tensors that each visible needle holds at least
NEEDLE_FLOOR = 5 % and all of them hold 30 % .. 70 %.  Rows that see too
few ordinary tokens for that (solved score below S_MIN) keep score S_MIN,
stay loud, and are left out of the assertion: a one-token row cannot keep
its only token under 70 %.  Needle values are randn like all others.
Poison keys are 2 * A * sum u, so they score twice a needle for every row
and head; poison values are +-64.  In prefill the keys 0 and 1 of every
sequence are needles, which makes them poison for the sequence before;
two poison rows follow the last sequence.

The floor is 5 % and not 8 * tol: with the tolerances measured below that
would be 12 % (decode) and 18 % (prefill), and the 10 edges a row of 5 or
more partitions has (0, 127, 128, len - 1, partition firsts and lasts)
could not share 70 %.  What the floor is for, that losing one needle
moves the output by far more than tol, is asserted directly: every
applicable mutant of every needle case errs by at least 4 * tol
(measured: at least 20 * tol).  At most 10 needles go into one softmax; a
decode row with more edges (5 to 8 split-K partitions) gives the first
tokens of its partitions to even kv heads and the last tokens to odd ones,
while 0, 127, 128, len - 1, kv_lo and kv_lo - 1 stay on every head.

The full-grid decode cases (B * Hkv = 2048) of one head size share their
ordinary K/V noise, and their mutants are applied to the first ten rows.

Tolerance (printed by `python -m tests.attn_oracle`; re-measured and
asserted by tests/test_attn_oracle_cpu.py::test_tolerances):
  worst emulation error vs fp64 over all cases, in the metric above
      decode  0.00389  (needle 0.00389, randn 0.00387; L = 1 .. 65 600,
                        D = 64 and 128, bf16 and fp8 caches)
      prefill 0.00575  (needle 0.00565, randn 0.00575)
  TOL_DECODE  = 4 * 0.00389 = 0.0156
  TOL_PREFILL = 4 * 0.00575 = 0.0231
  smallest mutant error: decode 0.350 (drop_last, [2048] at G = 8),
      prefill 0.478 (causal_plus_1, window 128 with cached prefix);
      a quarter of either is well above tol.
The decode figure is bf16's unit roundoff 2^-8 = 0.0039 on the output: the
max-norm half of the metric finds an element near the row's maximum that
sits at a rounding midpoint.  Its L2 half alone stays near 0.002.
Prefill adds the bf16 rounding of P, which is coherent over the D elements
of a needle's value row.  The factor 4 covers __expf and the accumulation
order (split-K, online softmax), which the emulation does not model.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import torch

import helix_amd.ops as ops

TOL_DECODE = 0.0156
TOL_PREFILL = 0.0231

# Geometry of the kernels under test (paged_attn_decode.hip,
# attn_prefill.hip); the needle positions and some mutants follow it.
CHUNK = 128
PART_QUANT = 128
MAX_PARTS = 512
TARGET_WGS = 1024
NTHREADS = 128
KTILE = 64

NEEDLE_MASS = 0.5
NEEDLE_FLOOR = 0.05    # least share of the softmax one visible needle holds
POOL_ROWS = 300_000
S_MIN = 2.0            # lowest needle score that keeps poison loud
MAX_NEEDLES = 10
POISON_V = 64.0


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------
# metric
# --------------------------------------------------------------------------

def attn_error(got, want64):
    """Per (row, head): max of the relative L2 error and of
    max|err| / max|want|. Returns a [rows, heads] fp64 tensor."""
    g = got.detach().double().cpu()
    w = want64.double()
    diff = g - w
    l2 = diff.norm(dim=-1) / w.norm(dim=-1)
    mx = diff.abs().amax(-1) / w.abs().amax(-1)
    err = torch.maximum(l2, mx)
    return torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)


def assert_attn_close(got, want64, tol, what=""):
    assert tuple(got.shape) == tuple(want64.shape), (got.shape, want64.shape)
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    err = attn_error(got, want64)
    worst = float(err.max())
    if worst <= tol:
        return worst
    row, head = divmod(int(err.argmax()), err.shape[1])
    d = (got.detach().double().cpu() - want64)[row, head].abs()
    pos = int(d.argmax())
    raise AssertionError(
        f"{what}: error {worst:.4g} > tol {tol:.4g} at row {row}, head "
        f"{head} (worst element {pos}: got "
        f"{float(got[row, head, pos]):.6g}, want "
        f"{float(want64[row, head, pos]):.6g}); "
        f"{int((err > tol).sum())} of {err.numel()} (row, head) pairs fail")


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------

@dataclass(frozen=True)
class DecodeCase:
    name: str
    d: int
    g: int
    lens: tuple
    hkv: int = 2
    kv8: bool = False
    window: int = 0
    bs: int = 16
    family: str = "needle"
    max_len: int = 0        # 0: max(lens), as ops.paged_attn_decode does
    ws_len: int = 0         # 0: workspace sized for max_len
    table_cols: int = 0     # 0: three more columns than the longest row
    tag: str = ""           # told apart in the id, same random inputs

    @property
    def id(self):
        return f"{self.name}{self.tag}-{self.family}"

    @property
    def seed_key(self):
        return f"{self.name}-{self.family}"


@dataclass(frozen=True)
class PrefillCase:
    name: str
    hq: int
    hkv: int
    d: int
    qlens: tuple
    klens: tuple = ()       # (): plain prefill, klens = qlens
    causal: bool = True
    window: int = 0
    max_seqlen: int = 0     # 0: max(qlens)
    family: str = "needle"

    @property
    def id(self):
        return f"{self.name}-{self.family}"

    seed_key = id


def _both(cases):
    out = []
    for c in cases:
        out.append(c)
        longest = max(c.lens) if isinstance(c, DecodeCase) else \
            max(c.klens or c.qlens)
        if longest <= 2048:
            out.append(type(c)(**{**c.__dict__, "family": "randn"}))
    return out


DG_PAIRS = [(d, g) for d in (64, 128) for g in (1, 2, 4, 8)]
FIVE = (1, 127, 128, 129, 300)


def _decode_cases():
    cs = []
    for d, g in DG_PAIRS:
        for kv8 in (False, True):
            cs.append(DecodeCase(f"pairs-d{d}-g{g}-{'fp8' if kv8 else 'bf16'}",
                                 d, g, FIVE, kv8=kv8))
    cs.append(DecodeCase("pairs-d128-g4-bf16-bs32", 128, 4, FIVE, bs=32))
    for d, g in DG_PAIRS:
        cs.append(DecodeCase(f"fullgrid-d{d}-g{g}", d, g,
                             tuple(FIVE[i % 5] for i in range(256)), hkv=8))
    for g in (1, 8):
        cs.append(DecodeCase(f"splitk-129-700-g{g}", 128, g, (129, 700)))
        cs.append(DecodeCase(f"splitk-2048-g{g}", 128, g, (2048,)))
    cs.append(DecodeCase("splitk-129-700-d64-g8", 64, 8, (129, 700)))
    cs.append(DecodeCase("splitk-multiples", 128, 4, (128, 256, 512)))
    cs.append(DecodeCase("splitk-cap-65600", 128, 1, (65600,), hkv=1))
    for kv8 in (False, True):
        t = "fp8" if kv8 else "bf16"
        for w in (1, 256, 300, 700, 4096):
            cs.append(DecodeCase(f"window{w}-700-{t}", 128, 4, (700,),
                                 kv8=kv8, window=w))
        cs.append(DecodeCase(f"window512-2048-{t}", 128, 4, (2048,),
                             kv8=kv8, window=512))
        cs.append(DecodeCase(f"window256-100-700-{t}", 128, 4, (100, 700),
                             kv8=kv8, window=256))
    return _both(cs)


def _engine_cases():
    """The engine's calling convention: a persistent workspace for 8 rows
    and 4096 tokens, three short rows, max_len rounded up to a bucket and
    block tables as wide as the longest sequence the model allows."""
    return [DecodeCase("engine", 128, 4, (1, 127, 300), max_len=m,
                       ws_len=4096, table_cols=4096 // 16 + 1,
                       tag=f"-maxlen{m}")
            for m in (512, 4096)]


def _prefill_cases():
    cs = []
    for hq, hkv, d in ((12, 12, 64), (8, 8, 128), (8, 2, 64)):
        cs.append(PrefillCase(f"noncausal-{hq}-{hkv}-{d}", hq, hkv, d,
                              (1, 63, 64, 65, 197), causal=False))
    edges = (15, 16, 17, 63, 64, 65, 129)
    for d in (128, 64):
        cs.append(PrefillCase(f"edges-d{d}", 8, 2, d, edges))
        cs.append(PrefillCase(f"edges-d{d}-maxseq512", 8, 2, d, edges,
                              max_seqlen=512))
    for w in (1, 24, 64, 65, 200):
        cs.append(PrefillCase(f"window{w}", 8, 2, 128, (200, 70), window=w))
    cs.append(PrefillCase("window24-d64", 8, 2, 64, (200, 70), window=24))
    for w in (24, 128):
        cs.append(PrefillCase(f"window{w}-prefix", 8, 2, 128, (7, 64, 1),
                              (200, 300, 130), window=w))
    for d in (128, 64):
        cs.append(PrefillCase(f"prefix-edges-d{d}", 8, 2, d, (1, 64, 65),
                              (64, 64, 193)))
    return _both(cs)


DECODE_CASES = _decode_cases()
ENGINE_CASES = _engine_cases()
PREFILL_CASES = _prefill_cases()

# The needle inputs that tests/test_ops_gpu.py gives its partition-cap test.
PARTITION_CAP_CASE = next(c for c in DECODE_CASES
                          if c.name == "splitk-cap-65600")


# --------------------------------------------------------------------------
# fp64 references
# --------------------------------------------------------------------------

def _scores(q, k, kvh, scale):
    """q [..., Tq, Hq, D], k [..., Tk, Hkv, D] -> [..., Hq, Tq, Tk].
    kvh None: q head h reads kv head h // G; else kvh[h]."""
    if kvh is None:
        hq, hkv = q.shape[-2], k.shape[-2]
        qg = q.unflatten(-2, (hkv, hq // hkv))
        return torch.einsum("...qjgd,...kjd->...jgqk", qg, k) \
            .flatten(-4, -3) * scale
    return torch.einsum("...qhd,...khd->...hqk", q, k[..., kvh, :]) * scale


def _weighted(p, v, kvh):
    """p [..., Hq, Tq, Tk], v [..., Tk, Hkv, D] -> [..., Tq, Hq, D]."""
    if kvh is None:
        hkv = v.shape[-2]
        pg = p.unflatten(-3, (hkv, p.shape[-3] // hkv))
        return torch.einsum("...jgqk,...kjd->...qjgd", pg, v).flatten(-3, -2)
    return torch.einsum("...hqk,...khd->...qhd", p, v[..., kvh, :])


def _attend64(q, k, v, mask, scale, kvh=None):
    """q [..., Tq, Hq, D], k/v [..., Tk, Hkv, D], mask bool [Tq, Tk]
    (True = attend). Returns out [..., Tq, Hq, D] and the softmax
    [..., Hq, Tq, Tk], both fp64."""
    s = _scores(q.double(), k.double(), kvh, scale)
    p = torch.softmax(s.masked_fill(~mask, -math.inf), dim=-1)
    return _weighted(p, v.double(), kvh), p


def _dequant(cache):
    return ops.kv_fp8_dequant(cache) if cache.dtype == torch.uint8 else cache


def _gather(cache, tables, n, bs):
    """The first n tokens of the rows whose tables [R, cols] are given:
    [R, n, Hkv, D]."""
    x = cache[tables[:, :cdiv(n, bs)].long()].permute(0, 1, 3, 2, 4)
    return x.reshape(tables.shape[0], -1, cache.shape[1], cache.shape[3])[:, :n]


def _by_length(lens):
    """[(L, rows)]: the rows of each distinct length."""
    lens = [int(x) for x in lens]
    return [(L, torch.tensor([i for i, x in enumerate(lens) if x == L]))
            for L in sorted(set(lens))]


def decode_geometry(B, hkv, d, max_len, ws_len, kv8):
    """Split-K sizing as the host code does it: partition size, number of
    partitions, and the tokens one phase-C load batch of the whole block
    covers (VPS * C_PAR)."""
    ws_parts = max(1, cdiv(ws_len, PART_QUANT))
    nparts = max(1, TARGET_WGS // max(1, B * hkv))
    nparts = min(nparts, cdiv(max_len, PART_QUANT), ws_parts, MAX_PARTS)
    part = cdiv(cdiv(max_len, nparts), PART_QUANT) * PART_QUANT
    nparts = cdiv(max_len, part)
    vps = 4 if (kv8 or B * hkv * nparts >= 2048) else 8
    return SimpleNamespace(part=part, nparts=nparts,
                           batch=vps * (NTHREADS // (d // 8)))


def _decode_rows(q, kc, vc, bt, lens, scale, window):
    """Rows of one length are computed together. Returns out [B, Hq, D]
    and [(L, rows, softmax [R, Hq, L])]."""
    kc, vc = _dequant(kc), _dequant(vc)
    bs = kc.shape[2]
    out = torch.zeros(q.shape, dtype=torch.float64)
    probs = []
    for L, rows in _by_length(lens):
        keep = torch.zeros(1, L, dtype=torch.bool)
        keep[:, (max(0, L - window) if window > 0 else 0):] = True
        o, p = _attend64(q[rows][:, None], _gather(kc, bt[rows], L, bs),
                         _gather(vc, bt[rows], L, bs), keep, scale)
        out[rows] = o[:, 0]
        probs.append((L, rows, p[:, :, 0]))
    return out, probs


def _decode_mutant_rows(b, row_fn, rows):
    """b.want with rows `rows` recomputed by row_fn(r, L, lo), which
    returns (keep [L + 1], table, kvh) or None where the error does not
    apply. Index L of keep is the slot one past the row's length.
    Returns None if no row changed."""
    kc, vc = _dequant(b.kc), _dequant(b.vc)
    out, changed = b.want.clone(), False
    for r in rows:
        L = int(b.lens[r])
        lo = max(0, L - b.window) if b.window > 0 else 0
        mod = row_fn(r, L, lo)
        if mod is None:
            continue
        keep, table, kvh = mod
        n = L + 1 if bool(keep[L]) else L
        out[r] = _attend64(b.q[r:r + 1], _gather(kc, table[None], n, b.bs)[0],
                           _gather(vc, table[None], n, b.bs)[0],
                           keep[None, :n], b.scale, kvh)[0][0]
        changed = True
    return out if changed else None


def decode_ref64(q, kc, vc, bt, lens, scale, window=0):
    """Paged decode in fp64. q [B, Hq, D]; caches [nblocks, Hkv, bs, D]
    bf16 or e4m3 bytes; bt [B, cols] int32; lens [B]. Row b attends to its
    tokens max(0, len - window) .. len - 1 (all of them for window = 0);
    q head h reads kv head h // G."""
    return _decode_rows(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), lens.cpu(),
                        scale, window)[0]


def _prefill_mask(qlen, klen, causal, window, ctx):
    qpos = torch.arange(qlen)[:, None] + ctx
    tp = torch.arange(klen)[None, :]
    if not causal:
        return torch.ones(qlen, klen, dtype=torch.bool)
    m = tp <= qpos
    if window > 0:
        m &= (qpos - tp) < window
    return m


def _prefill_seqs(q, k, v, cu_q, cu_k, scale, seq_fn):
    """seq_fn(i, qlen, klen) returns (mask [qlen, n], n, kvh): n >= klen
    keys are read from the sequence's first key on."""
    out = torch.zeros(q.shape, dtype=torch.float64)
    probs = []
    for i in range(cu_q.shape[0] - 1):
        q0, q1 = int(cu_q[i]), int(cu_q[i + 1])
        k0, k1 = int(cu_k[i]), int(cu_k[i + 1])
        mask, n, kvh = seq_fn(i, q1 - q0, k1 - k0)
        o, p = _attend64(q[q0:q1], k[k0:k0 + n], v[k0:k0 + n], mask, scale,
                         kvh)
        out[q0:q1] = o
        probs.append(p)
    return out, probs


def prefill_ref64(q, k, v, cu_q, scale, causal=True, window=0, cu_k=None):
    """Varlen prefill in fp64. q [T, Hq, D], k/v [>= Tk, Hkv, D]. Query i
    of a sequence sits at position ctx + i, ctx = klen - qlen; causal: it
    attends to keys tp <= ctx + i, and with a window to those with
    ctx + i - tp < window. Non-causal: to all klen keys (window unused)."""
    cu_k = cu_q if cu_k is None else cu_k

    def seq(i, qlen, klen):
        return (_prefill_mask(qlen, klen, causal, window, klen - qlen),
                klen, None)
    return _prefill_seqs(q.cpu(), k.cpu(), v.cpu(), cu_q.cpu(), cu_k.cpu(),
                         scale, seq)[0]


# --------------------------------------------------------------------------
# CPU emulations of the kernels' rounding
# --------------------------------------------------------------------------

def _attend_emul(q, k, v, mask, scale, prefill):
    if prefill:   # MFMA on bf16 operands, fp32 accumulate, then scale
        s = _scores(q.float(), k.float(), None, 1.0) * scale
    else:         # q * scale held in fp32, then the dot product
        s = _scores(q.float() * scale, k.float(), None, 1.0)
    s = s.masked_fill(~mask, -math.inf)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1)
    if prefill:   # P goes through bf16 into the PV MFMA; l does not
        p = p.bfloat16().float()
    o = _weighted(p, v.float(), None) / l.transpose(-1, -2)[..., None]
    return o.bfloat16()


def decode_emulation(b):
    kc, vc = _dequant(b.kc), _dequant(b.vc)
    out = torch.empty_like(b.q)
    for L, rows in _by_length(b.lens):
        keep = torch.zeros(1, L, dtype=torch.bool)
        keep[:, (max(0, L - b.window) if b.window > 0 else 0):] = True
        out[rows] = _attend_emul(b.q[rows][:, None],
                                 _gather(kc, b.bt[rows], L, b.bs),
                                 _gather(vc, b.bt[rows], L, b.bs), keep,
                                 b.scale, False)[:, 0]
    return out


def prefill_emulation(b):
    out = torch.empty_like(b.q)
    for i in range(len(b.qlens)):
        q0, q1 = int(b.cu_q[i]), int(b.cu_q[i + 1])
        k0, k1 = int(b.cu_k[i]), int(b.cu_k[i + 1])
        mask = _prefill_mask(q1 - q0, k1 - k0, b.causal, b.window,
                             (k1 - k0) - (q1 - q0))
        out[q0:q1] = _attend_emul(b.q[q0:q1], b.k[k0:k1], b.v[k0:k1], mask,
                                  b.scale, True)
    return out


# --------------------------------------------------------------------------
# input builders
# --------------------------------------------------------------------------

def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.seed_key.encode()))


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


@functools.lru_cache(maxsize=1)
def _noise_pool(d):
    """bf16 noise that the large (full-grid) decode cases of one head
    size share, so that they do not each draw 70 M normals."""
    gen = torch.Generator().manual_seed(d)
    return torch.randn(2, POOL_ROWS, d, generator=gen).bfloat16()


class _Noise:
    """Ordinary K and V values of a decode case: [R, L, Hkv, D] fp64."""

    def __init__(self, case, gen):
        self.gen, self.d, self.hkv = gen, case.d, case.hkv
        total = sum(case.lens) * case.hkv
        self.pool = _noise_pool(case.d) if total > POOL_ROWS // 4 else None
        assert total <= POOL_ROWS
        self.used = 0

    def kv(self, R, L):
        if self.pool is None:
            return (_randn(self.gen, R, L, self.hkv, self.d),
                    _randn(self.gen, R, L, self.hkv, self.d))
        n = R * L * self.hkv
        part = self.pool[:, self.used:self.used + n].double()
        self.used += n
        return (part[0].view(R, L, self.hkv, self.d),
                part[1].view(R, L, self.hkv, self.d))


def _directions(gen, hq, hkv, d):
    """u [Hq, D]: unit vectors, orthonormal within each kv group."""
    g = hq // hkv
    u = torch.empty(hq, d, dtype=torch.float64)
    for j in range(hkv):
        qmat, _ = torch.linalg.qr(_randn(gen, d, g))
        u[j * g:(j + 1) * g] = qmat.t()
    return u


def _orthogonal_part(r, u, hkv):
    """Remove from r [..., Hq, D] its components along the directions of
    its own kv group."""
    g = u.shape[0] // hkv
    rg = r.unflatten(-2, (hkv, g))
    ug = u.view(hkv, g, -1)
    coef = torch.einsum("...jgd,jed->...jge", rg, ug)
    return (rg - torch.einsum("...jge,jed->...jgd", coef, ug)).flatten(-3, -2)


def _needle_key(u, hkv, amp):
    """[Hkv, D]: amp * the sum of the group's directions."""
    return amp * u.view(hkv, u.shape[0] // hkv, -1).sum(1)


def _stored(x, kv8=False):
    """x after a round trip through the storage type, in fp64."""
    x = x.bfloat16()
    if kv8:
        x = ops.kv_fp8_dequant(ops.kv_fp8_quant(x))
    return x.double()


def _solve_c(r, u, k, vis, needle, nkey, scale):
    """c [..., Tq, Hq] so that, with q = c * u + r, the needles that each
    (row, head) sees hold the target share of its fp64 softmax.
    r [..., Tq, Hq, D], k [..., Tk, Hkv, D] (ordinary values as stored;
    rows that are needles are ignored), vis bool [Tq, Tk], needle bool
    [Hkv, Tk], nkey [Hkv, D] the needle key as stored. Also returns the
    [..., Tq, Hq] mask of pairs that reach the share (score >= S_MIN)."""
    hq, hkv = u.shape[0], k.shape[-2]
    kvh = torch.arange(hq) // (hq // hkv)
    a = _scores(u.expand(*k.shape[:-3], 1, hq, -1), k, None, scale)
    b = _scores(r, k, None, scale)                    # [..., Hq, Tq, Tk]
    nd = needle[kvh][:, None, :]                      # [Hq, 1, Tk]
    ordinary = vis[None] & ~nd
    n = (vis[None] & nd).sum(-1).double()             # [Hq, Tq]
    assert int(n.max()) <= MAX_NEEDLES, \
        f"{int(n.max())} needles in one softmax; {MAX_NEEDLES} fit"
    share = (n * NEEDLE_FLOOR * 1.1).clamp(NEEDLE_MASS, 0.66)
    logf = torch.log(share / (1 - share) / n.clamp(min=1))
    # needle score = c * alpha + beta (beta comes from the rounding of nkey)
    alpha = (torch.einsum("hd,hd->h", u, nkey[kvh]) * scale)[:, None]
    beta = torch.einsum("...qhd,hd->...hq", r, nkey[kvh]) * scale
    s = torch.full_like(beta, S_MIN)
    for _ in range(4):
        c = (s - beta) / alpha
        z = torch.logsumexp((c[..., None] * a + b).masked_fill(
            ~ordinary, -math.inf), dim=-1)
        s = torch.where(torch.isfinite(z), logf + z, s)
    ok = torch.isfinite(z) & (s >= S_MIN) & (n > 0)
    c = (s.clamp(min=S_MIN) - beta) / alpha
    return c.transpose(-1, -2).contiguous(), ok.transpose(-1, -2)


def _check_masses(p, vis_needle, ok, what):
    """p [..., Tk] fp64 softmax, vis_needle bool broadcastable to p,
    ok bool [...]: the rows the conditions are asserted for."""
    if not bool(ok.any()):
        return
    mass = (p * vis_needle).sum(-1)[ok]
    low = torch.where(vis_needle, p, torch.ones_like(p)).amin(-1)[ok]
    assert float(low.min()) >= NEEDLE_FLOOR, \
        f"{what}: a needle holds {float(low.min()):.4f}"
    assert 0.30 <= float(mass.min()) and float(mass.max()) <= 0.70, \
        f"{what}: needles hold {float(mass.min()):.3f}..{float(mass.max()):.3f}"


def _decode_needles(L, lo, geom, hkv, windowed):
    """bool [Hkv, L]: the needle positions of each kv head."""
    keep = lambda s: {t for t in s if 0 <= t < L}      # noqa: E731
    base = {0, L - 1, CHUNK - 1, CHUNK, lo}
    if windowed:
        base.add(lo - 1)
    nparts = cdiv(L, geom.part)
    parts = range(nparts) if nparts <= 8 else \
        (0, nparts // 2 - 1, nparts // 2, nparts - 1)
    edges = set()
    for p in parts:
        edges |= {p * geom.part, min(L, (p + 1) * geom.part) - 1}
    base, edges = keep(base), keep(edges) - keep(base)
    needle = torch.zeros(hkv, L, dtype=torch.bool)
    needle[:, sorted(base)] = True
    split = len([t for t in base | edges if t >= lo]) > MAX_NEEDLES
    for i, t in enumerate(sorted(edges)):
        if split:   # firsts (even i) to even kv heads, lasts to odd ones
            assert hkv > 1, "too many needles for one kv head"
            needle[i % 2::2, t] = True
        else:
            needle[:, t] = True
    return needle


@functools.lru_cache(maxsize=4)
def build_decode(case):
    """Inputs (CPU tensors) and the fp64 reference for one decode case."""
    gen = _gen(case)
    d, hkv, bs = case.d, case.hkv, case.bs
    hq, B = hkv * case.g, len(case.lens)
    scale = d ** -0.5
    max_len = case.max_len or max(case.lens)
    geom = decode_geometry(B, hkv, d, max_len, case.ws_len or max_len,
                           case.kv8)
    amp = 4 * math.sqrt(d)

    u = _directions(gen, hq, hkv, d)
    nblk = [cdiv(L, bs) for L in case.lens]
    cols = case.table_cols or max(nblk) + 3
    # physical blocks: 0 and 1 are poison (1 is where table padding
    # points), then every row's blocks shuffled together, then two spares
    nblocks = 2 + sum(nblk) + 2
    perm = torch.randperm(sum(nblk), generator=gen).int() + 2
    order = sorted((j, b) for b in range(B) for j in range(nblk[b]))
    bt = torch.ones(B, cols, dtype=torch.int32)
    jj, bb = zip(*order)                      # interleaved across rows
    bt[torch.tensor(bb), torch.tensor(jj)] = perm

    poison_k = _needle_key(u, hkv, 2 * amp).float()          # [Hkv, D]
    kc = poison_k[None, :, None, :].expand(nblocks, hkv, bs, d).clone()
    vc = torch.where(torch.rand(nblocks, hkv, bs, d, generator=gen) < 0.5,
                     -POISON_V, POISON_V)
    q = torch.empty(B, hq, d, dtype=torch.float64)
    needle_key = _stored(_needle_key(u, hkv, amp), case.kv8)
    noise = _Noise(case, gen)
    checks = {}
    for L, rows in _by_length(case.lens):
        R, nb = len(rows), cdiv(L, bs)
        lo = max(0, L - case.window) if case.window > 0 else 0
        k, v = noise.kv(R, L)
        k = _stored(k, case.kv8)
        if case.family == "needle":
            needle = _decode_needles(L, lo, geom, hkv, case.window > 0)
            vis = torch.zeros(1, L, dtype=torch.bool)
            vis[:, lo:] = True
            r = _orthogonal_part(_randn(gen, R, 1, hq, d), u, hkv)
            c, ok = _solve_c(r, u, k, vis, needle, needle_key, scale)
            q[rows] = (c[..., None] * u + r)[:, 0]
            k = torch.where(needle.t()[..., None], needle_key, k)
            vn = needle[torch.arange(hq) // case.g].clone()
            vn[:, :lo] = False
            checks[L] = (vn, ok[:, 0])
        else:
            q[rows] = _randn(gen, R, hq, d)
        # the slots past L in the row's last block keep their poison
        phys = bt[rows, :nb].long()
        kk = kc[phys].permute(0, 1, 3, 2, 4).reshape(R, nb * bs, hkv, d)
        vv = vc[phys].permute(0, 1, 3, 2, 4).reshape(R, nb * bs, hkv, d)
        kk[:, :L], vv[:, :L] = k.float(), v.float()
        kc[phys] = kk.view(R, nb, bs, hkv, d).permute(0, 1, 3, 2, 4)
        vc[phys] = vv.view(R, nb, bs, hkv, d).permute(0, 1, 3, 2, 4)

    q, kc, vc = q.bfloat16(), kc.bfloat16(), vc.bfloat16()
    if case.kv8:
        kc, vc = ops.kv_fp8_quant(kc), ops.kv_fp8_quant(vc)
    lens = torch.tensor(case.lens, dtype=torch.int32)
    want, probs = _decode_rows(q, kc, vc, bt, lens, scale, case.window)
    for L, rows, p in probs:
        if L in checks:
            _check_masses(p, checks[L][0], checks[L][1],
                          f"{case.id} rows of length {L}")
    return SimpleNamespace(case=case, q=q, kc=kc, vc=vc, bt=bt, lens=lens,
                           scale=scale, window=case.window, bs=bs,
                           want=want, geom=geom, tol=TOL_DECODE,
                           max_len=max_len)


def _prefill_needles(qlen, klen, causal, window):
    ctx = klen - qlen
    s = {0, 1, KTILE - 1, KTILE, KTILE + 1, klen - 1}
    if ctx > 0:
        s |= {ctx - 1, ctx}
    if causal and window > 0:
        # kv_lo and kv_lo - 1 of the last and of the first query row
        s |= {klen - window, klen - window - 1, ctx - window + 1,
              ctx - window}
    return sorted(t for t in s if 0 <= t < klen)


PREFILL_PAD = 2     # poison rows after the last sequence's keys


@functools.lru_cache(maxsize=4)
def build_prefill(case):
    """Inputs (CPU tensors) and the fp64 reference for one prefill case."""
    gen = _gen(case)
    hq, hkv, d = case.hq, case.hkv, case.d
    qlens = list(case.qlens)
    klens = list(case.klens or case.qlens)
    scale = d ** -0.5
    amp = 4 * math.sqrt(d)
    cu_q = torch.tensor([0] + qlens, dtype=torch.int32).cumsum(0).int()
    cu_k = torch.tensor([0] + klens, dtype=torch.int32).cumsum(0).int()
    Tq, Tk = sum(qlens), sum(klens)

    u = _directions(gen, hq, hkv, d)
    k = _stored(_randn(gen, Tk + PREFILL_PAD, hkv, d))
    v = _randn(gen, Tk + PREFILL_PAD, hkv, d)
    k[Tk:] = _needle_key(u, hkv, 2 * amp)
    v[Tk:] = (torch.randint(0, 2, (PREFILL_PAD, hkv, d), generator=gen)
              .double() * 2 - 1) * POISON_V
    q = _randn(gen, Tq, hq, d)
    checks = []
    if case.family == "needle":
        needle_key = _stored(_needle_key(u, hkv, amp))
        q = _orthogonal_part(q, u, hkv)
        for i, (ql, kl) in enumerate(zip(qlens, klens)):
            q0, k0 = int(cu_q[i]), int(cu_k[i])
            pos = _prefill_needles(ql, kl, case.causal, case.window)
            needle = torch.zeros(hkv, kl, dtype=torch.bool)
            needle[:, pos] = True
            vis = _prefill_mask(ql, kl, case.causal, case.window, kl - ql)
            c, ok = _solve_c(q[q0:q0 + ql], u, k[k0:k0 + kl], vis, needle,
                             needle_key, scale)
            q[q0:q0 + ql] += c[..., None] * u
            k[k0:k0 + kl][needle.t()] = needle_key.expand(len(pos), hkv, d) \
                .reshape(-1, d)
            checks.append((needle[0], vis, ok))
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()

    def seq(i, ql, kl):
        return (_prefill_mask(ql, kl, case.causal, case.window, kl - ql),
                kl, None)
    want, probs = _prefill_seqs(q, k, v, cu_q, cu_k, scale, seq)
    for i, (needle, vis, ok) in enumerate(checks):
        _check_masses(probs[i], (needle[None] & vis)[None], ok.t(),
                      f"{case.id} sequence {i}")
    return SimpleNamespace(case=case, q=q, k=k, v=v, cu_q=cu_q, cu_k=cu_k,
                           qlens=qlens, klens=klens, scale=scale,
                           causal=case.causal, window=case.window,
                           max_seqlen=case.max_seqlen or max(qlens),
                           want=want, tol=TOL_PREFILL)


# --------------------------------------------------------------------------
# mutants: the reference with one deliberate error. A mutant that changes
# no row's mask, table or head map does not apply to the case and is left
# out of the returned dict.
# --------------------------------------------------------------------------

def decode_mutants(b):
    B, Hq, _ = b.q.shape
    Hkv, bs = b.kc.shape[1], b.bs
    G = Hq // Hkv
    nblocks = b.kc.shape[0]
    part, batch = b.geom.part, b.geom.batch
    true_kvh = None
    # the error is applied to the first rows only (two rounds of the five
    # lengths in the full-grid cases): enough for the mutant to fail
    rows = range(min(B, 10))

    def last_partition_start(L, lo):
        return max(((L - 1) // part) * part, lo)

    def drop_last(keep, L, lo):
        if L - lo >= 2:
            keep[L - 1] = False

    def drop_first_in_window(keep, L, lo):
        if L - lo >= 2:
            keep[lo] = False

    def include_lo_minus_1(keep, L, lo):
        if lo >= 1:
            keep[lo - 1] = True

    def read_past_len(keep, L, lo):
        keep[L] = True

    def drop_last_partition(keep, L, lo):
        ps = last_partition_start(L, lo)
        if ps > lo:
            keep[ps:L] = False

    def drop_phase_c_tail(keep, L, lo):
        ps = last_partition_start(L, lo)
        cb = ps + ((L - 1 - ps) // CHUNK) * CHUNK
        full = cb + ((L - cb) // batch) * batch
        if lo < full < L:
            keep[full:L] = False

    def ignore_window(keep, L, lo):
        keep[:lo] = True

    def mask_mutant(edit):
        def row_fn(r, L, lo):
            keep = torch.zeros(L + 1, dtype=torch.bool)
            keep[lo:L] = True
            before = keep.clone()
            edit(keep, L, lo)
            if torch.equal(keep, before):
                return None
            return keep, b.bt[r], true_kvh
        return row_fn

    def ignore_table(r, L, lo):
        n = cdiv(L, bs)
        lin = ((int(b.bt[r, 0]) + torch.arange(b.bt.shape[1])) % nblocks).int()
        if torch.equal(lin[:n], b.bt[r, :n]):
            return None
        keep = torch.zeros(L + 1, dtype=torch.bool)
        keep[lo:L] = True
        return keep, lin, true_kvh

    def head_mod(r, L, lo):
        if G == 1 or Hkv == 1:
            return None
        keep = torch.zeros(L + 1, dtype=torch.bool)
        keep[lo:L] = True
        return keep, b.bt[r], torch.arange(Hq) % Hkv

    fns = {name: mask_mutant(f) for name, f in [
        ("drop_last", drop_last),
        ("drop_first_in_window", drop_first_in_window),
        ("include_kv_lo_minus_1", include_lo_minus_1),
        ("read_past_len", read_past_len),
        ("drop_last_partition", drop_last_partition),
        ("drop_phase_c_tail", drop_phase_c_tail),
        ("ignore_window", ignore_window)]}
    fns["ignore_block_table"] = ignore_table
    fns["head_mod_hkv"] = head_mod
    out = {"zeros": torch.zeros_like(b.want)}
    for name, fn in fns.items():
        got = _decode_mutant_rows(b, fn, rows)
        if got is not None:
            out[name] = got
    return out


def prefill_mutants(b):
    Hq, Hkv = b.q.shape[1], b.k.shape[1]
    G = Hq // Hkv
    true_kvh = None
    causal, window = b.causal, b.window

    def true_mask(ql, kl):
        return _prefill_mask(ql, kl, causal, window, kl - ql)

    def shifted(shift):
        # causal edge moved by shift keys; the window edge stays
        def f(ql, kl):
            if not causal:
                return None
            qpos = torch.arange(ql)[:, None] + (kl - ql)
            tp = torch.arange(kl)[None, :]
            m = tp <= qpos + shift
            if window > 0:
                m &= (qpos - tp) < window
            m[:, 0] |= ~m.any(-1)     # never leave a row without keys
            return m, kl
        return f

    def ignore_ctx(ql, kl):
        return (_prefill_mask(ql, kl, causal, window, 0), kl) if causal \
            else None

    def past_klen(ql, kl):
        if causal:
            return None
        return torch.ones(ql, kl + PREFILL_PAD, dtype=torch.bool), \
            kl + PREFILL_PAD

    def ignore_window(ql, kl):
        return _prefill_mask(ql, kl, causal, 0, kl - ql), kl

    def include_lo_minus_1(ql, kl):
        if not (causal and window > 0):
            return None
        return _prefill_mask(ql, kl, True, window + 1, kl - ql), kl

    def drop_first_in_window(ql, kl):
        m = true_mask(ql, kl)
        first = m.int().argmax(-1)
        many = m.sum(-1) >= 2
        m[torch.arange(ql)[many], first[many]] = False
        return m, kl

    def drop_last(ql, kl):
        if causal or kl < 2:
            return None
        m = true_mask(ql, kl)
        m[:, kl - 1] = False
        return m, kl

    def run(mask_fn, kvh):
        changed = []

        def seq(i, ql, kl):
            mod = mask_fn(ql, kl) if mask_fn is not None else None
            tm = true_mask(ql, kl)
            if mod is None:
                return tm, kl, kvh
            m, n = mod
            if n != kl or not torch.equal(m, tm):
                changed.append(i)
            return m, n, kvh
        got, _ = _prefill_seqs(b.q, b.k, b.v, b.cu_q, b.cu_k, b.scale, seq)
        return got, changed

    out = {"zeros": torch.zeros_like(b.want)}
    for name, fn in [("causal_plus_1", shifted(1)),
                     ("causal_minus_1", shifted(-1)),
                     ("ignore_ctx", ignore_ctx),
                     ("attend_past_klen", past_klen),
                     ("ignore_window", ignore_window),
                     ("include_kv_lo_minus_1", include_lo_minus_1),
                     ("drop_first_in_window", drop_first_in_window),
                     ("drop_last", drop_last)]:
        got, changed = run(fn, true_kvh)
        if changed:
            out[name] = got
    if G > 1 and Hkv > 1:
        out["head_mod_hkv"] = run(None, torch.arange(Hq) % Hkv)[0]
    return out


# --------------------------------------------------------------------------
# measurement: `python -m tests.attn_oracle` prints what the header quotes
# --------------------------------------------------------------------------

def measure(cases, build, emulate, mutants):
    """(worst emulation error by family, smallest needle-mutant error and
    which mutant of which case it is)."""
    emul = {"needle": 0.0, "randn": 0.0}
    smallest = (math.inf, "")
    for case in cases:
        b = build(case)
        e = float(attn_error(emulate(b), b.want).max())
        emul[case.family] = max(emul[case.family], e)
        if case.family == "needle":
            for name, got in mutants(b).items():
                m = float(attn_error(got, b.want).max())
                smallest = min(smallest, (m, f"{name} on {case.id}"))
    return emul, smallest


if __name__ == "__main__":
    import time
    t0 = time.time()
    for what, args in [
            ("decode", (DECODE_CASES + ENGINE_CASES, build_decode,
                        decode_emulation, decode_mutants)),
            ("prefill", (PREFILL_CASES, build_prefill, prefill_emulation,
                         prefill_mutants))]:
        emul, smallest = measure(*args)
        print(f"{what}: emulation error {emul}, 4x worst = "
              f"{4 * max(emul.values()):.5f}; smallest mutant error "
              f"{smallest[0]:.4f} ({smallest[1]}); {time.time() - t0:.1f} s")
