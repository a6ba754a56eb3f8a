"""Proof, on the CPU, that tests/test_decode_blockids_gpu.py can fail.

For every case of tests/decode_blockids_cases.py the CPU emulation of the
kernel's rounding passes the assertion the GPU test makes, and the fp64
reference with one deliberate error in how a chunk finds its block ids
fails it on the needle inputs. The errors are those the staging in
paged_attn_decode.hip invites. A partition is walked in 128-token chunks
from p_start = max(partition start, kv_lo); a chunk at cbase keeps the ids
of blocks (cbase >> s) .. ((chunk's last token) >> s) in slots 0, 1, ..
and token t reads slot (t >> s) - (cbase >> s):
  * stale_buffer: a chunk reads the slots the previous chunk staged;
  * one_entry_short: the last block a chunk straddles was not staged and
    takes the id of the block before it;
  * shift_off_by_one: the slot is computed with s + 1;
  * v_batch_from_next_chunk: the first V batch of a chunk that has a
    successor (VPS * C_PAR tokens) reads the slots of the next chunk; K
    is right. This is the error of a V batch that is issued next to the
    K prefetch, which reads the next chunk's buffer. That stage measured
    slower and is not in the tree (profiles/r07_decode_blockids.md); the
    mutant stays for the next attempt.
"""
import functools

import pytest
import torch

import attn_oracle as ao
import decode_blockids_cases as dc

CASES = dc.CASES + dc.ENGINE_CASES
MUTANTS = ("stale_buffer", "one_entry_short", "shift_off_by_one",
           "v_batch_from_next_chunk")


def _chunk_geometry(b, L, lo):
    """Per token t of a row (t < lo: unused): the base of its chunk, that
    chunk's last token, and whether the chunk has a successor."""
    part = b.geom.part
    t = torch.arange(L)
    p_start = torch.clamp((t // part) * part, min=lo)
    p_end = torch.clamp((t // part + 1) * part, max=L)
    cbase = p_start + ((t - p_start) // ao.CHUNK) * ao.CHUNK
    clast = torch.minimum(cbase + ao.CHUNK, p_end) - 1
    return t, cbase, clast, cbase + ao.CHUNK < p_end


def _columns(b, name, L, lo):
    """(table column of token t for K, for V) under the mutant."""
    s = b.bs.bit_length() - 1
    t, cbase, clast, has_next = _chunk_geometry(b, L, lo)
    true = t >> s
    first, slot = cbase >> s, (t >> s) - (cbase >> s)
    if name == "stale_buffer":
        prev = torch.where(cbase - ao.CHUNK >= torch.clamp(
            (t // b.geom.part) * b.geom.part, min=lo), cbase - ao.CHUNK, cbase)
        col = (prev >> s) + slot
        return col, col
    if name == "one_entry_short":
        last = clast >> s
        col = torch.where((true == last) & (last > first), last - 1, true)
        return col, col
    if name == "shift_off_by_one":
        col = first + (t >> (s + 1)) - (cbase >> (s + 1))
        return col, col
    if name == "v_batch_from_next_chunk":
        in_first = has_next & (t - cbase < b.geom.batch)
        vcol = torch.where(in_first, ((cbase + ao.CHUNK) >> s) + slot, true)
        return true, vcol
    raise KeyError(name)


def _mutant(b, name):
    """b.want with the first rows recomputed under the mutant, or None
    if it changes no row."""
    kc, vc = ao._dequant(b.kc), ao._dequant(b.vc)
    out, changed = b.want.clone(), False
    for r in range(min(len(b.lens), 10)):
        L = int(b.lens[r])
        lo = max(0, L - b.window) if b.window > 0 else 0
        kcol, vcol = _columns(b, name, L, lo)
        true = torch.arange(L) >> (b.bs.bit_length() - 1)
        vis = torch.arange(L) >= lo
        if torch.equal(kcol[vis], true[vis]) and \
                torch.equal(vcol[vis], true[vis]):
            continue
        off = torch.arange(L) % b.bs
        cols = b.bt.shape[1]
        k = kc[b.bt[r, kcol.clamp(0, cols - 1)].long(), :, off]
        v = vc[b.bt[r, vcol.clamp(0, cols - 1)].long(), :, off]
        out[r] = ao._attend64(b.q[r:r + 1], k, v, vis[None], b.scale)[0][0]
        changed = True
    return out if changed else None


@functools.lru_cache(maxsize=None)
def _result(case):
    """(emulation error, {mutant: its error}); floats only."""
    b = ao.build_decode(case)
    emul = ao.decode_emulation(b)
    e = ao.assert_attn_close(emul, b.want, ao.TOL_DECODE,
                             f"{case.id} emulation")
    errs = {}
    if case.family == "needle":
        for name in MUTANTS:
            got = _mutant(b, name)
            if got is None:
                continue
            with pytest.raises(AssertionError):
                ao.assert_attn_close(got, b.want, ao.TOL_DECODE,
                                     f"{case.id} {name}")
            errs[name] = float(ao.attn_error(got, b.want).max())
    print(f"{case.id}: emulation {e:.5f} passes tol {ao.TOL_DECODE}; "
          "rejected: " + ", ".join(f"{n} {v:.3f}"
                                   for n, v in sorted(errs.items())))
    return e, errs


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case(case):
    _result(case)


def test_identity_columns_reproduce_the_oracle():
    """The mutants' own gather, given the true columns, is the oracle."""
    b = ao.build_decode(next(c for c in CASES
                             if c.name == "ids-window203-bs8"))
    kc, vc = ao._dequant(b.kc), ao._dequant(b.vc)
    for r, L in enumerate(int(x) for x in b.lens):
        lo = max(0, L - b.window)
        t = torch.arange(L)
        k = kc[b.bt[r, t // b.bs].long(), :, t % b.bs]
        v = vc[b.bt[r, t // b.bs].long(), :, t % b.bs]
        got = ao._attend64(b.q[r:r + 1], k, v, (t >= lo)[None], b.scale)[0][0]
        assert torch.allclose(got, b.want[r], rtol=0, atol=1e-12)


def test_mutants_apply_and_fail():
    """Every mutant applies to the cases it was written for, and the
    smallest error of each is far above the tolerance."""
    dec = {c.name: _result(c)[1] for c in CASES if c.family == "needle"}
    # rows that walk several chunks in one partition: the full grid (no
    # split-K) and the one-partition workspaces
    multi = ["ids-fullgrid-bs32"] + [n for n in dec if "onepart" in n]
    assert len(multi) == 6
    for name in multi:
        assert {"stale_buffer", "v_batch_from_next_chunk"} <= \
            set(dec[name]), name
    for name in ("ids-onepart-bs8", "ids-onepart-window203-bs16",
                 "ids-bs8", "ids-bs32", "ids-bs64", "ids-window131-bs16",
                 "ids-window203-bs8", "ids-splitk-bs64", "ids-fullgrid-bs32",
                 "ids-fp8-d64-g8-bs32", "ids-engine-bs32"):
        assert {"one_entry_short", "shift_off_by_one"} <= set(dec[name]), name
    # at bs >= CHUNK an aligned chunk lies in one block: slot 0 whatever
    # the shift, and no second entry to leave out. What such a chunk can
    # get wrong is whose id it reads (stale_buffer, above).
    for name in ("ids-bs128", "ids-bs256", "ids-onepart-bs256"):
        assert not {"one_entry_short", "shift_off_by_one"} & set(dec[name])
    for m in MUTANTS:
        smallest = min(errs[m] for errs in dec.values() if m in errs)
        print(f"{m}: smallest error {smallest:.4f} "
              f"(tol {ao.TOL_DECODE})")
        assert smallest > 4 * ao.TOL_DECODE, (m, smallest)


def test_block_size_validation():
    """EngineConfig and KVCache refuse what the kernel's host code
    refuses: a block size that is no power of two or is below 8."""
    from helix_amd.engine.engine import EngineConfig
    from helix_amd.engine.kv_cache import KVCache
    for bs in (24, 4, 0):
        with pytest.raises(ValueError, match="power of two"):
            EngineConfig(block_size=bs)
        with pytest.raises(ValueError, match="power of two"):
            KVCache(1, 1, 64, bs, 2, "cpu")
    for bs in (8, 16, 32, 256):
        assert EngineConfig(block_size=bs).block_size == bs
        assert KVCache(1, 1, 64, bs, 2, "cpu").block_size == bs
