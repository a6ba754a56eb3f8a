"""ops.attn_prefill_paged on the CPU, and the cases and the paging of
tests/attn_oracle.py prefill inputs that tests/test_attn_paged_prefill_gpu.py
shares.

page_case lays a case's compact K/V (b.k, b.v) out as a paged cache: a
shuffled permutation of physical blocks interleaved across the sequences, a
table three columns wider than needed whose padding points at block 1, every
slot nobody owns (blocks 0 and 1, the spares, the tails) filled with the
case's poison row, and NaN (bf16 NaN, or the e4m3 byte 0x7F) in the V slots
at or past klen of each sequence's last block.
"""
import functools
import zlib
from types import SimpleNamespace

import pytest
import torch

import attn_oracle as ao
import helix_amd.ops as ops
from attn_oracle import PrefillCase, _both, build_prefill, cdiv


def _cases():
    cs = []
    for d in (128, 64):     # tile edges, a one-row suffix, ctx = 0 in the batch
        cs.append(PrefillCase(f"paged-edges-d{d}", 8, 2, d, (1, 64, 65, 17),
                              (64, 64, 193, 17)))
    for d in (128, 64):     # many tiles and blocks, more than one q-tile
        cs.append(PrefillCase(f"paged-long-d{d}", 8, 2, d, (130, 3),
                              (700, 51)))
    for w in (24, 128):
        cs.append(PrefillCase(f"paged-window{w}", 8, 2, 128, (7, 64, 1),
                              (200, 300, 130), window=w))
    cs.append(PrefillCase("paged-g1", 4, 4, 128, (5, 70), (133, 70)))
    cs.append(PrefillCase("paged-g8", 8, 1, 64, (5, 70), (133, 70)))
    return _both(cs)


PAGED_CASES = _cases()


@functools.lru_cache(maxsize=None)
def gathered(case, kv8):
    """(k, v) [Tk, Hkv, D] bf16 as a gather (and dequant) of the cache
    gives them, and the fp64 reference on those values."""
    b = build_prefill(case)
    k, v = b.k[:int(b.cu_k[-1])], b.v[:int(b.cu_k[-1])]
    if kv8:
        k = ops.kv_fp8_dequant(ops.kv_fp8_quant(k))
        v = ops.kv_fp8_dequant(ops.kv_fp8_quant(v))
    want = b.want if not kv8 else ao.prefill_ref64(
        b.q, k, v, b.cu_q, b.scale, True, b.window, b.cu_k)
    return k, v, want


@functools.lru_cache(maxsize=None)
def page_case(case, kv8, bs):
    b = build_prefill(case)
    B, hkv, d = len(b.klens), case.hkv, case.d
    nblk = [cdiv(kl, bs) for kl in b.klens]
    nblocks = 2 + sum(nblk) + 2
    gen = torch.Generator().manual_seed(zlib.crc32(f"{case.id}-{bs}".encode()))
    perm = torch.randperm(sum(nblk), generator=gen).int() + 2
    jj, ss = zip(*sorted((j, s) for s in range(B) for j in range(nblk[s])))
    bt = torch.ones(B, max(nblk) + 3, dtype=torch.int32)
    bt[torch.tensor(ss), torch.tensor(jj)] = perm
    kc = b.k[-1][None, :, None, :].expand(nblocks, hkv, bs, d).clone()
    vc = b.v[-1][None, :, None, :].expand(nblocks, hkv, bs, d).clone()
    if kv8:
        kc, vc = ops.kv_fp8_quant(kc), ops.kv_fp8_quant(vc)
    k, v, want = gathered(case, kv8)
    for s, kl in enumerate(b.klens):
        k0 = int(b.cu_k[s])
        pos = torch.arange(nblk[s] * bs)
        blk, off = bt[s, pos // bs].long(), pos % bs
        ks, vs = k[k0:k0 + kl], v[k0:k0 + kl]
        kc[blk[:kl], :, off[:kl]] = ops.kv_fp8_quant(ks) if kv8 else ks
        vc[blk[:kl], :, off[:kl]] = ops.kv_fp8_quant(vs) if kv8 else vs
        vc[blk[kl:], :, off[kl:]] = 0x7F if kv8 else float("nan")
    return SimpleNamespace(
        q=b.q, kc=kc, vc=vc, bt=bt, cu_q=b.cu_q, cu_k=b.cu_k,
        seq_lens=torch.tensor(b.klens, dtype=torch.int32), k=k, v=v,
        max_seqlen=b.max_seqlen, max_klen=max(b.klens), scale=b.scale,
        window=b.window, want=want)


def run_paged(p, dev):
    return ops.attn_prefill_paged(
        p.q.to(dev), p.kc.to(dev), p.vc.to(dev), p.bt.to(dev),
        p.cu_q.to(dev), p.seq_lens.to(dev), p.max_seqlen, p.max_klen,
        p.scale, window=p.window)


def run_gathered(p, dev):
    return ops.attn_prefill(p.q.to(dev), p.k.to(dev), p.v.to(dev),
                            p.cu_q.to(dev), p.max_seqlen, p.scale,
                            window=p.window, cu_seqlens_k=p.cu_k.to(dev))


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize(
    "case", [c for c in PAGED_CASES
             if c.name in ("paged-edges-d128", "paged-window24")],
    ids=lambda c: c.id)
def test_cpu_equals_gather(case, kv8):
    p = page_case(case, kv8, 16)
    assert torch.equal(run_paged(p, "cpu"), run_gathered(p, "cpu"))
