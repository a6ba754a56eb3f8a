#!/usr/bin/env python
"""A/B of cached-prefix prefill attention: ops.attn_prefill_paged (K/V read
through the block table) against the composition it replaced, timed as a
whole: index gather of K and V from the paged cache, fp8 dequant for an
e4m3 cache, then ops.attn_prefill on the compact copy.

Geometry: llama3-8b heads (Hq 32, Hkv 8, D 128), block size 16, shuffled
block tables, bf16 and fp8 caches. Shapes: one 2048-token chunk on a context
of 2048, 8192 and 32768 tokens (klen = ctx + 2048), and a prefix hit of 16
sequences x (ctx 2048, 32 new tokens).

Method: one process, both variants interleaved; device events around a
window of back-to-back calls sized to about --window seconds, --rounds
windows per variant after a warm-up of both; median and min microseconds per
call. Each call reads the next of several copies of the cache whose total
size exceeds the 256 MiB last-level cache, as consecutive layers of a model
do. The composition's gather index tensors are built once outside the timed
window (the engine used to rebuild them on the host every step, which is
not charged here). Before timing, the two outputs are compared bit for bit
at the timed size, and the bytes the composition allocates (its peak over
one call, less the output) are read from the allocator.

A GPU is required. Prints one JSON line per (shape, cache dtype); --out
appends them to a file. Run it twice for the spread.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helix_amd.ops as ops  # noqa: E402

HQ, HKV, D, BS = 32, 8, 128, 16
SHAPES = [("chunk2048-ctx2048", 1, 2048, 2048),       # name, B, ctx, new
          ("chunk2048-ctx8192", 1, 8192, 2048),
          ("chunk2048-ctx32768", 1, 32768, 2048),
          ("prefix16x2048+32", 16, 2048, 32)]
ROTATE_BYTES = 512 << 20


def build(B, ctx, new, kv8, dev, gen):
    klen = ctx + new
    nblk = -(-klen // BS)
    nblocks = B * nblk + 2
    bt = (torch.randperm(B * nblk, generator=gen, device=dev) + 2) \
        .int().view(B, nblk)
    kc = torch.randn(nblocks, HKV, BS, D, generator=gen, device=dev) \
        .to(torch.bfloat16)
    vc = torch.randn(nblocks, HKV, BS, D, generator=gen, device=dev) \
        .to(torch.bfloat16)
    if kv8:
        kc, vc = ops.kv_fp8_quant(kc), ops.kv_fp8_quant(vc)
    copies = max(2, -(-ROTATE_BYTES // (2 * kc.numel() * kc.element_size())))
    caches = [(kc, vc)] + [(kc.clone(), vc.clone()) for _ in range(copies - 1)]
    q = torch.randn(B * new, HQ, D, generator=gen, device=dev) \
        .to(torch.bfloat16)
    cu_q = torch.arange(B + 1, device=dev, dtype=torch.int32) * new
    cu_k = torch.arange(B + 1, device=dev, dtype=torch.int32) * klen
    seq_lens = torch.full((B,), klen, dtype=torch.int32, device=dev)
    pos = torch.arange(klen, device=dev)
    gblk = bt[:, pos // BS].long().reshape(-1)
    goff = (pos % BS).repeat(B)
    scale = D ** -0.5

    def paged(i):
        k, v = caches[i % copies]
        return ops.attn_prefill_paged(q, k, v, bt, cu_q, seq_lens, new, klen,
                                      scale)

    def composition(i):
        k, v = caches[i % copies]
        k_all, v_all = k[gblk, :, goff], v[gblk, :, goff]
        if kv8:
            k_all = ops.kv_fp8_dequant(k_all, q.dtype)
            v_all = ops.kv_fp8_dequant(v_all, q.dtype)
        return ops.attn_prefill(q, k_all, v_all, cu_q, new, scale,
                                cu_seqlens_k=cu_k)

    return {"paged": paged, "composition": composition}, q


def window_us(fn, iters):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append",
                    choices=[s[0] for s in SHAPES])
    ap.add_argument("--dtype", action="append", choices=["bf16", "fp8"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2,
                    help="seconds of back-to-back calls per timed window")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_paged_prefill.py needs a GPU")
    assert ops.have_native(), "native extension is not built"
    dev = torch.device("cuda:0")
    lines = []
    for name, B, ctx, new in SHAPES:
        if args.shape and name not in args.shape:
            continue
        for dt in args.dtype or ["bf16", "fp8"]:
            gen = torch.Generator(device=dev).manual_seed(ctx + new + B)
            fns, q = build(B, ctx, new, dt == "fp8", dev, gen)
            equal = torch.equal(fns["paged"](0), fns["composition"](0))
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fns["composition"](0)
            torch.cuda.synchronize()
            comp_alloc = torch.cuda.max_memory_allocated() - base \
                - q.numel() * q.element_size()
            iters = {}
            for v, fn in fns.items():                    # warm-up, sizing
                window_us(fn, 3)
                iters[v] = max(5, min(2000, int(
                    args.window * 1e6 / window_us(fn, 5))))
            times = {v: [] for v in fns}
            for _ in range(args.rounds):
                for v, fn in fns.items():
                    times[v].append(window_us(fn, iters[v]))
            med = {v: statistics.median(t) for v, t in times.items()}
            rec = {"shape": name, "B": B, "ctx": ctx, "new": new, "cache": dt,
                   "paged_us": round(med["paged"], 1),
                   "paged_us_min": round(min(times["paged"]), 1),
                   "composition_us": round(med["composition"], 1),
                   "composition_us_min": round(min(times["composition"]), 1),
                   "composition_over_paged": round(
                       med["composition"] / med["paged"], 3),
                   "composition_alloc_bytes": int(comp_alloc),
                   "bit_equal": equal, "iters": iters}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del fns, q
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
