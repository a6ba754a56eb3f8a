#!/usr/bin/env python
"""Mixture-of-experts layer benchmark: the fused routed-GEMM kernels against
the eager library path.

Times ops.moe_forward (route + lists + experts + combine) with fused=True
and fused=False on one Mixtral-shaped MoE layer (E 8, k 2, H 4096, I 14336
unless given) at decode and prefill token counts, under two routings:
  uniform  random router logits
  skewed   every token's first choice is expert 0, the second one random
and prints one JSON line per (T, routing, path): median and min
microseconds per call, and for the fused path the bytes of the distinct
activated experts' weights per second that time corresponds to.

Method: device events around a window of `--iters` back-to-back calls,
`--rounds` windows per path with the two paths interleaved inside one
process, after a warm-up of every shape. Each call uses the next of several
copies of the layer's weights (more than the 256 MiB last-level cache
between two uses of a weight), as consecutive layers of a model would. The
library path's host sync is inside its window: it is part of that path.

--fmt q4_0 | q8_0 times ops.moe_forward_wq on the same layer held as ggml
Q4_0 / Q8_0 planes (random payload bytes and scales: the time does not
depend on the values); its library path is the feature's own, with a
dequantise per non-empty expert. weight_bytes then counts the blocks
(18 / 34 bytes per 32 weights). Run bf16 and the quantised formats in one
session to compare them.

--fmt q4_k | q6_k times ops.moe_forward_kq on the layer held as ggml
Q4_K / Q6_K super-block planes (random payload and scale codes, small finite
fp16 d / dmin); H and I must be multiples of 256. weight_bytes counts the
super-blocks (144 / 210 bytes per 256 weights).

A GPU is required; there is no CPU fallback. Run under a time limit, e.g.
    timeout 600 python scripts/bench_moe.py --out moe.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helix_amd.ops as ops  # noqa: E402

TS = [1, 8, 16, 64, 128, 512]
ROUTINGS = ("uniform", "skewed")
CACHE_BYTES = 768 << 20       # rotate over at least this many weight bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--topk", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=14336)
    ap.add_argument("--t", type=int, action="append")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fmt", default="bf16", choices=("bf16", "q4_0", "q8_0", "q4_k", "q6_k"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe.py needs a GPU")
    assert ops.have_native(), "native extension is not built"
    dev = torch.device("cuda:0")
    E, k, H, I = args.experts, args.topk, args.hidden, args.inter
    fmt = args.fmt
    kq = fmt in ("q4_k", "q6_k")
    if kq and (H % 256 or I % 256):
        sys.exit(f"--fmt {fmt} needs --hidden and --inter to be multiples "
                 f"of 256")
    blk_bytes = {"bf16": 512, "q4_0": 144, "q8_0": 272, "q4_k": 144,
                 "q6_k": 210}[fmt]                          # per 256 weights
    expert_bytes = 3 * H * I * blk_bytes // 256
    # the least a call activates is k experts; keep two uses of a weight
    # more than the last-level cache apart
    copies = max(2, -(-CACHE_BYTES // (k * expert_bytes)))
    g = torch.Generator(device=dev).manual_seed(E + H + I)
    layers = []

    def planes(rows, K, std):
        # d * q with q uniform over the format's range has about this std
        qdt, per, qstd = (torch.uint8, K // 2, 4.6) if fmt == "q4_0" \
            else (torch.int8, K, 73.9)
        qs = torch.randint(0, 256, (E, rows, per), dtype=torch.uint8,
                           device=dev, generator=g).view(qdt)
        d = torch.empty(E, rows, K // 32, device=dev)
        d.uniform_(0.5, 1.5, generator=g)
        return qs, (d * (std / qstd)).to(torch.float16)

    def rbytes(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev,
                             generator=g)

    def kq_planes(rows, K, std):
        d = torch.empty(E, rows, K // 256, device=dev)
        d.uniform_(0.5, 1.5, generator=g)
        if fmt == "q4_k":
            # (d*sc)*nib - dmin*m with 6-bit sc, m: keep the std near `std`
            hdr = rbytes(E, rows, K // 256, 16)
            hdr[..., 0:2] = (d * (std / 150)).to(torch.float16)[..., None] \
                .view(torch.uint8)
            hdr[..., 2:4] = (d * (std / 30)).to(torch.float16)[..., None] \
                .view(torch.uint8)
            return rbytes(E, rows, K // 2), hdr
        return (rbytes(E, rows, K // 2), rbytes(E, rows, K // 4),
                rbytes(E, rows, K // 16).view(torch.int8),
                (d * (std / 1400)).to(torch.float16))

    for _ in range(copies):
        if kq:
            layers.append((kq_planes(2 * I, H, H ** -0.5),
                           kq_planes(H, I, I ** -0.5)))
            continue
        if fmt != "bf16":
            layers.append((planes(2 * I, H, H ** -0.5),
                           planes(H, I, I ** -0.5)))
            continue
        w13 = torch.empty(E, 2 * I, H, dtype=torch.bfloat16, device=dev)
        w2 = torch.empty(E, H, I, dtype=torch.bfloat16, device=dev)
        w13.normal_(0.0, H ** -0.5, generator=g)
        w2.normal_(0.0, I ** -0.5, generator=g)
        layers.append((w13, w2))

    def call(fused, x, logits, i):
        w13, w2 = layers[i % copies]
        if kq:
            return ops.moe_forward_kq(x, logits, w13, w2, fmt, k, fused=fused,
                                      scratch=scratch)
        if fmt != "bf16":
            return ops.moe_forward_wq(x, logits, w13, w2, fmt, k, fused=fused,
                                      scratch=scratch)
        return ops.moe_forward(x, logits, w13, w2, k, fused=fused)

    scratch = torch.empty(2 * I * H, dtype=torch.bfloat16, device=dev)
    lines = []
    for T in args.t or TS:
        for routing in ROUTINGS:
            x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
            logits = torch.randn(T, E, generator=g, device=dev)
            if routing == "skewed":
                logits[:, 0] += 100.0
            logits = logits.to(torch.bfloat16)
            ids, _ = ops.moe_route(logits, k)
            counts = torch.bincount(ids.reshape(-1).long(), minlength=E)
            distinct = int((counts > 0).sum())
            paths = {"fused": True, "library": False}
            got = {}
            for name, fused in paths.items():               # warm-up
                for i in range(2 * copies + 3):
                    got[name] = call(fused, x, logits, i)
            torch.cuda.synchronize()
            # the two paths agree on what they compute (same weights: both
            # ended the warm-up on the same copy)
            diff = (got["fused"].float() - got["library"].float()).abs().max()
            scale = got["library"].float().abs().max()
            times = {name: [] for name in paths}
            for _ in range(args.rounds):
                for name, fused in paths.items():
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for i in range(args.iters):
                        call(fused, x, logits, i)
                    t1.record()
                    t1.synchronize()
                    times[name].append(
                        t0.elapsed_time(t1) * 1e3 / args.iters)
            lib_med = statistics.median(times["library"])
            for name, ts in times.items():
                med, mn = statistics.median(ts), min(ts)
                rec = {"fmt": fmt, "E": E, "k": k, "H": H, "I": I, "T": T,
                       "routing": routing, "path": name,
                       "us_median": round(med, 1), "us_min": round(mn, 1),
                       "distinct_experts": distinct,
                       "longest_list": int(counts.max()),
                       "weight_bytes": distinct * expert_bytes,
                       "weight_GBps": round(
                           distinct * expert_bytes / med / 1e3, 1),
                       "speedup_vs_library": round(lib_med / med, 3),
                       "max_abs_diff_over_max": round(
                           float(diff / scale), 5)}
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
