#!/usr/bin/env python
"""Projection-GEMM benchmark for Q4_0/Q8_0 and Q4_K/Q6_K weight-only
serving.

Times ops.gemm_wq and ops.gemm_kq (every format, or those given with
--variant) against torch.nn.functional.linear on
bf16 weights (the dense path, the baseline) at the llama3-8b projection
shapes and decode/prefill batch sizes, and prints one JSON line per
(shape, M, variant): median and min microseconds per call and the weight
bytes per second that time corresponds to.

Method: device events around a window of `--iters` back-to-back calls,
`--rounds` windows per variant with the variants interleaved inside one
process, after a warm-up of every shape. Each call uses the next of
several copies of the weight whose total size exceeds the 256 MiB
last-level cache, as consecutive layers of a model would; timing one
resident weight would flatter the smaller formats.

A GPU is required; there is no CPU fallback. Run one shape per process
under its own time limit, e.g.
    timeout 300 python scripts/bench_wq.py --shape 4096x4096
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helix_amd.ops as ops  # noqa: E402

SHAPES = ["6144x4096", "4096x4096", "28672x4096", "4096x14336"]   # N x K
MS = [1, 4, 16, 64, 128, 512]
CACHE_BYTES = 768 << 20       # rotate over at least this many weight bytes


VARIANTS = ("bf16", "q8_0", "q4_0", "q4_k", "q6_k")
# bytes per 256 weights: bf16, 8 ggml blocks of 34 / 18, one super-block
BYTES_PER_256 = {"bf16": 512, "q8_0": 272, "q4_0": 144, "q4_k": 144,
                 "q6_k": 210}


def weight_bytes(variant: str, N: int, K: int) -> int:
    return N * K * BYTES_PER_256[variant] // 256


def fused_max_m(variant: str) -> int:
    return ops.KQ_FUSED_MAX_M if variant in ops.KQ_FORMATS \
        else ops.WQ_FUSED_MAX_M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append",
                    help="NxK, repeatable (default: the llama3-8b set)")
    ap.add_argument("--m", type=int, action="append")
    ap.add_argument("--variant", action="append", choices=VARIANTS[1:],
                    help="repeatable (default: all); bf16, the baseline, "
                    "is always timed")
    ap.add_argument("--fused-max-m", type=int, default=0,
                    help="time the fused kernels up to this M instead of "
                    "the shipped cutoffs (to measure where the cutoff "
                    "belongs)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_wq.py needs a GPU")
    assert ops.have_native(), "native extension is not built"
    if args.fused_max_m:
        ops.WQ_FUSED_MAX_M = min(args.fused_max_m, ops._C.WQ_KERNEL_MAX_M)
        ops.KQ_FUSED_MAX_M = min(args.fused_max_m, ops._C.KQ_KERNEL_MAX_M)
    dev = torch.device("cuda:0")
    lines = []
    for shape in args.shape or SHAPES:
        N, K = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(N + K)
        w = torch.randn(N, K, generator=g, device=dev) * 0.02
        variants = {}
        for v in ["bf16"] + list(args.variant or VARIANTS[1:]):
            copies = max(2, -(-CACHE_BYTES // weight_bytes(v, N, K)))
            if v == "bf16":
                wb = w.to(torch.bfloat16)
                variants[v] = [(wb.clone(),) for _ in range(copies)]
            elif v in ops.KQ_FORMATS:
                planes = ops.quantize_kq(w, v)
                variants[v] = [tuple(p.clone() for p in planes)
                               for _ in range(copies)]
            else:
                qs, d = ops.quantize_wq(w, v)
                variants[v] = [(qs.clone(), d.clone()) for _ in range(copies)]
        del w
        scratch = torch.empty(N * K, dtype=torch.bfloat16, device=dev)

        def call(v, x, i):
            ws = variants[v][i % len(variants[v])]
            if v == "bf16":
                return torch.nn.functional.linear(x, ws[0])
            if v in ops.KQ_FORMATS:
                return ops.gemm_kq(x, ws, v, scratch=scratch)
            return ops.gemm_wq(x, ws[0], ws[1], v, scratch=scratch)

        for M in args.m or MS:
            x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
            times = {v: [] for v in variants}
            for v in variants:                       # warm-up
                for i in range(2 * len(variants[v]) + 3):
                    call(v, x, i)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for v in variants:
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for i in range(args.iters):
                        call(v, x, i)
                    t1.record()
                    t1.synchronize()
                    times[v].append(t0.elapsed_time(t1) * 1e3 / args.iters)
            for v, ts in times.items():
                med, mn = statistics.median(ts), min(ts)
                rec = {"N": N, "K": K, "M": M, "variant": v,
                       "path": ("library" if v == "bf16" else
                                "fused" if M <= fused_max_m(v)
                                else "dequant+library"),
                       "us_median": round(med, 2), "us_min": round(mn, 2),
                       "weight_bytes": weight_bytes(v, N, K),
                       "weight_GBps": round(
                           weight_bytes(v, N, K) / med / 1e3, 1),
                       "speedup_vs_bf16": round(
                           statistics.median(times["bf16"]) / med, 3)}
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
        del variants, scratch
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
