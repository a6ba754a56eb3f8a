#!/usr/bin/env python
"""Qwen3 benchmark: the fused QK-norm + rope kernel against the unfused
composition, and (with --serving) decode throughput of the Qwen3 presets.

Kernel part, head configuration of qwen3-8b (32 / 8 / 128) unless given, at
T = 512 (a decode batch) and T = 8192 (a prefill chunk), bf16 paged cache:
  fused     ops.rope_qkv_cache with norm weights (ops/hip/rope_qkv_norm.hip)
  unfused   what serving QK-norm costs without that kernel: split Q and K
            with .contiguous(), ops.rms_norm on the [T*H, D] views, write
            back into qkv, then the un-normed ops.rope_qkv_cache
  floor     the un-normed ops.rope_qkv_cache alone (no QK-norm at all)
One JSON line per (T, path): median and min microseconds per call, and
fused_vs_unfused = unfused median / fused median.

Method: device events around a window of `--iters` back-to-back calls,
`--rounds` windows per path with the paths interleaved inside one process,
after a warm-up. Each call reads the next of several qkv buffers (together
more than the 256 MiB last-level cache), as a layer's fresh projection output
would be; all calls write the same cache slots.

--serving runs bench.py (the project's decode benchmark, unchanged) in a
child process per configuration: qwen3-8b at batch 64 and 512, llama3-8b at
batch 512, and repeats their JSON lines.

A GPU is required; there is no CPU fallback. Run under a time limit, e.g.
    timeout 600 python scripts/bench_qwen3.py --out qwen3.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import helix_amd.ops as ops  # noqa: E402

CACHE_BYTES = 512 << 20
SERVING = (("qwen3-8b", 64), ("qwen3-8b", 512), ("llama3-8b", 512))


def kernel_bench(args, lines):
    dev = torch.device("cuda:0")
    Hq, Hkv, D = args.heads, args.kv_heads, args.head_dim
    qs, ks = Hq * D, Hkv * D
    eps = 1e-6
    g = torch.Generator(device=dev).manual_seed(Hq + Hkv + D)
    cs = ops.make_cos_sin_cache(D, 40960, 1e6).to(dev)
    wq = (0.5 + torch.rand(D, generator=g, device=dev)).to(torch.bfloat16)
    wk = (0.5 + torch.rand(D, generator=g, device=dev)).to(torch.bfloat16)
    for T in args.t or (512, 8192):
        width = qs + 2 * ks
        copies = max(2, -(-CACHE_BYTES // (T * width * 2)))
        bufs = [torch.randn(T, width, generator=g, device=dev)
                .to(torch.bfloat16) for _ in range(copies)]
        pos = torch.randint(0, 40960, (T,), generator=g, device=dev)
        nblocks = -(-T // 16)
        cache = tuple(torch.zeros(nblocks, Hkv, 16, D, dtype=torch.bfloat16,
                                  device=dev) for _ in range(2))
        slots = torch.randperm(nblocks * 16, generator=g, device=dev)[:T]

        def fused(i):
            return ops.rope_qkv_cache(pos, bufs[i % copies], cs, Hq, Hkv, D,
                                      kv_cache=cache, slot_mapping=slots,
                                      q_norm_w=wq, k_norm_w=wk, eps=eps)

        def unfused(i):
            qkv = bufs[i % copies]
            q = qkv[:, :qs].contiguous()
            k = qkv[:, qs:qs + ks].contiguous()
            qn = ops.rms_norm(q.view(T * Hq, D), wq, eps)
            kn = ops.rms_norm(k.view(T * Hkv, D), wk, eps)
            qkv[:, :qs] = qn.view(T, qs)
            qkv[:, qs:qs + ks] = kn.view(T, ks)
            return ops.rope_qkv_cache(pos, qkv, cs, Hq, Hkv, D,
                                      kv_cache=cache, slot_mapping=slots)

        def floor(i):
            return ops.rope_qkv_cache(pos, bufs[i % copies], cs, Hq, Hkv, D,
                                      kv_cache=cache, slot_mapping=slots)

        # fused and unfused compute the same thing (bf16 rounding apart);
        # checked on a scratch copy, since unfused writes its input
        probe = bufs[0].clone()
        a = fused(0)[0].float()
        keep, bufs[0] = bufs[0], probe
        b = unfused(0)[0].float()
        bufs[0] = keep
        diff = float((a - b).abs().max() / b.abs().max())
        paths = {"fused": fused, "unfused": unfused, "floor": floor}
        for fn in paths.values():
            for i in range(copies + 3):
                fn(i)
        torch.cuda.synchronize()
        times = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, fn in paths.items():
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                for i in range(args.iters):
                    fn(i)
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        unf = statistics.median(times["unfused"])
        fus = statistics.median(times["fused"])
        for name, ts in times.items():
            rec = {"bench": "qknorm_kernel", "Hq": Hq, "Hkv": Hkv, "D": D,
                   "T": T, "path": name,
                   "us_median": round(statistics.median(ts), 1),
                   "us_min": round(min(ts), 1),
                   "fused_vs_unfused": round(unf / fus, 3),
                   "max_abs_diff_over_max": round(diff, 5)}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        del bufs, cache


def serving_bench(args, lines):
    for model, batch in SERVING:
        r = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
             "--model", model, "--batch", str(batch), "--steps",
             str(args.steps), "--warmup", str(args.warmup)],
            capture_output=True, text=True)
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not out:
            sys.exit(f"bench.py --model {model} --batch {batch} failed "
                     f"({r.returncode}):\n{r.stderr[-2000:]}")
        print(out[-1], flush=True)
        lines.append(out[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--t", type=int, action="append")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--serving", action="store_true",
                    help="run the decode benchmarks instead of the kernel one")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_qwen3.py needs a GPU")
    assert ops.have_native(), "native extension is not built"
    lines = []
    if args.serving:
        serving_bench(args, lines)
    else:
        kernel_bench(args, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
