#!/usr/bin/env python3
"""Multi-LoRA cost on an MI355X: kernel pair, decode step, prefill.

  kernels  us per shrink+expand pair at Llama-3-8B projection shapes, timed
           with device events. Run it once more under
           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`
           and feed the trace to `report` for per-kernel times.
  report   per-config kernel times + achieved bytes/s from a kernel trace.
  steps    ms/step of llama3-8b decode with max_loras=0, max_loras=4 with
           no row using an adapter, and max_loras=4 round-robin, the
           configurations alternating inside one process; plus prefill
           time for 8 x 1024-token prompts with and without adapters.

Outputs go to --out (default profiles/). Needs a GPU: nothing falls back.
"""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

S = 4                                    # adapter slots in the stacks
# Llama-3-8B projections: name -> (K, slice widths)
SHAPES = {
    "qkv": (4096, (4096, 1024, 1024)),
    "o": (4096, (4096,)),
    "gate_up": (4096, (14336, 14336)),
    "down": (14336, (4096,)),
}
PATTERNS = ("one", "rr4", "none")


def configs():
    for name, (K, widths) in SHAPES.items():
        for T in (64, 512):
            for r in (16, 64):
                for pat in PATTERNS:
                    yield {"proj": name, "K": K, "widths": list(widths),
                           "T": T, "r": r, "pattern": pat}


def algorithmic_bytes(c) -> int:
    """x + the A slice and B of every distinct slot + out read and written
    (what the pair must move once; y and the slot vector are left out)."""
    n_distinct = {"one": 1, "rr4": 4, "none": 0}[c["pattern"]]
    if n_distinct == 0:
        return 0
    N, ns = sum(c["widths"]), len(c["widths"])
    T, K, r = c["T"], c["K"], c["r"]
    return 2 * (T * K + n_distinct * (ns * r * K + N * r) + 2 * T * N)


def slot_vector(pattern: str, T: int) -> torch.Tensor:
    if pattern == "one":
        v = [1] * T
    elif pattern == "rr4":
        v = [t % 4 for t in range(T)]
    else:
        v = [-1] * T
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def need_gpu():
    import helix_amd.ops as ops
    if not torch.cuda.is_available() or not ops.have_native():
        sys.exit("bench_lora needs an MI355X and the built extension")
    return ops


def cmd_kernels(args):
    ops = need_gpu()
    torch.manual_seed(0)
    rows = []
    for c in configs():
        K, widths, T, r = c["K"], c["widths"], c["T"], c["r"]
        N, ns = sum(widths), len(widths)
        n_off = [0]
        for w in widths:
            n_off.append(n_off[-1] + w)
        x = torch.randn(T, K, device="cuda").bfloat16()
        A = (torch.randn(S, ns * r, K, device="cuda") / K ** 0.5).bfloat16()
        B = (torch.randn(S, N, r, device="cuda") / r ** 0.5).bfloat16()
        out = torch.randn(T, N, device="cuda").bfloat16()
        y = torch.empty(T, ns * r, device="cuda")
        scale = torch.full((S,), 0.01, device="cuda")
        slot = slot_vector(c["pattern"], T)

        def pair():
            ops.lora_shrink(y, x, A, slot)
            ops.lora_expand(out, y, B, slot, scale, n_off)

        for _ in range(args.warmup):
            pair()
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            pair()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / args.iters
        nbytes = algorithmic_bytes(c)
        rows.append({**c, "pair_us_events": round(us, 2),
                     "alg_bytes": nbytes,
                     "alg_TBps_events": (round(nbytes / us / 1e6, 3)
                                         if nbytes else None)})
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "lora_kernels_events.json"), "w") as f:
        json.dump({"warmup": args.warmup, "iters": args.iters,
                   "rows": rows}, f, indent=1)


def cmd_report(args):
    """The kernels run launches, per config and in order, (warmup + iters)
    shrink kernels and as many expand kernels; cut the trace accordingly."""
    paths = glob.glob(os.path.join(args.trace_dir, "**",
                                   "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {args.trace_dir}")
    dur = {"shrink": [], "expand": []}
    recs = []
    for p in paths:
        with open(p) as f:
            recs.extend(csv.DictReader(f))
    recs.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in recs:
        name = r["Kernel_Name"]
        for k in dur:
            if f"lora_{k}_kernel" in name:
                dur[k].append((int(r["End_Timestamp"])
                               - int(r["Start_Timestamp"])) / 1000.0)
    per = args.warmup + args.iters
    cfgs = list(configs())
    for k in dur:
        if len(dur[k]) != per * len(cfgs):
            sys.exit(f"{k}: {len(dur[k])} launches in the trace, expected "
                     f"{per * len(cfgs)} (same --warmup/--iters?)")
    rows = []
    for i, c in enumerate(cfgs):
        sh = dur["shrink"][i * per + args.warmup:(i + 1) * per]
        ex = dur["expand"][i * per + args.warmup:(i + 1) * per]
        sh_us, ex_us = sum(sh) / len(sh), sum(ex) / len(ex)
        nbytes = algorithmic_bytes(c)
        rows.append({**c, "shrink_us": round(sh_us, 2),
                     "expand_us": round(ex_us, 2),
                     "pair_us": round(sh_us + ex_us, 2),
                     "alg_bytes": nbytes,
                     "alg_TBps": (round(nbytes / (sh_us + ex_us) / 1e6, 3)
                                  if nbytes else None)})
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "lora_kernels_trace.json"), "w") as f:
        json.dump({"warmup": args.warmup, "iters": args.iters,
                   "rows": rows}, f, indent=1)
    print("| proj | T | r | slots | shrink us | expand us | pair us | "
          "alg MB | alg TB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['proj']} | {r['T']} | {r['r']} | {r['pattern']} | "
              f"{r['shrink_us']} | {r['expand_us']} | {r['pair_us']} | "
              f"{r['alg_bytes'] / 1e6:.1f} | {r['alg_TBps'] or '-'} |")


def cmd_steps(args):
    need_gpu()
    from helix_amd.engine.engine import EngineConfig, LLMEngine
    from helix_amd.engine.sampling_params import SamplingParams
    from helix_amd.models import lora as L
    from helix_amd.models.llama import LlamaForCausalLM, PRESETS

    mcfg = PRESETS[args.model]
    dev = args.device
    with torch.device(dev):
        model = LlamaForCausalLM(mcfg)
    model = model.to(torch.bfloat16).to(dev)
    model.init_random(0)
    torch.cuda.empty_cache()

    max_b = max(args.batches)
    max_len = max(args.prompt_len + args.warmup + args.steps + 64, 1024 + 64)
    blocks = max(max_b * (args.prompt_len + args.warmup + args.steps) // 16
                 + 2 * max_b, 8 * 1100 // 16) + 64

    def engine(max_loras):
        return LLMEngine(EngineConfig(
            model=args.model, max_num_seqs=max_b, max_model_len=max_len,
            max_prefill_tokens=16384, eos_token_id=-1, seed=0,
            kv_cache_blocks=blocks, enable_prefix_caching=False,
            max_loras=max_loras, max_lora_rank=args.rank),
            device=dev, model=model)

    # One model serves both engines: without lora_slots on the meta the
    # hooks are no-ops, so the max_loras=0 engine runs the base sequence.
    eng0 = engine(0)
    eng4 = engine(4)
    names = [f"a{i}" for i in range(4)]
    with tempfile.TemporaryDirectory() as d:
        for i, n in enumerate(names):
            t = L.random_adapter_tensors(mcfg, args.rank, seed=i + 1,
                                         b_std=0.01)
            L.save_peft_adapter(os.path.join(d, n), t, r=args.rank,
                                lora_alpha=args.rank)
            eng4.add_lora(n, os.path.join(d, n))
    sp = SamplingParams(temperature=0.0, max_tokens=10 ** 9, ignore_eos=True)
    gen = torch.Generator().manual_seed(1234)
    run_no = [0]

    def measure(eng, B, plen, loras, steps, warmup):
        """-> (prefill_s, ms_per_step)."""
        run_no[0] += 1
        prompts = torch.randint(3, mcfg.vocab_size - 1, (B, plen),
                                generator=gen).tolist()
        ids = [f"r{run_no[0]}-{i}" for i in range(B)]
        torch.cuda.synchronize()
        t0 = time.monotonic()
        for i, (sid, p) in enumerate(zip(ids, prompts)):
            eng.add_request(sid, p, sp,
                            lora=loras[i % len(loras)] if loras else None)
        while eng.waiting:
            eng.step()
        torch.cuda.synchronize()
        prefill_s = time.monotonic() - t0
        ms = None
        if steps:
            for _ in range(warmup):
                eng.step()
            torch.cuda.synchronize()
            t0 = time.monotonic()
            for _ in range(steps):
                eng.step()
            torch.cuda.synchronize()
            ms = (time.monotonic() - t0) / steps * 1000
        for sid in ids:
            eng.cancel(sid)
        return prefill_s, ms

    variants = [("max_loras=0", eng0, None),
                ("max_loras=4, no adapter rows", eng4, None),
                ("max_loras=4, round-robin", eng4, names)]
    res = {"model": args.model, "rank": args.rank,
           "prompt_len": args.prompt_len, "steps": args.steps,
           "warmup": args.warmup, "decode": [], "prefill_8x1024": []}
    for B in args.batches:
        # untimed pass: graph capture, adapter loads, library heuristics
        for _, eng, loras in variants:
            measure(eng, B, args.prompt_len, loras, 4, 2)
        for rep in range(args.repeats):
            for label, eng, loras in variants:
                _, ms = measure(eng, B, args.prompt_len, loras, args.steps,
                                args.warmup)
                row = {"B": B, "config": label, "repeat": rep,
                       "ms_per_step": round(ms, 3)}
                res["decode"].append(row)
                print(json.dumps(row), flush=True)
    for _, eng, loras in variants:
        measure(eng, 8, 1024, loras, 0, 0)                     # untimed
    for rep in range(args.repeats):
        for label, eng, loras in variants:
            pf, _ = measure(eng, 8, 1024, loras, 0, 0)
            row = {"config": label, "repeat": rep,
                   "prefill_ms": round(pf * 1000, 2)}
            res["prefill_8x1024"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "lora_steps.json"), "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--iters", type=int, default=20)
    k.add_argument("--warmup", type=int, default=3)
    r = sub.add_parser("report")
    r.add_argument("trace_dir")
    r.add_argument("--iters", type=int, default=20)
    r.add_argument("--warmup", type=int, default=3)
    s = sub.add_parser("steps")
    s.add_argument("--model", default="llama3-8b")
    s.add_argument("--device", default="cuda:0")
    s.add_argument("--batches", type=int, nargs="+", default=[64, 512])
    s.add_argument("--prompt-len", type=int, default=512)
    s.add_argument("--rank", type=int, default=16)
    s.add_argument("--steps", type=int, default=100)
    s.add_argument("--warmup", type=int, default=8)
    s.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    {"kernels": cmd_kernels, "report": cmd_report,
     "steps": cmd_steps}[args.cmd](args)


if __name__ == "__main__":
    main()
