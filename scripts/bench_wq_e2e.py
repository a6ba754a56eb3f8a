#!/usr/bin/env python
"""End-to-end decode rate and resident weight bytes of one engine
configuration: --model, --batch (= max_num_seqs, all slots busy) and
--quant in {none, q8_0, q4_0}; a mixture-of-experts preset takes
--expert-quant in {none, q8_0, q4_0} instead (its experts alone are
quantised), or q4_k / q6_k / q4_k_m: the model is then built in bf16 on the
GPU, its experts are quantised layer by layer
(quant.quantize_model_experts_kq) and it is handed to the engine as it is.
Prints one JSON line.

One configuration per process, so every run starts from a cold allocator
and can carry its own time limit:
    timeout 300 python scripts/bench_wq_e2e.py --model llama3-8b \\
        --batch 64 --quant q4_0
Decode steps are timed with a host clock around work that ends in a device
synchronise, after the prefill and `--warmup` untimed steps (the first
replays load the captured graphs). A GPU is required.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helix_amd.engine.engine import EngineConfig, LLMEngine  # noqa: E402
from helix_amd.engine.sampling_params import SamplingParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--quant", default="none",
                    choices=["none", "q8_0", "q4_0"])
    ap.add_argument("--expert-quant", default="none",
                    choices=["none", "q8_0", "q4_0", "q4_k", "q6_k",
                             "q4_k_m"])
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_wq_e2e.py needs a GPU")
    max_len = args.prompt_len + args.warmup + args.steps + 64
    cfg = EngineConfig(
        model=args.model, max_num_seqs=args.batch, max_model_len=max_len,
        kv_cache_blocks=args.batch * (max_len // 16 + 2), eos_token_id=-1,
        quantization=None if args.quant == "none" else args.quant,
        expert_quantization=args.expert_quant
        if args.expert_quant in ("q8_0", "q4_0") else None)
    model = None
    if args.expert_quant in ("q4_k", "q6_k", "q4_k_m"):
        from helix_amd.models.llama import LlamaForCausalLM, get_preset
        from helix_amd.models.quant import quantize_model_experts_kq
        model = LlamaForCausalLM(get_preset(args.model)).to(torch.bfloat16) \
            .to("cuda:0")
        model.init_random(cfg.seed)
        quantize_model_experts_kq(model, args.expert_quant)
    eng = LLMEngine(cfg, device="cuda:0", model=model)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    model_bytes = sum(t.numel() * t.element_size() for t in
                      list(eng.model.parameters()) + list(eng.model.buffers()))
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(3, eng.model_cfg.vocab_size - 1,
                            (args.batch, args.prompt_len), generator=g)
    sp = SamplingParams(temperature=0.0, max_tokens=10 ** 9, ignore_eos=True)
    for i, p in enumerate(prompts.tolist()):
        eng.add_request(f"b-{i}", p, sp)
    while eng.waiting:
        eng.step()
    for _ in range(args.warmup):
        eng.step()
    torch.cuda.synchronize()
    t0 = time.monotonic()
    for _ in range(args.steps):
        eng.step()
    torch.cuda.synchronize()
    dt = time.monotonic() - t0
    print(json.dumps({
        "model": args.model, "batch": args.batch, "quant": args.quant,
        "expert_quant": args.expert_quant,
        "tok_per_s": round(args.batch * args.steps / dt, 1),
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "model_bytes": model_bytes,
        "allocated_bytes": torch.cuda.memory_allocated(),
        "graphs": eng.graph_runner is not None}), flush=True)


if __name__ == "__main__":
    main()
