"""Weight IO: safetensors load/save with HF-checkpoint name mapping and
pinned-host + side-stream async H2D staging (SURVEY.md §2.8 "Weight
load": replaces vLLM's HF download/load with a native path that does not
stall serving streams).
"""
from __future__ import annotations

import glob
import json
import logging
import os
from typing import Dict, Iterator, Tuple

import torch

log = logging.getLogger("helix_amd.weights")


def save_sharded(model: torch.nn.Module, out_dir: str,
                 shard_bytes: int = 4 << 30):
    """Save a model as safetensors shards (our native checkpoint format)."""
    from safetensors.torch import save_file
    os.makedirs(out_dir, exist_ok=True)
    shard: Dict[str, torch.Tensor] = {}
    size = 0
    idx = 0
    index = {}
    sd = model.state_dict()
    for name, t in sd.items():
        tb = t.detach().cpu().contiguous()
        shard[name] = tb
        size += tb.numel() * tb.element_size()
        if size >= shard_bytes:
            fn = f"model-{idx:05d}.safetensors"
            save_file(shard, os.path.join(out_dir, fn))
            for n in shard:
                index[n] = fn
            shard, size = {}, 0
            idx += 1
    if shard:
        fn = f"model-{idx:05d}.safetensors"
        save_file(shard, os.path.join(out_dir, fn))
        for n in shard:
            index[n] = fn
    with open(os.path.join(out_dir, "model.safetensors.index.json"),
              "w") as f:
        json.dump({"weight_map": index}, f)


def iter_safetensors(ckpt_dir: str) -> Iterator[Tuple[str, torch.Tensor]]:
    from safetensors import safe_open
    files = sorted(glob.glob(os.path.join(ckpt_dir, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no .safetensors under {ckpt_dir}")
    for path in files:
        with safe_open(path, framework="pt", device="cpu") as f:
            for name in f.keys():
                yield name, f.get_tensor(name)


# HF Llama checkpoint name -> (our param, role). Roles q/k/v and
# gate/up are packed into the fused projections.
def _map_hf_name(name: str):
    name = name.replace("model.", "")
    if name == "embed_tokens.weight":
        return "embed_tokens.weight", None
    if name == "norm.weight":
        return "final_norm_w", None
    if name == "lm_head.weight":
        return "lm_head.weight", None
    if name.startswith("layers."):
        parts = name.split(".")
        i = parts[1]
        rest = ".".join(parts[2:])
        m = {
            "input_layernorm.weight": (f"layers.{i}.input_norm_w", None),
            "post_attention_layernorm.weight":
                (f"layers.{i}.post_norm_w", None),
            "self_attn.q_proj.weight":
                (f"layers.{i}.attn.qkv_proj.weight", "q"),
            "self_attn.k_proj.weight":
                (f"layers.{i}.attn.qkv_proj.weight", "k"),
            "self_attn.v_proj.weight":
                (f"layers.{i}.attn.qkv_proj.weight", "v"),
            "self_attn.q_proj.bias":
                (f"layers.{i}.attn.qkv_proj.bias", "q"),
            "self_attn.k_proj.bias":
                (f"layers.{i}.attn.qkv_proj.bias", "k"),
            "self_attn.v_proj.bias":
                (f"layers.{i}.attn.qkv_proj.bias", "v"),
            "self_attn.o_proj.weight":
                (f"layers.{i}.attn.o_proj.weight", None),
            # Qwen3 QK-norm
            "self_attn.q_norm.weight": (f"layers.{i}.attn.q_norm_w", None),
            "self_attn.k_norm.weight": (f"layers.{i}.attn.k_norm_w", None),
            "mlp.gate_proj.weight":
                (f"layers.{i}.mlp.gate_up_proj.weight", "gate"),
            "mlp.up_proj.weight":
                (f"layers.{i}.mlp.gate_up_proj.weight", "up"),
            "mlp.down_proj.weight":
                (f"layers.{i}.mlp.down_proj.weight", None),
        }
        if rest in m:
            return m[rest]
        # HF Mixtral: block_sparse_moe.gate + experts.{e}.w1 (gate) / w3
        # (up) / w2 (down), packed into the stacked expert parameters; the
        # role carries the expert index
        if rest == "block_sparse_moe.gate.weight":
            return f"layers.{i}.mlp.router_w", None
        if len(parts) == 7 and parts[2:4] == ["block_sparse_moe", "experts"] \
                and parts[4].isdigit() and parts[6] == "weight" \
                and parts[5] in ("w1", "w2", "w3"):
            e = int(parts[4])
            if parts[5] == "w2":
                return f"layers.{i}.mlp.w2", ("expert_down", e)
            return (f"layers.{i}.mlp.w13",
                    ("expert_gate" if parts[5] == "w1" else "expert_up", e))
        # HF Qwen3-MoE: mlp.gate (the router) + mlp.experts.{e}.gate_proj /
        # up_proj / down_proj, the same packing under other names
        if rest == "mlp.gate.weight":
            return f"layers.{i}.mlp.router_w", None
        if len(parts) == 7 and parts[2:4] == ["mlp", "experts"] \
                and parts[4].isdigit() and parts[6] == "weight" \
                and parts[5] in ("gate_proj", "up_proj", "down_proj"):
            e = int(parts[4])
            if parts[5] == "down_proj":
                return f"layers.{i}.mlp.w2", ("expert_down", e)
            return (f"layers.{i}.mlp.w13",
                    ("expert_gate" if parts[5] == "gate_proj"
                     else "expert_up", e))
    return name, None  # our native names pass through


@torch.inference_mode()
def load_llama_weights(model, ckpt_dir: str, use_async: bool = True,
                       keep_quantized: bool = False):
    """Load a Llama checkpoint (HF layout or our native layout) into the
    model. On GPU, tensors are staged through a pinned-host buffer and
    copied on a side stream (hipMemcpyAsync) so decode streams on the
    default stream are not serialized behind weight traffic.
    keep_quantized applies to GGUF checkpoints only: Q4_0/Q8_0 and
    Q4_K/Q6_K projections stay resident as the file's blocks
    (engine/gguf.py)."""
    # GGUF checkpoints (llama.cpp ecosystem) route through the native
    # GGUF loader (engine/gguf.py): file path or a dir holding one.
    gguf_path = None
    if ckpt_dir.endswith(".gguf") and os.path.isfile(ckpt_dir):
        gguf_path = ckpt_dir
    elif os.path.isdir(ckpt_dir):
        ggufs = sorted(glob.glob(os.path.join(ckpt_dir, "*.gguf")))
        if ggufs and not glob.glob(os.path.join(ckpt_dir, "*.safetensors")):
            gguf_path = ggufs[0]
    if gguf_path is not None:
        from . import gguf as _gguf
        n = _gguf.load_gguf_weights(model, gguf_path,
                                    keep_quantized=keep_quantized)
        log.info("loaded %d tensors from GGUF %s", n, gguf_path)
        return n

    params = dict(model.named_parameters())
    cfg = model.cfg
    q, kv = cfg.q_size, cfg.kv_size
    inter = cfg.intermediate_size
    device = next(model.parameters()).device
    on_gpu = device.type == "cuda"
    side = torch.cuda.Stream(device) if (on_gpu and use_async) else None
    # Double-buffered pinned staging: wait on a buffer's event before
    # refilling it so the async copy out of it has completed.
    pinned = [None, None]
    events = [None, None]
    cur = 0

    def stage_copy(dst_view: torch.Tensor, src: torch.Tensor):
        nonlocal cur
        src = src.to(dst_view.dtype)
        if side is None:
            dst_view.copy_(src)
            return
        n = src.numel() * src.element_size()
        if pinned[cur] is None or pinned[cur].numel() < n:
            pinned[cur] = torch.empty(max(n, 64 << 20), dtype=torch.uint8,
                                      pin_memory=True)
            events[cur] = torch.cuda.Event()
        else:
            events[cur].synchronize()
        flat = pinned[cur][:n]
        flat.copy_(src.contiguous().view(-1).view(torch.uint8))
        with torch.cuda.stream(side):
            dst_view.view(-1).view(torch.uint8).copy_(flat,
                                                      non_blocking=True)
            events[cur].record(side)
        cur ^= 1

    loaded = 0
    for name, tensor in iter_safetensors(ckpt_dir):
        our, role = _map_hf_name(name)
        if our not in params:
            log.debug("skipping unknown weight %s", name)
            continue
        p = params[our]
        if role == "q":
            stage_copy(p.data[:q], tensor)
        elif role == "k":
            stage_copy(p.data[q:q + kv], tensor)
        elif role == "v":
            stage_copy(p.data[q + kv:], tensor)
        elif role == "gate":
            stage_copy(p.data[:inter], tensor)
        elif role == "up":
            stage_copy(p.data[inter:], tensor)
        elif isinstance(role, tuple):
            kind, e = role
            if not 0 <= e < p.shape[0]:
                raise ValueError(f"{name}: expert {e} but the model has "
                                 f"{p.shape[0]} experts")
            if kind == "expert_gate":
                stage_copy(p.data[e, :inter], tensor)
            elif kind == "expert_up":
                stage_copy(p.data[e, inter:], tensor)
            else:
                stage_copy(p.data[e], tensor)
        else:
            stage_copy(p.data, tensor)
        loaded += 1
    if side is not None:
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
    log.info("loaded %d tensors from %s", loaded, ckpt_dir)
    return loaded
