"""LoRA adapters: HF-PEFT IO, packing onto the fused projections, and the
device-resident slot stacks the batched shrink/expand kernels read.

One base model serves many fine-tunes: every row of a batch names an
adapter *slot* (or -1), and `ops.lora_apply` adds that slot's low-rank
delta to the outputs of qkv_proj / o_proj / gate_up_proj / down_proj.

Per projection the manager owns two stacks (S = max_loras slots):

    A[S, n_slices * Rmax, K]     B[S, N, Rmax]

q/k/v are slices 0/1/2 of `attn.qkv_proj`, gate/up slices 0/1 of
`mlp.gate_up_proj` (the same packing as engine/weights.py:_map_hf_name);
an adapter of rank r < Rmax is zero-padded, a module the adapter does
not target is a zero slice.
"""
from __future__ import annotations

import json
import os
import re
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Tuple

import torch

# HF module -> (our sub-module, fused projection, slice index)
HF_TARGETS: Dict[str, Tuple[str, str, int]] = {
    "q_proj": ("attn", "qkv_proj", 0),
    "k_proj": ("attn", "qkv_proj", 1),
    "v_proj": ("attn", "qkv_proj", 2),
    "o_proj": ("attn", "o_proj", 0),
    "gate_proj": ("mlp", "gate_up_proj", 0),
    "up_proj": ("mlp", "gate_up_proj", 1),
    "down_proj": ("mlp", "down_proj", 0),
}
_HF_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn",
              "v_proj": "self_attn", "o_proj": "self_attn",
              "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
ALL_TARGETS = tuple(HF_TARGETS)
SUPPORTED_RANKS = (8, 16, 32, 64)
_KEY_RE = re.compile(
    r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\."
    r"(\w+)\.lora_([AB])\.weight$")


def proj_layout(cfg) -> Dict[str, Tuple[str, int, Tuple[int, ...]]]:
    """projection -> (sub-module, K, slice output widths)."""
    h, q, kv, i = (cfg.hidden_size, cfg.q_size, cfg.kv_size,
                   cfg.intermediate_size)
    return {
        "qkv_proj": ("attn", h, (q, kv, kv)),
        "o_proj": ("attn", q, (h,)),
        "gate_up_proj": ("mlp", h, (i, i)),
        "down_proj": ("mlp", i, (h,)),
    }


def _offsets(widths: Iterable[int]) -> Tuple[int, ...]:
    off = [0]
    for w in widths:
        off.append(off[-1] + w)
    return tuple(off)


def hf_key(layer: int, module: str, which: str) -> str:
    return (f"base_model.model.model.layers.{layer}.{_HF_PARENT[module]}."
            f"{module}.lora_{which}.weight")


def lora_stack_bytes(cfg, max_loras: int, max_lora_rank: int,
                     elem_bytes: int = 2) -> int:
    """Device bytes of the slot stacks for `max_loras` slots."""
    if max_loras <= 0:
        return 0
    per_layer = 0
    for _, K, widths in proj_layout(cfg).values():
        per_layer += len(widths) * max_lora_rank * K      # A
        per_layer += sum(widths) * max_lora_rank          # B
    return max_loras * (cfg.num_layers * per_layer * elem_bytes + 4)


# ---------------------------------------------------------------------------
# HF-PEFT adapter IO
# ---------------------------------------------------------------------------
def random_adapter_tensors(cfg, r: int, target_modules=ALL_TARGETS,
                           seed: int = 0, b_std: float = 0.05,
                           zero_b: bool = False) -> Dict[str, torch.Tensor]:
    """Seeded fp32 adapter tensors in HF-PEFT naming (lora_A [r, in],
    lora_B [out, r]) for every layer and target module."""
    g = torch.Generator().manual_seed(seed)
    layout = proj_layout(cfg)
    out: Dict[str, torch.Tensor] = {}
    for layer in range(cfg.num_layers):
        for mod in target_modules:
            _, proj, sl = HF_TARGETS[mod]
            _, K, widths = layout[proj]
            a = torch.randn(r, K, generator=g) / (K ** 0.5)
            b = torch.zeros(widths[sl], r) if zero_b else \
                torch.randn(widths[sl], r, generator=g) * b_std
            out[hf_key(layer, mod, "A")] = a
            out[hf_key(layer, mod, "B")] = b
    return out


def save_peft_adapter(out_dir: str, tensors: Dict[str, torch.Tensor],
                      r: int, lora_alpha: float,
                      target_modules=ALL_TARGETS) -> str:
    """Write an HF-PEFT adapter directory (adapter_config.json +
    adapter_model.safetensors): the inverse of load_peft_adapter."""
    from safetensors.torch import save_file
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": int(r),
                   "lora_alpha": float(lora_alpha),
                   "target_modules": list(target_modules)}, f)
    save_file({k: v.detach().cpu().contiguous() for k, v in tensors.items()},
              os.path.join(out_dir, "adapter_model.safetensors"))
    return out_dir


@dataclass
class LoRAAdapter:
    """One adapter packed for the slot stacks (CPU, fp32)."""
    r: int
    scale: float                    # lora_alpha / r
    # (layer, projection) -> (A [Rtot, K], B [N, Rmax]), zero-padded
    packed: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]] = \
        field(default_factory=dict)


def load_peft_adapter(adapter_dir: str, cfg,
                      max_lora_rank: int = 16) -> LoRAAdapter:
    """Read an HF-PEFT LoRA directory and pack it onto the fused
    projections of model config `cfg`, zero-padded to `max_lora_rank`."""
    from safetensors import safe_open
    cfg_path = os.path.join(adapter_dir, "adapter_config.json")
    st_path = os.path.join(adapter_dir, "adapter_model.safetensors")
    if not os.path.isfile(cfg_path) or not os.path.isfile(st_path):
        raise FileNotFoundError(
            f"{adapter_dir}: expected adapter_config.json and "
            "adapter_model.safetensors")
    with open(cfg_path) as f:
        acfg = json.load(f)
    r = int(acfg["r"])
    alpha = float(acfg.get("lora_alpha", r))
    targets = acfg.get("target_modules") or []
    if isinstance(targets, str):
        targets = [targets]
    if r < 1 or r > max_lora_rank:
        raise ValueError(
            f"adapter rank r={r} exceeds max_lora_rank={max_lora_rank}")
    bad = [t for t in targets if t not in HF_TARGETS]
    if bad:
        raise ValueError(
            f"unsupported LoRA target modules {bad}: only "
            f"{list(HF_TARGETS)} are supported (no embeddings / lm_head)")
    layout = proj_layout(cfg)
    R = max_lora_rank
    ad = LoRAAdapter(r=r, scale=alpha / r)
    for layer in range(cfg.num_layers):
        for proj, (_, K, widths) in layout.items():
            ad.packed[(layer, proj)] = (
                torch.zeros(len(widths) * R, K),
                torch.zeros(sum(widths), R))
    with safe_open(st_path, framework="pt", device="cpu") as f:
        for key in f.keys():
            m = _KEY_RE.match(key)
            if m is None or m.group(3) not in HF_TARGETS \
                    or _HF_PARENT[m.group(3)] != m.group(2):
                raise ValueError(f"unsupported adapter tensor {key!r}")
            layer, mod, which = int(m.group(1)), m.group(3), m.group(4)
            if mod not in targets:
                raise ValueError(
                    f"{key!r}: module not listed in target_modules")
            if layer >= cfg.num_layers:
                raise ValueError(
                    f"{key!r}: model {cfg.name} has {cfg.num_layers} layers")
            _, proj, sl = HF_TARGETS[mod]
            _, K, widths = layout[proj]
            off = _offsets(widths)
            t = f.get_tensor(key).float()
            A, B = ad.packed[(layer, proj)]
            if which == "A":
                if tuple(t.shape) != (r, K):
                    raise ValueError(
                        f"{key!r}: shape {tuple(t.shape)} != {(r, K)} for "
                        f"model {cfg.name}")
                A[sl * R:sl * R + r] = t
            else:
                if tuple(t.shape) != (widths[sl], r):
                    raise ValueError(
                        f"{key!r}: shape {tuple(t.shape)} != "
                        f"{(widths[sl], r)} for model {cfg.name}")
                B[off[sl]:off[sl + 1], :r] = t
    return ad


# ---------------------------------------------------------------------------
# Device-resident slot stacks
# ---------------------------------------------------------------------------
class LayerLoRA:
    """What Attention / MLP read: projection -> (A, B, n_off) plus the
    per-slot scale vector shared by the whole model."""

    def __init__(self, scale: torch.Tensor):
        self.scale = scale
        self.stacks: Dict[str, Tuple[torch.Tensor, torch.Tensor,
                                     Tuple[int, ...]]] = {}


class LoRAManager:
    """Owns the slot stacks, the name -> slot table (LRU eviction) and a
    per-name generation counter bumped on every (re)load, which seeds the
    prefix-cache hash chain so stale K/V is never shared."""

    def __init__(self, model, max_loras: int, max_lora_rank: int = 16):
        if max_lora_rank not in SUPPORTED_RANKS:
            raise ValueError(
                f"max_lora_rank must be one of {SUPPORTED_RANKS}, got "
                f"{max_lora_rank}")
        if max_loras < 1:
            raise ValueError("max_loras must be >= 1")
        self.cfg = model.cfg
        self.max_loras = max_loras
        self.max_lora_rank = max_lora_rank
        w = model.embed_tokens.weight
        self.device, self.dtype = w.device, w.dtype
        S, R = max_loras, max_lora_rank
        self.scale = torch.zeros(S, dtype=torch.float32, device=self.device)
        layout = proj_layout(self.cfg)
        for k_, (_, K, widths) in layout.items():
            if K % 8 or any(wd % 8 for wd in widths):
                raise ValueError(
                    f"{self.cfg.name}: {k_} dims must be multiples of 8")
        self.layers: List[Dict[str, LayerLoRA]] = []
        for layer in model.layers:
            per = {"attn": LayerLoRA(self.scale), "mlp": LayerLoRA(self.scale)}
            for proj, (sub, K, widths) in layout.items():
                A = torch.zeros(S, len(widths) * R, K, dtype=self.dtype,
                                device=self.device)
                B = torch.zeros(S, sum(widths), R, dtype=self.dtype,
                                device=self.device)
                per[sub].stacks[proj] = (A, B, _offsets(widths))
            layer.attn.lora = per["attn"]
            layer.mlp.lora = per["mlp"]
            self.layers.append(per)
        self.adapters: Dict[str, LoRAAdapter] = {}     # registered (CPU)
        self.generation: Dict[str, int] = {}           # survives removal
        self.slots: List[Optional[str]] = [None] * S   # slot -> name
        self._last_used = [0] * S
        self._clock = 0

    # -- registry -------------------------------------------------------
    def add(self, name: str, path: str):
        ad = load_peft_adapter(path, self.cfg, self.max_lora_rank)
        self._drop_slot(name)          # a reload must not serve old weights
        self.adapters[name] = ad
        self.generation[name] = self.generation.get(name, 0) + 1

    def remove(self, name: str):
        if name not in self.adapters:
            raise KeyError(name)
        del self.adapters[name]
        self._drop_slot(name)

    def names(self) -> List[str]:
        return sorted(self.adapters)

    def hash_seed(self, name: str) -> bytes:
        return f"{name}@{self.generation[name]}".encode()

    def memory_bytes(self) -> int:
        n = self.scale.numel() * 4
        for per in self.layers:
            for ll in per.values():
                for A, B, _ in ll.stacks.values():
                    n += A.numel() * A.element_size()
                    n += B.numel() * B.element_size()
        return n

    # -- slots ----------------------------------------------------------
    def slot_of(self, name: Optional[str]) -> int:
        """Resident slot of `name`, or -1."""
        if name is None:
            return -1
        try:
            return self.slots.index(name)
        except ValueError:
            return -1

    def _drop_slot(self, name: str):
        s = self.slot_of(name)
        if s >= 0:
            self.slots[s] = None

    def acquire(self, name: str, pinned: Iterable[str] = ()) -> int:
        """Make `name` resident and return its slot: reuse, else a free
        slot, else evict the least-recently-used slot whose adapter is
        not in `pinned`. Returns -1 when every slot is pinned."""
        self._clock += 1
        s = self.slot_of(name)
        if s >= 0:
            self._last_used[s] = self._clock
            return s
        pinned = set(pinned)
        free = [i for i, n in enumerate(self.slots) if n is None]
        if free:
            s = free[0]
        else:
            cand = [i for i, n in enumerate(self.slots) if n not in pinned]
            if not cand:
                return -1
            s = min(cand, key=lambda i: self._last_used[i])
        self._write_slot(s, self.adapters[name])
        self.slots[s] = name
        self._last_used[s] = self._clock
        return s

    @torch.inference_mode()
    def _write_slot(self, s: int, ad: LoRAAdapter):
        # Copies run on the current stream, so they are ordered before the
        # next forward / graph replay; the stacks keep their addresses.
        for layer, per in enumerate(self.layers):
            for ll in per.values():
                for proj, (A, B, _) in ll.stacks.items():
                    a, b = ad.packed[(layer, proj)]
                    A[s].copy_(a)
                    B[s].copy_(b)
        self.scale[s:s + 1].copy_(torch.tensor([ad.scale],
                                               dtype=torch.float32))
