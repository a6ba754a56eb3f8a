"""Llama-family decoder (Llama-3 8B/70B, Mistral-7B) on helix_amd CDNA4 ops.

Replaces the model execution the reference delegates to vLLM containers
(SURVEY.md §2.8): hand-written HIP kernels for RMSNorm/RoPE/attention/
activation; plain projection GEMMs via hipBLASLt (torch.linear); paged KV.

Tensor-parallel sharding (RCCL over xGMI) is applied by
helix_amd.parallel when tp_size > 1: column-parallel QKV/gate_up,
row-parallel o_proj/down_proj with all-reduce.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from helix_amd import ops
from helix_amd.ops import make_cos_sin_cache


@dataclass
class LlamaConfig:
    name: str = "llama3-8b"
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    rms_norm_eps: float = 1e-5
    rope_base: float = 500000.0
    max_position: int = 8192
    tie_embeddings: bool = False
    sliding_window: int = 0        # 0 = full attention (Mistral v0.1: 4096)
    attention_bias: bool = False   # Qwen2-style QKV bias
    rope_scaling: dict = field(default_factory=dict)  # llama3.1 scheme
    num_experts: int = 0           # 0 = dense MLP; > 0 = Mixtral-style MoE
    experts_per_token: int = 2
    qk_norm: bool = False          # Qwen3: per-head RMSNorm of Q and K

    @property
    def q_size(self) -> int:
        return self.num_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.num_kv_heads * self.head_dim


PRESETS = {
    "llama3-8b": LlamaConfig(),
    # Llama-3.1: same weights shape as 3.0 but 128k context via the
    # llama3 rope-scaling scheme (HF config.json rope_scaling)
    "llama3.1-8b": LlamaConfig(
        name="llama3.1-8b", max_position=32768, rope_base=500000.0,
        rope_scaling={"rope_type": "llama3", "factor": 8.0,
                      "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                      "original_max_position_embeddings": 8192}),
    "llama3-70b": LlamaConfig(
        name="llama3-70b", hidden_size=8192, intermediate_size=28672,
        num_layers=80, num_heads=64, num_kv_heads=8),
    "mistral-7b": LlamaConfig(
        name="mistral-7b", vocab_size=32000, rope_base=10000.0,
        sliding_window=4096),
    # Tiny configs for CPU tests and smoke runs.
    "tiny": LlamaConfig(
        name="tiny", vocab_size=512, hidden_size=256, intermediate_size=512,
        num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64,
        max_position=512, rope_base=10000.0),
    "tiny-gqa": LlamaConfig(
        name="tiny-gqa", vocab_size=1024, hidden_size=512,
        intermediate_size=1024, num_layers=4, num_heads=8, num_kv_heads=2,
        head_dim=64, max_position=1024, rope_base=10000.0),
    "qwen2-7b": LlamaConfig(
        name="qwen2-7b", vocab_size=152064, hidden_size=3584,
        intermediate_size=18944, num_layers=28, num_heads=28,
        num_kv_heads=4, head_dim=128, rope_base=1000000.0,
        max_position=32768, attention_bias=True),
    "tiny-qwen": LlamaConfig(
        name="tiny-qwen", vocab_size=512, hidden_size=256,
        intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=64, max_position=512, rope_base=10000.0,
        attention_bias=True),
    "tiny-sw": LlamaConfig(
        name="tiny-sw", vocab_size=512, hidden_size=256,
        intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=64, max_position=512, rope_base=10000.0,
        sliding_window=24),
    # Mixtral-8x7B (v0.1): 8 SwiGLU experts per layer, top-2 routing, no
    # sliding window
    "mixtral-8x7b": LlamaConfig(
        name="mixtral-8x7b", vocab_size=32000, hidden_size=4096,
        intermediate_size=14336, num_layers=32, num_heads=32, num_kv_heads=8,
        head_dim=128, rope_base=1000000.0, max_position=32768,
        num_experts=8, experts_per_token=2),
    "tiny-moe": LlamaConfig(
        name="tiny-moe", vocab_size=512, hidden_size=256,
        intermediate_size=256, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=64, max_position=512, rope_base=10000.0,
        num_experts=8, experts_per_token=2),
    # Qwen3: QK-norm, no QKV bias, head_dim 128 independent of hidden_size
    "qwen3-8b": LlamaConfig(
        name="qwen3-8b", vocab_size=151936, hidden_size=4096,
        intermediate_size=12288, num_layers=36, num_heads=32, num_kv_heads=8,
        head_dim=128, rms_norm_eps=1e-6, rope_base=1000000.0,
        max_position=40960, qk_norm=True),
    "qwen3-32b": LlamaConfig(
        name="qwen3-32b", vocab_size=151936, hidden_size=5120,
        intermediate_size=25600, num_layers=64, num_heads=64, num_kv_heads=8,
        head_dim=128, rms_norm_eps=1e-6, rope_base=1000000.0,
        max_position=40960, qk_norm=True),
    # q_size 512 != hidden 256, head_dim 128
    "tiny-qwen3": LlamaConfig(
        name="tiny-qwen3", vocab_size=512, hidden_size=256,
        intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=128, max_position=512, rope_base=10000.0, qk_norm=True),
}

# Qwen3's mixtures of experts. PRESETS stays the dense families plus the
# Mixtral pair; get_preset() resolves a name in either table, and the engine,
# the runner and the CLI look presets up through it.
QWEN3_MOE_PRESETS = {
    # Qwen3-30B-A3B: Mixtral's routing at 128 experts, top-8, with Qwen3's
    # attention; intermediate_size is per expert. The published HF config as
    # remembered, not yet checked against a real checkpoint.
    "qwen3-30b-a3b": LlamaConfig(
        name="qwen3-30b-a3b", vocab_size=151936, hidden_size=2048,
        intermediate_size=768, num_layers=48, num_heads=32, num_kv_heads=4,
        head_dim=128, rms_norm_eps=1e-6, rope_base=1000000.0,
        max_position=40960, qk_norm=True, num_experts=128,
        experts_per_token=8),
    # hidden and intermediate are multiples of 256: the experts can hold
    # K-quant super-blocks
    "tiny-qwen3-moe": LlamaConfig(
        name="tiny-qwen3-moe", vocab_size=512, hidden_size=256,
        intermediate_size=256, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=128, max_position=512, rope_base=10000.0, qk_norm=True,
        num_experts=16, experts_per_token=4),
}


def get_preset(name: str) -> LlamaConfig:
    """The LlamaConfig of a preset name, from PRESETS or QWEN3_MOE_PRESETS."""
    if name in QWEN3_MOE_PRESETS:
        return QWEN3_MOE_PRESETS[name]
    return PRESETS[name]


@dataclass
class PrefillMeta:
    """Varlen prefill: q/k/v are concatenated new tokens of all sequences.
    With prefix caching, q covers only the uncached suffix; attention
    gathers the full context K/V from the paged cache (gather_blk/off)
    and cu_seqlens_k carries the full-context boundaries."""
    cu_seqlens: torch.Tensor       # [B+1] int32 (new-token boundaries)
    max_seqlen: int
    slot_mapping: torch.Tensor     # [T] int64 cache slots for new tokens
    positions: torch.Tensor        # [T] int64
    cu_seqlens_k: Optional[torch.Tensor] = None   # [B+1] int32 full context
    gather_blk: Optional[torch.Tensor] = None     # [Tk] int64
    gather_off: Optional[torch.Tensor] = None     # [Tk] int64
    is_prefill: bool = True
    lora_slots: Optional[torch.Tensor] = None     # [T] int32, -1 = none


@dataclass
class DecodeMeta:
    """One new token per running sequence."""
    block_tables: torch.Tensor     # [B, max_blocks] int32
    seq_lens: torch.Tensor         # [B] int32 (context incl. current token)
    slot_mapping: torch.Tensor     # [B] int64
    positions: torch.Tensor        # [B] int64
    max_len: int = 0               # host-side max(seq_lens) (avoids sync)
    workspace: Optional[tuple] = None
    is_prefill: bool = False
    lora_slots: Optional[torch.Tensor] = None     # [B] int32, -1 = none


class HLinear(nn.Linear):
    """nn.Linear routed through ops.linear: decode-shaped (skinny-M)
    GEMMs run the owned split-K MFMA kernel, prefill-shaped ones stay on
    hipBLASLt (SURVEY §2.8 'Q/K/V + O projections, MLP GEMMs')."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear(x, self.weight, self.bias)


def _lora(out: torch.Tensor, x: torch.Tensor, lora, proj: str, meta):
    """Per-row adapter delta on a projection's output (models/lora.py).
    A no-op unless the module has adapter stacks AND the step names
    slots, so a model without a manager issues today's kernel sequence."""
    slots = getattr(meta, "lora_slots", None)
    if lora is None or slots is None:
        return out
    A, B, n_off = lora.stacks[proj]
    if not out.is_contiguous():
        out = out.contiguous()
    return ops.lora_apply(out, x, A, B, slots, lora.scale, n_off)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp_size: int = 1, tp_rank: int = 0):
        super().__init__()
        self.cfg = cfg
        assert cfg.num_heads % tp_size == 0 and cfg.num_kv_heads % tp_size == 0
        self.nh = cfg.num_heads // tp_size
        self.nkv = cfg.num_kv_heads // tp_size
        self.hd = cfg.head_dim
        self.scale = self.hd ** -0.5
        self.tp_size = tp_size
        self.window = cfg.sliding_window or 0
        q, kv, h = self.nh * self.hd, self.nkv * self.hd, cfg.hidden_size
        self.qkv_proj = HLinear(h, q + 2 * kv, bias=cfg.attention_bias)
        self.o_proj = HLinear(q, h, bias=False)
        self.lora = None               # LayerLoRA, set by LoRAManager
        # Qwen3 QK-norm: one [head_dim] weight shared by all Q heads, one
        # by all K heads; replicated under tensor parallelism
        self.eps = cfg.rms_norm_eps
        if cfg.qk_norm:
            self.q_norm_w = nn.Parameter(torch.ones(self.hd))
            self.k_norm_w = nn.Parameter(torch.ones(self.hd))
        else:
            self.q_norm_w = self.k_norm_w = None

    def forward(self, x: torch.Tensor, cos_sin: torch.Tensor, kv_cache,
                meta) -> torch.Tensor:
        T = x.shape[0]
        qkv = _lora(self.qkv_proj(x), x, self.lora, "qkv_proj", meta)
        # fused strided split + rope + paged-cache write (one kernel, no
        # .contiguous() copies); compact K/V emitted only when the
        # fresh-prefill attention path consumes them directly
        want_kv = meta.is_prefill and \
            getattr(meta, "cu_seqlens_k", None) is None
        q, k, v = ops.rope_qkv_cache(
            meta.positions, qkv, cos_sin, self.nh, self.nkv, self.hd,
            kv_cache=kv_cache, slot_mapping=meta.slot_mapping,
            want_kv=want_kv, q_norm_w=self.q_norm_w,
            k_norm_w=self.k_norm_w,
            eps=self.eps if self.q_norm_w is not None else 0.0)
        if meta.is_prefill:
            if meta.cu_seqlens_k is not None:
                # cached-prefix prefill: full-context K/V gathered from
                # the paged cache (new tokens were just written above)
                k_cache, v_cache = kv_cache
                k_all = k_cache[meta.gather_blk, :, meta.gather_off]
                v_all = v_cache[meta.gather_blk, :, meta.gather_off]
                if k_all.dtype == torch.uint8:      # fp8 KV cache
                    k_all = ops.kv_fp8_dequant(k_all, q.dtype)
                    v_all = ops.kv_fp8_dequant(v_all, q.dtype)
                o = ops.attn_prefill(q, k_all, v_all, meta.cu_seqlens,
                                     meta.max_seqlen, self.scale,
                                     window=self.window,
                                     cu_seqlens_k=meta.cu_seqlens_k)
            else:
                o = ops.attn_prefill(q, k, v, meta.cu_seqlens,
                                     meta.max_seqlen, self.scale,
                                     window=self.window)
        else:
            k_cache, v_cache = kv_cache
            o = ops.paged_attn_decode(q, k_cache, v_cache, meta.block_tables,
                                      meta.seq_lens, self.scale,
                                      meta.workspace,
                                      meta.max_len or None,
                                      window=self.window)
        o = o.view(T, -1)
        out = _lora(self.o_proj(o), o, self.lora, "o_proj", meta)
        if self.tp_size > 1:
            from helix_amd import parallel
            out = parallel.tp_all_reduce(out)
        return out


class MLP(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp_size: int = 1):
        super().__init__()
        assert cfg.intermediate_size % tp_size == 0
        self.tp_size = tp_size
        i = cfg.intermediate_size // tp_size
        self.gate_up_proj = HLinear(cfg.hidden_size, 2 * i, bias=False)
        self.down_proj = HLinear(i, cfg.hidden_size, bias=False)
        self.lora = None               # LayerLoRA, set by LoRAManager

    def forward(self, x: torch.Tensor, meta=None) -> torch.Tensor:
        if self.lora is None or getattr(meta, "lora_slots", None) is None:
            out = self.down_proj(ops.silu_and_mul(self.gate_up_proj(x)))
        else:
            gu = _lora(self.gate_up_proj(x), x, self.lora, "gate_up_proj",
                       meta)
            act = ops.silu_and_mul(gu)
            out = _lora(self.down_proj(act), act, self.lora, "down_proj",
                        meta)
        if self.tp_size > 1:
            from helix_amd import parallel
            out = parallel.tp_all_reduce(out)
        return out


# plane names of a K-quant expert stack, in ops.moe_experts_kq's order
_KQ_PLANES = {"q4_k": ("qs", "hdr"), "q6_k": ("ql", "qh", "sc", "d")}


class MoEMLP(nn.Module):
    """Mixtral-style sparse MLP: a router over E SwiGLU experts, the top
    `experts_per_token` of them per token (ops.moe_forward). The weights are
    plain Parameters, not nn.Linear, so the quantisers' and the LoRA
    manager's nn.Linear walks never see them; expert weights are neither
    adapted nor sharded.

    Quantised state (set_quantized_experts; models/quant.py
    quantize_model_experts or a resident GGUF load): the bf16 `w13` / `w2`
    Parameters are deleted and the experts live as ggml Q4_0/Q8_0 planes in
    the buffers `w13_qs`, `w13_d`, `w2_qs`, `w2_d`, with `expert_fmt` the
    (w13 format, w2 format) pair; forward runs ops.moe_forward_wq. The
    router stays a bf16 F.linear. `scratch` is the model's dequant buffer
    for the eager library prefill path (quant.attach_wq_scratch).

    K-quant state (set_kquant_experts; quant.quantize_model_experts_kq or a
    resident load of a Q4_K_M file): the same, with ggml Q4_K/Q6_K planes in
    the buffers `w13_<plane>` / `w2_<plane>` and forward running
    ops.moe_forward_kq. The two families do not mix inside one layer."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        e, h, i = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
        self.k = cfg.experts_per_token
        self.num_experts, self.hidden_size, self.intermediate_size = e, h, i
        self.expert_fmt = None
        self.scratch = None
        # created in bf16, the one dtype the kernels serve: mixtral-8x7b's
        # 45 G expert weights never exist in fp32, on the host or the GPU
        bf16 = torch.bfloat16
        self.router_w = nn.Parameter(torch.empty(e, h, dtype=bf16))
        # gate rows [:I], up rows [I:]
        self.w13 = nn.Parameter(torch.empty(e, 2 * i, h, dtype=bf16))
        self.w2 = nn.Parameter(torch.empty(e, h, i, dtype=bf16))

    def forward(self, x: torch.Tensor, meta=None) -> torch.Tensor:
        router_logits = F.linear(x, self.router_w)
        # decode runs under hipGraph capture: always the fused kernels there
        fused = True if not getattr(meta, "is_prefill", True) else None
        if self.expert_fmt is not None and self.expert_fmt[0] in _KQ_PLANES:
            return ops.moe_forward_kq(x, router_logits,
                                      self.expert_planes("w13"),
                                      self.expert_planes("w2"),
                                      self.expert_fmt, self.k, fused=fused,
                                      scratch=self.scratch)
        if self.expert_fmt is not None:
            return ops.moe_forward_wq(x, router_logits,
                                      (self.w13_qs, self.w13_d),
                                      (self.w2_qs, self.w2_d),
                                      self.expert_fmt, self.k, fused=fused,
                                      scratch=self.scratch)
        return ops.moe_forward(x, router_logits, self.w13, self.w2, self.k,
                               fused=fused)

    def set_quantized_experts(self, w13_planes, w2_planes, fmt) -> None:
        """Replace the bf16 experts by (qs, d) planes of the given format
        ("q4_0" / "q8_0", or a (w13, w2) pair). Shapes are checked against
        the config; the bf16 Parameters are deleted."""
        f13, f2 = (fmt, fmt) if isinstance(fmt, str) else tuple(fmt)
        e, h, i = self.num_experts, self.hidden_size, self.intermediate_size
        for name, (qs, d), f, rows, k in (
                ("w13", w13_planes, f13, 2 * i, h),
                ("w2", w2_planes, f2, h, i)):
            bits = ops.wq_bits(f)
            qdt = torch.uint8 if bits == 4 else torch.int8
            qshape = (e, rows, k // 2 if bits == 4 else k)
            if qs.dtype != qdt or tuple(qs.shape) != qshape \
                    or d.dtype != torch.float16 \
                    or tuple(d.shape) != (e, rows, k // 32):
                raise ValueError(
                    f"MoEMLP: {name} {f} planes are {qs.dtype} "
                    f"{tuple(qs.shape)} / {d.dtype} {tuple(d.shape)}, "
                    f"expected {qdt} {qshape} / fp16 {(e, rows, k // 32)}")
        for name in ("w13", "w2"):
            if name in self._parameters:
                del self._parameters[name]
        for name, t in (("w13_qs", w13_planes[0]), ("w13_d", w13_planes[1]),
                        ("w2_qs", w2_planes[0]), ("w2_d", w2_planes[1])):
            self._buffers.pop(name, None)
            self.register_buffer(name, t.contiguous(), persistent=True)
        self.expert_fmt = (f13, f2)

    def set_kquant_experts(self, w13_planes, w2_planes, fmt) -> None:
        """Replace the bf16 experts by ggml K-quant planes ("q4_k" / "q6_k",
        or a (w13, w2) pair; ops.moe_experts_kq has the plane shapes). Shapes
        are checked against the config; the bf16 Parameters are deleted. The
        planes become the buffers `w13_<plane>` / `w2_<plane>` (q4_k: qs,
        hdr; q6_k: ql, qh, sc, d)."""
        f13, f2 = (fmt, fmt) if isinstance(fmt, str) else tuple(fmt)
        e, h, i = self.num_experts, self.hidden_size, self.intermediate_size
        if h % 256 or i % 256:
            raise ValueError(f"MoEMLP: K-quant experts need hidden ({h}) and "
                             f"intermediate ({i}) sizes that are multiples "
                             f"of 256")
        stacks = (("w13", tuple(w13_planes), f13, 2 * i, h),
                  ("w2", tuple(w2_planes), f2, h, i))
        for name, planes, f, rows, k in stacks:
            ops.kq_check(f)
            if f == "q4_k":
                want = ((torch.uint8, (e, rows, k // 2)),
                        (torch.uint8, (e, rows, k // 256, 16)))
            else:
                want = ((torch.uint8, (e, rows, k // 2)),
                        (torch.uint8, (e, rows, k // 4)),
                        (torch.int8, (e, rows, k // 16)),
                        (torch.float16, (e, rows, k // 256)))
            got = tuple((p.dtype, tuple(p.shape)) for p in planes)
            if got != want:
                raise ValueError(f"MoEMLP: {name} {f} planes are {got}, "
                                 f"expected {want}")
        for name in ("w13", "w2"):
            if name in self._parameters:
                del self._parameters[name]
        for name, planes, f, _, _ in stacks:
            for stale in [b for b in self._buffers
                          if b.startswith(name + "_")]:
                del self._buffers[stale]
            for pn, t in zip(_KQ_PLANES[f], planes):
                self.register_buffer(f"{name}_{pn}", t.contiguous(),
                                     persistent=True)
        self.expert_fmt = (f13, f2)

    def expert_planes(self, name: str):
        """The quantised state's planes of stack "w13" or "w2", in their
        format's order."""
        f = self.expert_fmt[0 if name == "w13" else 1]
        names = _KQ_PLANES.get(f, ("qs", "d"))
        return tuple(self._buffers[f"{name}_{pn}"] for pn in names)

    def _apply(self, fn, recurse=True):
        # as WQLinear._apply: the fp16 scale planes (Q4_0/Q8_0 block scales,
        # Q6_K's super-block `d`) are fp16 by format and follow the device
        # only under model.to(dtype); a scratch left on another device is
        # dropped (attach_wq_scratch gives the model a new one)
        if self.expert_fmt is None:
            return super()._apply(fn, recurse)
        keep = {n: self._buffers[n] for n in ("w13_d", "w2_d")
                if n in self._buffers}
        super()._apply(fn, recurse)
        for n, b in keep.items():
            if self._buffers[n].dtype != torch.float16:
                self._buffers[n] = b.to(self._buffers[n].device)
        if self.scratch is not None \
                and self.scratch.device != self.expert_planes("w13")[0].device:
            self.scratch = None
        return self


class DecoderLayer(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp_size: int = 1, tp_rank: int = 0):
        super().__init__()
        self.input_norm_w = nn.Parameter(torch.ones(cfg.hidden_size))
        self.post_norm_w = nn.Parameter(torch.ones(cfg.hidden_size))
        self.attn = Attention(cfg, tp_size, tp_rank)
        self.mlp = MoEMLP(cfg) if cfg.num_experts > 0 else MLP(cfg, tp_size)
        self.eps = cfg.rms_norm_eps

    def forward(self, x, residual, cos_sin, kv_cache, meta):
        if residual is None:
            residual = x.clone()
            h = ops.rms_norm(x, self.input_norm_w, self.eps)
        else:
            h, residual = ops.fused_add_rms_norm(x, residual,
                                                 self.input_norm_w, self.eps)
        h = self.attn(h, cos_sin, kv_cache, meta)
        h, residual = ops.fused_add_rms_norm(h, residual, self.post_norm_w,
                                             self.eps)
        h = self.mlp(h, meta)
        return h, residual


class LlamaForCausalLM(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp_size: int = 1, tp_rank: int = 0):
        super().__init__()
        self.cfg = cfg
        self.tp_size = tp_size
        self.tp_rank = tp_rank
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList(
            [DecoderLayer(cfg, tp_size, tp_rank) for _ in range(cfg.num_layers)])
        self.final_norm_w = nn.Parameter(torch.ones(cfg.hidden_size))
        if cfg.tie_embeddings:
            self.lm_head = None
        else:
            self.lm_head = HLinear(cfg.hidden_size, cfg.vocab_size,
                                   bias=False)
        cs = make_cos_sin_cache(cfg.head_dim, cfg.max_position, cfg.rope_base,
                                rope_scaling=cfg.rope_scaling or None)
        self.register_buffer("cos_sin", cs, persistent=False)

    def _apply(self, fn, recurse=True):
        # keep the RoPE table fp32 through .to(bfloat16) casts — the HIP
        # kernel consumes fp32 cos/sin.
        super()._apply(fn, recurse)
        if self.cos_sin.dtype != torch.float32:
            self.cos_sin = self.cos_sin.float()
        return self

    @torch.inference_mode()
    def forward(self, input_ids: torch.Tensor, kv_caches, meta) -> torch.Tensor:
        x = self.embed_tokens(input_ids)
        residual = None
        for i, layer in enumerate(self.layers):
            cache = kv_caches[i] if kv_caches is not None else None
            x, residual = layer(x, residual, self.cos_sin, cache, meta)
        x = (x.float() + residual.float()).to(x.dtype)
        return ops.rms_norm(x, self.final_norm_w, self.cfg.rms_norm_eps)

    @torch.inference_mode()
    def compute_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        if self.lm_head is not None:
            return self.lm_head(hidden)
        return F.linear(hidden, self.embed_tokens.weight)

    @torch.inference_mode()
    def init_random(self, seed: int = 0):
        """Random-init weights (no network => no real checkpoints).

        CPU path is generator-deterministic (tests build identical twins);
        GPU path inits in-place at device speed (8B+ scale).
        """
        std = 0.02
        on_gpu = next(self.parameters()).is_cuda
        if on_gpu:
            torch.cuda.manual_seed(seed)
        g = None if on_gpu else torch.Generator().manual_seed(seed)
        for name, p in self.named_parameters():
            if name.endswith("norm_w"):
                p.data.fill_(1.0)
            elif name.endswith(".bias"):
                p.data.zero_() if on_gpu else p.data.copy_(
                    torch.zeros(p.shape, dtype=torch.float32).to(p.dtype))
            elif on_gpu:
                p.data.normal_(0.0, std)
            else:
                t = torch.empty(p.shape, dtype=torch.float32)
                t.normal_(0.0, std, generator=g)
                p.data.copy_(t.to(p.dtype))
        return self

    def memory_bytes(self) -> int:
        return sum(p.numel() * p.element_size() for p in self.parameters())
