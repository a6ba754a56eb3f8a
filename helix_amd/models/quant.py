"""Weights-quantized serving: fp8 e4m3 W8A8 with per-channel/per-token
scales, and weight-only ggml Q4_0/Q8_0 and Q4_K/Q6_K (second half of this
file).

The reference serves quantized checkpoints through vLLM/Ollama
quantization support; here quantization is a
post-load model pass: every eligible nn.Linear is swapped for an
FP8Linear holding e4m3 bytes + per-output-channel scales, and the
forward runs the hand-written 16x16x128 scaled-MFMA GEMM
(ops/hip/gemm_fp8.hip) with per-token activation quantization.

Why epilogue dequant instead of HW MX block scales: unity e8m0 scales
keep full per-channel accuracy without depending on the scale-lane
mapping (validated by tests/test_ops_gpu.py::test_mfma_probe_fp8_*),
and halve weight HBM (llama3-70b: 141 -> 71 GB resident).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from helix_amd import ops


class FP8Linear(nn.Module):
    """Drop-in nn.Linear replacement: e4m3 weights + fp32 out-channel
    scales; activations quantized per token at call time."""

    def __init__(self, weight8: torch.Tensor, w_scale: torch.Tensor):
        super().__init__()
        self.register_buffer("weight8", weight8, persistent=True)
        self.register_buffer("w_scale", w_scale, persistent=True)
        self.out_features, self.in_features = weight8.shape

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "FP8Linear":
        w8, ws = ops.quantize_fp8(lin.weight.data)
        return cls(w8.contiguous(), ws.contiguous())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shape = x.shape[:-1]
        x2 = x.reshape(-1, self.in_features)
        x8, xs = ops.quantize_fp8(x2)
        out = ops.gemm_fp8(x8.contiguous(), self.weight8, xs.contiguous(),
                           self.w_scale)
        return out.reshape(*shape, self.out_features)


def quantize_model_fp8(model: nn.Module,
                       skip: tuple = ("lm_head",)) -> int:
    """Swap eligible Linears (in_features % 128 == 0, not in `skip`) for
    FP8Linear. Returns the number of modules converted."""
    converted = 0
    for name, mod in list(model.named_modules()):
        for child_name, child in list(mod.named_children()):
            full = f"{name}.{child_name}" if name else child_name
            if not isinstance(child, nn.Linear):
                continue
            if any(s in full for s in skip):
                continue
            if child.in_features % 128 != 0 or child.bias is not None:
                continue
            setattr(mod, child_name, FP8Linear.from_linear(child))
            converted += 1
    return converted


# -- weight-only ggml Q4_0 / Q8_0 (ops/hip/gemm_wq.hip) -----------------
# Unlike the fp8 pass above this keeps activations bf16 and the weights in
# ggml's own blocks (32 along K, one fp16 scale): a GGUF file's blocks are
# served as they are on disk (engine/gguf.py keep_quantized), or a dense
# model is quantized after load with ggml's reference quantizer.

class WQLinear(nn.Module):
    """Drop-in nn.Linear replacement holding ggml Q4_0/Q8_0 planes:
    `qs` (payload bytes) and `d` (fp16 block scales), plus an optional
    bias. Up to ops.WQ_FUSED_MAX_M rows run the fused dequant GEMM; larger
    batches dequantize into `scratch` and use the library GEMM.

    `scratch` is a bf16 buffer owned by the MODEL this module belongs to
    (attach_wq_scratch): its layers run one after another on one stream
    and may share it, two models may not, because the large-M path is two
    launches (dequantize, GEMM) that another model's thread can get
    between. Without one the large-M path allocates per call."""

    def __init__(self, qs: torch.Tensor, d: torch.Tensor, fmt: str,
                 bias: torch.Tensor | None = None,
                 scratch: torch.Tensor | None = None):
        super().__init__()
        bits = ops.wq_bits(fmt)
        self.fmt = fmt
        self.register_buffer("qs", qs.contiguous(), persistent=True)
        self.register_buffer("d", d.contiguous(), persistent=True)
        if bias is not None:
            self.register_buffer("bias", bias.contiguous(), persistent=True)
        else:
            self.bias = None
        self.out_features = qs.shape[0]
        self.in_features = qs.shape[1] * 2 if bits == 4 else qs.shape[1]
        if d.dtype != torch.float16 or \
                tuple(d.shape) != (self.out_features, self.in_features // 32):
            raise ValueError(
                f"WQLinear: d is {d.dtype} {tuple(d.shape)}, expected fp16 "
                f"{(self.out_features, self.in_features // 32)}")
        self.scratch = scratch

    @classmethod
    def from_linear(cls, lin: nn.Linear, fmt: str) -> "WQLinear":
        qs, d = ops.quantize_wq(lin.weight.data, fmt)
        bias = None if lin.bias is None else lin.bias.data
        return cls(qs, d, fmt, bias)

    @property
    def device(self):
        return self.qs.device

    def _apply(self, fn, recurse=True):
        # model.to(dtype) / .half() / .bfloat16() convert every floating
        # buffer; the block scales are fp16 by format, so `d` follows the
        # device only. A scratch left on another device is dropped
        # (attach_wq_scratch gives the model a new one).
        d = self.d
        super()._apply(fn, recurse)
        if self.d.dtype != torch.float16:
            self.d = d.to(self.d.device)
        if self.scratch is not None and self.scratch.device != self.qs.device:
            self.scratch = None
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shape = x.shape[:-1]
        x2 = x.reshape(-1, self.in_features)
        if x2.is_cuda and not x2.is_contiguous():
            x2 = x2.contiguous()
        out = ops.gemm_wq(x2, self.qs, self.d, self.fmt, self.bias,
                          scratch=self.scratch)
        return out.reshape(*shape, self.out_features)


# -- weight-only ggml K-quants, Q4_K / Q6_K (ops/hip/gemm_kq.hip) -------

_KQ_PLANES = {"q4_k": ("qs", "hdr"), "q6_k": ("ql", "qh", "sc", "d")}


class KQLinear(nn.Module):
    """Drop-in nn.Linear replacement holding ggml K-quant planes. The rows
    are an ordered list of segments, each of its own format: a fused
    projection keeps the types its parts have in the file (a Q4_K_M file's
    qkv_proj is q4_k, q4_k, q6_k). Segment i's planes are the buffers
    `s{i}_{plane}` (ops/reference.py names the planes), `fmts[i]` its
    format, `rows[i]` its first output row.

    Up to ops.KQ_FUSED_MAX_M rows: one fused dequant GEMM launch per
    segment, each writing its columns of one [M, N] output. Larger batches:
    every segment dequantizes into its row range of `scratch`, then one
    library GEMM over the whole weight. `scratch` follows WQLinear's
    ownership rule (attach_wq_scratch): one buffer per model and GPU."""

    def __init__(self, segments, bias: torch.Tensor | None = None,
                 scratch: torch.Tensor | None = None):
        super().__init__()
        if not segments:
            raise ValueError("KQLinear: no segments")
        self.fmts, self.rows = [], []
        n, K = 0, None
        for i, (fmt, planes) in enumerate(segments):
            ops.kq_check(fmt)
            names = _KQ_PLANES[fmt]
            if len(planes) != len(names):
                raise ValueError(f"KQLinear: {fmt} takes {len(names)} planes")
            sn, sk = ops.kq_shape(planes, fmt)
            if K is not None and sk != K:
                raise ValueError(f"KQLinear: segment {i} has K={sk}, not {K}")
            if sk % 256 or sn % 16:
                raise ValueError(f"KQLinear: segment {i} is [{sn}, {sk}]; "
                                 f"need N % 16 == 0 and K % 256 == 0")
            K = sk
            for name, p in zip(names, planes):
                self.register_buffer(f"s{i}_{name}", p.contiguous(),
                                     persistent=True)
            self.fmts.append(fmt)
            self.rows.append(n)
            n += sn
        if bias is not None:
            self.register_buffer("bias", bias.contiguous(), persistent=True)
        else:
            self.bias = None
        self.out_features, self.in_features = n, K
        self.scratch = scratch

    @classmethod
    def from_linear(cls, lin: nn.Linear, fmt: str) -> "KQLinear":
        bias = None if lin.bias is None else lin.bias.data
        return cls([(fmt, ops.quantize_kq(lin.weight.data, fmt))], bias)

    def planes(self, i: int):
        return tuple(getattr(self, f"s{i}_{name}")
                     for name in _KQ_PLANES[self.fmts[i]])

    @property
    def segments(self):
        return [(f, self.planes(i)) for i, f in enumerate(self.fmts)]

    @property
    def device(self):
        return self.planes(0)[0].device

    def _apply(self, fn, recurse=True):
        # as WQLinear._apply: the fp16 super-block scales of q6_k are fp16 by
        # format and follow the device only (the integer planes are never
        # touched by a dtype cast)
        keep = {f"s{i}_d": getattr(self, f"s{i}_d")
                for i, f in enumerate(self.fmts) if f == "q6_k"}
        super()._apply(fn, recurse)
        for n, b in keep.items():
            if self._buffers[n].dtype != torch.float16:
                self._buffers[n] = b.to(self._buffers[n].device)
        if self.scratch is not None and self.scratch.device != self.device:
            self.scratch = None
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shape = x.shape[:-1]
        x2 = x.reshape(-1, self.in_features)
        if x2.is_cuda and not x2.is_contiguous():
            x2 = x2.contiguous()
        M, N, K = x2.shape[0], self.out_features, self.in_features
        if not x2.is_cuda:
            # the definition: F.linear on the dequantized fused weight
            w = torch.cat([ops.dequantize_kq(p, f).to(x2.dtype)
                           for f, p in self.segments], dim=0)
            out = torch.nn.functional.linear(x2, w, self.bias)
            return out.reshape(*shape, N)
        if 0 < M <= ops.KQ_FUSED_MAX_M:
            out = torch.empty(M, N, dtype=x2.dtype, device=x2.device)
            for i, fmt in enumerate(self.fmts):
                ops.gemm_kq(x2, self.planes(i), fmt, self.bias, out=out,
                            col_off=self.rows[i])
            return out.reshape(*shape, N)
        if self.scratch is not None:
            w = self.scratch.view(-1)[:N * K].view(N, K)
        else:
            w = torch.empty(N, K, dtype=torch.bfloat16, device=x2.device)
        ends = self.rows[1:] + [N]
        for i, fmt in enumerate(self.fmts):
            ops.dequant_kq(self.planes(i), fmt, out=w[self.rows[i]:ends[i]])
        out = torch.nn.functional.linear(x2, w, self.bias)
        return out.reshape(*shape, N)


def _is_wq_moe(m: nn.Module) -> bool:
    """A models/llama.py MoEMLP in its quantised state."""
    return getattr(m, "expert_fmt", None) is not None


def _wq_device(m: nn.Module):
    # the first w13 plane: `w13_qs` (Q4_0/Q8_0/Q4_K) or `w13_ql` (Q6_K)
    return m.expert_planes("w13")[0].device if _is_wq_moe(m) else m.device


def attach_wq_scratch(model: nn.Module) -> None:
    """Give `model` its own dequant buffer: one bf16 tensor per GPU it has
    WQLinears, KQLinears or quantised MoEMLPs on, sized for the largest of
    them and shared by them alone.
    Called when the weights are installed and again by the engine if the
    model was moved since; never from a forward. A model whose modules
    already hold a fitting buffer is left as it is (captured graphs point
    into it)."""
    mods = [m for m in model.modules()
            if (isinstance(m, (WQLinear, KQLinear)) or _is_wq_moe(m))
            and _wq_device(m).type == "cuda"]
    need: dict = {}
    for m in mods:
        if _is_wq_moe(m):
            # the library prefill path dequantizes one expert's w13, the
            # larger of its two weights: 2*I*H elements
            n = 2 * m.intermediate_size * m.hidden_size
        else:
            n = m.in_features * m.out_features
        need[_wq_device(m)] = max(need.get(_wq_device(m), 0), n)
    for dev, numel in need.items():
        mine = [m for m in mods if _wq_device(m) == dev]
        cur = mine[0].scratch
        if cur is not None and cur.device == dev and cur.numel() >= numel \
                and all(m.scratch is cur for m in mine):
            continue
        buf = torch.empty(numel, dtype=torch.bfloat16, device=dev)
        for m in mine:
            m.scratch = buf


def quantize_model_wq(model: nn.Module, fmt: str,
                      skip: tuple = ("lm_head",)) -> int:
    """Swap eligible Linears (in_features % 32 == 0, out_features % 16 == 0,
    name outside `skip`; a bias is kept) for WQLinear, then give the model
    its dequant scratch. With a K-quant format ("q4_k", "q6_k") the block
    is 256 (in_features % 256 == 0) and the module a single-segment
    KQLinear. Returns the number of modules converted."""
    kq = fmt in ops.KQ_FORMATS
    if not kq:
        ops.wq_bits(fmt)
    block = 256 if kq else 32
    cls = KQLinear if kq else WQLinear
    converted = 0
    for name, mod in list(model.named_modules()):
        for child_name, child in list(mod.named_children()):
            full = f"{name}.{child_name}" if name else child_name
            if not isinstance(child, nn.Linear):
                continue
            if any(s in full for s in skip):
                continue
            if child.in_features % block != 0 or child.out_features % 16 != 0:
                continue
            setattr(mod, child_name, cls.from_linear(child, fmt))
            converted += 1
    attach_wq_scratch(model)
    return converted


def quantize_model_experts(model: nn.Module, fmt: str) -> int:
    """Quantise the experts of every bf16 MoEMLP to ggml Q4_0/Q8_0 planes
    with ggml's reference quantizer (rows are independent, so a stack is
    quantize_wq on its [E*rows, K] view), layer by layer: a layer's bf16
    experts are freed before the next layer is touched. The router and
    everything outside the experts are left alone. Returns the number of
    layers converted; a layer already quantised is skipped."""
    from helix_amd.models.llama import MoEMLP
    ops.wq_bits(fmt)
    converted = 0
    for m in model.modules():
        if not isinstance(m, MoEMLP) or m.expert_fmt is not None:
            continue
        planes = []
        for name in ("w13", "w2"):
            w = getattr(m, name).data
            E, rows, K = w.shape
            qs, d = ops.quantize_wq(w.view(E * rows, K), fmt)
            planes.append((qs.view(E, rows, -1), d.view(E, rows, K // 32)))
            del w
        m.set_quantized_experts(planes[0], planes[1], fmt)
        converted += 1
    attach_wq_scratch(model)
    return converted


def quantize_model_experts_kq(model: nn.Module, fmt) -> int:
    """quantize_model_experts for the K formats: `fmt` is "q4_k" / "q6_k", a
    (w13, w2) pair, or "q4_k_m" (q4_k, with a q6_k w2 in the layers
    gguf.q4_k_m_uses_q6_k picks, counting the model's MoE layers), quantised
    by ops.quantize_kq (a plain quantizer, not ggml's search) on each
    stack's [E*rows, K] view, layer by layer with the layer's bf16 experts
    freed before the next. For benchmarks and tests: the engine option
    expert_quantization does not take these formats. Returns the number of
    layers converted; a layer already quantised is skipped."""
    from helix_amd.engine.gguf import q4_k_m_uses_q6_k
    from helix_amd.models.llama import MoEMLP
    mlps = [m for m in model.modules() if isinstance(m, MoEMLP)]
    if fmt == "q4_k_m":
        pairs = [("q4_k", "q6_k" if q4_k_m_uses_q6_k(i, len(mlps))
                  else "q4_k") for i in range(len(mlps))]
    else:
        f13, f2 = (fmt, fmt) if isinstance(fmt, str) else tuple(fmt)
        ops.kq_check(f13), ops.kq_check(f2)
        pairs = [(f13, f2)] * len(mlps)
    converted = 0
    for m, pair in zip(mlps, pairs):
        if m.expert_fmt is not None:
            continue
        stacks = []
        for name, f in zip(("w13", "w2"), pair):
            w = getattr(m, name).data
            E, rows, K = w.shape
            planes = ops.quantize_kq(w.view(E * rows, K), f)
            stacks.append(tuple(p.view(E, rows, *p.shape[1:])
                                for p in planes))
            del w
        m.set_kquant_experts(stacks[0], stacks[1], pair)
        converted += 1
    attach_wq_scratch(model)
    return converted


def has_wq(model: nn.Module) -> bool:
    return any(isinstance(m, (WQLinear, KQLinear)) or _is_wq_moe(m)
               for m in model.modules())
