"""helix_amd.ops — CDNA4 (gfx950) kernel dispatch.

GPU tensors run the hand-written HIP kernels in helix_amd._C and FAIL
LOUDLY if the extension is missing (no silent eager fallback on a GPU
box). CPU tensors use the pure-torch reference implementations so engine
logic is testable without a GPU.
"""
from __future__ import annotations

import os

import torch

from . import reference as ref
from .reference import make_cos_sin_cache  # re-export

_C = None
_C_ERR: str | None = None
try:
    from helix_amd import _C  # type: ignore  # noqa: F401
    from helix_amd import _C as _C_mod
    _C = _C_mod
except ImportError as e:  # pragma: no cover
    _C_ERR = str(e)


def _native():
    if _C is None:
        raise RuntimeError(
            "helix_amd._C native extension is not built but a GPU tensor was "
            "passed. Build it with `python setup.py build_ext --inplace` "
            f"(PYTORCH_ROCM_ARCH=gfx950). Import error: {_C_ERR}")
    return _C


def have_native() -> bool:
    return _C is not None


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        _native().rms_norm(out, x, w, eps)
        return out
    return ref.rms_norm(x, w, eps)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor,
                       w: torch.Tensor, eps: float):
    """In-place on GPU: x <- norm(x+res), residual <- x+res. Returns both."""
    if x.is_cuda:
        _native().fused_add_rms_norm(x, residual, w, eps)
        return x, residual
    out, new_res = ref.fused_add_rms_norm(x, residual, w, eps)
    x.copy_(out)
    residual.copy_(new_res)
    return x, residual


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
               eps: float) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        _native().layer_norm(out, x, w, b, eps)
        return out
    return ref.layer_norm(x, w, b, eps)


def rotary_embedding(positions: torch.Tensor, q: torch.Tensor,
                     k: torch.Tensor, cos_sin: torch.Tensor, head_dim: int):
    """In-place on GPU. Returns (q, k)."""
    if q.is_cuda:
        _native().rotary_embedding(positions, q, k, cos_sin, head_dim)
        return q, k
    qo, ko = ref.rotary_embedding(positions, q, k, cos_sin, head_dim)
    q.copy_(qo)
    k.copy_(ko)
    return q, k


def kv_fp8_quant(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> OCP e4m3 bytes (uint8 view), any shape."""
    return t.to(torch.float8_e4m3fn).view(torch.uint8)


def kv_fp8_dequant(t: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """OCP e4m3 bytes (uint8) -> dtype."""
    return t.view(torch.float8_e4m3fn).to(dtype)


def rope_qkv_cache(positions: torch.Tensor, qkv: torch.Tensor,
                   cos_sin: torch.Tensor, num_q: int, num_kv: int,
                   head_dim: int, kv_cache=None, slot_mapping=None,
                   want_kv: bool = False, q_norm_w=None, k_norm_w=None,
                   eps: float = 0.0):
    """Fused QKV epilogue: strided split + rope + paged-cache write.

    Returns (q [T, num_q, head_dim], k, v) — k/v are None unless
    want_kv (fresh-prefill path needs compact K/V for attn_prefill).

    q_norm_w / k_norm_w (bf16 [head_dim], both or neither) turn on Qwen3's
    QK-norm: each Q and K head is RMS-normalised over its own head_dim
    elements with `eps` and scaled by the weight before the rope
    (rope_qkv_norm.hip). Without them the GPU branch issues exactly the
    un-normed kernel.
    """
    if (q_norm_w is None) != (k_norm_w is None):
        raise ValueError("rope_qkv_cache: q_norm_w and k_norm_w go together "
                         "(got only one of them)")
    normed = q_norm_w is not None
    T = qkv.shape[0]
    if qkv.is_cuda:
        q_out = torch.empty(T, num_q * head_dim, dtype=qkv.dtype,
                            device=qkv.device)
        k_out = v_out = None
        if want_kv:
            k_out = torch.empty(T, num_kv * head_dim, dtype=qkv.dtype,
                                device=qkv.device)
            v_out = torch.empty_like(k_out)
        kc = vc = None
        if kv_cache is not None:
            kc, vc = kv_cache
        if normed:
            _native().rope_qkv_norm_cache(positions, qkv, q_out, kc, vc,
                                          slot_mapping, k_out, v_out,
                                          cos_sin, num_q, num_kv, head_dim,
                                          q_norm_w, k_norm_w, eps)
        else:
            _native().rope_qkv_cache(positions, qkv, q_out, kc, vc,
                                     slot_mapping, k_out, v_out, cos_sin,
                                     num_q, num_kv, head_dim)
        return (q_out.view(T, num_q, head_dim),
                k_out.view(T, num_kv, head_dim) if want_kv else None,
                v_out.view(T, num_kv, head_dim) if want_kv else None)
    # CPU reference composition (same semantics)
    q_sz, kv_sz = num_q * head_dim, num_kv * head_dim
    q, k, v = qkv.split([q_sz, kv_sz, kv_sz], dim=-1)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if normed:
        # fp32 through norm and rope, one rounding at the end (the kernel's
        # order); the fp8 cache below re-rounds the bf16 K on this branch
        q = ref.qk_rms_norm(q, q_norm_w, eps, head_dim)
        k = ref.qk_rms_norm(k, k_norm_w, eps, head_dim)
        qr, kr = ref.rotary_embedding(positions, q, k, cos_sin, head_dim)
        q, k = qr.to(qkv.dtype), kr.to(qkv.dtype)
    else:
        q, k = rotary_embedding(positions, q, k, cos_sin, head_dim)
    q = q.view(T, num_q, head_dim)
    k = k.view(T, num_kv, head_dim)
    v = v.view(T, num_kv, head_dim)
    if kv_cache is not None:
        if kv_cache[0].dtype == torch.uint8:    # fp8 KV cache
            reshape_and_cache(kv_fp8_quant(k), kv_fp8_quant(v),
                              kv_cache[0], kv_cache[1], slot_mapping)
        else:
            reshape_and_cache(k, v, kv_cache[0], kv_cache[1], slot_mapping)
    return q, (k if want_kv else None), (v if want_kv else None)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        i = x.shape[-1] // 2
        out = torch.empty(*x.shape[:-1], i, dtype=x.dtype, device=x.device)
        _native().silu_and_mul(out, x)
        return out
    return ref.silu_and_mul(x)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        _native().gelu_tanh(out, x)
        return out
    return ref.gelu_tanh(x)


def reshape_and_cache(k: torch.Tensor, v: torch.Tensor,
                      k_cache: torch.Tensor, v_cache: torch.Tensor,
                      slot_mapping: torch.Tensor):
    if k.is_cuda:
        _native().reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)
        return
    ref.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)


def attn_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 cu_seqlens: torch.Tensor, max_seqlen: int,
                 scale: float, causal: bool = True,
                 window: int = 0,
                 cu_seqlens_k: torch.Tensor | None = None) -> torch.Tensor:
    """Varlen attention. When cu_seqlens_k is given, q rows are the
    SUFFIX of each sequence (cached-prefix prefill): kv rows cover the
    full context and causal positions are offset by klen - qlen."""
    if cu_seqlens_k is None:
        cu_seqlens_k = cu_seqlens
    if q.is_cuda:
        out = torch.empty_like(q)
        _native().attn_prefill(out, q, k, v, cu_seqlens, cu_seqlens_k,
                               max_seqlen, scale, causal, window)
        return out
    return ref.attn_prefill(q, k, v, cu_seqlens, max_seqlen, scale, causal,
                            window, cu_seqlens_k)


# Flash-decoding split-K quantum: PART_QUANT in paged_attn_decode.hip,
# which the extension exports as _C.DECODE_PART_QUANT (a test holds the
# two equal).
DECODE_PARTITION = 128


def decode_workspace(max_batch: int, num_q_heads: int, head_dim: int,
                     max_seq_len: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """Persistent fp32 scratch for partitioned decode attention."""
    max_parts = max(1, (max_seq_len + DECODE_PARTITION - 1) // DECODE_PARTITION)
    tmp_out = torch.empty(max_batch, num_q_heads, max_parts, head_dim,
                          dtype=torch.float32, device=device)
    tmp_ml = torch.empty(max_batch, num_q_heads, max_parts, 2,
                         dtype=torch.float32, device=device)
    return tmp_out, tmp_ml


def paged_attn_decode(q: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, block_tables: torch.Tensor,
                      seq_lens: torch.Tensor, scale: float,
                      workspace=None, max_len: int | None = None,
                      window: int = 0) -> torch.Tensor:
    if q.is_cuda:
        out = torch.empty_like(q)
        if max_len is None:
            max_len = int(seq_lens.max())   # host sync — pass max_len to avoid
        if workspace is None:
            workspace = decode_workspace(q.shape[0], q.shape[1], q.shape[2],
                                         max_len, q.device)
        tmp_out, tmp_ml = workspace
        _native().paged_attn_decode(out, q, k_cache, v_cache, block_tables,
                                    seq_lens, scale,
                                    tmp_out[:q.shape[0]], tmp_ml[:q.shape[0]],
                                    max_len, window)
        return out
    if k_cache.dtype == torch.uint8:            # fp8 KV cache
        k_cache = kv_fp8_dequant(k_cache)
        v_cache = kv_fp8_dequant(v_cache)
    return ref.paged_attn_decode(q, k_cache, v_cache, block_tables, seq_lens,
                                 scale, window)


def sample_tokens(logits: torch.Tensor, temperatures: torch.Tensor,
                  seeds: torch.Tensor) -> torch.Tensor:
    if logits.is_cuda:
        out = torch.empty(logits.shape[0], dtype=torch.int64,
                          device=logits.device)
        _native().sample_tokens(out, logits, temperatures, seeds)
        return out
    return ref.sample_tokens(logits, temperatures, seeds)


def sample_tokens_ext(logits: torch.Tensor, temperatures: torch.Tensor,
                      seeds: torch.Tensor, top_p: torch.Tensor,
                      top_k: torch.Tensor, rep_pen: torch.Tensor,
                      pres_pen: torch.Tensor, freq_pen: torch.Tensor,
                      counts=None, seen=None, row_map=None) -> torch.Tensor:
    """Fused top-k/top-p/penalty Gumbel sampling (GPU only): one block
    per row, histogram-located threshold, no vocab sort. Penalties read
    per-row token-count tables indexed by row_map (engine row slots)."""
    out = torch.empty(logits.shape[0], dtype=torch.int64,
                      device=logits.device)
    _native().sample_tokens_ext(out, logits, temperatures, seeds, top_p,
                                top_k, rep_pen, pres_pen, freq_pen,
                                counts, seen, row_map)
    return out


def quantize_fp8(t: torch.Tensor, dim: int = -1):
    """Per-row (dim=-1 reduces over the last axis) e4m3 quantization.
    Returns (bytes uint8 view, float32 scales)."""
    amax = t.float().abs().amax(dim=dim, keepdim=True).clamp(min=1e-8)
    scale = amax / 448.0                      # e4m3fn max normal
    q = (t.float() / scale).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale.squeeze(dim).float()


def gemm_fp8(x8: torch.Tensor, w8: torch.Tensor, x_scale: torch.Tensor,
             w_scale: torch.Tensor, bias: torch.Tensor | None = None,
             act: int = 0) -> torch.Tensor:
    """out[M,N] = dequant(x8 @ w8^T): e4m3 inputs as uint8 views with
    per-row activation scales and per-output-channel weight scales
    (epilogue dequant; MFMA runs at the 2x fp8 rate)."""
    M, N = x8.shape[0], w8.shape[0]
    if x8.is_cuda:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x8.device)
        _native().gemm_fp8(out, x8, w8, x_scale.contiguous(),
                           w_scale.contiguous(), bias, act)
        return out
    xf = x8.view(torch.float8_e4m3fn).float() * x_scale[:, None]
    wf = w8.view(torch.float8_e4m3fn).float() * w_scale[:, None]
    out = xf @ wf.t()
    if bias is not None:
        out = out + bias.float()
    if act == 1:
        out = torch.nn.functional.gelu(out, approximate="tanh")
    return out.to(torch.bfloat16)


def gemm_bf16(x: torch.Tensor, w: torch.Tensor, bias=None,
              act: int = 0) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype,
                          device=x.device)
        _native().gemm_bf16(out, x, w, bias, act)
        return out
    return ref.gemm_bf16(x, w, bias, act)


_SKINNY_MAX_M = 1024
_SKINNY_SCRATCH: dict = {}        # device -> fp32 workspace tensor
_SKINNY_SWIZZLE = os.environ.get("HELIX_SKINNY_SWIZZLE", "1") == "1"
_SKINNY_ENABLED = os.environ.get("HELIX_SKINNY_GEMM", "0") == "1"


def _skinny_split(M: int, N: int, K: int) -> int:
    """Split-K factor: enough workgroups to put ~3 on each of the 256
    CUs (m97-structure occupancy), subject to K dividing into 64s."""
    bm = 128 if M > 64 else 64
    tiles = ((M + bm - 1) // bm) * ((N + 127) // 128)
    s = 1
    while s < 8 and tiles * s < 768 and K % (s * 2 * 64) == 0:
        s *= 2
    return s


def gemm_skinny_bf16(x: torch.Tensor, w: torch.Tensor, bias=None,
                     act: int = 0) -> torch.Tensor:
    """Decode-shape GEMM (M <= 1024): split-K skinny tiles, fused
    bias/act epilogue. Caller guarantees bf16 CUDA contiguous inputs."""
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    s = _skinny_split(M, N, K)
    scratch = None
    if s > 1:
        need = s * M * N
        key = x.device.index
        cur = _SKINNY_SCRATCH.get(key)
        if cur is None or cur.numel() < need:
            cur = torch.empty(need, dtype=torch.float32, device=x.device)
            _SKINNY_SCRATCH[key] = cur
        scratch = cur
    _native().gemm_skinny_bf16(out, x, w, bias, scratch, s, act,
                               1 if _SKINNY_SWIZZLE else 0)
    return out


def linear(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """Projection dispatch: skinny-M decode GEMMs on the owned kernel,
    everything else (prefill-sized M, CPU, odd dims) via torch/hipBLASLt."""
    if (_SKINNY_ENABLED and x.is_cuda and x.dtype == torch.bfloat16
            and x.dim() == 2
            and w.dtype == torch.bfloat16 and 0 < x.shape[0] <= _SKINNY_MAX_M
            and x.shape[1] % 64 == 0 and w.shape[0] % 16 == 0
            and x.is_contiguous() and w.is_contiguous()):
        return gemm_skinny_bf16(x, w, bias)
    return torch.nn.functional.linear(x, w, bias)


# -- ggml Q4_0 / Q8_0 weight-only GEMM (ops/hip/gemm_wq.hip) ------------
from .reference import (quantize_wq, dequantize_wq, pack_ggml,  # noqa: E402,F401
                        unpack_ggml, wq_bits, WQ_FORMATS)

# Largest M the fused dequant+MFMA kernel serves; above it the weight is
# dequantized into a scratch buffer and the library GEMM runs. Must be a
# member of graph_runner.BATCH_BUCKETS so a batch and its padded bucket
# take the same path (tests/test_wq_cpu.py holds that). The kernel itself
# goes to 64 (_C.WQ_KERNEL_MAX_M); 16 is the largest bucket at which it
# still beats the bf16 library GEMM at the llama3-8b projection shapes
# (profiles/r05_wq.md: 0.99-2.4x at M = 16, 0.81-1.8x at M = 32).
WQ_FUSED_MAX_M = 16


def dequant_wq(qs: torch.Tensor, d: torch.Tensor, fmt: str,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Planes -> bf16 [N, K]. GPU: the HIP kernel, into `out` when given
    (any contiguous bf16 buffer of at least N*K elements). CPU: the torch
    reference, `out` unused."""
    bits = wq_bits(fmt)
    if not qs.is_cuda:
        return dequantize_wq(qs, d, fmt, torch.bfloat16)
    N = qs.shape[0]
    K = qs.shape[1] * 2 if bits == 4 else qs.shape[1]
    if out is None:
        w = torch.empty(N, K, dtype=torch.bfloat16, device=qs.device)
    else:
        if out.dtype != torch.bfloat16 or out.numel() < N * K \
                or not out.is_contiguous():
            raise ValueError(
                f"dequant_wq: scratch must be contiguous bf16 with at least "
                f"{N * K} elements, got {out.dtype} x {out.numel()}")
        w = out.view(-1)[:N * K].view(N, K)
    _native().dequant_wq(w, qs, d, bits)
    return w


def gemm_wq(x: torch.Tensor, qs: torch.Tensor, d: torch.Tensor, fmt: str,
            bias: torch.Tensor | None = None,
            scratch: torch.Tensor | None = None) -> torch.Tensor:
    """out[M,N] = x[M,K] @ dequant(qs, d)^T (+ bias): ggml Q4_0/Q8_0
    weights kept quantized. GPU, M <= WQ_FUSED_MAX_M: dequant fused into the
    MFMA loop. GPU, larger M: dequant_wq into `scratch` (allocated per call
    when None, so capture-safe callers pass one) + the library GEMM.
    CPU: F.linear on the dequantized weight, the definition tests hold the
    rest of the stack to."""
    bits = wq_bits(fmt)
    if not x.is_cuda:
        w = dequantize_wq(qs, d, fmt, torch.float32).to(x.dtype)
        return torch.nn.functional.linear(x, w, bias)
    if x.dim() != 2:
        raise ValueError(f"gemm_wq: x must be [M, K], got {tuple(x.shape)}")
    M, N = x.shape[0], qs.shape[0]
    if 0 < M <= WQ_FUSED_MAX_M:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        _native().gemm_wq(out, x, qs, d, bias, bits)
        return out
    if x.dtype != torch.bfloat16:
        raise ValueError(f"gemm_wq: x must be bf16 on GPU, got {x.dtype}")
    w = dequant_wq(qs, d, fmt, out=scratch)
    return torch.nn.functional.linear(x, w, bias)


# -- ggml Q4_K / Q6_K weight-only GEMM (ops/hip/gemm_kq.hip) ------------
from .reference import (quantize_kq, dequantize_kq, pack_ggml_kq,  # noqa: E402,F401
                        unpack_ggml_kq, kq_check, kq_shape, KQ_FORMATS,
                        KQ_BLOCK_BYTES)

# Largest M the fused K-quant kernel serves; the same rule as
# WQ_FUSED_MAX_M: a member of graph_runner.BATCH_BUCKETS, not above the
# kernel's own limit (_C.KQ_KERNEL_MAX_M = 32), at which the kernel still
# beats the bf16 library GEMM for both formats at all four llama3-8b
# projection shapes (profiles/r06_kquant.md, two runs: q4_k 1.15-2.68x and
# q6_k 1.01-2.31x at M = 16; 0.64-1.56x at M = 32, three of four shapes
# losing).
KQ_FUSED_MAX_M = 16


def kq_waves(N: int, K: int) -> int:
    """K-split factor (waves per workgroup) the fused kernel uses for a
    [N, K] weight: the host's own function, a property of the shape."""
    return int(_native().kq_waves(N, K))


def dequant_kq(planes, fmt: str,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Planes -> bf16 [N, K]. GPU: the HIP kernel, into `out` when given
    (any contiguous bf16 buffer of at least N*K elements). CPU: the torch
    reference, `out` unused."""
    kq_check(fmt)
    if not planes[0].is_cuda:
        return dequantize_kq(planes, fmt, torch.bfloat16)
    N, K = kq_shape(planes, fmt)
    if out is None:
        w = torch.empty(N, K, dtype=torch.bfloat16, device=planes[0].device)
    else:
        if out.dtype != torch.bfloat16 or out.numel() < N * K \
                or not out.is_contiguous():
            raise ValueError(
                f"dequant_kq: scratch must be contiguous bf16 with at least "
                f"{N * K} elements, got {out.dtype} x {out.numel()}")
        w = out.view(-1)[:N * K].view(N, K)
    _native().dequant_kq(w, list(planes), fmt)
    return w


def gemm_kq(x: torch.Tensor, planes, fmt: str,
            bias: torch.Tensor | None = None,
            scratch: torch.Tensor | None = None,
            out: torch.Tensor | None = None,
            col_off: int = 0) -> torch.Tensor:
    """out[:, col_off:col_off+N] = x[M,K] @ dequant(planes)^T
    (+ bias[col_off:col_off+N]): ggml Q4_K/Q6_K weights kept quantized.
    `out` is a bf16 [M, ldo] buffer shared by the segments of a fused
    projection (allocated [M, N] when None, with col_off = 0); `bias`
    is indexed like `out`'s columns. Returns `out`.
    GPU, M <= KQ_FUSED_MAX_M: dequant fused into the MFMA loop. GPU, larger
    M: dequant_kq into `scratch` (allocated per call when None) + the
    library GEMM. CPU: F.linear on the dequantized weight, the definition
    tests hold the rest of the stack to."""
    kq_check(fmt)
    N, K = kq_shape(planes, fmt)
    if x.dim() != 2:
        raise ValueError(f"gemm_kq: x must be [M, K], got {tuple(x.shape)}")
    M = x.shape[0]
    if out is None:
        if col_off:
            raise ValueError("gemm_kq: col_off needs an `out` buffer")
    elif out.dim() != 2 or out.shape[0] != M or out.shape[1] < col_off + N:
        raise ValueError(f"gemm_kq: out is {tuple(out.shape)}, need "
                         f"[{M}, >= {col_off + N}]")
    seg_bias = None if bias is None else bias[col_off:col_off + N]
    if x.is_cuda and 0 < M <= KQ_FUSED_MAX_M:
        if out is None:
            out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        _native().gemm_kq(out, col_off, x, list(planes), bias, fmt)
        return out
    if not x.is_cuda:
        w = dequantize_kq(planes, fmt, torch.float32).to(x.dtype)
    elif x.dtype != torch.bfloat16:
        raise ValueError(f"gemm_kq: x must be bf16 on GPU, got {x.dtype}")
    else:
        w = dequant_kq(planes, fmt, out=scratch)
    y = torch.nn.functional.linear(x, w, seg_bias)
    if out is None:
        return y
    out[:, col_off:col_off + N] = y
    return out


# -- mixture-of-experts routed expert GEMMs (ops/hip/moe.hip) -----------
# Largest T at which moe_experts(fused=None) takes the fused kernels; above
# it the eager library path runs (one host sync, so never under capture;
# decode passes fused=True). The rule: the largest benchmarked T at which
# the fused path is not slower than the library path on uniform routing, in
# two runs of scripts/bench_moe.py (T = 1, 8, 16, 64, 128, 512).
# MEASURED, not the placeholder of 64 (profiles/r08_moe.md): fused over
# library on uniform routing 2.2x at T = 1, 1.4x at 64, 1.1x at 128 and
# 0.47x at 512 in both runs.
MOE_FUSED_MAX_T = 128


def moe_waves(N: int, K: int, gated: bool) -> int:
    """K-split factor (waves per workgroup) the routed GEMM uses for one
    expert's [N, K] weight (N = I, K = H for the gated GEMM; N = H, K = I
    for the down GEMM): the host's own function, a property of the shape."""
    return int(_native().moe_waves(N, K, gated))


def moe_route(logits: torch.Tensor, k: int):
    """(topk_ids [T, k] int32, topk_w [T, k] fp32): fp32 softmax over the
    experts, the k largest renormalised to sum 1, ties to the lower expert
    index, slot j = the j-th largest."""
    if not logits.is_cuda:
        return ref.moe_route(logits, k)
    T = logits.shape[0]
    ids = torch.empty(T, k, dtype=torch.int32, device=logits.device)
    w = torch.empty(T, k, dtype=torch.float32, device=logits.device)
    _native().moe_route(ids, w, logits)
    return ids, w


def moe_align(topk_ids: torch.Tensor, E: int):
    """(expert_off [E+1] int32, sorted_pairs [P] int32): per expert, its
    pair indices p = t*k + j in ascending order. Ids outside [0, E) belong
    to no list (sorted_pairs past expert_off[E] is then unspecified on GPU)."""
    if not topk_ids.is_cuda:
        return ref.moe_align(topk_ids, E)
    off = torch.empty(E + 1, dtype=torch.int32, device=topk_ids.device)
    pairs = torch.empty(topk_ids.numel(), dtype=torch.int32,
                        device=topk_ids.device)
    _native().moe_align(off, pairs, topk_ids, E)
    return off, pairs


def moe_combine(ypair: torch.Tensor, k: int,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """out[t] = bf16(sum_j ypair[t*k + j]), ascending j, in fp32."""
    if not ypair.is_cuda:
        return ref.moe_combine(ypair, k)
    if out is None:
        out = torch.empty(ypair.shape[0] // k, ypair.shape[1],
                          dtype=torch.bfloat16, device=ypair.device)
    _native().moe_combine(out, ypair, k)
    return out


def moe_experts(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor,
                topk_ids: torch.Tensor, topk_w: torch.Tensor,
                fused: bool | None = None, out: torch.Tensor | None = None,
                act: torch.Tensor | None = None,
                ypair: torch.Tensor | None = None) -> torch.Tensor:
    """Routed SwiGLU experts: out[t] = sum_j topk_w[t, j] *
    w2[e] @ (silu(w13[e, :I] @ x[t]) * (w13[e, I:] @ x[t])), e = topk_ids[t, j].
    x [T, H] bf16, w13 [E, 2I, H], w2 [E, H, I], topk_ids int32 in [0, E)
    (a pair with any other id is computed by no expert and its share of the
    sum is unspecified).
    GPU, fused=True: moe_align + the two routed GEMM kernels + moe_combine;
    no host sync, no host-sized shape, no memset, so always capture-safe,
    and correct for any T. GPU, fused=False: the eager library path (one
    host sync): x gathered by list, per-expert F.linear / silu_and_mul /
    F.linear, scaled into the same fp32 ypair, the same moe_combine.
    fused=None: fused up to MOE_FUSED_MAX_T tokens. `out` [T, H] bf16, `act`
    [T*k, I] bf16 and `ypair` [T*k, H] fp32 are allocated when None.
    CPU: the torch reference."""
    if not x.is_cuda:
        return ref.moe_experts(x, w13, w2, topk_ids, topk_w)
    if x.dim() != 2 or topk_ids.dim() != 2:
        raise ValueError("moe_experts: x must be [T, H] and topk_ids [T, k]")
    T, k = topk_ids.shape
    E, I, H = w13.shape[0], w13.shape[1] // 2, w13.shape[2]
    P = T * k
    if x.shape[0] != T or tuple(topk_w.shape) != (T, k):
        raise ValueError(
            f"moe_experts: x {tuple(x.shape)}, topk_ids {tuple(topk_ids.shape)}"
            f" and topk_w {tuple(topk_w.shape)} disagree on [T, k]")
    if fused is None:
        fused = T <= MOE_FUSED_MAX_T
    if act is None:
        act = torch.empty(P, I, dtype=torch.bfloat16, device=x.device)
    if ypair is None:
        ypair = torch.empty(P, H, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(T, H, dtype=torch.bfloat16, device=x.device)
    C = _native()
    off = torch.empty(E + 1, dtype=torch.int32, device=x.device)
    pairs = torch.empty(P, dtype=torch.int32, device=x.device)
    C.moe_align(off, pairs, topk_ids, E)
    if fused:
        C.moe_gemm_gated(act, x, w13, off, pairs, k)
        C.moe_gemm_down(ypair, act, w2, topk_w, off, pairs)
    else:
        if x.dtype != torch.bfloat16 or w13.dtype != torch.bfloat16 \
                or w2.dtype != torch.bfloat16:
            raise ValueError("moe_experts: x, w13 and w2 must be bf16 on GPU")
        if tuple(w2.shape) != (E, H, I) or x.shape[1] != H \
                or tuple(act.shape) != (P, I) or tuple(ypair.shape) != (P, H) \
                or ypair.dtype != torch.float32:
            raise ValueError("moe_experts: shape mismatch between x, w13, w2,"
                             " act and ypair")
        offs = off.tolist()                       # the one host sync
        rows = pairs[:offs[E]].long()
        xg = x[rows // k]
        tw = topk_w.reshape(-1)[rows]
        for e in range(E):
            lo, hi = offs[e], offs[e + 1]
            if hi == lo:
                continue
            a = silu_and_mul(torch.nn.functional.linear(xg[lo:hi], w13[e]))
            act[rows[lo:hi]] = a
            y = torch.nn.functional.linear(a, w2[e])
            ypair[rows[lo:hi]] = y.float() * tw[lo:hi, None]
    C.moe_combine(out, ypair, k)
    return out


def moe_forward(x: torch.Tensor, router_logits: torch.Tensor,
                w13: torch.Tensor, w2: torch.Tensor, k: int,
                fused: bool | None = None) -> torch.Tensor:
    """One MoE MLP: route (moe_route) and run the routed experts
    (moe_experts)."""
    ids, w = moe_route(router_logits, k)
    return moe_experts(x, w13, w2, ids, w, fused=fused)


# -- routed expert GEMMs over Q4_0 / Q8_0 experts (ops/hip/moe_wq.hip) --
# Largest T at which moe_experts_wq(fused=None) takes the fused kernels.
# MOE_FUSED_MAX_T's rule: the largest benchmarked T at which the fused path
# is not slower than this feature's own library path (which pays a
# dequantise per non-empty expert) on uniform routing, in two runs of
# scripts/bench_moe.py --fmt q4_0 / q8_0; the smaller of the two formats.
# MEASURED, not the placeholder (profiles/r09_moe_wq.md): both formats give
# 128. Fused over library on uniform routing, q4_0 / q8_0: 4.9x / 4.2x at
# T = 1, 3.6x / 3.4x at 64, 2.5x / 2.2x at 128 and 0.86x / 0.80x at 512, in
# both runs. The value equals the bf16 one, the margin at 128 does not: the
# library path pays a dequantise per expert, and between 128 and 512 no T
# was benchmarked.
MOE_WQ_FUSED_MAX_T = 128


def _moe_fmt_pair(fmt):
    f13, f2 = (fmt, fmt) if isinstance(fmt, str) else tuple(fmt)
    wq_bits(f13), wq_bits(f2)
    return f13, f2


def dequantize_experts_wq(qs: torch.Tensor, d: torch.Tensor, fmt: str,
                          dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Expert stack planes [E, rows, ...] -> [E, rows, K] with the torch
    reference (rows are independent, so it is dequantize_wq on E*rows
    rows): d*q in fp32, one rounding to `dtype`."""
    E, rows, nblk = d.shape
    w = dequantize_wq(qs.reshape(E * rows, -1), d.reshape(E * rows, nblk),
                      fmt, dtype)
    return w.view(E, rows, nblk * 32)


def moe_experts_wq(x: torch.Tensor, w13_planes, w2_planes, fmt,
                   topk_ids: torch.Tensor, topk_w: torch.Tensor,
                   fused: bool | None = None, out: torch.Tensor | None = None,
                   act: torch.Tensor | None = None,
                   ypair: torch.Tensor | None = None,
                   scratch: torch.Tensor | None = None) -> torch.Tensor:
    """moe_experts over experts kept as ggml Q4_0/Q8_0 planes.
    w13_planes = (qs [E, 2I, H/2 or H], d fp16 [E, 2I, H/32]), w2_planes =
    (qs [E, H, I/2 or I], d fp16 [E, H, I/32]); `fmt` is "q4_0" / "q8_0" or
    a (w13 format, w2 format) pair.
    GPU, fused=True: moe_align + the two dequant-fused routed GEMM kernels +
    moe_combine; capture-safe, any T. GPU, fused=False: the eager library
    path (one host sync): per non-empty expert dequant_wq of w13[e] into
    `scratch`, F.linear, silu_and_mul, dequant_wq of w2[e] into the same
    scratch (same stream, so ordered), F.linear; scaled into the same fp32
    ypair, the same moe_combine. `scratch` is a contiguous bf16 buffer of at
    least 2*I*H elements, allocated per call when None. fused=None: fused
    up to MOE_WQ_FUSED_MAX_T tokens.
    CPU: moe_experts (the torch reference) on the stacks dequantised to
    bf16, the definition."""
    f13, f2 = _moe_fmt_pair(fmt)
    q13, d13 = w13_planes
    q2, d2 = w2_planes
    if not x.is_cuda:
        return ref.moe_experts(x, dequantize_experts_wq(q13, d13, f13),
                               dequantize_experts_wq(q2, d2, f2),
                               topk_ids, topk_w)
    if x.dim() != 2 or topk_ids.dim() != 2:
        raise ValueError("moe_experts_wq: x must be [T, H] and topk_ids "
                         "[T, k]")
    if d13.dim() != 3 or d2.dim() != 3:
        raise ValueError("moe_experts_wq: scale planes must be 3-D")
    T, k = topk_ids.shape
    E, I, H = d13.shape[0], d13.shape[1] // 2, d13.shape[2] * 32
    P = T * k
    if x.shape[0] != T or tuple(topk_w.shape) != (T, k):
        raise ValueError(
            f"moe_experts_wq: x {tuple(x.shape)}, topk_ids "
            f"{tuple(topk_ids.shape)} and topk_w {tuple(topk_w.shape)} "
            f"disagree on [T, k]")
    if fused is None:
        fused = T <= MOE_WQ_FUSED_MAX_T
    if act is None:
        act = torch.empty(P, I, dtype=torch.bfloat16, device=x.device)
    if ypair is None:
        ypair = torch.empty(P, H, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(T, H, dtype=torch.bfloat16, device=x.device)
    C = _native()
    off = torch.empty(E + 1, dtype=torch.int32, device=x.device)
    pairs = torch.empty(P, dtype=torch.int32, device=x.device)
    C.moe_align(off, pairs, topk_ids, E)
    if fused:
        C.moe_gemm_gated_wq(act, x, q13, d13, wq_bits(f13), off, pairs, k)
        C.moe_gemm_down_wq(ypair, act, q2, d2, wq_bits(f2), topk_w, off,
                           pairs)
    else:
        if x.dtype != torch.bfloat16:
            raise ValueError("moe_experts_wq: x must be bf16 on GPU")
        if tuple(d2.shape) != (E, H, I // 32) or x.shape[1] != H \
                or tuple(act.shape) != (P, I) or tuple(ypair.shape) != (P, H) \
                or ypair.dtype != torch.float32:
            raise ValueError("moe_experts_wq: shape mismatch between x, the "
                             "planes, act and ypair")
        if scratch is None:
            scratch = torch.empty(2 * I * H, dtype=torch.bfloat16,
                                  device=x.device)
        offs = off.tolist()                       # the one host sync
        rows = pairs[:offs[E]].long()
        xg = x[rows // k]
        tw = topk_w.reshape(-1)[rows]
        for e in range(E):
            lo, hi = offs[e], offs[e + 1]
            if hi == lo:
                continue
            w = dequant_wq(q13[e], d13[e], f13, out=scratch)
            a = silu_and_mul(torch.nn.functional.linear(xg[lo:hi], w))
            act[rows[lo:hi]] = a
            w = dequant_wq(q2[e], d2[e], f2, out=scratch)
            y = torch.nn.functional.linear(a, w)
            ypair[rows[lo:hi]] = y.float() * tw[lo:hi, None]
    C.moe_combine(out, ypair, k)
    return out


def moe_forward_wq(x: torch.Tensor, router_logits: torch.Tensor,
                   w13_planes, w2_planes, fmt, k: int,
                   fused: bool | None = None,
                   scratch: torch.Tensor | None = None) -> torch.Tensor:
    """One MoE MLP over quantised experts: route (moe_route) and run the
    routed experts (moe_experts_wq)."""
    ids, w = moe_route(router_logits, k)
    return moe_experts_wq(x, w13_planes, w2_planes, fmt, ids, w, fused=fused,
                          scratch=scratch)


# -- routed expert GEMMs over Q4_K / Q6_K experts (ops/hip/moe_kq.hip) --
# Largest T at which moe_experts_kq(fused=None) takes the fused kernels.
# MOE_FUSED_MAX_T's rule: the largest benchmarked T at which the fused path
# is not slower than this feature's own library path (a dequant_kq per
# non-empty expert) on uniform routing, in two runs of scripts/bench_moe.py
# --fmt q4_k / q6_k; the smaller of the two formats.
# MEASURED, not the placeholder it started as (profiles/r11_moe_kq.md): the
# Mixtral layer decides, and both formats give 128. Fused over library on
# uniform routing, q4_k / q6_k, second run (first): 5.0 (4.7) / 4.0 (3.9) at
# T = 1, 3.5 (3.3) / 2.9 (3.0) at 64, 2.4 (2.3) / 2.2 (2.2) at 128 and 0.87
# (0.82) / 0.79 (0.79) at 512; no T between 128 and 512 was benchmarked. On
# the Qwen3-30B-A3B layer (E = 128) the library path pays up to 256
# dequantise launches and the fused kernels are 20-57x faster at every
# benchmarked T, 512 included: one cutoff for all shapes leaves that on the
# table for eager prefill above 128 tokens.
MOE_KQ_FUSED_MAX_T = 128

_MOE_KQ_NPLANES = {"q4_k": 2, "q6_k": 4}


def moe_kq_waves(N: int, K: int, gated: bool) -> int:
    """K-split factor (waves per workgroup) the K-quant routed GEMM uses for
    one expert's [N, K] weight: the host's own function, a property of the
    shape."""
    return int(_native().moe_kq_waves(N, K, gated))


def _moe_kq_fmt_pair(fmt):
    f13, f2 = (fmt, fmt) if isinstance(fmt, str) else tuple(fmt)
    kq_check(f13), kq_check(f2)
    return f13, f2


def _moe_kq_planes(planes, fmt: str, what: str):
    planes = tuple(planes)
    if len(planes) != _MOE_KQ_NPLANES[fmt]:
        raise ValueError(f"moe_experts_kq: {what} {fmt} takes "
                         f"{_MOE_KQ_NPLANES[fmt]} planes, got {len(planes)}")
    if any(p.dim() < 3 for p in planes):
        raise ValueError(f"moe_experts_kq: {what} planes must be "
                         f"[E, rows, ...]")
    return planes


def dequantize_experts_kq(planes, fmt: str,
                          dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Expert stack planes [E, rows, ...] -> [E, rows, K] with the torch
    reference (a super-block never crosses a row, so it is dequantize_kq on
    E*rows rows)."""
    E, rows = planes[0].shape[:2]
    flat = tuple(p.reshape(E * rows, *p.shape[2:]) for p in planes)
    return dequantize_kq(flat, fmt, dtype).view(E, rows, -1)


def moe_experts_kq(x: torch.Tensor, w13_planes, w2_planes, fmt,
                   topk_ids: torch.Tensor, topk_w: torch.Tensor,
                   fused: bool | None = None, out: torch.Tensor | None = None,
                   act: torch.Tensor | None = None,
                   ypair: torch.Tensor | None = None,
                   scratch: torch.Tensor | None = None) -> torch.Tensor:
    """moe_experts over experts kept as ggml Q4_K/Q6_K planes, gemm_kq's
    planes with the expert in front: q4_k (qs [E, rows, K/2], hdr
    [E, rows, K/256, 16]), q6_k (ql [E, rows, K/2], qh [E, rows, K/4], sc int8
    [E, rows, K/16], d fp16 [E, rows, K/256]); rows = 2I, K = H for w13 and
    rows = H, K = I for w2. `fmt` is "q4_k" / "q6_k" or a (w13 format, w2
    format) pair; gate and up share a format.
    GPU, fused=True: moe_align + the two dequant-fused routed GEMM kernels +
    moe_combine; capture-safe, any T. GPU, fused=False: the eager library
    path (one host sync): per non-empty expert dequant_kq of w13[e]'s plane
    slices into `scratch`, F.linear, silu_and_mul, dequant_kq of w2[e] into
    the same scratch (same stream, so ordered), F.linear; scaled into the
    same fp32 ypair, the same moe_combine. `scratch` is a contiguous bf16
    buffer of at least 2*I*H elements, allocated per call when None.
    fused=None: fused up to MOE_KQ_FUSED_MAX_T tokens.
    CPU: moe_experts (the torch reference) on the stacks dequantised to
    bf16, the definition."""
    f13, f2 = _moe_kq_fmt_pair(fmt)
    p13 = _moe_kq_planes(w13_planes, f13, "w13")
    p2 = _moe_kq_planes(w2_planes, f2, "w2")
    if not x.is_cuda:
        return ref.moe_experts(x, dequantize_experts_kq(p13, f13),
                               dequantize_experts_kq(p2, f2),
                               topk_ids, topk_w)
    if x.dim() != 2 or topk_ids.dim() != 2:
        raise ValueError("moe_experts_kq: x must be [T, H] and topk_ids "
                         "[T, k]")
    T, k = topk_ids.shape
    E, I, H = p13[0].shape[0], p13[0].shape[1] // 2, p13[0].shape[2] * 2
    P = T * k
    if x.shape[0] != T or tuple(topk_w.shape) != (T, k):
        raise ValueError(
            f"moe_experts_kq: x {tuple(x.shape)}, topk_ids "
            f"{tuple(topk_ids.shape)} and topk_w {tuple(topk_w.shape)} "
            f"disagree on [T, k]")
    if fused is None:
        fused = T <= MOE_KQ_FUSED_MAX_T
    if act is None:
        act = torch.empty(P, I, dtype=torch.bfloat16, device=x.device)
    if ypair is None:
        ypair = torch.empty(P, H, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(T, H, dtype=torch.bfloat16, device=x.device)
    C = _native()
    off = torch.empty(E + 1, dtype=torch.int32, device=x.device)
    pairs = torch.empty(P, dtype=torch.int32, device=x.device)
    C.moe_align(off, pairs, topk_ids, E)
    if fused:
        C.moe_gemm_gated_kq(act, x, list(p13), f13, off, pairs, k)
        C.moe_gemm_down_kq(ypair, act, list(p2), f2, topk_w, off, pairs)
    else:
        if x.dtype != torch.bfloat16:
            raise ValueError("moe_experts_kq: x must be bf16 on GPU")
        if tuple(p2[0].shape) != (E, H, I // 2) or x.shape[1] != H \
                or tuple(act.shape) != (P, I) or tuple(ypair.shape) != (P, H) \
                or ypair.dtype != torch.float32:
            raise ValueError("moe_experts_kq: shape mismatch between x, the "
                             "planes, act and ypair")
        if scratch is None:
            scratch = torch.empty(2 * I * H, dtype=torch.bfloat16,
                                  device=x.device)
        offs = off.tolist()                       # the one host sync
        rows = pairs[:offs[E]].long()
        xg = x[rows // k]
        tw = topk_w.reshape(-1)[rows]
        for e in range(E):
            lo, hi = offs[e], offs[e + 1]
            if hi == lo:
                continue
            w = dequant_kq([p[e] for p in p13], f13, out=scratch)
            a = silu_and_mul(torch.nn.functional.linear(xg[lo:hi], w))
            act[rows[lo:hi]] = a
            w = dequant_kq([p[e] for p in p2], f2, out=scratch)
            y = torch.nn.functional.linear(a, w)
            ypair[rows[lo:hi]] = y.float() * tw[lo:hi, None]
    C.moe_combine(out, ypair, k)
    return out


def moe_forward_kq(x: torch.Tensor, router_logits: torch.Tensor,
                   w13_planes, w2_planes, fmt, k: int,
                   fused: bool | None = None,
                   scratch: torch.Tensor | None = None) -> torch.Tensor:
    """One MoE MLP over K-quant experts: route (moe_route) and run the
    routed experts (moe_experts_kq)."""
    ids, w = moe_route(router_logits, k)
    return moe_experts_kq(x, w13_planes, w2_planes, fmt, ids, w, fused=fused,
                          scratch=scratch)


def mfma_probe(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    d = torch.empty(16, 16, dtype=torch.float32, device=a.device)
    _native().mfma_probe(d, a, b)
    return d


def lora_shrink(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
                slot: torch.Tensor) -> torch.Tensor:
    """y[T,Rtot] (fp32, in place) = per-row A[slot[t]] @ x[t]. Rows whose
    slot is outside [0, S) are not written."""
    if x.is_cuda:
        _native().lora_shrink(y, x, A, slot)
        return y
    return ref.lora_shrink(y, x, A, slot)


def lora_expand(out: torch.Tensor, y: torch.Tensor, B: torch.Tensor,
                slot: torch.Tensor, scale: torch.Tensor,
                n_off) -> torch.Tensor:
    """out[T,N] += scale[s] * per-row B[slot[t]] @ y[t], in place. n_off is
    a host sequence of slice boundaries (0, ..., N)."""
    if out.is_cuda:
        _native().lora_expand(out, y, B, slot, scale,
                              [int(v) for v in n_off])
        return out
    return ref.lora_expand(out, y, B, slot, scale, n_off)


def lora_apply(out: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
               B: torch.Tensor, slot: torch.Tensor, scale: torch.Tensor,
               n_off) -> torch.Tensor:
    """Shrink + expand: adds each row's adapter delta into `out` in place.
    Rows with no adapter (slot outside [0, S)) keep `out` bit-identical."""
    y = torch.empty(x.shape[0], A.shape[1], dtype=torch.float32,
                    device=x.device)
    lora_shrink(y, x, A, slot)
    return lora_expand(out, y, B, slot, scale, n_off)
