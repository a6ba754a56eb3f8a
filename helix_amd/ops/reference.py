"""Pure-PyTorch fp32 reference implementations of every HIP kernel.

These define the numerics contract: GPU tests compare the CDNA4 kernels
against these (run in fp32) within bf16 tolerance. They also serve the
CPU-only paths (unit tests, engine logic tests on this no-GPU container).
"""
from __future__ import annotations

import torch


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps) * w.float()
    return out.to(x.dtype)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor,
                       w: torch.Tensor, eps: float):
    """Returns (normed, new_residual); mirrors the in-place HIP op."""
    new_res = (x.float() + residual.float()).to(x.dtype)
    return rms_norm(new_res, w, eps), new_res


def qk_rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float,
                head_dim: int) -> torch.Tensor:
    """Qwen3 QK-norm: RMSNorm of every head of x [T, H*head_dim] over that
    head's head_dim elements, times w [head_dim]. Returns fp32, unrounded:
    the rope that follows rounds once (rope_qkv_norm.hip does the same)."""
    T = x.shape[0]
    xf = x.float().view(T, -1, head_dim)
    var = xf.pow(2).mean(-1, keepdim=True)
    return (xf * torch.rsqrt(var + eps) * w.float()).view(T, -1)


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
               eps: float) -> torch.Tensor:
    return torch.nn.functional.layer_norm(
        x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(x.dtype)


def rotary_embedding(positions: torch.Tensor, q: torch.Tensor,
                     k: torch.Tensor, cos_sin: torch.Tensor, head_dim: int):
    """Neox-style rotate-half RoPE, applied out-of-place; returns (q, k)."""
    half = head_dim // 2
    cs = cos_sin[positions]  # [T, D]
    cos = cs[:, :half].float()  # [T, half]
    sin = cs[:, half:].float()

    def rot(t: torch.Tensor) -> torch.Tensor:
        T = t.shape[0]
        th = t.float().view(T, -1, head_dim)
        x1, x2 = th[..., :half], th[..., half:]
        c = cos.unsqueeze(1)
        s = sin.unsqueeze(1)
        out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
        return out.view(t.shape).to(t.dtype)

    return rot(q), rot(k)


def make_cos_sin_cache(head_dim: int, max_pos: int, base: float = 10000.0,
                       device="cpu",
                       rope_scaling: dict | None = None) -> torch.Tensor:
    """[max_pos, D] fp32 rows = [cos(0..D/2), sin(0..D/2)].

    rope_scaling supports the llama3.1 scheme (HF config.json
    rope_scaling: rope_type "llama3" with factor / low_freq_factor /
    high_freq_factor / original_max_position_embeddings): wavelengths
    longer than original/low_freq are divided by `factor`, shorter than
    original/high_freq are untouched, with a smooth ramp between —
    the long-context extension Llama-3.1 ships with."""
    import math
    half = head_dim // 2
    inv_freq = 1.0 / (base ** (torch.arange(half, dtype=torch.float32,
                                            device=device) / half))
    if rope_scaling and rope_scaling.get("rope_type", rope_scaling.get(
            "type", "")) == "llama3":
        factor = float(rope_scaling.get("factor", 8.0))
        lo = float(rope_scaling.get("low_freq_factor", 1.0))
        hi = float(rope_scaling.get("high_freq_factor", 4.0))
        orig = float(rope_scaling.get(
            "original_max_position_embeddings", 8192))
        wavelen = 2 * math.pi / inv_freq
        low_wl = orig / lo
        high_wl = orig / hi
        scaled = inv_freq / factor
        # smooth interpolation in the medium-frequency band
        smooth = (orig / wavelen - lo) / (hi - lo)
        smooth = smooth.clamp(0.0, 1.0)
        mid = (1 - smooth) * scaled + smooth * inv_freq
        inv_freq = torch.where(wavelen > low_wl, scaled,
                               torch.where(wavelen < high_wl,
                                           inv_freq, mid))
    t = torch.arange(max_pos, dtype=torch.float32, device=device)
    freqs = torch.outer(t, inv_freq)  # [max_pos, half]
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    i = x.shape[-1] // 2
    g, u = x[..., :i].float(), x[..., i:].float()
    return (torch.nn.functional.silu(g) * u).to(x.dtype)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.gelu(x.float(), approximate="tanh").to(x.dtype)


def reshape_and_cache(k: torch.Tensor, v: torch.Tensor,
                      k_cache: torch.Tensor, v_cache: torch.Tensor,
                      slot_mapping: torch.Tensor):
    """k/v: [T, Hkv, D]; caches: [nblocks, Hkv, bs, D]."""
    bs = k_cache.shape[2]
    for t in range(slot_mapping.shape[0]):
        slot = int(slot_mapping[t])
        if slot < 0:
            continue
        b, off = slot // bs, slot % bs
        k_cache[b, :, off] = k[t]
        v_cache[b, :, off] = v[t]


def attn_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 cu_seqlens: torch.Tensor, max_seqlen: int,
                 scale: float, causal: bool = True,
                 window: int = 0, cu_seqlens_k=None) -> torch.Tensor:
    """Varlen causal GQA attention (optional sliding window and
    cached-prefix query offset). q: [T, Hq, D], k/v: [Tk, Hkv, D]."""
    Hq, Hkv = q.shape[1], k.shape[1]
    G = Hq // Hkv
    if cu_seqlens_k is None:
        cu_seqlens_k = cu_seqlens
    out = torch.empty_like(q)
    for i in range(cu_seqlens.shape[0] - 1):
        qs0, qe = int(cu_seqlens[i]), int(cu_seqlens[i + 1])
        ks0, ke = int(cu_seqlens_k[i]), int(cu_seqlens_k[i + 1])
        qlen, klen = qe - qs0, ke - ks0
        ctx = klen - qlen
        qs = q[qs0:qe].float()
        ks = k[ks0:ke].float().repeat_interleave(G, dim=1)
        vs = v[ks0:ke].float().repeat_interleave(G, dim=1)
        qpos = torch.arange(ctx, klen)
        kpos = torch.arange(klen)
        if causal:
            m = kpos[None, :] <= qpos[:, None]
            if window > 0:
                m &= (qpos[:, None] - kpos[None, :]) < window
        else:
            m = torch.ones(qlen, klen, dtype=torch.bool)
        mask = torch.where(m, 0.0, float("-inf"))
        o = torch.nn.functional.scaled_dot_product_attention(
            qs.transpose(0, 1), ks.transpose(0, 1), vs.transpose(0, 1),
            attn_mask=mask, scale=scale)
        out[qs0:qe] = o.transpose(0, 1).to(q.dtype)
    return out


def paged_attn_decode(q: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, block_tables: torch.Tensor,
                      seq_lens: torch.Tensor, scale: float,
                      window: int = 0) -> torch.Tensor:
    """q: [B, Hq, D] single token per seq. Gathers KV then full attention."""
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    bs = k_cache.shape[2]
    G = Hq // Hkv
    out = torch.empty_like(q)
    for b in range(B):
        L = int(seq_lens[b])
        nb = (L + bs - 1) // bs
        blocks = block_tables[b, :nb].long()
        k = k_cache[blocks].permute(0, 2, 1, 3).reshape(nb * bs, Hkv, D)[:L]
        v = v_cache[blocks].permute(0, 2, 1, 3).reshape(nb * bs, Hkv, D)[:L]
        if window > 0:
            k = k[max(0, L - window):]
            v = v[max(0, L - window):]
        kf = k.float().repeat_interleave(G, dim=1)  # [L, Hq, D]
        vf = v.float().repeat_interleave(G, dim=1)
        qf = q[b].float()  # [Hq, D]
        s = torch.einsum("hd,lhd->hl", qf, kf) * scale
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hl,lhd->hd", p, vf)
        out[b] = o.to(q.dtype)
    return out


def sample_tokens(logits: torch.Tensor, temperatures: torch.Tensor,
                  seeds: torch.Tensor) -> torch.Tensor:
    """Greedy for T<=0; Gumbel-max for T>0 driven by the per-row seeds.

    Seed-determinism matters even on CPU: SPMD-TP ranks each run this
    sampler and must pick identical tokens (the HIP kernel derives its
    Gumbel noise from the same seeds; distribution-equal, not bit-equal
    — GPU tests check greedy exactly and stochastic statistically).
    """
    out = torch.empty(logits.shape[0], dtype=torch.int64,
                      device=logits.device)
    for i in range(logits.shape[0]):
        t = float(temperatures[i])
        row = logits[i].float()
        if t <= 0:
            out[i] = int(row.argmax())
        else:
            g = torch.Generator()
            g.manual_seed(int(seeds[i]) & 0x7FFFFFFFFFFFFFFF)
            u = torch.rand(row.shape[0], generator=g)
            gumbel = -torch.log(-torch.log(u.clamp(min=1e-20)))
            out[i] = int((row / t + gumbel).argmax())
    return out


def gemm_bf16(x: torch.Tensor, w: torch.Tensor, bias=None,
              act: int = 0) -> torch.Tensor:
    out = x.float() @ w.float().t()
    if bias is not None:
        out = out + bias.float()
    if act == 1:
        out = torch.nn.functional.gelu(out, approximate="tanh")
    return out.to(x.dtype)


def lora_shrink(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
                slot: torch.Tensor) -> torch.Tensor:
    """y[t, :] = A[slot[t]] @ x[t] in fp32 for rows whose slot is in
    [0, S); other rows of y are left untouched. x[T,K], A[S,Rtot,K],
    y[T,Rtot] fp32 (written in place and returned)."""
    S = A.shape[0]
    sl = slot.long()
    for s in torch.unique(sl).tolist():
        if s < 0 or s >= S:
            continue
        rows = (sl == s).nonzero(as_tuple=True)[0]
        y[rows] = x[rows].float() @ A[s].float().t()
    return y


def lora_expand(out: torch.Tensor, y: torch.Tensor, B: torch.Tensor,
                slot: torch.Tensor, scale: torch.Tensor,
                n_off) -> torch.Tensor:
    """out[t, n] += scale[s] * sum_j y[t, i(n)*Rmax + j] * B[s, n, j] for
    rows whose slot s is in [0, S); other rows stay bit-identical.
    out[T,N] (in place), y[T,Rtot] fp32, B[S,N,Rmax]; slice i owns output
    columns [n_off[i], n_off[i+1]) and y columns [i*Rmax, (i+1)*Rmax)."""
    S, _, R = B.shape
    sl = slot.long()
    for s in torch.unique(sl).tolist():
        if s < 0 or s >= S:
            continue
        rows = (sl == s).nonzero(as_tuple=True)[0]
        delta = torch.cat(
            [y[rows, i * R:(i + 1) * R].float()
             @ B[s, n_off[i]:n_off[i + 1]].float().t()
             for i in range(len(n_off) - 1)], dim=1)
        out[rows] = (out[rows].float()
                     + scale[s].float() * delta).to(out.dtype)
    return out


# -- ggml Q4_0 / Q8_0 weight-only formats -------------------------------
# Blocks of 32 consecutive elements along K with one fp16 scale each.
# Device layout is two planes: the blocks' payload bytes, unchanged and in
# order (qs: uint8 [N, K/2] for q4_0, int8 [N, K] for q8_0) and the scales
# (d: fp16 [N, K/32]).

WQ_BLOCK = 32
WQ_FORMATS = {"q4_0": (4, 16, 18), "q8_0": (8, 32, 34)}   # bits, payload, block


def wq_bits(fmt: str) -> int:
    if fmt not in WQ_FORMATS:
        raise ValueError(f"unknown weight-only format {fmt!r} "
                         f"(expected one of {sorted(WQ_FORMATS)})")
    return WQ_FORMATS[fmt][0]


def quantize_wq(w: torch.Tensor, fmt: str):
    """ggml's reference quantizer. w [N, K] -> (qs, d) planes."""
    bits = wq_bits(fmt)
    if w.dim() != 2 or w.shape[1] % WQ_BLOCK:
        raise ValueError(f"quantize_wq: need [N, K] with K % 32 == 0, "
                         f"got {tuple(w.shape)}")
    N, K = w.shape
    x = w.detach().float().reshape(N, K // WQ_BLOCK, WQ_BLOCK)
    if bits == 4:
        idx = x.abs().argmax(dim=-1, keepdim=True)
        mx = x.gather(-1, idx)                  # signed, largest magnitude
        d = mx / -8.0
        inv = torch.where(d != 0, 1.0 / d, torch.zeros_like(d))
        nib = (x * inv + 8.5).to(torch.int32).clamp_(max=15)   # truncation
        nib = nib.to(torch.uint8)
        qs = (nib[..., :16] | (nib[..., 16:] << 4)).reshape(N, K // 2)
    else:
        d = x.abs().amax(dim=-1, keepdim=True) / 127.0
        inv = torch.where(d != 0, 1.0 / d, torch.zeros_like(d))
        v = x * inv
        q = torch.sign(v) * torch.floor(v.abs() + 0.5)         # roundf
        qs = q.to(torch.int8).reshape(N, K)
    return qs.contiguous(), d.squeeze(-1).to(torch.float16).contiguous()


def dequantize_wq(qs: torch.Tensor, d: torch.Tensor, fmt: str,
                  dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Planes -> [N, K]: d * (nib - 8) resp. d * q in fp32, one rounding
    to `dtype`."""
    bits = wq_bits(fmt)
    N, nblk = d.shape
    df = d.float().unsqueeze(-1)
    if bits == 4:
        b = qs.reshape(N, nblk, 16)
        q = torch.cat([b & 0x0F, b >> 4], dim=-1).float() - 8.0
    else:
        q = qs.reshape(N, nblk, 32).float()
    return (df * q).reshape(N, nblk * WQ_BLOCK).to(dtype)


def pack_ggml(qs: torch.Tensor, d: torch.Tensor, fmt: str) -> bytes:
    """Planes -> ggml block bytes (fp16 d, then the payload, per block)."""
    wq_bits(fmt)
    payload = WQ_FORMATS[fmt][1]
    N, nblk = d.shape
    db = d.detach().cpu().contiguous().view(torch.uint8).reshape(N, nblk, 2)
    qb = qs.detach().cpu().contiguous().view(torch.uint8).reshape(
        N, nblk, payload)
    return torch.cat([db, qb], dim=-1).contiguous().numpy().tobytes()


def unpack_ggml(raw, shape, fmt: str):
    """ggml block bytes of a [N, K] tensor -> (qs, d) planes: a strided
    copy, no re-encoding."""
    bits = wq_bits(fmt)
    _, payload, blk = WQ_FORMATS[fmt]
    N, K = shape
    if K % WQ_BLOCK:
        raise ValueError(f"unpack_ggml: K={K} is not a multiple of 32")
    nblk = K // WQ_BLOCK
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    if buf.numel() != N * nblk * blk:
        raise ValueError(f"unpack_ggml: {buf.numel()} bytes for shape "
                         f"{tuple(shape)} {fmt}, expected {N * nblk * blk}")
    b = buf.reshape(N, nblk, blk)
    d = b[..., :2].contiguous().view(torch.float16).reshape(N, nblk)
    qs = b[..., 2:].contiguous().reshape(N, nblk * payload)
    if bits == 8:
        qs = qs.view(torch.int8)
    return qs, d


# -- ggml K-quant weight-only formats: Q4_K / Q6_K ----------------------
# Super-blocks of 256 consecutive elements along K. Device layout is the
# block's fields as planes, byte for byte as in the file (unpack is a
# strided copy, pack its exact inverse; scales are NOT pre-multiplied into a
# wider plane, which would cost a third more weight bytes):
#   q4_k: (qs  uint8 [N, K/2],          128 nibble bytes per super-block
#          hdr uint8 [N, K/256, 16])    d fp16, dmin fp16, scales[12]
#   q6_k: (ql  uint8 [N, K/2], qh uint8 [N, K/4], sc int8 [N, K/16],
#          d   fp16  [N, K/256])
# docs/KERNELS.md has the bit layout. No file written by llama.cpp has been
# read with this code yet.

KQ_BLOCK = 256
KQ_FORMATS = {"q4_k", "q6_k"}
KQ_BLOCK_BYTES = {"q4_k": 144, "q6_k": 210}


def kq_check(fmt: str) -> str:
    if fmt not in KQ_FORMATS:
        raise ValueError(f"unknown K-quant format {fmt!r} "
                         f"(expected one of {sorted(KQ_FORMATS)})")
    return fmt


def kq_shape(planes, fmt: str):
    """(N, K) of a plane tuple."""
    kq_check(fmt)
    return planes[0].shape[0], planes[0].shape[1] * 2


def _q4k_scale_min(hdr: torch.Tensor):
    """hdr [..., 16] uint8 -> (d*sc, dmin*m), each fp32 [..., 8]."""
    d = hdr[..., 0:2].contiguous().view(torch.float16).float()      # [..., 1]
    dmin = hdr[..., 2:4].contiguous().view(torch.float16).float()
    s = hdr[..., 4:16].to(torch.int32)
    sc = torch.cat([s[..., 0:4] & 63,
                    (s[..., 8:12] & 0xF) | ((s[..., 0:4] >> 6) << 4)], -1)
    m = torch.cat([s[..., 4:8] & 63,
                   (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], -1)
    return d * sc.float(), dmin * m.float()


def dequantize_kq(planes, fmt: str,
                  dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Planes -> [N, K]. Q4_K: (d*sc)*nib - dmin*m, Q6_K: (d*sc)*q, in fp32
    in that order (one fp32 rounding each), then one rounding to `dtype`."""
    kq_check(fmt)
    N, K = kq_shape(planes, fmt)
    nb = K // KQ_BLOCK
    if fmt == "q4_k":
        qs, hdr = planes
        ds, dm = _q4k_scale_min(hdr)                          # [N, nb, 8]
        b = qs.reshape(N, nb, 4, 1, 32)
        # bytes 32c..32c+31: low nibbles are sub-block 2c, high 2c+1
        nib = torch.cat([b & 0x0F, b >> 4], dim=3).reshape(N, nb, 8, 32)
        y = ds[..., None] * nib.float() - dm[..., None]
    else:
        ql, qh, sc, d = planes
        b = ql.reshape(N, nb, 2, 2, 32)                       # half, g&1, l
        low = torch.cat([b & 0x0F, b >> 4], dim=3)            # half, g, l
        h = qh.reshape(N, nb, 2, 1, 32)
        shift = torch.tensor([0, 2, 4, 6], dtype=torch.uint8).view(4, 1)
        high = (h >> shift) & 3
        q = (low | (high << 4)).to(torch.int32) - 32          # [N,nb,2,4,32]
        s = d.float().reshape(N, nb, 1) * sc.reshape(N, nb, 16).float()
        s = s.reshape(N, nb, 2, 4, 2, 1)                      # 8h + 2g + l/16
        y = s * q.reshape(N, nb, 2, 4, 2, 16).float()
    return y.reshape(N, K).to(dtype)


def _nearest(v: torch.Tensor) -> torch.Tensor:
    return torch.floor(v + 0.5)


def _safe_div(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.where(b != 0, a / torch.where(b != 0, b, torch.ones_like(b)),
                       torch.zeros_like(a))


def quantize_kq(w: torch.Tensor, fmt: str):
    """A plain deterministic K-quant quantizer, NOT ggml's search quantizer
    (make_qkx2_quants / make_qx_quants): it only has to write valid blocks.
    w [N, K] -> planes.

    Q4_K, per 32-element sub-block: m = max(0, -min), s = (max + m) / 15;
    per super-block d = max_j s / 63 and dmin = max_j m / 63, stored as fp16;
    the 6-bit codes and the nibbles are rounded to nearest and clamped.
    Q6_K: the per-16 scale is the signed value of largest magnitude over
    -32, d = max |scale| / 127 as fp16, int8 scale codes and q rounded to
    nearest, q clamped to [-32, 31]. All-zero blocks give all-zero fields."""
    kq_check(fmt)
    if w.dim() != 2 or w.shape[1] % KQ_BLOCK:
        raise ValueError(f"quantize_kq: need [N, K] with K % 256 == 0, "
                         f"got {tuple(w.shape)}")
    N, K = w.shape
    nb = K // KQ_BLOCK
    if fmt == "q4_k":
        x = w.detach().float().reshape(N, nb, 8, 32)
        m = x.amin(-1).clamp_(max=0).abs_()                    # [N, nb, 8]
        s = (x.amax(-1) + m) / 15.0
        d = (s.amax(-1, keepdim=True) / 63.0).to(torch.float16)
        dmin = (m.amax(-1, keepdim=True) / 63.0).to(torch.float16)
        sc = _nearest(_safe_div(s, d.float())).clamp_(0, 63)
        mc = _nearest(_safe_div(m, dmin.float())).clamp_(0, 63)
        ds, dm = d.float() * sc, dmin.float() * mc             # as decoded
        nib = _nearest(_safe_div(x + dm[..., None], ds[..., None]))
        nib = nib.clamp_(0, 15).to(torch.uint8).reshape(N, nb, 4, 2, 32)
        qs = (nib[..., 0, :] | (nib[..., 1, :] << 4)).reshape(N, K // 2)
        sc, mc = sc.to(torch.uint8), mc.to(torch.uint8)
        scales = torch.cat([
            sc[..., :4] | ((sc[..., 4:] >> 4) << 6),
            mc[..., :4] | ((mc[..., 4:] >> 4) << 6),
            (sc[..., 4:] & 0xF) | ((mc[..., 4:] & 0xF) << 4)], -1)
        hdr = torch.cat([d.view(torch.uint8), dmin.view(torch.uint8), scales],
                        -1)
        return qs.contiguous(), hdr.contiguous()
    x = w.detach().float().reshape(N, nb, 16, 16)
    idx = x.abs().argmax(dim=-1, keepdim=True)
    s = x.gather(-1, idx).squeeze(-1) / -32.0                  # [N, nb, 16]
    d = (s.abs().amax(-1, keepdim=True) / 127.0).to(torch.float16)
    sc = _nearest(_safe_div(s, d.float())).clamp_(-128, 127)
    ds = d.float() * sc
    q = _nearest(_safe_div(x, ds[..., None])).clamp_(-32, 31)
    u = (q + 32).to(torch.uint8).reshape(N, nb, 2, 4, 32)      # half, g, l
    lo4, hi2 = u & 0x0F, u >> 4
    ql = (lo4[..., :2, :] | (lo4[..., 2:, :] << 4)).reshape(N, K // 2)
    qh = (hi2[..., 0, :] | (hi2[..., 1, :] << 2) | (hi2[..., 2, :] << 4)
          | (hi2[..., 3, :] << 6)).reshape(N, K // 4)
    return (ql.contiguous(), qh.contiguous(),
            sc.to(torch.int8).reshape(N, K // 16).contiguous(),
            d.reshape(N, nb).contiguous())


def pack_ggml_kq(planes, fmt: str) -> bytes:
    """Planes -> ggml super-block bytes (block_q4_K: d, dmin, scales[12],
    qs[128]; block_q6_K: ql[128], qh[64], scales[16], d)."""
    kq_check(fmt)
    N, K = kq_shape(planes, fmt)
    nb = K // KQ_BLOCK
    ps = [p.detach().cpu().contiguous() for p in planes]
    if fmt == "q4_k":
        parts = [ps[1].reshape(N, nb, 16), ps[0].reshape(N, nb, 128)]
    else:
        parts = [ps[0].reshape(N, nb, 128), ps[1].reshape(N, nb, 64),
                 ps[2].view(torch.uint8).reshape(N, nb, 16),
                 ps[3].view(torch.uint8).reshape(N, nb, 2)]
    return torch.cat(parts, dim=-1).contiguous().numpy().tobytes()


def unpack_ggml_kq(raw, shape, fmt: str):
    """ggml super-block bytes of a [N, K] tensor -> planes: a strided copy,
    no re-encoding."""
    kq_check(fmt)
    N, K = shape
    if K % KQ_BLOCK:
        raise ValueError(f"unpack_ggml_kq: K={K} is not a multiple of 256")
    nb, bsz = K // KQ_BLOCK, KQ_BLOCK_BYTES[fmt]
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    if buf.numel() != N * nb * bsz:
        raise ValueError(f"unpack_ggml_kq: {buf.numel()} bytes for shape "
                         f"{tuple(shape)} {fmt}, expected {N * nb * bsz}")
    b = buf.reshape(N, nb, bsz)
    if fmt == "q4_k":
        return (b[..., 16:].contiguous().reshape(N, K // 2),
                b[..., :16].contiguous())
    return (b[..., :128].contiguous().reshape(N, K // 2),
            b[..., 128:192].contiguous().reshape(N, K // 4),
            b[..., 192:208].contiguous().view(torch.int8).reshape(N, K // 16),
            b[..., 208:210].contiguous().view(torch.float16).reshape(N, nb))


# -- mixture of experts (ops/hip/moe.hip) --------------------------------

def moe_route(logits: torch.Tensor, k: int):
    """Mixtral routing: fp32 softmax over the E experts, the k largest kept
    and renormalised to sum 1. Slot j holds the j-th largest expert; equal
    logits go to the lower expert index (a stable descending sort).
    Returns (topk_ids [T, k] int32, topk_w [T, k] fp32)."""
    lf = logits.float()
    order = torch.sort(lf, dim=-1, descending=True, stable=True).indices
    ids = order[:, :k]
    p = torch.softmax(lf, dim=-1).gather(-1, ids)
    return ids.to(torch.int32), p / p.sum(-1, keepdim=True)


def moe_align(topk_ids: torch.Tensor, E: int):
    """(expert_off [E+1] int32, sorted_pairs [P] int32): for each expert its
    pair indices (p = t*k + j) in ascending order. Ids outside [0, E)
    belong to no list; the tail of sorted_pairs past expert_off[E] is 0."""
    flat = topk_ids.reshape(-1).long()
    P = flat.numel()
    valid = (flat >= 0) & (flat < E)
    key = torch.where(valid, flat, torch.full_like(flat, E))
    order = torch.sort(key, stable=True).indices
    counts = torch.bincount(key, minlength=E + 1)[:E]
    off = torch.zeros(E + 1, dtype=torch.int64, device=flat.device)
    off[1:] = counts.cumsum(0)
    pairs = order.clone()
    pairs[int(off[E]):] = 0
    assert pairs.numel() == P
    return off.to(torch.int32), pairs.to(torch.int32)


def moe_combine(ypair: torch.Tensor, k: int) -> torch.Tensor:
    """out[t] = bf16(sum_j ypair[t*k + j]) in ascending j, fp32."""
    P, H = ypair.shape
    y = ypair.float().view(P // k, k, H)
    out = y[:, 0].clone()
    for j in range(1, k):
        out += y[:, j]
    return out.to(torch.bfloat16)


def moe_experts(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor,
                topk_ids: torch.Tensor, topk_w: torch.Tensor) -> torch.Tensor:
    """out[t] = sum_j topk_w[t, j] * down_e(silu(gate_e(x[t])) * up_e(x[t])),
    e = topk_ids[t, j]. Rounds where the kernels round: fp32 accumulation,
    the activation to bf16, fp32 per-pair results, one rounding of the sum."""
    T, k = topk_ids.shape
    E, I2, H = w13.shape
    I = I2 // 2
    off, pairs = moe_align(topk_ids, E)
    off = off.tolist()
    ypair = torch.zeros(T * k, H, dtype=torch.float32, device=x.device)
    xf = x.float()
    twf = topk_w.reshape(-1).float()
    for e in range(E):
        p = pairs[off[e]:off[e + 1]].long()
        if p.numel() == 0:
            continue
        gu = xf[p // k] @ w13[e].float().t()
        act = (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]) \
            .to(torch.bfloat16)
        ypair[p] = (act.float() @ w2[e].float().t()) * twf[p, None]
    return moe_combine(ypair, k).to(x.dtype)
