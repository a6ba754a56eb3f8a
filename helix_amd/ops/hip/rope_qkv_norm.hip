// Fused QKV epilogue with QK-norm (Qwen3): rope_qkv.hip's single pass with
// a per-head RMSNorm of Q and of K in front of the rotation.
//
//   r   = rsqrt(mean_d(x_d^2) + eps)          fp32, over one head's D elements
//   y_d = x_d * r * w_d                       w = q_norm_w / k_norm_w
//   (z_d, z_{d+D/2}) = rope(y_d, y_{d+D/2})   rotate-half, fp32 table
//
// One workgroup per token, 4 waves. A head occupies D/2 adjacent lanes:
// lane d of the group holds elements d and d + D/2, which is the rope pair,
// so the only cross-lane traffic is the sum of squares (log2(D/2) xor
// shuffles that never leave the group) and the rotation needs no exchange.
// At D = 128 that is one head per wave, at D = 64 two. Each 2-byte load or
// store of a group covers D/2 consecutive bf16, so a wave touches whole
// 128-byte (D = 128) or 64-byte (D = 64) runs. Values stay in fp32 from the
// load to one final rounding: bf16 for q_out / k_out / a bf16 cache, e4m3
// straight from fp32 for an fp8 cache. No LDS, no barrier, no atomics.
//
// Outputs, V pass-through, slot < 0 handling and the strided qkv row are
// those of rope_qkv_cache_kernel, which is left as it is: models without
// QK-norm keep launching it.
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

constexpr int QKN_THREADS = 256;

template <int D>
__global__ __launch_bounds__(QKN_THREADS) void rope_qkv_norm_cache_kernel(
    const int64_t* __restrict__ positions,
    const uint16_t* __restrict__ qkv, int64_t qkv_stride,
    uint16_t* __restrict__ q_out,
    uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
    const int64_t* __restrict__ slot_mapping,
    uint16_t* __restrict__ k_out, uint16_t* __restrict__ v_out,
    const float* __restrict__ cos_sin,
    const uint16_t* __restrict__ q_norm_w,
    const uint16_t* __restrict__ k_norm_w, float eps,
    int Hq, int Hkv, int block_size, int kv8) {
  constexpr int HALF = D / 2;               // lanes per head
  constexpr int HPW = WAVE / HALF;          // heads per wave
  constexpr int HPB = HPW * (QKN_THREADS / WAVE);   // heads per pass
  const int t = blockIdx.x;
  const int64_t pos = positions[t];
  const float* cs = cos_sin + pos * D;
  const uint16_t* src = qkv + (int64_t)t * qkv_stride;
  const int64_t slot = slot_mapping ? slot_mapping[t] : -1;
  int64_t cblock = 0;
  int coff = 0;
  if (slot >= 0) {
    cblock = slot / block_size;
    coff = (int)(slot % block_size);
  }

  // --- Q and K heads: norm, weight, rotate (q heads first, then k) ---
  const int d = threadIdx.x % HALF;
  const int hsub = threadIdx.x / HALF;      // head within a pass
  const float c = cs[d];
  const float sn = cs[HALF + d];
  const float wq1 = bf16_to_f32(q_norm_w[d]);
  const float wq2 = bf16_to_f32(q_norm_w[d + HALF]);
  const float wk1 = bf16_to_f32(k_norm_w[d]);
  const float wk2 = bf16_to_f32(k_norm_w[d + HALF]);
  const int nheads = Hq + Hkv;
  // the trip count is the same for every lane of the workgroup; a group
  // past the last head runs the shuffles on zeros and stores nothing
  for (int h0 = 0; h0 < nheads; h0 += HPB) {
    const int h = h0 + hsub;
    const bool live = h < nheads;
    float x1 = 0.f, x2 = 0.f;
    if (live) {
      const uint16_t* b = src + h * D;
      x1 = bf16_to_f32(b[d]);
      x2 = bf16_to_f32(b[d + HALF]);
    }
    float ss = x1 * x1 + x2 * x2;
#pragma unroll
    for (int off = HALF / 2; off > 0; off >>= 1)
      ss += __shfl_xor(ss, off, WAVE);
    if (!live) continue;
    const float r = rsqrtf(ss * (1.0f / D) + eps);
    const bool isq = h < Hq;
    const float n1 = x1 * r * (isq ? wq1 : wk1);
    const float n2 = x2 * r * (isq ? wq2 : wk2);
    const float z1 = n1 * c - n2 * sn;
    const float z2 = n2 * c + n1 * sn;
    const uint16_t y1 = f32_to_bf16(z1);
    const uint16_t y2 = f32_to_bf16(z2);
    if (isq) {
      uint16_t* o = q_out + ((int64_t)t * Hq + h) * D;
      o[d] = y1;
      o[d + HALF] = y2;
    } else {
      const int hk = h - Hq;
      if (k_out != nullptr) {
        uint16_t* o = k_out + ((int64_t)t * Hkv + hk) * D;
        o[d] = y1;
        o[d + HALF] = y2;
      }
      if (slot >= 0) {
        const int64_t ko =
            ((cblock * Hkv + hk) * (int64_t)block_size + coff) * D;
        if (kv8) {           // OCP e4m3 cache: one rounding, from fp32
          uint8_t* o = (uint8_t*)k_cache + ko;
          o[d] = f32_to_fp8(z1);
          o[d + HALF] = f32_to_fp8(z2);
        } else {
          uint16_t* o = k_cache + ko;
          o[d] = y1;
          o[d + HALF] = y2;
        }
      }
    }
  }

  // --- V pass-through (vectorized), as rope_qkv_cache_kernel ---
  const uint16_t* vsrc = src + (Hq + Hkv) * D;
  const int nvec = Hkv * D / 8;
  for (int idx = threadIdx.x; idx < nvec; idx += blockDim.x) {
    const int h = (idx * 8) / D;
    const int dv = (idx * 8) % D;
    const u16x8 val = *reinterpret_cast<const u16x8*>(vsrc + idx * 8);
    if (v_out != nullptr)
      *reinterpret_cast<u16x8*>(v_out + (int64_t)t * Hkv * D + idx * 8) =
          val;
    if (slot >= 0) {
      const int64_t vo =
          ((cblock * Hkv + h) * (int64_t)block_size + coff) * D + dv;
      if (kv8) {
        u8x8 q8;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          q8[e] = f32_to_fp8(bf16_to_f32(val[e]));
        *reinterpret_cast<u8x8*>((uint8_t*)v_cache + vo) = q8;
      } else {
        *reinterpret_cast<u16x8*>(v_cache + vo) = val;
      }
    }
  }
}

}  // namespace

void rope_qkv_norm_cache(torch::Tensor positions, torch::Tensor qkv,
                         torch::Tensor q_out,
                         c10::optional<torch::Tensor> k_cache,
                         c10::optional<torch::Tensor> v_cache,
                         c10::optional<torch::Tensor> slot_mapping,
                         c10::optional<torch::Tensor> k_out,
                         c10::optional<torch::Tensor> v_out,
                         torch::Tensor cos_sin, int64_t num_q_heads,
                         int64_t num_kv_heads, int64_t head_dim,
                         torch::Tensor q_norm_w, torch::Tensor k_norm_w,
                         double eps) {
  // every check runs before the T == 0 return and before any launch
  TORCH_CHECK(head_dim == 64 || head_dim == 128,
              "rope_qkv_norm_cache: head_dim must be 64 or 128, got ",
              head_dim);
  for (const torch::Tensor* w : {&q_norm_w, &k_norm_w}) {
    TORCH_CHECK(w->scalar_type() == torch::kBFloat16,
                "rope_qkv_norm_cache: norm weights must be bf16");
    TORCH_CHECK(w->dim() == 1 && w->size(0) == head_dim,
                "rope_qkv_norm_cache: norm weights must be [head_dim]");
    TORCH_CHECK(w->is_contiguous(),
                "rope_qkv_norm_cache: norm weights must be contiguous");
    TORCH_CHECK(w->device() == qkv.device(),
                "rope_qkv_norm_cache: norm weights must be on qkv's device");
  }
  TORCH_CHECK(eps > 0.0, "rope_qkv_norm_cache: eps must be > 0");
  TORCH_CHECK(num_q_heads > 0 && num_kv_heads > 0);
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 && qkv.dim() == 2);
  TORCH_CHECK(qkv.size(1) == (num_q_heads + 2 * num_kv_heads) * head_dim,
              "rope_qkv_norm_cache: qkv width does not match the heads");
  TORCH_CHECK(positions.scalar_type() == torch::kInt64);
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32);
  TORCH_CHECK(cos_sin.size(-1) == head_dim);
  TORCH_CHECK(qkv.stride(-1) == 1, "qkv innermost must be contiguous");
  const int T = positions.size(0);
  TORCH_CHECK(qkv.size(0) == T);
  TORCH_CHECK(q_out.scalar_type() == torch::kBFloat16 &&
              q_out.is_contiguous() &&
              q_out.numel() == (int64_t)T * num_q_heads * head_dim,
              "rope_qkv_norm_cache: q_out must be contiguous bf16 [T, Hq*D]");
  for (const auto* o : {&k_out, &v_out}) {
    TORCH_CHECK(!o->has_value() ||
                ((*o)->scalar_type() == torch::kBFloat16 &&
                 (*o)->is_contiguous() &&
                 (*o)->numel() == (int64_t)T * num_kv_heads * head_dim),
                "rope_qkv_norm_cache: k_out / v_out must be contiguous bf16 "
                "[T, Hkv*D]");
  }
  int block_size = 1;
  int kv8 = 0;
  uint16_t* kc = nullptr;
  uint16_t* vc = nullptr;
  const int64_t* slots = nullptr;
  if (k_cache.has_value()) {
    kv8 = (k_cache->scalar_type() == torch::kUInt8) ? 1 : 0;
    TORCH_CHECK(v_cache.has_value() && slot_mapping.has_value());
    TORCH_CHECK(slot_mapping->scalar_type() == torch::kInt64);
    TORCH_CHECK(slot_mapping->size(0) == T);
    TORCH_CHECK(kv8 || k_cache->scalar_type() == torch::kBFloat16,
                "rope_qkv_norm_cache: the cache must be bf16 or uint8 (e4m3)");
    TORCH_CHECK(v_cache->scalar_type() == k_cache->scalar_type() &&
                k_cache->dim() == 4 && v_cache->sizes() == k_cache->sizes() &&
                k_cache->is_contiguous() && v_cache->is_contiguous());
    TORCH_CHECK(k_cache->size(1) == num_kv_heads &&
                k_cache->size(3) == head_dim);
    block_size = k_cache->size(2);
    kc = (uint16_t*)k_cache->data_ptr();
    vc = (uint16_t*)v_cache->data_ptr();
    slots = slot_mapping->data_ptr<int64_t>();
  }
  if (T == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(
        kernel, dim3(T), dim3(QKN_THREADS), 0, stream,
        positions.data_ptr<int64_t>(), (const uint16_t*)qkv.data_ptr(),
        qkv.stride(0), (uint16_t*)q_out.data_ptr(), kc, vc, slots,
        k_out.has_value() ? (uint16_t*)k_out->data_ptr() : nullptr,
        v_out.has_value() ? (uint16_t*)v_out->data_ptr() : nullptr,
        cos_sin.data_ptr<float>(), (const uint16_t*)q_norm_w.data_ptr(),
        (const uint16_t*)k_norm_w.data_ptr(), (float)eps, (int)num_q_heads,
        (int)num_kv_heads, block_size, kv8);
  };
  if (head_dim == 128)
    launch(rope_qkv_norm_cache_kernel<128>);
  else
    launch(rope_qkv_norm_cache_kernel<64>);
}
