// Register-level dequantization helpers shared by the weight-only GEMMs
// (gemm_wq.hip and moe_wq.hip: ggml Q4_0/Q8_0; gemm_kq.hip and moe_kq.hip:
// ggml Q4_K/Q6_K, through kq_common.h).
#pragma once

#include "common.h"

namespace helix {

__device__ __forceinline__ float half_bits_to_f32(uint16_t h) {
  union { uint16_t u; _Float16 f; } v;
  v.u = h;
  return (float)v.f;
}

// Two fp32 -> packed bf16, round to nearest even: one v_cvt_pk_bf16_f32.
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// 8 unsigned bytes (two dwords) -> 8 bf16 of fma(byte, d, off).
__device__ __forceinline__ bf16x8 dq8(uint32_t a, uint32_t b, float d,
                                      float off) {
  u32x4 r;
  r[0] = pack_bf16x2(fmaf((float)(a & 0xffu), d, off),
                     fmaf((float)((a >> 8) & 0xffu), d, off));
  r[1] = pack_bf16x2(fmaf((float)((a >> 16) & 0xffu), d, off),
                     fmaf((float)(a >> 24), d, off));
  r[2] = pack_bf16x2(fmaf((float)(b & 0xffu), d, off),
                     fmaf((float)((b >> 8) & 0xffu), d, off));
  r[3] = pack_bf16x2(fmaf((float)((b >> 16) & 0xffu), d, off),
                     fmaf((float)(b >> 24), d, off));
  return __builtin_bit_cast(bf16x8, r);
}

// -- ggml Q4_0 / Q8_0 blocks as two planes (gemm_wq.hip, moe_wq.hip) --------
template <int BITS>
struct WQRaw {
  u32x4 q[BITS == 4 ? 1 : 2];
  float d;
};

// The lane's block: payload bytes + scale of block kb of row n, where n
// counts rows from the start of the planes (for a stack of experts it
// already includes expert * rows). An invalid lane gets d = 0 and zero
// payload, which dequantizes to +0 everywhere.
template <int BITS>
__device__ __forceinline__ WQRaw<BITS> wq_load(const uint8_t* __restrict__ qs,
                                               const uint16_t* __restrict__ ds,
                                               int64_t n, int kb, int nblk,
                                               bool valid) {
  WQRaw<BITS> r;
  constexpr int BB = BITS == 4 ? 16 : 32;        // payload bytes per block
  constexpr int NV = BITS == 4 ? 1 : 2;
  if (valid) {
    const u32x4* p = reinterpret_cast<const u32x4*>(
        qs + (n * nblk + kb) * BB);
#pragma unroll
    for (int i = 0; i < NV; ++i) r.q[i] = p[i];
    r.d = half_bits_to_f32(ds[n * nblk + kb]);
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) r.q[i] = u32x4{0, 0, 0, 0};
    r.d = 0.f;
  }
  return r;
}

// Fragment j (elements 8j..8j+7 of the block), j a compile-time constant.
template <int BITS, int J>
__device__ __forceinline__ bf16x8 wq_frag(const WQRaw<BITS>& r) {
  if constexpr (BITS == 4) {
    // element e < 16: low nibble of byte e; e >= 16: high nibble of e-16
    constexpr int DW = (J & 1) * 2;
    constexpr int SH = (J >> 1) * 4;
    uint32_t a = (r.q[0][DW] >> SH) & 0x0f0f0f0fu;
    uint32_t b = (r.q[0][DW + 1] >> SH) & 0x0f0f0f0fu;
    return dq8(a, b, r.d, -8.f * r.d);
  } else {
    constexpr int V = J >> 1;
    constexpr int DW = (J & 1) * 2;
    uint32_t a = r.q[V][DW] ^ 0x80808080u;       // int8 -> biased uint8
    uint32_t b = r.q[V][DW + 1] ^ 0x80808080u;
    return dq8(a, b, r.d, -128.f * r.d);
  }
}

}  // namespace helix
