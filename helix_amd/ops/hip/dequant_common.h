// Register-level dequantization helpers shared by the weight-only GEMMs
// (gemm_wq.hip: ggml Q4_0/Q8_0, gemm_kq.hip: ggml Q4_K/Q6_K).
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

}  // namespace helix
