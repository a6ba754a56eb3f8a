// Per-lane fetch, decode and MFMA fragments of ggml Q4_K / Q6_K super-blocks,
// shared by gemm_kq.hip (one weight) and moe_kq.hip (a stack of experts).
// gemm_kq.hip's header has the layout, the lane mapping and the rounding
// argument; `blk` counts super-blocks from the start of the planes, so for a
// stack of experts it already includes expert * rows * K/256.
#pragma once

#include "dequant_common.h"

namespace helix {

constexpr int KQ_SB = 256;                      // elements per super-block

template <int FMT>
struct KQRaw;

// Q4_K lane state: 32 payload bytes and the two sub-blocks' d*sc, -(dmin*m).
template <>
struct KQRaw<4> {
  u32x4 q[2];
  float s[2], o[2];
};

// Q6_K lane state: 32 ql bytes, 32 qh bytes pre-shifted so that group G's
// two bits sit at bit 4G of every byte, and d*sc, -32*d*sc of the four
// 16-element runs (group G, run r at index 2G + r).
template <>
struct KQRaw<6> {
  u32x4 ql[2], qh[2];
  float s[4], o[4];
};

// Decode sub-block j's (sc, m) from the header dwords h1..h3 = scales[0..12).
// jj = j & 3; hi_half = j >= 4.
__device__ __forceinline__ void q4k_scale_min(uint32_t h1, uint32_t h2,
                                              uint32_t h3, int jj,
                                              bool hi_half, float d,
                                              float dmin, float* s,
                                              float* o) {
  const int sh = 8 * jj;
  const uint32_t a1 = (h1 >> sh) & 0xffu;       // scales[jj]
  const uint32_t a2 = (h2 >> sh) & 0xffu;       // scales[jj + 4]
  const uint32_t a3 = (h3 >> sh) & 0xffu;       // scales[jj + 8]
  const uint32_t sc = hi_half ? ((a3 & 0xfu) | ((a1 >> 6) << 4)) : (a1 & 63u);
  const uint32_t m = hi_half ? ((a3 >> 4) | ((a2 >> 6) << 4)) : (a2 & 63u);
  *s = d * (float)sc;
  *o = -(dmin * (float)m);
}

// The lane's bytes of one super-block as loaded, before any arithmetic: the
// K loop fetches the next step's while it computes the current one.
template <int FMT>
struct KQFetch;

template <>
struct KQFetch<4> {
  u32x4 q[2], h;
};

template <>
struct KQFetch<6> {
  u32x4 ql[2], qh[2];
  u32x2 sv;
  uint16_t d;
};

__device__ __forceinline__ KQFetch<4> kq_fetch4(const uint8_t* __restrict__ qs,
                                                const uint8_t* __restrict__ hdr,
                                                int64_t blk, int hi) {
  KQFetch<4> f;
  const u32x4* p = reinterpret_cast<const u32x4*>(qs + blk * 128 + 32 * hi);
  f.q[0] = p[0];
  f.q[1] = p[1];
  f.h = *reinterpret_cast<const u32x4*>(hdr + blk * 16);
  return f;
}

__device__ __forceinline__ KQRaw<4> kq_decode(const KQFetch<4>& f, int hi) {
  KQRaw<4> r;
  r.q[0] = f.q[0];
  r.q[1] = f.q[1];
  const float d = half_bits_to_f32((uint16_t)(f.h[0] & 0xffffu));
  const float dmin = half_bits_to_f32((uint16_t)(f.h[0] >> 16));
  const int jj = 2 * (hi & 1);
  q4k_scale_min(f.h[1], f.h[2], f.h[3], jj, hi >= 2, d, dmin, &r.s[0],
                &r.o[0]);
  q4k_scale_min(f.h[1], f.h[2], f.h[3], jj + 1, hi >= 2, d, dmin, &r.s[1],
                &r.o[1]);
  return r;
}

__device__ __forceinline__ KQFetch<6> kq_fetch6(const uint8_t* __restrict__ ql,
                                                const uint8_t* __restrict__ qh,
                                                const int8_t* __restrict__ sc,
                                                const uint16_t* __restrict__ ds,
                                                int64_t blk, int hi) {
  KQFetch<6> f;
  const int h = hi >> 1, p = hi & 1;
  const u32x4* pl = reinterpret_cast<const u32x4*>(
      ql + blk * 128 + 64 * h + 32 * p);
  f.ql[0] = pl[0];
  f.ql[1] = pl[1];
  const u32x4* ph = reinterpret_cast<const u32x4*>(qh + blk * 64 + 32 * h);
  f.qh[0] = ph[0];
  f.qh[1] = ph[1];
  // scales[8h + 2g + r]: g = p in dword 0, g = p+2 in dword 1, bytes 2p+r
  f.sv = *reinterpret_cast<const u32x2*>(sc + blk * 16 + 8 * h);
  f.d = ds[blk];
  return f;
}

__device__ __forceinline__ KQRaw<6> kq_decode(const KQFetch<6>& f, int hi) {
  KQRaw<6> r;
  const int p = hi & 1;
  r.ql[0] = f.ql[0];
  r.ql[1] = f.ql[1];
  // group p's bits to bit 0 of each byte; group p+2's are then at bit 4
  r.qh[0] = f.qh[0] >> (uint32_t)(2 * p);
  r.qh[1] = f.qh[1] >> (uint32_t)(2 * p);
  const float d = half_bits_to_f32(f.d);
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int v = (int)(int8_t)((f.sv[g] >> (16 * p + 8 * k)) & 0xffu);
      const float s = d * (float)v;
      r.s[2 * g + k] = s;
      r.o[2 * g + k] = -32.f * s;
    }
  return r;
}

template <int FMT>
__device__ __forceinline__ KQFetch<FMT> kq_fetch(const void* p0,
                                                 const void* p1,
                                                 const void* p2,
                                                 const void* p3, int64_t blk,
                                                 int hi) {
  if constexpr (FMT == 4)
    return kq_fetch4((const uint8_t*)p0, (const uint8_t*)p1, blk, hi);
  else
    return kq_fetch6((const uint8_t*)p0, (const uint8_t*)p1,
                     (const int8_t*)p2, (const uint16_t*)p3, blk, hi);
}

// Fragment J of the lane's 64 elements (MFMA J of the step), J constant.
template <int J>
__device__ __forceinline__ bf16x8 kq_frag(const KQRaw<4>& r) {
  constexpr int V = (J & 3) >> 1, DW = (J & 1) * 2, G = J >> 2;
  const uint32_t a = (r.q[V][DW] >> (4 * G)) & 0x0f0f0f0fu;
  const uint32_t b = (r.q[V][DW + 1] >> (4 * G)) & 0x0f0f0f0fu;
  return dq8(a, b, r.s[G], r.o[G]);
}

template <int J>
__device__ __forceinline__ bf16x8 kq_frag(const KQRaw<6>& r) {
  constexpr int V = (J & 3) >> 1, DW = (J & 1) * 2, G = J >> 2;
  constexpr int S = 2 * G + ((J & 3) >> 1);     // run of 16 within the group
  const uint32_t a = ((r.ql[V][DW] >> (4 * G)) & 0x0f0f0f0fu) |
                     (((r.qh[V][DW] >> (4 * G)) & 0x03030303u) << 4);
  const uint32_t b = ((r.ql[V][DW + 1] >> (4 * G)) & 0x0f0f0f0fu) |
                     (((r.qh[V][DW + 1] >> (4 * G)) & 0x03030303u) << 4);
  return dq8(a, b, r.s[S], r.o[S]);
}

}  // namespace helix
