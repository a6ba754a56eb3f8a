// What the grouped MoE prefill kernels over quantised experts share
// (moe_grouped_kq.hip: Q4_K / Q6_K, moe_grouped_wq.hip: Q4_0 / Q8_0): the
// tile geometry, the tile lookup and the row operand's staging, all of them
// moe_grouped.hip's (which keeps its own copies and is not edited).
//
// Device code of the including file is compiled without packed fp32
// arithmetic, as moe_grouped.hip's: NO_PK_F32_BEGIN / NO_PK_F32_END open and
// close the attribute region, which has to cover the shared headers too, so
// include this header first and wrap later device headers in the macros.
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
#define NO_PK_F32_BEGIN                                                      \
  _Pragma("clang attribute push(__attribute__((target(\"no-packed-fp32-ops\"))), apply_to = function)")
#define NO_PK_F32_END _Pragma("clang attribute pop")
#else
#define NO_PK_F32_BEGIN
#define NO_PK_F32_END
#endif

NO_PK_F32_BEGIN
#include "common.h"
NO_PK_F32_END

namespace helix {

constexpr int GROUPED_WAVES = 4;
constexpr int GROUPED_THREADS = GROUPED_WAVES * WAVE;
constexpr int BN = 128;                  // weight rows per workgroup
constexpr int BK = 64;                   // elements per K step
constexpr int PITCH = BK * 2 + 16;       // padded LDS row, bytes
constexpr int STAGE_ROWS = GROUPED_THREADS / 8;   // x rows one staging pass covers

// Pairs per row tile: moe_grouped.hip's rule, a function of T, k and E only.
inline int grouped_bm(int64_t P, int64_t E) { return P / E < 64 ? 64 : 128; }

NO_PK_F32_BEGIN

__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int lane_read(int v, int src_lane) {
  return __builtin_amdgcn_ds_bpermute(src_lane << 2, v);
}

struct Tile {
  int e;        // expert
  int list0;    // first entry of the expert's list in sorted_pairs[]
  int n;        // list length
  int r0;       // first list entry of this tile
};

// (expert, row tile) of workgroup b, or false past the last tile. A list
// that does not lie inside [0, P] (a corrupt table) counts as empty.
template <int BM>
__device__ __forceinline__ bool find_tile(const int* __restrict__ expert_off,
                                          int E, int P, int b, int lane,
                                          Tile& tl) {
  int base = 0;
  for (int c = 0; c < E; c += WAVE) {
    const int e = c + lane;
    int l0 = 0, n = 0;
    if (e < E) {
      l0 = expert_off[e];
      n = expert_off[e + 1] - l0;
    }
    if (l0 < 0 || n < 0 || l0 > P || n > P - l0) n = 0;
    const int tiles = (n + BM - 1) / BM;
    int incl = tiles;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int o = lane_read(incl, (lane - d) & (WAVE - 1));
      if (lane >= d) incl += o;
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(base + incl > b);
    if (m != 0) {                                  // wave-uniform
      const int f = __builtin_ctzll(m);
      tl.e = c + f;
      tl.list0 = lane_read(l0, f);
      tl.n = lane_read(n, f);
      tl.r0 = (b - base - lane_read(incl - tiles, f)) * BM;
      return true;
    }
    base += lane_read(incl, WAVE - 1);
  }
  return false;
}

// Row operand: one staging pass per 32 rows, NV 16-byte vectors per thread,
// zero where the row does not exist.
template <int NV>
__device__ __forceinline__ void tile_fetch(u32x4 (&v)[NV],
                                           const uint16_t* __restrict__ base,
                                           const int64_t (&row_off)[NV],
                                           int kv) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (row_off[i] >= 0)
      v[i] = *reinterpret_cast<const u32x4*>(base + row_off[i] + kv);
    else
      v[i] = u32x4{0, 0, 0, 0};
  }
}

template <int NV>
__device__ __forceinline__ void tile_stage(uint8_t* buf, const u32x4 (&v)[NV],
                                           int r, int c) {
#pragma unroll
  for (int i = 0; i < NV; ++i)
    *reinterpret_cast<u32x4*>(buf + (STAGE_ROWS * i + r) * PITCH + 16 * c) =
        v[i];
}

NO_PK_F32_END

}  // namespace helix
