// Mixture-of-experts routed expert GEMMs for prefill: grouped, LDS-tiled
// MFMA kernels over the lists moe_align builds (gfx950). moe.hip is built
// for decode (16-channel workgroups, operands straight to registers, K split
// over waves): from T = 64 it re-reads gathered rows per 16 channels and
// from lists of 65 pairs it streams the weight tile again per chunk. Here a
// workgroup owns BM pairs of ONE expert's list times 128 weight rows, both
// operands go through LDS, and weights and rows are each read once per tile.
//
//   act[p, n]   = bf16(silu(x[p/k] . w13[e, n]) * (x[p/k] . w13[e, I+n]))
//   ypair[p, n] = topk_w[p] * (act[p] . w2[e, n])                   (fp32)
//
// Operands, intermediates and rounding points are moe.hip's; moe_route,
// moe_align and moe_combine are shared with it.
//
// Tile lookup (find_tile, lora_sgmv.hip's scheme): grid.x is the host-side
//   bound ceil(P / BM) + E on sum_e ceil(n_e / BM). Every wave of workgroup
//   b scans expert_off 64 experts at a time: a lane's expert has
//   ceil(n_e / BM) row tiles, an inclusive wave scan plus the running base
//   orders them, ballot(base + incl > b) and its first set bit name the
//   expert. A workgroup past the last tile returns (workgroup-uniform). A
//   list that does not lie inside [0, P] counts as empty. No device value
//   reaches the host: no sync, no host-sized shape, no memset.
//
// moe_grouped_kernel<GATED, BM>, 4 waves, grid (row tiles, channel tiles):
//   * Channel tile = 128 weight rows. !GATED: channels [n0, n0 + 128) of
//     w2[e]. GATED: gate rows [n0, n0 + 64) in LDS rows 0-63 and up rows
//     [I + n0, I + n0 + 64) in LDS rows 64-127; they share the staged x rows.
//   * Waves form a 2 x 2 layout (wr, wc): BM/2 pairs x half of the channels,
//     4 channel tiles x BM/32 row tiles of mfma_f32_16x16x32_bf16 (BM = 128:
//     64 accumulator registers). A GATED wave holds gate tiles 2wc, 2wc+1 and
//     the up tiles of the SAME channels, so the epilogue needs no exchange.
//     16-channel tiles at or past N and 16-row tiles at or past the list's
//     end are skipped wave-uniformly; the wave still stages and meets every
//     barrier.
//   * K step BK = 64, double buffered, one barrier per step: the global
//     loads of step s+1 (b128, through registers) are issued before the
//     MFMAs of step s and written to the other buffer after them. Thread
//     (r = tid / 8, c = tid % 8) stages bytes [16c, 16c + 16) of rows r,
//     r + 32, ...: eight lanes cover the 128 contiguous bytes of one row.
//     The row operand is gathered: the tile's pair ids are read once, before
//     the K loop, into LDS (epilogue) and registers (source-row offsets).
//     Weight rows at or past N, rows at or past the list's end and vectors
//     at or past K are zero-filled in both operands, never loaded:
//     0 * garbage may be NaN.
//   * LDS rows are padded from 128 to 144 bytes, so that the 16 rows of an
//     MFMA operand start 4 banks apart instead of on one bank; a fragment is
//     one ds_read_b128 of row lo at bytes 64*ks + 16*hi (k = 32*ks + 8*hi +
//     i, the natural order, the same for both operands). 2 x (128 + BM) x
//     144 bytes + the pair ids: 72.5 KiB at BM = 128, two workgroups per CU.
//   * Weights are the MFMA row (A) operand: a lane holds D[channel = hi*4 +
//     r][pair = lo], four consecutive channels of one pair, so act is stored
//     as one 8-byte and ypair as one 16-byte vector per tile, scattered by
//     pair id.
//   * No split-K, no atomics, nothing accumulated across workgroups: every
//     output element is one accumulator taking the K steps in ascending
//     order. A pair's bits depend on its row and its expert's weights only,
//     not on T, BM, its place in the list, its neighbours or the grid.
//   * grid.x (row tiles) runs fastest: the row tiles of one (expert, channel
//     tile) are neighbours in launch order and re-read the weight tile from
//     L2.

// Device code of this file is compiled without packed fp32 arithmetic
// (scalar fp32 ops only); the attribute region has to cover common.h, and
// the kernels read ids and exchange lanes through builtins, so that no
// callee with other target features stays out of line.
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
#include "moe_common.h"
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

constexpr int GROUPED_WAVES = 4;
constexpr int GROUPED_THREADS = GROUPED_WAVES * WAVE;
constexpr int BN = 128;                  // weight rows per workgroup
constexpr int BK = 64;                   // elements per K step
constexpr int PITCH = BK * 2 + 16;       // padded LDS row, bytes
constexpr int STAGE_ROWS = GROUPED_THREADS / 8;   // rows one staging pass covers

// Pairs per row tile: a function of T, k and E only. 64 while the mean list
// is shorter than 64 pairs, so that a short list does not pay for 128 rows.
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

// One staging pass per 32 rows: NV 16-byte vectors per thread, zero where
// the row or the K position does not exist.
template <int NV>
__device__ __forceinline__ void tile_fetch(u32x4 (&v)[NV],
                                           const uint16_t* __restrict__ base,
                                           const int64_t (&row_off)[NV],
                                           int kv, int K) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (row_off[i] >= 0 && kv < K)
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

template <bool GATED, int BM>
__global__ __launch_bounds__(GROUPED_THREADS) void moe_grouped_kernel(
    void* __restrict__ dst,                  // GATED: bf16 act[P, N]; else fp32 ypair[P, N]
    const uint16_t* __restrict__ src,        // GATED: x[T, K]; else act[P, K]
    const uint16_t* __restrict__ wgt,        // [E, GATED ? 2N : N, K]
    const float* __restrict__ topk_w,        // [P] (!GATED)
    const int32_t* __restrict__ expert_off,  // [E + 1]
    const int32_t* __restrict__ sorted_pairs,  // [P]
    int P, int N, int K, int E, int k) {
  constexpr int RT = BM / 32;                // 16-row tiles per wave
  constexpr int CT = 4;                      // 16-channel tiles per wave
  constexpr int WV = BN / STAGE_ROWS;        // staged weight vectors per thread
  constexpr int XV = BM / STAGE_ROWS;        // staged row vectors per thread
  constexpr int W_BYTES = BN * PITCH, X_BYTES = BM * PITCH;
  constexpr int BUF_BYTES = W_BYTES + X_BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * BUF_BYTES];
  __shared__ int pid[BM];

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  Tile tl;
  if (!find_tile<BM>(expert_off, E, P, __builtin_amdgcn_workgroup_id_x(), lane,
                     tl))
    return;                                  // workgroup-uniform

  // the tile's pair ids, once
  if (tid < BM) {
    const int i = tl.r0 + tid;
    int p = i < tl.n ? sorted_pairs[tl.list0 + i] : -1;
    if (p >= P) p = -1;
    pid[tid] = p;
  }
  block_barrier();

  const int sr = tid >> 3, sc = tid & 7;     // staging row and 16-byte column
  const int n0 = __builtin_amdgcn_workgroup_id_y() * (GATED ? BN / 2 : BN);
  int64_t w_off[WV], x_off[XV];              // element offsets, -1: zero-fill
#pragma unroll
  for (int i = 0; i < WV; ++i) {
    const int lr = STAGE_ROWS * i + sr;      // LDS weight row
    const int ch = GATED ? n0 + (lr & 63) : n0 + lr;
    const int row = GATED ? (lr >> 6) * N + ch : ch;
    w_off[i] = ch < N
        ? ((int64_t)tl.e * (GATED ? 2 * N : N) + row) * K : -1;
  }
#pragma unroll
  for (int i = 0; i < XV; ++i) {
    const int p = pid[STAGE_ROWS * i + sr];
    x_off[i] = p < 0 ? -1 : (int64_t)(GATED ? p / k : p) * K;
  }

  // wave-uniform tile skips
  bool ct_on[CT], rt_on[RT];
  int ct_row[CT];                            // LDS weight row of channel tile ct
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    ct_row[c] = GATED ? (c >> 1) * 64 + wc * 32 + (c & 1) * 16
                      : wc * 64 + c * 16;
    ct_on[c] = n0 + (GATED ? ct_row[c] & 63 : ct_row[c]) < N;
  }
#pragma unroll
  for (int t = 0; t < RT; ++t)
    rt_on[t] = tl.r0 + wr * (BM / 2) + t * 16 < tl.n;

  floatx4 acc[CT][RT];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[c][t] = floatx4{0, 0, 0, 0};

  const int steps = (K + BK - 1) / BK;
  u32x4 wv[WV], xv[XV];
  tile_fetch<WV>(wv, wgt, w_off, sc * 8, K);
  tile_fetch<XV>(xv, src, x_off, sc * 8, K);
  tile_stage<WV>(lds, wv, sr, sc);
  tile_stage<XV>(lds + W_BYTES, xv, sr, sc);
  block_barrier();

  for (int s = 0; s < steps; ++s) {
    const uint8_t* wb = lds + (s & 1) * BUF_BYTES;
    const uint8_t* xb = wb + W_BYTES;
    const bool more = s + 1 < steps;         // workgroup-uniform
    if (more) {
      tile_fetch<WV>(wv, wgt, w_off, (s + 1) * BK + sc * 8, K);
      tile_fetch<XV>(xv, src, x_off, (s + 1) * BK + sc * 8, K);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int col = 64 * ks + 16 * hi;
      bf16x8 a[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c)
        a[c] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
            wb + (ct_row[c] + lo) * PITCH + col));
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        if (!rt_on[t]) continue;
        const bf16x8 b = __builtin_bit_cast(bf16x8,
            *reinterpret_cast<const u32x4*>(
                xb + (wr * (BM / 2) + t * 16 + lo) * PITCH + col));
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (ct_on[c])
            acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[c], b, acc[c][t], 0, 0, 0);
      }
    }
    if (more) {
      uint8_t* nb = lds + ((s + 1) & 1) * BUF_BYTES;
      tile_stage<WV>(nb, wv, sr, sc);
      tile_stage<XV>(nb + W_BYTES, xv, sr, sc);
    }
    block_barrier();
  }

  // C/D: lane holds D[channel = hi*4 + r][pair = lo] of tile (c, t)
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    if (!rt_on[t]) continue;
    const int p = pid[wr * (BM / 2) + t * 16 + lo];
    if (p < 0) continue;
    if constexpr (GATED) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (!ct_on[c]) continue;
        u16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float g = acc[c][t][r];
          const float e = __builtin_amdgcn_exp2f(g * -1.44269504088896f);
          o[r] = f32_to_bf16(g / (1.f + e) * acc[c + 2][t][r]);
        }
        *reinterpret_cast<u16x4*>(
            static_cast<uint16_t*>(dst) + (int64_t)p * N + n0 + ct_row[c] +
            hi * 4) = o;
      }
    } else {
      const float sw = topk_w[p];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (!ct_on[c]) continue;
        floatx4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = sw * acc[c][t][r];
        *reinterpret_cast<floatx4*>(
            static_cast<float*>(dst) + (int64_t)p * N + n0 + ct_row[c] +
            hi * 4) = o;
      }
    }
  }
}

NO_PK_F32_END

template <bool GATED>
void launch_grouped(void* dst, const torch::Tensor& src,
                    const torch::Tensor& wgt, const float* tw,
                    const torch::Tensor& expert_off,
                    const torch::Tensor& sorted_pairs, int64_t P, int N, int K,
                    int E, int k) {
  const int bm = grouped_bm(P, E);
  const dim3 grid((unsigned)((P + bm - 1) / bm + E),
                  (unsigned)cdiv(N, GATED ? BN / 2 : BN));
  auto stream = at::hip::getCurrentHIPStream();
#define GROUPED_LAUNCH(BM_)                                                   \
  hipLaunchKernelGGL((moe_grouped_kernel<GATED, BM_>), grid,                  \
                     dim3(GROUPED_THREADS), 0, stream, dst,                   \
                     (const uint16_t*)src.data_ptr(),                         \
                     (const uint16_t*)wgt.data_ptr(), tw,                     \
                     (const int32_t*)expert_off.data_ptr(),                   \
                     (const int32_t*)sorted_pairs.data_ptr(), (int)P, N, K,   \
                     E, k)
  if (bm == 64) GROUPED_LAUNCH(64); else GROUPED_LAUNCH(128);
#undef GROUPED_LAUNCH
}

}  // namespace

// act[P, I] = silu(x[p/k] @ w13[e, :I]^T) * (x[p/k] @ w13[e, I:]^T)
void moe_grouped_gated(torch::Tensor act, torch::Tensor x, torch::Tensor w13,
                       torch::Tensor expert_off, torch::Tensor sorted_pairs,
                       int64_t k) {
  TORCH_CHECK(w13.is_cuda(), "moe_grouped_gated: w13 must be on GPU");
  TORCH_CHECK(w13.dim() == 3 && x.dim() == 2 && act.dim() == 2,
              "moe_grouped_gated: w13 must be 3-D, x and act 2-D");
  const int64_t E = w13.size(0), I = w13.size(1) / 2, H = w13.size(2);
  const int64_t T = x.size(0), P = T * k;
  check_ek(E, k);
  check_tensor(w13, w13, torch::kBFloat16, "moe_grouped_gated: w13");
  check_tensor(x, w13, torch::kBFloat16, "moe_grouped_gated: x");
  check_tensor(act, w13, torch::kBFloat16, "moe_grouped_gated: act");
  TORCH_CHECK(H > 0 && H % 32 == 0, "moe_grouped_gated: H (", H,
              ") must be a positive multiple of 32");
  TORCH_CHECK(I > 0 && I % 32 == 0 && w13.size(1) == 2 * I,
              "moe_grouped_gated: w13 must be [E, 2I, H] with I a positive "
              "multiple of 32");
  TORCH_CHECK(x.size(1) == H, "moe_grouped_gated: x must be [T, H], H = ", H);
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_grouped_gated: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && 2 * I * H < (int64_t(1) << 31) &&
              I / 64 < 65535,
              "moe_grouped_gated: problem too large");
  check_lists(expert_off, sorted_pairs, w13, E, P);
  if (T == 0) return;
  launch_grouped<true>(act.data_ptr(), x, w13, nullptr, expert_off,
                       sorted_pairs, P, (int)I, (int)H, (int)E, (int)k);
}

// ypair[P, H] (fp32) = topk_w[p] * (act[p] @ w2[e]^T)
void moe_grouped_down(torch::Tensor ypair, torch::Tensor act, torch::Tensor w2,
                      torch::Tensor topk_w, torch::Tensor expert_off,
                      torch::Tensor sorted_pairs) {
  TORCH_CHECK(w2.is_cuda(), "moe_grouped_down: w2 must be on GPU");
  TORCH_CHECK(w2.dim() == 3 && act.dim() == 2 && ypair.dim() == 2 &&
              topk_w.dim() == 2,
              "moe_grouped_down: w2 must be 3-D, act, ypair and topk_w 2-D");
  const int64_t E = w2.size(0), H = w2.size(1), I = w2.size(2);
  const int64_t T = topk_w.size(0), k = topk_w.size(1), P = T * k;
  check_ek(E, k);
  check_tensor(w2, w2, torch::kBFloat16, "moe_grouped_down: w2");
  check_tensor(act, w2, torch::kBFloat16, "moe_grouped_down: act");
  check_tensor(ypair, w2, torch::kFloat32, "moe_grouped_down: ypair");
  check_tensor(topk_w, w2, torch::kFloat32, "moe_grouped_down: topk_w");
  TORCH_CHECK(H > 0 && H % 32 == 0, "moe_grouped_down: H (", H,
              ") must be a positive multiple of 32");
  TORCH_CHECK(I > 0 && I % 32 == 0, "moe_grouped_down: I (", I,
              ") must be a positive multiple of 32");
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_grouped_down: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(ypair.size(0) == P && ypair.size(1) == H,
              "moe_grouped_down: ypair must be [T*k, H] = [", P, ", ", H, "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && I * H < (int64_t(1) << 31) &&
              H / 128 < 65535,
              "moe_grouped_down: problem too large");
  check_lists(expert_off, sorted_pairs, w2, E, P);
  if (T == 0) return;
  launch_grouped<false>(ypair.data_ptr(), act, w2,
                        (const float*)topk_w.data_ptr(), expert_off,
                        sorted_pairs, P, (int)H, (int)I, (int)E, (int)k);
}
