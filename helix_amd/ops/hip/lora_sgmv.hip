// Multi-LoRA for prefill and large batches: segment-tiled MFMA shrink and
// expand (gfx950). lora.hip runs one workgroup per token and re-reads the
// adapter for every token; here the rows are grouped by slot first
// (moe_align with k = 1: seg_off[S+1], rows[T]) and a workgroup owns ROWS =
// 16*MT rows of ONE slot, so A / B are read once per ROWS rows and both
// halves run on mfma_f32_16x16x32_bf16.
//
//   y[t, j]   = sum_k x[t,k] * A[s, j, k]                           (fp32)
//   out[t, n] = bf16(out[t,n] + scale[s] * sum_j y[t, i(n)*R + j] * B[s,n,j])
//
// Tile lookup (find_tile): the grid's x dimension is the host-side bound
//   ceil(T / ROWS) + S on sum_s ceil(n_s / ROWS). Every wave of workgroup b
//   scans seg_off 64 slots at a time: a lane's slot has ceil(n_s / ROWS)
//   tiles, an inclusive wave scan plus the running base orders the tiles,
//   ballot(base + incl > b) and its first set bit name the slot. A
//   workgroup past the last tile returns (workgroup-uniform: all waves
//   compute the same answer). No LDS, no barrier.
//
// lora_sgmv_shrink_kernel<RT, MT>: the tile's ROWS gathered rows against all
//   Rtot channels (RT = ceil(Rtot / 16) rank tiles). A[s] is the MFMA row
//   operand: lane (lo, hi) loads the 64 contiguous bytes of rank row lo, K
//   block 4*step + hi, and feeds four MFMAs with values [8j, 8j+8); the
//   token operand is the same 64-byte run of gathered row lo (moe_gemm's
//   mapping). x goes from global memory to registers, once per launch. The
//   W waves take the 128-element K steps w, w+W, ... and are summed through
//   LDS in the fixed order ((w0 + w1) + w2) + ...; W depends on (Rtot, K)
//   only, MT on T only. Rank rows at or past Rtot (Rtot = 8, 24) load zeros,
//   row tiles past the list's end are skipped wave-uniformly.
//
// lora_sgmv_expand_kernel<R, MT>: grid y walks 256-column blocks, wave w owns
//   the four 16-column tiles [64w, 64w + 64) of the block. B[s] is the row
//   operand: lane (lo, hi) loads B[s, n0 + lo, 16m + 8*(hi&1) .. +8) with one
//   b128 load per MFMA m and keeps it for all MT row tiles. y stays fp32-
//   accurate without an fp32 MFMA: y = yh + yl with yh = bf16(y), yl =
//   bf16(y - yh); k-slots 0-15 of the MFMA carry yh (lanes hi = 0, 1), 16-31
//   carry yl (hi = 2, 3), both against the same B values, so one MFMA does
//   16 ranks (R = 8: half the slots are zero; R = 32 / 64: 2 / 4 MFMAs).
//   Write-back: the MFMA leaves 4 channels x 16 rows per lane group, so a
//   wave parks its 16 x 64 fp32 tile in its own LDS strip (pitch 68 floats)
//   and reads it back with lane -> (row = lane / 8, 8 columns = lane % 8):
//   eight lanes cover 128 contiguous bytes of an out row, each with one b128
//   load, scale[s] * delta added in fp32, one rounding, one b128 store. The
//   strip is private to the wave, so the exchange needs no workgroup barrier
//   (waves of a workgroup may own different numbers of column tiles).
//
// No atomics, nothing accumulated across workgroups; a row's bits depend on
// (Rtot, K) through W and on nothing else: MT, the tile and its neighbours
// only regroup MFMA columns. Rows in no list are never touched.

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
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

constexpr int SGMV_MAX_S = 256;
constexpr int SGMV_MAX_MT = 2;
constexpr int SGMV_MAX_W = 8;
constexpr int EXPAND_WAVES = 4;
constexpr int EXPAND_COLS = EXPAND_WAVES * 64;     // columns per workgroup
constexpr int STAGE_PITCH = 68;                    // floats per staged row
constexpr int MAX_SLICES = 3;

struct SliceOffsets {
  int off[MAX_SLICES + 1];      // unused tail entries hold N
};

// Row tiles per workgroup: a function of T only.
inline int sgmv_mt(int64_t T) { return T <= 64 ? 1 : 2; }

// K-split factor of the shrink: a function of (Rtot, K) only. Every wave
// gets at least two 128-element steps, and the reduction buffer
// (W-1) x RT x MT KiB stays under 64 KiB for MT = SGMV_MAX_MT.
inline int sgmv_waves(int64_t Rtot, int64_t K) {
  const int rt = (int)((Rtot + 15) / 16);
  const int cap = rt <= 4 ? 8 : rt <= 8 ? 4 : 2;
  const int64_t steps = (K + 127) / 128;
  int w = 1;
  while (w < cap && steps >= 4 * w) w *= 2;
  return w;
}

NO_PK_F32_BEGIN

__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// Orders a wave's own LDS writes before its later LDS reads (and back):
// the lanes of a wave run in lockstep and its DS operations stay in order.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int lane_read(int v, int src_lane) {
  return __builtin_amdgcn_ds_bpermute(src_lane << 2, v);
}

struct Tile {
  int s;        // slot
  int list0;    // first entry of the slot's list in rows[]
  int n;        // list length
  int r0;       // first list entry of this tile
};

// (slot, tile) of workgroup b, or false past the last tile. A list that
// does not lie inside [0, T) (a corrupt table) counts as empty.
template <int ROWS>
__device__ __forceinline__ bool find_tile(const int* __restrict__ seg_off,
                                          int S, int T, int b, int lane,
                                          Tile& tl) {
  int base = 0;
  for (int c = 0; c < S; c += WAVE) {
    const int s = c + lane;
    int l0 = 0, n = 0;
    if (s < S) {
      l0 = seg_off[s];
      n = seg_off[s + 1] - l0;
    }
    if (l0 < 0 || n < 0 || l0 > T || n > T - l0) n = 0;
    const int tiles = (n + ROWS - 1) / ROWS;
    int incl = tiles;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int o = lane_read(incl, (lane - d) & (WAVE - 1));
      if (lane >= d) incl += o;
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(base + incl > b);
    if (m != 0) {                                  // wave-uniform
      const int f = __builtin_ctzll(m);
      tl.s = c + f;
      tl.list0 = lane_read(l0, f);
      tl.n = lane_read(n, f);
      tl.r0 = (b - base - lane_read(incl - tiles, f)) * ROWS;
      return true;
    }
    base += lane_read(incl, WAVE - 1);
  }
  return false;
}

// grid (ceil(T / ROWS) + S), block W * 64, dynamic LDS (W-1)*RT*MT KiB.
template <int RT, int MT>
__global__ __launch_bounds__(SGMV_MAX_W * WAVE) void lora_sgmv_shrink_kernel(
    float* __restrict__ y,                   // [T, Rtot]
    const uint16_t* __restrict__ x,          // [T, K]
    const uint16_t* __restrict__ A,          // [S, Rtot, K]
    const int* __restrict__ seg_off,         // [S + 1]
    const int* __restrict__ rows,            // [T]
    int T, int K, int Rtot, int S, int W) {
  extern __shared__ floatx4 red[];           // [W - 1][RT * MT][WAVE]
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  Tile tl;
  if (!find_tile<16 * MT>(seg_off, S, T, __builtin_amdgcn_workgroup_id_x(),
                          lane, tl))
    return;                                  // workgroup-uniform

  int rid[MT];
  const uint16_t* xrow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int i = tl.r0 + t * 16 + lo;
    int p = i < tl.n ? rows[tl.list0 + i] : -1;
    if (p >= T) p = -1;
    rid[t] = p;
    xrow[t] = x + (int64_t)(p < 0 ? 0 : p) * K;
  }
  const uint16_t* arow[RT];
  bool avalid[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    avalid[r] = r * 16 + lo < Rtot;
    arow[r] = A + ((int64_t)tl.s * Rtot + (avalid[r] ? r * 16 + lo : 0)) * K;
  }

  floatx4 acc[RT][MT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[r][t] = floatx4{0, 0, 0, 0};

  const int nblk = K / 32;
  for (int kb0 = wave * 4; kb0 < nblk; kb0 += 4 * W) {
    const int kb = kb0 + hi;
    const bool kvalid = kb < nblk;
    u32x4 xf[MT][4];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (kvalid && rid[t] >= 0) {
        const u32x4* q = reinterpret_cast<const u32x4*>(xrow[t] + kb * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[t][j] = q[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[t][j] = u32x4{0, 0, 0, 0};
      }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      u32x4 af[4];
      if (kvalid && avalid[r]) {
        const u32x4* q = reinterpret_cast<const u32x4*>(arow[r] + kb * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = q[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = u32x4{0, 0, 0, 0};
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (tl.r0 + t * 16 >= tl.n) continue;      // wave-uniform tile skip
        floatx4 a = acc[r][t];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, af[j]),
              __builtin_bit_cast(bf16x8, xf[t][j]), a, 0, 0, 0);
        acc[r][t] = a;
      }
    }
  }

  // fixed-order K reduction: ((w0 + w1) + w2) + ... by wave 0
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        red[((wave - 1) * RT * MT + r * MT + t) * WAVE + lane] = acc[r][t];
  }
  block_barrier();
  if (wave != 0) return;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (tl.r0 + t * 16 >= tl.n) continue;
    const int p = rid[t];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      floatx4 a = acc[r][t];
      for (int w = 0; w < W - 1; ++w) {
        const floatx4 q = red[(w * RT * MT + r * MT + t) * WAVE + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] += q[e];
      }
      // C/D: lane holds D[channel = r*16 + hi*4 + e][row = lo of tile t]
      const int j = r * 16 + hi * 4;
      if (p >= 0 && j < Rtot)
        *reinterpret_cast<floatx4*>(y + (int64_t)p * Rtot + j) = a;
    }
  }
}

// 8 fp32 of y -> the lane's MFMA operand: part 0 = bf16(y), part 1 =
// bf16(y - bf16(y)).
__device__ __forceinline__ u32x4 split_y(const floatx4& a, const floatx4& b,
                                         int part) {
  u16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float v = i < 4 ? a[i] : b[i - 4];
    const uint16_t h = f32_to_bf16(v);
    const uint16_t l = f32_to_bf16(v - bf16_to_f32(h));
    o[i] = part ? l : h;
  }
  return __builtin_bit_cast(u32x4, o);
}

// grid (ceil(T / ROWS) + S, ceil(N / 256)), block 256.
template <int R, int MT>
__global__ __launch_bounds__(EXPAND_WAVES * WAVE) void lora_sgmv_expand_kernel(
    uint16_t* __restrict__ out,              // [T, N]
    const float* __restrict__ y,             // [T, Rtot]
    const uint16_t* __restrict__ B,          // [S, N, R]
    const int* __restrict__ seg_off,         // [S + 1]
    const int* __restrict__ rows,            // [T]
    const float* __restrict__ scale,         // [S]
    SliceOffsets so, int T, int N, int Rtot, int S) {
  constexpr int NM = R <= 16 ? 1 : R / 16;   // MFMAs per column tile
  __shared__ float stage[EXPAND_WAVES][16 * STAGE_PITCH];
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int lo = lane & 15, hi = lane >> 4;

  Tile tl;
  if (!find_tile<16 * MT>(seg_off, S, T, __builtin_amdgcn_workgroup_id_x(),
                          lane, tl))
    return;                                  // workgroup-uniform
  const int nw0 = __builtin_amdgcn_workgroup_id_y() * EXPAND_COLS + wave * 64;
  if (nw0 >= N) return;                      // wave-uniform; no barrier below

  int rid[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int i = tl.r0 + t * 16 + lo;
    int p = i < tl.n ? rows[tl.list0 + i] : -1;
    if (p >= T) p = -1;
    rid[t] = p;
  }

  const int jl = (hi & 1) * 8, part = hi >> 1;
  u32x4 bf[4][NM];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int n = nw0 + ct * 16 + lo;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int j = m * 16 + jl;
      if (n < N && j < R)
        bf[ct][m] = *reinterpret_cast<const u32x4*>(
            B + ((int64_t)tl.s * N + n) * R + j);
      else
        bf[ct][m] = u32x4{0, 0, 0, 0};
    }
  }
  const float sc = scale[tl.s];
  float* st = stage[wave];

#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (tl.r0 + t * 16 >= tl.n) continue;    // wave-uniform tile skip
    int cur = -1;
    u32x4 yf[NM];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int n0 = nw0 + ct * 16;
      if (n0 >= N) continue;                 // wave-uniform
      const int sl = (n0 >= so.off[1]) + (n0 >= so.off[2]);
      if (sl != cur) {                       // wave-uniform
        cur = sl;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const int j = m * 16 + jl;
          if (rid[t] >= 0 && j < R) {
            const floatx4* q = reinterpret_cast<const floatx4*>(
                y + (int64_t)rid[t] * Rtot + sl * R + j);
            yf[m] = split_y(q[0], q[1], part);
          } else {
            yf[m] = u32x4{0, 0, 0, 0};
          }
        }
      }
      floatx4 a = floatx4{0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < NM; ++m)
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(bf16x8, bf[ct][m]),
            __builtin_bit_cast(bf16x8, yf[m]), a, 0, 0, 0);
      // C/D: lane holds D[channel = ct*16 + hi*4 + e][row = lo]
      *reinterpret_cast<floatx4*>(st + lo * STAGE_PITCH + ct * 16 + hi * 4) = a;
    }
    wave_sync();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int row = pass * 8 + (lane >> 3);
      const int c = (lane & 7) * 8;
      const int p = lane_read(rid[t], row);
      if (p >= 0 && nw0 + c < N) {
        const floatx4 d0 =
            *reinterpret_cast<const floatx4*>(st + row * STAGE_PITCH + c);
        const floatx4 d1 =
            *reinterpret_cast<const floatx4*>(st + row * STAGE_PITCH + c + 4);
        uint16_t* op = out + (int64_t)p * N + nw0 + c;
        float ov[8];
        load_bf16x8(op, ov);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          ov[i] = ov[i] + sc * (i < 4 ? d0[i] : d1[i - 4]);
        store_bf16x8(op, ov);
      }
    }
    wave_sync();                             // the strip is reused by tile t+1
  }
}

NO_PK_F32_END

void check_tensor(const torch::Tensor& t, const torch::Tensor& like,
                  c10::ScalarType dt, int64_t dim, const char* what) {
  TORCH_CHECK(t.is_cuda(), what, " must be on the GPU");
  TORCH_CHECK(t.device() == like.device(), what, ": device mismatch");
  TORCH_CHECK(t.scalar_type() == dt, what, " must be ", dt, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == dim, what, " must be ", dim, "-D");
  TORCH_CHECK(t.is_contiguous(), what, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what,
              " must be 16-byte aligned");
}

void check_groups(const torch::Tensor& seg_off, const torch::Tensor& rows,
                  const torch::Tensor& like, int64_t S, int64_t T) {
  TORCH_CHECK(S >= 1 && S <= SGMV_MAX_S, "lora_sgmv: slot count ", S,
              " must be in [1, ", SGMV_MAX_S, "]");
  check_tensor(seg_off, like, torch::kInt32, 1, "lora_sgmv: seg_off");
  check_tensor(rows, like, torch::kInt32, 1, "lora_sgmv: rows");
  TORCH_CHECK(seg_off.size(0) == S + 1, "lora_sgmv: seg_off must be [S + 1] = [",
              S + 1, "]");
  TORCH_CHECK(rows.size(0) == T, "lora_sgmv: rows must be [T] = [", T, "]");
}

}  // namespace

void lora_sgmv_shrink(torch::Tensor y, torch::Tensor x, torch::Tensor A,
                      torch::Tensor seg_off, torch::Tensor rows) {
  check_tensor(x, x, torch::kBFloat16, 2, "lora_sgmv_shrink: x");
  check_tensor(A, x, torch::kBFloat16, 3, "lora_sgmv_shrink: A");
  check_tensor(y, x, torch::kFloat32, 2, "lora_sgmv_shrink: y");
  const int64_t T = x.size(0), K = x.size(1);
  const int64_t S = A.size(0), Rtot = A.size(1);
  check_groups(seg_off, rows, x, S, T);
  TORCH_CHECK(T < (1LL << 31), "lora_sgmv_shrink: T too large");
  TORCH_CHECK(A.size(2) == K, "lora_sgmv_shrink: A K dim ", A.size(2), " != ",
              K);
  TORCH_CHECK(y.size(0) == T && y.size(1) == Rtot,
              "lora_sgmv_shrink: y must be [T, Rtot]");
  TORCH_CHECK(K >= 32 && K % 32 == 0 && K < (1 << 30),
              "lora_sgmv_shrink: K must be a multiple of 32, got ", K);
  const int rt = (int)((Rtot + 15) / 16);
  TORCH_CHECK(Rtot >= 8 && Rtot % 8 == 0 &&
              (rt == 1 || rt == 2 || rt == 3 || rt == 4 || rt == 6 ||
               rt == 8 || rt == 12),
              "lora_sgmv_shrink: Rtot must be n_slices (1..3) * Rmax "
              "(8, 16, 32, 64), got ", Rtot);
  if (T == 0) return;
  const int mt = sgmv_mt(T), W = sgmv_waves(Rtot, K);
  const int rows_per = 16 * mt;
  dim3 grid((unsigned)((T + rows_per - 1) / rows_per + S));
  const size_t lds = (size_t)(W - 1) * rt * mt * WAVE * sizeof(floatx4);
  auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_SHRINK(RT_, MT_)                                               \
  hipLaunchKernelGGL((lora_sgmv_shrink_kernel<RT_, MT_>), grid,               \
                     dim3(W * WAVE), lds, stream, (float*)y.data_ptr(),       \
                     (const uint16_t*)x.data_ptr(),                           \
                     (const uint16_t*)A.data_ptr(),                           \
                     (const int*)seg_off.data_ptr(),                          \
                     (const int*)rows.data_ptr(), (int)T, (int)K, (int)Rtot,  \
                     (int)S, W)
#define SHRINK_RT(RT_)                                                        \
  case RT_:                                                                   \
    if (mt == 1) LAUNCH_SHRINK(RT_, 1); else LAUNCH_SHRINK(RT_, 2);           \
    break
  switch (rt) {
    SHRINK_RT(1); SHRINK_RT(2); SHRINK_RT(3); SHRINK_RT(4); SHRINK_RT(6);
    SHRINK_RT(8);
    default:
      if (mt == 1) LAUNCH_SHRINK(12, 1); else LAUNCH_SHRINK(12, 2);
      break;
  }
#undef SHRINK_RT
#undef LAUNCH_SHRINK
}

void lora_sgmv_expand(torch::Tensor out, torch::Tensor y, torch::Tensor B,
                      torch::Tensor seg_off, torch::Tensor rows,
                      torch::Tensor scale, std::vector<int64_t> n_off) {
  check_tensor(out, out, torch::kBFloat16, 2, "lora_sgmv_expand: out");
  check_tensor(B, out, torch::kBFloat16, 3, "lora_sgmv_expand: B");
  check_tensor(y, out, torch::kFloat32, 2, "lora_sgmv_expand: y");
  check_tensor(scale, out, torch::kFloat32, 1, "lora_sgmv_expand: scale");
  const int64_t T = out.size(0), N = out.size(1);
  const int64_t S = B.size(0), Rmax = B.size(2), Rtot = y.size(1);
  const int64_t n_slices = (int64_t)n_off.size() - 1;
  check_groups(seg_off, rows, out, S, T);
  TORCH_CHECK(T < (1LL << 31), "lora_sgmv_expand: T too large");
  TORCH_CHECK(N >= 16 && N % 16 == 0 && N < (1 << 30),
              "lora_sgmv_expand: N must be a multiple of 16, got ", N);
  TORCH_CHECK(Rmax == 8 || Rmax == 16 || Rmax == 32 || Rmax == 64,
              "lora_sgmv_expand: Rmax must be 8, 16, 32 or 64, got ", Rmax);
  TORCH_CHECK(n_slices >= 1 && n_slices <= MAX_SLICES,
              "lora_sgmv_expand: n_off must describe 1..3 slices");
  TORCH_CHECK(Rtot == n_slices * Rmax, "lora_sgmv_expand: y width ", Rtot,
              " != n_slices * Rmax = ", n_slices * Rmax);
  TORCH_CHECK(B.size(1) == N, "lora_sgmv_expand: B N dim ", B.size(1), " != ",
              N);
  TORCH_CHECK(y.size(0) == T && scale.size(0) == S,
              "lora_sgmv_expand: y / scale shapes inconsistent");
  TORCH_CHECK(n_off.front() == 0 && n_off.back() == N,
              "lora_sgmv_expand: n_off must run from 0 to N");
  SliceOffsets so;
  for (int i = 0; i <= MAX_SLICES; ++i) so.off[i] = (int)N;
  for (int64_t i = 0; i <= n_slices; ++i) {
    TORCH_CHECK(n_off[i] % 16 == 0, "lora_sgmv_expand: slice boundary ",
                n_off[i], " is not a multiple of 16");
    TORCH_CHECK(i == 0 || n_off[i] >= n_off[i - 1],
                "lora_sgmv_expand: n_off must be non-decreasing");
    so.off[i] = (int)n_off[i];
  }
  if (T == 0) return;
  const int mt = sgmv_mt(T);
  const int rows_per = 16 * mt;
  dim3 grid((unsigned)((T + rows_per - 1) / rows_per + S),
            (unsigned)((N + EXPAND_COLS - 1) / EXPAND_COLS));
  auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_EXPAND(R_, MT_)                                                \
  hipLaunchKernelGGL((lora_sgmv_expand_kernel<R_, MT_>), grid,                \
                     dim3(EXPAND_WAVES * WAVE), 0, stream,                    \
                     (uint16_t*)out.data_ptr(), (const float*)y.data_ptr(),   \
                     (const uint16_t*)B.data_ptr(),                           \
                     (const int*)seg_off.data_ptr(),                          \
                     (const int*)rows.data_ptr(),                             \
                     (const float*)scale.data_ptr(), so, (int)T, (int)N,      \
                     (int)Rtot, (int)S)
#define EXPAND_R(R_)                                                          \
  case R_:                                                                    \
    if (mt == 1) LAUNCH_EXPAND(R_, 1); else LAUNCH_EXPAND(R_, 2);             \
    break
  switch (Rmax) {
    EXPAND_R(8); EXPAND_R(16); EXPAND_R(32);
    default:
      if (mt == 1) LAUNCH_EXPAND(64, 1); else LAUNCH_EXPAND(64, 2);
      break;
  }
#undef EXPAND_R
#undef LAUNCH_EXPAND
}
