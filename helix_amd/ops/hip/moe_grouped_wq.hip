// Mixture-of-experts routed expert GEMMs for prefill over ggml Q4_0 / Q8_0
// experts: moe_grouped.hip's grouped, LDS-tiled MFMA kernels with the weight
// operand dequantised on its way into LDS (gfx950).
//
//   act[p, n]   = bf16(silu(x[p/k] . dq(w13)[e, n]) * (x[p/k] . dq(w13)[e, I+n]))
//   ypair[p, n] = topk_w[p] * (act[p] . dq(w2)[e, n])                  (fp32)
//
// Operands are moe_wq.hip's plane stacks (qs and d with the expert in front;
// its header has the layout), the intermediates and rounding points are
// moe.hip's; moe_route, moe_align and moe_combine are shared.
//
// moe_grouped_wq_kernel<BITS, GATED, BM>, 4 waves, grid (row tiles, channel
// tiles). From moe_grouped_kernel, through moe_grouped_common.h and
// unchanged: the tile lookup (find_tile) with its workgroup-uniform return
// and corrupt-list guard; the 128-row channel tile (64 gate + 64 up rows when
// GATED); the 2 x 2 wave layout with 4 channel tiles x BM/32 row tiles of
// mfma_f32_16x16x32_bf16 per wave; the wave-uniform tile skips; the K step of
// 64, double buffered with one barrier per step; the gathered row operand;
// the 144-byte LDS pitch and the ds_read_b128 fragments; weights as the A
// operand; both epilogues; row tiles fastest in the grid.
//
// The weight side is this file's own. LDS holds bf16 in natural K order, so
// the MFMA loop cannot tell this kernel from moe_grouped_kernel. A weight row
// is staged by TWO threads (row = tid / 2, c = tid % 2); thread c owns block
// 2 step + c of every step: elements [32c, 32c + 32) of the step, LDS bytes
// [64c, 64c + 64) of the row.
//   * load(step + 1), issued before the MFMAs of `step` and after the row
//     operand's loads: the block's raw bytes to registers, one b128 (Q4_0) or
//     two (Q8_0) plus its fp16 scale, read as a 2-byte load (a row of d has
//     K/32 halves and is only 2-byte aligned when that is odd). The two
//     threads of a row request 32 (Q4_0) or 64 (Q8_0) contiguous bytes; a
//     workgroup has 4 / 8 KiB in flight across one step of MFMAs.
//   * stage, after the step's MFMAs and just before the barrier: decode the
//     block with wq_frag<BITS, 0..3> (fma(nib, d, -8d) / fma(byte ^ 0x80, d,
//     -128d), ONE rounding to bf16: dequant_wq's bits) and four ds_write_b128
//     into the other buffer at 64c + 16j.
//   * Fetching by 128-element span (four blocks of a row, i.e. two steps, at
//     once and two steps ahead: twice the bytes in flight, twice as long)
//     was built and MEASURED SLOWER, 2-3 % (Q4_0) and 7-10 % (Q8_0) on the
//     Mixtral layer at T = 256 and 512 in two runs, and left the tree
//     (docs/KERNELS.md, profiles/r18_moe_grouped_wq.md).
//   * K % 32 == 0 is the only K requirement: steps = ceil(K / 64); a block at
//     or past K/32 and a weight row at or past N are +0, never loaded
//     (WQRaw's invalid state); the row operand's vectors at or past K are
//     zero-filled, because 0 * garbage may be NaN.
//
// Arithmetic contract: every accumulator takes 32-element K chunks in
// ascending natural order, and the A operand is the bf16 value dequant_wq
// produces, so act, ypair and out are bit-identical to moe_grouped_gated /
// moe_grouped_down on the dequantised stack, and moe_grouped's row
// independence carries over. No split-K, no atomics, nothing accumulated
// across workgroups.
//
// LDS: 2 x (128 + BM) x 144 bytes + the pair ids, 72.5 KiB at BM = 128, two
// workgroups per CU, as moe_grouped_kernel. docs/KERNELS.md has the resource
// table and what was chosen without a measurement.
#include "moe_grouped_common.h"

NO_PK_F32_BEGIN
#include "dequant_common.h"
NO_PK_F32_END
#include "moe_wq_common.h"
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

NO_PK_F32_BEGIN

// One thread's share (row, c) of a weight row of the tile: blocks 2 step + c.
template <int BITS>
struct BlockLoader {
  const uint8_t* qs;       // the stack's payload plane
  const uint16_t* ds;      // the stack's scale plane
  int64_t row;             // weight row, expert included
  int nblk, c;
  bool valid;              // false: a row at or past N, +0 and never loaded
  WQRaw<BITS> r;           // the block in flight

  __device__ __forceinline__ void load(int step) {
    const int kb = 2 * step + c;
    r = wq_load<BITS>(qs, ds, row, kb, nblk, valid && kb < nblk);
  }
  // the 32 bf16 of the block in flight, at LDS row dst
  __device__ __forceinline__ void stage(uint8_t* dst) const {
    dst += 64 * c;
    *reinterpret_cast<u32x4*>(dst) =
        __builtin_bit_cast(u32x4, wq_frag<BITS, 0>(r));
    *reinterpret_cast<u32x4*>(dst + 16) =
        __builtin_bit_cast(u32x4, wq_frag<BITS, 1>(r));
    *reinterpret_cast<u32x4*>(dst + 32) =
        __builtin_bit_cast(u32x4, wq_frag<BITS, 2>(r));
    *reinterpret_cast<u32x4*>(dst + 48) =
        __builtin_bit_cast(u32x4, wq_frag<BITS, 3>(r));
  }
};

template <int BITS, bool GATED, int BM>
__global__ __launch_bounds__(GROUPED_THREADS) void moe_grouped_wq_kernel(
    void* __restrict__ dst,                  // GATED: bf16 act[P, N]; else fp32 ypair[P, N]
    const uint16_t* __restrict__ src,        // GATED: x[T, K]; else act[P, K]
    const uint8_t* __restrict__ qs,          // [E, GATED ? 2N : N, K/2 or K]
    const uint16_t* __restrict__ ds,         // [E, GATED ? 2N : N, K/32] fp16
    const float* __restrict__ topk_w,        // [P] (!GATED)
    const int32_t* __restrict__ expert_off,  // [E + 1]
    const int32_t* __restrict__ sorted_pairs,  // [P]
    int P, int N, int K, int E, int k) {
  constexpr int RT = BM / 32;                // 16-row tiles per wave
  constexpr int CT = 4;                      // 16-channel tiles per wave
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

  const int n0 = __builtin_amdgcn_workgroup_id_y() * (GATED ? BN / 2 : BN);

  // weight side: LDS row wrow, 32-element half of every step
  const int wrow = tid >> 1;
  const int wch = GATED ? n0 + (wrow & 63) : n0 + wrow;
  BlockLoader<BITS> wl;
  wl.qs = qs;
  wl.ds = ds;
  wl.row =
      (int64_t)tl.e * (GATED ? 2 * N : N) + (GATED ? (wrow >> 6) * N : 0) + wch;
  wl.nblk = K / 32;
  wl.c = tid & 1;
  wl.valid = wch < N;

  // row side: staging row and 16-byte column
  const int sr = tid >> 3, sc = tid & 7;
  int64_t x_off[XV];                         // element offsets, -1: zero-fill
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
  u32x4 xv[XV];
  // the thread's vector of step s, zero at or past K
  auto x_fetch = [&](int s) {
    const int kv = s * BK + sc * 8;
    if (kv < K) {
      tile_fetch<XV>(xv, src, x_off, kv);
    } else {
#pragma unroll
      for (int i = 0; i < XV; ++i) xv[i] = u32x4{0, 0, 0, 0};
    }
  };

  x_fetch(0);
  wl.load(0);
  wl.stage(lds + wrow * PITCH);
  tile_stage<XV>(lds + W_BYTES, xv, sr, sc);
  block_barrier();

  for (int s = 0; s < steps; ++s) {
    const uint8_t* wb = lds + (s & 1) * BUF_BYTES;
    const uint8_t* xb = wb + W_BYTES;
    const bool more = s + 1 < steps;         // workgroup-uniform
    if (more) {
      x_fetch(s + 1);
      wl.load(s + 1);
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
      wl.stage(nb + wrow * PITCH);
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

struct GroupedWQArgs {
  void* dst;
  const uint16_t* src;
  const uint8_t* qs;
  const uint16_t* ds;
  const float* tw;
  const int32_t* off;
  const int32_t* pairs;
  int64_t P;
  int N, K, E, k;
};

template <int BITS, bool GATED>
void launch_grouped_wq(const GroupedWQArgs& a) {
  const int bm = grouped_bm(a.P, a.E);
  const dim3 grid((unsigned)((a.P + bm - 1) / bm + a.E),
                  (unsigned)cdiv(a.N, GATED ? BN / 2 : BN));
  auto stream = at::hip::getCurrentHIPStream();
#define GROUPED_WQ_LAUNCH(BM_)                                                \
  hipLaunchKernelGGL((moe_grouped_wq_kernel<BITS, GATED, BM_>), grid,         \
                     dim3(GROUPED_THREADS), 0, stream, a.dst, a.src, a.qs,    \
                     a.ds, a.tw, a.off, a.pairs, (int)a.P, a.N, a.K, a.E, a.k)
  if (bm == 64) GROUPED_WQ_LAUNCH(64); else GROUPED_WQ_LAUNCH(128);
#undef GROUPED_WQ_LAUNCH
}

template <bool GATED>
void dispatch_grouped_wq(int64_t bits, const GroupedWQArgs& a) {
  if (bits == 4)
    launch_grouped_wq<4, GATED>(a);
  else
    launch_grouped_wq<8, GATED>(a);
}

}  // namespace

// act[P, I] = silu(x[p/k] @ dq(w13[e, :I])^T) * (x[p/k] @ dq(w13[e, I:])^T)
void moe_grouped_gated_wq(torch::Tensor act, torch::Tensor x,
                          torch::Tensor w13_qs, torch::Tensor w13_d,
                          int64_t bits, torch::Tensor expert_off,
                          torch::Tensor sorted_pairs, int64_t k) {
  int64_t rows = 0, H = 0;
  const int64_t E = check_stack_wq(w13_qs, w13_d, bits,
                                   "moe_grouped_gated_wq: w13", &rows, &H);
  TORCH_CHECK(x.dim() == 2 && act.dim() == 2,
              "moe_grouped_gated_wq: x and act must be 2-D");
  const int64_t I = rows / 2;
  const int64_t T = x.size(0), P = T * k;
  check_ek(E, k);
  check_tensor(x, w13_qs, torch::kBFloat16, "moe_grouped_gated_wq: x");
  check_tensor(act, w13_qs, torch::kBFloat16, "moe_grouped_gated_wq: act");
  TORCH_CHECK(I > 0 && I % 16 == 0 && rows == 2 * I,
              "moe_grouped_gated_wq: w13 must have 2I rows with I (", I,
              ") a positive multiple of 16");
  TORCH_CHECK(x.size(1) == H,
              "moe_grouped_gated_wq: x must be [T, H], H = ", H);
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_grouped_gated_wq: act must be [T*k, I] = [", P, ", ", I,
              "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && I / 64 < 65535,
              "moe_grouped_gated_wq: problem too large");
  check_lists(expert_off, sorted_pairs, w13_qs, E, P);
  if (T == 0) return;
  GroupedWQArgs a{};
  a.dst = act.data_ptr();
  a.src = (const uint16_t*)x.data_ptr();
  a.qs = (const uint8_t*)w13_qs.data_ptr();
  a.ds = (const uint16_t*)w13_d.data_ptr();
  a.off = (const int32_t*)expert_off.data_ptr();
  a.pairs = (const int32_t*)sorted_pairs.data_ptr();
  a.P = P, a.N = (int)I, a.K = (int)H, a.E = (int)E, a.k = (int)k;
  dispatch_grouped_wq<true>(bits, a);
}

// ypair[P, H] (fp32) = topk_w[p] * (act[p] @ dq(w2[e])^T)
void moe_grouped_down_wq(torch::Tensor ypair, torch::Tensor act,
                         torch::Tensor w2_qs, torch::Tensor w2_d, int64_t bits,
                         torch::Tensor topk_w, torch::Tensor expert_off,
                         torch::Tensor sorted_pairs) {
  int64_t H = 0, I = 0;
  const int64_t E = check_stack_wq(w2_qs, w2_d, bits,
                                   "moe_grouped_down_wq: w2", &H, &I);
  TORCH_CHECK(act.dim() == 2 && ypair.dim() == 2 && topk_w.dim() == 2,
              "moe_grouped_down_wq: act, ypair and topk_w must be 2-D");
  const int64_t T = topk_w.size(0), k = topk_w.size(1), P = T * k;
  check_ek(E, k);
  check_tensor(act, w2_qs, torch::kBFloat16, "moe_grouped_down_wq: act");
  check_tensor(ypair, w2_qs, torch::kFloat32, "moe_grouped_down_wq: ypair");
  check_tensor(topk_w, w2_qs, torch::kFloat32, "moe_grouped_down_wq: topk_w");
  TORCH_CHECK(H > 0 && H % 16 == 0, "moe_grouped_down_wq: H (", H,
              ") must be a positive multiple of 16");
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_grouped_down_wq: act must be [T*k, I] = [", P, ", ", I,
              "]");
  TORCH_CHECK(ypair.size(0) == P && ypair.size(1) == H,
              "moe_grouped_down_wq: ypair must be [T*k, H] = [", P, ", ", H,
              "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && H / 128 < 65535,
              "moe_grouped_down_wq: problem too large");
  check_lists(expert_off, sorted_pairs, w2_qs, E, P);
  if (T == 0) return;
  GroupedWQArgs a{};
  a.dst = ypair.data_ptr();
  a.src = (const uint16_t*)act.data_ptr();
  a.qs = (const uint8_t*)w2_qs.data_ptr();
  a.ds = (const uint16_t*)w2_d.data_ptr();
  a.tw = (const float*)topk_w.data_ptr();
  a.off = (const int32_t*)expert_off.data_ptr();
  a.pairs = (const int32_t*)sorted_pairs.data_ptr();
  a.P = P, a.N = (int)H, a.K = (int)I, a.E = (int)E, a.k = (int)k;
  dispatch_grouped_wq<false>(bits, a);
}
