// Mixture-of-experts routed expert GEMMs for prefill over ggml Q4_K / Q6_K
// experts: moe_grouped.hip's grouped, LDS-tiled MFMA kernels with the weight
// operand dequantised on its way into LDS (gfx950).
//
//   act[p, n]   = bf16(silu(x[p/k] . dq(w13)[e, n]) * (x[p/k] . dq(w13)[e, I+n]))
//   ypair[p, n] = topk_w[p] * (act[p] . dq(w2)[e, n])                  (fp32)
//
// Operands are moe_kq.hip's plane stacks (its header has the layout), the
// intermediates and rounding points are moe.hip's; moe_route, moe_align and
// moe_combine are shared.
//
// moe_grouped_kq_kernel<FMT, GATED, BM>, 4 waves, grid (row tiles, channel
// tiles). From moe_grouped_kernel, unchanged: the tile lookup (find_tile)
// with its workgroup-uniform return and corrupt-list guard; the 128-row
// channel tile (64 gate + 64 up rows when GATED); the 2 x 2 wave layout with
// 4 channel tiles x BM/32 row tiles of mfma_f32_16x16x32_bf16 per wave; the
// wave-uniform tile skips; the K step of 64, double buffered with one barrier
// per step; the gathered row operand (8 lanes per 128-byte row run); the
// 144-byte LDS pitch and the ds_read_b128 fragments; weights as the A
// operand; both epilogues; row tiles fastest in the grid.
//
// The weight side is this file's own. LDS holds bf16: the weight half of a
// buffer is the tile moe_grouped_kernel stages, in natural K order, so the
// MFMA loop cannot tell the two kernels apart. A weight row is staged by TWO
// threads (row = tid / 2, c = tid % 2; 256 threads, 128 rows), each of which
// owns 32 of the step's 64 elements:
//   * fetch(step), issued before the MFMAs of the step before: raw bytes to
//     registers, b128 loads.
//       Q4_K, j2 = step % 4 of super-block step / 4: the 16 payload bytes
//         qs[32 j2 + 16c ..] every step (4 VGPRs) and the super-block's
//         16-byte header when j2 = 0 (4 VGPRs, kept for its four steps).
//       Q6_K, half h = (step / 2) % 2 of the super-block, nibble side
//         step % 2: when the side is 0, the half's bytes ql[64h + 16c ..],
//         ql[64h + 32 + 16c ..], qh[32h + 16c ..], its 8 scales and d
//         (15 VGPRs), kept for both steps: no ql byte is loaded twice.
//     Against 16 VGPRs of bf16 per thread in moe_grouped_kernel.
//   * stage(step), after the MFMAs and just before the barrier: decode with
//     kq_common.h / dequant_common.h arithmetic (q4k_scale_min, dq8 =
//     fma(q, d*sc, off) and ONE rounding to bf16, dequant_kq's) and four
//     ds_write_b128 into the other buffer. Nibble side p in {0, 1} (Q4_K:
//     low / high nibbles = sub-blocks 2 j2 + p; Q6_K: groups 2 side + p) of
//     bytes 16c .. 16c+15 are elements 32p + 16c .. of the step: LDS bytes
//     [64p + 32c, 64p + 32c + 32) of the row. Scale fields are decoded again
//     in every step (two q4k_scale_min resp. two byte picks) rather than
//     carried: it costs a few VALU ops next to 32 cvt/fma and saves 4 VGPRs.
//   * A weight row at or past N is zero-filled, never loaded. K % 256 == 0,
//     so there is no K tail in either operand.
//
// Arithmetic contract: every accumulator takes 32-element K chunks in
// ascending natural order, and the A operand is the bf16 value dequant_kq
// produces, so act, ypair and out are bit-identical to moe_grouped_gated /
// moe_grouped_down on the dequantised stack, and moe_grouped's row
// independence carries over. No split-K, no atomics, nothing accumulated
// across workgroups.
//
// LDS: 2 x (128 + BM) x 144 bytes + the pair ids, 72.5 KiB at BM = 128, two
// workgroups per CU, as moe_grouped_kernel. docs/KERNELS.md has the resource
// table and what was chosen without a measurement.

// Device code of this file is compiled without packed fp32 arithmetic, as
// moe_grouped.hip's; the attribute region has to cover the shared headers.
// moe_grouped_common.h has the macros and what this kernel shares with
// moe_grouped_wq.hip: the tile geometry, find_tile, the row operand's staging.
#include "moe_grouped_common.h"

NO_PK_F32_BEGIN
#include "kq_common.h"
NO_PK_F32_END
#include "moe_kq_common.h"
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

NO_PK_F32_BEGIN

// 16 bytes of 6-bit resp. 4-bit codes (one per byte) -> 16 bf16 at dst.
__device__ __forceinline__ void stage16(uint8_t* dst, const u32x4& q, float s,
                                        float o) {
  *reinterpret_cast<u32x4*>(dst) =
      __builtin_bit_cast(u32x4, dq8(q[0], q[1], s, o));
  *reinterpret_cast<u32x4*>(dst + 16) =
      __builtin_bit_cast(u32x4, dq8(q[2], q[3], s, o));
}

// The weight loader: one thread's share (row, c) of a weight row of the tile.
// fetch(step) loads what step `step` needs and is not held yet; stage(dst,
// step) decodes the step's 32 elements of the thread to bf16 at LDS row
// `dst`. Steps are fetched and staged in ascending order, fetch before stage.
template <int FMT>
struct WeightLoader;

template <>
struct WeightLoader<4> {
  const uint8_t* qs;       // the row's payload, + 16c; nullptr: zero row
  const uint8_t* hdr;      // the row's headers
  u32x4 q, h;

  __device__ __forceinline__ WeightLoader(const void* p0, const void* p1,
                                          const void*, const void*,
                                          int64_t blk0, int c, bool valid) {
    qs = valid ? (const uint8_t*)p0 + blk0 * 128 + 16 * c : nullptr;
    hdr = (const uint8_t*)p1 + blk0 * 16;
    q = h = u32x4{0, 0, 0, 0};
  }
  __device__ __forceinline__ void fetch(int step) {
    if (qs == nullptr) return;
    q = *reinterpret_cast<const u32x4*>(qs + (int64_t)step * 32);
    if ((step & 3) == 0)
      h = *reinterpret_cast<const u32x4*>(hdr + (int64_t)(step >> 2) * 16);
  }
  __device__ __forceinline__ void stage(uint8_t* dst, int step, int c) const {
    dst += 32 * c;
    if (qs == nullptr) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<u32x4*>(dst + 64 * (i >> 1) + 16 * (i & 1)) =
            u32x4{0, 0, 0, 0};
      return;
    }
    const int j2 = step & 3;
    const float d = half_bits_to_f32((uint16_t)(h[0] & 0xffffu));
    const float dmin = half_bits_to_f32((uint16_t)(h[0] >> 16));
#pragma unroll
    for (int p = 0; p < 2; ++p) {                // sub-block 2 j2 + p
      float s, o;
      q4k_scale_min(h[1], h[2], h[3], (2 * j2 + p) & 3, j2 >= 2, d, dmin, &s,
                    &o);
      stage16(dst + 64 * p, (q >> (uint32_t)(4 * p)) & 0x0f0f0f0fu, s, o);
    }
  }
};

template <>
struct WeightLoader<6> {
  const uint8_t* ql;       // the row's low nibbles, + 16c; nullptr: zero row
  const uint8_t* qh;       // the row's high bits, + 16c
  const int8_t* sc;        // the row's scales
  const uint16_t* ds;      // the row's d
  u32x4 l[2], hb;
  u32x2 sv;
  uint16_t d16;

  __device__ __forceinline__ WeightLoader(const void* p0, const void* p1,
                                          const void* p2, const void* p3,
                                          int64_t blk0, int c, bool valid) {
    ql = valid ? (const uint8_t*)p0 + blk0 * 128 + 16 * c : nullptr;
    qh = (const uint8_t*)p1 + blk0 * 64 + 16 * c;
    sc = (const int8_t*)p2 + blk0 * 16;
    ds = (const uint16_t*)p3 + blk0;
    l[0] = l[1] = hb = u32x4{0, 0, 0, 0};
    sv = u32x2{0, 0};
    d16 = 0;
  }
  __device__ __forceinline__ void fetch(int step) {
    if (ql == nullptr || (step & 1)) return;
    const int64_t hf = step >> 1;                // 128-element halves so far
    l[0] = *reinterpret_cast<const u32x4*>(ql + hf * 64);
    l[1] = *reinterpret_cast<const u32x4*>(ql + hf * 64 + 32);
    hb = *reinterpret_cast<const u32x4*>(qh + hf * 32);
    sv = *reinterpret_cast<const u32x2*>(sc + hf * 8);
    d16 = ds[hf >> 1];
  }
  __device__ __forceinline__ void stage(uint8_t* dst, int step, int c) const {
    dst += 32 * c;
    if (ql == nullptr) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<u32x4*>(dst + 64 * (i >> 1) + 16 * (i & 1)) =
            u32x4{0, 0, 0, 0};
      return;
    }
    const int side = step & 1;                   // groups 2 side + p
    const float d = half_bits_to_f32(d16);
    const uint32_t svs = side ? sv[1] : sv[0];   // scales[8h + 4 side ..]
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      // scales[8h + 2g + c], g = 2 side + p: byte 2p + c of svs
      const int v = (int)(int8_t)((svs >> (uint32_t)(16 * p + 8 * c)) & 0xffu);
      const float s = d * (float)v;
      const u32x4 u =
          ((l[p] >> (uint32_t)(4 * side)) & 0x0f0f0f0fu) |
          (((hb >> (uint32_t)(4 * side + 2 * p)) & 0x03030303u) << 4);
      stage16(dst + 64 * p, u, s, -32.f * s);
    }
  }
};

template <int FMT, bool GATED, int BM>
__global__ __launch_bounds__(GROUPED_THREADS) void moe_grouped_kq_kernel(
    void* __restrict__ dst,                  // GATED: bf16 act[P, N]; else fp32 ypair[P, N]
    const uint16_t* __restrict__ src,        // GATED: x[T, K]; else act[P, K]
    const void* __restrict__ p0, const void* __restrict__ p1,
    const void* __restrict__ p2, const void* __restrict__ p3,
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

  // weight side: LDS row wrow, 32-element half wcol of every step
  const int wrow = tid >> 1, wcol = tid & 1;
  const int wch = GATED ? n0 + (wrow & 63) : n0 + wrow;
  const int64_t w_row =
      (int64_t)tl.e * (GATED ? 2 * N : N) + (GATED ? (wrow >> 6) * N : 0) + wch;
  WeightLoader<FMT> wl(p0, p1, p2, p3, w_row * (K / KQ_SB), wcol, wch < N);

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

  const int steps = K / BK;
  u32x4 xv[XV];
  wl.fetch(0);
  tile_fetch<XV>(xv, src, x_off, sc * 8);
  wl.stage(lds + wrow * PITCH, 0, wcol);
  tile_stage<XV>(lds + W_BYTES, xv, sr, sc);
  block_barrier();

  for (int s = 0; s < steps; ++s) {
    const uint8_t* wb = lds + (s & 1) * BUF_BYTES;
    const uint8_t* xb = wb + W_BYTES;
    const bool more = s + 1 < steps;         // workgroup-uniform
    if (more) {
      wl.fetch(s + 1);
      tile_fetch<XV>(xv, src, x_off, (s + 1) * BK + sc * 8);
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
      wl.stage(nb + wrow * PITCH, s + 1, wcol);
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

struct GroupedKQArgs {
  void* dst;
  const uint16_t* src;
  const void* p[4];
  const float* tw;
  const int32_t* off;
  const int32_t* pairs;
  int64_t P;
  int N, K, E, k;
};

template <int FMT, bool GATED>
void launch_grouped_kq(const GroupedKQArgs& a) {
  const int bm = grouped_bm(a.P, a.E);
  const dim3 grid((unsigned)((a.P + bm - 1) / bm + a.E),
                  (unsigned)cdiv(a.N, GATED ? BN / 2 : BN));
  auto stream = at::hip::getCurrentHIPStream();
#define GROUPED_KQ_LAUNCH(BM_)                                                \
  hipLaunchKernelGGL((moe_grouped_kq_kernel<FMT, GATED, BM_>), grid,          \
                     dim3(GROUPED_THREADS), 0, stream, a.dst, a.src, a.p[0],  \
                     a.p[1], a.p[2], a.p[3], a.tw, a.off, a.pairs, (int)a.P,  \
                     a.N, a.K, a.E, a.k)
  if (bm == 64) GROUPED_KQ_LAUNCH(64); else GROUPED_KQ_LAUNCH(128);
#undef GROUPED_KQ_LAUNCH
}

template <bool GATED>
void dispatch_grouped_kq(int fmt, const GroupedKQArgs& a) {
  if (fmt == 4)
    launch_grouped_kq<4, GATED>(a);
  else
    launch_grouped_kq<6, GATED>(a);
}

}  // namespace

// act[P, I] = silu(x[p/k] @ dq(w13[e, :I])^T) * (x[p/k] @ dq(w13[e, I:])^T)
void moe_grouped_gated_kq(torch::Tensor act, torch::Tensor x,
                          std::vector<torch::Tensor> w13_planes,
                          std::string fmt_name, torch::Tensor expert_off,
                          torch::Tensor sorted_pairs, int64_t k) {
  const int fmt = moe_kq_fmt(fmt_name, "moe_grouped_gated_kq");
  int64_t rows = 0, H = 0;
  const int64_t E = check_stack_kq(w13_planes, fmt,
                                   "moe_grouped_gated_kq: w13", &rows, &H);
  const auto& like = w13_planes[0];
  TORCH_CHECK(x.dim() == 2 && act.dim() == 2,
              "moe_grouped_gated_kq: x and act must be 2-D");
  const int64_t I = rows / 2;
  const int64_t T = x.size(0), P = T * k;
  check_ek(E, k);
  check_tensor(x, like, torch::kBFloat16, "moe_grouped_gated_kq: x");
  check_tensor(act, like, torch::kBFloat16, "moe_grouped_gated_kq: act");
  TORCH_CHECK(I > 0 && I % 16 == 0 && rows == 2 * I,
              "moe_grouped_gated_kq: w13 must have 2I rows with I (", I,
              ") a positive multiple of 16");
  TORCH_CHECK(x.size(1) == H,
              "moe_grouped_gated_kq: x must be [T, H], H = ", H);
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_grouped_gated_kq: act must be [T*k, I] = [", P, ", ", I,
              "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && I / 64 < 65535,
              "moe_grouped_gated_kq: problem too large");
  check_lists(expert_off, sorted_pairs, like, E, P);
  if (T == 0) return;
  GroupedKQArgs a{};
  a.dst = act.data_ptr();
  a.src = (const uint16_t*)x.data_ptr();
  for (size_t i = 0; i < w13_planes.size(); ++i)
    a.p[i] = w13_planes[i].data_ptr();
  a.off = (const int32_t*)expert_off.data_ptr();
  a.pairs = (const int32_t*)sorted_pairs.data_ptr();
  a.P = P, a.N = (int)I, a.K = (int)H, a.E = (int)E, a.k = (int)k;
  dispatch_grouped_kq<true>(fmt, a);
}

// ypair[P, H] (fp32) = topk_w[p] * (act[p] @ dq(w2[e])^T)
void moe_grouped_down_kq(torch::Tensor ypair, torch::Tensor act,
                         std::vector<torch::Tensor> w2_planes,
                         std::string fmt_name, torch::Tensor topk_w,
                         torch::Tensor expert_off,
                         torch::Tensor sorted_pairs) {
  const int fmt = moe_kq_fmt(fmt_name, "moe_grouped_down_kq");
  int64_t H = 0, I = 0;
  const int64_t E = check_stack_kq(w2_planes, fmt, "moe_grouped_down_kq: w2",
                                   &H, &I);
  const auto& like = w2_planes[0];
  TORCH_CHECK(act.dim() == 2 && ypair.dim() == 2 && topk_w.dim() == 2,
              "moe_grouped_down_kq: act, ypair and topk_w must be 2-D");
  const int64_t T = topk_w.size(0), k = topk_w.size(1), P = T * k;
  check_ek(E, k);
  check_tensor(act, like, torch::kBFloat16, "moe_grouped_down_kq: act");
  check_tensor(ypair, like, torch::kFloat32, "moe_grouped_down_kq: ypair");
  check_tensor(topk_w, like, torch::kFloat32, "moe_grouped_down_kq: topk_w");
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_grouped_down_kq: act must be [T*k, I] = [", P, ", ", I,
              "]");
  TORCH_CHECK(ypair.size(0) == P && ypair.size(1) == H,
              "moe_grouped_down_kq: ypair must be [T*k, H] = [", P, ", ", H,
              "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && H / 128 < 65535,
              "moe_grouped_down_kq: problem too large");
  check_lists(expert_off, sorted_pairs, like, E, P);
  if (T == 0) return;
  GroupedKQArgs a{};
  a.dst = ypair.data_ptr();
  a.src = (const uint16_t*)act.data_ptr();
  for (size_t i = 0; i < w2_planes.size(); ++i)
    a.p[i] = w2_planes[i].data_ptr();
  a.tw = (const float*)topk_w.data_ptr();
  a.off = (const int32_t*)expert_off.data_ptr();
  a.pairs = (const int32_t*)sorted_pairs.data_ptr();
  a.P = P, a.N = (int)H, a.K = (int)I, a.E = (int)E, a.k = (int)k;
  dispatch_grouped_kq<false>(fmt, a);
}
