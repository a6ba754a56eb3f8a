// Routed expert GEMMs over ggml Q4_K / Q6_K expert weights (gfx950).
//
// moe_gemm_kq_kernel<FMT, GATED, MT, W> is moe_wq.hip's moe_gemm_wq_kernel
// with its weight operand replaced by gemm_kq.hip's: the expert stack stays
// in the super-block planes and is dequantised in registers.
//
// Planes of one expert stack (rows = 2I, K = H for w13; rows = H, K = I for
// w2; the expert is the slowest dimension, gate rows [:I], up [I:]):
//   q4_k : qs  uint8 [E, rows, K/2]
//          hdr uint8 [E, rows, K/256, 16]
//   q6_k : ql  uint8 [E, rows, K/2]
//          qh  uint8 [E, rows, K/4]
//          sc  int8  [E, rows, K/16]
//          d   fp16  [E, rows, K/256]
// i.e. gemm_kq's planes of the [E*rows, K] weight: a super-block never
// crosses a row, so a merged GGUF tensor [E, rows, K] unpacks as [E*rows, K].
//
// Unchanged from moe_gemm_wq_kernel: grid (channel tiles, E) with a
// workgroup-uniform return on an empty list; the corrupt-offset guard; chunks
// of 16*MT pairs whose pair ids and gathered source rows are loaded once per
// chunk; the wave-uniform tile skip; MT from T alone; W waves splitting K,
// summed through LDS as ((w0 + w1) + w2) + ...; both epilogues.
//
// From gemm_kq (kq_common.h, arithmetic unchanged, so the rounding argument
// in gemm_kq.hip's header holds): lane (lo, hi) owns 64 elements of channel
// row lo of a super-block; 8 MFMAs per super-block with the weights as the A
// operand; the x operand of MFMA j is the run gemm_kq documents.
//
// K split: a wave step is a WHOLE super-block (wave w takes w, w+W, ...), as
// in gemm_kq, not half of one. A half step would need a second lane mapping
// and decode next to the one whose rounding is argued and tested, for the
// one shape where it matters: Qwen3's down GEMM, K = I = 768 = 3
// super-blocks, where one of W = 4 waves idles. That wave costs no
// bandwidth: the workgroup reads the same bytes either way, and the kernel
// is bound by those bytes. W = moe_kq_waves(N, K, gated) is a function of
// the weight's shape alone, never of T.
//
// Registers: a K step runs as two passes, MFMAs 0..3 then 4..7. A pass
// dequantises its four fragments (16 VGPRs per weight row, two rows in the
// gated kernel) once and reuses them for the chunk's MT token tiles; x (16
// VGPRs) is loaded per tile inside the tile loop, so MT only adds
// accumulators, and each accumulator still takes MFMAs 0..7 in order. With
// all eight fragments held at once the 16-wave kernels (128 VGPRs) spilled.
// The one-tile kernels of up to 8 waves fetch the next step's weight bytes
// before they compute the current one; the 16-wave one has no room for it.
// No instantiation spills or uses scratch (docs/KERNELS.md has the table).
//
// No atomics, no accumulation across workgroups; a pair's bits do not
// depend on T, on its place in its list or on its tile's neighbours.
#include "kq_common.h"
#include "moe_common.h"
#include <ATen/hip/HIPContext.h>
#include <string>
#include <vector>

using namespace helix;

namespace {

// K-split factor of one expert's [N, K] K-quant weight: gemm_kq's rule (a
// wave per super-block until every wave of the result has at least one),
// with moe_waves' cap of 8 for the gated kernel (reduction buffer
// (W-1) x 2 x MT KiB under 64 KiB).
int moe_kq_waves_host(int64_t N, int64_t K, bool gated) {
  int w = 4;
  const int cap = gated ? 8 : 16;
  while (w < cap && (N / 16) * w < 4096 && K / KQ_SB >= 2 * w) w *= 2;
  return w;
}

// Fragments 4H .. 4H+3 of a super-block: the lane's x run H (gemm_kq's
// xoff0 / xoff1).
template <int FMT, int H>
__device__ __forceinline__ void kq_half_frags(const KQRaw<FMT>& raw,
                                              bf16x8 (&wf)[4]) {
  wf[0] = kq_frag<4 * H + 0>(raw);
  wf[1] = kq_frag<4 * H + 1>(raw);
  wf[2] = kq_frag<4 * H + 2>(raw);
  wf[3] = kq_frag<4 * H + 3>(raw);
}

template <int FMT, bool GATED, int MT, int W>
__global__ __launch_bounds__(W * WAVE) void moe_gemm_kq_kernel(
    void* __restrict__ dst,                  // GATED: bf16 act[P, N]; else fp32 ypair[P, N]
    const uint16_t* __restrict__ src,        // GATED: x[T, K]; else act[P, K]
    const void* __restrict__ p0, const void* __restrict__ p1,
    const void* __restrict__ p2, const void* __restrict__ p3,
    const float* __restrict__ topk_w,        // [P] (!GATED)
    const int32_t* __restrict__ expert_off,  // [E + 1]
    const int32_t* __restrict__ sorted_pairs,  // [P]
    int P, int N, int K, int k) {
  constexpr int CT = GATED ? 2 : 1;
  constexpr bool PREFETCH = MT == 1 && W <= 8;
  __shared__ floatx4 red[W - 1][CT * MT][WAVE];

  const int e = blockIdx.y;
  const int list0 = expert_off[e];
  const int n_e = expert_off[e + 1] - list0;
  // workgroup-uniform; the second test only fails on a corrupt offset table
  if (n_e <= 0) return;
  if (list0 < 0 || list0 + n_e > P) return;

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lo = lane & 15, hi = lane >> 4;
  const int nsb = K / KQ_SB;
  const int n0 = blockIdx.x * 16;
  const int rows = CT * N;                       // weight rows per expert
  int64_t blk0[CT];                              // first super-block of the row
#pragma unroll
  for (int c = 0; c < CT; ++c)
    blk0[c] = ((int64_t)e * rows + c * N + n0 + lo) * nsb;

  // x run(s) of the lane inside a super-block, in elements
  const int xoff0 = FMT == 4 ? 64 * hi : 128 * (hi >> 1) + 32 * (hi & 1);
  const int xoff1 = FMT == 4 ? xoff0 + 32 : xoff0 + 64;

  for (int c0 = 0; c0 < n_e; c0 += 16 * MT) {
    // the chunk's pairs and source rows, once, before the K loop
    int pair[MT];
    const uint16_t* xrow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int i = c0 + t * 16 + lo;
      int p = i < n_e ? sorted_pairs[list0 + i] : -1;
      if (p >= P) p = -1;
      pair[t] = p;
      const int r = GATED ? p / k : p;
      xrow[t] = src + (int64_t)(p < 0 ? 0 : r) * K;
    }

    floatx4 acc[CT][MT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[c][t] = floatx4{0, 0, 0, 0};

    KQFetch<FMT> nxt[CT];
    if constexpr (PREFETCH) {
      if (wave < nsb) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
          nxt[c] = kq_fetch<FMT>(p0, p1, p2, p3, blk0[c] + wave, hi);
      }
    }

    for (int sb = wave; sb < nsb; sb += W) {     // wave-uniform
      KQFetch<FMT> cur[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if constexpr (PREFETCH) {
          cur[c] = nxt[c];
          if (sb + W < nsb)
            nxt[c] = kq_fetch<FMT>(p0, p1, p2, p3, blk0[c] + sb + W, hi);
        } else {
          cur[c] = kq_fetch<FMT>(p0, p1, p2, p3, blk0[c] + sb, hi);
        }
      }

      KQRaw<FMT> raw[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) raw[c] = kq_decode(cur[c], hi);

      // MFMAs 0..3, then 4..7: each half's fragments are dequantised once
      // and reused by the MT token tiles; every accumulator still takes its
      // eight MFMAs in the order 0..7
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bf16x8 wf[CT][4];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          if (h == 0)
            kq_half_frags<FMT, 0>(raw[c], wf[c]);
          else
            kq_half_frags<FMT, 1>(raw[c], wf[c]);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          if (c0 + t * 16 >= n_e) continue;      // wave-uniform tile skip
          u32x4 xf[4];
          if (pair[t] >= 0) {
            const u32x4* q = reinterpret_cast<const u32x4*>(
                xrow[t] + sb * KQ_SB + (h == 0 ? xoff0 : xoff1));
#pragma unroll
            for (int j = 0; j < 4; ++j) xf[j] = q[j];
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) xf[j] = u32x4{0, 0, 0, 0};
          }
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            floatx4 a = acc[c][t];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  wf[c][j], __builtin_bit_cast(bf16x8, xf[j]), a, 0, 0, 0);
            acc[c][t] = a;
          }
        }
      }
    }

    // fixed-order K reduction: ((w0 + w1) + w2) + ... by wave 0
    if (wave > 0) {
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int t = 0; t < MT; ++t)
          red[wave - 1][c * MT + t][lane] = acc[c][t];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (c0 + t * 16 >= n_e) continue;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          floatx4 a = acc[c][t];
#pragma unroll
          for (int w = 0; w < W - 1; ++w) {
            const floatx4 q = red[w][c * MT + t][lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] += q[r];
          }
          acc[c][t] = a;
        }
        // C/D: lane holds D[channel = hi*4 + r][pair = lo of tile t]
        const int p = pair[t];
        if (p < 0) continue;
        const int n = n0 + hi * 4;
        if constexpr (GATED) {
          u16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float g = acc[0][t][r];
            o[r] = f32_to_bf16(g / (1.f + __expf(-g)) * acc[CT - 1][t][r]);
          }
          *reinterpret_cast<u16x4*>(
              static_cast<uint16_t*>(dst) + (int64_t)p * N + n) = o;
        } else {
          const float s = topk_w[p];
          floatx4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = s * acc[0][t][r];
          *reinterpret_cast<floatx4*>(
              static_cast<float*>(dst) + (int64_t)p * N + n) = o;
        }
      }
    }
    __syncthreads();                             // red is reused by the next chunk
  }
}

int moe_kq_fmt(const std::string& fmt, const char* what) {
  TORCH_CHECK(fmt == "q4_k" || fmt == "q6_k", what, ": unknown format '", fmt,
              "' (expected q4_k or q6_k)");
  return fmt == "q4_k" ? 4 : 6;
}

void check_stack_plane(const torch::Tensor& t, const torch::Tensor& first,
                       const char* what, const char* name,
                       c10::ScalarType dtype, std::vector<int64_t> shape) {
  TORCH_CHECK(t.is_cuda(), what, ": ", name, " must be on GPU");
  TORCH_CHECK(t.device() == first.device(), what, ": ", name,
              " is on another device than the first plane");
  TORCH_CHECK(t.scalar_type() == dtype, what, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes().vec() == shape, what, ": ", name, " must be ",
              c10::IntArrayRef(shape), ", got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), what, ": ", name, " must be contiguous");
  TORCH_CHECK(aligned16(t), what, ": ", name, " must be 16-byte aligned");
}

// Contract of one expert stack's planes: returns E; sets rows and K.
int64_t check_stack_kq(const std::vector<torch::Tensor>& planes, int fmt,
                       const char* what, int64_t* rows_out, int64_t* K_out) {
  const size_t want = fmt == 4 ? 2 : 4;
  TORCH_CHECK(planes.size() == want, what, ": ", fmt == 4 ? "q4_k" : "q6_k",
              " takes ", want, " planes, got ", planes.size());
  const auto& q = planes[0];
  TORCH_CHECK(q.dim() == 3, what,
              ": the payload plane must be 3-D [E, rows, K/2]");
  const int64_t E = q.size(0), rows = q.size(1), K = q.size(2) * 2;
  TORCH_CHECK(K > 0 && K % KQ_SB == 0, what, ": K (", K,
              ") must be a positive multiple of 256");
  TORCH_CHECK(rows > 0 && rows % 16 == 0, what, ": rows (", rows,
              ") must be a positive multiple of 16");
  TORCH_CHECK(rows * K < (int64_t(1) << 31), what, ": expert too large");
  if (fmt == 4) {
    check_stack_plane(q, q, what, "qs", torch::kUInt8, {E, rows, K / 2});
    check_stack_plane(planes[1], q, what, "hdr", torch::kUInt8,
                      {E, rows, K / KQ_SB, 16});
  } else {
    check_stack_plane(q, q, what, "ql", torch::kUInt8, {E, rows, K / 2});
    check_stack_plane(planes[1], q, what, "qh", torch::kUInt8,
                      {E, rows, K / 4});
    check_stack_plane(planes[2], q, what, "sc", torch::kInt8,
                      {E, rows, K / 16});
    check_stack_plane(planes[3], q, what, "d", torch::kFloat16,
                      {E, rows, K / KQ_SB});
  }
  *rows_out = rows;
  *K_out = K;
  return E;
}

struct MoeKQArgs {
  void* dst;
  const uint16_t* src;
  const void* p[4];
  const float* tw;
  const int32_t* off;
  const int32_t* pairs;
  int P, N, K, E, k;
};

template <int FMT, bool GATED, int MT>
void launch_moe_gemm_kq(int waves, const MoeKQArgs& a) {
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid(a.N / 16, a.E);
#define MOE_KQ_LAUNCH(WV)                                                     \
  hipLaunchKernelGGL((moe_gemm_kq_kernel<FMT, GATED, MT, WV>), grid,          \
                     dim3(WV * WAVE), 0, stream, a.dst, a.src, a.p[0],        \
                     a.p[1], a.p[2], a.p[3], a.tw, a.off, a.pairs, a.P, a.N,  \
                     a.K, a.k)
  if constexpr (!GATED) {
    if (waves == 16) {
      MOE_KQ_LAUNCH(16);
      return;
    }
  }
  if (waves == 8) {
    MOE_KQ_LAUNCH(8);
    return;
  }
  MOE_KQ_LAUNCH(4);
#undef MOE_KQ_LAUNCH
}

template <int FMT, bool GATED>
void dispatch_mt_kq(int64_t T, int waves, const MoeKQArgs& a) {
  // n_e <= T, so T alone bounds the token tiles a chunk can fill
  if (T <= 16) return launch_moe_gemm_kq<FMT, GATED, 1>(waves, a);
  if (T <= 32) return launch_moe_gemm_kq<FMT, GATED, 2>(waves, a);
  launch_moe_gemm_kq<FMT, GATED, MOE_MAX_MT>(waves, a);
}

template <bool GATED>
void dispatch_moe_gemm_kq(int fmt, int64_t T, int waves, const MoeKQArgs& a) {
  if (fmt == 4)
    dispatch_mt_kq<4, GATED>(T, waves, a);
  else
    dispatch_mt_kq<6, GATED>(T, waves, a);
}

}  // namespace

int64_t moe_kq_waves(int64_t N, int64_t K, bool gated) {
  return moe_kq_waves_host(N, K, gated);
}

// act[P, I] = silu(x[p/k] @ dq(w13[e, :I])^T) * (x[p/k] @ dq(w13[e, I:])^T)
void moe_gemm_gated_kq(torch::Tensor act, torch::Tensor x,
                       std::vector<torch::Tensor> w13_planes,
                       std::string fmt_name, torch::Tensor expert_off,
                       torch::Tensor sorted_pairs, int64_t k) {
  const int fmt = moe_kq_fmt(fmt_name, "moe_gemm_gated_kq");
  int64_t rows = 0, H = 0;
  const int64_t E = check_stack_kq(w13_planes, fmt, "moe_gemm_gated_kq: w13",
                                   &rows, &H);
  const auto& like = w13_planes[0];
  TORCH_CHECK(x.dim() == 2 && act.dim() == 2,
              "moe_gemm_gated_kq: x and act must be 2-D");
  const int64_t I = rows / 2;
  const int64_t T = x.size(0), P = T * k;
  check_ek(E, k);
  check_tensor(x, like, torch::kBFloat16, "moe_gemm_gated_kq: x");
  check_tensor(act, like, torch::kBFloat16, "moe_gemm_gated_kq: act");
  TORCH_CHECK(I > 0 && I % 16 == 0 && rows == 2 * I,
              "moe_gemm_gated_kq: w13 must have 2I rows with I (", I,
              ") a positive multiple of 16");
  TORCH_CHECK(x.size(1) == H, "moe_gemm_gated_kq: x must be [T, H], H = ", H);
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_gemm_gated_kq: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(P < (int64_t(1) << 31), "moe_gemm_gated_kq: too many pairs");
  check_lists(expert_off, sorted_pairs, like, E, P);
  if (T == 0) return;
  MoeKQArgs a{};
  a.dst = act.data_ptr();
  a.src = (const uint16_t*)x.data_ptr();
  for (size_t i = 0; i < w13_planes.size(); ++i)
    a.p[i] = w13_planes[i].data_ptr();
  a.off = (const int32_t*)expert_off.data_ptr();
  a.pairs = (const int32_t*)sorted_pairs.data_ptr();
  a.P = (int)P, a.N = (int)I, a.K = (int)H, a.E = (int)E, a.k = (int)k;
  dispatch_moe_gemm_kq<true>(fmt, T, moe_kq_waves_host(I, H, true), a);
}

// ypair[P, H] (fp32) = topk_w[p] * (act[p] @ dq(w2[e])^T)
void moe_gemm_down_kq(torch::Tensor ypair, torch::Tensor act,
                      std::vector<torch::Tensor> w2_planes,
                      std::string fmt_name, torch::Tensor topk_w,
                      torch::Tensor expert_off, torch::Tensor sorted_pairs) {
  const int fmt = moe_kq_fmt(fmt_name, "moe_gemm_down_kq");
  int64_t H = 0, I = 0;
  const int64_t E = check_stack_kq(w2_planes, fmt, "moe_gemm_down_kq: w2",
                                   &H, &I);
  const auto& like = w2_planes[0];
  TORCH_CHECK(act.dim() == 2 && ypair.dim() == 2 && topk_w.dim() == 2,
              "moe_gemm_down_kq: act, ypair and topk_w must be 2-D");
  const int64_t T = topk_w.size(0), k = topk_w.size(1), P = T * k;
  check_ek(E, k);
  check_tensor(act, like, torch::kBFloat16, "moe_gemm_down_kq: act");
  check_tensor(ypair, like, torch::kFloat32, "moe_gemm_down_kq: ypair");
  check_tensor(topk_w, like, torch::kFloat32, "moe_gemm_down_kq: topk_w");
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_gemm_down_kq: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(ypair.size(0) == P && ypair.size(1) == H,
              "moe_gemm_down_kq: ypair must be [T*k, H] = [", P, ", ", H, "]");
  TORCH_CHECK(P < (int64_t(1) << 31), "moe_gemm_down_kq: too many pairs");
  check_lists(expert_off, sorted_pairs, like, E, P);
  if (T == 0) return;
  MoeKQArgs a{};
  a.dst = ypair.data_ptr();
  a.src = (const uint16_t*)act.data_ptr();
  for (size_t i = 0; i < w2_planes.size(); ++i)
    a.p[i] = w2_planes[i].data_ptr();
  a.tw = (const float*)topk_w.data_ptr();
  a.off = (const int32_t*)expert_off.data_ptr();
  a.pairs = (const int32_t*)sorted_pairs.data_ptr();
  a.P = (int)P, a.N = (int)H, a.K = (int)I, a.E = (int)E, a.k = (int)k;
  dispatch_moe_gemm_kq<false>(fmt, T, moe_kq_waves_host(H, I, false), a);
}
