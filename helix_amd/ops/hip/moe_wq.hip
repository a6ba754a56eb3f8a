// Routed expert GEMMs over ggml Q4_0 / Q8_0 expert weights (gfx950).
//
// moe_gemm_wq_kernel<BITS, GATED, MT, W> is moe.hip's moe_gemm_kernel with
// its weight operand replaced by gemm_wq.hip's: the expert stack stays
// quantised in two planes and is dequantised in registers.
//
// Planes of one expert stack (rows = 2I, K = H for w13; rows = H, K = I
// for w2; the expert is the slowest dimension, gate rows [:I], up [I:]):
//   qs : Q4_0 uint8 [E, rows, K/2]  /  Q8_0 int8 [E, rows, K]
//   d  : fp16 [E, rows, K/32]
// i.e. the payload bytes and scales of ggml's blocks, unchanged and in
// order, as docs/KERNELS.md defines them for gemm_wq.
//
// Unchanged from moe_gemm_kernel: grid (channel tiles, E) with a
// workgroup-uniform return on an empty list; chunks of 16*MT pairs whose
// pair ids and gathered source rows are loaded once per chunk; the
// wave-uniform tile skip; W waves splitting K in 128-element steps, summed
// through LDS as ((w0 + w1) + w2) + ...; W = moe_waves(N, K, gated) and MT
// from T alone; both epilogues.
//
// New: lane (lo, hi) loads one b128 (Q4_0) or two (Q8_0) plus the fp16
// scale of block kb+hi of channel row lo of expert e (wq_load), and
// dequantises it with fma(nib, d, -8d) / fma(byte^0x80, d, -128d) and one
// rounding to bf16 (wq_frag / dq8) into the four MFMA fragments. The
// fragments are computed once per K step and reused by the chunk's MT token
// tiles; the gated kernel keeps its gate and its up tile's. No LDS in the
// K loop.
//
// No atomics, no accumulation across workgroups; a pair's bits do not
// depend on T, on its place in its list or on its tile's neighbours.
#include "dequant_common.h"
#include "moe_common.h"
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

template <int BITS, bool GATED, int MT, int W>
__global__ __launch_bounds__(W * WAVE) void moe_gemm_wq_kernel(
    void* __restrict__ dst,                  // GATED: bf16 act[P, N]; else fp32 ypair[P, N]
    const uint16_t* __restrict__ src,        // GATED: x[T, K]; else act[P, K]
    const uint8_t* __restrict__ qs,          // [E, GATED ? 2N : N, K/2 or K]
    const uint16_t* __restrict__ ds,         // [E, GATED ? 2N : N, K/32] fp16
    const float* __restrict__ topk_w,        // [P] (!GATED)
    const int32_t* __restrict__ expert_off,  // [E + 1]
    const int32_t* __restrict__ sorted_pairs,  // [P]
    int P, int N, int K, int k) {
  constexpr int CT = GATED ? 2 : 1;
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
  const int nblk = K / 32;
  const int n0 = blockIdx.x * 16;
  const int rows = CT * N;                       // weight rows per expert
  int64_t wrow[CT];                              // row index, expert included
#pragma unroll
  for (int c = 0; c < CT; ++c) wrow[c] = (int64_t)e * rows + c * N + n0 + lo;

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

    for (int kb0 = wave * 4; kb0 < nblk; kb0 += 4 * W) {
      const int kb = kb0 + hi;
      const bool kvalid = kb < nblk;

      WQRaw<BITS> raw[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c)
        raw[c] = wq_load<BITS>(qs, ds, wrow[c], kb, nblk, kvalid);

      // dequantised once per K step, reused by the MT token tiles
      bf16x8 wf[CT][4];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        wf[c][0] = wq_frag<BITS, 0>(raw[c]);
        wf[c][1] = wq_frag<BITS, 1>(raw[c]);
        wf[c][2] = wq_frag<BITS, 2>(raw[c]);
        wf[c][3] = wq_frag<BITS, 3>(raw[c]);
      }

#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (c0 + t * 16 >= n_e) continue;        // wave-uniform tile skip
        u32x4 xf[4];
        if (kvalid && pair[t] >= 0) {
          const u32x4* q = reinterpret_cast<const u32x4*>(xrow[t] + kb * 32);
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

// Contract of one expert stack's (qs, d) pair: returns E; sets rows and K.
int64_t check_stack(const torch::Tensor& qs, const torch::Tensor& d,
                    int64_t bits, const char* what, int64_t* rows_out,
                    int64_t* K_out) {
  TORCH_CHECK(bits == 4 || bits == 8, what, ": bits must be 4 or 8, got ",
              bits);
  TORCH_CHECK(qs.is_cuda(), what, ": qs must be on GPU");
  TORCH_CHECK(qs.dim() == 3 && d.dim() == 3, what,
              ": qs and d must be 3-D [E, rows, ...]");
  check_tensor(qs, qs, bits == 4 ? torch::kUInt8 : torch::kInt8, what);
  check_tensor(d, qs, torch::kFloat16, what);
  const int64_t E = qs.size(0), rows = qs.size(1);
  const int64_t K = bits == 4 ? qs.size(2) * 2 : qs.size(2);
  TORCH_CHECK(K > 0 && K % 32 == 0, what, ": K (", K,
              ") must be a positive multiple of 32");
  TORCH_CHECK(d.size(0) == E && d.size(1) == rows && d.size(2) == K / 32,
              what, ": d must be [E, rows, K/32] = [", E, ", ", rows, ", ",
              K / 32, "]");
  TORCH_CHECK(rows * K < (int64_t(1) << 31), what, ": expert too large");
  *rows_out = rows;
  *K_out = K;
  return E;
}

template <int BITS, bool GATED, int MT>
void launch_moe_gemm_wq(int waves, void* dst, const torch::Tensor& src,
                        const torch::Tensor& qs, const torch::Tensor& d,
                        const float* tw, const torch::Tensor& expert_off,
                        const torch::Tensor& sorted_pairs, int P, int N, int K,
                        int E, int k) {
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid(N / 16, E);
#define MOE_WQ_LAUNCH(WV)                                                     \
  hipLaunchKernelGGL((moe_gemm_wq_kernel<BITS, GATED, MT, WV>), grid,         \
                     dim3(WV * WAVE), 0, stream, dst,                         \
                     (const uint16_t*)src.data_ptr(),                         \
                     (const uint8_t*)qs.data_ptr(),                           \
                     (const uint16_t*)d.data_ptr(), tw,                       \
                     (const int32_t*)expert_off.data_ptr(),                   \
                     (const int32_t*)sorted_pairs.data_ptr(), P, N, K, k)
  if constexpr (!GATED) {
    if (waves == 16) {
      MOE_WQ_LAUNCH(16);
      return;
    }
  }
  if (waves == 8) {
    MOE_WQ_LAUNCH(8);
    return;
  }
  MOE_WQ_LAUNCH(4);
#undef MOE_WQ_LAUNCH
}

template <int BITS, bool GATED>
void dispatch_mt_wq(int64_t T, int waves, void* dst, const torch::Tensor& src,
                    const torch::Tensor& qs, const torch::Tensor& d,
                    const float* tw, const torch::Tensor& expert_off,
                    const torch::Tensor& sorted_pairs, int P, int N, int K,
                    int E, int k) {
  // n_e <= T, so T alone bounds the token tiles a chunk can fill
  if (T <= 16)
    return launch_moe_gemm_wq<BITS, GATED, 1>(waves, dst, src, qs, d, tw,
                                              expert_off, sorted_pairs, P, N,
                                              K, E, k);
  if (T <= 32)
    return launch_moe_gemm_wq<BITS, GATED, 2>(waves, dst, src, qs, d, tw,
                                              expert_off, sorted_pairs, P, N,
                                              K, E, k);
  launch_moe_gemm_wq<BITS, GATED, MOE_MAX_MT>(waves, dst, src, qs, d, tw,
                                              expert_off, sorted_pairs, P, N,
                                              K, E, k);
}

template <bool GATED>
void dispatch_moe_gemm_wq(int64_t bits, int64_t T, int waves, void* dst,
                          const torch::Tensor& src, const torch::Tensor& qs,
                          const torch::Tensor& d, const float* tw,
                          const torch::Tensor& expert_off,
                          const torch::Tensor& sorted_pairs, int P, int N,
                          int K, int E, int k) {
  if (bits == 4)
    dispatch_mt_wq<4, GATED>(T, waves, dst, src, qs, d, tw, expert_off,
                             sorted_pairs, P, N, K, E, k);
  else
    dispatch_mt_wq<8, GATED>(T, waves, dst, src, qs, d, tw, expert_off,
                             sorted_pairs, P, N, K, E, k);
}

}  // namespace

// act[P, I] = silu(x[p/k] @ dq(w13[e, :I])^T) * (x[p/k] @ dq(w13[e, I:])^T)
void moe_gemm_gated_wq(torch::Tensor act, torch::Tensor x,
                       torch::Tensor w13_qs, torch::Tensor w13_d, int64_t bits,
                       torch::Tensor expert_off, torch::Tensor sorted_pairs,
                       int64_t k) {
  int64_t rows = 0, H = 0;
  const int64_t E = check_stack(w13_qs, w13_d, bits, "moe_gemm_gated_wq: w13",
                                &rows, &H);
  TORCH_CHECK(x.dim() == 2 && act.dim() == 2,
              "moe_gemm_gated_wq: x and act must be 2-D");
  const int64_t I = rows / 2;
  const int64_t T = x.size(0), P = T * k;
  check_ek(E, k);
  check_tensor(x, w13_qs, torch::kBFloat16, "moe_gemm_gated_wq: x");
  check_tensor(act, w13_qs, torch::kBFloat16, "moe_gemm_gated_wq: act");
  TORCH_CHECK(I > 0 && I % 16 == 0 && rows == 2 * I,
              "moe_gemm_gated_wq: w13 must have 2I rows with I (", I,
              ") a positive multiple of 16");
  TORCH_CHECK(x.size(1) == H, "moe_gemm_gated_wq: x must be [T, H], H = ", H);
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_gemm_gated_wq: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(P < (int64_t(1) << 31), "moe_gemm_gated_wq: too many pairs");
  check_lists(expert_off, sorted_pairs, w13_qs, E, P);
  if (T == 0) return;
  dispatch_moe_gemm_wq<true>(bits, T, moe_waves_host(I, H, true),
                             act.data_ptr(), x, w13_qs, w13_d, nullptr,
                             expert_off, sorted_pairs, (int)P, (int)I, (int)H,
                             (int)E, (int)k);
}

// ypair[P, H] (fp32) = topk_w[p] * (act[p] @ dq(w2[e])^T)
void moe_gemm_down_wq(torch::Tensor ypair, torch::Tensor act,
                      torch::Tensor w2_qs, torch::Tensor w2_d, int64_t bits,
                      torch::Tensor topk_w, torch::Tensor expert_off,
                      torch::Tensor sorted_pairs) {
  int64_t H = 0, I = 0;
  const int64_t E = check_stack(w2_qs, w2_d, bits, "moe_gemm_down_wq: w2",
                                &H, &I);
  TORCH_CHECK(act.dim() == 2 && ypair.dim() == 2 && topk_w.dim() == 2,
              "moe_gemm_down_wq: act, ypair and topk_w must be 2-D");
  const int64_t T = topk_w.size(0), k = topk_w.size(1), P = T * k;
  check_ek(E, k);
  check_tensor(act, w2_qs, torch::kBFloat16, "moe_gemm_down_wq: act");
  check_tensor(ypair, w2_qs, torch::kFloat32, "moe_gemm_down_wq: ypair");
  check_tensor(topk_w, w2_qs, torch::kFloat32, "moe_gemm_down_wq: topk_w");
  TORCH_CHECK(H > 0 && H % 16 == 0, "moe_gemm_down_wq: H (", H,
              ") must be a positive multiple of 16");
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_gemm_down_wq: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(ypair.size(0) == P && ypair.size(1) == H,
              "moe_gemm_down_wq: ypair must be [T*k, H] = [", P, ", ", H, "]");
  TORCH_CHECK(P < (int64_t(1) << 31), "moe_gemm_down_wq: too many pairs");
  check_lists(expert_off, sorted_pairs, w2_qs, E, P);
  if (T == 0) return;
  dispatch_moe_gemm_wq<false>(bits, T, moe_waves_host(H, I, false),
                              ypair.data_ptr(), act, w2_qs, w2_d,
                              (const float*)topk_w.data_ptr(), expert_off,
                              sorted_pairs, (int)P, (int)H, (int)I, (int)E,
                              (int)k);
}
