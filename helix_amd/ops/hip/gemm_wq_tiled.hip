// Weight-only quantized GEMM for ggml Q4_0 / Q8_0 weights at M in the tens
// to hundreds (gfx950): the LDS-tiled, split-K sibling of gemm_wq.hip.
//
//   out[M,N] (bf16) = x[M,K] (bf16) @ dequant(W)^T (+ bias[N])
//
// Same two planes as gemm_wq.hip (qs, fp16 d [N, K/32]) and the same
// dequantization (wq_load / wq_frag of dequant_common.h: fma(q, d, off) and
// one bf16 rounding, bit-identical to dequant_wq).
//
// gemm_wq_tiled_kernel<BITS, MT>, 4 waves,
// grid (ceil(N/64), ceil(M/(16*MT)), KS):
//   * Weights never touch LDS. Wave w owns the 16-channel tile
//     64*blockIdx.x + 16*w; lane (lo = lane&15, hi = lane>>4) loads block
//     kb+hi of channel row lo straight to registers, dequantizes it into the
//     four A fragments of mfma_f32_16x16x32_bf16 and reuses them over the MT
//     token tiles of the workgroup. The raw bytes of the next K step (5 or 9
//     VGPRs) are fetched before the MFMAs of the current one.
//   * The x tile [16*MT][128] of a K step goes through LDS once per
//     workgroup and is shared by the four waves, so x is read from L2 once
//     per 64 channels instead of once per 16. Threads stage it as 16-byte
//     vectors through registers (loaded before the MFMAs of the current
//     step, written after them) into the other half of a double buffer: one
//     barrier per step. The B operand of MFMA j is one ds_read_b128 of row
//     16t+lo at bytes 64*hi + 16*j, the K permutation of the weight
//     fragments. Rows are padded from 256 to 272 bytes so that the 16 rows
//     of a token tile start 4 banks apart instead of on one bank.
//     Rows at or past M and vectors at or past K are zero-filled: an
//     invalid weight lane is +0, and 0 * garbage may be NaN.
//   * K is split over blockIdx.z = s, which takes the 128-element steps
//     [s*q, min((s+1)*q, steps)), q = ceil(steps/KS). KS = wq_tiled_splits
//     (N, K) is a function of the weight's shape alone. KS == 1 adds the
//     bias in fp32 and stores bf16. KS > 1 stores the fp32 partial tile to
//     ws[s][m][n], each element written once and without atomics;
//     wq_splitk_reduce_kernel then sums the splits in ascending s, adds the
//     bias and rounds once.
//   * MT, grid.x and grid.y only regroup columns and channels, and neither
//     the split nor the order of the steps inside one looks at M: out[m, :]
//     is the same bits for every M and every set of neighbour rows.
#include "dequant_common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace helix {
// gemm_wq.hip: shape / dtype / layout contract of a (qs, d) pair.
int64_t wq_check_planes(const torch::Tensor& qs, const torch::Tensor& d,
                        int64_t bits, int64_t* K_out);
}  // namespace helix

namespace {

// The kernels of this file are compiled without packed fp32 arithmetic
// (v_pk_fma_f32 and kin, which the compiler otherwise forms from the pairs
// of dq8 and the epilogue): scalar fp32 ops only.
#if defined(__HIP_DEVICE_COMPILE__)
#define NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define NO_PK_F32
#endif

constexpr int TILED_WAVES = 4;
constexpr int TILED_THREADS = TILED_WAVES * WAVE;
constexpr int TILED_N = 16 * TILED_WAVES;        // channels per workgroup
constexpr int STEP_K = 128;                      // elements per K step
constexpr int ROW_BYTES = STEP_K * 2 + 16;       // padded LDS row

// One 16-byte vector per thread and 16 rows: thread (r = tid>>4, c = tid&15)
// stages bytes [16c, 16c+16) of rows r, r+16, ... of the tile.
template <int MT>
__device__ __forceinline__ void x_fetch(u32x4 (&v)[MT],
                                        const uint16_t* __restrict__ x,
                                        int m0, int k0, int M, int K) {
  const int r = threadIdx.x >> 4;
  const int k = k0 + (threadIdx.x & 15) * 8;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + 16 * i + r;
    if (m < M && k < K)
      v[i] = *reinterpret_cast<const u32x4*>(x + (int64_t)m * K + k);
    else
      v[i] = u32x4{0, 0, 0, 0};
  }
}

template <int MT>
__device__ __forceinline__ void x_stage(uint8_t* buf, const u32x4 (&v)[MT]) {
  const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < MT; ++i)
    *reinterpret_cast<u32x4*>(buf + (16 * i + r) * ROW_BYTES + 16 * c) = v[i];
}

template <int BITS, int MT>
__global__ NO_PK_F32 __launch_bounds__(TILED_THREADS) void
gemm_wq_tiled_kernel(
    uint16_t* __restrict__ out, float* __restrict__ ws,
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ qs,
    const uint16_t* __restrict__ ds, const uint16_t* __restrict__ bias,
    int M, int N, int K, int steps_per_split) {
  constexpr int BUF_BYTES = 16 * MT * ROW_BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t xs[2 * BUF_BYTES];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lo = lane & 15, hi = lane >> 4;
  const int nblk = K / 32;
  const int steps = (K + STEP_K - 1) / STEP_K;
  const int n0 = blockIdx.x * TILED_N + wave * 16;     // wave-uniform
  const bool wave_on = n0 < N;
  const int m0 = blockIdx.y * (16 * MT);
  const int s_begin = blockIdx.z * steps_per_split;
  const int s_end = min(s_begin + steps_per_split, steps);

  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0, 0, 0, 0};

  if (s_begin < s_end) {
    u32x4 xv[MT];
    x_fetch<MT>(xv, x, m0, s_begin * STEP_K, M, K);
    int kb = s_begin * 4 + hi;
    WQRaw<BITS> raw = wq_load<BITS>(qs, ds, (int64_t)(n0 + lo), kb, nblk,
                                    wave_on && kb < nblk);
    x_stage<MT>(xs, xv);
    __syncthreads();

    for (int s = s_begin; s < s_end; ++s) {
      const int cur = (s - s_begin) & 1;
      const bool more = s + 1 < s_end;                 // workgroup-uniform
      WQRaw<BITS> next = raw;
      if (more) {
        x_fetch<MT>(xv, x, m0, (s + 1) * STEP_K, M, K);
        kb = (s + 1) * 4 + hi;
        next = wq_load<BITS>(qs, ds, (int64_t)(n0 + lo), kb, nblk,
                             wave_on && kb < nblk);
      }
      if (wave_on) {
        const bf16x8 w0 = wq_frag<BITS, 0>(raw);
        const bf16x8 w1 = wq_frag<BITS, 1>(raw);
        const bf16x8 w2 = wq_frag<BITS, 2>(raw);
        const bf16x8 w3 = wq_frag<BITS, 3>(raw);
        const uint8_t* row = xs + cur * BUF_BYTES + lo * ROW_BYTES + 64 * hi;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const u32x4* p =
              reinterpret_cast<const u32x4*>(row + 16 * t * ROW_BYTES);
          floatx4 a = acc[t];
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              w0, __builtin_bit_cast(bf16x8, p[0]), a, 0, 0, 0);
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              w1, __builtin_bit_cast(bf16x8, p[1]), a, 0, 0, 0);
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              w2, __builtin_bit_cast(bf16x8, p[2]), a, 0, 0, 0);
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              w3, __builtin_bit_cast(bf16x8, p[3]), a, 0, 0, 0);
          acc[t] = a;
        }
      }
      if (more) x_stage<MT>(xs + (cur ^ 1) * BUF_BYTES, xv);
      __syncthreads();
      raw = next;
    }
  }

  if (!wave_on) return;
  // C/D: lane holds D[channel = hi*4 + r][token = lo]
  const int n = n0 + hi * 4;
  if (gridDim.z > 1) {
    float* part = ws + (int64_t)blockIdx.z * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int tok = m0 + t * 16 + lo;
      if (tok < M)
        *reinterpret_cast<floatx4*>(part + (int64_t)tok * N + n) = acc[t];
    }
    return;
  }
  float b[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) {
    const u16x4 bv = *reinterpret_cast<const u16x4*>(bias + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = bf16_to_f32(bv[r]);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int tok = m0 + t * 16 + lo;
    if (tok < M) {
      u16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(acc[t][r] + b[r]);
      *reinterpret_cast<u16x4*>(out + (int64_t)tok * N + n) = o;
    }
  }
}

// out[m][n] = bf16(sum_s ws[s][m][n] + bias[n]), s ascending; one thread owns
// four consecutive channels of one token.
__global__ NO_PK_F32 __launch_bounds__(256) void wq_splitk_reduce_kernel(
    uint16_t* __restrict__ out, const float* __restrict__ ws,
    const uint16_t* __restrict__ bias, int64_t total4, int64_t MN, int N,
    int KS) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int64_t e = i * 4;
  floatx4 a = *reinterpret_cast<const floatx4*>(ws + e);
  for (int s = 1; s < KS; ++s) {
    const floatx4 p = *reinterpret_cast<const floatx4*>(ws + s * MN + e);
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] += p[r];
  }
  if (bias != nullptr) {
    const u16x4 bv = *reinterpret_cast<const u16x4*>(bias + (int)(e % N));
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] += bf16_to_f32(bv[r]);
  }
  u16x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(a[r]);
  *reinterpret_cast<u16x4*>(out + e) = o;
}

template <int BITS, int MT>
void launch_tiled(uint16_t* out, float* ws, const torch::Tensor& x,
                  const torch::Tensor& qs, const torch::Tensor& d,
                  const uint16_t* bias, int M, int N, int K, int KS) {
  const int steps = cdiv(K, STEP_K);
  const dim3 grid(cdiv(N, TILED_N), cdiv(M, 16 * MT), KS);
  hipLaunchKernelGGL((gemm_wq_tiled_kernel<BITS, MT>), grid,
                     dim3(TILED_THREADS), 0, at::hip::getCurrentHIPStream(),
                     out, ws, (const uint16_t*)x.data_ptr(),
                     (const uint8_t*)qs.data_ptr(),
                     (const uint16_t*)d.data_ptr(), bias, M, N, K,
                     cdiv(steps, KS));
}

template <int BITS>
void dispatch_tiled(uint16_t* out, float* ws, const torch::Tensor& x,
                    const torch::Tensor& qs, const torch::Tensor& d,
                    const uint16_t* bias, int M, int N, int K, int KS) {
  if (M <= 32) return launch_tiled<BITS, 2>(out, ws, x, qs, d, bias, M, N, K, KS);
  if (M <= 64) return launch_tiled<BITS, 4>(out, ws, x, qs, d, bias, M, N, K, KS);
  launch_tiled<BITS, 8>(out, ws, x, qs, d, bias, M, N, K, KS);
}

}  // namespace

// K-split factor (grid.z) of a weight: double it while the 64-channel
// workgroups of one M tile leave CUs idle and every split keeps at least 16
// K steps. Depends on the weight's shape only, never on M.
int64_t wq_tiled_splits(int64_t N, int64_t K) {
  const int64_t groups = (N + TILED_N - 1) / TILED_N;
  const int64_t steps = (K + STEP_K - 1) / STEP_K;
  int64_t s = 1;
  while (s < 8 && groups * s < 256 && steps >= 16 * s) s *= 2;
  return s;
}

void gemm_wq_tiled(torch::Tensor out, torch::Tensor x, torch::Tensor qs,
                   torch::Tensor d, c10::optional<torch::Tensor> bias,
                   int64_t bits, c10::optional<torch::Tensor> ws) {
  int64_t K = 0;
  const int64_t N = wq_check_planes(qs, d, bits, &K);
  TORCH_CHECK(x.is_cuda() && out.is_cuda(),
              "gemm_wq_tiled: x/out must be on GPU");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16,
              "gemm_wq_tiled: x and out must be bf16");
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2,
              "gemm_wq_tiled: x/out must be 2-D");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous(),
              "gemm_wq_tiled: x and out must be contiguous");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1, "gemm_wq_tiled: M must be at least 1");
  const int mt = M <= 32 ? 2 : (M <= 64 ? 4 : 8);
  TORCH_CHECK((M + 16 * mt - 1) / (16 * mt) <= 65535, "gemm_wq_tiled: M (",
              M, ") needs more than 65535 row tiles");
  TORCH_CHECK(M * N < (int64_t(1) << 40), "gemm_wq_tiled: output too large");
  TORCH_CHECK(x.size(1) == K, "gemm_wq_tiled: x has K=", x.size(1),
              ", weight has K=", K);
  TORCH_CHECK(out.size(0) == M && out.size(1) == N,
              "gemm_wq_tiled: out must be [M, N]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "gemm_wq_tiled: x must be 16-byte and out 8-byte aligned");
  TORCH_CHECK(x.device() == qs.device() && x.device() == d.device() &&
              x.device() == out.device(), "gemm_wq_tiled: device mismatch");
  const uint16_t* bptr = nullptr;
  if (bias.has_value()) {
    const auto& b = bias.value();
    TORCH_CHECK(b.is_cuda() && b.device() == x.device() &&
                b.scalar_type() == torch::kBFloat16 && b.dim() == 1 &&
                b.size(0) == N && b.is_contiguous(),
                "gemm_wq_tiled: bias must be contiguous bf16 [N] on x's "
                "device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(b.data_ptr()) % 8 == 0,
                "gemm_wq_tiled: bias must be 8-byte aligned");
    bptr = (const uint16_t*)b.data_ptr();
  }
  const int KS = (int)wq_tiled_splits(N, K);
  float* wptr = nullptr;
  if (KS > 1) {
    TORCH_CHECK(ws.has_value(), "gemm_wq_tiled: a [", N, ", ", K,
                "] weight is split ", KS, " ways over K and needs ws");
    const auto& w = ws.value();
    TORCH_CHECK(w.is_cuda() && w.device() == x.device() &&
                w.scalar_type() == torch::kFloat32 && w.is_contiguous(),
                "gemm_wq_tiled: ws must be contiguous fp32 on x's device");
    TORCH_CHECK(w.numel() >= KS * M * N, "gemm_wq_tiled: ws has ", w.numel(),
                " elements, needs KS*M*N = ", KS * M * N);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
                "gemm_wq_tiled: ws must be 16-byte aligned");
    wptr = (float*)w.data_ptr();
  }
  uint16_t* optr = (uint16_t*)out.data_ptr();
  if (bits == 4)
    dispatch_tiled<4>(optr, wptr, x, qs, d, bptr, (int)M, (int)N, (int)K, KS);
  else
    dispatch_tiled<8>(optr, wptr, x, qs, d, bptr, (int)M, (int)N, (int)K, KS);
  if (KS > 1) {
    const int64_t total4 = M * N / 4;
    hipLaunchKernelGGL(wq_splitk_reduce_kernel,
                       dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0,
                       at::hip::getCurrentHIPStream(), optr,
                       (const float*)wptr, bptr, total4, M * N, (int)N, KS);
  }
}
