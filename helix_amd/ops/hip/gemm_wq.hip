// Weight-only quantized GEMM for ggml Q4_0 / Q8_0 weights (gfx950).
//
//   out[M,N] (bf16) = x[M,K] (bf16) @ dequant(W)^T (+ bias[N])
//
// Device layout (two planes per weight, see docs/KERNELS.md):
//   qs : Q4_0 uint8 [N, K/2]  /  Q8_0 int8 [N, K]   -- the payload bytes of
//        ggml block b of row n at qs[n][b*16 .. b*16+16) resp. [b*32 .. +32)
//   d  : fp16 [N, K/32]                              -- one scale per block
//
// gemm_wq_kernel<BITS, MT, CT, W>, M <= 16*MT <= 64:
//   * mfma_f32_16x16x32_bf16 with the WEIGHTS as the row (A) operand and the
//     tokens as the column (B) operand. Lane (lo = lane&15, hi = lane>>4)
//     owns one whole 32-element block `kb + hi` of channel row `lo`: one b128
//     (Q4_0) or two b128 (Q8_0) plus the fp16 scale, straight to registers.
//     It dequantizes to bf16 in registers and feeds four consecutive MFMAs
//     with values [8j, 8j+8) of the block. MFMA j therefore sees the K index
//     (kb+hi)*32 + 8j + i in slot (hi, i); the x operand uses the same
//     permutation, which makes its load 64 contiguous bytes of a token row.
//   * A workgroup is W waves that split K: wave w takes the 128-element steps
//     w, w+W, w+2W, ...  The partial tiles are summed through LDS in the
//     fixed order ((w0 + w1) + w2) + ... No atomics, no cross-workgroup sum.
//     W is 4, 8 or 16 and is a function of the WEIGHT's shape (N, K) alone
//     (wq_waves below): a narrow, deep weight such as llama's down_proj has
//     too few 16-channel workgroups to fill the chip unless K is split more.
//   * A wave owns CT channel tiles (16*CT channels) and MT token tiles; one x
//     fragment set is reused by the CT channel tiles, one dequantized weight
//     fragment by the MT token tiles. CT only regroups channels into
//     workgroups and MT only adds columns, so neither changes the order in
//     which any out[m, n] is accumulated: out[m, :] is the same bits for
//     every M and every neighbour row (the K split never looks at M).
//   * x is read with plain global loads, not staged in LDS: it is at most
//     64 rows and L2-resident, and staging it would put a barrier into every
//     K step of a loop that otherwise has none.
//
// dequant_wq_kernel<BITS>: bf16 [N,K] for the large-M path, 8 elements and
// one b128 store per thread, with the same d*q -> bf16 rounding.
//
// d*(nib-8) is computed as fma(nib, d, -8d): nib*d is exact in fp32 (4 x 11
// bits), -8d is a power-of-two multiple, and the sum d*(nib-8) is
// representable, so the fma returns it exactly; the only rounding is the
// final fp32 -> bf16 (nearest even). Q8_0 uses q = (byte ^ 0x80) - 128 the
// same way.
#include "dequant_common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

constexpr int WQ_MAX_M = 64;

// K-split factor (waves per workgroup) of a weight: enough waves to give
// every SIMD of the 256 CUs about four, never fewer than two K steps per
// wave. Depends on the weight's shape only, never on M.
int wq_waves(int64_t N, int64_t K) {
  int w = 4;
  while (w < 16 && (N / 16) * w < 4096 && K / 128 >= 4 * w) w *= 2;
  return w;
}

// half_bits_to_f32, pack_bf16x2 and dq8 (8 bytes -> 8 bf16 of
// fma(byte, d, off)) live in dequant_common.h, shared with gemm_kq.hip;
// WQRaw, wq_load and wq_frag too, shared with moe_wq.hip.

template <int BITS, int MT, int CT, int WQ_WAVES>
__global__ __launch_bounds__(WQ_WAVES * WAVE) void gemm_wq_kernel(
    uint16_t* __restrict__ out, const uint16_t* __restrict__ x,
    const uint8_t* __restrict__ qs, const uint16_t* __restrict__ ds,
    const uint16_t* __restrict__ bias, int M, int N, int K) {
  __shared__ floatx4 red[WQ_WAVES - 1][CT * MT][WAVE];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lo = lane & 15, hi = lane >> 4;
  const int nblk = K / 32;
  const int n_base = blockIdx.x * (16 * CT);

  floatx4 acc[CT][MT];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[c][t] = floatx4{0, 0, 0, 0};

  for (int kb0 = wave * 4; kb0 < nblk; kb0 += 4 * WQ_WAVES) {
    const int kb = kb0 + hi;
    const bool kvalid = kb < nblk;

    // x fragments: 64 contiguous bytes of token row t*16+lo
    u32x4 xf[MT][4];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int tok = t * 16 + lo;
      if (kvalid && tok < M) {
        const u32x4* p = reinterpret_cast<const u32x4*>(
            x + (int64_t)tok * K + (int64_t)kb * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[t][j] = p[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[t][j] = u32x4{0, 0, 0, 0};
      }
    }

    WQRaw<BITS> raw[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int n0 = n_base + c * 16;            // wave-uniform
      raw[c] = wq_load<BITS>(qs, ds, (int64_t)(n0 + lo), kb, nblk,
                             kvalid && n0 < N);
    }

#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const bf16x8 w0 = wq_frag<BITS, 0>(raw[c]);
      const bf16x8 w1 = wq_frag<BITS, 1>(raw[c]);
      const bf16x8 w2 = wq_frag<BITS, 2>(raw[c]);
      const bf16x8 w3 = wq_frag<BITS, 3>(raw[c]);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        floatx4 a = acc[c][t];
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            w0, __builtin_bit_cast(bf16x8, xf[t][0]), a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            w1, __builtin_bit_cast(bf16x8, xf[t][1]), a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            w2, __builtin_bit_cast(bf16x8, xf[t][2]), a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            w3, __builtin_bit_cast(bf16x8, xf[t][3]), a, 0, 0, 0);
        acc[c][t] = a;
      }
    }
  }

  // fixed-order K reduction: ((w0 + w1) + w2) + ... by wave 0
  if (wave > 0) {
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int t = 0; t < MT; ++t) red[wave - 1][c * MT + t][lane] = acc[c][t];
  }
  __syncthreads();
  if (wave != 0) return;

#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int n0 = n_base + c * 16;
    if (n0 >= N) continue;
    // C/D: lane holds D[channel = hi*4 + r][token = lo]
    const int n = n0 + hi * 4;
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias != nullptr) {
      u16x4 bv = *reinterpret_cast<const u16x4*>(bias + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) b[r] = bf16_to_f32(bv[r]);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      floatx4 a = acc[c][t];
#pragma unroll
      for (int w = 0; w < WQ_WAVES - 1; ++w) {
        const floatx4 p = red[w][c * MT + t][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] += p[r];
      }
      const int tok = t * 16 + lo;
      if (tok < M) {
        u16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(a[r] + b[r]);
        *reinterpret_cast<u16x4*>(out + (int64_t)tok * N + n) = o;
      }
    }
  }
}

template <int BITS>
__global__ __launch_bounds__(256) void dequant_wq_kernel(
    uint16_t* __restrict__ out, const uint8_t* __restrict__ qs,
    const uint16_t* __restrict__ ds, int64_t total8, int K) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total8) return;
  const int k8 = K / 8;
  const int64_t n = i / k8;
  const int g = (int)(i - n * k8);               // group of 8 within the row
  const int kb = g >> 2, j = g & 3;
  const int nblk = K / 32;
  const float d = half_bits_to_f32(ds[n * nblk + kb]);
  uint32_t a, b;
  float off;
  if constexpr (BITS == 4) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(
        qs + (n * nblk + kb) * 16 + (j & 1) * 8);
    const int sh = (j >> 1) * 4;
    a = (v[0] >> sh) & 0x0f0f0f0fu;
    b = (v[1] >> sh) & 0x0f0f0f0fu;
    off = -8.f * d;
  } else {
    const u32x2 v = *reinterpret_cast<const u32x2*>(
        qs + (n * nblk + kb) * 32 + j * 8);
    a = v[0] ^ 0x80808080u;
    b = v[1] ^ 0x80808080u;
    off = -128.f * d;
  }
  const bf16x8 r = dq8(a, b, d, off);
  *reinterpret_cast<u32x4*>(out + n * K + (int64_t)g * 8) =
      __builtin_bit_cast(u32x4, r);
}

// Shape / dtype / layout contract of a (qs, d) pair. Returns N; sets K.
int64_t check_planes(const torch::Tensor& qs, const torch::Tensor& d,
                     int64_t bits, int64_t* K_out) {
  TORCH_CHECK(bits == 4 || bits == 8, "gemm_wq: bits must be 4 or 8");
  TORCH_CHECK(qs.is_cuda() && d.is_cuda(), "gemm_wq: planes must be on GPU");
  TORCH_CHECK(qs.dim() == 2 && d.dim() == 2, "gemm_wq: planes must be 2-D");
  TORCH_CHECK(qs.is_contiguous(), "gemm_wq: qs must be contiguous");
  TORCH_CHECK(d.is_contiguous(), "gemm_wq: d must be contiguous");
  TORCH_CHECK(d.scalar_type() == torch::kFloat16, "gemm_wq: d must be fp16");
  if (bits == 4) {
    TORCH_CHECK(qs.scalar_type() == torch::kUInt8,
                "gemm_wq: Q4_0 qs must be uint8");
  } else {
    TORCH_CHECK(qs.scalar_type() == torch::kInt8,
                "gemm_wq: Q8_0 qs must be int8");
  }
  const int64_t N = qs.size(0);
  const int64_t K = bits == 4 ? qs.size(1) * 2 : qs.size(1);
  TORCH_CHECK(K > 0 && K % 32 == 0, "gemm_wq: K (", K,
              ") must be a positive multiple of 32");
  TORCH_CHECK(N > 0 && N % 16 == 0, "gemm_wq: N (", N,
              ") must be a positive multiple of 16");
  TORCH_CHECK(d.size(0) == N && d.size(1) == K / 32,
              "gemm_wq: d must be [N, K/32] = [", N, ", ", K / 32, "]");
  TORCH_CHECK(N < (int64_t(1) << 31) && K < (int64_t(1) << 31) &&
              N * K < (int64_t(1) << 40), "gemm_wq: weight too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qs.data_ptr()) % 16 == 0,
              "gemm_wq: qs must be 16-byte aligned");
  *K_out = K;
  return N;
}

template <int BITS, int MT, int CT, int W>
void launch_one(torch::Tensor& out, const torch::Tensor& x,
                const torch::Tensor& qs, const torch::Tensor& d,
                const uint16_t* bias, int M, int N, int K) {
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = cdiv(N, 16 * CT);
  hipLaunchKernelGGL((gemm_wq_kernel<BITS, MT, CT, W>), dim3(grid),
                     dim3(W * WAVE), 0, stream,
                     (uint16_t*)out.data_ptr(), (const uint16_t*)x.data_ptr(),
                     (const uint8_t*)qs.data_ptr(),
                     (const uint16_t*)d.data_ptr(), bias, M, N, K);
}

// More than 4 waves only come with CT == 1 (the host picks CT > 1 only for
// weights wide enough to stay at 4 waves), which bounds the reduction buffer
// at 15 x 4 KiB.
template <int BITS, int MT, int CT>
void launch_gemm_wq(int waves, torch::Tensor& out, const torch::Tensor& x,
                    const torch::Tensor& qs, const torch::Tensor& d,
                    const uint16_t* bias, int M, int N, int K) {
  if constexpr (CT == 1) {
    if (waves == 16)
      return launch_one<BITS, MT, 1, 16>(out, x, qs, d, bias, M, N, K);
    if (waves == 8)
      return launch_one<BITS, MT, 1, 8>(out, x, qs, d, bias, M, N, K);
  }
  launch_one<BITS, MT, CT, 4>(out, x, qs, d, bias, M, N, K);
}

template <int BITS, int MT>
void dispatch_ct(int waves, int ct, torch::Tensor& out, const torch::Tensor& x,
                 const torch::Tensor& qs, const torch::Tensor& d,
                 const uint16_t* bias, int M, int N, int K) {
  if constexpr (MT >= 4) {
    if (ct == 4) return launch_gemm_wq<BITS, MT, 4>(waves, out, x, qs, d, bias, M, N, K);
  }
  if constexpr (MT >= 2) {
    if (ct >= 2) return launch_gemm_wq<BITS, MT, 2>(waves, out, x, qs, d, bias, M, N, K);
  }
  launch_gemm_wq<BITS, MT, 1>(waves, out, x, qs, d, bias, M, N, K);
}

template <int BITS>
void dispatch_mt(int waves, int ct, torch::Tensor& out, const torch::Tensor& x,
                 const torch::Tensor& qs, const torch::Tensor& d,
                 const uint16_t* bias, int M, int N, int K) {
  if (M <= 16) return dispatch_ct<BITS, 1>(waves, ct, out, x, qs, d, bias, M, N, K);
  if (M <= 32) return dispatch_ct<BITS, 2>(waves, ct, out, x, qs, d, bias, M, N, K);
  dispatch_ct<BITS, 4>(waves, ct, out, x, qs, d, bias, M, N, K);
}

}  // namespace

int64_t wq_kernel_max_m() { return WQ_MAX_M; }

void gemm_wq(torch::Tensor out, torch::Tensor x, torch::Tensor qs,
             torch::Tensor d, c10::optional<torch::Tensor> bias,
             int64_t bits) {
  int64_t K64 = 0;
  const int64_t N = check_planes(qs, d, bits, &K64);
  TORCH_CHECK(x.is_cuda() && out.is_cuda(), "gemm_wq: x/out must be on GPU");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16,
              "gemm_wq: x and out must be bf16");
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2, "gemm_wq: x/out must be 2-D");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous(),
              "gemm_wq: x and out must be contiguous");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= WQ_MAX_M, "gemm_wq: M (", M,
              ") must be in [1, ", WQ_MAX_M, "]");
  TORCH_CHECK(x.size(1) == K64, "gemm_wq: x has K=", x.size(1),
              ", weight has K=", K64);
  TORCH_CHECK(out.size(0) == M && out.size(1) == N,
              "gemm_wq: out must be [M, N]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "gemm_wq: x must be 16-byte and out 8-byte aligned");
  TORCH_CHECK(x.device() == qs.device() && x.device() == d.device() &&
              x.device() == out.device(), "gemm_wq: device mismatch");
  const uint16_t* bptr = nullptr;
  if (bias.has_value()) {
    const auto& b = bias.value();
    TORCH_CHECK(b.is_cuda() && b.device() == x.device() &&
                b.scalar_type() == torch::kBFloat16 && b.dim() == 1 &&
                b.size(0) == N && b.is_contiguous(),
                "gemm_wq: bias must be contiguous bf16 [N] on x's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(b.data_ptr()) % 8 == 0,
                "gemm_wq: bias must be 8-byte aligned");
    bptr = (const uint16_t*)b.data_ptr();
  }
  // Channel tiles per wave: as many as the token tiles (so x fragments are
  // reused), but never so many that the grid drops under one workgroup per
  // CU. Regroups channels only; results do not depend on it.
  const int waves = wq_waves(N, K64);
  int ct = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  while (ct > 1 && (waves > 4 || N / (16 * ct) < 256)) ct >>= 1;
  if (bits == 4)
    dispatch_mt<4>(waves, ct, out, x, qs, d, bptr, (int)M, (int)N, (int)K64);
  else
    dispatch_mt<8>(waves, ct, out, x, qs, d, bptr, (int)M, (int)N, (int)K64);
}

void dequant_wq(torch::Tensor out, torch::Tensor qs, torch::Tensor d,
                int64_t bits) {
  int64_t K = 0;
  const int64_t N = check_planes(qs, d, bits, &K);
  TORCH_CHECK(out.is_cuda() && out.device() == qs.device() &&
              out.scalar_type() == torch::kBFloat16 && out.dim() == 2 &&
              out.size(0) == N && out.size(1) == K && out.is_contiguous(),
              "dequant_wq: out must be contiguous bf16 [N, K] on qs's device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "dequant_wq: out must be 16-byte aligned");
  const int64_t total8 = N * K / 8;
  auto stream = at::hip::getCurrentHIPStream();
  const unsigned grid = (unsigned)((total8 + 255) / 256);
  if (bits == 4)
    hipLaunchKernelGGL((dequant_wq_kernel<4>), dim3(grid), dim3(256), 0,
                       stream, (uint16_t*)out.data_ptr(),
                       (const uint8_t*)qs.data_ptr(),
                       (const uint16_t*)d.data_ptr(), total8, (int)K);
  else
    hipLaunchKernelGGL((dequant_wq_kernel<8>), dim3(grid), dim3(256), 0,
                       stream, (uint16_t*)out.data_ptr(),
                       (const uint8_t*)qs.data_ptr(),
                       (const uint16_t*)d.data_ptr(), total8, (int)K);
}
