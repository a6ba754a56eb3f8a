// Weight-only quantized GEMM for ggml Q4_K / Q6_K weights at M in the tens
// to hundreds (gfx950): the LDS-tiled, split-K sibling of gemm_kq.hip.
//
//   out[:, col_off : col_off+N] (bf16, row stride ldo)
//       = x[M,K] (bf16) @ dequant(W)^T (+ bias[col_off : col_off+N])
//
// Same planes, lane mapping and dequantization as gemm_kq.hip (kq_fetch /
// kq_decode / kq_frag of kq_common.h, arithmetic untouched: bit-identical to
// dequant_kq). One launch per segment of a fused projection, each writing
// its own columns of the shared output.
//
// gemm_kq_tiled_kernel<FMT, MT>, 4 waves, grid (N/64, ceil(M/(16*MT)), KS):
//   * Weights never touch LDS. Wave w owns the 16-channel tile
//     64*blockIdx.x + 16*w (N % 64 == 0: every tile and every lane's channel
//     row exists). A K step is one 256-element super-block: lane (lo =
//     lane&15, hi = lane>>4) fetches its 64 elements of super-block sb of
//     channel row lo straight to registers, decodes them, builds the eight A
//     fragments of mfma_f32_16x16x32_bf16 and reuses them over the MT token
//     tiles of the workgroup. A step is two passes, fragments 0-3 over all
//     token tiles and then 4-7 (four live fragments instead of eight), so
//     every accumulator takes MFMAs 0..7 in order and the steps in ascending
//     order. The raw bytes of the next super-block (KQFetch, 12 or 19 VGPRs)
//     are fetched before the MFMAs of the current one.
//   * The x tile [16*MT][256] of a step goes through LDS once per workgroup
//     and is shared by the four waves, so x is read from L2 once per 64
//     channels instead of once per 16. Thread (r = tid>>5, c = tid&31) stages
//     bytes [16c, 16c+16) of rows r, r+8, ... as 16-byte vectors through
//     registers (loaded before the MFMAs of the current step, written after
//     them) into the other half of a double buffer: one barrier per step.
//     The B operand of MFMA j is one ds_read_b128 of row 16t+lo: for Q4_K at
//     element 64*hi + 8j, one 128-byte run; for Q6_K at 128*(hi>>1) +
//     32*(hi&1) + 8j for j < 4 and 64 elements further for j >= 4, two
//     64-byte runs (gemm_kq_kernel's xoff0 / xoff1).
//   * Row padding: 16 bytes, 512 -> 528 bytes = 132 dwords, the sibling's
//     choice. With a 512-byte stride the 16 rows `lo` of a token tile start
//     on one bank and a ds_read_b128 of one lane group is a 16-way conflict;
//     with 132 dwords row lo starts at bank 4*lo mod 64, so the 16 lanes of
//     a group cover the 64 banks exactly once for every hi and j (the run
//     offsets are multiples of 16 bytes, which only rotates the banks). 16
//     is the smallest pad that keeps the vectors 16-byte aligned; the
//     staging writes are 32 consecutive vectors of one row and need none.
//     Rows at or past M are zero-filled.
//   * K is split over blockIdx.z = s, which takes the super-blocks
//     [s*q, min((s+1)*q, nsb)), q = ceil(nsb/KS). KS = kq_tiled_splits(N, K)
//     is a function of the segment's shape alone. KS == 1 adds the bias in
//     fp32 and stores bf16. KS > 1 stores the fp32 partial tile to
//     ws[s][m][n], n local to the segment, each element written once and
//     without atomics; kq_splitk_reduce_kernel then sums the splits in
//     ascending s, adds the bias, rounds once and writes the segment's
//     columns of out.
//   * MT, grid.x and grid.y only regroup columns and channels, and neither
//     the split nor the order of the steps inside one looks at M: out[m, :]
//     is the same bits for every M and every set of neighbour rows.
//   * MT = 2 / 4 for M <= 32 / larger: 33 / 66 KiB of LDS, 4 / 2 workgroups
//     per CU. MT = 8 (132 KiB, one workgroup per CU, one wave per SIMD) was
//     measured against MT = 4 with two row tiles in grid.y at M = 96 and 128
//     and lost at every shape in both formats (profiles/r13_kq_tiled.md), so
//     it is not instantiated.
#include "kq_common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <string>
#include <vector>

using namespace helix;

namespace helix {
// gemm_kq.hip: shape / dtype / layout contract of a format's planes.
int64_t check_kq_planes(const std::vector<torch::Tensor>& planes, int fmt,
                        int64_t* K_out);
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
constexpr int ROW_BYTES = KQ_SB * 2 + 16;        // padded LDS row

// Token tiles per workgroup: a function of M only.
constexpr int kq_tiled_mt(int64_t M) { return M <= 32 ? 2 : 4; }

// One 16-byte vector per thread and 8 rows: thread (r = tid>>5, c = tid&31)
// stages bytes [16c, 16c+16) of rows r, r+8, ... of the tile.
template <int MT>
__device__ __forceinline__ void x_fetch(u32x4 (&v)[2 * MT],
                                        const uint16_t* __restrict__ x,
                                        int m0, int k0, int M, int K) {
  const int r = threadIdx.x >> 5;
  const int k = k0 + (threadIdx.x & 31) * 8;
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i) {
    const int m = m0 + 8 * i + r;
    if (m < M)
      v[i] = *reinterpret_cast<const u32x4*>(x + (int64_t)m * K + k);
    else
      v[i] = u32x4{0, 0, 0, 0};
  }
}

template <int MT>
__device__ __forceinline__ void x_stage(uint8_t* buf,
                                        const u32x4 (&v)[2 * MT]) {
  const int r = threadIdx.x >> 5, c = threadIdx.x & 31;
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i)
    *reinterpret_cast<u32x4*>(buf + (8 * i + r) * ROW_BYTES + 16 * c) = v[i];
}

// Fragments J0..J0+3 of the step over all token tiles; `run` is the lane's
// 64-byte x run of these fragments in row lo of token tile 0.
template <int FMT, int MT, int J0>
__device__ __forceinline__ void kq_pass(const KQRaw<FMT>& raw,
                                        const uint8_t* run,
                                        floatx4 (&acc)[MT]) {
  const bf16x8 w0 = kq_frag<J0>(raw);
  const bf16x8 w1 = kq_frag<J0 + 1>(raw);
  const bf16x8 w2 = kq_frag<J0 + 2>(raw);
  const bf16x8 w3 = kq_frag<J0 + 3>(raw);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const u32x4* p = reinterpret_cast<const u32x4*>(run + 16 * t * ROW_BYTES);
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

// p0..p3 are the format's planes in the order of gemm_kq.hip's header.
template <int FMT, int MT>
__global__ NO_PK_F32 __launch_bounds__(TILED_THREADS) void
gemm_kq_tiled_kernel(
    uint16_t* __restrict__ out, float* __restrict__ ws,
    const uint16_t* __restrict__ x, const void* __restrict__ p0,
    const void* __restrict__ p1, const void* __restrict__ p2,
    const void* __restrict__ p3, const uint16_t* __restrict__ bias,
    int M, int N, int K, int ldo, int col_off, int sb_per_split) {
  constexpr int BUF_BYTES = 16 * MT * ROW_BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t xs[2 * BUF_BYTES];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lo = lane & 15, hi = lane >> 4;
  const int nsb = K / KQ_SB;
  const int n0 = blockIdx.x * TILED_N + wave * 16;     // < N: N % 64 == 0
  const int m0 = blockIdx.y * (16 * MT);
  const int s_begin = blockIdx.z * sb_per_split;
  const int s_end = min(s_begin + sb_per_split, nsb);

  // byte offsets of the lane's x run(s) inside a padded row
  const int xoff0 =
      2 * (FMT == 4 ? 64 * hi : 128 * (hi >> 1) + 32 * (hi & 1));
  const int xoff1 = xoff0 + 2 * (FMT == 4 ? 32 : 64);

  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0, 0, 0, 0};

  if (s_begin < s_end) {
    const int64_t blk0 = (int64_t)(n0 + lo) * nsb;
    u32x4 xv[2 * MT];
    x_fetch<MT>(xv, x, m0, s_begin * KQ_SB, M, K);
    KQFetch<FMT> cur = kq_fetch<FMT>(p0, p1, p2, p3, blk0 + s_begin, hi);
    x_stage<MT>(xs, xv);
    __syncthreads();

    for (int s = s_begin; s < s_end; ++s) {
      const int buf = (s - s_begin) & 1;
      const bool more = s + 1 < s_end;                 // workgroup-uniform
      KQFetch<FMT> nxt = cur;
      if (more) {
        x_fetch<MT>(xv, x, m0, (s + 1) * KQ_SB, M, K);
        nxt = kq_fetch<FMT>(p0, p1, p2, p3, blk0 + s + 1, hi);
      }
      const KQRaw<FMT> raw = kq_decode(cur, hi);
      const uint8_t* row = xs + buf * BUF_BYTES + lo * ROW_BYTES;
      kq_pass<FMT, MT, 0>(raw, row + xoff0, acc);
      kq_pass<FMT, MT, 4>(raw, row + xoff1, acc);
      if (more) x_stage<MT>(xs + (buf ^ 1) * BUF_BYTES, xv);
      __syncthreads();
      cur = nxt;
    }
  }

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
    const u16x4 bv = *reinterpret_cast<const u16x4*>(bias + col_off + n);
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
      *reinterpret_cast<u16x4*>(out + (int64_t)tok * ldo + col_off + n) = o;
    }
  }
}

// out[m][col_off + n] = bf16(sum_s ws[s][m][n] + bias[col_off + n]), s
// ascending; one thread owns four consecutive channels of one token.
__global__ NO_PK_F32 __launch_bounds__(256) void kq_splitk_reduce_kernel(
    uint16_t* __restrict__ out, const float* __restrict__ ws,
    const uint16_t* __restrict__ bias, int64_t total4, int64_t MN, int N,
    int KS, int ldo, int col_off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int64_t e = i * 4;
  floatx4 a = *reinterpret_cast<const floatx4*>(ws + e);
  for (int s = 1; s < KS; ++s) {
    const floatx4 p = *reinterpret_cast<const floatx4*>(ws + s * MN + e);
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] += p[r];
  }
  const int64_t m = e / N;
  const int n = col_off + (int)(e - m * N);
  if (bias != nullptr) {
    const u16x4 bv = *reinterpret_cast<const u16x4*>(bias + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] += bf16_to_f32(bv[r]);
  }
  u16x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(a[r]);
  *reinterpret_cast<u16x4*>(out + m * ldo + n) = o;
}

struct KQTiledArgs {
  uint16_t* out;
  float* ws;
  const uint16_t* x;
  const void* p[4];
  const uint16_t* bias;
  int M, N, K, ldo, col_off, KS;
};

template <int FMT, int MT>
void launch_tiled(const KQTiledArgs& a) {
  const dim3 grid(a.N / TILED_N, cdiv(a.M, 16 * MT), a.KS);
  hipLaunchKernelGGL((gemm_kq_tiled_kernel<FMT, MT>), grid,
                     dim3(TILED_THREADS), 0, at::hip::getCurrentHIPStream(),
                     a.out, a.ws, a.x, a.p[0], a.p[1], a.p[2], a.p[3], a.bias,
                     a.M, a.N, a.K, a.ldo, a.col_off,
                     cdiv(a.K / KQ_SB, a.KS));
}

template <int FMT>
void dispatch_tiled(const KQTiledArgs& a) {
  if (kq_tiled_mt(a.M) == 2) return launch_tiled<FMT, 2>(a);
  launch_tiled<FMT, 4>(a);
}

}  // namespace

// K-split factor (grid.z) of a segment: double it while the 64-channel
// workgroups of one M tile leave CUs idle and every split keeps at least 8
// super-blocks. Depends on the segment's shape only, never on M.
int64_t kq_tiled_splits(int64_t N, int64_t K) {
  const int64_t groups = N / TILED_N;
  const int64_t nsb = K / KQ_SB;
  int64_t s = 1;
  while (s < 8 && groups * s < 256 && nsb >= 8 * s) s *= 2;
  return s;
}

void gemm_kq_tiled(torch::Tensor out, int64_t col_off, torch::Tensor x,
                   std::vector<torch::Tensor> planes,
                   c10::optional<torch::Tensor> bias, std::string fmt_name,
                   c10::optional<torch::Tensor> ws) {
  TORCH_CHECK(fmt_name == "q4_k" || fmt_name == "q6_k",
              "gemm_kq_tiled: unknown format '", fmt_name,
              "' (expected q4_k or q6_k)");
  const int fmt = fmt_name == "q4_k" ? 4 : 6;
  int64_t K = 0;
  const int64_t N = check_kq_planes(planes, fmt, &K);
  TORCH_CHECK(N % TILED_N == 0, "gemm_kq_tiled: N (", N,
              ") must be a multiple of 64");
  TORCH_CHECK(x.is_cuda() && out.is_cuda(),
              "gemm_kq_tiled: x/out must be on GPU");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16,
              "gemm_kq_tiled: x and out must be bf16");
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2,
              "gemm_kq_tiled: x/out must be 2-D");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous(),
              "gemm_kq_tiled: x and out must be contiguous");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1, "gemm_kq_tiled: M must be at least 1");
  const int mt = kq_tiled_mt(M);
  TORCH_CHECK((M + 16 * mt - 1) / (16 * mt) <= 65535, "gemm_kq_tiled: M (",
              M, ") needs more than 65535 row tiles");
  TORCH_CHECK(M * N < (int64_t(1) << 40), "gemm_kq_tiled: output too large");
  TORCH_CHECK(x.size(1) == K, "gemm_kq_tiled: x has K=", x.size(1),
              ", weight has K=", K);
  const int64_t ldo = out.size(1);
  TORCH_CHECK(col_off >= 0 && col_off % 4 == 0, "gemm_kq_tiled: col_off (",
              col_off, ") must be a non-negative multiple of 4");
  TORCH_CHECK(out.size(0) == M && ldo >= col_off + N && ldo % 4 == 0 &&
              ldo < (int64_t(1) << 31),
              "gemm_kq_tiled: out must be [M, ldo] with ldo % 4 == 0 and "
              "ldo >= col_off + N = ", col_off + N, ", got ", out.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "gemm_kq_tiled: x must be 16-byte and out 8-byte aligned");
  TORCH_CHECK(x.device() == planes[0].device() && x.device() == out.device(),
              "gemm_kq_tiled: device mismatch");
  KQTiledArgs a{};
  if (bias.has_value()) {
    const auto& b = bias.value();
    TORCH_CHECK(b.is_cuda() && b.device() == x.device() &&
                b.scalar_type() == torch::kBFloat16 && b.dim() == 1 &&
                b.size(0) >= col_off + N && b.is_contiguous(),
                "gemm_kq_tiled: bias must be contiguous bf16 [>= col_off + "
                "N] on x's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(b.data_ptr()) % 8 == 0,
                "gemm_kq_tiled: bias must be 8-byte aligned");
    a.bias = (const uint16_t*)b.data_ptr();
  }
  a.KS = (int)kq_tiled_splits(N, K);
  if (a.KS > 1) {
    TORCH_CHECK(ws.has_value(), "gemm_kq_tiled: a [", N, ", ", K,
                "] segment is split ", a.KS, " ways over K and needs ws");
    const auto& w = ws.value();
    TORCH_CHECK(w.is_cuda() && w.device() == x.device() &&
                w.scalar_type() == torch::kFloat32 && w.is_contiguous(),
                "gemm_kq_tiled: ws must be contiguous fp32 on x's device");
    TORCH_CHECK(w.numel() >= a.KS * M * N, "gemm_kq_tiled: ws has ",
                w.numel(), " elements, needs KS*M*N = ", a.KS * M * N);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
                "gemm_kq_tiled: ws must be 16-byte aligned");
    a.ws = (float*)w.data_ptr();
  }
  a.out = (uint16_t*)out.data_ptr();
  a.x = (const uint16_t*)x.data_ptr();
  for (size_t i = 0; i < planes.size(); ++i) a.p[i] = planes[i].data_ptr();
  a.M = (int)M;
  a.N = (int)N;
  a.K = (int)K;
  a.ldo = (int)ldo;
  a.col_off = (int)col_off;
  if (fmt == 4)
    dispatch_tiled<4>(a);
  else
    dispatch_tiled<6>(a);
  if (a.KS > 1) {
    const int64_t total4 = M * N / 4;
    hipLaunchKernelGGL(kq_splitk_reduce_kernel,
                       dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0,
                       at::hip::getCurrentHIPStream(), a.out,
                       (const float*)a.ws, a.bias, total4, M * N, (int)N,
                       a.KS, a.ldo, a.col_off);
  }
}
