// Weight-only quantized GEMM for ggml K-quant weights, Q4_K / Q6_K (gfx950).
//
//   out[:, col_off : col_off+N] (bf16, row stride ldo)
//       = x[M,K] (bf16) @ dequant(W)^T (+ bias[col_off : col_off+N])
//
// A fused projection whose parts have different types (a Q4_K_M file's
// qkv_proj is Q4_K, Q4_K, Q6_K) is one launch per part, each writing its
// own columns of the shared output.
//
// Device layout: the super-block's fields as planes, byte for byte as in the
// file (256 elements along K per super-block, see docs/KERNELS.md):
//   q4_k : qs  uint8 [N, K/2]         128 nibble bytes per super-block
//          hdr uint8 [N, K/256, 16]   d fp16, dmin fp16, scales[12]
//   q6_k : ql  uint8 [N, K/2]         low nibbles, 128 bytes per super-block
//          qh  uint8 [N, K/4]         high 2 bits, 64 bytes
//          sc  int8  [N, K/16]        16 sub-block scales
//          d   fp16  [N, K/256]
//
// gemm_kq_kernel<FMT, MT, W>, M <= 16*MT <= 32, has gemm_wq.hip's structure:
//   * mfma_f32_16x16x32_bf16 with the WEIGHTS as the row (A) operand. A wave
//     step is one super-block = 8 MFMAs. Lane (lo = lane&15, hi = lane>>4)
//     owns 64 elements of channel row `lo`, loaded straight to registers:
//       Q4_K: sub-blocks 2hi and 2hi+1 = the 32 payload bytes at qs + 32*hi.
//             MFMA j < 4 takes the low nibbles of bytes 8j..8j+7, MFMA
//             j >= 4 the high nibbles of bytes 8(j-4)..; element i of MFMA j
//             in lane group hi is K index 64*hi + 8j + i of the super-block,
//             so the x operand is ONE contiguous 128-byte run of a token row.
//       Q6_K: half h = hi>>1, groups p = hi&1 (low nibbles) and p+2 (high
//             nibbles) of the same 32 ql bytes at ql + 64h + 32p, with the
//             half's 32 qh bytes. MFMA j < 4 is K index 128h + 32p + 8j + i,
//             MFMA j >= 4 is 128h + 64 + 32p + 8(j-4) + i: two 64-byte runs.
//   * A workgroup is W waves that split K by super-block (wave w takes
//     w, w+W, ...), summed through LDS in the fixed order ((w0+w1)+w2)+...
//     No atomics, no cross-workgroup sum. W in {4, 8, 16} is a function of
//     the WEIGHT's shape alone (kq_waves), and MT only adds token columns,
//     so out[m, :] is the same bits for every M and every neighbour row.
//   * The one-tile kernels (MT = 1) fetch the next step's weight bytes
//     before they compute the current step; the two-tile kernels have no
//     registers left for that under the 16-wave bound of 128 VGPRs.
//   * A workgroup owns 16 channels; N % 16 == 0 and the grid is exactly
//     N/16, so every lane's channel row exists. A lane whose token row is
//     past M feeds zeros and its column is not stored.
//
// Rounding. Q4_K: y = (d*sc)*nib - dmin*m. d*sc and dmin*m are exact in
// fp32 (11 x 6 bits), (d*sc)*nib is exact (17 x 4 bits), so
// fma(nib, d*sc, -(dmin*m)) rounds the exact value once, like the reference's
// subtraction. Q6_K: y = (d*sc)*q with q = u - 32, u in [0, 64): d*sc is
// exact (11 x 8 bits), -32*(d*sc) is a power-of-two multiple, and
// fma(u, d*sc, -32*(d*sc)) rounds the exact (d*sc)*(u-32) once. The second
// rounding, fp32 -> bf16 (nearest even), is the same in both.
//
// dequant_kq_kernel<FMT>: bf16 [N,K] for the large-M path, 8 elements and
// one b128 store per thread, same arithmetic.
//
// The per-lane fetch, decode and fragment helpers (KQFetch, kq_decode,
// kq_frag, q4k_scale_min) live in kq_common.h, shared with moe_kq.hip.
#include "kq_common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <string>
#include <vector>

using namespace helix;

namespace {

constexpr int KQ_MAX_M = 32;

// K-split factor of a weight: enough waves to give every SIMD of the 256
// CUs about four, never more waves than half the super-blocks before the
// last doubling (every wave of the result has at least one when K/256 >= W).
// Depends on the weight's shape only, never on M.
int kq_waves_host(int64_t N, int64_t K) {
  int w = 4;
  while (w < 16 && (N / 16) * w < 4096 && K / KQ_SB >= 2 * w) w *= 2;
  return w;
}

template <int FMT, int MT, int J>
__device__ __forceinline__ void kq_mfma(const KQRaw<FMT>& raw,
                                        const u32x4 (&xf)[MT][8],
                                        floatx4 (&acc)[MT]) {
  const bf16x8 w = kq_frag<J>(raw);
#pragma unroll
  for (int t = 0; t < MT; ++t)
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        w, __builtin_bit_cast(bf16x8, xf[t][J]), acc[t], 0, 0, 0);
}

// p0..p3 are the format's planes in the order of the header comment.
template <int FMT, int MT, int KQ_WAVES>
__global__ __launch_bounds__(KQ_WAVES * WAVE) void gemm_kq_kernel(
    uint16_t* __restrict__ out, const uint16_t* __restrict__ x,
    const void* __restrict__ p0, const void* __restrict__ p1,
    const void* __restrict__ p2, const void* __restrict__ p3,
    const uint16_t* __restrict__ bias, int M, int K, int ldo, int col_off) {
  __shared__ floatx4 red[KQ_WAVES - 1][MT][WAVE];

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int lo = lane & 15, hi = lane >> 4;
  const int nsb = K / KQ_SB;
  const int64_t row = (int64_t)blockIdx.x * 16 + lo;   // < N: grid == N/16

  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0, 0, 0, 0};

  // x run(s) of the lane inside a super-block, in elements
  const int xoff0 = FMT == 4 ? 64 * hi : 128 * (hi >> 1) + 32 * (hi & 1);
  const int xoff1 = FMT == 4 ? xoff0 + 32 : xoff0 + 64;

  // One token tile leaves registers to fetch the next step's weight bytes
  // while this step computes; with two tiles (and 16 waves: 128 VGPRs) the
  // second x fragment set takes that room. Same arithmetic either way.
  constexpr bool PREFETCH = MT == 1;
  const int64_t blk0 = row * nsb;
  KQFetch<FMT> nxt;
  if (PREFETCH && wave < nsb)
    nxt = kq_fetch<FMT>(p0, p1, p2, p3, blk0 + wave, hi);

  for (int sb = wave; sb < nsb; sb += KQ_WAVES) {      // wave-uniform
    KQFetch<FMT> cur;
    if constexpr (PREFETCH) {
      cur = nxt;
      if (sb + KQ_WAVES < nsb)
        nxt = kq_fetch<FMT>(p0, p1, p2, p3, blk0 + sb + KQ_WAVES, hi);
    } else {
      cur = kq_fetch<FMT>(p0, p1, p2, p3, blk0 + sb, hi);
    }

    u32x4 xf[MT][8];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int tok = t * 16 + lo;
      if (tok < M) {
        const uint16_t* xr = x + (int64_t)tok * K + (int64_t)sb * KQ_SB;
        const u32x4* a = reinterpret_cast<const u32x4*>(xr + xoff0);
        const u32x4* b = reinterpret_cast<const u32x4*>(xr + xoff1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xf[t][j] = a[j];
          xf[t][4 + j] = b[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[t][j] = u32x4{0, 0, 0, 0};
      }
    }

    const KQRaw<FMT> raw = kq_decode(cur, hi);

    kq_mfma<FMT, MT, 0>(raw, xf, acc);
    kq_mfma<FMT, MT, 1>(raw, xf, acc);
    kq_mfma<FMT, MT, 2>(raw, xf, acc);
    kq_mfma<FMT, MT, 3>(raw, xf, acc);
    kq_mfma<FMT, MT, 4>(raw, xf, acc);
    kq_mfma<FMT, MT, 5>(raw, xf, acc);
    kq_mfma<FMT, MT, 6>(raw, xf, acc);
    kq_mfma<FMT, MT, 7>(raw, xf, acc);
  }

  // fixed-order K reduction: ((w0 + w1) + w2) + ... by wave 0
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) red[wave - 1][t][lane] = acc[t];
  }
  __syncthreads();
  if (wave != 0) return;

  // C/D: lane holds D[channel = hi*4 + r][token = lo]
  const int n = col_off + blockIdx.x * 16 + hi * 4;
  float b[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) {
    u16x4 bv = *reinterpret_cast<const u16x4*>(bias + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = bf16_to_f32(bv[r]);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    floatx4 a = acc[t];
#pragma unroll
    for (int w = 0; w < KQ_WAVES - 1; ++w) {
      const floatx4 p = red[w][t][lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] += p[r];
    }
    const int tok = t * 16 + lo;
    if (tok < M) {
      u16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(a[r] + b[r]);
      *reinterpret_cast<u16x4*>(out + (int64_t)tok * ldo + n) = o;
    }
  }
}

// One thread: elements [8*e8, 8*e8+8) of super-block `blk`.
template <int FMT>
__global__ __launch_bounds__(256) void dequant_kq_kernel(
    uint16_t* __restrict__ out, const void* __restrict__ p0,
    const void* __restrict__ p1, const void* __restrict__ p2,
    const void* __restrict__ p3, int64_t total8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total8) return;
  const int64_t blk = i >> 5;                   // 32 groups of 8 per block
  const int e8 = (int)(i & 31);
  const int l0 = (e8 & 3) * 8;                  // offset within the 32-run
  uint32_t a, b;
  float s, o;
  if constexpr (FMT == 4) {
    const int j = e8 >> 2;                      // sub-block
    const u32x2 v = *reinterpret_cast<const u32x2*>(
        (const uint8_t*)p0 + blk * 128 + 32 * (j >> 1) + l0);
    const u32x4 h = *reinterpret_cast<const u32x4*>(
        (const uint8_t*)p1 + blk * 16);
    const float d = half_bits_to_f32((uint16_t)(h[0] & 0xffffu));
    const float dmin = half_bits_to_f32((uint16_t)(h[0] >> 16));
    q4k_scale_min(h[1], h[2], h[3], j & 3, j >= 4, d, dmin, &s, &o);
    const int sh = 4 * (j & 1);
    a = (v[0] >> sh) & 0x0f0f0f0fu;
    b = (v[1] >> sh) & 0x0f0f0f0fu;
  } else {
    const int h = e8 >> 4, g = (e8 >> 2) & 3;
    const u32x2 vl = *reinterpret_cast<const u32x2*>(
        (const uint8_t*)p0 + blk * 128 + 64 * h + 32 * (g & 1) + l0);
    const u32x2 vh = *reinterpret_cast<const u32x2*>(
        (const uint8_t*)p1 + blk * 64 + 32 * h + l0);
    const int sc = ((const int8_t*)p2)[blk * 16 + 8 * h + 2 * g + (l0 >> 4)];
    const float d = half_bits_to_f32(((const uint16_t*)p3)[blk]);
    s = d * (float)sc;
    o = -32.f * s;
    const int shl = 4 * (g >> 1), shh = 2 * g;
    a = ((vl[0] >> shl) & 0x0f0f0f0fu) | (((vh[0] >> shh) & 0x03030303u) << 4);
    b = ((vl[1] >> shl) & 0x0f0f0f0fu) | (((vh[1] >> shh) & 0x03030303u) << 4);
  }
  const bf16x8 r = dq8(a, b, s, o);
  *reinterpret_cast<u32x4*>(out + i * 8) = __builtin_bit_cast(u32x4, r);
}

int kq_fmt(const std::string& fmt) {
  TORCH_CHECK(fmt == "q4_k" || fmt == "q6_k", "gemm_kq: unknown format '",
              fmt, "' (expected q4_k or q6_k)");
  return fmt == "q4_k" ? 4 : 6;
}

void check_plane(const torch::Tensor& t, const char* name,
                 torch::ScalarType dtype, std::vector<int64_t> shape,
                 const torch::Tensor& first) {
  TORCH_CHECK(t.is_cuda(), "gemm_kq: ", name, " must be on GPU");
  TORCH_CHECK(t.device() == first.device(), "gemm_kq: ", name,
              " is on another device than the first plane");
  TORCH_CHECK(t.scalar_type() == dtype, "gemm_kq: ", name, " must be ",
              dtype, ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes().vec() == shape, "gemm_kq: ", name, " must be ",
              c10::IntArrayRef(shape), ", got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), "gemm_kq: ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "gemm_kq: ", name, " must be 16-byte aligned");
}

// Shape / dtype / layout contract of a format's planes. Returns N; sets K.
int64_t check_kq_planes(const std::vector<torch::Tensor>& planes, int fmt,
                        int64_t* K_out) {
  const size_t want = fmt == 4 ? 2 : 4;
  TORCH_CHECK(planes.size() == want, "gemm_kq: ", fmt == 4 ? "q4_k" : "q6_k",
              " takes ", want, " planes, got ", planes.size());
  const auto& q = planes[0];
  TORCH_CHECK(q.dim() == 2, "gemm_kq: the payload plane must be 2-D");
  const int64_t N = q.size(0), K = q.size(1) * 2;
  TORCH_CHECK(K > 0 && K % KQ_SB == 0, "gemm_kq: K (", K,
              ") must be a positive multiple of 256");
  TORCH_CHECK(N > 0 && N % 16 == 0, "gemm_kq: N (", N,
              ") must be a positive multiple of 16");
  TORCH_CHECK(N < (int64_t(1) << 31) && K < (int64_t(1) << 31) &&
              N * K < (int64_t(1) << 40), "gemm_kq: weight too large");
  if (fmt == 4) {
    check_plane(q, "qs", torch::kUInt8, {N, K / 2}, q);
    check_plane(planes[1], "hdr", torch::kUInt8, {N, K / KQ_SB, 16}, q);
  } else {
    check_plane(q, "ql", torch::kUInt8, {N, K / 2}, q);
    check_plane(planes[1], "qh", torch::kUInt8, {N, K / 4}, q);
    check_plane(planes[2], "sc", torch::kInt8, {N, K / 16}, q);
    check_plane(planes[3], "d", torch::kFloat16, {N, K / KQ_SB}, q);
  }
  *K_out = K;
  return N;
}

struct KQArgs {
  uint16_t* out;
  const uint16_t* x;
  const void* p[4];
  const uint16_t* bias;
  int M, N, K, ldo, col_off;
};

template <int FMT, int MT, int W>
void launch_one(const KQArgs& a) {
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL((gemm_kq_kernel<FMT, MT, W>), dim3(a.N / 16),
                     dim3(W * WAVE), 0, stream, a.out, a.x, a.p[0], a.p[1],
                     a.p[2], a.p[3], a.bias, a.M, a.K, a.ldo, a.col_off);
}

template <int FMT, int MT>
void dispatch_waves(int waves, const KQArgs& a) {
  if (waves == 16) return launch_one<FMT, MT, 16>(a);
  if (waves == 8) return launch_one<FMT, MT, 8>(a);
  launch_one<FMT, MT, 4>(a);
}

template <int FMT>
void dispatch_mt(int waves, const KQArgs& a) {
  if (a.M <= 16) return dispatch_waves<FMT, 1>(waves, a);
  dispatch_waves<FMT, 2>(waves, a);
}

}  // namespace

int64_t kq_kernel_max_m() { return KQ_MAX_M; }

int64_t kq_waves(int64_t N, int64_t K) { return kq_waves_host(N, K); }

void gemm_kq(torch::Tensor out, int64_t col_off, torch::Tensor x,
             std::vector<torch::Tensor> planes,
             c10::optional<torch::Tensor> bias, std::string fmt_name) {
  const int fmt = kq_fmt(fmt_name);
  int64_t K = 0;
  const int64_t N = check_kq_planes(planes, fmt, &K);
  TORCH_CHECK(x.is_cuda() && out.is_cuda(), "gemm_kq: x/out must be on GPU");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              out.scalar_type() == torch::kBFloat16,
              "gemm_kq: x and out must be bf16");
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2, "gemm_kq: x/out must be 2-D");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous(),
              "gemm_kq: x and out must be contiguous");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= KQ_MAX_M, "gemm_kq: M (", M,
              ") must be in [1, ", KQ_MAX_M, "]");
  TORCH_CHECK(x.size(1) == K, "gemm_kq: x has K=", x.size(1),
              ", weight has K=", K);
  const int64_t ldo = out.size(1);
  TORCH_CHECK(col_off >= 0 && col_off % 4 == 0, "gemm_kq: col_off (",
              col_off, ") must be a non-negative multiple of 4");
  TORCH_CHECK(out.size(0) == M && ldo >= col_off + N && ldo % 4 == 0 &&
              ldo < (int64_t(1) << 31),
              "gemm_kq: out must be [M, ldo] with ldo % 4 == 0 and ldo >= "
              "col_off + N = ", col_off + N, ", got ", out.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "gemm_kq: x must be 16-byte and out 8-byte aligned");
  TORCH_CHECK(x.device() == planes[0].device() && x.device() == out.device(),
              "gemm_kq: device mismatch");
  KQArgs a{};
  if (bias.has_value()) {
    const auto& b = bias.value();
    TORCH_CHECK(b.is_cuda() && b.device() == x.device() &&
                b.scalar_type() == torch::kBFloat16 && b.dim() == 1 &&
                b.size(0) >= col_off + N && b.is_contiguous(),
                "gemm_kq: bias must be contiguous bf16 [>= col_off + N] on "
                "x's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(b.data_ptr()) % 8 == 0,
                "gemm_kq: bias must be 8-byte aligned");
    a.bias = (const uint16_t*)b.data_ptr();
  }
  a.out = (uint16_t*)out.data_ptr();
  a.x = (const uint16_t*)x.data_ptr();
  for (size_t i = 0; i < planes.size(); ++i) a.p[i] = planes[i].data_ptr();
  a.M = (int)M;
  a.N = (int)N;
  a.K = (int)K;
  a.ldo = (int)ldo;
  a.col_off = (int)col_off;
  const int waves = kq_waves_host(N, K);
  if (fmt == 4)
    dispatch_mt<4>(waves, a);
  else
    dispatch_mt<6>(waves, a);
}

void dequant_kq(torch::Tensor out, std::vector<torch::Tensor> planes,
                std::string fmt_name) {
  const int fmt = kq_fmt(fmt_name);
  int64_t K = 0;
  const int64_t N = check_kq_planes(planes, fmt, &K);
  TORCH_CHECK(out.is_cuda() && out.device() == planes[0].device() &&
              out.scalar_type() == torch::kBFloat16 && out.dim() == 2 &&
              out.size(0) == N && out.size(1) == K && out.is_contiguous(),
              "dequant_kq: out must be contiguous bf16 [N, K] on the planes' "
              "device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "dequant_kq: out must be 16-byte aligned");
  const int64_t total8 = N * K / 8;
  auto stream = at::hip::getCurrentHIPStream();
  const unsigned grid = (unsigned)((total8 + 255) / 256);
  const void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  for (size_t i = 0; i < planes.size(); ++i) p[i] = planes[i].data_ptr();
  if (fmt == 4)
    hipLaunchKernelGGL((dequant_kq_kernel<4>), dim3(grid), dim3(256), 0,
                       stream, (uint16_t*)out.data_ptr(), p[0], p[1], p[2],
                       p[3], total8);
  else
    hipLaunchKernelGGL((dequant_kq_kernel<6>), dim3(grid), dim3(256), 0,
                       stream, (uint16_t*)out.data_ptr(), p[0], p[1], p[2],
                       p[3], total8);
}
