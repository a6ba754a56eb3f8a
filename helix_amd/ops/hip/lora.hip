// Multi-LoRA batched shrink/expand (CDNA4). Every row of the batch names
// its own adapter slot, so the low-rank update is a gather-by-row GEMV
// pair rather than a library GEMM:
//
//   y[t, j]   = sum_k x[t,k] * A[slot[t], j, k]                    (fp32)
//   out[t, n] = bf16(out[t,n] + scale[s] * sum_j y[t, i(n)*R + j] * B[s,n,j])
//
// Both kernels are memory/latency-bound: wave64, 16-byte bf16 loads, fp32
// accumulate. Each y / out element is produced by exactly one wave / lane
// in a fixed order (no atomics, no cross-workgroup accumulation), so
// results are bit-reproducible between eager and hipGraph replays. Rows
// whose slot is outside [0, S) touch nothing: no A/B/y read, out untouched.
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

constexpr int SHRINK_THREADS = 256;                 // 4 waves
constexpr int SHRINK_ROWS_PER_WAVE = 2;
constexpr int SHRINK_CHUNK = (SHRINK_THREADS / WAVE) * SHRINK_ROWS_PER_WAVE;  // 8
constexpr int EXPAND_THREADS = 256;
constexpr int EXPAND_COLS = EXPAND_THREADS * 8;     // n columns per workgroup
constexpr int MAX_SLICES = 3;

struct SliceOffsets {
  int off[MAX_SLICES + 1];      // unused tail entries hold N
};

// grid (T, Rtot / 8). Each wave owns two rank rows of the token's adapter:
// lanes stride K with b128 loads of x and of both A rows, then a wave
// shuffle reduction; lane 0 stores.
__global__ void __launch_bounds__(SHRINK_THREADS)
lora_shrink_kernel(float* __restrict__ y, const uint16_t* __restrict__ x,
                   const uint16_t* __restrict__ A,
                   const int* __restrict__ slot, int K, int Rtot, int S) {
  const int t = blockIdx.x;
  const int s = slot[t];
  if (s < 0 || s >= S) return;                      // workgroup-uniform
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int j0 = blockIdx.y * SHRINK_CHUNK + wid * SHRINK_ROWS_PER_WAVE;
  const uint16_t* xr = x + (int64_t)t * K;
  const uint16_t* a0 = A + ((int64_t)s * Rtot + j0) * K;
  const uint16_t* a1 = a0 + K;
  float acc0 = 0.f, acc1 = 0.f;
  for (int k = lane * 8; k < K; k += WAVE * 8) {
    float xv[8], av[8], bv[8];
    load_bf16x8(xr + k, xv);
    load_bf16x8(a0 + k, av);
    load_bf16x8(a1 + k, bv);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc0 = fmaf(xv[i], av[i], acc0);
      acc1 = fmaf(xv[i], bv[i], acc1);
    }
  }
  acc0 = wave_reduce_sum(acc0);
  acc1 = wave_reduce_sum(acc1);
  if (lane == 0) {
    float* yr = y + (int64_t)t * Rtot + j0;
    yr[0] = acc0;
    yr[1] = acc1;
  }
}

// grid (T, ceil(N / 2048)). y[t, :] is staged in LDS; each lane owns 8
// consecutive output columns (one slice: boundaries are multiples of 8),
// reads their B rows (contiguous R bf16 each) as b128 and does the
// read-modify-write of out as one b128.
template <int R>
__global__ void __launch_bounds__(EXPAND_THREADS)
lora_expand_kernel(uint16_t* __restrict__ out, const float* __restrict__ y,
                   const uint16_t* __restrict__ B,
                   const int* __restrict__ slot,
                   const float* __restrict__ scale, SliceOffsets so,
                   int N, int Rtot, int S) {
  __shared__ float ys[MAX_SLICES * R];
  const int t = blockIdx.x;
  const int s = slot[t];
  if (s < 0 || s >= S) return;                      // workgroup-uniform
  for (int j = threadIdx.x; j < Rtot; j += EXPAND_THREADS)
    ys[j] = y[(int64_t)t * Rtot + j];
  __syncthreads();
  const int n0 = blockIdx.y * EXPAND_COLS + threadIdx.x * 8;
  if (n0 >= N) return;
  const int sl = (n0 >= so.off[1]) + (n0 >= so.off[2]);
  const float* yv = ys + sl * R;
  const float sc = scale[s];
  const uint16_t* br = B + ((int64_t)s * N + n0) * R;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < R; j += 8) {
      float bv[8];
      load_bf16x8(br + i * R + j, bv);
#pragma unroll
      for (int e = 0; e < 8; ++e) a = fmaf(yv[j + e], bv[e], a);
    }
    acc[i] = a;
  }
  uint16_t* op = out + (int64_t)t * N + n0;
  float ov[8];
  load_bf16x8(op, ov);
#pragma unroll
  for (int i = 0; i < 8; ++i) ov[i] = ov[i] + sc * acc[i];
  store_bf16x8(op, ov);
}

bool aligned16(const torch::Tensor& t) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
}

}  // namespace

void lora_shrink(torch::Tensor y, torch::Tensor x, torch::Tensor A,
                 torch::Tensor slot) {
  TORCH_CHECK(x.is_cuda() && A.is_cuda() && y.is_cuda() && slot.is_cuda(),
              "lora_shrink: all tensors must be on the GPU");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              A.scalar_type() == torch::kBFloat16,
              "lora_shrink: x and A must be bf16");
  TORCH_CHECK(y.scalar_type() == torch::kFloat32, "lora_shrink: y must be fp32");
  TORCH_CHECK(slot.scalar_type() == torch::kInt32,
              "lora_shrink: slot must be int32");
  TORCH_CHECK(x.is_contiguous() && A.is_contiguous() && y.is_contiguous() &&
              slot.is_contiguous(), "lora_shrink: tensors must be contiguous");
  TORCH_CHECK(x.dim() == 2 && A.dim() == 3 && y.dim() == 2 && slot.dim() == 1,
              "lora_shrink: expected x[T,K], A[S,Rtot,K], y[T,Rtot], slot[T]");
  const int64_t T = x.size(0), K = x.size(1);
  const int64_t S = A.size(0), Rtot = A.size(1);
  TORCH_CHECK(T >= 1, "lora_shrink: T must be >= 1");
  TORCH_CHECK(S >= 1 && S < (1 << 20), "lora_shrink: bad slot count ", S);
  TORCH_CHECK(A.size(2) == K, "lora_shrink: A K dim ", A.size(2), " != ", K);
  TORCH_CHECK(y.size(0) == T && y.size(1) == Rtot,
              "lora_shrink: y must be [T, Rtot]");
  TORCH_CHECK(slot.size(0) == T, "lora_shrink: slot must be [T]");
  TORCH_CHECK(K >= 8 && K % 8 == 0 && K < (1 << 30),
              "lora_shrink: K must be a multiple of 8, got ", K);
  TORCH_CHECK(Rtot % 8 == 0 && Rtot >= 8 && Rtot <= MAX_SLICES * 64,
              "lora_shrink: Rtot must be n_slices * Rmax, got ", Rtot);
  TORCH_CHECK(T < (1LL << 31), "lora_shrink: T too large");
  TORCH_CHECK(aligned16(x) && aligned16(A),
              "lora_shrink: x and A must be 16-byte aligned");
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid((unsigned)T, (unsigned)(Rtot / SHRINK_CHUNK));
  hipLaunchKernelGGL(lora_shrink_kernel, grid, dim3(SHRINK_THREADS), 0, stream,
                     (float*)y.data_ptr(), (const uint16_t*)x.data_ptr(),
                     (const uint16_t*)A.data_ptr(),
                     (const int*)slot.data_ptr(), (int)K, (int)Rtot, (int)S);
}

void lora_expand(torch::Tensor out, torch::Tensor y, torch::Tensor B,
                 torch::Tensor slot, torch::Tensor scale,
                 std::vector<int64_t> n_off) {
  TORCH_CHECK(out.is_cuda() && y.is_cuda() && B.is_cuda() && slot.is_cuda() &&
              scale.is_cuda(), "lora_expand: all tensors must be on the GPU");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 &&
              B.scalar_type() == torch::kBFloat16,
              "lora_expand: out and B must be bf16");
  TORCH_CHECK(y.scalar_type() == torch::kFloat32 &&
              scale.scalar_type() == torch::kFloat32,
              "lora_expand: y and scale must be fp32");
  TORCH_CHECK(slot.scalar_type() == torch::kInt32,
              "lora_expand: slot must be int32");
  TORCH_CHECK(out.is_contiguous() && y.is_contiguous() && B.is_contiguous() &&
              slot.is_contiguous() && scale.is_contiguous(),
              "lora_expand: tensors must be contiguous");
  TORCH_CHECK(out.dim() == 2 && y.dim() == 2 && B.dim() == 3 &&
              slot.dim() == 1 && scale.dim() == 1,
              "lora_expand: expected out[T,N], y[T,Rtot], B[S,N,Rmax], "
              "slot[T], scale[S]");
  const int64_t T = out.size(0), N = out.size(1);
  const int64_t S = B.size(0), Rmax = B.size(2), Rtot = y.size(1);
  const int64_t n_slices = (int64_t)n_off.size() - 1;
  TORCH_CHECK(T >= 1 && T < (1LL << 31), "lora_expand: bad T ", T);
  TORCH_CHECK(S >= 1 && S < (1 << 20), "lora_expand: bad slot count ", S);
  TORCH_CHECK(N >= 8 && N % 8 == 0 && N < (1 << 30),
              "lora_expand: N must be a multiple of 8, got ", N);
  TORCH_CHECK(Rmax == 8 || Rmax == 16 || Rmax == 32 || Rmax == 64,
              "lora_expand: Rmax must be 8, 16, 32 or 64, got ", Rmax);
  TORCH_CHECK(n_slices >= 1 && n_slices <= MAX_SLICES,
              "lora_expand: n_off must describe 1..3 slices");
  TORCH_CHECK(Rtot == n_slices * Rmax, "lora_expand: y width ", Rtot,
              " != n_slices * Rmax = ", n_slices * Rmax);
  TORCH_CHECK(B.size(1) == N, "lora_expand: B N dim ", B.size(1), " != ", N);
  TORCH_CHECK(y.size(0) == T && slot.size(0) == T && scale.size(0) == S,
              "lora_expand: y/slot/scale shapes inconsistent");
  TORCH_CHECK(n_off.front() == 0 && n_off.back() == N,
              "lora_expand: n_off must run from 0 to N");
  SliceOffsets so;
  for (int i = 0; i <= MAX_SLICES; ++i) so.off[i] = (int)N;
  for (int64_t i = 0; i <= n_slices; ++i) {
    TORCH_CHECK(n_off[i] % 8 == 0, "lora_expand: slice boundary ", n_off[i],
                " is not a multiple of 8");
    TORCH_CHECK(i == 0 || n_off[i] >= n_off[i - 1],
                "lora_expand: n_off must be non-decreasing");
    so.off[i] = (int)n_off[i];
  }
  TORCH_CHECK(aligned16(out) && aligned16(B),
              "lora_expand: out and B must be 16-byte aligned");
  auto stream = at::hip::getCurrentHIPStream();
  dim3 grid((unsigned)T, (unsigned)((N + EXPAND_COLS - 1) / EXPAND_COLS));
#define LAUNCH_EXPAND(R)                                                      \
  hipLaunchKernelGGL(lora_expand_kernel<R>, grid, dim3(EXPAND_THREADS), 0,    \
                     stream, (uint16_t*)out.data_ptr(),                       \
                     (const float*)y.data_ptr(),                              \
                     (const uint16_t*)B.data_ptr(),                           \
                     (const int*)slot.data_ptr(),                             \
                     (const float*)scale.data_ptr(), so, (int)N, (int)Rtot,   \
                     (int)S)
  switch (Rmax) {
    case 8: LAUNCH_EXPAND(8); break;
    case 16: LAUNCH_EXPAND(16); break;
    case 32: LAUNCH_EXPAND(32); break;
    default: LAUNCH_EXPAND(64); break;
  }
#undef LAUNCH_EXPAND
}
