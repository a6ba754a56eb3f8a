// Mixture-of-experts (Mixtral-style) routed expert kernels (gfx950).
//
//   T tokens, E experts (<= 256), k experts per token (<= 8), hidden H,
//   expert intermediate I; P = T*k pairs, pair p = t*k + j is slot j of
//   token t.
//
// moe_route_kernel: one wave per token. fp32 softmax over the E logits, the
//   k largest kept (ties to the LOWER expert index, slot j = j-th largest)
//   and renormalised to sum 1. No global scratch.
//
// moe_align_kernel: one workgroup. Per-expert counts in LDS, an exclusive
//   scan into expert_off[E+1], then every wave walks the pairs once per
//   expert it owns, 64 at a time: ballot(id == e) and a prefix popcount give
//   each pair its place, so every list is in ascending pair order with no
//   atomics on positions. Ids outside [0, E) belong to no list.
//
// moe_gemm_kernel<GATED, MT, W>: gemm_wq.hip's structure with bf16 weights,
//   an expert index on the grid and a gather on the token operand.
//   * grid = (channel tiles, E). Workgroup (n, e) reads its expert's list
//     length n_e and returns if it is 0, else walks the list in chunks of
//     16*MT pairs; the source-row index of each of the chunk's pairs is
//     loaded into a register once, before the K loop.
//   * mfma_f32_16x16x32_bf16, weights as the row (A) operand: lane (lo, hi)
//     loads the 64 contiguous bytes of channel row lo, K block kb+hi, of
//     expert e, straight to registers, and feeds four consecutive MFMAs
//     with values [8j, 8j+8) of the block. The token (B) operand uses the
//     same K permutation: 64 contiguous bytes of one gathered row.
//   * W waves split K (wave w takes the 128-element steps w, w+W, ...) and
//     are summed through LDS in the fixed order ((w0 + w1) + w2) + ...
//     W is a function of the weight's shape alone (moe_waves).
//   * GATED: weight w13[E, 2I, H]; the workgroup owns gate tile n and up
//     tile I+n, which share one x fragment set; source row x[p / k];
//     act[p, n] = bf16(silu(gate) * up), computed in fp32, rounded once.
//   * !GATED: weight w2[E, H, I]; source row act[p];
//     ypair[p, n] = topk_w[p] * acc in fp32.
//   * No atomics, no accumulation across workgroups. A pair's value does
//     not depend on T, on its place in the list or on its tile's other
//     columns: MT, the chunking and the grid only regroup MFMA columns, and
//     the K split never looks at them.
//
// moe_combine_kernel: out[t, :] = bf16(sum_j ypair[t*k + j, :]), ascending j,
//   fp32, one rounding; b128 loads, one lane per output element.
#include "moe_common.h"
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

// MOE_MAX_E, MOE_MAX_K, MOE_MAX_MT, moe_waves_host and the host checks
// (check_tensor, check_ek, check_lists) live in moe_common.h, shared with
// moe_wq.hip.
constexpr int ALIGN_THREADS = 1024;

// ---------------------------------------------------------------------------
// route
// ---------------------------------------------------------------------------
__device__ __forceinline__ float load_logit(const float* p) { return *p; }
__device__ __forceinline__ float load_logit(const uint16_t* p) {
  return bf16_to_f32(*p);
}

template <typename LT>
__global__ __launch_bounds__(256) void moe_route_kernel(
    int32_t* __restrict__ ids, float* __restrict__ wts,
    const LT* __restrict__ logits, int T, int E, int k) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int t = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  if (t >= T) return;                              // wave-uniform
  constexpr int PER = MOE_MAX_E / WAVE;            // experts per lane
  float v[PER];
  bool taken[PER];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = lane + i * WAVE;
    taken[i] = e >= E;
    v[i] = taken[i] ? -INFINITY : load_logit(logits + (int64_t)t * E + e);
    mx = fmaxf(mx, v[i]);
  }
  mx = wave_reduce_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (!taken[i]) sum += expf(v[i] - mx);
  sum = wave_reduce_sum(sum);

  float myw = 0.f;                                 // lane j keeps slot j
  int myid = 0;
  float ksum = 0.f;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = lane + i * WAVE;
      if (!taken[i] && (v[i] > bv || (v[i] == bv && e < bi))) {
        bv = v[i];
        bi = e;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, WAVE);
      const int oi = __shfl_xor(bi, off, WAVE);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if (lane + i * WAVE == bi) taken[i] = true;
    const float p = expf(bv - mx) / sum;
    ksum += p;
    if (lane == j) {
      myw = p;
      myid = bi;
    }
  }
  if (lane < k) {
    ids[(int64_t)t * k + lane] = myid;
    wts[(int64_t)t * k + lane] = myw / ksum;
  }
}

// ---------------------------------------------------------------------------
// align
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ALIGN_THREADS) void moe_align_kernel(
    int32_t* __restrict__ expert_off, int32_t* __restrict__ sorted_pairs,
    const int32_t* __restrict__ ids, int P, int E) {
  __shared__ int cnt[MOE_MAX_E];
  __shared__ int off[MOE_MAX_E + 1];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  if (tid < MOE_MAX_E) cnt[tid] = 0;
  __syncthreads();
  for (int p = tid; p < P; p += ALIGN_THREADS) {
    const int e = ids[p];
    if (e >= 0 && e < E) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  if (wave == 0) {
    // exclusive scan: lane owns experts 4*lane .. 4*lane+3
    int c[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane * 4 + i;
      c[i] = e < E ? cnt[e] : 0;
      s += c[i];
    }
    int incl = s;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int o = __shfl_up(incl, d, WAVE);
      if (lane >= d) incl += o;
    }
    int run = incl - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane * 4 + i;
      if (e < E) off[e] = run;
      run += c[i];
    }
    if (lane == WAVE - 1) off[E] = incl;         // number of listed pairs
  }
  __syncthreads();
  if (tid <= E) expert_off[tid] = off[tid];

  const uint64_t below = (uint64_t(1) << lane) - 1;
  for (int e = wave; e < E; e += ALIGN_THREADS / WAVE) {
    int base = off[e];
#pragma unroll 4
    for (int p0 = 0; p0 < P; p0 += WAVE) {
      const int p = p0 + lane;
      const bool hit = p < P && ids[p] == e;
      const uint64_t m = __ballot(hit);
      if (hit) sorted_pairs[base + __popcll(m & below)] = p;
      base += __popcll(m);
    }
  }
}

// ---------------------------------------------------------------------------
// routed expert GEMM
// ---------------------------------------------------------------------------
template <bool GATED, int MT, int W>
__global__ __launch_bounds__(W * WAVE) void moe_gemm_kernel(
    void* __restrict__ dst,                  // GATED: bf16 act[P, N]; else fp32 ypair[P, N]
    const uint16_t* __restrict__ src,        // GATED: x[T, K]; else act[P, K]
    const uint16_t* __restrict__ wgt,        // [E, GATED ? 2N : N, K]
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
  const uint16_t* wrow[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c)
    wrow[c] = wgt + ((int64_t)e * rows + c * N + n0 + lo) * K;

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

      u32x4 wf[CT][4];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (kvalid) {
          const u32x4* q = reinterpret_cast<const u32x4*>(wrow[c] + kb * 32);
#pragma unroll
          for (int j = 0; j < 4; ++j) wf[c][j] = q[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) wf[c][j] = u32x4{0, 0, 0, 0};
        }
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
                __builtin_bit_cast(bf16x8, wf[c][j]),
                __builtin_bit_cast(bf16x8, xf[j]), a, 0, 0, 0);
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

// ---------------------------------------------------------------------------
// combine
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_combine_kernel(
    uint16_t* __restrict__ out, const float* __restrict__ ypair,
    int64_t total8, int H, int k) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total8) return;
  const int h8 = H / 8;
  const int64_t t = i / h8;
  const int h = (int)(i - t * h8) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j) {
    const floatx4* q = reinterpret_cast<const floatx4*>(
        ypair + (t * k + j) * H + h);
    const floatx4 a = q[0], b = q[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[r] += a[r];
      s[4 + r] += b[r];
    }
  }
  store_bf16x8(out + t * H + h, s);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <bool GATED, int MT>
void launch_moe_gemm(int waves, void* dst, const torch::Tensor& src,
                     const torch::Tensor& wgt, const float* tw,
                     const torch::Tensor& expert_off,
                     const torch::Tensor& sorted_pairs, int P, int N, int K,
                     int E, int k) {
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid(N / 16, E);
#define MOE_LAUNCH(WV)                                                        \
  hipLaunchKernelGGL((moe_gemm_kernel<GATED, MT, WV>), grid, dim3(WV * WAVE), \
                     0, stream, dst, (const uint16_t*)src.data_ptr(),         \
                     (const uint16_t*)wgt.data_ptr(), tw,                     \
                     (const int32_t*)expert_off.data_ptr(),                   \
                     (const int32_t*)sorted_pairs.data_ptr(), P, N, K, k)
  if constexpr (!GATED) {
    if (waves == 16) {
      MOE_LAUNCH(16);
      return;
    }
  }
  if (waves == 8) {
    MOE_LAUNCH(8);
    return;
  }
  MOE_LAUNCH(4);
#undef MOE_LAUNCH
}

template <bool GATED>
void dispatch_moe_gemm(int64_t T, int waves, void* dst,
                       const torch::Tensor& src, const torch::Tensor& wgt,
                       const float* tw, const torch::Tensor& expert_off,
                       const torch::Tensor& sorted_pairs, int P, int N, int K,
                       int E, int k) {
  // n_e <= T, so T alone bounds the token tiles a chunk can fill
  if (T <= 16)
    return launch_moe_gemm<GATED, 1>(waves, dst, src, wgt, tw, expert_off,
                                     sorted_pairs, P, N, K, E, k);
  if (T <= 32)
    return launch_moe_gemm<GATED, 2>(waves, dst, src, wgt, tw, expert_off,
                                     sorted_pairs, P, N, K, E, k);
  launch_moe_gemm<GATED, MOE_MAX_MT>(waves, dst, src, wgt, tw, expert_off,
                                     sorted_pairs, P, N, K, E, k);
}

}  // namespace

int64_t moe_max_experts() { return MOE_MAX_E; }
int64_t moe_max_topk() { return MOE_MAX_K; }
int64_t moe_chunk_pairs() { return 16 * MOE_MAX_MT; }

int64_t moe_waves(int64_t N, int64_t K, bool gated) {
  return moe_waves_host(N, K, gated);
}

void moe_route(torch::Tensor topk_ids, torch::Tensor topk_w,
               torch::Tensor logits) {
  TORCH_CHECK(logits.is_cuda(), "moe_route: logits must be on GPU");
  TORCH_CHECK(logits.dim() == 2 && topk_ids.dim() == 2 && topk_w.dim() == 2,
              "moe_route: logits, topk_ids and topk_w must be 2-D");
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 ||
              logits.scalar_type() == torch::kFloat32,
              "moe_route: logits must be bf16 or fp32");
  TORCH_CHECK(logits.is_contiguous(), "moe_route: logits must be contiguous");
  const int64_t T = logits.size(0), E = logits.size(1), k = topk_ids.size(1);
  check_ek(E, k);
  check_tensor(topk_ids, logits, torch::kInt32, "moe_route: topk_ids");
  check_tensor(topk_w, logits, torch::kFloat32, "moe_route: topk_w");
  TORCH_CHECK(topk_ids.size(0) == T && topk_w.size(0) == T &&
              topk_w.size(1) == k,
              "moe_route: topk_ids and topk_w must be [T, k]");
  TORCH_CHECK(T * k < (int64_t(1) << 31), "moe_route: too many pairs");
  if (T == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)((T + 3) / 4));
  if (logits.scalar_type() == torch::kFloat32)
    hipLaunchKernelGGL((moe_route_kernel<float>), grid, dim3(256), 0, stream,
                       (int32_t*)topk_ids.data_ptr(),
                       (float*)topk_w.data_ptr(),
                       (const float*)logits.data_ptr(), (int)T, (int)E,
                       (int)k);
  else
    hipLaunchKernelGGL((moe_route_kernel<uint16_t>), grid, dim3(256), 0,
                       stream, (int32_t*)topk_ids.data_ptr(),
                       (float*)topk_w.data_ptr(),
                       (const uint16_t*)logits.data_ptr(), (int)T, (int)E,
                       (int)k);
}

void moe_align(torch::Tensor expert_off, torch::Tensor sorted_pairs,
               torch::Tensor topk_ids, int64_t E) {
  TORCH_CHECK(topk_ids.is_cuda(), "moe_align: topk_ids must be on GPU");
  TORCH_CHECK(topk_ids.dim() == 2, "moe_align: topk_ids must be [T, k]");
  const int64_t P = topk_ids.numel(), k = topk_ids.size(1);
  check_ek(E, k);
  check_tensor(topk_ids, topk_ids, torch::kInt32, "moe_align: topk_ids");
  TORCH_CHECK(P < (int64_t(1) << 31), "moe_align: too many pairs");
  check_lists(expert_off, sorted_pairs, topk_ids, E, P);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(ALIGN_THREADS), 0,
                     stream, (int32_t*)expert_off.data_ptr(),
                     (int32_t*)sorted_pairs.data_ptr(),
                     (const int32_t*)topk_ids.data_ptr(), (int)P, (int)E);
}

// act[P, I] = silu(x[p/k] @ w13[e, :I]^T) * (x[p/k] @ w13[e, I:]^T)
void moe_gemm_gated(torch::Tensor act, torch::Tensor x, torch::Tensor w13,
                    torch::Tensor expert_off, torch::Tensor sorted_pairs,
                    int64_t k) {
  TORCH_CHECK(w13.is_cuda(), "moe_gemm_gated: w13 must be on GPU");
  TORCH_CHECK(w13.dim() == 3 && x.dim() == 2 && act.dim() == 2,
              "moe_gemm_gated: w13 must be 3-D, x and act 2-D");
  const int64_t E = w13.size(0), I = w13.size(1) / 2, H = w13.size(2);
  const int64_t T = x.size(0), P = T * k;
  check_ek(E, k);
  check_tensor(w13, w13, torch::kBFloat16, "moe_gemm_gated: w13");
  check_tensor(x, w13, torch::kBFloat16, "moe_gemm_gated: x");
  check_tensor(act, w13, torch::kBFloat16, "moe_gemm_gated: act");
  TORCH_CHECK(H > 0 && H % 32 == 0, "moe_gemm_gated: H (", H,
              ") must be a positive multiple of 32");
  TORCH_CHECK(I > 0 && I % 32 == 0 && w13.size(1) == 2 * I,
              "moe_gemm_gated: w13 must be [E, 2I, H] with I a positive "
              "multiple of 32");
  TORCH_CHECK(x.size(1) == H, "moe_gemm_gated: x must be [T, H], H = ", H);
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_gemm_gated: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && 2 * I * H < (int64_t(1) << 31),
              "moe_gemm_gated: problem too large");
  check_lists(expert_off, sorted_pairs, w13, E, P);
  if (T == 0) return;
  dispatch_moe_gemm<true>(T, moe_waves_host(I, H, true), act.data_ptr(), x,
                          w13, nullptr, expert_off, sorted_pairs, (int)P,
                          (int)I, (int)H, (int)E, (int)k);
}

// ypair[P, H] (fp32) = topk_w[p] * (act[p] @ w2[e]^T)
void moe_gemm_down(torch::Tensor ypair, torch::Tensor act, torch::Tensor w2,
                   torch::Tensor topk_w, torch::Tensor expert_off,
                   torch::Tensor sorted_pairs) {
  TORCH_CHECK(w2.is_cuda(), "moe_gemm_down: w2 must be on GPU");
  TORCH_CHECK(w2.dim() == 3 && act.dim() == 2 && ypair.dim() == 2 &&
              topk_w.dim() == 2,
              "moe_gemm_down: w2 must be 3-D, act, ypair and topk_w 2-D");
  const int64_t E = w2.size(0), H = w2.size(1), I = w2.size(2);
  const int64_t T = topk_w.size(0), k = topk_w.size(1), P = T * k;
  check_ek(E, k);
  check_tensor(w2, w2, torch::kBFloat16, "moe_gemm_down: w2");
  check_tensor(act, w2, torch::kBFloat16, "moe_gemm_down: act");
  check_tensor(ypair, w2, torch::kFloat32, "moe_gemm_down: ypair");
  check_tensor(topk_w, w2, torch::kFloat32, "moe_gemm_down: topk_w");
  TORCH_CHECK(H > 0 && H % 32 == 0, "moe_gemm_down: H (", H,
              ") must be a positive multiple of 32");
  TORCH_CHECK(I > 0 && I % 32 == 0, "moe_gemm_down: I (", I,
              ") must be a positive multiple of 32");
  TORCH_CHECK(act.size(0) == P && act.size(1) == I,
              "moe_gemm_down: act must be [T*k, I] = [", P, ", ", I, "]");
  TORCH_CHECK(ypair.size(0) == P && ypair.size(1) == H,
              "moe_gemm_down: ypair must be [T*k, H] = [", P, ", ", H, "]");
  TORCH_CHECK(P < (int64_t(1) << 31) && I * H < (int64_t(1) << 31),
              "moe_gemm_down: problem too large");
  check_lists(expert_off, sorted_pairs, w2, E, P);
  if (T == 0) return;
  dispatch_moe_gemm<false>(T, moe_waves_host(H, I, false), ypair.data_ptr(),
                           act, w2, (const float*)topk_w.data_ptr(),
                           expert_off, sorted_pairs, (int)P, (int)H, (int)I,
                           (int)E, (int)k);
}

void moe_combine(torch::Tensor out, torch::Tensor ypair, int64_t k) {
  TORCH_CHECK(ypair.is_cuda(), "moe_combine: ypair must be on GPU");
  TORCH_CHECK(out.dim() == 2 && ypair.dim() == 2,
              "moe_combine: out and ypair must be 2-D");
  check_tensor(ypair, ypair, torch::kFloat32, "moe_combine: ypair");
  check_tensor(out, ypair, torch::kBFloat16, "moe_combine: out");
  const int64_t T = out.size(0), H = out.size(1);
  TORCH_CHECK(k >= 1 && k <= MOE_MAX_K, "moe_combine: k (", k,
              ") must be in [1, ", MOE_MAX_K, "]");
  TORCH_CHECK(H > 0 && H % 32 == 0, "moe_combine: H (", H,
              ") must be a positive multiple of 32");
  TORCH_CHECK(ypair.size(0) == T * k && ypair.size(1) == H,
              "moe_combine: ypair must be [T*k, H] = [", T * k, ", ", H, "]");
  if (T == 0) return;
  const int64_t total8 = T * H / 8;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((total8 + 255) / 256)),
                     dim3(256), 0, stream, (uint16_t*)out.data_ptr(),
                     (const float*)ypair.data_ptr(), total8, (int)H, (int)k);
}
