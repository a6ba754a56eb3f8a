// Limits and host-side checks shared by the routed expert GEMMs
// (moe.hip: bf16 experts, moe_wq.hip: ggml Q4_0/Q8_0 experts, moe_kq.hip:
// ggml Q4_K/Q6_K experts).
#pragma once

#include "common.h"
#include <torch/extension.h>

namespace helix {

constexpr int MOE_MAX_E = 256;
constexpr int MOE_MAX_K = 8;
constexpr int MOE_MAX_MT = 4;            // token tiles per chunk

// K-split factor of one expert's [N, K] weight (N = I for the gated GEMM,
// whose workgroups own a gate and an up tile): gemm_wq's rule. The gated
// kernel stops at 8 waves, which keeps its reduction buffer (W-1) x 2 x MT
// KiB under 64 KiB.
inline int moe_waves_host(int64_t N, int64_t K, bool gated) {
  int w = 4;
  const int cap = gated ? 8 : 16;
  while (w < cap && (N / 16) * w < 4096 && K / 128 >= 4 * w) w *= 2;
  return w;
}

inline bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

inline void check_tensor(const torch::Tensor& t, const torch::Tensor& like,
                         c10::ScalarType dt, const char* what) {
  TORCH_CHECK(t.is_cuda(), what, " must be on GPU");
  TORCH_CHECK(t.device() == like.device(), what, ": device mismatch");
  TORCH_CHECK(t.scalar_type() == dt, what, " must be ", dt, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), what, " must be contiguous");
  TORCH_CHECK(aligned16(t), what, " must be 16-byte aligned");
}

inline void check_ek(int64_t E, int64_t k) {
  TORCH_CHECK(E >= 1 && E <= MOE_MAX_E, "moe: E (", E, ") must be in [1, ",
              MOE_MAX_E, "]");
  TORCH_CHECK(k >= 1 && k <= MOE_MAX_K && k <= E, "moe: k (", k,
              ") must be in [1, min(E, ", MOE_MAX_K, ")]");
}

// expert_off [E+1] and sorted_pairs [P], int32
inline void check_lists(const torch::Tensor& expert_off,
                        const torch::Tensor& sorted_pairs,
                        const torch::Tensor& like, int64_t E, int64_t P) {
  check_tensor(expert_off, like, torch::kInt32, "moe: expert_off");
  check_tensor(sorted_pairs, like, torch::kInt32, "moe: sorted_pairs");
  TORCH_CHECK(expert_off.dim() == 1 && expert_off.size(0) == E + 1,
              "moe: expert_off must be [E + 1] = [", E + 1, "]");
  TORCH_CHECK(sorted_pairs.dim() == 1 && sorted_pairs.size(0) == P,
              "moe: sorted_pairs must be [P] = [", P, "]");
}

}  // namespace helix
