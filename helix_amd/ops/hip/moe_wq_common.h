// Host-side contract of a stack of ggml Q4_0 / Q8_0 experts, shared by the
// routed expert GEMMs over them (moe_wq.hip: decode, moe_grouped_wq.hip:
// prefill). moe_wq.hip's header has the plane layout.
#pragma once

#include "moe_common.h"

namespace helix {

// Contract of one expert stack's (qs, d) pair: returns E; sets rows and K.
inline int64_t check_stack_wq(const torch::Tensor& qs, const torch::Tensor& d,
                              int64_t bits, const char* what,
                              int64_t* rows_out, int64_t* K_out) {
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

}  // namespace helix
