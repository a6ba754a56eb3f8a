// Host-side contract of a stack of ggml Q4_K / Q6_K experts, shared by the
// routed expert GEMMs over them (moe_kq.hip: decode, moe_grouped_kq.hip:
// prefill). moe_kq.hip's header has the plane layout.
#pragma once

#include "moe_common.h"
#include <string>
#include <vector>

namespace helix {

constexpr int MOE_KQ_SB = 256;                  // elements per super-block

inline int moe_kq_fmt(const std::string& fmt, const char* what) {
  TORCH_CHECK(fmt == "q4_k" || fmt == "q6_k", what, ": unknown format '", fmt,
              "' (expected q4_k or q6_k)");
  return fmt == "q4_k" ? 4 : 6;
}

inline void check_stack_plane(const torch::Tensor& t,
                              const torch::Tensor& first, const char* what,
                              const char* name, c10::ScalarType dtype,
                              std::vector<int64_t> shape) {
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
inline int64_t check_stack_kq(const std::vector<torch::Tensor>& planes,
                              int fmt, const char* what, int64_t* rows_out,
                              int64_t* K_out) {
  const size_t want = fmt == 4 ? 2 : 4;
  TORCH_CHECK(planes.size() == want, what, ": ", fmt == 4 ? "q4_k" : "q6_k",
              " takes ", want, " planes, got ", planes.size());
  const auto& q = planes[0];
  TORCH_CHECK(q.dim() == 3, what,
              ": the payload plane must be 3-D [E, rows, K/2]");
  const int64_t E = q.size(0), rows = q.size(1), K = q.size(2) * 2;
  TORCH_CHECK(K > 0 && K % MOE_KQ_SB == 0, what, ": K (", K,
              ") must be a positive multiple of 256");
  TORCH_CHECK(rows > 0 && rows % 16 == 0, what, ": rows (", rows,
              ") must be a positive multiple of 16");
  TORCH_CHECK(rows * K < (int64_t(1) << 31), what, ": expert too large");
  if (fmt == 4) {
    check_stack_plane(q, q, what, "qs", torch::kUInt8, {E, rows, K / 2});
    check_stack_plane(planes[1], q, what, "hdr", torch::kUInt8,
                      {E, rows, K / MOE_KQ_SB, 16});
  } else {
    check_stack_plane(q, q, what, "ql", torch::kUInt8, {E, rows, K / 2});
    check_stack_plane(planes[1], q, what, "qh", torch::kUInt8,
                      {E, rows, K / 4});
    check_stack_plane(planes[2], q, what, "sc", torch::kInt8,
                      {E, rows, K / 16});
    check_stack_plane(planes[3], q, what, "d", torch::kFloat16,
                      {E, rows, K / MOE_KQ_SB});
  }
  *rows_out = rows;
  *K_out = K;
  return E;
}

}  // namespace helix
