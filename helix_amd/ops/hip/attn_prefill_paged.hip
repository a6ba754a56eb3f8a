// Flash-attention prefill over the paged KV cache (varlen, causal, GQA,
// query offset, optional sliding window) for CDNA4.
//
// Prefix-cached and chunked prefill attend to a context that lives in the
// paged cache. attn_prefill.hip takes compact [T, Hkv, D] K/V, so the
// context used to be gathered (and, for an fp8 cache, dequantized) into a
// per-layer copy first. This kernel reads K and V through the block table,
// in bf16 or e4m3, and needs no copy, no scratch and no second kernel.
//
// Arithmetic contract: for every (query row, head) the floating-point
// operations are those of attn_prefill_kernel<1, D> on the gathered (and
// dequantized) K/V, so the output is bit-identical to that composition
// (tests/test_attn_paged_prefill_gpu.py::test_bit_identical_to_gather).
// The tile body below (QK^T, online softmax, P -> bf16, PV, epilogue) is a
// copy of that kernel's: 64-token K tiles at absolute multiples of 64,
// ascending from tile kv_lo / 64, the same MFMA k-order and 16-lane
// reductions, o / max(l, 1e-20) at the end. e4m3 -> bf16 is exact (the
// upper 16 bits of the converted fp32), so LDS holds the same bits as after
// a gather + dequant. Folding the two bodies is left for later.
//
// What is this kernel's own: the paged loader.
//  - Token tok of kv head hkv is at ((id * Hkv + hkv) * bs + (tok & (bs-1)))
//    * D, id = table[tok >> log2(bs)], in 64-bit; the host passes log2(bs).
//    A 64-token tile is one block at an offset for bs >= 64 and 64 / bs
//    whole blocks otherwise; a thread needs one id per 16-byte load.
//  - No K or V address waits on a table load in the main loop: the ids a
//    thread needs for tile t+2 are loaded right after load_tile(t+1)
//    issues and sit in registers for a whole tile's compute before
//    load_tile(t+2) forms addresses from them. Only the prologue waits on
//    the table (once, for the ids of the first two tiles).
//  - Table indices are clamped to the sequence's last block and to the
//    table's last column, ids to the cache's last block: no lane reads past
//    a table row or the cache, whatever the device data holds.
//  - Tokens at or past klen are zero-filled, not loaded: an unwritten fp8
//    slot can hold the NaN byte 0x7F, and 0 * NaN would poison the PV sum.
//  - bf16: the chunk map of attn_prefill.hip, 8 elements per b128, 4 (D =
//    128) or 2 (D = 64) K and V loads per thread and tile.
//  - e4m3: one b128 carries 16 elements, so 2 / 1 loads per thread; the
//    raw bytes stay in registers while in flight (a quarter of the bf16
//    staging registers) and are converted when the tile is written to LDS:
//    two 16-byte K vectors into the k_swz slots the bf16 path would use,
//    16 V scalars through v_swz.
//  - LDS layout and footprint, and __launch_bounds__(256, 2), are those of
//    attn_prefill.hip: two workgroups per CU.

// Everything device-side in this file is compiled without packed fp32
// arithmetic (v_pk_mul_f32 and kin, which the compiler otherwise forms from
// the softmax and rescale pairs): scalar fp32 ops only. The attribute has to
// cover the helpers of common.h and the kernel's lambdas as well as the
// kernel: a callee whose target features differ from its caller's is not
// inlined. For the same reason the kernel calls no inline function of the
// HIP runtime headers (they may be included ahead of this file): it has
// its own barrier and lane exchange below, and reads the ids from builtins.
#if defined(__HIP_DEVICE_COMPILE__)
#define NO_PK_F32_BEGIN                                                      \
  _Pragma("clang attribute push(__attribute__((target(\"no-packed-fp32-ops\"))), apply_to = function)")
#define NO_PK_F32_END _Pragma("clang attribute pop")
#else
#define NO_PK_F32_BEGIN
#define NO_PK_F32_END
#endif

NO_PK_F32_BEGIN
#include "common.h"
NO_PK_F32_END
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace helix {
// paged_attn_decode.hip: the rule a cache block size obeys (a power of two
// of at least 8), checked; returns log2(block_size).
int kv_block_log2(int64_t block_size);
}  // namespace helix

namespace {
NO_PK_F32_BEGIN

constexpr int QTILE = 64;     // q rows per block
constexpr int KTILE = 64;     // kv tokens per tile
constexpr int DMAX = 128;
constexpr int P_PITCH = 72;   // p_lds row pitch (elements): 144B = 9 slots

// LDS swizzles of attn_prefill.hip (K row-major, V transposed).
__device__ __forceinline__ int k_swz(int tok, int byte_in_row) {
  return tok * (DMAX * 2) + (byte_in_row ^ ((tok & 7) << 4));
}
__device__ __forceinline__ int v_swz(int dim, int byte_in_row) {
  const int s = ((dim >> 3) ^ dim) & 7;
  return dim * (KTILE * 2) + (byte_in_row ^ (s << 4));
}

// __syncthreads() and __shfl_xor(v, off) for off < 64, as the runtime
// headers define them.
__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ float lane_xor(float v, int off, int lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ off) << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ uint16_t f32_hi16(float f) {
  return (uint16_t)(__builtin_bit_cast(uint32_t, f) >> 16);
}

// 16 e4m3 bytes -> 16 bf16, exactly: every e4m3 value is a bf16 value, so
// the upper half of the converted fp32 is the whole number.
__device__ __forceinline__ void fp8x16_to_bf16(const u32x4& raw, u16x8& lo,
                                               u16x8& hi) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], true);
    u16x8& dst = w < 2 ? lo : hi;
    const int o = (w & 1) * 4;
    dst[o + 0] = f32_hi16(a[0]);
    dst[o + 1] = f32_hi16(a[1]);
    dst[o + 2] = f32_hi16(b[0]);
    dst[o + 3] = f32_hi16(b[1]);
  }
}

template <int D, bool KV8>
__global__ __launch_bounds__(256, 2) void attn_prefill_paged_kernel(
    uint16_t* __restrict__ out,            // [T, Hq, D]
    const uint16_t* __restrict__ q,        // [T, Hq, D]
    const void* __restrict__ k_cache,      // [nblocks, Hkv, bs, D]
    const void* __restrict__ v_cache,      //   bf16, or e4m3 bytes (KV8)
    const int* __restrict__ block_tables,  // [B, cols]
    const int* __restrict__ cu_seqlens_q,  // [B+1] query rows
    const int* __restrict__ seq_lens,      // [B] context lengths (>= q rows)
    float scale, int Hq, int Hkv, int bs_log2, int cols, int nblocks,
    int window) {
  // not blockIdx / threadIdx: those go through device-library functions
  const int qtile = __builtin_amdgcn_workgroup_id_x();
  const int seq = __builtin_amdgcn_workgroup_id_y();
  const int hq = __builtin_amdgcn_workgroup_id_z();
  const int hkv = hq / (Hq / Hkv);
  const int q_start = cu_seqlens_q[seq];
  const int qlen = cu_seqlens_q[seq + 1] - q_start;
  const int klen = seq_lens[seq];
  const int ctx = klen - qlen;   // cached-prefix offset (0 = plain prefill)
  const int qbase = qtile * QTILE;
  if (qbase >= qlen) return;

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int wid = tid / WAVE;
  const int lane = tid & (WAVE - 1);
  const int lane_hi = lane >> 4;   // 0..3
  const int lane_lo = lane & 15;   // 0..15

  // double-buffered K/V: ONE barrier per tile (attn_prefill.hip)
  __shared__ uint16_t k_lds[2][KTILE * DMAX];
  __shared__ uint16_t v_lds[2][DMAX * KTILE];       // transposed
  __shared__ uint16_t p_lds[4][16 * P_PITCH];

  // ---- Q fragments (A-operand layout), 16 rows per wave ----
  const int my_qrow = qbase + wid * 16 + lane_lo;
  constexpr int nkt = D / 32;
  bf16x8 q_frag[nkt];
#pragma unroll
  for (int kt = 0; kt < nkt; ++kt) {
    if (my_qrow < qlen) {
      const uint16_t* src =
          q + ((int64_t)(q_start + my_qrow) * Hq + hq) * D + kt * 32 +
          lane_hi * 8;
      u16x8 raw = *reinterpret_cast<const u16x8*>(src);
      q_frag[kt] = *reinterpret_cast<bf16x8*>(&raw);
    } else {
      q_frag[kt] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -INFINITY;
    l_run[r] = 0.f;
  }
  constexpr int nc = D / 16;
  floatx4 o_acc[nc];
#pragma unroll
  for (int c = 0; c < nc; ++c) o_acc[c] = floatx4{0, 0, 0, 0};

  const int kv_max = min(klen, ctx + qbase + QTILE);
  // sliding window: rows in this q-tile never look below kv_lo
  const int kv_lo = window > 0 ? max(0, ctx + qbase - window + 1) : 0;
  const int t_first = kv_lo / KTILE;
  const int ntiles = (kv_max + KTILE - 1) / KTILE;

  // ---- paged loader ----
  // Per-thread staging: the tile's 16-byte vectors over 256 threads. A
  // vector is VE elements of one token (8 bf16 or 16 e4m3), so a thread
  // has nld = 4 / 2 (bf16, D = 128 / 64) or 2 / 1 (e4m3) loads of K and
  // of V, each with a token, and so a block id, of its own.
  constexpr int VE = KV8 ? 16 : 8;
  constexpr int nld = KTILE * D / VE / 256;
  constexpr int TOK_STEP = 256 * VE / D;   // tokens between a thread's loads
  const int tok0 = tid * VE / D;           // token of load 0, then +TOK_STEP
  const int d0 = tid * VE % D;             // first dim of every load
  u32x4 k_reg[nld], v_reg[nld];

  const int* btable = block_tables + (int64_t)seq * cols;
  const int bs_mask = (1 << bs_log2) - 1;
  const int last_idx = max(0, min((klen - 1) >> bs_log2, cols - 1));
  // Block ids of this thread's loads of tile t, as the table holds them.
  // Every lane loads (index clamped, no branch around the load). Nothing
  // here touches the loaded value: its first use, the clamp in load_tile,
  // is a tile later, so no wait lands behind the K/V loads just issued.
  auto fetch_ids = [&](int t, int (&ids)[nld]) {
#pragma unroll
    for (int c = 0; c < nld; ++c) {
      const int idx = (t * KTILE + c * TOK_STEP + tok0) >> bs_log2;
      ids[c] = btable[min(idx, last_idx)];
    }
  };
  auto load_tile = [&](int t, const int (&ids)[nld]) {
#pragma unroll
    for (int c = 0; c < nld; ++c) {
      const int gtok = t * KTILE + c * TOK_STEP + tok0;
      if (gtok < klen) {
        const int64_t id = min(max(ids[c], 0), nblocks - 1);
        const int64_t row = ((id * Hkv + hkv) << bs_log2) + (gtok & bs_mask);
        const int64_t byte = (row * D + d0) * (KV8 ? 1 : 2);
        k_reg[c] = *reinterpret_cast<const u32x4*>(
            (const char*)k_cache + byte);
        v_reg[c] = *reinterpret_cast<const u32x4*>(
            (const char*)v_cache + byte);
      } else {
        k_reg[c] = u32x4{0, 0, 0, 0};
        v_reg[c] = u32x4{0, 0, 0, 0};
      }
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int c = 0; c < nld; ++c) {
      const int tok = c * TOK_STEP + tok0;
      if constexpr (KV8) {
        u16x8 klo, khi, vlo, vhi;
        fp8x16_to_bf16(k_reg[c], klo, khi);
        fp8x16_to_bf16(v_reg[c], vlo, vhi);
        *reinterpret_cast<u16x8*>((char*)k_lds[buf] + k_swz(tok, d0 * 2)) =
            klo;
        *reinterpret_cast<u16x8*>(
            (char*)k_lds[buf] + k_swz(tok, (d0 + 8) * 2)) = khi;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          *reinterpret_cast<uint16_t*>(
              (char*)v_lds[buf] + v_swz(d0 + i, tok * 2)) = vlo[i];
          *reinterpret_cast<uint16_t*>(
              (char*)v_lds[buf] + v_swz(d0 + 8 + i, tok * 2)) = vhi[i];
        }
      } else {
        *reinterpret_cast<u32x4*>((char*)k_lds[buf] + k_swz(tok, d0 * 2)) =
            k_reg[c];
        const u16x8 vv = *reinterpret_cast<const u16x8*>(&v_reg[c]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          *reinterpret_cast<uint16_t*>(
              (char*)v_lds[buf] + v_swz(d0 + i, tok * 2)) = vv[i];
        }
      }
    }
  };

  // Prologue: the one wait on the table, for the ids of the first two
  // tiles. From here on `ids` holds the ids of the tile the next
  // load_tile reads, loaded one tile of compute before that.
  int ids[nld], ids_b[nld];
  fetch_ids(t_first, ids);
  fetch_ids(t_first + 1, ids_b);
  load_tile(t_first, ids);
  store_tile(0);
  if (t_first + 1 < ntiles) load_tile(t_first + 1, ids_b);
  fetch_ids(t_first + 2, ids);
  for (int t = t_first; t < ntiles; ++t) {
    const int buf = (t - t_first) & 1;
    block_barrier();            // buf's staging (and last compute) done

    const int kv_base = t * KTILE;
    // ---- QK^T: 4 halves of 16 tokens ----
    floatx4 s_frag[KTILE / 16];
    float p_val[KTILE / 16][4];
#pragma unroll
    for (int h = 0; h < KTILE / 16; ++h) {
      s_frag[h] = floatx4{0, 0, 0, 0};
      const int tok = h * 16 + lane_lo;
#pragma unroll
      for (int kt = 0; kt < nkt; ++kt) {
        const int byte = (kt * 32 + lane_hi * 8) * 2;
        u16x8 raw = *reinterpret_cast<const u16x8*>(
            (char*)k_lds[buf] + k_swz(tok, byte));
        s_frag[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            q_frag[kt], *reinterpret_cast<bf16x8*>(&raw), s_frag[h], 0, 0, 0);
      }
    }

    // ---- Online softmax over the 4 halves ----
    float corr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qpos = ctx + qbase + wid * 16 + lane_hi * 4 + r;
      float s[KTILE / 16];
      float m_tile = -INFINITY;
#pragma unroll
      for (int h = 0; h < KTILE / 16; ++h) {
        s[h] = s_frag[h][r] * scale;
        const int tp = kv_base + h * 16 + lane_lo;
        if ((tp > qpos || (window > 0 && qpos - tp >= window)) ||
            tp >= klen) s[h] = -1e30f;
        m_tile = fmaxf(m_tile, s[h]);
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1)
        m_tile = fmaxf(m_tile, lane_xor(m_tile, off, lane));
      const float m_new = fmaxf(m_run[r], m_tile);
      corr[r] = (m_run[r] == -INFINITY) ? 0.f : __expf(m_run[r] - m_new);
      float l_tile = 0.f;
#pragma unroll
      for (int h = 0; h < KTILE / 16; ++h) {
        p_val[h][r] = __expf(s[h] - m_new);
        l_tile += p_val[h][r];
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1)
        l_tile += lane_xor(l_tile, off, lane);
      l_run[r] = l_run[r] * corr[r] + l_tile;
      m_run[r] = m_new;
    }

    // ---- P -> per-wave LDS, then PV ----
#pragma unroll
    for (int h = 0; h < KTILE / 16; ++h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p_lds[wid][(lane_hi * 4 + r) * P_PITCH + h * 16 + lane_lo] =
            f32_to_bf16(p_val[h][r]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    bf16x8 p_frag[KTILE / 32];
#pragma unroll
    for (int kk = 0; kk < KTILE / 32; ++kk) {
      u16x8 raw = *reinterpret_cast<const u16x8*>(
          &p_lds[wid][lane_lo * P_PITCH + kk * 32 + lane_hi * 8]);
      p_frag[kk] = *reinterpret_cast<bf16x8*>(&raw);
    }
#pragma unroll
    for (int c = 0; c < nc; ++c) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[c][r] *= corr[r];
#pragma unroll
      for (int kk = 0; kk < KTILE / 32; ++kk) {
        u16x8 raw = *reinterpret_cast<const u16x8*>(
            (char*)v_lds[buf] +
            v_swz(c * 16 + lane_lo, (kk * 32 + lane_hi * 8) * 2));
        o_acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            p_frag[kk], *reinterpret_cast<bf16x8*>(&raw), o_acc[c], 0, 0, 0);
      }
    }
    // stage tile t+1 into the other buffer (nobody reads it this iter);
    // then issue tile t+2's loads, from the ids fetched a tile ago, and
    // behind them the table loads for tile t+3
    if (t + 1 < ntiles) {
      store_tile(buf ^ 1);
      if (t + 2 < ntiles) {
        load_tile(t + 2, ids);
        fetch_ids(t + 3, ids);
      }
    }
  }

  // ---- Epilogue ----
#pragma unroll
  for (int c = 0; c < nc; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qbase + wid * 16 + lane_hi * 4 + r;
      if (qrow < qlen) {
        out[((int64_t)(q_start + qrow) * Hq + hq) * D + c * 16 + lane_lo] =
            f32_to_bf16(o_acc[c][r] / fmaxf(l_run[r], 1e-20f));
      }
    }
  }
}

NO_PK_F32_END
}  // namespace

// Precondition on device data, not checked here: seq_lens[b] >= the query
// rows of sequence b (the CPU reference asserts it), and block ids within
// the cache (the kernel clamps them).
void attn_prefill_paged(torch::Tensor out, torch::Tensor q,
                        torch::Tensor k_cache, torch::Tensor v_cache,
                        torch::Tensor block_tables, torch::Tensor cu_seqlens,
                        torch::Tensor seq_lens, int64_t max_seqlen,
                        int64_t max_klen, double scale, int64_t window) {
  TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && block_tables.dim() == 2 &&
                  cu_seqlens.dim() == 1 && seq_lens.dim() == 1,
              "attn_prefill_paged: q [T, Hq, D], caches [nblocks, Hkv, bs, "
              "D], block_tables [B, cols], cu_seqlens [B+1], seq_lens [B]");
  const int64_t Hq = q.size(1);
  const int64_t D = q.size(2);
  const int64_t Hkv = k_cache.size(1);
  const int64_t cols = block_tables.size(1);
  const int64_t B = cu_seqlens.size(0) - 1;
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  out.scalar_type() == torch::kBFloat16 &&
                  out.sizes() == q.sizes(),
              "q and out must be bf16 of one shape");
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type() &&
                  (k_cache.scalar_type() == torch::kBFloat16 ||
                   k_cache.scalar_type() == torch::kUInt8),
              "k_cache and v_cache must share a dtype, bf16 or uint8 (e4m3)");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes() && k_cache.size(3) == D,
              "k_cache and v_cache must share the shape [nblocks, Hkv, bs, ",
              D, "]; got ", k_cache.sizes(), " and ", v_cache.sizes());
  const int bs_log2 = kv_block_log2(k_cache.size(2));
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  TORCH_CHECK(block_tables.scalar_type() == torch::kInt32 &&
                  cu_seqlens.scalar_type() == torch::kInt32 &&
                  seq_lens.scalar_type() == torch::kInt32,
              "block_tables, cu_seqlens and seq_lens must be int32");
  TORCH_CHECK(B >= 0 && seq_lens.size(0) == B && block_tables.size(0) == B,
              "seq_lens and block_tables must have B = ", B,
              " rows (cu_seqlens has B + 1 entries)");
  TORCH_CHECK(q.is_contiguous() && out.is_contiguous() &&
                  k_cache.is_contiguous() && v_cache.is_contiguous() &&
                  block_tables.is_contiguous() && cu_seqlens.is_contiguous() &&
                  seq_lens.is_contiguous(),
              "attn_prefill_paged takes contiguous tensors");
  TORCH_CHECK(max_seqlen >= 0 && max_klen >= 0 && window >= 0,
              "max_seqlen, max_klen and window must be >= 0");
  TORCH_CHECK(cols * k_cache.size(2) >= max_klen, "block_tables has ", cols,
              " columns of ", k_cache.size(2), " tokens, max_klen is ",
              max_klen);
  for (const torch::Tensor* t : {&out, &k_cache, &v_cache, &block_tables,
                                 &cu_seqlens, &seq_lens})
    TORCH_CHECK(t->is_cuda() && t->device() == q.device(),
                "attn_prefill_paged: all tensors must be on q's device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % 16 == 0,
              "q and the caches must be 16-byte aligned (vector loads)");
  const int n_qtiles = cdiv((int)max_seqlen, QTILE);
  TORCH_CHECK(B <= 65535 && Hq <= 65535 && k_cache.size(0) <= INT32_MAX,
              "attn_prefill_paged: B, Hq or the block count is too large");
  if (B == 0 || max_seqlen == 0) return;

  auto stream = at::hip::getCurrentHIPStream();
  const bool kv8 = k_cache.scalar_type() == torch::kUInt8;
#define LAUNCH(DH, K8)                                                       \
  hipLaunchKernelGGL((attn_prefill_paged_kernel<DH, K8>),                    \
                     dim3(n_qtiles, B, Hq), dim3(256), 0, stream,            \
                     (uint16_t*)out.data_ptr(),                              \
                     (const uint16_t*)q.data_ptr(), k_cache.data_ptr(),      \
                     v_cache.data_ptr(), block_tables.data_ptr<int>(),       \
                     cu_seqlens.data_ptr<int>(), seq_lens.data_ptr<int>(),   \
                     (float)scale, (int)Hq, (int)Hkv, bs_log2, (int)cols,    \
                     (int)k_cache.size(0), (int)window)
  if (D == 128) {
    if (kv8) LAUNCH(128, true); else LAUNCH(128, false);
  } else {
    if (kv8) LAUNCH(64, true); else LAUNCH(64, false);
  }
#undef LAUNCH
}
