// Paged-attention decode (single query token per sequence) for CDNA4.
//
// Replaces the decode attention the reference delegates to vLLM
// (SURVEY.md §2.8 "Decode attention (paged KV)").
//
// Design:
//  - KV-bandwidth-bound: each KV byte is read once per kv-head and
//    amortized across the G = Hq/Hkv GQA query heads.
//  - grid = (num_seqs, Hkv, num_partitions): flash-decoding split-K, host
//    sizes partitions to fill the 256 CUs (>= TARGET_WGS workgroups, at
//    most MAX_PARTS partitions); a reduce kernel merges the partials.
//  - DHEAD and G are template parameters so every inner loop fully
//    unrolls; K rows and V tiles are loaded into registers in batches
//    BEFORE any math so the wave keeps many VMEM ops in flight.
//  - 128-thread blocks (2 waves) walk the partition in 128-token chunks:
//      A: thread t dots the K row of token t (16B loads issued one chunk
//         ahead, see kpre below) against the G query vectors in LDS
//         (broadcast reads).
//      B: per-head online softmax (running m, l), one wave per head.
//      C: V accumulation, thread owns 8 dims, VPS-token load batches
//         (bf16 rows staged raw, fp8 rows converted as they land).
//  - No K or V address waits on a block-table load: the physical ids
//    of the blocks a chunk touches (at most 128 / bs + 1) are staged in
//    LDS two chunks ahead (blk_ids below); a token's address is a
//    ds_read, a shift and a mask (block_size is a power of two >= 8).
//  - KV8: the paged cache holds OCP e4m3 bytes (opt-in
//    kv_cache_dtype="fp8"): halves the KV traffic this kernel is
//    latency/BW-bound on; dequant is one v_cvt per element.
//  - launch bounds floor of 2 waves/SIMD: register room for the 16-deep
//    K prefetch (168 VGPRs, no spills, still 3 waves/SIMD).
//
// Retired variants, all measured slower; the last commit that holds
// them is named in profiles/r03_decode_prune.md:
//  - MFMA phase A (16x16x32 bf16 scores): -20 %, docs/KERNELS.md and
//    profiles/r01_pmc_decode_b512.txt (latency-bound, not VALU-bound).
//  - K prefetch without the waves/SIMD floor of 2: -3 % on the
//    microbench, profiles/r02_decode_kpre.md (compiler re-sinks it).
//  - waves/SIMD floor of 2 without K prefetch: +-0, same file.
//  - V prefetch across chunks: 202 VGPRs, occupancy 3 -> 2, -7 % e2e,
//    same file.
//  - First V batch of a chunk issued ahead of the K prefetch (consumed
//    at vmcnt(16) with the K rows in flight): 192 VGPRs, occupancy
//    3 -> 2, +5 % time at B=512, profiles/r07_decode_blockids.md.
#include "common.h"
#include <type_traits>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

using namespace helix;

namespace {

constexpr int NTHREADS = 128;
constexpr int CHUNK = 128;
constexpr int MAX_G = 8;
constexpr int PART_QUANT = 128;   // split-K partition sizes are multiples
constexpr int MAX_PARTS = 512;    // weights the reduce kernel holds in LDS
constexpr int TARGET_WGS = 1024;  // split-K until the grid is this large
constexpr int MIN_BS = 8;         // smallest cache block the host lets in
// Block ids one chunk can touch: CHUNK / bs, plus one because a window
// starts the chunks off the block grid.
constexpr int IDS_MAX = CHUNK / MIN_BS + 1;

// How a cache of each type is read: 16-byte K-row vectors, 8-element
// V vectors, and the widen to fp32.
template <bool KV8> struct CacheElem;
template <> struct CacheElem<false> {
  using elem = uint16_t;
  using kvec = u16x8;
  using vvec = u16x8;
  static constexpr int KVEC = 8;
  static __device__ __forceinline__ float to_f32(uint16_t x) {
    return bf16_to_f32(x);
  }
};
template <> struct CacheElem<true> {
  using elem = uint8_t;
  using kvec = u8x16;
  using vvec = u8x8;
  static constexpr int KVEC = 16;
  static __device__ __forceinline__ float to_f32(uint8_t x) {
    return fp8_to_f32(x);
  }
};

// VPS: phase-C V rows loaded per batch. bf16 rows are staged raw, so
// more V bytes are in flight per wave before any conversion VALU
// touches them: 4 on a full grid, 8 when the grid underfills the chip
// (see launch_decode). fp8 does not stage raw and is built with 4 only.
//
// Waves/SIMD floor (second launch bound): 2 gives the register room for
// the 16-deep K prefetch at D = 128 bf16. The kernels whose K row is 32
// registers or fewer and that serve at most two heads fit 128 VGPRs, as
// they always did; the floor of 4 keeps them there (at a floor of 2 the
// scheduler takes 129-132 and loses a wave: +9 % time at D = 64, G = 2).
template <int DHEAD, int G, bool KV8, int VPS>
__global__ __launch_bounds__(NTHREADS,
                             (G <= 2 && (DHEAD == 64 || KV8)) ? 4 : 2)
void paged_attn_decode_kernel(
    uint16_t* __restrict__ out,          // [B, Hq, D] (used when nparts==1)
    float* __restrict__ tmp_out,         // [B, Hq, maxP, D]
    float* __restrict__ tmp_ml,          // [B, Hq, maxP, 2]
    const uint16_t* __restrict__ q,      // [B, Hq, D]
    const uint16_t* __restrict__ k_cache,// [nblocks, Hkv, bs, D]
    const uint16_t* __restrict__ v_cache,
    const int* __restrict__ block_tables,// [B, max_blocks]
    const int* __restrict__ seq_lens,    // [B]
    float scale, int Hkv, int bs_log2, int max_blocks,
    int partition_size, int max_parts, int window) {
  using CE = CacheElem<KV8>;
  using elem_t = typename CE::elem;
  using kvec_t = typename CE::kvec;
  using vvec_t = typename CE::vvec;
  constexpr int KVEC = CE::KVEC;

  const int seq = blockIdx.x;
  const int hkv = blockIdx.y;
  const int part = blockIdx.z;
  const int nparts = gridDim.z;
  const int Hq = Hkv * G;
  const int len = seq_lens[seq];
  const int kv_lo = (window > 0) ? max(0, len - window) : 0;
  int p_start = part * partition_size;
  const int p_hi = min(len, p_start + partition_size);
  if (p_start < kv_lo) p_start = kv_lo;
  if (p_start >= len || p_hi <= kv_lo) {
    if (nparts > 1 && threadIdx.x == 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int hq = hkv * G + g;
        float* ml = tmp_ml + (((int64_t)seq * Hq + hq) * max_parts + part) * 2;
        ml[0] = -INFINITY;
        ml[1] = 0.f;
      }
    }
    return;
  }
  const int p_end = p_hi;

  __shared__ float q_lds[G][DHEAD];
  __shared__ float s_lds[G][CHUNK];
  __shared__ float head_m[MAX_G], head_l[MAX_G], head_corr[MAX_G];
  // Physical block ids of the chunk in flight, of the next one (its K
  // rows are prefetched during this one) and of the one after (staged
  // during this one): no K or V address waits on a block-table load.
  // Entry i of a chunk's buffer is the block of token (first >> bs_log2)
  // + i. Three buffers and not two, because a buffer is read from the K
  // prefetch at the end of the previous chunk's phase A until the end
  // of its own phase C, and with two the refill would need a barrier of
  // its own; with three, the barriers that close each phase publish it.
  __shared__ int blk_ids[3][IDS_MAX];

  const int* btable = block_tables + (int64_t)seq * max_blocks;
  const int bs_mask = (1 << bs_log2) - 1;
  // The table entry thread t stages for the chunk at cbase. Every thread
  // loads (no branch around the load, so the waits behind it stay
  // counted); the index is clamped to the chunk's last block and only
  // threads below IDS_MAX write theirs to LDS.
  auto load_id = [&](int cbase) {
    const int last = (min(cbase + CHUNK, p_end) - 1) >> bs_log2;
    return btable[min((cbase >> bs_log2) + (int)threadIdx.x, last)];
  };
  // a partition of one chunk stages that chunk twice
  const int id0 = load_id(p_start);
  const int id1 = load_id(min(p_start + CHUNK, p_end - 1));

  // q: the group's G rows are contiguous, one vector load per thread
  {
    constexpr int QV = G * DHEAD >= NTHREADS ? G * DHEAD / NTHREADS : 1;
    typedef __attribute__((ext_vector_type(QV))) uint16_t qvec_t;
    const int idx = threadIdx.x * QV;
    if (idx < G * DHEAD) {
      const uint16_t* qp = q + ((int64_t)seq * Hq + hkv * G) * DHEAD + idx;
      float* dst = &q_lds[0][0] + idx;
      if constexpr (QV == 1) {
        dst[0] = bf16_to_f32(qp[0]) * scale;
      } else {
        const qvec_t raw = *reinterpret_cast<const qvec_t*>(qp);
#pragma unroll
        for (int i = 0; i < QV; ++i) dst[i] = bf16_to_f32(raw[i]) * scale;
      }
    }
  }
  if (threadIdx.x < IDS_MAX) {
    blk_ids[0][threadIdx.x] = id0;
    blk_ids[1][threadIdx.x] = id1;
  }
  if (threadIdx.x < MAX_G) {
    head_m[threadIdx.x] = -INFINITY;
    head_l[threadIdx.x] = 0.f;
  }
  __syncthreads();

  // Phase-C ownership: a thread owns 8 consecutive dims (one 16B load
  // per token) — the ablation probe showed b32 V loads were 64% of the
  // kernel (8x more VMEM instructions per byte than phase A's b128s).
  constexpr int NGRP = DHEAD / 8;            // dim-groups (16 for D=128)
  constexpr int C_PAR = NTHREADS / NGRP;     // token parities (8 / 16)
  const int d8 = (threadIdx.x % NGRP) * 8;   // my dims [d8, d8+8)
  const int cpar = threadIdx.x / NGRP;
  // Lets the compiler drop the one-row tail loop from the full chunks
  // (npass is then a constant). Only where the registers need it: the
  // bf16 G = 8 kernels spill without it (VPS = 8, D = 128: 18 VGPRs),
  // while the smaller groups schedule worse with it (<128, 4, false, 4>
  // goes from 168 to 182 VGPRs, one wave per SIMD less).
  if constexpr (G == 8 && !KV8) __builtin_assume(cpar < C_PAR);
  float acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;

  const int nwaves = NTHREADS / WAVE;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);

  // Element offset of token tok's row for this kv head; tok lies in the
  // chunk at cbase, whose block ids are in blk_ids[buf].
  auto row_off = [&](int buf, int cbase, int tok) {
    const int64_t blk =
        blk_ids[buf][(tok >> bs_log2) - (cbase >> bs_log2)];
    return (((blk * Hkv + hkv) << bs_log2) + (tok & bs_mask)) * DHEAD;
  };

  // Raw K row for the chunk about to be scored, loaded one full chunk
  // ahead: the 16B loads stay live across phases B+C of the previous
  // chunk — the latency they need to hide. Without this the compiler
  // sinks the loads into the consume loop and ~2 are in flight per wave
  // (ISA audit, profiles/r02_decode_kpre.md).
  kvec_t kpre[DHEAD / KVEC];
  auto issue_kpre = [&](int buf, int cbase) {
    const int tok = min(cbase + (int)threadIdx.x, p_end - 1);
    const elem_t* krow = (const elem_t*)k_cache + row_off(buf, cbase, tok);
#pragma unroll
    for (int j = 0; j < DHEAD / KVEC; ++j)
      kpre[j] = *reinterpret_cast<const kvec_t*>(krow + j * KVEC);
  };
  issue_kpre(0, p_start);

  // blk_ids buffer of this chunk, of the next and of the one after
  int cur = 0, nxt = 1, aft = 2;

  // One chunk. It is compiled twice, for the chunks that have a
  // successor and for the partition's last chunk: with the K prefetch
  // under a run-time condition the compiler cannot count the loads that
  // are younger than a V batch and waits for all of them (vmcnt(0)),
  // which drains the prefetch at the first V use. A chunk with a
  // successor is also a full one, so its trip counts are constants.
  auto do_chunk = [&](auto has_next, const int base) {
    constexpr bool HAS_NEXT = decltype(has_next)::value;
    const int chunk_n = HAS_NEXT ? CHUNK : p_end - base;
    const int npass = (chunk_n - cpar + C_PAR - 1) / C_PAR;  // my V rows
    auto vrow_off = [&](int tok) { return row_off(cur, base, tok) + d8; };

    // --- Phase A: scores -------------------------------------------------
    if (HAS_NEXT || (int)threadIdx.x < chunk_n) {
      float s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) s[g] = 0.f;
#pragma unroll
      for (int j = 0; j < DHEAD / KVEC; ++j) {
        float kv[KVEC];
#pragma unroll
        for (int i = 0; i < KVEC; ++i) kv[i] = CE::to_f32(kpre[j][i]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
          for (int i = 0; i < KVEC; ++i)
            s[g] += q_lds[g][j * KVEC + i] * kv[i];
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) s_lds[g][threadIdx.x] = s[g];
    }
    // Scores consumed. Issue the table loads for the chunk after the
    // next first (they return first and go to LDS in phase C), then the
    // NEXT chunk's K rows, which fly during softmax + V accumulation.
    const bool stage_ids = HAS_NEXT && base + 2 * CHUNK < p_end;
    int id_aft = 0;
    if constexpr (HAS_NEXT)
      id_aft = load_id(min(base + 2 * CHUNK, p_end - 1));
    if constexpr (HAS_NEXT) issue_kpre(nxt, base + CHUNK);
    __syncthreads();

    // --- Phase B: online softmax per head --------------------------------
    for (int g = wid; g < G; g += nwaves) {
      float m_chunk = -INFINITY;
      for (int i = lane; i < chunk_n; i += WAVE)
        m_chunk = fmaxf(m_chunk, s_lds[g][i]);
      m_chunk = wave_reduce_max(m_chunk);
      const float m_old = head_m[g];
      const float m_new = fmaxf(m_old, m_chunk);
      const float corr = (m_old == -INFINITY) ? 0.f : __expf(m_old - m_new);
      float l_add = 0.f;
      for (int i = lane; i < chunk_n; i += WAVE) {
        const float p = __expf(s_lds[g][i] - m_new);
        s_lds[g][i] = p;
        l_add += p;
      }
      l_add = wave_reduce_sum(l_add);
      if (lane == 0) {
        head_l[g] = head_l[g] * corr + l_add;
        head_m[g] = m_new;
        head_corr[g] = corr;
      }
    }
    __syncthreads();

    // --- Phase C: V accumulation (VPS-token load batches) ----------------
    // The multiply-accumulate is written out three times on purpose:
    // behind a shared helper the compiler schedules 12 of the 24 kernels
    // differently (profiles/r03_decode_prune.md).
    {
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] *= head_corr[g];
      // read next at the end of the next chunk's phase A: the barrier
      // that closes this phase publishes it
      if (stage_ids && threadIdx.x < IDS_MAX)
        blk_ids[aft][threadIdx.x] = id_aft;
      auto load_v = [&](int64_t off, float v[8]) {
        const vvec_t raw =
            *reinterpret_cast<const vvec_t*>((const elem_t*)v_cache + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = CE::to_f32(raw[i]);
      };
      int ps = 0;
      if constexpr (!KV8) {
        // raw-staged batches: VPS x 16B loads issue back-to-back (pure,
        // no dependent converts between them); conversion + FMA consume
        // them in order while later loads are still in flight
        for (; ps + VPS <= npass; ps += VPS) {
          u16x8 vraw[VPS];
#pragma unroll
          for (int u = 0; u < VPS; ++u)
            vraw[u] = *reinterpret_cast<const u16x8*>(
                v_cache + vrow_off(base + (ps + u) * C_PAR + cpar));
#pragma unroll
          for (int u = 0; u < VPS; ++u) {
            const int tok_i = (ps + u) * C_PAR + cpar;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = bf16_to_f32(vraw[u][i]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const float pv = s_lds[g][tok_i];
#pragma unroll
              for (int i = 0; i < 8; ++i) acc[g][i] += pv * v[i];
            }
          }
        }
      } else {
        // fp8 rows are half as wide: batches are converted as they land
        for (; ps + VPS <= npass; ps += VPS) {
          int64_t voff[VPS];
#pragma unroll
          for (int u = 0; u < VPS; ++u)
            voff[u] = vrow_off(base + (ps + u) * C_PAR + cpar);
          float v4[VPS][8];
#pragma unroll
          for (int u = 0; u < VPS; ++u) load_v(voff[u], v4[u]);
#pragma unroll
          for (int u = 0; u < VPS; ++u) {
            const int tok_i = (ps + u) * C_PAR + cpar;
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const float pv = s_lds[g][tok_i];
#pragma unroll
              for (int i = 0; i < 8; ++i) acc[g][i] += pv * v4[u][i];
            }
          }
        }
      }
      for (; ps < npass; ++ps) {
        const int tok_i = ps * C_PAR + cpar;
        float v[8];
        load_v(vrow_off(base + tok_i), v);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float pv = s_lds[g][tok_i];
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[g][i] += pv * v[i];
        }
      }
    }
    __syncthreads();
    const int t = cur;
    cur = nxt;
    nxt = aft;
    aft = t;
  };
  int base = p_start;
  for (; base + CHUNK < p_end; base += CHUNK)
    do_chunk(std::true_type{}, base);
  do_chunk(std::false_type{}, base);

  // Combine the C_PAR token parities via LDS, then write out.
  __shared__ float comb[G * DHEAD];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (cpar == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) comb[g * DHEAD + d8 + i] = acc[g][i];
    }
  }
  __syncthreads();
  for (int p = 1; p < C_PAR; ++p) {
    if (cpar == p) {
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i)
          comb[g * DHEAD + d8 + i] += acc[g][i];
    }
    __syncthreads();
  }
  if (cpar == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int hq = hkv * G + g;
      if (nparts == 1) {
        const float inv_l = 1.f / fmaxf(head_l[g], 1e-20f);
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          o[i] = comb[g * DHEAD + d8 + i] * inv_l;
        store_bf16x8(out + ((int64_t)seq * Hq + hq) * DHEAD + d8, o);
      } else {
        float* tp =
            tmp_out + (((int64_t)seq * Hq + hq) * max_parts + part) * DHEAD;
#pragma unroll
        for (int i = 0; i < 8; ++i) tp[d8 + i] = comb[g * DHEAD + d8 + i];
        if (d8 == 0) {
          float* ml =
              tmp_ml + (((int64_t)seq * Hq + hq) * max_parts + part) * 2;
          ml[0] = head_m[g];
          ml[1] = head_l[g];
        }
      }
    }
  }
}

// Reduce partials: out[seq, hq, :] = sum_p w_p * tmp_out[p] / L
__global__ __launch_bounds__(128) void paged_attn_reduce_kernel(
    uint16_t* __restrict__ out, const float* __restrict__ tmp_out,
    const float* __restrict__ tmp_ml, const int* __restrict__ seq_lens,
    int Hq, int D, int partition_size, int max_parts) {
  const int seq = blockIdx.x;
  const int hq = blockIdx.y;
  const int nparts =
      min(max_parts, (seq_lens[seq] + partition_size - 1) / partition_size);
  const float* ml = tmp_ml + ((int64_t)seq * Hq + hq) * max_parts * 2;

  __shared__ float w[MAX_PARTS];
  __shared__ float l_sh;
  if (threadIdx.x == 0) {
    float M = -INFINITY;
    for (int p = 0; p < nparts; ++p) M = fmaxf(M, ml[p * 2]);
    float L = 0.f;
    for (int p = 0; p < nparts; ++p) {
      const float e = (ml[p * 2] == -INFINITY) ? 0.f : __expf(ml[p * 2] - M);
      w[p] = e;
      L += e * ml[p * 2 + 1];
    }
    l_sh = fmaxf(L, 1e-20f);
  }
  __syncthreads();
  const float* tp = tmp_out + ((int64_t)seq * Hq + hq) * max_parts * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float o = 0.f;
    for (int p = 0; p < nparts; ++p) {
      // skip dead partitions explicitly: their tmp_out is uninitialized
      // and 0 * NaN would poison the sum (windowed-out partitions)
      if (w[p] != 0.f) o += w[p] * tp[p * D + d];
    }
    out[((int64_t)seq * Hq + hq) * D + d] = f32_to_bf16(o / l_sh);
  }
}

template <int DHEAD, int G>
void launch_decode(uint16_t* out, float* tmp_out, float* tmp_ml,
                   const uint16_t* q, const uint16_t* kc, const uint16_t* vc,
                   const int* bt, const int* lens, float scale, int B,
                   int Hkv, int bs_log2, int max_blocks, int eff_part,
                   int nparts, int max_parts, int window, bool kv8,
                   hipStream_t stream) {
#define LAUNCH_PD(K8, VPS)                                                   \
  hipLaunchKernelGGL((paged_attn_decode_kernel<DHEAD, G, K8, VPS>),          \
                     dim3(B, Hkv, nparts), dim3(NTHREADS), 0, stream, out,   \
                     tmp_out, tmp_ml, q, kc, vc, bt, lens, scale, Hkv,       \
                     bs_log2, max_blocks, eff_part, max_parts, window)
  // Measured in profiles/r02_decode_kpre.md. A grid under 2048
  // workgroups underfills the chip (256 CUs x 4 SIMDs), so
  // per-wave depth has to replace occupancy-based latency hiding: the
  // 8-deep V staging wins those shapes (4.25-4.29 vs 3.6-3.7 TB/s at
  // B<=64 / L>=2048) but loses the full-grid B=512 headline (27.5k vs
  // 28.1k tok/s).
  if (kv8)                          LAUNCH_PD(true, 4);
  else if (B * Hkv * nparts < 2048) LAUNCH_PD(false, 8);
  else                              LAUNCH_PD(false, 4);
#undef LAUNCH_PD
}

}  // namespace

int64_t decode_part_quant() { return PART_QUANT; }

void paged_attn_decode(torch::Tensor out, torch::Tensor q,
                       torch::Tensor k_cache, torch::Tensor v_cache,
                       torch::Tensor block_tables, torch::Tensor seq_lens,
                       double scale, torch::Tensor tmp_out,
                       torch::Tensor tmp_ml, int64_t max_len,
                       int64_t window) {
  const int B = q.size(0);
  const int Hq = q.size(1);
  const int D = q.size(2);
  const int Hkv = k_cache.size(1);
  const int block_size = k_cache.size(2);
  const int max_blocks = block_tables.size(1);
  const int max_parts = tmp_out.dim() == 4 ? tmp_out.size(2) : 0;
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  const int G = Hq / Hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, "G must be 1/2/4/8");
  TORCH_CHECK(max_len >= 1, "max_len must be >= 1, got ", max_len);
  // the kernel addresses a token with shift and mask, and a chunk's
  // block ids have IDS_MAX slots in LDS
  TORCH_CHECK(block_size >= MIN_BS && (block_size & (block_size - 1)) == 0,
              "KV cache block_size must be a power of two and at least ",
              MIN_BS, ", got ", block_size);
  int bs_log2 = 0;
  while ((1 << bs_log2) < block_size) ++bs_log2;
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
                  out.scalar_type() == torch::kBFloat16,
              "q and out must be bf16");
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(),
              "k_cache and v_cache must share a dtype");
  TORCH_CHECK(block_tables.scalar_type() == torch::kInt32,
              "block_tables must be int32");
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt32,
              "seq_lens must be int32");
  TORCH_CHECK(seq_lens.size(0) == B && block_tables.size(0) == B,
              "seq_lens and block_tables must have B = ", B, " rows");
  TORCH_CHECK(q.is_contiguous() && out.is_contiguous() &&
                  k_cache.is_contiguous() && v_cache.is_contiguous() &&
                  block_tables.is_contiguous() && seq_lens.is_contiguous() &&
                  tmp_out.is_contiguous() && tmp_ml.is_contiguous(),
              "paged_attn_decode takes contiguous tensors");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "q must be 16-byte aligned (it is read with vector loads)");
  TORCH_CHECK(tmp_out.scalar_type() == torch::kFloat32 && max_parts >= 1 &&
                  tmp_out.sizes() == at::IntArrayRef({B, Hq, max_parts, D}),
              "tmp_out must be fp32 [B, Hq, max_parts, D] with B = ", B,
              ", Hq = ", Hq, ", D = ", D, "; got ", tmp_out.sizes());
  TORCH_CHECK(tmp_ml.scalar_type() == torch::kFloat32 &&
                  tmp_ml.sizes() == at::IntArrayRef({B, Hq, max_parts, 2}),
              "tmp_ml must be fp32 [B, Hq, max_parts, 2] with tmp_out's "
              "max_parts = ", max_parts, "; got ", tmp_ml.sizes());

  // split-K sizing: enough workgroups to fill the 256 CUs, never more
  // partitions than the longest row needs, the workspace holds or the
  // reduce kernel's weight array takes
  const int max_useful = cdiv((int)max_len, PART_QUANT);
  int nparts = std::max(1, TARGET_WGS / std::max(1, B * Hkv));
  nparts = std::min({nparts, max_useful, max_parts, MAX_PARTS});
  int eff_part = cdiv(cdiv((int)max_len, nparts), PART_QUANT) * PART_QUANT;
  nparts = cdiv((int)max_len, eff_part);

  auto stream = at::hip::getCurrentHIPStream();
  auto* o = (uint16_t*)out.data_ptr();
  auto* to = tmp_out.data_ptr<float>();
  auto* tm = tmp_ml.data_ptr<float>();
  auto* qp = (const uint16_t*)q.data_ptr();
  auto* kp = (const uint16_t*)k_cache.data_ptr();
  auto* vp = (const uint16_t*)v_cache.data_ptr();
  auto* bp = block_tables.data_ptr<int>();
  auto* lp = seq_lens.data_ptr<int>();

  const bool kv8 = k_cache.scalar_type() == torch::kUInt8;
#define DISPATCH(DH, GG)                                                     \
  launch_decode<DH, GG>(o, to, tm, qp, kp, vp, bp, lp, (float)scale, B,     \
                        Hkv, bs_log2, max_blocks, eff_part, nparts,         \
                        max_parts, (int)window, kv8, stream)
  if (D == 128) {
    if (G == 1) DISPATCH(128, 1);
    else if (G == 2) DISPATCH(128, 2);
    else if (G == 4) DISPATCH(128, 4);
    else DISPATCH(128, 8);
  } else {
    if (G == 1) DISPATCH(64, 1);
    else if (G == 2) DISPATCH(64, 2);
    else if (G == 4) DISPATCH(64, 4);
    else DISPATCH(64, 8);
  }
#undef DISPATCH

  if (nparts > 1) {
    hipLaunchKernelGGL(paged_attn_reduce_kernel, dim3(B, Hq), dim3(128), 0,
                       stream, o, to, tm, lp, Hq, D, eff_part, max_parts);
    // note: dead (windowed-out) partitions wrote ml = -inf and are
    // skipped by the reduce weighting
  }
}
