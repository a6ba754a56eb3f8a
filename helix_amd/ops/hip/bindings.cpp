// Python bindings for the helix_amd CDNA4 kernel library.
#include <torch/extension.h>

void rms_norm(torch::Tensor out, torch::Tensor x, torch::Tensor w, double eps);
void fused_add_rms_norm(torch::Tensor x, torch::Tensor residual,
                        torch::Tensor w, double eps);
void layer_norm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                torch::Tensor b, double eps);
void rotary_embedding(torch::Tensor positions, torch::Tensor q,
                      torch::Tensor k, torch::Tensor cos_sin,
                      int64_t head_dim);
void silu_and_mul(torch::Tensor out, torch::Tensor x);
void rope_qkv_cache(torch::Tensor positions, torch::Tensor qkv,
                    torch::Tensor q_out,
                    c10::optional<torch::Tensor> k_cache,
                    c10::optional<torch::Tensor> v_cache,
                    c10::optional<torch::Tensor> slot_mapping,
                    c10::optional<torch::Tensor> k_out,
                    c10::optional<torch::Tensor> v_out,
                    torch::Tensor cos_sin, int64_t num_q_heads,
                    int64_t num_kv_heads, int64_t head_dim);
void rope_qkv_norm_cache(torch::Tensor positions, torch::Tensor qkv,
                         torch::Tensor q_out,
                         c10::optional<torch::Tensor> k_cache,
                         c10::optional<torch::Tensor> v_cache,
                         c10::optional<torch::Tensor> slot_mapping,
                         c10::optional<torch::Tensor> k_out,
                         c10::optional<torch::Tensor> v_out,
                         torch::Tensor cos_sin, int64_t num_q_heads,
                         int64_t num_kv_heads, int64_t head_dim,
                         torch::Tensor q_norm_w, torch::Tensor k_norm_w,
                         double eps);
void gelu_tanh(torch::Tensor out, torch::Tensor x);
void reshape_and_cache(torch::Tensor k, torch::Tensor v,
                       torch::Tensor k_cache, torch::Tensor v_cache,
                       torch::Tensor slot_mapping);
void paged_attn_decode(torch::Tensor out, torch::Tensor q,
                       torch::Tensor k_cache, torch::Tensor v_cache,
                       torch::Tensor block_tables, torch::Tensor seq_lens,
                       double scale, torch::Tensor tmp_out,
                       torch::Tensor tmp_ml, int64_t max_len,
                       int64_t window);
int64_t decode_part_quant();
void attn_prefill(torch::Tensor out, torch::Tensor q, torch::Tensor k,
                  torch::Tensor v, torch::Tensor cu_seqlens,
                  torch::Tensor cu_seqlens_k, int64_t max_seqlen,
                  double scale, bool causal, int64_t window);
void sample_tokens(torch::Tensor out, torch::Tensor logits,
                   torch::Tensor temperatures, torch::Tensor seeds);
void sample_tokens_ext(torch::Tensor out, torch::Tensor logits,
                       torch::Tensor temperatures, torch::Tensor seeds,
                       torch::Tensor top_p, torch::Tensor top_k,
                       torch::Tensor rep_pen, torch::Tensor pres_pen,
                       torch::Tensor freq_pen,
                       c10::optional<torch::Tensor> counts,
                       c10::optional<torch::Tensor> seen,
                       c10::optional<torch::Tensor> row_map);
void gemm_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w,
               c10::optional<torch::Tensor> bias, int64_t act);
void gemm_skinny_bf16(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                      c10::optional<torch::Tensor> bias,
                      c10::optional<torch::Tensor> scratch, int64_t split_k,
                      int64_t act, int64_t swizzle);
void gemm_fp8(torch::Tensor out, torch::Tensor x, torch::Tensor w,
              torch::Tensor x_scale, torch::Tensor w_scale,
              c10::optional<torch::Tensor> bias, int64_t act);
void lora_shrink(torch::Tensor y, torch::Tensor x, torch::Tensor A,
                 torch::Tensor slot);
void lora_expand(torch::Tensor out, torch::Tensor y, torch::Tensor B,
                 torch::Tensor slot, torch::Tensor scale,
                 std::vector<int64_t> n_off);
void gemm_wq(torch::Tensor out, torch::Tensor x, torch::Tensor qs,
             torch::Tensor d, c10::optional<torch::Tensor> bias,
             int64_t bits);
void dequant_wq(torch::Tensor out, torch::Tensor qs, torch::Tensor d,
                int64_t bits);
int64_t wq_kernel_max_m();
void gemm_kq(torch::Tensor out, int64_t col_off, torch::Tensor x,
             std::vector<torch::Tensor> planes,
             c10::optional<torch::Tensor> bias, std::string fmt);
void dequant_kq(torch::Tensor out, std::vector<torch::Tensor> planes,
                std::string fmt);
int64_t kq_kernel_max_m();
int64_t kq_waves(int64_t N, int64_t K);
void moe_route(torch::Tensor topk_ids, torch::Tensor topk_w,
               torch::Tensor logits);
void moe_align(torch::Tensor expert_off, torch::Tensor sorted_pairs,
               torch::Tensor topk_ids, int64_t E);
void moe_gemm_gated(torch::Tensor act, torch::Tensor x, torch::Tensor w13,
                    torch::Tensor expert_off, torch::Tensor sorted_pairs,
                    int64_t k);
void moe_gemm_down(torch::Tensor ypair, torch::Tensor act, torch::Tensor w2,
                   torch::Tensor topk_w, torch::Tensor expert_off,
                   torch::Tensor sorted_pairs);
void moe_combine(torch::Tensor out, torch::Tensor ypair, int64_t k);
void moe_gemm_gated_wq(torch::Tensor act, torch::Tensor x,
                       torch::Tensor w13_qs, torch::Tensor w13_d, int64_t bits,
                       torch::Tensor expert_off, torch::Tensor sorted_pairs,
                       int64_t k);
void moe_gemm_down_wq(torch::Tensor ypair, torch::Tensor act,
                      torch::Tensor w2_qs, torch::Tensor w2_d, int64_t bits,
                      torch::Tensor topk_w, torch::Tensor expert_off,
                      torch::Tensor sorted_pairs);
int64_t moe_waves(int64_t N, int64_t K, bool gated);
void moe_gemm_gated_kq(torch::Tensor act, torch::Tensor x,
                       std::vector<torch::Tensor> w13_planes, std::string fmt,
                       torch::Tensor expert_off, torch::Tensor sorted_pairs,
                       int64_t k);
void moe_gemm_down_kq(torch::Tensor ypair, torch::Tensor act,
                      std::vector<torch::Tensor> w2_planes, std::string fmt,
                      torch::Tensor topk_w, torch::Tensor expert_off,
                      torch::Tensor sorted_pairs);
int64_t moe_kq_waves(int64_t N, int64_t K, bool gated);
int64_t moe_max_experts();
int64_t moe_max_topk();
int64_t moe_chunk_pairs();
void mfma_probe(torch::Tensor d, torch::Tensor a, torch::Tensor b);
torch::Tensor ar_create(int64_t world, int64_t rank, int64_t capacity);
void ar_open(std::vector<torch::Tensor> handles);
int64_t ar_capacity();
void ar_allreduce(torch::Tensor inp, torch::Tensor out);
void ar_destroy();
void mfma_probe_fp8(torch::Tensor d, torch::Tensor a, torch::Tensor b,
                    int64_t scale_a, int64_t scale_b);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rms_norm", &rms_norm, "RMSNorm (bf16, CDNA4)");
  m.def("fused_add_rms_norm", &fused_add_rms_norm,
        "Fused residual-add + RMSNorm (in-place)");
  m.def("layer_norm", &layer_norm, "LayerNorm (bf16)");
  m.def("rotary_embedding", &rotary_embedding,
        "Apply rotary embedding to q,k in-place");
  m.def("silu_and_mul", &silu_and_mul, "Fused SiLU-gated multiply");
  m.def("rope_qkv_cache", &rope_qkv_cache,
        "Fused strided-QKV rope + paged-cache write");
  m.def("rope_qkv_norm_cache", &rope_qkv_norm_cache,
        "rope_qkv_cache with a per-head RMSNorm of Q and K before the rope "
        "(Qwen3 QK-norm), head_dim 64 or 128");
  m.def("gelu_tanh", &gelu_tanh, "GELU (tanh approx)");
  m.def("reshape_and_cache", &reshape_and_cache,
        "Scatter K/V rows into paged cache");
  m.def("paged_attn_decode", &paged_attn_decode,
        "Paged decode attention (GQA, flash-decoding partitions)");
  m.attr("DECODE_PART_QUANT") = decode_part_quant();
  m.def("attn_prefill", &attn_prefill,
        "Varlen causal flash prefill attention (MFMA)");
  m.def("sample_tokens", &sample_tokens, "Greedy/Gumbel token sampling");
  m.def("sample_tokens_ext", &sample_tokens_ext,
        "Fused top-k/top-p/penalty Gumbel sampling (histogram threshold)");
  m.def("gemm_bf16", &gemm_bf16, "MFMA bf16 GEMM: x @ w^T (+bias, act)");
  m.def("gemm_skinny_bf16", &gemm_skinny_bf16,
        "Skinny-M decode GEMM: split-K + XCD-chunked tile swizzle");
  m.def("gemm_fp8", &gemm_fp8,
        "MX-fp8 e4m3 MFMA GEMM with epilogue per-row/col dequant");
  m.def("lora_shrink", &lora_shrink,
        "Multi-LoRA shrink: y[t] = A[slot[t]] @ x[t] (fp32 out)");
  m.def("lora_expand", &lora_expand,
        "Multi-LoRA expand: out[t] += scale[s] * B[s] @ y[t] (in place)");
  m.def("gemm_wq", &gemm_wq,
        "Q4_0/Q8_0 weight-only GEMM, dequant fused into the MFMA loop (M <= 64)");
  m.def("dequant_wq", &dequant_wq,
        "Q4_0/Q8_0 planes -> bf16 [N,K] into a caller buffer");
  m.attr("WQ_KERNEL_MAX_M") = wq_kernel_max_m();
  m.def("gemm_kq", &gemm_kq,
        "Q4_K/Q6_K weight-only GEMM into out[:, col_off:col_off+N], dequant "
        "fused into the MFMA loop (M <= 32)");
  m.def("dequant_kq", &dequant_kq,
        "Q4_K/Q6_K planes -> bf16 [N,K] into a caller buffer");
  m.def("kq_waves", &kq_waves,
        "K-split factor (waves per workgroup) gemm_kq uses for a [N,K] weight");
  m.attr("KQ_KERNEL_MAX_M") = kq_kernel_max_m();
  m.def("moe_route", &moe_route,
        "MoE routing: fp32 softmax, top-k (ties to the lower expert), "
        "renormalised weights");
  m.def("moe_align", &moe_align,
        "MoE pair lists: expert_off[E+1] and per-expert ascending pair ids");
  m.def("moe_gemm_gated", &moe_gemm_gated,
        "Routed expert GEMM 1: act[p] = silu(x[p/k] @ gate_e^T) * (x[p/k] @ "
        "up_e^T)");
  m.def("moe_gemm_down", &moe_gemm_down,
        "Routed expert GEMM 2: ypair[p] = topk_w[p] * (act[p] @ w2_e^T), fp32");
  m.def("moe_combine", &moe_combine,
        "out[t] = bf16(sum over slots of ypair[t*k + j]), fixed order");
  m.def("moe_gemm_gated_wq", &moe_gemm_gated_wq,
        "Routed expert GEMM 1 over Q4_0/Q8_0 expert planes, dequant fused "
        "into the MFMA loop");
  m.def("moe_gemm_down_wq", &moe_gemm_down_wq,
        "Routed expert GEMM 2 over Q4_0/Q8_0 expert planes, fp32 ypair");
  m.def("moe_waves", &moe_waves,
        "K-split factor (waves per workgroup) moe_gemm uses for one expert's "
        "[N, K] weight");
  m.def("moe_gemm_gated_kq", &moe_gemm_gated_kq,
        "Routed expert GEMM 1 over Q4_K/Q6_K expert planes, dequant fused "
        "into the MFMA loop");
  m.def("moe_gemm_down_kq", &moe_gemm_down_kq,
        "Routed expert GEMM 2 over Q4_K/Q6_K expert planes, fp32 ypair");
  m.def("moe_kq_waves", &moe_kq_waves,
        "K-split factor (waves per workgroup) moe_gemm_*_kq uses for one "
        "expert's [N, K] weight");
  m.attr("MOE_MAX_EXPERTS") = moe_max_experts();
  m.attr("MOE_MAX_TOPK") = moe_max_topk();
  m.attr("MOE_CHUNK_PAIRS") = moe_chunk_pairs();
  m.def("mfma_probe", &mfma_probe, "16x16x32 MFMA layout probe");
  m.def("ar_create", &ar_create,
        "Allocate one-shot allreduce mailbox; returns IPC handle bytes");
  m.def("ar_open", &ar_open, "Map peer mailboxes from IPC handles");
  m.def("ar_capacity", &ar_capacity, "Opened AR data capacity in bytes");
  m.def("ar_allreduce", &ar_allreduce,
        "One-shot bf16 allreduce over xGMI peer mailboxes");
  m.def("ar_destroy", &ar_destroy, "Tear down the allreduce context");
  m.def("mfma_probe_fp8", &mfma_probe_fp8,
        "16x16x128 MX-fp8 MFMA layout probe (unity e8m0 scales)");
}
