"""Qwen3 on CPU: the model against a plain-torch Qwen3, HF checkpoint names,
GGUF export / load under the qwen3 architectures, tensor parallelism,
catalogue and admission. The dense model is the preset tiny-qwen3. No
mixture-of-experts Qwen3 preset is served yet; the model and the loaders take
one, which QWEN3_MOE below (a config built here, head_dim 64, 128 experts,
top-8) puts through them."""
import dataclasses
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from helix_amd import ops
from helix_amd.engine import gguf
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.kv_cache import KVCache
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.engine.weights import load_llama_weights
from helix_amd.models.llama import (PRESETS, LlamaForCausalLM, MoEMLP,
                                    PrefillMeta)
from helix_amd.models.quant import KQLinear

# not a preset: the shape of a small Qwen3-MoE, for the model and loaders
QWEN3_MOE = dataclasses.replace(
    PRESETS["tiny-qwen3"], name="qwen3-moe-test", intermediate_size=64,
    num_heads=8, num_kv_heads=2, head_dim=64, num_experts=128,
    experts_per_token=8)
CONFIGS = {"tiny-qwen3": PRESETS["tiny-qwen3"], "qwen3-moe": QWEN3_MOE}
TINY = tuple(CONFIGS)
IDS = [5, 9, 2, 77, 31, 8, 300, 511, 1, 64, 200, 17]


def randomize_qk_norms(model, seed=11):
    """init_random fills every norm weight with 1, where norm-before-rope
    and norm-after-rope coincide: draw the QK-norm weights in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(seed)
    n = 0
    for name, p in model.named_parameters():
        if name.endswith(("q_norm_w", "k_norm_w")):
            p.data.copy_((0.5 + torch.rand(p.shape, generator=g)).to(p.dtype))
            n += 1
    assert n == 2 * model.cfg.num_layers
    return model


def _model(preset, seed=3, dtype=torch.float32):
    m = LlamaForCausalLM(CONFIGS[preset]).to(dtype).init_random(seed)
    return randomize_qk_norms(m)


def _logits(model, ids):
    cfg = model.cfg
    kv = KVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim, 16, 8,
                 torch.device("cpu"), dtype=next(model.parameters()).dtype)
    T = len(ids)
    meta = PrefillMeta(
        cu_seqlens=torch.tensor([0, T], dtype=torch.int32), max_seqlen=T,
        slot_mapping=torch.arange(T, dtype=torch.int64),
        positions=torch.arange(T, dtype=torch.int64))
    with torch.inference_mode():
        h = model(torch.tensor(ids, dtype=torch.int64), kv.caches, meta)
        return model.compute_logits(h)


# -- a plain-torch Qwen3, from the HF formulas -------------------------------

def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def plain_qwen3_logits(model, ids, variant=None):
    """fp32 throughout, except where a bf16 mixture of experts rounds (the
    activation and the layer's output, as ops.reference.moe_experts says):
    without those two, a layer-1 routing decision on a near-tie could differ.
    variant: 'no_qk_norm' / 'norm_after_rope' are deliberately wrong."""
    cfg = model.cfg
    sd = {k: v.detach().float() for k, v in model.named_parameters()}
    Hq, Hkv, D, eps = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, \
        cfg.rms_norm_eps
    T = len(ids)
    pos = torch.arange(T, dtype=torch.float32)
    inv_freq = 1.0 / (cfg.rope_base ** (torch.arange(0, D, 2).float() / D))
    ang = torch.outer(pos, inv_freq)
    emb = torch.cat([ang, ang], dim=-1)
    cos, sin = emb.cos()[:, None], emb.sin()[:, None]          # [T, 1, D]
    x = sd["embed_tokens.weight"][torch.tensor(ids)]
    causal = torch.ones(T, T).tril().bool()
    for i in range(cfg.num_layers):
        pre = f"layers.{i}."
        h = _rms(x, sd[pre + "input_norm_w"], eps)
        qkv = h @ sd[pre + "attn.qkv_proj.weight"].t()
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q, k, v = q.view(T, Hq, D), k.view(T, Hkv, D), v.view(T, Hkv, D)
        qn, kn = sd[pre + "attn.q_norm_w"], sd[pre + "attn.k_norm_w"]

        def rope(t):
            return t * cos + _rotate_half(t) * sin
        if variant == "no_qk_norm":
            q, k = rope(q), rope(k)
        elif variant == "norm_after_rope":
            q, k = _rms(rope(q), qn, eps), _rms(rope(k), kn, eps)
        else:
            q, k = rope(_rms(q, qn, eps)), rope(_rms(k, kn, eps))
        rep = Hq // Hkv
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
        s = torch.einsum("thd,shd->hts", q, k) * D ** -0.5
        s = s.masked_fill(~causal, float("-inf"))
        o = torch.einsum("hts,shd->thd", s.softmax(-1), v).reshape(T, Hq * D)
        x = x + o @ sd[pre + "attn.o_proj.weight"].t()
        h = _rms(x, sd[pre + "post_norm_w"], eps)
        if cfg.num_experts > 0:
            I = cfg.intermediate_size
            p = (h @ sd[pre + "mlp.router_w"].t()).softmax(-1)
            w, idx = p.topk(cfg.experts_per_token, dim=-1)
            w = w / w.sum(-1, keepdim=True)                # norm_topk_prob
            y = torch.zeros_like(h)
            for t in range(T):
                for j in range(cfg.experts_per_token):
                    e = int(idx[t, j])
                    gu = h[t] @ sd[pre + "mlp.w13"][e].t()
                    act = (F.silu(gu[:I]) * gu[I:]).to(torch.bfloat16).float()
                    y[t] += w[t, j] * (act @ sd[pre + "mlp.w2"][e].t())
            y = y.to(torch.bfloat16).float()
        else:
            I = cfg.intermediate_size
            gu = h @ sd[pre + "mlp.gate_up_proj.weight"].t()
            y = (F.silu(gu[:, :I]) * gu[:, I:]) @ \
                sd[pre + "mlp.down_proj.weight"].t()
        x = x + y
    x = _rms(x, sd["final_norm_w"], eps)
    return x @ sd["lm_head.weight"].t()


@pytest.mark.parametrize("preset", TINY)
def test_model_matches_plain_torch_qwen3(preset):
    """Both sides compute in fp32 from the same weights, so the dense model
    differs by summation order alone (~1e-6). In the mixture of experts an
    fp32 difference can flip a bf16 rounding of the layer output: one bf16
    ulp of a value of ~0.01 is 4e-5, and the final norm scales the stream
    up by a few. Hence 1e-3 relative, 5e-4 absolute on logits of ~0.3 to 1.
    The deliberately wrong references miss by 1e-2 at the least."""
    model = _model(preset)
    cfg = model.cfg
    assert cfg.qk_norm
    got = _logits(model, IDS)
    want = plain_qwen3_logits(model, IDS)
    print(f"{preset}: max |diff| {float((got - want).abs().max()):.3g}, "
          f"max |logit| {float(want.abs().max()):.3g}")
    torch.testing.assert_close(got, want, rtol=1e-3, atol=5e-4)
    for variant in ("no_qk_norm", "norm_after_rope"):
        wrong = plain_qwen3_logits(model, IDS, variant)
        assert float((got - wrong).abs().max()) > 1e-2, variant


def test_presets_and_parameters():
    for name in ("qwen3-8b", "qwen3-32b"):
        c = PRESETS[name]
        assert (c.vocab_size, c.rms_norm_eps, c.rope_base, c.max_position,
                c.tie_embeddings, c.attention_bias, c.qk_norm, c.head_dim) \
            == (151936, 1e-6, 1e6, 40960, False, False, True, 128)
    c = PRESETS["qwen3-8b"]
    assert (c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads,
            c.intermediate_size, c.num_experts) == (4096, 36, 32, 8, 12288, 0)
    c = PRESETS["qwen3-32b"]
    assert (c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads,
            c.intermediate_size, c.q_size) == (5120, 64, 64, 8, 25600, 8192)
    assert {CONFIGS[n].head_dim for n in TINY} == {64, 128}
    m = LlamaForCausalLM(PRESETS["tiny-qwen3"]).init_random(0)
    a = m.layers[0].attn
    assert a.q_norm_w.shape == (128,) and a.k_norm_w.shape == (128,)
    assert bool((a.q_norm_w == 1).all()) and bool((a.k_norm_w == 1).all())
    assert isinstance(LlamaForCausalLM(QWEN3_MOE).layers[0].mlp, MoEMLP)
    # models without QK-norm own no such parameter
    assert not any("q_norm" in n or "k_norm" in n for n, _ in
                   LlamaForCausalLM(PRESETS["tiny"]).named_parameters())


# -- HF checkpoint names -----------------------------------------------------

@pytest.mark.parametrize("preset", TINY)
def test_checkpoint_round_trip_hf_qwen3_names(preset, tmp_path):
    from safetensors.torch import save_file
    cfg = CONFIGS[preset]
    src = _model(preset, dtype=torch.bfloat16)
    I, q, kv = cfg.intermediate_size, cfg.q_size, cfg.kv_size
    sd = {"model.embed_tokens.weight": src.embed_tokens.weight,
          "model.norm.weight": src.final_norm_w,
          "lm_head.weight": src.lm_head.weight}
    for i, layer in enumerate(src.layers):
        pre = f"model.layers.{i}."
        qkv = layer.attn.qkv_proj.weight
        sd[pre + "input_layernorm.weight"] = layer.input_norm_w
        sd[pre + "post_attention_layernorm.weight"] = layer.post_norm_w
        sd[pre + "self_attn.q_proj.weight"] = qkv[:q]
        sd[pre + "self_attn.k_proj.weight"] = qkv[q:q + kv]
        sd[pre + "self_attn.v_proj.weight"] = qkv[q + kv:]
        sd[pre + "self_attn.o_proj.weight"] = layer.attn.o_proj.weight
        sd[pre + "self_attn.q_norm.weight"] = layer.attn.q_norm_w
        sd[pre + "self_attn.k_norm.weight"] = layer.attn.k_norm_w
        if cfg.num_experts > 0:
            sd[pre + "mlp.gate.weight"] = layer.mlp.router_w
            for e in range(cfg.num_experts):
                ex = pre + f"mlp.experts.{e}."
                sd[ex + "gate_proj.weight"] = layer.mlp.w13[e, :I]
                sd[ex + "up_proj.weight"] = layer.mlp.w13[e, I:]
                sd[ex + "down_proj.weight"] = layer.mlp.w2[e]
        else:
            gu = layer.mlp.gate_up_proj.weight
            sd[pre + "mlp.gate_proj.weight"] = gu[:I]
            sd[pre + "mlp.up_proj.weight"] = gu[I:]
            sd[pre + "mlp.down_proj.weight"] = layer.mlp.down_proj.weight
    save_file({n: t.detach().clone().contiguous() for n, t in sd.items()},
              str(tmp_path / "model.safetensors"))
    dst = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(4)
    assert load_llama_weights(dst, str(tmp_path)) == len(sd)
    want, got = dict(src.named_parameters()), dict(dst.named_parameters())
    assert set(got) == set(want)
    for name in want:
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(_logits(dst, IDS), _logits(src, IDS))


# -- GGUF ---------------------------------------------------------------------

@pytest.mark.parametrize("preset, arch", [("tiny-qwen3", "qwen3"),
                                          ("qwen3-moe", "qwen3moe")])
def test_gguf_round_trip_bf16(preset, arch, tmp_path):
    cfg = CONFIGS[preset]
    src = _model(preset, dtype=torch.bfloat16)
    path = str(tmp_path / "m.gguf")
    n = gguf.export_model_gguf(src, path)
    g = gguf.GGUFFile(path)
    assert g.arch() == arch and len(g.tensors) == n
    md = g.metadata
    assert md[f"{arch}.attention.key_length"] == cfg.head_dim
    assert md[f"{arch}.attention.value_length"] == cfg.head_dim
    assert md[f"{arch}.attention.head_count"] == cfg.num_heads
    assert md[f"{arch}.block_count"] == cfg.num_layers
    assert abs(md[f"{arch}.attention.layer_norm_rms_epsilon"]
               - cfg.rms_norm_eps) < 1e-9
    assert not any(k.startswith("llama.") for k in md)
    if cfg.num_experts:
        assert md[f"{arch}.expert_count"] == 128
        assert md[f"{arch}.expert_used_count"] == 8
        assert md[f"{arch}.expert_feed_forward_length"] == 64
    q, kv = cfg.q_size, cfg.kv_size
    for i, layer in enumerate(src.layers):
        w = layer.attn.qkv_proj.weight
        # rows as the model holds them: not permuted
        assert torch.equal(g.load_tensor(f"blk.{i}.attn_q.weight"), w[:q])
        assert torch.equal(g.load_tensor(f"blk.{i}.attn_k.weight"),
                           w[q:q + kv])
        assert torch.equal(g.load_tensor(f"blk.{i}.attn_q_norm.weight"),
                           layer.attn.q_norm_w)
        assert torch.equal(g.load_tensor(f"blk.{i}.attn_k_norm.weight"),
                           layer.attn.k_norm_w)
    dst = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(4)
    assert gguf.load_gguf_weights(dst, path) == n
    want, got = dict(src.named_parameters()), dict(dst.named_parameters())
    for name in want:
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(_logits(dst, IDS), _logits(src, IDS))


def _rewrite_as_llama(src_path, dst_path, cfg):
    """The same tensors, unpermuted, under a llama architecture key."""
    g = gguf.GGUFFile(src_path)
    meta = {"general.architecture": "llama",
            "llama.block_count": cfg.num_layers,
            "llama.embedding_length": cfg.hidden_size,
            "llama.attention.head_count": cfg.num_heads,
            "llama.attention.head_count_kv": cfg.num_kv_heads}
    gguf.write_gguf(dst_path, meta,
                    {n: g.load_tensor(n) for n in g.tensors})


def test_architecture_key_decides_the_permutation(tmp_path):
    cfg = PRESETS["tiny-qwen3"]
    src = _model("tiny-qwen3", dtype=torch.bfloat16)
    qpath, lpath = str(tmp_path / "q.gguf"), str(tmp_path / "l.gguf")
    gguf.export_model_gguf(src, qpath)
    _rewrite_as_llama(qpath, lpath, cfg)
    dst = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(4)
    gguf.load_gguf_weights(dst, lpath)
    q, kv = cfg.q_size, cfg.kv_size
    for s, d in zip(src.layers, dst.layers):
        ws, wd = s.attn.qkv_proj.weight, d.attn.qkv_proj.weight
        assert not torch.equal(wd[:q], ws[:q])
        assert not torch.equal(wd[q:q + kv], ws[q:q + kv])
        assert torch.equal(wd[:q], gguf.unpermute_rope(ws[:q], cfg.num_heads))
        assert torch.equal(wd[q:q + kv], gguf.unpermute_rope(
            ws[q:q + kv], cfg.num_kv_heads))
        assert torch.equal(wd[q + kv:], ws[q + kv:])
        assert torch.equal(d.attn.q_norm_w, s.attn.q_norm_w)
    # a llama model still exports permuted, under llama keys
    lsrc = LlamaForCausalLM(PRESETS["tiny"]).init_random(1)
    tpath = str(tmp_path / "t.gguf")
    gguf.export_model_gguf(lsrc, tpath)
    gt = gguf.GGUFFile(tpath)
    assert gt.arch() == "llama"
    assert "llama.attention.key_length" not in gt.metadata
    assert not torch.equal(gt.load_tensor("blk.0.attn_q.weight"),
                           lsrc.layers[0].attn.qkv_proj.weight[:256])


def test_estimate_gguf_bytes_honours_key_length(tmp_path):
    cfg = PRESETS["tiny-qwen3"]
    src = _model("tiny-qwen3", dtype=torch.bfloat16)
    qpath, lpath = str(tmp_path / "q.gguf"), str(tmp_path / "l.gguf")
    gguf.export_model_gguf(src, qpath)
    _rewrite_as_llama(qpath, lpath, cfg)
    per_tok = 2 * cfg.num_layers * cfg.num_kv_heads * 2
    est = gguf.estimate_gguf_bytes(qpath, kv_tokens=100)
    assert est["kv"] == per_tok * 128 * 100
    assert est["total"] == est["weights"] + est["kv"]
    # no key_length: n_embd / n_head as before (256 / 4)
    assert gguf.estimate_gguf_bytes(lpath, kv_tokens=100)["kv"] == \
        per_tok * 64 * 100


@pytest.fixture(scope="module")
def q4_k_m_file(tmp_path_factory):
    """`helix export-gguf --preset tiny-qwen3 --quant q4_k_m`, the CLI."""
    path = str(tmp_path_factory.mktemp("qwen3") / "tiny-qwen3-q4_k_m.gguf")
    r = subprocess.run(
        [sys.executable, "-m", "helix_amd.cli", "export-gguf", "--preset",
         "tiny-qwen3", "-o", path, "--seed", "3", "--quant", "q4_k_m"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return path


def test_dense_q4_k_m_stays_resident(q4_k_m_file):
    """As tests/test_kq_cpu.py for `tiny`: KQLinear projections holding the
    file's blocks, and logits equal to the dequantised load's."""
    cfg = PRESETS["tiny-qwen3"]
    g = gguf.GGUFFile(q4_k_m_file)
    assert g.arch() == "qwen3"
    assert g.tensors["blk.0.attn_q.weight"].type_name == "Q4_K"
    assert g.tensors["blk.0.attn_q_norm.weight"].type_name == "F32"
    dense = LlamaForCausalLM(cfg)
    assert gguf.load_gguf_weights(dense, q4_k_m_file) == len(g.tensors)
    res = LlamaForCausalLM(cfg)
    assert gguf.load_gguf_weights(res, q4_k_m_file, keep_quantized=True) \
        == len(g.tensors)
    for layer in res.layers:
        for m in (layer.attn.qkv_proj, layer.attn.o_proj,
                  layer.mlp.gate_up_proj, layer.mlp.down_proj):
            assert isinstance(m, KQLinear)
        assert isinstance(layer.attn.q_norm_w, torch.nn.Parameter)
        assert layer.attn.q_norm_w.shape == (cfg.head_dim,)
        # Q rows are the file's own blocks, in the file's order
        raw = g.read_raw("blk.0.attn_q.weight")
    assert ops.pack_ggml_kq(res.layers[0].attn.qkv_proj.planes(0),
                            "q4_k") == raw
    assert torch.equal(_logits(dense, IDS), _logits(res, IDS))
    # served in bf16, the norm weights are bf16 tensors
    res16 = res.to(torch.bfloat16)
    assert res16.layers[0].attn.k_norm_w.dtype == torch.bfloat16
    eng = LLMEngine(EngineConfig(model="tiny-qwen3", max_model_len=256,
                                 max_num_seqs=4, kv_cache_blocks=64,
                                 eos_token_id=-1), device="cpu", model=res16)
    out = eng.generate([IDS], SamplingParams(temperature=0.0, max_tokens=4,
                                             ignore_eos=True))
    assert len(out[0]) == 4


def test_moe_q4_0_experts_stay_resident(tmp_path):
    cfg = QWEN3_MOE
    src = _model("qwen3-moe", dtype=torch.bfloat16)
    path = str(tmp_path / "moe.gguf")
    n = gguf.export_model_gguf(src, path, quant="q4_0")
    g = gguf.GGUFFile(path)
    assert g.arch() == "qwen3moe"
    assert g.tensors["blk.0.ffn_gate_exps.weight"].type_name == "Q4_0"
    assert tuple(g.tensors["blk.0.ffn_down_exps.weight"].shape) == \
        (128, cfg.hidden_size, cfg.intermediate_size)
    dense = LlamaForCausalLM(cfg).to(torch.bfloat16)
    assert gguf.load_gguf_weights(dense, path) == n
    res = LlamaForCausalLM(cfg).to(torch.bfloat16)
    assert gguf.load_gguf_weights(res, path, keep_quantized=True) == n
    for layer in res.layers:
        assert layer.mlp.expert_fmt == ("q4_0", "q4_0")
        assert "w13" not in dict(layer.mlp.named_parameters())
    assert all(l.mlp.expert_fmt is None for l in dense.layers)
    a, b = _logits(dense, IDS).float(), _logits(res, IDS).float()
    # the same Q4_0 weights, dequantised up front or in the routed GEMM
    assert float((a - b).norm() / a.norm()) < 0.02


# -- tensor parallelism ------------------------------------------------------

def test_tp2_matches_single_process():
    from test_parallel import _spawn2, _tp_worker
    cfg = PRESETS["tiny-qwen3"]
    torch.manual_seed(42)
    lens = [9, 5]
    T = sum(lens)
    ids = torch.randint(0, cfg.vocab_size, (T,))
    positions = torch.cat([torch.arange(l) for l in lens])
    cu = torch.tensor([0, lens[0], T], dtype=torch.int32)
    model = _model("tiny-qwen3", seed=0)
    meta = PrefillMeta(cu_seqlens=cu, max_seqlen=max(lens),
                       slot_mapping=torch.full((T,), -1, dtype=torch.int64),
                       positions=positions)
    full = model.compute_logits(model(ids, None, meta))
    sd = model.state_dict()
    assert "layers.0.attn.q_norm_w" in sd
    with tempfile.TemporaryDirectory() as td:
        out_path = os.path.join(td, "logits.pt")
        _spawn2(_tp_worker,
                lambda r, port: (r, 2, "tiny-qwen3", ids, positions, cu,
                                 max(lens), sd, out_path, port))
        tp_logits = torch.load(out_path)
    torch.testing.assert_close(tp_logits, full, atol=2e-3, rtol=2e-3)


# -- serving plumbing ---------------------------------------------------------

def test_catalogue_and_specs():
    from helix_amd.runner.service import DEFAULT_SPECS, estimate_model_bytes
    from helix_amd.server.models_catalog import (ModelCatalog,
                                                 resolve_model_name)
    from helix_amd.store import Store
    cat = ModelCatalog(Store(":memory:"))
    for alias, want in (("qwen3:8b", "qwen3-8b"), ("qwen3:32b", "qwen3-32b"),
                        ("Qwen/Qwen3-8B", "qwen3-8b"),
                        ("Qwen/Qwen3-32B", "qwen3-32b")):
        assert resolve_model_name(alias) == want
        info = cat.get(alias)
        assert info == cat.get(want)
        assert info["family"] == "qwen" and info["kind"] == "chat"
        assert info["context_length"] == 40960
        assert set(info) == set(cat.get("llama3-8b"))
    for name in ("qwen3-8b", "qwen3-32b", "tiny-qwen3"):
        spec = DEFAULT_SPECS[name]
        assert spec.preset == name and spec.kind == "llm"
        assert estimate_model_bytes(spec) > 0
    for name in ("tiny-qwen3",):
        assert DEFAULT_SPECS[name].max_model_len == 256
        assert DEFAULT_SPECS[name].kv_cache_blocks == 256
        m = LlamaForCausalLM(PRESETS[name]).to(torch.bfloat16)
        assert estimate_model_bytes(DEFAULT_SPECS[name]) >= m.memory_bytes()
    # parameters in bf16: ~8.2 G, ~32.8 G
    for name, lo, hi in (("qwen3-8b", 16e9, 17e9), ("qwen3-32b", 65e9, 66e9)):
        c = PRESETS[name]
        mlp = 3 * c.hidden_size * c.intermediate_size
        if c.num_experts:
            mlp = c.num_experts * (mlp + c.hidden_size)
        params = 2 * c.vocab_size * c.hidden_size + c.num_layers * (
            c.hidden_size * (c.q_size + 2 * c.kv_size)
            + c.q_size * c.hidden_size + mlp)
        assert lo < 2 * params < hi, (name, 2 * params)
        assert estimate_model_bytes(DEFAULT_SPECS[name]) > 2 * params


def test_tiny_engine_generates(preset="tiny-qwen3"):
    cfg = EngineConfig(model=preset, max_model_len=256, max_num_seqs=8,
                       kv_cache_blocks=128, eos_token_id=-1, seed=2)
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    eng = LLMEngine(cfg, device="cpu")
    assert eng.model.layers[0].attn.q_norm_w is not None
    out = eng.generate([[1, 2, 3, 4, 5], [7, 8, 9]], sp)
    assert all(len(o) == 8 for o in out)
    assert out == LLMEngine(cfg, device="cpu").generate(
        [[1, 2, 3, 4, 5], [7, 8, 9]], sp)
