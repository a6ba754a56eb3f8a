"""Mixture-of-experts serving on CPU: the test oracle itself (tolerance,
mutants), the torch reference ops, the tiny-moe model, checkpoint names,
admission estimate, engine guards and catalogue aliases."""
import functools
from collections import defaultdict

import pytest
import torch

import helix_amd.ops as ops
import moe_oracle as mo
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import LlamaForCausalLM, MoEMLP, PRESETS


@functools.lru_cache(maxsize=None)
def _result(case):
    """(emulation error, {mutant: error}) of one case, each the worst row."""
    b = mo.build(case)
    err = float(mo.wq_error(mo.emulate(b, case.k), b.want).max())
    muts = {n: float(mo.wq_error(o, b.want).max())
            for n, o in mo.mutant_outputs(case, b).items()}
    return err, muts


def test_tolerance():
    """TOL_MOE = 4 x the worst emulation error over all cases (within
    rounding of the constant), and every mutant misses it on every case it
    applies to. Prints the mutant / tol table."""
    res = [_result(c) for c in mo.CASES]
    worst, wcase = max(zip((r[0] for r in res), mo.CASES), key=lambda p: p[0])
    table = defaultdict(list)
    for c, r in zip(mo.CASES, res):
        for n, v in r[1].items():
            table[n].append((v, c))
    print(f"worst emulation error {worst:.5f} ({wcase.id}), "
          f"TOL_MOE {mo.TOL_MOE}")
    print(f"{'mutant':24s} {'cases':>5s} {'min err':>9s} {'x tol':>7s}  at")
    for n in mo.MUTANTS:
        v, c = min(table[n], key=lambda p: p[0])
        print(f"{n:24s} {len(table[n]):5d} {v:9.4f} {v / mo.TOL_MOE:7.1f}  "
              f"{c.id}")
    assert set(table) == set(mo.MUTANTS)
    assert 4 * worst <= mo.TOL_MOE * 1.02, worst
    assert mo.TOL_MOE <= 4 * worst * 1.10, worst
    for n in mo.MUTANTS:
        v, c = min(table[n], key=lambda p: p[0])
        assert v > mo.TOL_MOE, (n, c.id, v)


def test_mutant_fails_the_assertion():
    """The mutants fail assert_wq_close itself, the assertion the GPU tests
    use, not only a number next to it."""
    case = mo.Case(8, 2, 256, 256, 65, "skewed")
    b = mo.build(case)
    mo.assert_wq_close(mo.emulate(b, case.k), b.want, mo.TOL_MOE)
    outs = mo.mutant_outputs(case, b)
    assert set(outs) == set(mo.MUTANTS)
    for name, o in outs.items():
        with pytest.raises(AssertionError, match="error"):
            mo.assert_wq_close(o, b.want, mo.TOL_MOE, name)


def test_case_lists_cover_the_mechanisms():
    """Skewed lists have the lengths that cross the tile and chunk edges;
    sparse cases leave experts empty; some uniform list is longer than one
    chunk."""
    skew = {int(mo.build(c).counts.max()) for c in mo.CASES
            if c.family == "skewed" and (c.E, c.k) == (8, 2)}
    assert {1, 16, 17, 64, 65, 130} <= skew
    assert all(int((mo.build(c).counts == 0).sum()) * 2 >= c.E
               for c in mo.CASES if c.family == "sparse")
    assert len(mo.CASES) == len(mo.SHAPES) * len(mo.TS) * len(mo.FAMILIES)


CPU_CASES = [c for c in mo.CASES if c.T in (1, 17, 130)]


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_ops_cpu_match_oracle(case):
    b = mo.build(case)
    ids, w = ops.moe_route(b.logits, case.k)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert torch.equal(ids.long(), b.ids)
    _, w64 = mo.route_ref(b.logits, case.k)
    assert torch.allclose(w.double(), w64, rtol=1e-5, atol=0)
    off, pairs = ops.moe_align(ids, case.E)
    assert off.dtype == torch.int32 and pairs.dtype == torch.int32
    assert torch.equal(off[1:] - off[:-1], b.counts.to(torch.int32))
    for e, want in enumerate(mo.align_ref(b.ids, case.E)):
        assert torch.equal(pairs[off[e]:off[e + 1]].long(), want)
    out = ops.moe_experts(b.x, b.w13, b.w2, ids, w)
    assert out.dtype == torch.bfloat16
    mo.assert_wq_close(out, b.want, mo.TOL_MOE, case.id)
    out2 = ops.moe_forward(b.x, b.logits, b.w13, b.w2, case.k)
    assert torch.equal(out, out2)


def test_align_ascending_and_drops_bad_ids():
    g = torch.Generator().manual_seed(5)
    E, T, k = 8, 37, 2
    ids = torch.randint(0, E, (T, k), generator=g, dtype=torch.int32)
    ids[3, 1] = -1
    ids[10, 0] = E
    ids[36, 1] = 1 << 20
    off, pairs = ops.moe_align(ids, E)
    assert int(off[0]) == 0 and int(off[E]) == T * k - 3
    listed = pairs[:int(off[E])].long()
    for e in range(E):
        p = pairs[off[e]:off[e + 1]].long()
        assert torch.all(p[1:] > p[:-1])
        assert torch.all(ids.reshape(-1)[p] == e)
    assert sorted(listed.tolist()) == [
        p for p in range(T * k) if 0 <= int(ids.reshape(-1)[p]) < E]


def test_route_ties_go_to_the_lower_expert():
    logits = torch.zeros(3, 8, dtype=torch.bfloat16)
    logits[1, 5] = 1.0
    logits[2, 6] = logits[2, 2] = 2.0
    ids, w = ops.moe_route(logits, 3)
    assert ids.tolist() == [[0, 1, 2], [5, 0, 1], [2, 6, 0]]
    assert torch.allclose(w.sum(-1), torch.ones(3))
    assert torch.allclose(w[0], torch.full((3,), 1 / 3))


def _engine(seed=0, **kw):
    cfg = EngineConfig(model="tiny-moe", max_model_len=256, max_num_seqs=8,
                       kv_cache_blocks=128, eos_token_id=0, seed=seed, **kw)
    return LLMEngine(cfg, device="cpu")


def test_tiny_moe_engine_deterministic():
    prompts = [[1, 2, 3, 4, 5], [7, 8, 9]]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    eng = _engine()
    assert all(isinstance(l.mlp, MoEMLP) for l in eng.model.layers)
    out1 = eng.generate(prompts, sp)
    assert out1 == eng.generate(prompts, sp)
    assert all(len(o) == 8 for o in out1)
    assert out1 == _engine().generate(prompts, sp)
    assert out1 != _engine(seed=1).generate(prompts, sp)


def test_checkpoint_round_trip_hf_mixtral_names(tmp_path):
    """A tiny-moe checkpoint written under HF Mixtral names loads bit-equal
    into every parameter."""
    from safetensors.torch import save_file
    from helix_amd.engine.weights import load_llama_weights
    cfg = PRESETS["tiny-moe"]
    src = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(3)
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
        sd[pre + "block_sparse_moe.gate.weight"] = layer.mlp.router_w
        for e in range(cfg.num_experts):
            ex = pre + f"block_sparse_moe.experts.{e}."
            sd[ex + "w1.weight"] = layer.mlp.w13[e, :I]
            sd[ex + "w3.weight"] = layer.mlp.w13[e, I:]
            sd[ex + "w2.weight"] = layer.mlp.w2[e]
    save_file({n: t.detach().clone().contiguous() for n, t in sd.items()},
              str(tmp_path / "model.safetensors"))
    dst = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(4)
    assert load_llama_weights(dst, str(tmp_path)) == len(sd)
    want = dict(src.named_parameters())
    got = dict(dst.named_parameters())
    assert set(got) == set(want)
    for name in want:
        assert torch.equal(got[name], want[name]), name


def test_estimate_covers_tiny_moe_weights():
    from helix_amd.runner.service import DEFAULT_SPECS, estimate_model_bytes
    m = LlamaForCausalLM(PRESETS["tiny-moe"]).to(torch.bfloat16)
    assert estimate_model_bytes(DEFAULT_SPECS["tiny-moe"]) >= m.memory_bytes()
    # the expert term is counted: eight experts outweigh tiny's one MLP
    assert estimate_model_bytes(DEFAULT_SPECS["tiny-moe"]) > \
        estimate_model_bytes(DEFAULT_SPECS["tiny"])
    assert DEFAULT_SPECS["mixtral-8x7b"].preset == "mixtral-8x7b"
    # ~46.7 G parameters in bf16
    est = estimate_model_bytes(DEFAULT_SPECS["mixtral-8x7b"])
    assert 93e9 < est < 288e9


@pytest.mark.parametrize("kw, tp, what", [
    (dict(quantization="q4_0"), 1, "quantization"),
    (dict(quantization="fp8"), 1, "quantization"),
    (dict(max_loras=2), 1, "max_loras"),
    (dict(), 2, "tp_size"),
])
def test_engine_refuses_unsupported_moe_options(kw, tp, what):
    cfg = EngineConfig(model="tiny-moe", max_model_len=256, max_num_seqs=8,
                       kv_cache_blocks=128, **kw)
    with pytest.raises(ValueError, match=what):
        LLMEngine(cfg, device="cpu", tp_size=tp)


def test_catalogue_aliases_resolve():
    from helix_amd.server.models_catalog import (ModelCatalog,
                                                 resolve_model_name)
    from helix_amd.server.router import InferenceRouter, NoRunnerError
    from helix_amd.store import Store
    cat = ModelCatalog(Store(":memory:"))
    want = cat.get("mixtral-8x7b")
    assert want["kind"] == "chat" and want["runtime"] == "helix_amd"
    assert set(want) == set(cat.get("llama3-8b"))
    for alias in ("helix-mixtral", "mixtral:instruct",
                  "mistralai/Mixtral-8x7B-Instruct-v0.1"):
        assert resolve_model_name(alias) == "mixtral-8x7b"
        assert cat.get(alias) == want
    assert resolve_model_name("llama3-8b") == "llama3-8b"
    with pytest.raises(NoRunnerError, match="mixtral-8x7b"):
        InferenceRouter().pick_runner("helix-mixtral")


def test_dense_presets_unchanged():
    for name, cfg in PRESETS.items():
        if name in ("mixtral-8x7b", "tiny-moe"):
            assert cfg.num_experts == 8 and cfg.experts_per_token == 2
        else:
            assert cfg.num_experts == 0, name
    names = [n for n, _ in LlamaForCausalLM(PRESETS["tiny"])
             .named_parameters()]
    assert "layers.0.mlp.gate_up_proj.weight" in names
    assert "layers.1.mlp.down_proj.weight" in names
    assert not any("router" in n or "w13" in n for n in names)
    assert len(names) == 3 + 6 * PRESETS["tiny"].num_layers
    moe = [n for n, _ in LlamaForCausalLM(PRESETS["tiny-moe"])
           .named_parameters()]
    assert {"layers.0.mlp.router_w", "layers.0.mlp.w13",
            "layers.0.mlp.w2"} <= set(moe)
    mix = PRESETS["mixtral-8x7b"]
    assert (mix.vocab_size, mix.hidden_size, mix.intermediate_size,
            mix.num_layers, mix.num_heads, mix.num_kv_heads, mix.head_dim,
            mix.rope_base, mix.max_position, mix.sliding_window) == \
        (32000, 4096, 14336, 32, 32, 8, 128, 1e6, 32768, 0)
