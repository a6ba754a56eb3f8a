"""K-quant mixture-of-experts serving on CPU: the test oracle itself
(tolerance, mutants), the torch definition of the ops, MoEMLP's K-quant
state, GGUF expert tensors (export, resident load), the tiny-qwen3-moe
engine, and the qwen3-30b-a3b preset, spec, aliases and admission estimate."""
import functools
import subprocess
import sys
from collections import defaultdict

import pytest
import torch

import helix_amd.ops as ops
import moe_kq_oracle as mq
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import (LlamaForCausalLM, MoEMLP, PRESETS,
                                    QWEN3_MOE_PRESETS, get_preset)
from helix_amd.models.quant import (attach_wq_scratch, has_wq,
                                    quantize_model_experts_kq)

FMTS = ("q4_k", "q6_k")
NAMES = {"q4_k": ("qs", "hdr"), "q6_k": ("ql", "qh", "sc", "d")}


@functools.lru_cache(maxsize=None)
def _result(case):
    """(emulation error, {mutant: error}) of one case, each the worst row."""
    b = mq.build(case)
    err = float(mq.wq_error(mq.emulate(case, b), b.want).max())
    muts = {n: float(mq.wq_error(o, b.want).max())
            for n, o in mq.mutant_outputs(case, b).items()}
    return err, muts


def test_tolerance():
    """TOL_MOE_KQ = 4 x the worst emulation error over all cases (within
    rounding of the constant), and every mutant misses it on every case it
    applies to. Prints the mutant / tol table."""
    res = [_result(c) for c in mq.CASES]
    worst, wcase = max(zip((r[0] for r in res), mq.CASES), key=lambda p: p[0])
    table = defaultdict(list)
    for c, r in zip(mq.CASES, res):
        for n, v in r[1].items():
            table[n].append((v, c))
    print(f"worst emulation error {worst:.5f} ({wcase.id}), "
          f"TOL_MOE_KQ {mq.TOL_MOE_KQ}")
    print(f"{'mutant':28s} {'cases':>5s} {'min err':>9s} {'x tol':>7s}  at")
    for n in mq.MUTANTS:
        v, c = min(table[n], key=lambda p: p[0])
        print(f"{n:28s} {len(table[n]):5d} {v:9.4f} "
              f"{v / mq.TOL_MOE_KQ:7.1f}  {c.id}")
    assert set(table) == set(mq.MUTANTS)
    assert 4 * worst <= mq.TOL_MOE_KQ * 1.02, worst
    assert mq.TOL_MOE_KQ <= 4 * worst * 1.10, worst
    for n in mq.MUTANTS:
        v, c = min(table[n], key=lambda p: p[0])
        assert v > mq.TOL_MOE_KQ, (n, c.id, v)


@pytest.mark.parametrize("pair", mq.FMT_PAIRS, ids="+".join)
def test_mutant_fails_the_assertion(pair):
    """The mutants fail assert_wq_close itself, the assertion the GPU tests
    use, not only a number next to it."""
    case = mq.Case(*pair, 8, 2, 256, 256, 65, "skewed")
    b = mq.build(case)
    mq.assert_wq_close(mq.emulate(case, b), b.want, mq.TOL_MOE_KQ)
    outs = mq.mutant_outputs(case, b)
    assert len(outs) == 5 + 2 * len(set(pair))
    for name, o in outs.items():
        with pytest.raises(AssertionError, match="error"):
            mq.assert_wq_close(o, b.want, mq.TOL_MOE_KQ, name)


def test_cases_cover_the_kernels():
    """Every wave count the K split can return is taken by some shape, in
    the GEMM it belongs to, with uneven shares among the waves."""
    assert len(mq.CASES) == 3 * len(mq.SHAPES) * len(mq.TS) * len(mq.FAMILIES)
    assert {c.T for c in mq.CASES} == {1, 16, 17, 65, 130}
    assert {mq.waves(I, H, True) for (_, _, H, I) in mq.SHAPES} == {4, 8}
    assert {mq.waves(H, I, False) for (_, _, H, I) in mq.SHAPES} == {4, 8, 16}
    assert {c.H // 256 for c in mq.CASES} == {1, 3, 9}
    assert {c.I // 256 for c in mq.CASES} == {1, 3, 9, 17}
    # the cap: no shape, however deep, takes more
    assert mq.waves(16, 256 * 1024, True) == 8
    assert mq.waves(16, 256 * 1024, False) == 16
    assert mq.waves(65536, 256 * 1024, False) == 4


@pytest.mark.parametrize("fmt", FMTS)
def test_oracle_dequantiser_is_the_reference(fmt):
    """The oracle's own exact decode, rounded once to fp32, is
    ops.dequantize_kq bit for bit, and the stack layout is the [E*rows, K]
    weight's."""
    E, k, H, I = mq.SHAPES[1]
    for which in ("w13", "w2"):
        st = mq.stack_planes(fmt, which, E, H, I)
        flat = tuple(p.reshape(-1, *p.shape[2:]) for p in st)
        want = ops.dequantize_kq(flat, fmt)
        got = mq.dequant_stack(st, fmt).float()
        assert torch.equal(got.view(want.shape), want)
        assert torch.equal(ops.dequantize_experts_kq(st, fmt, torch.float32),
                           want.view(got.shape))
        assert torch.equal(mq.dense_stack(fmt, which, E, H, I),
                           ops.dequantize_experts_kq(st, fmt))


CPU_CASES = [c for c in mq.CASES if c.T in (1, 17, 130)
             and (c.E, c.k, c.H, c.I) in mq.SHAPES[:4]]


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_ops_cpu_definition(case):
    """ops.moe_experts_kq on the CPU is ref.moe_experts on the dequantised
    weights, bit for bit, and is within tolerance of the fp64 oracle."""
    b = mq.build(case)
    ids, w = ops.moe_route(b.logits, case.k)
    out = ops.moe_experts_kq(b.x, b.w13, b.w2, case.fmt, ids, w)
    assert out.dtype == torch.bfloat16
    w13 = ops.dequantize_experts_kq(b.w13, case.f13)
    w2 = ops.dequantize_experts_kq(b.w2, case.f2)
    want = ops.reference.moe_experts(b.x, w13, w2, ids, w)
    assert torch.equal(out, want)
    mq.assert_wq_close(out, b.want, mq.TOL_MOE_KQ, case.id)
    out2 = ops.moe_forward_kq(b.x, b.logits, list(b.w13), list(b.w2),
                              case.fmt, case.k)
    assert torch.equal(out, out2)
    if case.f13 == case.f2:
        out3 = ops.moe_forward_kq(b.x, b.logits, b.w13, b.w2, case.f13,
                                  case.k)
        assert torch.equal(out, out3)


def test_ops_bad_formats():
    c = mq.Case("q4_k", "q6_k", 8, 2, 256, 256, 17, "uniform")
    b = mq.build(c)
    ids, w = ops.moe_route(b.logits, 2)
    for fmt in ("q4_0", "q5_k", ("q4_k", "q8_0"), ("q4_k",)):
        with pytest.raises(ValueError):
            ops.moe_experts_kq(b.x, b.w13, b.w2, fmt, ids, w)
    # plane counts: a q6_k stack named q4_k and the reverse
    with pytest.raises(ValueError):
        ops.moe_experts_kq(b.x, b.w13, b.w2, "q4_k", ids, w)
    with pytest.raises(ValueError):
        ops.moe_experts_kq(b.x, b.w13, b.w2, "q6_k", ids, w)
    # the Q4_0/Q8_0 functions do not take the K formats
    with pytest.raises(ValueError):
        ops.moe_experts_wq(b.x, b.w13, b.w13, "q4_k", ids, w)
    assert ops.MOE_KQ_FUSED_MAX_T >= 1


# -- model ----------------------------------------------------------------

CFG = get_preset("tiny-qwen3-moe")


def _tiny(seed=3):
    return LlamaForCausalLM(CFG).to(torch.bfloat16).init_random(seed)


def _planes_of(w, fmt):
    E, rows, K = w.shape
    return tuple(p.view(E, rows, *p.shape[1:])
                 for p in ops.quantize_kq(w.data.view(E * rows, K), fmt))


@pytest.mark.parametrize("pair", mq.FMT_PAIRS, ids="+".join)
def test_quantize_model_experts_kq(pair):
    """The planes are quantize_kq of the bf16 experts, registered as
    persistent buffers; the Parameters are gone; Q6_K's `d` stays fp16 under
    model.to(bfloat16); the state_dict round-trips; the model computes what
    the dequantised model computes."""
    f13, f2 = pair
    src, m = _tiny(), _tiny()
    E, H, I = CFG.num_experts, CFG.hidden_size, CFG.intermediate_size
    assert not has_wq(m)
    assert quantize_model_experts_kq(m, pair) == CFG.num_layers
    assert quantize_model_experts_kq(m, pair) == 0          # served as it is
    assert has_wq(m)
    m = m.to(torch.bfloat16)
    names = {n for n, _ in m.named_parameters()}
    assert not any(n.endswith(("mlp.w13", "mlp.w2")) for n in names)
    assert "layers.0.mlp.router_w" in names
    sd = m.state_dict()
    for ls, lm in zip(src.layers, m.layers):
        assert isinstance(lm.mlp, MoEMLP)
        assert lm.mlp.expert_fmt == pair
        assert lm.mlp.router_w.dtype == torch.bfloat16
        for name, w, f in (("w13", ls.mlp.w13, f13), ("w2", ls.mlp.w2, f2)):
            got = lm.mlp.expert_planes(name)
            bufs = dict(lm.mlp.named_buffers())
            assert {n for n in bufs if n.startswith(name + "_")} == \
                {f"{name}_{p}" for p in NAMES[f]}
            for pn, g, want in zip(NAMES[f], got, _planes_of(w, f)):
                assert g is bufs[f"{name}_{pn}"]
                assert g.dtype == want.dtype and torch.equal(g, want), pn
                assert g.shape[:2] == (E, w.shape[1])
            if f == "q6_k":
                assert got[3].dtype == torch.float16
                assert got[2].dtype == torch.int8
    assert f"layers.0.mlp.w13_{NAMES[f13][0]}" in sd
    assert f"layers.1.mlp.w2_{NAMES[f2][-1]}" in sd
    attach_wq_scratch(m)                                    # CPU: a no-op
    assert m.layers[0].mlp.scratch is None
    # state_dict round trip into a model of the same state, other weights
    other = _tiny(4)
    quantize_model_experts_kq(other, pair)
    assert not torch.equal(other.layers[0].mlp.expert_planes("w13")[0],
                           m.layers[0].mlp.expert_planes("w13")[0])
    other.load_state_dict(sd, strict=True)
    so = other.state_dict()
    assert set(so) == set(sd)
    assert all(so[k].dtype == sd[k].dtype and torch.equal(so[k], sd[k])
               for k in sd)
    # forward: the dequantised twin
    twin = _tiny()
    for lt, lm in zip(twin.layers, m.layers):
        lt.mlp.w13.data = ops.dequantize_experts_kq(
            lm.mlp.expert_planes("w13"), f13)
        lt.mlp.w2.data = ops.dequantize_experts_kq(
            lm.mlp.expert_planes("w2"), f2)
    x = torch.randn(5, H, generator=torch.Generator().manual_seed(1)) \
        .to(torch.bfloat16)
    assert torch.equal(m.layers[0].mlp(x), twin.layers[0].mlp(x))
    assert float(m.layers[0].mlp(x).detach().float().abs().max()) > 0


def test_set_kquant_experts_checks_shapes():
    m = _tiny().layers[0].mlp
    p13, p2 = _planes_of(m.w13, "q4_k"), _planes_of(m.w2, "q6_k")
    flat = tuple(p.reshape(-1, *p.shape[2:]) for p in p13)
    with pytest.raises(ValueError):
        m.set_kquant_experts(flat, p2, ("q4_k", "q6_k"))          # 2-D
    with pytest.raises(ValueError):
        m.set_kquant_experts(p13, p2, "q4_k")                      # w2 is q6_k
    with pytest.raises(ValueError):
        m.set_kquant_experts(p13, p2[:3] + (p2[3].float(),),
                             ("q4_k", "q6_k"))
    with pytest.raises(ValueError):
        m.set_kquant_experts(p13, p2, ("q4_k", "q8_0"))
    with pytest.raises(ValueError):
        m.set_kquant_experts(tuple(p[:-1] for p in p13), p2,
                             ("q4_k", "q6_k"))                     # E - 1
    assert m.expert_fmt is None and "w13" in dict(m.named_parameters())
    # sizes that cannot hold a super-block
    small = LlamaForCausalLM(PRESETS["tiny-moe"]).layers[0].mlp
    small.hidden_size = 128
    with pytest.raises(ValueError, match="256"):
        small.set_kquant_experts(p13, p2, ("q4_k", "q6_k"))
    m.set_kquant_experts(p13, p2, ("q4_k", "q6_k"))
    assert m.expert_fmt == ("q4_k", "q6_k")
    assert "w13" not in dict(m.named_parameters())


# -- engine, preset, spec, estimate ---------------------------------------

def _cfg(**kw):
    return EngineConfig(model="tiny-qwen3-moe", max_model_len=256,
                        max_num_seqs=8, kv_cache_blocks=128, eos_token_id=0,
                        seed=5, **kw)


@pytest.mark.parametrize("pair", [("q4_k", "q6_k"), ("q6_k", "q6_k")],
                         ids="+".join)
def test_engine_kquant_experts_match_dequantised(pair):
    """A model handed to the engine with K-quant experts is served as it
    is, and decodes the greedy tokens of the bf16 engine that carries the
    dequantised experts."""
    prompts = [[1, 2, 3, 4, 5], [7, 8, 9]]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    model = _tiny(5)
    quantize_model_experts_kq(model, pair)
    eng = LLMEngine(_cfg(), device="cpu", model=model)
    assert all(l.mlp.expert_fmt == pair for l in eng.model.layers)
    assert eng.model.layers[0].attn.q_norm_w is not None
    out = eng.generate(prompts, sp)
    dense = LLMEngine(_cfg(), device="cpu", model=_tiny(5))
    for ld, lq in zip(dense.model.layers, eng.model.layers):
        ld.mlp.w13.data = ops.dequantize_experts_kq(
            lq.mlp.expert_planes("w13"), pair[0])
        ld.mlp.w2.data = ops.dequantize_experts_kq(
            lq.mlp.expert_planes("w2"), pair[1])
    assert out == dense.generate(prompts, sp)
    assert all(len(o) == 8 for o in out)
    # the engine option still takes the Q4_0/Q8_0 names alone
    with pytest.raises(ValueError, match="expert_quantization"):
        LLMEngine(_cfg(expert_quantization="q4_k"), device="cpu")


def test_presets_specs_and_aliases():
    from helix_amd.runner.service import DEFAULT_SPECS, estimate_model_bytes
    from helix_amd.server.models_catalog import (ModelCatalog,
                                                 resolve_model_name)
    from helix_amd.store import Store
    # their own table: PRESETS keeps its entries, get_preset finds both
    assert set(QWEN3_MOE_PRESETS) == {"qwen3-30b-a3b", "tiny-qwen3-moe"}
    assert not set(QWEN3_MOE_PRESETS) & set(PRESETS)
    assert get_preset("tiny-moe") is PRESETS["tiny-moe"]
    assert all(c.name == n for n, c in QWEN3_MOE_PRESETS.items())
    with pytest.raises(KeyError):
        get_preset("qwen3-30b")
    c = get_preset("qwen3-30b-a3b")
    assert (c.vocab_size, c.hidden_size, c.intermediate_size, c.num_layers,
            c.num_heads, c.num_kv_heads, c.head_dim, c.rms_norm_eps,
            c.rope_base, c.max_position, c.qk_norm, c.num_experts,
            c.experts_per_token, c.attention_bias, c.sliding_window) == \
        (151936, 2048, 768, 48, 32, 4, 128, 1e-6, 1e6, 40960, True, 128, 8,
         False, 0)
    t = get_preset("tiny-qwen3-moe")
    assert (t.hidden_size, t.intermediate_size, t.num_layers, t.num_heads,
            t.num_kv_heads, t.head_dim, t.num_experts, t.experts_per_token,
            t.qk_norm) == (256, 256, 2, 4, 2, 128, 16, 4, True)
    assert t.hidden_size % 256 == 0 and t.intermediate_size % 256 == 0
    cat = ModelCatalog(Store(":memory:"))
    for alias in ("qwen3:30b", "Qwen/Qwen3-30B-A3B"):
        assert resolve_model_name(alias) == "qwen3-30b-a3b"
        info = cat.get(alias)
        assert info == cat.get("qwen3-30b-a3b")
        assert info["family"] == "qwen" and info["kind"] == "chat"
        assert info["runtime"] == "helix_amd"
        assert info["context_length"] == 40960
        assert set(info) == set(cat.get("llama3-8b"))
    spec = DEFAULT_SPECS["qwen3-30b-a3b"]
    assert spec.preset == "qwen3-30b-a3b" and spec.kind == "llm"
    assert spec.max_model_len == 40960
    assert spec.quantization is None and spec.expert_quantization is None
    tiny = DEFAULT_SPECS["tiny-qwen3-moe"]
    assert tiny.preset == "tiny-qwen3-moe" and tiny.max_model_len == 256
    m = LlamaForCausalLM(t).to(torch.bfloat16)
    assert estimate_model_bytes(tiny) >= m.memory_bytes()


def test_estimate_is_the_arithmetic_of_the_shapes():
    from helix_amd.runner.service import DEFAULT_SPECS, estimate_model_bytes
    spec = DEFAULT_SPECS["qwen3-30b-a3b"]
    V, H, I, L, E = 151936, 2048, 768, 48, 128
    q, kv = 32 * 128, 4 * 128
    experts = L * E * 3 * H * I
    assert experts == 28_991_029_248                        # 29.0 G weights
    rest = 2 * V * H + L * (H * (q + 2 * kv) + q * H + E * H)
    kv_bytes = 2 * L * 4 * 16 * 128 * 2 * spec.kv_cache_blocks
    assert estimate_model_bytes(spec) == \
        2 * (experts + rest) + kv_bytes + (1 << 30)
    assert 57.9e9 < 2 * experts < 58.0e9                    # 58 GB in bf16
    assert 16.3e9 < experts // 256 * 144 < 16.4e9           # as Q4_K


# -- GGUF -------------------------------------------------------------------

def _src():
    """What `helix export-gguf --preset tiny-qwen3-moe --seed 9` exports."""
    return LlamaForCausalLM(CFG).init_random(9)


def _export_cli(path, *args, preset="tiny-qwen3-moe"):
    subprocess.run(
        [sys.executable, "-m", "helix_amd.cli", "export-gguf", "--preset",
         preset, "--seed", "9", "-o", path, *args], check=True)


def _file_planes(g, name, fmt):
    """unpack_ggml_kq of a merged expert tensor's raw bytes, as a stack."""
    E, rows, K = g.tensors[name].shape
    planes = ops.unpack_ggml_kq(g.read_raw(name), (E * rows, K), fmt)
    return tuple(p.view(E, rows, *p.shape[1:]) for p in planes)


def _assert_resident(dst, g, fmts):
    """Every layer's planes are byte-equal to the file's tensors unpacked."""
    for i, (layer, (f13, f2)) in enumerate(zip(dst.layers, fmts)):
        m = layer.mlp
        assert m.expert_fmt == (f13, f2)
        assert not hasattr(m, "w13") and not hasattr(m, "w2")
        gate = _file_planes(g, f"blk.{i}.ffn_gate_exps.weight", f13)
        up = _file_planes(g, f"blk.{i}.ffn_up_exps.weight", f13)
        down = _file_planes(g, f"blk.{i}.ffn_down_exps.weight", f2)
        for got, a, b in zip(m.expert_planes("w13"), gate, up):
            want = torch.cat([a, b], dim=1)
            assert got.dtype == want.dtype and torch.equal(got, want)
        for got, want in zip(m.expert_planes("w2"), down):
            assert got.dtype == want.dtype and torch.equal(got, want)


Q4_K_M = [("q4_k", "q4_k"), ("q4_k", "q6_k")]


def test_gguf_q4_k_m_experts_resident_and_dense(tmp_path):
    """`export-gguf --preset tiny-qwen3-moe --expert-quant q4_k_m` (through
    the CLI): Q4_K gate/up, Q4_K down in layer 0 and Q6_K down in layer 1,
    everything else as without the flag; loaded resident every plane is the
    file's bytes, loaded dense every expert weight is their dequantisation."""
    from helix_amd.engine.gguf import (GGUFFile, load_gguf_weights,
                                       q4_k_m_uses_q6_k)
    assert [q4_k_m_uses_q6_k(i, 2) for i in range(2)] == [False, True]
    path = str(tmp_path / "m.gguf")
    _export_cli(path, "--expert-quant", "q4_k_m")
    E, H, I = CFG.num_experts, CFG.hidden_size, CFG.intermediate_size
    g = GGUFFile(path)
    assert g.arch() == "qwen3moe"
    assert g.metadata["qwen3moe.expert_count"] == E
    t = g.tensors
    assert t["blk.0.ffn_gate_exps.weight"].shape == (E, I, H)
    assert t["blk.1.ffn_down_exps.weight"].shape == (E, H, I)
    want = {"gate": ("Q4_K", "Q4_K"), "up": ("Q4_K", "Q4_K"),
            "down": ("Q4_K", "Q6_K")}
    for part, types in want.items():
        for i, ty in enumerate(types):
            assert t[f"blk.{i}.ffn_{part}_exps.weight"].type_name == ty
    assert t["blk.0.attn_q.weight"].type_name == "F32"
    assert t["blk.0.ffn_gate_inp.weight"].type_name == "BF16"
    src = _src()
    dst = LlamaForCausalLM(CFG).init_random(1)
    assert load_gguf_weights(dst, path, keep_quantized=True) == len(t)
    _assert_resident(dst, g, Q4_K_M)
    assert has_wq(dst)
    for ls, ld in zip(src.layers, dst.layers):
        assert torch.equal(ld.mlp.router_w, ls.mlp.router_w)
        assert torch.equal(ld.attn.q_norm_w, ls.attn.q_norm_w)
    # the file's blocks are quantize_kq of the source weights
    got = dst.layers[1].mlp.expert_planes("w2")
    for a, b in zip(got, _planes_of(src.layers[1].mlp.w2, "q6_k")):
        assert torch.equal(a, b)
    dst = dst.to(torch.bfloat16)
    assert dst.layers[1].mlp.w2_d.dtype == torch.float16
    dense = LlamaForCausalLM(CFG).init_random(2)
    assert load_gguf_weights(dense, path) == len(t)
    for ld, lr, (f13, f2) in zip(dense.layers, dst.layers, Q4_K_M):
        assert ld.mlp.expert_fmt is None
        assert torch.equal(ld.mlp.w13.data, ops.dequantize_experts_kq(
            lr.mlp.expert_planes("w13"), f13))
        assert torch.equal(ld.mlp.w2.data, ops.dequantize_experts_kq(
            lr.mlp.expert_planes("w2"), f2))
    # keep_quantized=False is unchanged: the experts are bf16 Parameters
    assert "layers.0.mlp.w13" in dict(dense.named_parameters())


@pytest.mark.parametrize("eq", FMTS)
def test_gguf_uniform_expert_quant_with_quant(tmp_path, eq):
    """--expert-quant next to --quant q4_k_m: the experts take the expert
    format in every layer, the projections keep llama.cpp's mix, and both
    stay resident."""
    from helix_amd.engine.gguf import GGUFFile, load_gguf_weights
    from helix_amd.models.quant import KQLinear
    path = str(tmp_path / "m.gguf")
    _export_cli(path, "--quant", "q4_k_m", "--expert-quant", eq)
    g = GGUFFile(path)
    for i in range(CFG.num_layers):
        for part in ("gate", "up", "down"):
            assert g.tensors[f"blk.{i}.ffn_{part}_exps.weight"].type_name \
                == eq.upper()
    assert g.tensors["blk.1.attn_v.weight"].type_name == "Q6_K"
    dst = LlamaForCausalLM(CFG).init_random(1)
    load_gguf_weights(dst, path, keep_quantized=True)
    _assert_resident(dst, g, [(eq, eq)] * 2)
    assert isinstance(dst.layers[0].attn.qkv_proj, KQLinear)


def test_gguf_expert_quant_guards_and_default(tmp_path):
    """expert_quant=None writes today's file byte for byte; --quant q4_k
    keeps leaving the experts bf16; the refusals."""
    from helix_amd.engine.gguf import GGUFFile, export_model_gguf
    src = LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(9)
    a, b = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    for quant in ("", "q4_0", "q4_k_m"):
        export_model_gguf(src, a, quant=quant)
        export_model_gguf(src, b, quant=quant, expert_quant=None)
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), quant
    assert GGUFFile(a).tensors["blk.0.ffn_up_exps.weight"].type_name == "BF16"
    with pytest.raises(ValueError, match="expert_quant"):
        export_model_gguf(src, a, expert_quant="q4_0")
    with pytest.raises(ValueError, match="expert_quant"):
        export_model_gguf(src, a, quant="q8_0", expert_quant="q4_k")
    with pytest.raises(ValueError, match="no experts"):
        export_model_gguf(LlamaForCausalLM(PRESETS["tiny"]).init_random(1),
                          a, expert_quant="q4_k")
    # tiny-moe's sizes are multiples of 256 too: its experts can be written
    export_model_gguf(src, a, expert_quant="q6_k")
    assert GGUFFile(a).tensors["blk.0.ffn_up_exps.weight"].type_name == "Q6_K"
    assert GGUFFile(a).arch() == "llama"


def _rewrite(path, out, rename=None, requant=None):
    """Copy a GGUF file tensor by tensor, with tensors renamed / split
    (rename(name, GGMLQuantized-or-tensor) -> {name: value}) or
    re-quantised from their dequantisation."""
    from helix_amd.engine.gguf import (GGMLQuantized, GGUFFile, quantize_ggml,
                                       write_gguf)
    g = GGUFFile(path)
    tensors = {}
    for name, info in g.tensors.items():
        if info.type_name in ("F32", "BF16", "F16"):
            v = g.load_tensor(name)
        else:
            v = GGMLQuantized(g.read_raw(name), info.shape, info.type_name)
        if requant and name in requant:
            w = g.load_tensor(name)
            q = quantize_ggml(w.reshape(-1, w.shape[-1]).float(),
                              requant[name])
            v = GGMLQuantized(q.raw, info.shape, q.type_name)
        tensors.update(rename(name, v) if rename else {name: v})
    md = {k: v for k, v in g.metadata.items() if k != "general.alignment"}
    write_gguf(out, md, tensors)


def test_gguf_legacy_per_expert_names(tmp_path):
    """blk.i.ffn_gate.{e}.weight etc. with K-quant blocks load to the same
    resident model as the merged tensors."""
    from helix_amd.engine.gguf import (GGMLQuantized, GGUFFile,
                                       export_model_gguf, load_gguf_weights)
    src = _src()
    merged, legacy = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    export_model_gguf(src, merged, expert_quant="q4_k_m")
    E = CFG.num_experts

    def split(name, v):
        parts = name.split(".")
        if len(parts) < 4 or not parts[2].endswith("_exps"):
            return {name: v}
        stem = parts[2][:-len("_exps")]
        per = len(v.raw) // E
        return {f"blk.{parts[1]}.{stem}.{e}.weight": GGMLQuantized(
            v.raw[e * per:(e + 1) * per], v.shape[1:], v.type_name)
            for e in range(E)}

    _rewrite(merged, legacy, rename=split)
    assert "blk.0.ffn_down.3.weight" in GGUFFile(legacy).tensors
    a = LlamaForCausalLM(CFG).init_random(1)
    b = LlamaForCausalLM(CFG).init_random(2)
    load_gguf_weights(a, merged, keep_quantized=True)
    load_gguf_weights(b, legacy, keep_quantized=True)
    _assert_resident(b, GGUFFile(merged), Q4_K_M)
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_gguf_mixed_families_load_dense(tmp_path):
    """A layer with a Q4_0 gate/up and a Q6_K down, or with Q4_K gate and
    Q6_K up, loads dense; the file's other layer stays resident."""
    from helix_amd.engine.gguf import export_model_gguf, load_gguf_weights
    src = _src()
    base = str(tmp_path / "bf16.gguf")
    export_model_gguf(src, base)
    for n, requant in enumerate((
            {"blk.0.ffn_gate_exps.weight": "Q4_0",
             "blk.0.ffn_up_exps.weight": "Q4_0",
             "blk.0.ffn_down_exps.weight": "Q6_K"},
            {"blk.0.ffn_gate_exps.weight": "Q4_K",
             "blk.0.ffn_up_exps.weight": "Q6_K",
             "blk.0.ffn_down_exps.weight": "Q6_K"})):
        requant.update({"blk.1.ffn_gate_exps.weight": "Q6_K",
                        "blk.1.ffn_up_exps.weight": "Q6_K",
                        "blk.1.ffn_down_exps.weight": "Q4_K"})
        mixed = str(tmp_path / f"mixed{n}.gguf")
        _rewrite(base, mixed, requant=requant)
        dst = LlamaForCausalLM(CFG).init_random(1)
        load_gguf_weights(dst, mixed, keep_quantized=True)
        m0, m1 = dst.layers[0].mlp, dst.layers[1].mlp
        assert m0.expert_fmt is None
        assert "w13" in dict(m0.named_parameters())
        assert m1.expert_fmt == ("q6_k", "q4_k")
        for got, want in zip(m1.expert_planes("w2"),
                             _planes_of(src.layers[1].mlp.w2, "q4_k")):
            assert torch.equal(got, want)
        x = torch.randn(3, CFG.hidden_size).to(torch.bfloat16)
        dst = dst.to(torch.bfloat16)
        assert torch.isfinite(dst.layers[0].mlp(x).float()).all()
        assert torch.isfinite(dst.layers[1].mlp(x).float()).all()
