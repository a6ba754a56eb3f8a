"""Quantised mixture-of-experts serving on CPU: the test oracle itself
(tolerance, mutants), the torch definition of the ops, the quantised MoEMLP
state, GGUF expert tensors, the engine option and the admission estimate."""
import functools
from collections import defaultdict

import pytest
import torch

import helix_amd.ops as ops
import moe_wq_oracle as mq
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import LlamaForCausalLM, MoEMLP, PRESETS
from helix_amd.models.quant import (attach_wq_scratch, has_wq,
                                    quantize_model_experts)


@functools.lru_cache(maxsize=None)
def _result(case):
    """(emulation error, {mutant: error}) of one case, each the worst row."""
    b = mq.build(case)
    err = float(mq.wq_error(mq.emulate(case, b), b.want).max())
    muts = {n: float(mq.wq_error(o, b.want).max())
            for n, o in mq.mutant_outputs(case, b).items()}
    return err, muts


def test_tolerance():
    """TOL_MOE_WQ = 4 x the worst emulation error over all cases (within
    rounding of the constant), and every mutant misses it on every case it
    applies to. Prints the mutant / tol table."""
    res = [_result(c) for c in mq.CASES]
    worst, wcase = max(zip((r[0] for r in res), mq.CASES), key=lambda p: p[0])
    table = defaultdict(list)
    for c, r in zip(mq.CASES, res):
        for n, v in r[1].items():
            table[n].append((v, c))
    print(f"worst emulation error {worst:.5f} ({wcase.id}), "
          f"TOL_MOE_WQ {mq.TOL_MOE_WQ}")
    print(f"{'mutant':24s} {'cases':>5s} {'min err':>9s} {'x tol':>7s}  at")
    for n in mq.MUTANTS:
        v, c = min(table[n], key=lambda p: p[0])
        print(f"{n:24s} {len(table[n]):5d} {v:9.4f} "
              f"{v / mq.TOL_MOE_WQ:7.1f}  {c.id}")
    assert set(table) == set(mq.MUTANTS)
    assert 4 * worst <= mq.TOL_MOE_WQ * 1.02, worst
    assert mq.TOL_MOE_WQ <= 4 * worst * 1.10, worst
    for n in mq.MUTANTS:
        v, c = min(table[n], key=lambda p: p[0])
        assert v > mq.TOL_MOE_WQ, (n, c.id, v)


@pytest.mark.parametrize("fmt", mq.FMTS)
def test_mutant_fails_the_assertion(fmt):
    """The mutants fail assert_wq_close itself, the assertion the GPU tests
    use, not only a number next to it."""
    case = mq.Case(fmt, 8, 2, 256, 256, 65, "skewed")
    b = mq.build(case)
    mq.assert_wq_close(mq.emulate(case, b), b.want, mq.TOL_MOE_WQ)
    outs = mq.mutant_outputs(case, b)
    assert len(outs) == (6 if fmt == "q4_0" else 5)
    for name, o in outs.items():
        with pytest.raises(AssertionError, match="error"):
            mq.assert_wq_close(o, b.want, mq.TOL_MOE_WQ, name)


def test_cases_cover_the_kernels():
    assert len(mq.CASES) == 2 * len(mq.SHAPES) * len(mq.TS) * len(mq.FAMILIES)
    assert {c.T for c in mq.CASES} == {1, 16, 17, 65, 130}
    # 129 blocks along the down GEMM's K, 65 along the gated GEMM's
    assert {c.I // 32 for c in mq.CASES} >= {129, 65}
    assert {c.H // 32 for c in mq.CASES} >= {65, 5}


CPU_CASES = [c for c in mq.CASES if c.T in (1, 17, 130)]


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_ops_cpu_definition(case):
    """ops.moe_experts_wq on the CPU is ref.moe_experts on the dequantised
    weights, bit for bit, and is within tolerance of the fp64 oracle."""
    b = mq.build(case)
    ids, w = ops.moe_route(b.logits, case.k)
    out = ops.moe_experts_wq(b.x, b.w13, b.w2, case.fmt, ids, w)
    assert out.dtype == torch.bfloat16
    w13 = ops.dequantize_wq(b.w13[0].reshape(case.E * 2 * case.I, -1),
                            b.w13[1].reshape(case.E * 2 * case.I, -1),
                            case.fmt, torch.bfloat16).view(
                                case.E, 2 * case.I, case.H)
    w2 = ops.dequantize_wq(b.w2[0].reshape(case.E * case.H, -1),
                           b.w2[1].reshape(case.E * case.H, -1),
                           case.fmt, torch.bfloat16).view(
                               case.E, case.H, case.I)
    d13, d2 = mq.dense_weights(case.fmt, case.E, case.H, case.I)
    assert torch.equal(w13, d13) and torch.equal(w2, d2)
    want = ops.reference.moe_experts(b.x, w13, w2, ids, w)
    assert torch.equal(out, want)
    mq.assert_wq_close(out, b.want, mq.TOL_MOE_WQ, case.id)
    out2 = ops.moe_forward_wq(b.x, b.logits, b.w13, b.w2,
                              (case.fmt, case.fmt), case.k)
    assert torch.equal(out, out2)


def test_ops_mixed_formats_and_bad_format():
    c4 = mq.Case("q4_0", 8, 2, 256, 256, 17, "uniform")
    c8 = mq.Case("q8_0", 8, 2, 256, 256, 17, "uniform")
    b4, b8 = mq.build(c4), mq.build(c8)
    ids, w = ops.moe_route(b4.logits, 2)
    out = ops.moe_experts_wq(b4.x, b4.w13, b8.w2, ("q4_0", "q8_0"), ids, w)
    w13, _ = mq.dense_weights("q4_0", 8, 256, 256)
    _, w2 = mq.dense_weights("q8_0", 8, 256, 256)
    assert torch.equal(out, ops.reference.moe_experts(b4.x, w13, w2, ids, w))
    with pytest.raises(ValueError):
        ops.moe_experts_wq(b4.x, b4.w13, b4.w2, "q4_k", ids, w)


# -- model ----------------------------------------------------------------

def _tiny_moe(seed=3):
    return LlamaForCausalLM(PRESETS["tiny-moe"]).to(torch.bfloat16) \
        .init_random(seed)


@pytest.mark.parametrize("fmt", mq.FMTS)
def test_quantize_model_experts(fmt):
    """The planes are quantize_wq of the bf16 experts, the Parameters are
    gone, the scales stay fp16 under model.to(bfloat16), and the model
    computes what the dequantised model computes."""
    src = _tiny_moe()
    m = _tiny_moe()
    cfg = PRESETS["tiny-moe"]
    E, H, I = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
    assert not has_wq(m)
    assert quantize_model_experts(m, fmt) == cfg.num_layers
    assert quantize_model_experts(m, fmt) == 0          # served as it is
    assert has_wq(m)
    m = m.to(torch.bfloat16)
    names = {n for n, _ in m.named_parameters()}
    assert not any(n.endswith(("mlp.w13", "mlp.w2")) for n in names)
    assert "layers.0.mlp.router_w" in names
    for ls, lm in zip(src.layers, m.layers):
        assert isinstance(lm.mlp, MoEMLP)
        assert lm.mlp.expert_fmt == (fmt, fmt)
        assert lm.mlp.router_w.dtype == torch.bfloat16
        for name, w in (("w13", ls.mlp.w13), ("w2", ls.mlp.w2)):
            qs, d = ops.quantize_wq(w.data.view(-1, w.shape[-1]), fmt)
            gq = getattr(lm.mlp, name + "_qs")
            gd = getattr(lm.mlp, name + "_d")
            assert gd.dtype == torch.float16
            assert gq.dtype == (torch.uint8 if fmt == "q4_0" else torch.int8)
            assert tuple(gd.shape) == (E, w.shape[1], w.shape[2] // 32)
            assert torch.equal(gq.view(qs.shape), qs)
            assert torch.equal(gd.view(d.shape), d)
    sd = m.state_dict()
    assert "layers.0.mlp.w13_qs" in sd and "layers.0.mlp.w2_d" in sd
    attach_wq_scratch(m)                                # CPU: a no-op
    assert m.layers[0].mlp.scratch is None
    # forward: the dequantised twin
    twin = _tiny_moe()
    for lt, lm in zip(twin.layers, m.layers):
        lt.mlp.w13.data = ops.dequantize_experts_wq(lm.mlp.w13_qs,
                                                    lm.mlp.w13_d, fmt)
        lt.mlp.w2.data = ops.dequantize_experts_wq(lm.mlp.w2_qs,
                                                   lm.mlp.w2_d, fmt)
    x = torch.randn(5, H, generator=torch.Generator().manual_seed(1)) \
        .to(torch.bfloat16)
    assert torch.equal(m.layers[0].mlp(x), twin.layers[0].mlp(x))


def test_set_quantized_experts_checks_shapes():
    m = _tiny_moe().layers[0].mlp
    E, rows, K = m.w13.shape
    qs, d = ops.quantize_wq(m.w13.data.view(-1, K), "q4_0")
    q2, d2 = ops.quantize_wq(m.w2.data.view(-1, m.w2.shape[-1]), "q4_0")
    p2 = (q2.view(E, m.w2.shape[1], -1), d2.view(E, m.w2.shape[1], -1))
    with pytest.raises(ValueError):
        m.set_quantized_experts((qs, d), p2, "q4_0")            # 2-D
    with pytest.raises(ValueError):
        m.set_quantized_experts((qs.view(E, rows, -1),
                                 d.view(E, rows, -1).float()), p2, "q4_0")
    with pytest.raises(ValueError):
        m.set_quantized_experts((qs.view(E, rows, -1), d.view(E, rows, -1)),
                                p2, "q8_0")
    assert m.expert_fmt is None and "w13" in dict(m.named_parameters())


# -- engine and estimate --------------------------------------------------

def _cfg(model="tiny-moe", **kw):
    return EngineConfig(model=model, max_model_len=256, max_num_seqs=8,
                        kv_cache_blocks=128, eos_token_id=0, seed=5, **kw)


@pytest.mark.parametrize("fmt", mq.FMTS)
def test_engine_expert_quantization_matches_dequantised(fmt):
    prompts = [[1, 2, 3, 4, 5], [7, 8, 9]]
    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    eng = LLMEngine(_cfg(expert_quantization=fmt), device="cpu")
    assert all(l.mlp.expert_fmt == (fmt, fmt) for l in eng.model.layers)
    out = eng.generate(prompts, sp)
    dense = LLMEngine(_cfg(), device="cpu")
    for ld, lq in zip(dense.model.layers, eng.model.layers):
        ld.mlp.w13.data = ops.dequantize_experts_wq(lq.mlp.w13_qs,
                                                    lq.mlp.w13_d, fmt)
        ld.mlp.w2.data = ops.dequantize_experts_wq(lq.mlp.w2_qs,
                                                   lq.mlp.w2_d, fmt)
    assert out == dense.generate(prompts, sp)
    assert all(len(o) == 8 for o in out)


def test_engine_option_guards():
    with pytest.raises(ValueError, match="expert_quantization"):
        LLMEngine(_cfg(model="tiny", expert_quantization="q4_0"),
                  device="cpu")
    with pytest.raises(ValueError, match="expert_quantization"):
        LLMEngine(_cfg(expert_quantization="q4_k"), device="cpu")
    # the other refusals stand next to the new option
    with pytest.raises(ValueError, match="quantization"):
        LLMEngine(_cfg(quantization="q4_0", expert_quantization="q4_0"),
                  device="cpu")
    with pytest.raises(ValueError, match="max_loras"):
        LLMEngine(_cfg(max_loras=2, expert_quantization="q4_0"),
                  device="cpu")
    with pytest.raises(ValueError, match="tp_size"):
        LLMEngine(_cfg(expert_quantization="q8_0"), device="cpu", tp_size=2)


def test_estimate_counts_quantised_experts():
    import dataclasses
    from helix_amd.runner.service import DEFAULT_SPECS, estimate_model_bytes
    m = _tiny_moe()
    quantize_model_experts(m, "q4_0")
    have = sum(t.numel() * t.element_size() for t in m.parameters()) + \
        sum(t.numel() * t.element_size() for t in m.buffers())
    spec = dataclasses.replace(DEFAULT_SPECS["tiny-moe"],
                               expert_quantization="q4_0")
    assert estimate_model_bytes(spec) >= have
    assert estimate_model_bytes(spec) < \
        estimate_model_bytes(DEFAULT_SPECS["tiny-moe"])
    mix = DEFAULT_SPECS["mixtral-8x7b"]
    bf16 = estimate_model_bytes(mix)
    q4 = estimate_model_bytes(
        dataclasses.replace(mix, expert_quantization="q4_0"))
    q8 = estimate_model_bytes(
        dataclasses.replace(mix, expert_quantization="q8_0"))
    assert q4 < bf16 - 60e9
    assert q4 < q8 < bf16 - 40e9
    # 45.1 G expert weights at 18 bytes per 32
    assert q4 > 25.3e9


# -- GGUF -------------------------------------------------------------------

def _src():
    """What `helix export-gguf --preset tiny-moe --seed 9` exports."""
    return LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(9)


def _expert_planes(src, fmt13, fmt2=None):
    out = []
    for layer in src.layers:
        per = []
        for w, f in ((layer.mlp.w13, fmt13), (layer.mlp.w2, fmt2 or fmt13)):
            qs, d = ops.quantize_wq(w.data.view(-1, w.shape[-1]), f)
            per.append((qs.view(w.shape[0], w.shape[1], -1),
                        d.view(w.shape[0], w.shape[1], -1)))
        out.append(per)
    return out


def _assert_resident(dst, src, fmt13, fmt2=None):
    for layer, (p13, p2) in zip(dst.layers, _expert_planes(src, fmt13, fmt2)):
        m = layer.mlp
        assert m.expert_fmt == (fmt13, fmt2 or fmt13)
        assert not hasattr(m, "w13") and not hasattr(m, "w2")
        for got, want in ((m.w13_qs, p13[0]), (m.w13_d, p13[1]),
                          (m.w2_qs, p2[0]), (m.w2_d, p2[1])):
            assert got.dtype == want.dtype and torch.equal(got, want)


@pytest.mark.parametrize("fmt", mq.FMTS)
def test_gguf_quantised_experts_resident_and_dense(tmp_path, fmt):
    """`export-gguf --preset tiny-moe --quant FMT` (through the CLI): the
    file holds the merged 3-D expert tensors and the two metadata keys;
    loaded resident every plane equals quantize_wq of the source weights,
    loaded dense every expert weight equals their dequantisation."""
    import subprocess
    import sys
    from helix_amd.engine.gguf import GGUFFile, load_gguf_weights
    path = str(tmp_path / "m.gguf")
    subprocess.run(
        [sys.executable, "-m", "helix_amd.cli", "export-gguf", "--preset",
         "tiny-moe", "--seed", "9", "--quant", fmt, "-o", path], check=True)
    cfg = PRESETS["tiny-moe"]
    E, H, I = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
    g = GGUFFile(path)
    assert g.metadata["llama.expert_count"] == E
    assert g.metadata["llama.expert_used_count"] == cfg.experts_per_token
    t = g.tensors
    assert t["blk.0.ffn_gate_exps.weight"].shape == (E, I, H)
    assert t["blk.1.ffn_up_exps.weight"].shape == (E, I, H)
    assert t["blk.1.ffn_down_exps.weight"].shape == (E, H, I)
    assert t["blk.0.ffn_gate_inp.weight"].shape == (E, H)
    assert t["blk.0.ffn_down_exps.weight"].type_name == fmt.upper()
    assert t["blk.0.attn_q.weight"].type_name == fmt.upper()
    assert t["blk.0.ffn_gate_inp.weight"].type_name == "BF16"
    assert "blk.0.ffn_gate.weight" not in t
    src = _src()
    dst = LlamaForCausalLM(cfg).init_random(1)
    n = load_gguf_weights(dst, path, keep_quantized=True)
    assert n == len(t)
    _assert_resident(dst, src, fmt)
    assert has_wq(dst)
    for ls, ld in zip(src.layers, dst.layers):
        assert torch.equal(ld.mlp.router_w, ls.mlp.router_w)
    dst = dst.to(torch.bfloat16)
    assert dst.layers[0].mlp.w2_d.dtype == torch.float16
    dense = LlamaForCausalLM(cfg).init_random(2)
    assert load_gguf_weights(dense, path) == len(t)
    for ld, (p13, p2) in zip(dense.layers, _expert_planes(src, fmt)):
        assert ld.mlp.expert_fmt is None
        assert torch.equal(ld.mlp.w13.data,
                           ops.dequantize_experts_wq(*p13, fmt))
        assert torch.equal(ld.mlp.w2.data,
                           ops.dequantize_experts_wq(*p2, fmt))


def test_gguf_export_without_quant_round_trips(tmp_path):
    """The export that used to die with a KeyError on mlp.gate_up_proj."""
    import subprocess
    import sys
    from helix_amd.engine.gguf import load_gguf_weights
    path = str(tmp_path / "m.gguf")
    subprocess.run(
        [sys.executable, "-m", "helix_amd.cli", "export-gguf", "--preset",
         "tiny-moe", "--seed", "9", "-o", path], check=True)
    src = _src()
    for keep in (False, True):
        dst = LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(1)
        load_gguf_weights(dst, path, keep_quantized=keep)
        want, got = dict(src.named_parameters()), dict(dst.named_parameters())
        assert set(got) == set(want)
        for name in want:
            assert torch.equal(got[name], want[name]), name


def _rewrite(path, out, rename=None, requant=None, meta=None):
    """Copy a GGUF file tensor by tensor, with tensors renamed / split
    (rename(name, GGMLQuantized-or-tensor) -> {name: value}), re-quantised
    or with other metadata."""
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
    md.update(meta or {})
    write_gguf(out, md, tensors)


def test_gguf_legacy_per_expert_names(tmp_path):
    """blk.i.ffn_gate.{e}.weight etc. load to the same model, resident and
    dense."""
    from helix_amd.engine.gguf import (GGMLQuantized, export_model_gguf,
                                       load_gguf_weights)
    src = _src()
    merged, legacy = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    export_model_gguf(src, merged, quant="q8_0")
    E = PRESETS["tiny-moe"].num_experts

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
    a = LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(1)
    b = LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(2)
    load_gguf_weights(a, merged, keep_quantized=True)
    load_gguf_weights(b, legacy, keep_quantized=True)
    _assert_resident(b, src, "q8_0")
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    a = LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(1)
    b = LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(2)
    load_gguf_weights(a, merged)
    load_gguf_weights(b, legacy)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_gguf_mixed_expert_types(tmp_path):
    """gate Q4_0 with up Q8_0 loads that layer's experts dense and the other
    layer resident; Q4_0 gate/up with a Q8_0 down stays resident with a
    format pair; K-quant flags leave the experts bf16."""
    from helix_amd.engine.gguf import (GGUFFile, export_model_gguf,
                                       load_gguf_weights)
    cfg = PRESETS["tiny-moe"]
    src = _src()
    base = str(tmp_path / "bf16.gguf")
    export_model_gguf(src, base)
    mixed = str(tmp_path / "mixed.gguf")
    _rewrite(base, mixed, requant={
        "blk.0.ffn_gate_exps.weight": "Q4_0",
        "blk.0.ffn_up_exps.weight": "Q8_0",
        "blk.0.ffn_down_exps.weight": "Q4_0",
        "blk.1.ffn_gate_exps.weight": "Q4_0",
        "blk.1.ffn_up_exps.weight": "Q4_0",
        "blk.1.ffn_down_exps.weight": "Q8_0"})
    dst = LlamaForCausalLM(cfg).init_random(1)
    load_gguf_weights(dst, mixed, keep_quantized=True)
    m0, m1 = dst.layers[0].mlp, dst.layers[1].mlp
    assert m0.expert_fmt is None
    I = cfg.intermediate_size
    p13, p2 = _expert_planes(src, "q4_0")[0]
    p13_8, _ = _expert_planes(src, "q8_0")[0]
    assert torch.equal(m0.w13.data[:, :I],
                       ops.dequantize_experts_wq(*p13, "q4_0")[:, :I])
    assert torch.equal(m0.w13.data[:, I:],
                       ops.dequantize_experts_wq(*p13_8, "q8_0")[:, I:])
    assert torch.equal(m0.w2.data, ops.dequantize_experts_wq(*p2, "q4_0"))
    assert m1.expert_fmt == ("q4_0", "q8_0")
    w13, w2 = _expert_planes(src, "q4_0", "q8_0")[1]
    assert torch.equal(m1.w13_qs, w13[0]) and torch.equal(m1.w2_qs, w2[0])
    assert torch.equal(m1.w2_d, w2[1])
    x = torch.randn(3, cfg.hidden_size).to(torch.bfloat16)
    dst = dst.to(torch.bfloat16)
    assert torch.isfinite(dst.layers[1].mlp(x).float()).all()
    # K-quant flags: experts stay bf16, the rest is quantised as before
    kq = str(tmp_path / "kq.gguf")
    export_model_gguf(src, kq, quant="q4_k")
    t = GGUFFile(kq).tensors
    assert t["blk.0.ffn_up_exps.weight"].type_name == "BF16"
    assert t["blk.0.attn_output.weight"].type_name == "Q4_K"
    dst = LlamaForCausalLM(cfg).init_random(1)
    load_gguf_weights(dst, kq, keep_quantized=True)
    assert dst.layers[0].mlp.expert_fmt is None
    assert torch.equal(dst.layers[0].mlp.w13, src.layers[0].mlp.w13)
    # --experts-only: nothing but the experts is quantised
    eo = str(tmp_path / "eo.gguf")
    export_model_gguf(src, eo, quant="q4_0", experts_only=True)
    t = GGUFFile(eo).tensors
    assert t["blk.0.ffn_up_exps.weight"].type_name == "Q4_0"
    assert t["blk.0.attn_output.weight"].type_name == "F32"


def test_gguf_wrong_expert_count_raises(tmp_path):
    from helix_amd.engine.gguf import export_model_gguf, load_gguf_weights
    src = _src()
    good = str(tmp_path / "good.gguf")
    export_model_gguf(src, good, quant="q4_0")
    for key, val in (("llama.expert_count", 4),
                     ("llama.expert_used_count", 1)):
        bad = str(tmp_path / "bad.gguf")
        _rewrite(good, bad, meta={key: val})
        for keep in (False, True):
            dst = LlamaForCausalLM(PRESETS["tiny-moe"]).init_random(1)
            with pytest.raises(ValueError, match=key):
                load_gguf_weights(dst, bad, keep_quantized=keep)
    # a mixture-of-experts file into a dense preset
    dense = LlamaForCausalLM(PRESETS["tiny"]).init_random(1)
    with pytest.raises(ValueError, match="expert_count"):
        load_gguf_weights(dense, good)
