"""Q4_0/Q8_0 weight-only serving, everything that needs no GPU: the
quantizer, the ggml <-> plane layout, the GGUF writer and resident loader,
the model pass, the engine, the memory estimate, and the proof that the GPU
oracle tests (tests/test_wq_gpu.py) can fail: on every GPU case's inputs the
emulation of the kernel's rounding passes and every mutant is rejected.
"""
import functools
import math

import pytest
import torch

import wq_oracle as wo
import helix_amd.ops as ops
from helix_amd.engine import gguf
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import LlamaForCausalLM, PRESETS
from helix_amd.models.quant import WQLinear, quantize_model_wq

TYPE = {"q4_0": "Q4_0", "q8_0": "Q8_0"}
BLOCK_BYTES = {"q4_0": 18, "q8_0": 34}


# -- quantizer on hand-built blocks ---------------------------------------

def test_q4_zero_block():
    qs, d = ops.quantize_wq(torch.zeros(1, 32), "q4_0")
    assert float(d[0, 0]) == 0.0
    assert torch.equal(qs, torch.full((1, 16), 0x88, dtype=torch.uint8))
    assert torch.equal(ops.dequantize_wq(qs, d, "q4_0"), torch.zeros(1, 32))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_q4_extremes(sign):
    """The largest-magnitude element maps to nibble 0 (d = max / -8); the
    opposite extreme would be 16 and clamps to 15."""
    w = torch.zeros(1, 32)
    w[0, 3] = 4.0 * sign           # largest magnitude -> low nibble of byte 3
    w[0, 20] = -4.0 * sign         # opposite extreme  -> high nibble of byte 4
    w[0, 7] = 1.0 * sign
    qs, d = ops.quantize_wq(w, "q4_0")
    assert float(d[0, 0]) == -0.5 * sign
    assert int(qs[0, 3]) & 0x0F == 0
    assert int(qs[0, 4]) >> 4 == 15
    assert int(qs[0, 7]) & 0x0F == 6          # 1/-0.5 + 8.5 = 6.5 -> 6
    assert int(qs[0, 0]) == 0x88
    deq = ops.dequantize_wq(qs, d, "q4_0")
    assert float(deq[0, 3]) == 4.0 * sign
    assert float(deq[0, 20]) == -3.5 * sign


def test_q4_scale_rounded_after_inverse():
    """d is stored as fp16 but the nibbles come from the unrounded d."""
    w = torch.zeros(1, 32)
    w[0, 0] = -8.0 * 0.1234567      # d = 0.1234567, not an fp16 number
    w[0, 1] = 0.1234567 * 6.5       # exactly on the .5 boundary of unrounded d
    qs, d = ops.quantize_wq(w, "q4_0")
    assert d.dtype == torch.float16
    assert float(d[0, 0]) == float(torch.tensor(0.1234567).half())
    x = torch.tensor(0.1234567 * 6.5) * (1.0 / torch.tensor(0.1234567))
    assert int(qs[0, 1]) & 0x0F == min(15, int(float(x + 8.5)))


def test_q8_extremes():
    w = torch.zeros(2, 32)
    w[0, 5], w[0, 9], w[0, 11] = 2.54, -2.54, 0.01
    qs, d = ops.quantize_wq(w, "q8_0")
    assert qs.dtype == torch.int8 and d.dtype == torch.float16
    assert int(qs[0, 5]) == 127 and int(qs[0, 9]) == -127
    assert int(qs[0, 11]) == 1                   # round(0.5) away from zero
    assert float(d[1, 0]) == 0.0 and not qs[1].any()


def test_formats_are_checked():
    with pytest.raises(ValueError):
        ops.quantize_wq(torch.zeros(2, 32), "q5_0")
    with pytest.raises(ValueError):
        ops.quantize_wq(torch.zeros(2, 48), "q4_0")


# -- layout ---------------------------------------------------------------

@pytest.mark.parametrize("fmt", wo.FMTS)
def test_layout_round_trip(fmt):
    torch.manual_seed(1)
    w = torch.randn(48, 160)
    qs, d = ops.quantize_wq(w, fmt)
    assert tuple(d.shape) == (48, 5)
    assert tuple(qs.shape) == ((48, 80) if fmt == "q4_0" else (48, 160))
    raw = ops.pack_ggml(qs, d, fmt)
    assert len(raw) == 48 * 5 * BLOCK_BYTES[fmt]
    info = gguf.GGUFTensorInfo("w", (48, 160),
                               gguf._NAME_TO_GGML[TYPE[fmt]], 0)
    via_ggml = gguf._dequantize(raw, info).reshape(48, 160)
    assert torch.equal(via_ggml, ops.dequantize_wq(qs, d, fmt))
    qs2, d2 = ops.unpack_ggml(raw, (48, 160), fmt)
    assert qs2.dtype == qs.dtype and torch.equal(qs2, qs)
    assert torch.equal(d2, d)
    # quantization error is what the format allows: half a step (a whole
    # one at the clamped q4_0 extreme) plus the fp16 rounding of d, which
    # moves an element by at most |q| * d * 2^-11
    step = d.float().abs().repeat_interleave(32, dim=1)
    bound = (1.0 + 8 * 2.0 ** -11) if fmt == "q4_0" else (0.5 + 127 * 2.0 ** -11)
    assert ((via_ggml - w).abs() <= step * bound + 1e-6).all()


@pytest.mark.parametrize("fmt", wo.FMTS)
def test_writer_quantized(tmp_path, fmt):
    torch.manual_seed(2)
    w = torch.randn(32, 64)
    norm = torch.randn(64)
    qt = gguf.quantize_ggml(w, TYPE[fmt])
    path = str(tmp_path / "q.gguf")
    gguf.write_gguf(path, {"general.architecture": "llama"},
                    {"blk.0.ffn_down.weight": qt, "output_norm.weight": norm})
    g = gguf.GGUFFile(path)
    assert g.tensors["blk.0.ffn_down.weight"].type_name == TYPE[fmt]
    assert g.tensors["blk.0.ffn_down.weight"].shape == (32, 64)
    want = ops.dequantize_wq(*ops.quantize_wq(w, fmt), fmt)
    assert torch.equal(g.load_tensor("blk.0.ffn_down.weight"), want)
    assert torch.equal(g.load_tensor("output_norm.weight"), norm)
    assert g.tensor_bytes() == 32 * 2 * BLOCK_BYTES[fmt] + 64 * 4
    with pytest.raises(ValueError):
        gguf.write_gguf(path, {}, {"w": gguf.GGMLQuantized(
            qt.raw[:-1], (32, 64), TYPE[fmt])})


# -- resident load --------------------------------------------------------

def _permute(w, n_head):
    o, i = w.shape
    return (w.reshape(n_head, 2, o // n_head // 2, i)
            .swapaxes(1, 2).reshape(o, i))


def _export(src, path, types):
    """Converter-style file: llama.cpp names, Q/K permuted; `types` maps a
    projection part ("attn_q", ...) to its ggml type."""
    cfg = src.cfg
    q, kv, inter = cfg.q_size, cfg.kv_size, cfg.intermediate_size
    sd = dict(src.named_parameters())
    tensors = {"token_embd.weight": sd["embed_tokens.weight"].data,
               "output_norm.weight": sd["final_norm_w"].data,
               "output.weight": sd["lm_head.weight"].data}
    for i in range(cfg.num_layers):
        qkv = sd[f"layers.{i}.attn.qkv_proj.weight"].data
        gu = sd[f"layers.{i}.mlp.gate_up_proj.weight"].data
        parts = {
            "attn_q": _permute(qkv[:q], cfg.num_heads),
            "attn_k": _permute(qkv[q:q + kv], cfg.num_kv_heads),
            "attn_v": qkv[q + kv:],
            "attn_output": sd[f"layers.{i}.attn.o_proj.weight"].data,
            "ffn_gate": gu[:inter], "ffn_up": gu[inter:],
            "ffn_down": sd[f"layers.{i}.mlp.down_proj.weight"].data}
        for p, w in parts.items():
            tensors[f"blk.{i}.{p}.weight"] = gguf.quantize_ggml(
                w.float(), types[p])
        tensors[f"blk.{i}.attn_norm.weight"] = \
            sd[f"layers.{i}.input_norm_w"].data
        tensors[f"blk.{i}.ffn_norm.weight"] = \
            sd[f"layers.{i}.post_norm_w"].data
    gguf.write_gguf(path, {"general.architecture": "llama"}, tensors)
    return tensors


def _logits(model, ids):
    from helix_amd.engine.kv_cache import KVCache
    from helix_amd.models.llama import PrefillMeta
    cfg = model.cfg
    kv = KVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim, 16, 8,
                 torch.device("cpu"),
                 dtype=next(model.parameters()).dtype)
    T = len(ids)
    meta = PrefillMeta(
        cu_seqlens=torch.tensor([0, T], dtype=torch.int32), max_seqlen=T,
        slot_mapping=torch.arange(T, dtype=torch.int64),
        positions=torch.arange(T, dtype=torch.int64))
    with torch.inference_mode():
        h = model(torch.tensor(ids, dtype=torch.int64), kv.caches, meta)
        return model.compute_logits(h)


PARTS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up",
         "ffn_down")


def test_resident_load(tmp_path):
    torch.manual_seed(0)
    cfg = PRESETS["tiny"]
    src = LlamaForCausalLM(cfg)
    path = str(tmp_path / "tiny-q4.gguf")
    tensors = _export(src, path, {p: "Q4_0" for p in PARTS})

    dense = LlamaForCausalLM(cfg)
    assert gguf.load_gguf_weights(dense, path) == len(tensors)
    res = LlamaForCausalLM(cfg)
    assert gguf.load_gguf_weights(res, path, keep_quantized=True) \
        == len(tensors)

    q, kv = cfg.q_size, cfg.kv_size
    for i, layer in enumerate(res.layers):
        for m in (layer.attn.qkv_proj, layer.attn.o_proj,
                  layer.mlp.gate_up_proj, layer.mlp.down_proj):
            assert isinstance(m, WQLinear) and m.fmt == "q4_0"
        # the planes hold the file's own blocks: V and O rows as they are,
        # Q rows after the whole-row un-permutation
        qkv = layer.attn.qkv_proj
        v_qs, v_d = ops.unpack_ggml(
            tensors[f"blk.{i}.attn_v.weight"].raw, (kv, cfg.hidden_size),
            "q4_0")
        assert torch.equal(qkv.qs[q + kv:], v_qs)
        assert torch.equal(qkv.d[q + kv:], v_d)
        q_qs, q_d = ops.unpack_ggml(
            tensors[f"blk.{i}.attn_q.weight"].raw, (q, cfg.hidden_size),
            "q4_0")
        assert torch.equal(qkv.qs[:q], gguf.unpermute_rope(q_qs, cfg.num_heads))
        assert torch.equal(qkv.d[:q], gguf.unpermute_rope(q_d, cfg.num_heads))
        raw = ops.pack_ggml(layer.attn.o_proj.qs, layer.attn.o_proj.d, "q4_0")
        assert raw == tensors[f"blk.{i}.attn_output.weight"].raw
    assert isinstance(res.lm_head, torch.nn.Linear)
    assert not isinstance(dense.layers[0].attn.qkv_proj, WQLinear)

    ids = [5, 9, 2, 77, 31, 8]
    assert torch.equal(_logits(dense, ids), _logits(res, ids))


def test_resident_load_mixed_types_stay_dense(tmp_path):
    torch.manual_seed(0)
    cfg = PRESETS["tiny"]
    src = LlamaForCausalLM(cfg)
    path = str(tmp_path / "tiny-mixed.gguf")
    types = {p: "Q4_0" for p in PARTS}
    types["attn_v"] = "Q8_0"
    _export(src, path, types)
    dense = LlamaForCausalLM(cfg)
    gguf.load_gguf_weights(dense, path)
    res = LlamaForCausalLM(cfg)
    gguf.load_gguf_weights(res, path, keep_quantized=True)
    for layer in res.layers:
        assert type(layer.attn.qkv_proj) is not WQLinear
        assert isinstance(layer.attn.qkv_proj, torch.nn.Linear)
        assert isinstance(layer.attn.o_proj, WQLinear)
        assert isinstance(layer.mlp.gate_up_proj, WQLinear)
    ids = [5, 9, 2, 77, 31, 8]
    assert torch.equal(_logits(dense, ids), _logits(res, ids))


def test_weights_loader_passes_keep_quantized(tmp_path):
    from helix_amd.engine.weights import load_llama_weights
    torch.manual_seed(0)
    cfg = PRESETS["tiny"]
    path = str(tmp_path / "tiny-q8.gguf")
    _export(LlamaForCausalLM(cfg), path, {p: "Q8_0" for p in PARTS})
    m = LlamaForCausalLM(cfg)
    load_llama_weights(m, path, keep_quantized=True)
    assert m.layers[0].mlp.down_proj.fmt == "q8_0"
    m = LlamaForCausalLM(cfg)
    load_llama_weights(m, path)
    assert isinstance(m.layers[0].mlp.down_proj, torch.nn.Linear)


# -- model pass, engine, estimate -----------------------------------------

def test_model_pass():
    m = LlamaForCausalLM(PRESETS["tiny"])
    m.init_random(0)
    n = quantize_model_wq(m, "q4_0")
    assert n == 4 * PRESETS["tiny"].num_layers
    assert isinstance(m.lm_head, torch.nn.Linear)
    assert all(isinstance(l.mlp.down_proj, WQLinear) for l in m.layers)

    m = LlamaForCausalLM(PRESETS["tiny-qwen"])
    m.init_random(0)
    bias = m.layers[0].attn.qkv_proj.bias.data.clone()
    assert quantize_model_wq(m, "q8_0") == 4 * PRESETS["tiny-qwen"].num_layers
    qkv = m.layers[0].attn.qkv_proj
    assert isinstance(qkv, WQLinear) and torch.equal(qkv.bias, bias)
    assert m.layers[0].attn.o_proj.bias is None


def test_dtype_cast_keeps_scales_fp16():
    """model.to(dtype) converts every floating buffer; the block scales are
    fp16 by format and must come through bit for bit."""
    m = LlamaForCausalLM(PRESETS["tiny-qwen"])
    m.init_random(0)
    quantize_model_wq(m, "q4_0")
    qkv = m.layers[0].attn.qkv_proj
    d, qs = qkv.d.clone(), qkv.qs.clone()
    for cast in (lambda x: x.to(torch.bfloat16), lambda x: x.half(),
                 lambda x: x.float()):
        cast(m)
        qkv = m.layers[0].attn.qkv_proj
        assert qkv.d.dtype == torch.float16 and torch.equal(qkv.d, d)
        assert torch.equal(qkv.qs, qs)
    assert qkv.bias.dtype == torch.float32
    assert qkv.scratch is None            # CPU modules need none


def test_cutoff_is_a_graph_bucket():
    from helix_amd.engine.graph_runner import BATCH_BUCKETS
    assert ops.WQ_FUSED_MAX_M in BATCH_BUCKETS
    if ops.have_native():
        assert ops.WQ_FUSED_MAX_M <= ops._C.WQ_KERNEL_MAX_M


@pytest.mark.parametrize("fmt", wo.FMTS)
def test_engine_equals_dequantized_bf16_engine(fmt):
    """Exact: on the CPU a WQLinear computes F.linear on the dequantized
    weight, so the quantized engine and a bf16 engine carrying those
    weights generate the same tokens."""
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    prompts = [[1, 2, 3, 4, 5], [7, 8]]
    base = dict(model="tiny-gqa", max_model_len=512, max_num_seqs=8,
                kv_cache_blocks=256, eos_token_id=-1, seed=7)
    quant = LLMEngine(EngineConfig(**base, quantization=fmt), device="cpu")
    assert isinstance(quant.model.layers[0].attn.qkv_proj, WQLinear)
    ref = LLMEngine(EngineConfig(**base), device="cpu")
    for layer in ref.model.layers:
        for lin in (layer.attn.qkv_proj, layer.attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            lin.weight.data.copy_(ops.dequantize_wq(
                *ops.quantize_wq(lin.weight.data, fmt), fmt))
    got = quant.generate(prompts, sp)
    assert got == ref.generate(prompts, sp)
    assert all(len(g) == 12 for g in got)
    # an engine handed a model that already holds WQLinears leaves it alone
    again = LLMEngine(EngineConfig(**base, quantization=fmt), device="cpu",
                      model=quant.model)
    assert again.model.layers[0].attn.qkv_proj is \
        quant.model.layers[0].attn.qkv_proj


def test_estimate():
    from helix_amd.runner.service import ModelSpec, estimate_model_bytes
    est = {q: estimate_model_bytes(ModelSpec("m", "llm", "llama3-8b",
                                             quantization=q))
           for q in (None, "fp8", "q8_0", "q4_0")}
    assert est["q4_0"] < est["fp8"] < est["q8_0"] < est[None]
    cfg = PRESETS["llama3-8b"]
    elems = cfg.num_layers * (
        cfg.hidden_size * (cfg.q_size + 2 * cfg.kv_size)
        + cfg.q_size * cfg.hidden_size
        + 3 * cfg.hidden_size * cfg.intermediate_size)
    # plus the model's dequant scratch: its largest projection in bf16
    scratch = 2 * max(cfg.hidden_size * (cfg.q_size + 2 * cfg.kv_size),
                      2 * cfg.hidden_size * cfg.intermediate_size)
    assert est[None] - est["q4_0"] == 2 * elems - 18 * elems // 32 - scratch
    assert est[None] - est["q8_0"] == 2 * elems - 34 * elems // 32 - scratch
    assert isinstance(est["q4_0"], int)


# -- oracle, emulation, mutants -------------------------------------------

@functools.lru_cache(maxsize=None)
def _result(case):
    """(emulation error, {mutant: error}) of one case."""
    b = wo.build(case)
    emul = wo.emulate(b.x, ops.dequantize_wq(b.qs, b.d, case.fmt), b.bias)
    e = wo.assert_wq_close(emul, b.want, wo.TOL_WQ, f"{case.id} emulation")
    errs = {}
    for name, got in wo.mutant_outputs(case, b).items():
        with pytest.raises(AssertionError):
            wo.assert_wq_close(got, b.want, wo.TOL_WQ, f"{case.id} {name}")
        errs[name] = float(wo.wq_error(got, b.want).max())
    return e, errs


ALL_CASES = list(dict.fromkeys(wo.CASES + wo.FALLBACK_CASES))


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_case_can_fail(case):
    e, errs = _result(case)
    assert set(errs) == (wo.MUTANTS_Q4 if case.fmt == "q4_0"
                         else wo.MUTANTS_Q8)
    print(f"{case.id}: emulation {e:.5f} passes tol {wo.TOL_WQ}; rejected: "
          + ", ".join(f"{n} {v:.3f}" for n, v in sorted(errs.items())))


def test_cpu_op_is_the_definition():
    """ops.gemm_wq on CPU tensors is F.linear on the dequantized weight."""
    case = wo.Case("q4_0", 17, 48, 160, True, "randn")
    b = wo.build(case)
    got = ops.gemm_wq(b.x, b.qs, b.d, "q4_0", b.bias)
    want = torch.nn.functional.linear(
        b.x, ops.dequantize_wq(b.qs, b.d, "q4_0", torch.bfloat16), b.bias)
    assert torch.equal(got, want)
    wo.assert_wq_close(got, b.want, wo.TOL_WQ, "cpu op")


def test_tolerance():
    """tol = 4 x the worst emulation error (within rounding of the
    constant), and every mutant misses it by a wide factor.

    The weakest pairs are known beforehand: one of K/32 blocks dropped from
    i.i.d. inputs (randn family) removes 32/K of a row's variance, a
    relative error of sqrt(32/K) in expectation: 0.124 at K = 2080 and
    0.088 at K = 4128. Those pairs must clear 2.5 x tol; every other
    (mutant, case) pair 6 x tol."""
    cases = ALL_CASES
    res = [_result(c) for c in cases]
    worst = max(r[0] for r in res)
    pairs = [(v, n, c) for c, r in zip(cases, res) for n, v in r[1].items()]
    weak = [p for p in pairs if p[1] == "drop_last_k_block"
            and p[2].K >= 2080 and p[2].family == "randn"]
    rest = [p for p in pairs if p not in weak]
    sw = min(weak, key=lambda p: p[0])
    sr = min(rest, key=lambda p: p[0])
    print(f"worst emulation error {worst:.5f}, tol {wo.TOL_WQ}; smallest "
          f"mutant error {sw[0]:.4f} ({sw[1]}, {sw[2].id}) = "
          f"{sw[0] / wo.TOL_WQ:.1f} x tol; next {sr[0]:.4f} ({sr[1]}, "
          f"{sr[2].id}) = {sr[0] / wo.TOL_WQ:.1f} x tol")
    assert 4 * worst <= wo.TOL_WQ * 1.02, worst
    assert wo.TOL_WQ <= 4 * worst * 1.10, worst
    assert sw[0] >= 2.5 * wo.TOL_WQ, sw
    assert sr[0] >= 6 * wo.TOL_WQ, sr


def test_metric_reports_the_worst_row():
    want = torch.randn(3, 8, dtype=torch.float64)
    got = want.clone()
    assert wo.assert_wq_close(got, want, 1e-9) == 0.0
    got[2, 5] += 1.0
    with pytest.raises(AssertionError, match=r"row 2 .*channel 5"):
        wo.assert_wq_close(got, want, 1e-3)
    got = want.clone()
    got[0, 0] = math.nan
    with pytest.raises(AssertionError, match="non-finite"):
        wo.assert_wq_close(got, want, 1e-3)


def test_export_gguf_quant_cli(tmp_path):
    """`helix export-gguf --quant q4_0` writes Q4_0 projections (norms and
    embeddings as before) that load resident."""
    import subprocess
    import sys
    out = str(tmp_path / "tiny-q4.gguf")
    r = subprocess.run(
        [sys.executable, "-m", "helix_amd.cli", "export-gguf", "--preset",
         "tiny", "-o", out, "--seed", "3", "--quant", "q4_0"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    g = gguf.GGUFFile(out)
    assert g.tensors["blk.0.ffn_down.weight"].type_name == "Q4_0"
    assert g.tensors["blk.0.attn_q.weight"].type_name == "Q4_0"
    assert g.tensors["token_embd.weight"].type_name != "Q4_0"
    assert g.tensors["blk.0.attn_norm.weight"].type_name != "Q4_0"
    m = LlamaForCausalLM(PRESETS["tiny"])
    gguf.load_gguf_weights(m, out, keep_quantized=True)
    assert sum(isinstance(x, WQLinear) for x in m.modules()) \
        == 4 * PRESETS["tiny"].num_layers
