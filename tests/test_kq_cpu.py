"""Q4_K/Q6_K weight-only serving, everything that needs no GPU: the block
decoders against a byte-by-byte transcription of the format, the quantizer,
the ggml <-> plane layout, the GGUF loader (dense and resident, a Q4_K_M
file), the model pass, the engine, the memory estimate, and the proof that
the GPU oracle tests (tests/test_kq_gpu.py) can fail: on every GPU case's
inputs the emulation of the kernel's rounding passes and every mutant is
rejected.
"""
import functools
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import kq_oracle as ko
import helix_amd.ops as ops
from helix_amd.engine import gguf
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import LlamaForCausalLM, PRESETS
from helix_amd.models.quant import KQLinear, WQLinear, quantize_model_wq

TYPE = {"q4_k": "Q4_K", "q6_k": "Q6_K"}
BLOCK_BYTES = {"Q4_K": 144, "Q5_K": 176, "Q6_K": 210}


# -- scalar decoders: the format text, transcribed ------------------------

def _f16(b):
    return np.float32(struct.unpack("<e", bytes(b))[0])


def _scale_min(scales, j):
    if j < 4:
        return scales[j] & 63, scales[j + 4] & 63
    sc = (scales[j + 4] & 0xF) | ((scales[j - 4] >> 6) << 4)
    m = (scales[j + 4] >> 4) | ((scales[j] >> 6) << 4)
    return sc, m


def _decode_q45_k(blk, five):
    """One block_q4_K (144 bytes) or block_q5_K (176) -> 256 np.float32."""
    d, dmin, scales = _f16(blk[0:2]), _f16(blk[2:4]), blk[4:16]
    qh = blk[16:48] if five else None
    qs = blk[48:176] if five else blk[16:144]
    y = np.zeros(256, dtype=np.float32)
    for j in range(8):
        sc, m = _scale_min(scales, j)
        ds = np.float32(d * np.float32(sc))
        dm = np.float32(dmin * np.float32(m))
        for l in range(32):
            byte = qs[32 * (j // 2) + l]
            q = (byte >> 4) if j & 1 else (byte & 0xF)
            if five:
                q += 16 * ((qh[l] >> j) & 1)
            y[32 * j + l] = np.float32(ds * np.float32(q)) - dm
    return y


def _decode_q6_k(blk):
    """One block_q6_K (210 bytes) -> 256 np.float32."""
    ql, qh = blk[0:128], blk[128:192]
    scales = struct.unpack("<16b", bytes(blk[192:208]))
    d = _f16(blk[208:210])
    y = np.zeros(256, dtype=np.float32)
    for h in range(2):
        for g in range(4):
            for l in range(32):
                byte = ql[64 * h + 32 * (g & 1) + l]
                low4 = (byte & 0xF) if g < 2 else (byte >> 4)
                high2 = (qh[32 * h + l] >> (2 * g)) & 3
                q = (low4 | (high2 << 4)) - 32
                ds = np.float32(d * np.float32(scales[8 * h + 2 * g + l // 16]))
                y[128 * h + 32 * g + l] = ds * np.float32(q)
    return y


def _random_blocks(tname, n, seed):
    """n blocks of random bytes in every field; the fp16 fields are finite
    and normal (exponent field 1..30), either sign."""
    rng = np.random.default_rng(seed)
    bsz = BLOCK_BYTES[tname]
    blk = rng.integers(0, 256, size=(n, bsz), dtype=np.uint8)
    for off in ((208,) if tname == "Q6_K" else (0, 2)):
        bits = rng.integers(0, 1 << 16, size=n).astype(np.uint16)
        exp = rng.integers(1, 31, size=n).astype(np.uint16)
        bits = (bits & 0x83FF) | (exp << 10)
        blk[:, off] = bits & 0xFF
        blk[:, off + 1] = bits >> 8
    return blk


def _scalar(tname, blk):
    if tname == "Q6_K":
        return np.concatenate([_decode_q6_k(b) for b in blk.tolist()])
    return np.concatenate([_decode_q45_k(b, tname == "Q5_K")
                           for b in blk.tolist()])


@pytest.mark.parametrize("tname", ["Q4_K", "Q5_K", "Q6_K"])
def test_decoders_equal_the_scalar_transcription(tname):
    N, K = 32, 2048            # 256 blocks: 1024 draws per packing of a code
    blk = _random_blocks(tname, N * K // 256, seed=len(tname) + ord(tname[1]))
    if tname != "Q6_K":
        # all 64 codes occur as a scale and as a min, in both packings
        codes = {(j, _scale_min(b[4:16], j)) for b in blk.tolist()
                 for j in range(8)}
        for half in (range(4), range(4, 8)):
            assert {c[0] for j, c in codes if j in half} == set(range(64))
            assert {c[1] for j, c in codes if j in half} == set(range(64))
    want = torch.from_numpy(_scalar(tname, blk)).reshape(N, K)
    assert torch.isfinite(want).all()
    raw = blk.tobytes()
    info = gguf.GGUFTensorInfo("w", (N, K), gguf._NAME_TO_GGML[tname], 0)
    got = gguf._dequantize(raw, info).reshape(N, K)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    if tname == "Q5_K":
        return
    fmt = tname.lower()
    planes = ops.unpack_ggml_kq(raw, (N, K), fmt)
    assert torch.equal(ops.dequantize_kq(planes, fmt), want)
    assert torch.equal(ops.dequantize_kq(planes, fmt, torch.bfloat16),
                       want.to(torch.bfloat16))
    # the single fma the kernel uses rounds the same exact value once
    if fmt == "q4_k":
        d, dmin, sc, m, lo, hi = ko._q4k_fields(planes)
        nib = torch.stack([lo, hi], dim=3).reshape(N, K // 256, 8, 32)
        exact = ((d * sc).double()[..., None] * nib.double()
                 - (dmin * m).double()[..., None]).reshape(N, K)
    else:
        low, qh, sc, d = ko._q6k_fields(planes)
        high = ((qh >> ko._SHIFTS) & 3).to(torch.int32)
        s = (d * sc.float()).double().reshape(N, K // 256, 2, 4, 2, 1)
        u = (low | (high << 4)).reshape(N, K // 256, 2, 4, 2, 16).double()
        exact = (u * s + (-32.0 * s)).reshape(N, K)
    assert torch.equal(exact.float(), want)


# -- layout and quantizer ---------------------------------------------------

@pytest.mark.parametrize("fmt", ko.FMTS)
def test_layout_round_trip(fmt):
    N, K = 48, 768
    raw = _random_blocks(TYPE[fmt], N * K // 256, seed=3).tobytes()
    planes = ops.unpack_ggml_kq(raw, (N, K), fmt)
    if fmt == "q4_k":
        qs, hdr = planes
        assert qs.dtype == torch.uint8 and tuple(qs.shape) == (N, K // 2)
        assert hdr.dtype == torch.uint8 and tuple(hdr.shape) == (N, 3, 16)
        assert bytes(hdr[1, 2].tolist()) == raw[(3 + 2) * 144:][:16]
    else:
        ql, qh, sc, d = planes
        assert ql.dtype == torch.uint8 and tuple(ql.shape) == (N, K // 2)
        assert qh.dtype == torch.uint8 and tuple(qh.shape) == (N, K // 4)
        assert sc.dtype == torch.int8 and tuple(sc.shape) == (N, K // 16)
        assert d.dtype == torch.float16 and tuple(d.shape) == (N, 3)
    assert all(p.is_contiguous() for p in planes)
    assert ops.pack_ggml_kq(planes, fmt) == raw
    assert ops.kq_shape(planes, fmt) == (N, K)
    with pytest.raises(ValueError):
        ops.unpack_ggml_kq(raw[:-1], (N, K), fmt)
    with pytest.raises(ValueError):
        ops.unpack_ggml_kq(raw, (N, K), "q5_k")


@pytest.mark.parametrize("fmt,bound", [("q4_k", 0.10), ("q6_k", 0.03)])
def test_quantizer_round_trip(fmt, bound):
    torch.manual_seed(1)
    w = torch.randn(64, 1024)
    planes = ops.quantize_kq(w, fmt)
    back = ops.dequantize_kq(planes, fmt)
    rel = float((back - w).norm() / w.norm())
    print(f"{fmt}: round-trip relative error {rel:.4f} (bound {bound})")
    assert rel < bound
    raw = ops.pack_ggml_kq(planes, fmt)
    assert len(raw) == 64 * 4 * BLOCK_BYTES[TYPE[fmt]]
    again = ops.unpack_ggml_kq(raw, (64, 1024), fmt)
    assert all(torch.equal(a, b) and a.dtype == b.dtype
               for a, b in zip(again, planes))
    assert ops.quantize_kq(w, fmt)[0].equal(planes[0])      # deterministic
    qt = gguf.quantize_ggml(w, TYPE[fmt])
    assert qt.raw == raw and qt.type_name == TYPE[fmt]


@pytest.mark.parametrize("fmt", ko.FMTS)
def test_zero_blocks(fmt):
    w = torch.randn(16, 512, generator=torch.Generator().manual_seed(4))
    w[:, :256] = 0                   # a zero super-block
    w[3] = 0                         # a zero row
    w[5, 256:288] = 0                # a zero sub-block among others
    planes = ops.quantize_kq(w, fmt)
    back = ops.dequantize_kq(planes, fmt)
    assert torch.isfinite(back).all()
    assert not back[:, :256].any() and not back[3].any()
    if fmt == "q4_k":                 # (q6_k codes a zero as 32)
        assert not any(p[3].any() for p in planes)
    assert float((back - w).norm() / w.norm()) < 0.10
    with pytest.raises(ValueError):
        ops.quantize_kq(torch.zeros(16, 128), fmt)
    with pytest.raises(ValueError):
        ops.quantize_kq(w, "q5_k")


def test_existing_formats_are_untouched():
    assert set(ops.WQ_FORMATS) == {"q4_0", "q8_0"}
    assert ops.KQ_FORMATS == {"q4_k", "q6_k"}
    with pytest.raises(ValueError):
        ops.wq_bits("q4_k")


# -- oracle, emulation, mutants -------------------------------------------

@functools.lru_cache(maxsize=None)
def _result(case):
    """(emulation error, {mutant: error}) of one case."""
    b = ko.build(case)
    emul = ko.emulate(b.x, ops.dequantize_kq(b.planes, case.fmt), b.bias)
    e = ko.assert_wq_close(emul, b.want, ko.TOL_KQ, f"{case.id} emulation")
    errs = {}
    for name, got in ko.mutant_outputs(case, b).items():
        with pytest.raises(AssertionError):
            ko.assert_wq_close(got, b.want, ko.TOL_KQ, f"{case.id} {name}")
        errs[name] = float(ko.wq_error(got, b.want).max())
    return e, errs


@pytest.mark.parametrize("case", ko.CASES, ids=lambda c: c.id)
def test_case_can_fail(case):
    e, errs = _result(case)
    own = ko.MUTANTS_Q4K if case.fmt == "q4_k" else ko.MUTANTS_Q6K
    assert set(errs) == own | ko.MUTANTS_BOTH
    print(f"{case.id}: emulation {e:.5f} passes tol {ko.TOL_KQ}; rejected: "
          + ", ".join(f"{n} {v:.3f}" for n, v in sorted(errs.items())))


def test_tolerance():
    """TOL_KQ is the Q4_0/Q8_0 tests' 4 x 0.0068 as long as the K-quant
    emulation's worst error over all cases is within 0.0068, and every
    mutant misses it by at least 2 x. Prints the table of the smallest
    error of each mutant."""
    res = [_result(c) for c in ko.CASES]
    worst = max(r[0] for r in res)
    table = {}
    for c, r in zip(ko.CASES, res):
        for n, v in r[1].items():
            if n not in table or v < table[n][0]:
                table[n] = (v, c.id)
    print(f"worst emulation error {worst:.5f}, tol {ko.TOL_KQ}")
    for n, (v, cid) in sorted(table.items(), key=lambda kv: kv[1][0]):
        print(f"  {n:28s} {v:8.4f} = {v / ko.TOL_KQ:6.1f} x tol  ({cid})")
    assert worst <= 0.0068, worst
    assert min(v for v, _ in table.values()) >= 2 * ko.TOL_KQ, table


def test_cpu_op_is_the_definition():
    """ops.gemm_kq on CPU tensors is F.linear on the dequantized weight,
    written into the segment's columns of `out`."""
    for fmt in ko.FMTS:
        b = ko.build(ko.Case(fmt, 17, 48, 768, True, "randn"))
        want = torch.nn.functional.linear(
            b.x, ops.dequantize_kq(b.planes, fmt, torch.bfloat16), b.bias)
        assert torch.equal(ops.gemm_kq(b.x, b.planes, fmt, b.bias), want)
        ko.assert_wq_close(want, b.want, ko.TOL_KQ, "cpu op")
        buf = torch.full((17, 80), float("nan"), dtype=torch.bfloat16)
        bias = torch.cat([torch.zeros(16, dtype=torch.bfloat16), b.bias,
                          torch.zeros(16, dtype=torch.bfloat16)])
        assert ops.gemm_kq(b.x, b.planes, fmt, bias, out=buf,
                           col_off=16) is buf
        assert torch.equal(buf[:, 16:64], want)
        assert torch.isnan(buf[:, :16]).all() and torch.isnan(buf[:, 64:]).all()
        assert torch.equal(ops.dequant_kq(b.planes, fmt),
                           ops.dequantize_kq(b.planes, fmt, torch.bfloat16))
    with pytest.raises(ValueError):
        ops.gemm_kq(b.x, b.planes, "q5_k")


def test_cutoff_is_a_graph_bucket():
    from helix_amd.engine.graph_runner import BATCH_BUCKETS
    assert ops.KQ_FUSED_MAX_M in BATCH_BUCKETS
    assert ops.KQ_FUSED_MAX_M <= ko.KQ_KERNEL_MAX_M
    if ops.have_native():
        assert ops._C.KQ_KERNEL_MAX_M == ko.KQ_KERNEL_MAX_M


# -- GGUF: a Q4_K_M file ----------------------------------------------------

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


def _export_cli(path, quant, preset="tiny"):
    r = subprocess.run(
        [sys.executable, "-m", "helix_amd.cli", "export-gguf", "--preset",
         preset, "-o", path, "--seed", "3", "--quant", quant],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def q4_k_m_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("kq") / "tiny-q4_k_m.gguf")
    _export_cli(path, "q4_k_m")
    return path


def test_q4_k_m_rule():
    n = 32
    more = [i for i in range(n) if gguf.q4_k_m_uses_q6_k(i, n)]
    assert more == [0, 1, 2, 3, 6, 9, 12, 15, 18, 21, 24, 27, 28, 29, 30, 31]
    assert [gguf.q4_k_m_uses_q6_k(i, 2) for i in range(2)] == [False, True]


def test_q4_k_m_file_types(q4_k_m_file):
    g = gguf.GGUFFile(q4_k_m_file)
    cfg = PRESETS["tiny"]
    for i in range(cfg.num_layers):
        more = gguf.q4_k_m_uses_q6_k(i, cfg.num_layers)
        for part in ("attn_q", "attn_k", "attn_output", "ffn_gate", "ffn_up"):
            assert g.tensors[f"blk.{i}.{part}.weight"].type_name == "Q4_K"
        for part in ("attn_v", "ffn_down"):
            assert g.tensors[f"blk.{i}.{part}.weight"].type_name == \
                ("Q6_K" if more else "Q4_K")
        assert g.tensors[f"blk.{i}.attn_norm.weight"].type_name == "F32"
    assert g.tensors["output.weight"].type_name == "Q6_K"
    assert g.tensors["token_embd.weight"].type_name == "Q4_K"


def test_q4_k_m_dense_and_resident_load(q4_k_m_file):
    cfg = PRESETS["tiny"]
    g = gguf.GGUFFile(q4_k_m_file)
    dense = LlamaForCausalLM(cfg)
    # the dense load alone needs the K-quant decoders
    assert gguf.load_gguf_weights(dense, q4_k_m_file) == len(g.tensors)
    res = LlamaForCausalLM(cfg)
    assert gguf.load_gguf_weights(res, q4_k_m_file, keep_quantized=True) \
        == len(g.tensors)
    assert not any(isinstance(m, KQLinear) for m in dense.modules())
    assert isinstance(res.lm_head, torch.nn.Linear)
    assert not isinstance(res.embed_tokens, KQLinear)

    q, kv = cfg.q_size, cfg.kv_size
    some_q6 = False
    for i, layer in enumerate(res.layers):
        more = gguf.q4_k_m_uses_q6_k(i, cfg.num_layers)
        some_q6 |= more
        vfmt = "q6_k" if more else "q4_k"
        mods = (layer.attn.qkv_proj, layer.attn.o_proj,
                layer.mlp.gate_up_proj, layer.mlp.down_proj)
        assert all(isinstance(m, KQLinear) for m in mods)
        qkv = layer.attn.qkv_proj
        assert qkv.fmts == ["q4_k", "q4_k", vfmt]
        assert qkv.rows == [0, q, q + kv]
        assert layer.attn.o_proj.fmts == ["q4_k"]
        assert layer.mlp.gate_up_proj.fmts == ["q4_k", "q4_k"]
        assert layer.mlp.down_proj.fmts == [vfmt]
        # the planes hold the file's own blocks: V, O, gate, up and down
        # re-pack to the raw bytes; Q and K after the whole-row permutation
        for mod, seg, name in ((qkv, 2, "attn_v"),
                               (layer.attn.o_proj, 0, "attn_output"),
                               (layer.mlp.gate_up_proj, 0, "ffn_gate"),
                               (layer.mlp.gate_up_proj, 1, "ffn_up"),
                               (layer.mlp.down_proj, 0, "ffn_down")):
            raw = g.read_raw(f"blk.{i}.{name}.weight")
            assert ops.pack_ggml_kq(mod.planes(seg), mod.fmts[seg]) == raw
        for seg, name, heads in ((0, "attn_q", cfg.num_heads),
                                 (1, "attn_k", cfg.num_kv_heads)):
            info = g.tensors[f"blk.{i}.{name}.weight"]
            filed = ops.unpack_ggml_kq(g.read_raw(info.name), info.shape,
                                       "q4_k")
            for got, f in zip(qkv.planes(seg), filed):
                want = gguf.unpermute_rope(f.reshape(f.shape[0], -1), heads)
                assert torch.equal(got.reshape(got.shape[0], -1), want)
    assert some_q6

    ids = [5, 9, 2, 77, 31, 8]
    assert torch.equal(_logits(dense, ids), _logits(res, ids))


def test_q5_k_file_loads_dense(tmp_path):
    """A Q5_K tensor (a Q5_K_M file's bulk) has no resident form: it loads
    dense, also with keep_quantized."""
    cfg = PRESETS["tiny"]
    blk = _random_blocks("Q5_K", cfg.hidden_size * cfg.q_size // 256, seed=9)
    # small magnitudes, as a weight: d, dmin exponents near 2^-8
    blk[:, 1] = (blk[:, 1] & 0x83) | 0x1C
    blk[:, 3] = (blk[:, 3] & 0x83) | 0x1C
    qt = gguf.GGMLQuantized(blk.tobytes(), (cfg.q_size, cfg.hidden_size),
                            "Q5_K")
    path = str(tmp_path / "q5.gguf")
    gguf.write_gguf(path, {"general.architecture": "llama"},
                    {"blk.0.attn_output.weight": qt})
    want = torch.from_numpy(_scalar("Q5_K", blk)).reshape(qt.shape)
    for keep in (False, True):
        m = LlamaForCausalLM(cfg)
        assert gguf.load_gguf_weights(m, path, keep_quantized=keep) == 1
        o = m.layers[0].attn.o_proj
        assert isinstance(o, torch.nn.Linear)
        assert torch.equal(o.weight.data, want.to(o.weight.dtype))


PARTS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up",
         "ffn_down")


def _permute(w, n_head):
    o, i = w.shape
    return (w.reshape(n_head, 2, o // n_head // 2, i)
            .swapaxes(1, 2).reshape(o, i))


def test_k_quant_mixed_with_legacy_or_float_stays_dense(tmp_path):
    torch.manual_seed(0)
    cfg = PRESETS["tiny"]
    src = LlamaForCausalLM(cfg)
    src.init_random(0)
    q, kv, inter = cfg.q_size, cfg.kv_size, cfg.intermediate_size
    sd = dict(src.named_parameters())
    types = {p: "Q4_K" for p in PARTS}
    types["attn_v"] = "Q4_0"           # K-quant next to a legacy part
    types["ffn_up"] = None             # K-quant next to a float part
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
            tensors[f"blk.{i}.{p}.weight"] = w.float() if types[p] is None \
                else gguf.quantize_ggml(w.float(), types[p])
        tensors[f"blk.{i}.attn_norm.weight"] = \
            sd[f"layers.{i}.input_norm_w"].data
        tensors[f"blk.{i}.ffn_norm.weight"] = \
            sd[f"layers.{i}.post_norm_w"].data
    path = str(tmp_path / "mixed.gguf")
    gguf.write_gguf(path, {"general.architecture": "llama"}, tensors)
    dense = LlamaForCausalLM(cfg)
    gguf.load_gguf_weights(dense, path)
    res = LlamaForCausalLM(cfg)
    gguf.load_gguf_weights(res, path, keep_quantized=True)
    for layer in res.layers:
        assert isinstance(layer.attn.qkv_proj, torch.nn.Linear)
        assert isinstance(layer.mlp.gate_up_proj, torch.nn.Linear)
        assert type(layer.attn.o_proj) is KQLinear
        assert type(layer.mlp.down_proj) is KQLinear
    assert not any(isinstance(m, WQLinear) for m in res.modules())
    ids = [5, 9, 2, 77, 31, 8]
    assert torch.equal(_logits(dense, ids), _logits(res, ids))


# -- model pass, engine, estimate -----------------------------------------

def test_model_pass():
    m = LlamaForCausalLM(PRESETS["tiny"])
    m.init_random(0)
    assert quantize_model_wq(m, "q4_k") == 4 * PRESETS["tiny"].num_layers
    assert isinstance(m.lm_head, torch.nn.Linear)
    for layer in m.layers:
        d = layer.mlp.down_proj
        assert isinstance(d, KQLinear) and d.fmts == ["q4_k"]
        assert (d.out_features, d.in_features) == (256, 512)
    # the bias is kept; a Linear whose K is no multiple of 256 stays dense
    m = LlamaForCausalLM(PRESETS["tiny-qwen"])
    m.init_random(0)
    bias = m.layers[0].attn.qkv_proj.bias.data.clone()
    assert quantize_model_wq(m, "q6_k") == 4 * PRESETS["tiny-qwen"].num_layers
    qkv = m.layers[0].attn.qkv_proj
    assert isinstance(qkv, KQLinear) and torch.equal(qkv.bias, bias)
    holder = torch.nn.Sequential(torch.nn.Linear(128, 32),
                                 torch.nn.Linear(256, 24),
                                 torch.nn.Linear(256, 32))
    assert quantize_model_wq(holder, "q4_k") == 1
    assert isinstance(holder[2], KQLinear)
    assert type(holder[0]) is type(holder[1]) is torch.nn.Linear
    with pytest.raises(ValueError):
        quantize_model_wq(holder, "q5_k")
    with pytest.raises(ValueError):
        KQLinear([("q4_k", ops.quantize_kq(torch.zeros(16, 256), "q4_k")),
                  ("q6_k", ops.quantize_kq(torch.zeros(16, 512), "q6_k"))])


def test_dtype_cast_keeps_planes():
    """model.to(dtype) converts every floating buffer; the fp16 super-block
    scales are fp16 by format and must come through bit for bit, like the
    integer planes."""
    m = LlamaForCausalLM(PRESETS["tiny-qwen"])
    m.init_random(0)
    quantize_model_wq(m, "q6_k")
    before = [p.clone() for p in m.layers[0].attn.qkv_proj.planes(0)]
    for cast in (lambda x: x.to(torch.bfloat16), lambda x: x.half(),
                 lambda x: x.float()):
        cast(m)
        qkv = m.layers[0].attn.qkv_proj
        for got, want in zip(qkv.planes(0), before):
            assert got.dtype == want.dtype and torch.equal(got, want)
    assert qkv.bias.dtype == torch.float32
    assert qkv.scratch is None            # CPU modules need none
    sd = m.state_dict()
    assert "layers.0.attn.qkv_proj.s0_ql" in sd
    assert sd["layers.0.attn.qkv_proj.s0_d"].dtype == torch.float16


def test_mixed_module_is_the_concatenated_weight():
    x, segs, bias, want = ko.build_mixed(17, True)
    mod = KQLinear(segs, bias)
    assert (mod.out_features, mod.in_features) == (64, ko.MIXED_K)
    assert mod.fmts == ["q4_k", "q4_k", "q6_k"] and mod.rows == [0, 16, 32]
    w = torch.cat([ops.dequantize_kq(p, f, torch.bfloat16) for f, p in segs])
    got = mod(x.view(1, 17, -1))
    assert tuple(got.shape) == (1, 17, 64)
    assert torch.equal(got[0], torch.nn.functional.linear(x, w, bias))
    ko.assert_wq_close(got[0], want, ko.TOL_KQ, "mixed module")


@pytest.mark.parametrize("fmt", ko.FMTS)
def test_engine_equals_dequantized_bf16_engine(fmt):
    """Exact: on the CPU a KQLinear computes F.linear on the dequantized
    weight, so the quantized engine and a bf16 engine carrying those
    weights generate the same tokens."""
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    prompts = [[1, 2, 3, 4, 5], [7, 8]]
    base = dict(model="tiny-gqa", max_model_len=512, max_num_seqs=8,
                kv_cache_blocks=256, eos_token_id=-1, seed=7)
    quant = LLMEngine(EngineConfig(**base, quantization=fmt), device="cpu")
    assert isinstance(quant.model.layers[0].attn.qkv_proj, KQLinear)
    ref = LLMEngine(EngineConfig(**base), device="cpu")
    for layer in ref.model.layers:
        for lin in (layer.attn.qkv_proj, layer.attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            lin.weight.data.copy_(ops.dequantize_kq(
                ops.quantize_kq(lin.weight.data, fmt), fmt))
    got = quant.generate(prompts, sp)
    assert got == ref.generate(prompts, sp)
    assert all(len(g) == 12 for g in got)
    # an engine handed a model that already holds KQLinears leaves it alone
    again = LLMEngine(EngineConfig(**base, quantization=fmt), device="cpu",
                      model=quant.model)
    assert again.model.layers[0].attn.qkv_proj is \
        quant.model.layers[0].attn.qkv_proj


def test_estimate():
    from helix_amd.runner.service import ModelSpec, estimate_model_bytes
    est = {q: estimate_model_bytes(ModelSpec("m", "llm", "llama3-8b",
                                             quantization=q))
           for q in (None, "fp8", "q8_0", "q4_0", "q4_k", "q6_k")}
    assert est["q4_k"] == est["q4_0"] < est["q6_k"] < est["fp8"] < est["q8_0"]
    cfg = PRESETS["llama3-8b"]
    elems = cfg.num_layers * (
        cfg.hidden_size * (cfg.q_size + 2 * cfg.kv_size)
        + cfg.q_size * cfg.hidden_size
        + 3 * cfg.hidden_size * cfg.intermediate_size)
    scratch = 2 * max(cfg.hidden_size * (cfg.q_size + 2 * cfg.kv_size),
                      2 * cfg.hidden_size * cfg.intermediate_size)
    assert est[None] - est["q4_k"] == 2 * elems - 144 * elems // 256 - scratch
    assert est[None] - est["q6_k"] == 2 * elems - 210 * elems // 256 - scratch


def test_export_gguf_quant_cli_single_types(tmp_path):
    for quant in ("q4_k", "q6_k"):
        out = str(tmp_path / f"tiny-{quant}.gguf")
        _export_cli(out, quant)
        g = gguf.GGUFFile(out)
        assert g.tensors["blk.0.ffn_down.weight"].type_name == quant.upper()
        assert g.tensors["token_embd.weight"].type_name == "F32"
        m = LlamaForCausalLM(PRESETS["tiny"])
        gguf.load_gguf_weights(m, out, keep_quantized=True)
        assert sum(isinstance(x, KQLinear) for x in m.modules()) \
            == 4 * PRESETS["tiny"].num_layers
