"""Grouped MoE prefill kernels over Q4_0/Q8_0 experts
(ops/hip/moe_grouped_wq.hip) on the GPU: bit identity with the bf16 grouped
kernels on the dequantised stacks, the fp64 oracle, the default-path cutoff,
the engine, host guards.

Tolerance: mq.emulate over the 120 oracle cases below has a worst error of
0.01004 (q8_0-E4k2-H2080-I32-T300-skewed); 4 x that, 0.0402, is below
mq.TOL_MOE_WQ = 0.0428, so the constant is used. The kernels' worst measured
error over them is 0.01004, on that case."""
import dataclasses
import functools

import pytest
import torch

import helix_amd.ops as ops
import moe_wq_oracle as mq
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import LlamaForCausalLM, get_preset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
TOL = mq.TOL_MOE_WQ
SHAPES = ((8, 2, 256, 256), (8, 2, 160, 96), (64, 8, 256, 64),
          (4, 2, 2080, 32), (4, 2, 32, 2080))
assert set(SHAPES) <= set(mq.SHAPES)
FMT_PAIRS = (("q4_0", "q4_0"), ("q8_0", "q8_0"), ("q4_0", "q8_0"))


@functools.lru_cache(maxsize=None)
def _planes(fmt, which, E, H, I):
    return tuple(t.to(DEV) for t in mq.planes(fmt, E, H, I)[which == "w2"])


@functools.lru_cache(maxsize=None)
def _dense(fmt, which, E, H, I):
    """What the bf16 kernels are given: the reference dequantisation."""
    qs, d = mq.planes(fmt, E, H, I)[which == "w2"]
    return ops.dequantize_experts_wq(qs, d, fmt).to(DEV)


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _run(fn, x, w13, w2, ids, w, T, k, H, I, *fmt):
    """fn(fused="grouped") with NaN-filled act / ypair and NaN guard rows
    around out. Returns (act, ypair, out)."""
    big, act = _nan(T + 2, H), _nan(T * k, I)
    ypair = _nan(T * k, H, dtype=torch.float32)
    out = fn(x, w13, w2, *fmt, ids, w, fused="grouped", out=big[1:T + 1],
             act=act, ypair=ypair)
    assert out.data_ptr() == big[1].data_ptr()
    assert torch.isnan(big[0]).all() and torch.isnan(big[T + 1]).all()
    assert torch.isfinite(act.float()).all() and torch.isfinite(ypair).all()
    return act, ypair, out


@pytest.mark.parametrize("T", (1, 129, 300))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("fmt", FMT_PAIRS, ids="+".join)
def test_bit_identical_to_bf16_grouped(fmt, shape, T):
    """act, ypair and out equal, bit for bit, those of the bf16 grouped
    kernels on the dequantised stacks."""
    E, k, H, I = shape
    b = mq.build(mq.Case(fmt[0], E, k, H, I, T, "uniform"))
    x = b.x.to(DEV)
    ids, w = ops.moe_route(b.logits.to(DEV), k)
    got = _run(ops.moe_experts_wq, x, _planes(fmt[0], "w13", E, H, I),
               _planes(fmt[1], "w2", E, H, I), ids, w, T, k, H, I, fmt)
    want = _run(ops.moe_experts, x, _dense(fmt[0], "w13", E, H, I),
                _dense(fmt[1], "w2", E, H, I), ids, w, T, k, H, I)
    for name, a, c in zip(("act", "ypair", "out"), got, want):
        assert torch.equal(a, c), name


CASES = [mq.Case(f, E, k, H, I, T, fam) for f in mq.FMTS
         for (E, k, H, I) in SHAPES for T in (17, 129, 300)
         for fam in mq.FAMILIES]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    """fused="grouped" against the fp64 oracle on the exact weights."""
    b = mq.build(case)
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    ids, w = ops.moe_route(b.logits.to(DEV), k)
    out = _run(ops.moe_experts_wq, b.x.to(DEV),
               _planes(case.fmt, "w13", E, H, I),
               _planes(case.fmt, "w2", E, H, I), ids, w, T, k, H, I,
               case.fmt)[2].cpu()
    print(f"{case.id}: grouped {float(mq.wq_error(out, b.want).max()):.5f}, "
          f"tol {TOL}")
    mq.assert_wq_close(out, b.want, TOL, case.id + " grouped")


@pytest.mark.parametrize("fmt", mq.FMTS)
def test_default_path_follows_the_cutoff(monkeypatch, fmt):
    """fused=None: the grouped kernels from MOE_WQ_GROUPED_MIN_T tokens (no
    host sync), the library path just below (its one sync)."""
    assert ops.MOE_WQ_GROUPED_MIN_T >= 193
    E, k, H, I = 8, 2, 256, 256
    p13, p2 = _planes(fmt, "w13", E, H, I), _planes(fmt, "w2", E, H, I)
    c13, c2 = mq.planes(fmt, E, H, I)
    synced = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist",
                        lambda t: synced.append(1) or real(t))
    for T in (ops.MOE_WQ_GROUPED_MIN_T, ops.MOE_WQ_GROUPED_MIN_T - 1):
        g = torch.Generator().manual_seed(T)
        x = torch.randn(T, H, generator=g).to(torch.bfloat16).to(DEV)
        logits = torch.randn(T, E, generator=g).to(torch.bfloat16).to(DEV)
        synced.clear()
        out = ops.moe_forward_wq(x, logits, p13, p2, fmt, k)
        assert bool(synced) == (T < ops.MOE_WQ_GROUPED_MIN_T)
        ref = ops.moe_forward_wq(x.cpu(), logits.cpu(), c13, c2, fmt, k)
        mq.assert_wq_close(out.cpu(), ref.double(), 2 * mq.TOL_MOE_WQ,
                           f"T={T}")


def test_long_prompt_prefills_grouped(monkeypatch):
    """A prompt of MOE_WQ_GROUPED_MIN_T + 7 tokens on q4_0 experts prefills
    without the library path's expert_off.tolist(), decodes with fused=True,
    and generates the tokens of the same model forced onto the library
    path."""
    n = ops.MOE_WQ_GROUPED_MIN_T + 7
    prompt = [[(3 * i) % 500 + 1 for i in range(n)]]
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    mcfg = dataclasses.replace(get_preset("tiny-moe"), max_position=n + 64)
    model = LlamaForCausalLM(mcfg).to(torch.bfloat16).init_random(7).to(DEV)

    def engine():
        return LLMEngine(EngineConfig(
            model="tiny-moe", max_model_len=n + 64, max_num_seqs=8,
            kv_cache_blocks=256, eos_token_id=-1, enforce_eager=True,
            expert_quantization="q4_0"), device=DEV, model=model)

    calls, syncs, force = [], [], [None]
    real, real_tolist = ops.moe_experts_wq, torch.Tensor.tolist

    def spy(x, p13, p2, fmt, ids, w, fused=None, **kw):
        calls.append((x.shape[0], fused))
        if fused is None:
            fused = force[0]
        return real(x, p13, p2, fmt, ids, w, fused=fused, **kw)

    monkeypatch.setattr(ops, "moe_experts_wq", spy)
    eng, eng_lib = engine(), engine()
    monkeypatch.setattr(
        torch.Tensor, "tolist",
        lambda t: (syncs.append(tuple(t.shape)) or real_tolist(t)))
    out = eng.generate(prompt, sp)[0]
    layers, E = mcfg.num_layers, mcfg.num_experts
    assert len(out) == 6
    assert calls[:layers] == [(n, None)] * layers          # prefill
    assert calls[layers:] == [(1, True)] * (5 * layers)    # decode
    assert syncs.count((E + 1,)) == 0
    force[0] = False
    lib = eng_lib.generate(prompt, sp)[0]
    assert syncs.count((E + 1,)) == layers
    assert out == lib, [i for i in range(6) if out[i] != lib[i]]


def _fresh(E=8, k=2, H=256, I=256, T=5, bits=4, rows13=None, rows2=None):
    P, z = T * k, functools.partial(torch.zeros, device=DEV)
    rows13, rows2 = rows13 or 2 * I, rows2 or H
    qdt, per = (torch.uint8, 2) if bits == 4 else (torch.int8, 1)
    return dict(
        bits=bits, k=k, x=z(T, H, dtype=torch.bfloat16),
        q13=z(E, rows13, H // per, dtype=qdt),
        d13=z(E, rows13, H // 32, dtype=torch.float16),
        q2=z(E, rows2, I // per, dtype=qdt),
        d2=z(E, rows2, I // 32, dtype=torch.float16),
        tw=torch.ones(T, k, dtype=torch.float32, device=DEV),
        off=z(E + 1, dtype=torch.int32), pairs=z(P, dtype=torch.int32),
        act=_nan(P, rows13 // 2), ypair=_nan(P, rows2, dtype=torch.float32))


def _gated(d):
    ops._native().moe_grouped_gated_wq(d["act"], d["x"], d["q13"], d["d13"],
                                       d["bits"], d["off"], d["pairs"],
                                       d["k"])


def _down(d):
    ops._native().moe_grouped_down_wq(d["ypair"], d["act"], d["q2"], d["d2"],
                                      d["bits"], d["tw"], d["off"],
                                      d["pairs"])


def _misaligned(t):
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    return buf[1:].view(t.shape)


def _both(f, *names):
    return lambda d: d.update({n: f(d[n]) for n in names})


# (change, calls it must break, _fresh() arguments)
GUARDS = {
    "bits": (lambda d: d.update(bits=5), (_gated, _down), {}),
    "d_dtype": (_both(lambda t: t.float(), "d13", "d2"), (_gated, _down), {}),
    "qs_cpu": (_both(lambda t: t.cpu(), "q13", "q2"), (_gated, _down), {}),
    "qs_misaligned": (_both(_misaligned, "q13", "q2"), (_gated, _down),
                      dict(bits=8)),
    "K%32_gated": (lambda d: None, (_gated,), dict(H=48)),
    "K%32_down": (lambda d: None, (_down,), dict(I=48)),
    "rows%16_gated": (lambda d: None, (_gated,), dict(rows13=2 * 24)),
    "rows%16_down": (lambda d: None, (_down,), dict(rows2=40)),
    "E=257": (lambda d: None, (_gated, _down), dict(E=257)),
    "k=9": (lambda d: None, (_gated, _down), dict(k=9, E=16)),
    "short_off": (lambda d: d.update(off=d["off"][:8]), (_gated, _down), {}),
}


@pytest.mark.parametrize("name", GUARDS)
def test_host_guards(name):
    """A refused input raises before any launch: the NaN-filled outputs stay
    untouched."""
    change, fns, kw = GUARDS[name]
    d = _fresh(**kw)
    change(d)
    for fn in fns:
        with pytest.raises(RuntimeError):
            fn(d)
    torch.cuda.synchronize()
    assert torch.isnan(d["act"].float()).all()
    assert torch.isnan(d["ypair"]).all()


@pytest.mark.parametrize("bits", (4, 8))
def test_empty_lists_and_no_tokens(bits):
    """An all-zero offset table writes nothing, T = 0 returns, and a
    misspelt `fused` raises."""
    d = _fresh(bits=bits)
    _gated(d), _down(d)
    torch.cuda.synchronize()
    assert torch.isnan(d["act"].float()).all()
    assert torch.isnan(d["ypair"]).all()
    d0 = _fresh(bits=bits, T=0)
    _gated(d0), _down(d0)
    ids = torch.zeros(5, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.moe_experts_wq(d["x"], (d["q13"], d["d13"]), (d["q2"], d["d2"]),
                           "q4_0" if bits == 4 else "q8_0", ids, d["tw"],
                           fused="group")
