"""Routed expert GEMMs over Q4_0/Q8_0 experts (ops/hip/moe_wq.hip) and the
tiny-moe engine with quantised experts on the GPU: exact fragment mapping
of both kernels, every oracle case on both paths, the library path's
dequantiser, row independence, host guards, hipGraph serving, resident GGUF
serving."""
import functools

import pytest
import torch

import helix_amd.ops as ops
import moe_oracle as mo
import moe_wq_oracle as mq
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _gpu_planes(fmt, E, H, I):
    p13, p2 = mq.planes(fmt, E, H, I)
    return tuple(t.to(DEV) for t in p13), tuple(t.to(DEV) for t in p2)


def test_waves_cover_every_kernel():
    """The shapes take every K split the quantised kernels are built for
    (the bf16 kernels' own rule): 4 and 8 waves gated, 4, 8 and 16 down."""
    assert ops.MOE_WQ_FUSED_MAX_T >= 1
    assert {ops.moe_waves(I, H, True) for (_, _, H, I) in mq.SHAPES} == {4, 8}
    assert {ops.moe_waves(H, I, False) for (_, _, H, I) in mq.SHAPES} == \
        {4, 8, 16}


# -- exact fragment mapping -------------------------------------------------

def _integer_stack(fmt, E, rows, K, positive=False):
    """Planes with an asymmetric integer payload and per-block distinct
    power-of-two scales, and the bf16-exact weight they dequantise to.
    positive: every weight is >= 32 (see test_one_hot_gated_exact)."""
    e_, r_, k_ = torch.meshgrid(torch.arange(E), torch.arange(rows),
                                torch.arange(K), indexing="ij")
    pat = r_ * 7 + k_ * 3 + e_ * 11
    if fmt == "q4_0":
        q = pat % 7 + 1 if positive else pat % 16 - 8
        nib = (q + 8).to(torch.uint8).view(E, rows, K // 32, 32)
        qs = (nib[..., :16] | (nib[..., 16:] << 4)).reshape(E, rows, K // 2)
    else:
        q = pat % 127 + 1 if positive else pat % 255 - 127
        qs = q.to(torch.int8)
    b_ = torch.arange(K // 32)
    ex = (r_[:, :, 0:1] * 3 + b_[None, None, :] * 5 + e_[:, :, 0:1]) % 9
    d = 2.0 ** (ex.float() + (5 if positive else -4))
    w = (d[..., None] * q.view(E, rows, K // 32, 32).float()) \
        .reshape(E, rows, K)
    assert torch.equal(w.to(torch.bfloat16).float(), w)      # exact in bf16
    assert not torch.equal(w[0, :32, :32], w[0, :32, :32].t())
    assert not positive or float(w.min()) >= 32
    return qs.contiguous(), d.to(torch.float16).contiguous(), w


def _one_hot_tokens(E, K, seed):
    """T = E*K tokens, token t the one-hot row `pos` of expert `e`."""
    T = E * K
    order = torch.randperm(T, generator=torch.Generator().manual_seed(seed))
    ids = (order // K).to(torch.int32).view(T, 1)
    rows = torch.zeros(T, K, dtype=torch.bfloat16)
    rows[torch.arange(T), order % K] = 1.0
    return ids, rows, order // K, order % K


@pytest.mark.parametrize("fmt", mq.FMTS)
@pytest.mark.parametrize("E, H, I", [(4, 64, 160), (2, 32, 2080),
                                     (2, 32, 4128)])
def test_one_hot_down_exact(E, H, I, fmt):
    """The down GEMM with topk_w = 1, k = 1 and one-hot activation rows
    returns bf16(d * q) transposed, bit for bit, for every K position and
    every expert (4-, 8- and 16-wave kernels)."""
    C = ops._native()
    qs, d, w = _integer_stack(fmt, E, H, I)
    ids, act, ex, pos = _one_hot_tokens(E, I, E + I)
    T = E * I
    want = w[ex, :, pos]                                     # [T, H]
    off, pairs = ops.moe_align(ids.to(DEV), E)
    ypair = torch.full((T, H), NAN, dtype=torch.float32, device=DEV)
    C.moe_gemm_down_wq(ypair, act.to(DEV), qs.to(DEV), d.to(DEV),
                       ops.wq_bits(fmt),
                       torch.ones(T, 1, dtype=torch.float32, device=DEV),
                       off, pairs)
    assert torch.equal(ypair.cpu(), want)


@pytest.mark.parametrize("fmt", mq.FMTS)
@pytest.mark.parametrize("E, H, I", [(4, 160, 64), (2, 2080, 32)])
def test_one_hot_gated_exact(E, H, I, fmt):
    """The gated GEMM on one-hot x rows, one side at a time (4- and 8-wave
    kernels). Every driven weight is >= 32, where silu(g) = g exactly in
    fp32 whatever the exponential's last bit is (e^-32 < 2^-24), and the
    other side is the constant 1 resp. 64 (silu(64) = 64):
    gate driven: act = bf16(silu(g) * 1) = g; up driven: act = 64 * u."""
    C = ops._native()
    T = E * H
    ids, x, ex, pos = _one_hot_tokens(E, H, E + H)
    off, pairs = ops.moe_align(ids.to(DEV), E)
    qs, d, w = _integer_stack(fmt, E, I, H, positive=True)
    one = 0x99 if fmt == "q4_0" else 1                   # nibble 9 = q 1
    cq = torch.full_like(qs, one)
    for side in ("gate", "up"):
        cd = torch.full_like(d, 1.0 if side == "gate" else 64.0)
        halves = ((qs, d), (cq, cd)) if side == "gate" else ((cq, cd), (qs, d))
        w13_qs = torch.cat([halves[0][0], halves[1][0]], dim=1).contiguous()
        w13_d = torch.cat([halves[0][1], halves[1][1]], dim=1).contiguous()
        want = w[ex, :, pos] * (1.0 if side == "gate" else 64.0)   # [T, I]
        assert torch.equal(want.to(torch.bfloat16).float(), want)
        act = torch.full((T, I), NAN, dtype=torch.bfloat16, device=DEV)
        C.moe_gemm_gated_wq(act, x.to(DEV), w13_qs.to(DEV), w13_d.to(DEV),
                            ops.wq_bits(fmt), off, pairs, 1)
        assert torch.equal(act.cpu().float(), want), side


# -- oracle cases -----------------------------------------------------------

def _run(b, case, fused):
    """moe_experts_wq on the GPU with NaN-filled act / ypair and NaN guard
    rows around out. Returns out (on the CPU)."""
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    p13, p2 = _gpu_planes(case.fmt, E, H, I)
    ids, w = ops.moe_route(b.logits.to(DEV), k)
    big = torch.full((T + 2, H), NAN, dtype=torch.bfloat16, device=DEV)
    act = torch.full((T * k, I), NAN, dtype=torch.bfloat16, device=DEV)
    ypair = torch.full((T * k, H), NAN, dtype=torch.float32, device=DEV)
    out = ops.moe_experts_wq(b.x.to(DEV), p13, p2, case.fmt, ids, w,
                             fused=fused, out=big[1:T + 1], act=act,
                             ypair=ypair)
    assert out.data_ptr() == big[1].data_ptr()
    assert torch.isnan(big[0]).all() and torch.isnan(big[T + 1]).all()
    assert torch.isfinite(act.float()).all()
    assert torch.isfinite(ypair).all()
    return out.cpu()


@pytest.mark.parametrize("case", mq.CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    """Fused kernels and the library path against the fp64 oracle."""
    b = mq.build(case)
    got = _run(b, case, True)
    err = float(mq.wq_error(got, b.want).max())
    lib = _run(b, case, False)
    err_lib = float(mq.wq_error(lib, b.want).max())
    print(f"{case.id}: fused {err:.5f}, library {err_lib:.5f}, "
          f"tol {mq.TOL_MOE_WQ}")
    mq.assert_wq_close(got, b.want, mq.TOL_MOE_WQ, case.id + " fused")
    mq.assert_wq_close(lib, b.want, mq.TOL_MOE_WQ, case.id + " library")


@pytest.mark.parametrize("fmt", mq.FMTS)
def test_library_dequant_of_a_stack_slice_is_exact(fmt):
    """The library path's weight: dequant_wq of one expert's slice of the
    stack equals the CPU dequantisation (what the fused kernel's registers
    hold), bit for bit, also through a shared scratch."""
    E, H, I = 4, 32, 2080
    p13, p2 = _gpu_planes(fmt, E, H, I)
    w13, w2 = mq.dense_weights(fmt, E, H, I)
    scratch = torch.empty(2 * I * H + 64, dtype=torch.bfloat16, device=DEV)
    for e in range(E):
        got = ops.dequant_wq(p13[0][e], p13[1][e], fmt, out=scratch)
        assert got.data_ptr() == scratch.data_ptr()
        assert torch.equal(got.cpu(), w13[e])
        got = ops.dequant_wq(p2[0][e], p2[1][e], fmt, out=scratch)
        assert torch.equal(got.cpu(), w2[e])
        assert torch.equal(ops.dequant_wq(p2[0][e], p2[1][e], fmt).cpu(),
                           w2[e])


@pytest.mark.parametrize("fmt", mq.FMTS)
def test_default_path_follows_the_cutoff(monkeypatch, fmt):
    """fused=None: the fused kernels up to MOE_WQ_FUSED_MAX_T tokens, the
    library path above (told apart by the library path's host sync)."""
    E, k, H, I = 8, 2, 256, 256
    p13, p2 = _gpu_planes(fmt, E, H, I)
    c13, c2 = mq.planes(fmt, E, H, I)
    synced = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist",
                        lambda t: synced.append(1) or real(t))
    for T in (ops.MOE_WQ_FUSED_MAX_T, ops.MOE_WQ_FUSED_MAX_T + 1):
        g = torch.Generator().manual_seed(T)
        x = torch.randn(T, H, generator=g).to(torch.bfloat16).to(DEV)
        logits = torch.randn(T, E, generator=g).to(torch.bfloat16).to(DEV)
        synced.clear()
        out = ops.moe_forward_wq(x, logits, p13, p2, fmt, k)
        assert bool(synced) == (T > ops.MOE_WQ_FUSED_MAX_T)
        ref = ops.moe_forward_wq(x.cpu(), logits.cpu(), c13, c2, fmt, k)
        mq.assert_wq_close(out.cpu(), ref.double(), 2 * mq.TOL_MOE_WQ,
                           f"T={T}")


@pytest.mark.parametrize("fmt", mq.FMTS)
@pytest.mark.parametrize("shape", [(8, 2, 256, 256), (4, 2, 2080, 32),
                                   (4, 2, 32, 4128)], ids=str)
def test_row_independence(shape, fmt):
    """One token row (its x and its logits) gives the same bits whatever
    T is, wherever it sits, whoever its neighbours are (crowding its experts
    or avoiding them) and however many zero pad rows follow."""
    E, k, H, I = shape
    p13, p2 = _gpu_planes(fmt, E, H, I)
    g = torch.Generator().manual_seed(17 + H)
    x0 = torch.randn(H, generator=g).to(torch.bfloat16)
    l0, _ = mo.make_logits(E, k, 1, "uniform", g)
    mine = mo.route_ref(l0, k)[0][0].tolist()

    def neighbours(T, how):
        x = torch.randn(T, H, generator=g).to(torch.bfloat16)
        lg, perm = mo.make_logits(E, k, T, "uniform", g)
        if how == "crowd":                       # everyone wants my experts
            lg = l0.expand(T, E).clone()
        elif how == "avoid":                     # nobody does
            lg[:, mine] = -30.0
        return x, lg

    def run(T, pos, how, pad=0):
        x, lg = neighbours(T, how)
        x[pos], lg[pos] = x0, l0[0]
        if pad:
            x = torch.cat([x, torch.zeros(pad, H, dtype=x.dtype)])
            lg = torch.cat([lg, torch.zeros(pad, E, dtype=lg.dtype)])
        ids = mo.route_ref(lg, k)[0]
        n_mine = int((ids == mine[0]).sum())
        out = ops.moe_forward_wq(x.to(DEV), lg.to(DEV), p13, p2, fmt, k,
                                 fused=True)
        assert torch.isfinite(out.float()).all()
        return out[pos].cpu(), n_mine

    base, _ = run(1, 0, "uniform")
    assert float(base.float().abs().max()) > 0
    seen = []
    for T, pos, how, pad in ((17, 5, "uniform", 0), (64, 63, "crowd", 0),
                             (130, 100, "crowd", 0), (130, 100, "avoid", 0),
                             (64, 0, "avoid", 0), (3, 2, "uniform", 1),
                             (17, 16, "uniform", 15), (65, 64, "crowd", 63)):
        got, n_mine = run(T, pos, how, pad)
        seen.append(n_mine)
        assert torch.equal(got, base), (T, pos, how, pad)
    assert max(seen) >= 128 and min(seen) == 1    # both extremes were run


def test_host_guards():
    """Each rejected input raises before any launch: the NaN-filled outputs
    stay untouched."""
    C = ops._native()
    E, k, H, I, T = 8, 2, 64, 64, 5
    P = T * k

    def fresh(E=E, k=k, H=H, I=I, T=T, fmt="q4_0"):
        P = T * k
        bits = ops.wq_bits(fmt)
        qdt = torch.uint8 if bits == 4 else torch.int8
        div = 2 if bits == 4 else 1
        return dict(
            bits=bits,
            x=torch.zeros(T, H, dtype=torch.bfloat16, device=DEV),
            q13=torch.zeros(E, 2 * I, H // div, dtype=qdt, device=DEV),
            d13=torch.zeros(E, 2 * I, H // 32, dtype=torch.float16,
                            device=DEV),
            q2=torch.zeros(E, H, I // div, dtype=qdt, device=DEV),
            d2=torch.zeros(E, H, I // 32, dtype=torch.float16, device=DEV),
            tw=torch.ones(T, k, dtype=torch.float32, device=DEV),
            off=torch.zeros(E + 1, dtype=torch.int32, device=DEV),
            pairs=torch.zeros(P, dtype=torch.int32, device=DEV),
            act=torch.full((P, I), NAN, dtype=torch.bfloat16, device=DEV),
            ypair=torch.full((P, H), NAN, dtype=torch.float32, device=DEV))

    def gated(d, k=k):
        C.moe_gemm_gated_wq(d["act"], d["x"], d["q13"], d["d13"], d["bits"],
                            d["off"], d["pairs"], k)

    def down(d):
        C.moe_gemm_down_wq(d["ypair"], d["act"], d["q2"], d["d2"], d["bits"],
                           d["tw"], d["off"], d["pairs"])

    def misaligned(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        return buf[1:].view(t.shape)

    def strided(t):
        buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype,
                          device=DEV)
        return buf[..., :t.shape[-1]]

    def bad(change, call=None, **shape):
        d = fresh(**shape)
        change(d)
        for fn in ([call] if call else [gated, down]):
            with pytest.raises(RuntimeError):
                fn(d)
        torch.cuda.synchronize()
        for n in ("act", "ypair"):               # still all NaN
            assert bool(torch.isnan(d[n].float()).all()), n

    # the good calls run, both formats (an empty offset table: nothing is
    # written)
    for fmt in mq.FMTS:
        d = fresh(fmt=fmt)
        gated(d), down(d)
        torch.cuda.synchronize()
        assert bool(torch.isnan(d["ypair"]).all())

    has_two = torch.cuda.device_count() > 1
    for q, dd, call in (("q13", "d13", gated), ("q2", "d2", down)):
        # payload plane: dtype per bits, rank, alignment, layout, device
        bad(lambda d: d.update({q: d[q].view(torch.int8)}), call)
        bad(lambda d: d.update({q: d[q].view(torch.uint8)}), call, fmt="q8_0")
        bad(lambda d: d.update({q: d[q].to(torch.int32)}), call)
        bad(lambda d: d.update({q: d[q][0]}), call)
        bad(lambda d: d.update({q: misaligned(d[q])}), call)
        bad(lambda d: d.update({q: strided(d[q])}), call)
        bad(lambda d: d.update({q: d[q].cpu()}), call)
        # scale plane: fp16, [E, rows, K/32], alignment, layout, device
        bad(lambda d: d.update({dd: d[dd].float()}), call)
        bad(lambda d: d.update({dd: d[dd].bfloat16()}), call)
        bad(lambda d: d.update({dd: d[dd][:, :, :1].contiguous()}), call)
        bad(lambda d: d.update({dd: d[dd][:, :-1].contiguous()}), call)
        bad(lambda d: d.update({dd: d[dd][:-1].contiguous()}), call)
        bad(lambda d: d.update({dd: d[dd].reshape(-1, d[dd].shape[-1])}),
            call)
        bad(lambda d: d.update({dd: misaligned(d[dd])}), call)
        bad(lambda d: d.update({dd: strided(d[dd])}), call)
        bad(lambda d: d.update({dd: d[dd].cpu()}), call)
        if has_two:
            bad(lambda d: d.update({dd: d[dd].to("cuda:1")}), call)
            bad(lambda d: d.update({q: d[q].to("cuda:1"),
                                    dd: d[dd].to("cuda:1")}), call)
        # bits
        for bits in (0, 5, 16, -4):
            bad(lambda d: d.update(bits=bits), call)
        # a q4_0 payload read as q8_0 has half the K the scales say
        bad(lambda d: d.update(bits=8, **{q: d[q].view(torch.int8)}), call)
    # K % 32, N % 16
    bad(lambda d: None, H=40)                    # K of gated, N of down
    bad(lambda d: None, gated, H=48)
    bad(lambda d: None, gated, I=24)             # N of gated
    bad(lambda d: None, down, I=48)              # K of down
    bad(lambda d: None, down, H=40, fmt="q8_0")
    # x / act / ypair / topk_w
    bad(lambda d: d.update(x=d["x"].half()), gated)
    bad(lambda d: d.update(x=d["x"].cpu()), gated)
    bad(lambda d: d.update(x=strided(d["x"])), gated)
    bad(lambda d: d.update(x=misaligned(d["x"])), gated)
    bad(lambda d: d.update(x=d["x"][:, :32].contiguous()), gated)
    bad(lambda d: d.update(x=d["x"][:T - 1]), gated)
    bad(lambda d: d.update(act=d["act"][:P - 1]), gated)
    bad(lambda d: d.update(act=d["act"].float()), gated)
    bad(lambda d: d.update(ypair=d["ypair"].bfloat16()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:, :32].contiguous()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:P - 1]), down)
    bad(lambda d: d.update(act=d["act"][:P - 1]), down)
    bad(lambda d: d.update(tw=d["tw"].double()), down)
    bad(lambda d: d.update(tw=d["tw"][:, :1].contiguous()), down)
    # lists, E and k: as the bf16 entry points
    bad(lambda d: d.update(off=d["off"].long()))
    bad(lambda d: d.update(off=d["off"][:E]))
    bad(lambda d: d.update(pairs=d["pairs"][:P - 1]))
    bad(lambda d: d.update(pairs=d["pairs"].long()))
    bad(lambda d: None, E=257)
    bad(lambda d: None, lambda d: gated(d, k=9), k=9, E=16)
    bad(lambda d: None, down, k=9, E=16)
    bad(lambda d: None, E=1, k=2)
    bad(lambda d: None, lambda d: gated(d, k=0))
    # the op-level wrapper refuses what the library path cannot take
    d = fresh()
    with pytest.raises(ValueError):
        ops.moe_experts_wq(d["x"], (d["q13"], d["d13"]), (d["q2"], d["d2"]),
                           "q4_0",
                           torch.zeros(T, k, dtype=torch.int32, device=DEV),
                           d["tw"][:, :1], fused=False)
    with pytest.raises(ValueError):
        ops.moe_experts_wq(d["x"], (d["q13"], d["d13"]), (d["q2"], d["d2"]),
                           "q5_0",
                           torch.zeros(T, k, dtype=torch.int32, device=DEV),
                           d["tw"])


# -- engine -----------------------------------------------------------------

def _mk(enforce_eager: bool, seed=7, model=None, **kw):
    cfg = EngineConfig(model="tiny-moe", max_model_len=512, max_num_seqs=8,
                       kv_cache_blocks=256, eos_token_id=-1, seed=seed,
                       enforce_eager=enforce_eager, **kw)
    return LLMEngine(cfg, device=DEV, model=model)


def test_quantised_experts_graph_matches_eager_greedy():
    """q4_0 experts: batch 3 replays the bucket-4 graph and equals eager
    greedy token for token; the model owns one dequant scratch."""
    prompts = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11], [12] * 33]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    eager = _mk(True, expert_quantization="q4_0")
    mlps = [l.mlp for l in eager.model.layers]
    assert all(m.expert_fmt == ("q4_0", "q4_0") for m in mlps)
    assert all(m.w13_d.dtype == torch.float16 and m.w13_qs.is_cuda
               for m in mlps)
    assert mlps[0].scratch is not None
    assert all(m.scratch is mlps[0].scratch for m in mlps)
    cfg = eager.model_cfg
    assert mlps[0].scratch.numel() >= \
        2 * cfg.intermediate_size * cfg.hidden_size
    out_eager = eager.generate(prompts, sp)
    eng = _mk(False, expert_quantization="q4_0")
    assert eng.graph_runner is not None
    out_graph = eng.generate(prompts, sp)
    assert out_eager == out_graph
    assert all(len(o) == 24 for o in out_graph)
    # and the experts matter: bf16 experts decode something else
    assert out_graph != _mk(False).generate(prompts, sp)


def test_quantised_experts_continuous_batching():
    """Mixed prompt lengths joined mid-flight match one-by-one generation."""
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    prompts = {"a": [1, 2, 3], "b": [4, 5, 6, 7] * 9, "c": [8] * 17}
    eng = _mk(False, expert_quantization="q4_0")
    eng.add_request("a", prompts["a"], sp)
    eng.step()
    eng.add_request("b", prompts["b"], sp)
    eng.step()
    eng.add_request("c", prompts["c"], sp)
    while eng.has_work:
        eng.step()
    assert eng.num_free_blocks() == 256
    solo = _mk(False, expert_quantization="q4_0")
    for name, p in prompts.items():
        assert eng.seqs[name].output_ids == solo.generate([p], sp)[0], name


def test_resident_gguf_serves_what_expert_quantization_serves(tmp_path):
    """A q4_0 GGUF of the same source weights, loaded resident, serves the
    tokens of expert_quantization="q4_0" (attention left bf16 in both: the
    file's attention tensors are written dense)."""
    from helix_amd.engine.gguf import export_model_gguf, load_gguf_weights
    from helix_amd.models.llama import LlamaForCausalLM, PRESETS
    cfg = PRESETS["tiny-moe"]
    src = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(11)
    path = str(tmp_path / "moe-q4_0.gguf")
    export_model_gguf(src, path, quant="q4_0", experts_only=True)
    dst = LlamaForCausalLM(cfg).to(torch.bfloat16).init_random(12)
    load_gguf_weights(dst, path, keep_quantized=True)
    assert all(l.mlp.expert_fmt == ("q4_0", "q4_0") for l in dst.layers)
    prompts = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11]]
    sp = SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True)
    got = _mk(False, model=dst.to(DEV)).generate(prompts, sp)
    # quantised where the exporter quantises, on the CPU: ggml's Q4_0 scale
    # comes from an argmax over |w|, whose choice among equal bf16
    # magnitudes of opposite sign is not promised to agree across devices
    from helix_amd.models.quant import quantize_model_experts
    quantize_model_experts(src, "q4_0")
    want_eng = _mk(False, model=src.to(DEV), expert_quantization="q4_0")
    for a, b in zip(dst.layers, want_eng.model.layers):
        assert torch.equal(a.mlp.w13_qs, b.mlp.w13_qs)
        assert torch.equal(a.mlp.w2_d, b.mlp.w2_d)
    assert got == want_eng.generate(prompts, sp)
