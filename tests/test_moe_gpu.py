"""Mixture-of-experts HIP kernels (ops/hip/moe.hip) and the tiny-moe engine
on the GPU: exact routing and lists, exact fragment mapping, every oracle
case on both paths, row independence, host guards, hipGraph serving."""
import functools

import pytest
import torch

import helix_amd.ops as ops
import moe_oracle as mo
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _gpu_weights(E, H, I):
    w13, w2 = mo.weights(E, H, I)
    return w13.to(DEV), w2.to(DEV)


def test_constants_and_waves():
    """The kernel's limits are exported, and the cases take every K split
    the routed GEMM is built for: 4 and 8 waves gated, 4, 8 and 16 down."""
    C = ops._native()
    assert (C.MOE_MAX_EXPERTS, C.MOE_MAX_TOPK, C.MOE_CHUNK_PAIRS) == \
        (256, 8, 64)
    assert ops.MOE_FUSED_MAX_T >= 1
    assert {ops.moe_waves(I, H, True) for (_, _, H, I) in mo.SHAPES} == {4, 8}
    assert {ops.moe_waves(H, I, False) for (_, _, H, I) in mo.SHAPES} == \
        {4, 8, 16}
    # a property of the weight's shape: mixtral's own
    assert ops.moe_waves(14336, 4096, True) == 8
    assert ops.moe_waves(4096, 14336, False) == 16


@pytest.mark.parametrize("shape", mo.SHAPES, ids=str)
def test_route_exact(shape):
    """Ids equal the stable-sort reference exactly on every family (tied
    included), weights within 1e-5 relative, and moe_align's output equals
    the reference's exactly; bf16 and fp32 logits."""
    E, k, H, I = shape
    for T in mo.TS:
        for fam in mo.FAMILIES:
            b = mo.build(mo.Case(E, k, H, I, T, fam))
            _, w64 = mo.route_ref(b.logits, k)
            for lg in (b.logits, b.logits.float()):
                ids, w = ops.moe_route(lg.to(DEV), k)
                assert ids.dtype == torch.int32 and w.dtype == torch.float32
                assert torch.equal(ids.cpu().long(), b.ids), (T, fam)
                rel = ((w.cpu().double() - w64).abs() / w64).max()
                assert float(rel) <= 1e-5, (T, fam, float(rel))
            off, pairs = ops.moe_align(ids, E)
            roff, rpairs = ops.moe_align(ids.cpu(), E)
            assert torch.equal(off.cpu(), roff), (T, fam)
            assert torch.equal(pairs.cpu(), rpairs), (T, fam)


def test_align_large_and_bad_ids():
    """P = 8192 * 8 pairs over 256 experts, with ids outside [0, E) that
    belong to no list."""
    g = torch.Generator().manual_seed(11)
    E, T, k = 256, 8192, 8
    ids = torch.randint(0, E, (T, k), generator=g, dtype=torch.int32)
    bad = torch.randperm(T * k, generator=g)[:1000]
    ids.view(-1)[bad[:400]] = -1
    ids.view(-1)[bad[400:700]] = E
    ids.view(-1)[bad[700:]] = 1 << 30
    off, pairs = ops.moe_align(ids.to(DEV), E)
    roff, rpairs = ops.moe_align(ids, E)
    assert int(roff[E]) == T * k - 1000
    assert torch.equal(off.cpu(), roff)
    n = int(roff[E])
    assert torch.equal(pairs.cpu()[:n], rpairs[:n])


@pytest.mark.parametrize("E, H, I", [(4, 64, 160), (2, 32, 2080),
                                     (2, 32, 4128)])
def test_one_hot_exact(E, H, I):
    """The down GEMM with topk_w = 1, k = 1 and one-hot activation rows
    returns w2[e] transposed, bit for bit, for every K position and every
    expert: the fragment mapping and the K split, on an asymmetric integer
    weight (4-, 8- and 16-wave kernels)."""
    C = ops._native()
    e_, h_, i_ = torch.meshgrid(torch.arange(E), torch.arange(H),
                                torch.arange(I), indexing="ij")
    w2 = (((h_ * 7 + i_ * 3 + e_ * 11) % 251) - 125).to(torch.bfloat16)
    assert not torch.equal(w2[0, :32, :32], w2[0, :32, :32].t())
    T = E * I
    g = torch.Generator().manual_seed(E + I)
    order = torch.randperm(T, generator=g)       # token -> (expert, position)
    ids = (order // I).to(torch.int32).view(T, 1)
    act = torch.zeros(T, I, dtype=torch.bfloat16)
    act[torch.arange(T), order % I] = 1.0
    want = w2.float()[order // I, :, order % I]   # [T, H]
    ids_d = ids.to(DEV)
    off, pairs = ops.moe_align(ids_d, E)
    ypair = torch.full((T, H), NAN, dtype=torch.float32, device=DEV)
    C.moe_gemm_down(ypair, act.to(DEV), w2.to(DEV),
                    torch.ones(T, 1, dtype=torch.float32, device=DEV),
                    off, pairs)
    assert torch.equal(ypair.cpu(), want)


def _run(b, case, fused):
    """moe_forward on the GPU with NaN-filled act / ypair and NaN guard rows
    around out. Returns out (on the CPU)."""
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    w13, w2 = _gpu_weights(E, H, I)
    ids, w = ops.moe_route(b.logits.to(DEV), k)
    big = torch.full((T + 2, H), NAN, dtype=torch.bfloat16, device=DEV)
    act = torch.full((T * k, I), NAN, dtype=torch.bfloat16, device=DEV)
    ypair = torch.full((T * k, H), NAN, dtype=torch.float32, device=DEV)
    out = ops.moe_experts(b.x.to(DEV), w13, w2, ids, w, fused=fused,
                          out=big[1:T + 1], act=act, ypair=ypair)
    assert out.data_ptr() == big[1].data_ptr()
    assert torch.isnan(big[0]).all() and torch.isnan(big[T + 1]).all()
    assert torch.isfinite(act.float()).all()
    assert torch.isfinite(ypair).all()
    return out.cpu()


@pytest.mark.parametrize("case", mo.CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    """Fused kernels and the library path against the fp64 oracle."""
    b = mo.build(case)
    got = _run(b, case, True)
    err = float(mo.wq_error(got, b.want).max())
    lib = _run(b, case, False)
    err_lib = float(mo.wq_error(lib, b.want).max())
    print(f"{case.id}: fused {err:.5f}, library {err_lib:.5f}, "
          f"tol {mo.TOL_MOE}")
    mo.assert_wq_close(got, b.want, mo.TOL_MOE, case.id + " fused")
    mo.assert_wq_close(lib, b.want, mo.TOL_MOE, case.id + " library")


def test_default_path_follows_the_cutoff(monkeypatch):
    """fused=None: the fused kernels up to MOE_FUSED_MAX_T tokens, the
    library path above (told apart by the library path's host sync)."""
    E, k, H, I = 8, 2, 256, 256
    w13, w2 = _gpu_weights(E, H, I)
    synced = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist",
                        lambda t: synced.append(1) or real(t))
    for T in (ops.MOE_FUSED_MAX_T, ops.MOE_FUSED_MAX_T + 1):
        g = torch.Generator().manual_seed(T)
        x = torch.randn(T, H, generator=g).to(torch.bfloat16).to(DEV)
        logits = torch.randn(T, E, generator=g).to(torch.bfloat16).to(DEV)
        synced.clear()
        out = ops.moe_forward(x, logits, w13, w2, k)
        assert bool(synced) == (T > ops.MOE_FUSED_MAX_T)
        ref = ops.moe_forward(x.cpu(), logits.cpu(), w13.cpu(), w2.cpu(), k)
        mo.assert_wq_close(out.cpu(), ref.double(), 2 * mo.TOL_MOE, f"T={T}")


@pytest.mark.parametrize("shape", [(8, 2, 256, 256), (4, 2, 2080, 32),
                                   (4, 2, 32, 4128)], ids=str)
def test_row_independence(shape):
    """One token row (its x and its logits) gives the same bits whatever
    T is, wherever it sits, whoever its neighbours are (crowding its experts
    or avoiding them) and however many zero pad rows follow."""
    E, k, H, I = shape
    w13, w2 = _gpu_weights(E, H, I)
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
        out = ops.moe_forward(x.to(DEV), lg.to(DEV), w13, w2, k, fused=True)
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

    def fresh(E=E, k=k, H=H, I=I, T=T):
        P = T * k
        return dict(
            x=torch.zeros(T, H, dtype=torch.bfloat16, device=DEV),
            w13=torch.zeros(E, 2 * I, H, dtype=torch.bfloat16, device=DEV),
            w2=torch.zeros(E, H, I, dtype=torch.bfloat16, device=DEV),
            tw=torch.ones(T, k, dtype=torch.float32, device=DEV),
            off=torch.zeros(E + 1, dtype=torch.int32, device=DEV),
            pairs=torch.zeros(P, dtype=torch.int32, device=DEV),
            act=torch.full((P, I), NAN, dtype=torch.bfloat16, device=DEV),
            ypair=torch.full((P, H), NAN, dtype=torch.float32, device=DEV),
            out=torch.full((T, H), NAN, dtype=torch.bfloat16, device=DEV))

    def gated(d, k=k):
        C.moe_gemm_gated(d["act"], d["x"], d["w13"], d["off"], d["pairs"], k)

    def down(d):
        C.moe_gemm_down(d["ypair"], d["act"], d["w2"], d["tw"], d["off"],
                        d["pairs"])

    def combine(d, k=k):
        C.moe_combine(d["out"], d["ypair"], k)

    def misaligned(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        return buf[1:].view(t.shape)

    def bad(change, call=None, **shape):
        d = fresh(**shape)
        change(d)
        for fn in ([call] if call else [gated, down]):
            with pytest.raises(RuntimeError):
                fn(d)
        torch.cuda.synchronize()
        for n in ("act", "ypair", "out"):        # still all NaN
            assert bool(torch.isnan(d[n].float()).all()), n

    # the good call runs (an empty offset table: nothing is written)
    d = fresh()
    gated(d), down(d)
    d["ypair"].zero_()
    combine(d)
    assert float(d["out"].float().abs().max()) == 0.0

    bad(lambda d: d.update(x=d["x"].half()), gated)
    bad(lambda d: d.update(x=d["x"].cpu()), gated)
    bad(lambda d: d.update(x=torch.zeros(T, 2 * H, dtype=torch.bfloat16,
                                         device=DEV)[:, :H]), gated)
    bad(lambda d: d.update(x=misaligned(d["x"])), gated)
    bad(lambda d: d.update(x=d["x"][:, :32].contiguous()), gated)
    bad(lambda d: d.update(x=d["x"][:T - 1]), gated)
    bad(lambda d: d.update(w13=d["w13"].float()), gated)
    bad(lambda d: d.update(w13=d["w13"][0]), gated)
    bad(lambda d: d.update(act=d["act"][:P - 1]), gated)
    bad(lambda d: d.update(act=torch.full((P, 2 * I), NAN, device=DEV,
                                          dtype=torch.bfloat16)), gated)
    bad(lambda d: d.update(act=d["act"].float()), gated)
    bad(lambda d: d.update(w2=d["w2"].half()), down)
    bad(lambda d: d.update(ypair=d["ypair"].bfloat16()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:, :32].contiguous()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:P - 1]), down)
    bad(lambda d: d.update(act=d["act"][:P - 1]), down)
    bad(lambda d: d.update(tw=d["tw"].double()), down)
    bad(lambda d: d.update(tw=d["tw"][:, :1].contiguous()), down)
    # lists: dtype, length
    bad(lambda d: d.update(off=d["off"].long()))
    bad(lambda d: d.update(off=d["off"][:E]))
    bad(lambda d: d.update(pairs=d["pairs"][:P - 1]))
    bad(lambda d: d.update(pairs=d["pairs"].long()))
    # H, I no multiple of 32; E and k out of range
    bad(lambda d: None, H=48)
    bad(lambda d: None, I=48)
    bad(lambda d: None, E=257)
    bad(lambda d: None, lambda d: gated(d, k=9), k=9, E=16)
    bad(lambda d: None, down, k=9, E=16)
    bad(lambda d: None, E=1, k=2)
    bad(lambda d: None, lambda d: gated(d, k=0))
    # combine
    bad(lambda d: d.update(out=d["out"].float()), combine)
    bad(lambda d: d.update(out=d["out"][:T - 1]), combine)
    bad(lambda d: d.update(ypair=d["ypair"].double()), combine)
    bad(lambda d: None, lambda d: combine(d, k=3))
    # route and align
    lg = torch.zeros(T, E, dtype=torch.bfloat16, device=DEV)
    ids = torch.full((T, k), -7, dtype=torch.int32, device=DEV)
    w = torch.full((T, k), NAN, dtype=torch.float32, device=DEV)
    for args in ((ids, w, lg.half()), (ids, w, lg.cpu()),
                 (ids.long(), w, lg), (ids, w.double(), lg),
                 (ids[:, :1].contiguous(), w, lg), (ids[:T - 1], w[:T - 1], lg),
                 (torch.zeros(T, 9, dtype=torch.int32, device=DEV),
                  torch.zeros(T, 9, dtype=torch.float32, device=DEV), lg),
                 (ids, w, torch.zeros(T, 257, dtype=torch.bfloat16,
                                      device=DEV))):
        with pytest.raises(RuntimeError):
            C.moe_route(*args)
    off = torch.full((E + 1,), -7, dtype=torch.int32, device=DEV)
    pairs = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    for args in ((off, pairs, ids.long(), E), (off[:E], pairs, ids, E),
                 (off, pairs[:P - 1], ids, E), (off, pairs, ids, E + 1),
                 (off, pairs, ids.cpu(), E), (off, pairs, ids, 0)):
        with pytest.raises(RuntimeError):
            C.moe_align(*args)
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool(torch.isnan(w).all())
    assert bool((off == -7).all()) and bool((pairs == -7).all())
    # the op-level wrapper refuses what the library path cannot take
    d = fresh()
    with pytest.raises(ValueError):
        ops.moe_experts(d["x"], d["w13"], d["w2"],
                        torch.zeros(T, k, dtype=torch.int32, device=DEV),
                        d["tw"][:, :1], fused=False)


# -- engine ---------------------------------------------------------------

def _mk(enforce_eager: bool, seed=7):
    cfg = EngineConfig(model="tiny-moe", max_model_len=512, max_num_seqs=8,
                       kv_cache_blocks=256, eos_token_id=-1, seed=seed,
                       enforce_eager=enforce_eager)
    return LLMEngine(cfg, device=DEV)


def test_moe_graph_matches_eager_greedy():
    """Batch 3 replays the bucket-4 graph: the pad row is routed like any
    row and changes nothing."""
    prompts = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11], [12] * 33]
    sp = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    out_eager = _mk(True).generate(prompts, sp)
    eng = _mk(False)
    assert eng.graph_runner is not None
    out_graph = eng.generate(prompts, sp)
    assert out_eager == out_graph
    assert all(len(o) == 24 for o in out_graph)


def test_moe_continuous_batching_gpu():
    eng = _mk(False)
    sp = SamplingParams(temperature=0.0, max_tokens=12, ignore_eos=True)
    eng.add_request("a", [1, 2, 3], sp)
    eng.step()
    eng.add_request("b", [4, 5, 6, 7], sp)
    while eng.has_work:
        eng.step()
    assert len(eng.seqs["a"].output_ids) == 12
    assert len(eng.seqs["b"].output_ids) == 12
    assert eng.num_free_blocks() == 256


def test_moe_long_prompt_takes_library_prefill_and_fused_decode(monkeypatch):
    calls = []
    real = ops.moe_experts

    def spy(x, w13, w2, ids, w, fused=None, **kw):
        calls.append((x.shape[0], fused))
        return real(x, w13, w2, ids, w, fused=fused, **kw)

    monkeypatch.setattr(ops, "moe_experts", spy)
    syncs = []
    real_tolist = torch.Tensor.tolist
    n = ops.MOE_FUSED_MAX_T + 7
    assert n < 500
    eng = _mk(True)
    monkeypatch.setattr(
        torch.Tensor, "tolist",
        lambda t: (syncs.append(tuple(t.shape)) or real_tolist(t)))
    out = eng.generate([[(3 * i) % 500 + 1 for i in range(n)]],
                       SamplingParams(temperature=0.0, max_tokens=6,
                                      ignore_eos=True))[0]
    assert len(out) == 6
    layers = eng.model_cfg.num_layers
    assert calls[:layers] == [(n, None)] * layers          # prefill
    assert calls[layers:] == [(1, True)] * (5 * layers)    # decode
    # the library path's one sync per layer is expert_off.tolist()
    E = eng.model_cfg.num_experts
    assert syncs.count((E + 1,)) == layers
