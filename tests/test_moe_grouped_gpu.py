"""Grouped MoE prefill kernels (ops/hip/moe_grouped.hip) on the GPU: the fp64
oracle at lists of one or two full row tiles plus a tail, exact fragment
mapping, row independence, the default-path cutoff, the engine, host guards.

Tolerance: mo.TOL_MOE (0.0242 = 4 x the rounding emulation's worst error
over mo.CASES, 0.00603) carries over: the kernels round where moe.hip does,
and mo.emulate over the 84 new cases at T = 129, 257, 300 has a worst error
of 0.00599 (E4k2-H2080-I32-T300-sparse). The weakest mutants on them are
drop_last_of_longest 0.112 = 4.6 x tol and drop_last_k_down 0.179."""
import dataclasses
import functools

import pytest
import torch

import helix_amd.ops as ops
import moe_oracle as mo
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models.llama import LlamaForCausalLM, get_preset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
CASES = [mo.Case(E, k, H, I, T, fam) for (E, k, H, I) in mo.SHAPES
         for T in (1, 17, 129, 257, 300) for fam in mo.FAMILIES]


@functools.lru_cache(maxsize=None)
def _gpu_weights(E, H, I):
    w13, w2 = mo.weights(E, H, I)
    return w13.to(DEV), w2.to(DEV)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_oracle_case(case):
    """fused="grouped" against the fp64 oracle, with NaN-filled act / ypair
    and NaN guard rows around out."""
    b = mo.build(case)
    E, k, H, I, T = case.E, case.k, case.H, case.I, case.T
    w13, w2 = _gpu_weights(E, H, I)
    ids, w = ops.moe_route(b.logits.to(DEV), k)
    big = torch.full((T + 2, H), NAN, dtype=torch.bfloat16, device=DEV)
    act = torch.full((T * k, I), NAN, dtype=torch.bfloat16, device=DEV)
    ypair = torch.full((T * k, H), NAN, dtype=torch.float32, device=DEV)
    out = ops.moe_experts(b.x.to(DEV), w13, w2, ids, w, fused="grouped",
                          out=big[1:T + 1], act=act, ypair=ypair)
    assert out.data_ptr() == big[1].data_ptr()
    assert torch.isnan(big[0]).all() and torch.isnan(big[T + 1]).all()
    assert torch.isfinite(act.float()).all()
    assert torch.isfinite(ypair).all()
    got = out.cpu()
    print(f"{case.id}: grouped {float(mo.wq_error(got, b.want).max()):.5f}, "
          f"tol {mo.TOL_MOE}")
    mo.assert_wq_close(got, b.want, mo.TOL_MOE, case.id + " grouped")


@pytest.mark.parametrize("E, H, I", [(4, 64, 160), (2, 160, 2080)])
def test_one_hot_exact(E, H, I):
    """The grouped down GEMM with topk_w = 1, k = 1 and one-hot activation
    rows returns w2[e] transposed, bit for bit, for every K position, channel
    and expert: fragment mapping, LDS layout, gather and scatter, on an
    asymmetric integer weight."""
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
    off, pairs = ops.moe_align(ids.to(DEV), E)
    ypair = torch.full((T, H), NAN, dtype=torch.float32, device=DEV)
    C.moe_grouped_down(ypair, act.to(DEV), w2.to(DEV),
                       torch.ones(T, 1, dtype=torch.float32, device=DEV),
                       off, pairs)
    assert torch.equal(ypair.cpu(), want)


@pytest.mark.parametrize("shape", [(8, 2, 256, 256), (4, 2, 2080, 32)],
                         ids=str)
def test_row_independence(shape):
    """One token row gives the same bits at T = 1 and in batches of 17, 130
    (its experts crowded and avoided) and 300 (crowded: its list spans three
    row tiles and it sits in the last), at either row-tile size."""
    E, k, H, I = shape
    w13, w2 = _gpu_weights(E, H, I)
    g = torch.Generator().manual_seed(17 + H)
    x0 = torch.randn(H, generator=g).to(torch.bfloat16)
    l0, _ = mo.make_logits(E, k, 1, "uniform", g)
    mine = mo.route_ref(l0, k)[0][0].tolist()

    def run(T, pos, how):
        x = torch.randn(T, H, generator=g).to(torch.bfloat16)
        lg, _ = mo.make_logits(E, k, T, "uniform", g)
        if how == "crowd":                       # everyone wants my experts
            lg = l0.expand(T, E).clone()
        elif how == "avoid":                     # nobody does
            lg[:, mine] = -30.0
        x[pos], lg[pos] = x0, l0[0]
        n_mine = int((mo.route_ref(lg, k)[0] == mine[0]).sum())
        out = ops.moe_forward(x.to(DEV), lg.to(DEV), w13, w2, k,
                              fused="grouped")
        assert torch.isfinite(out.float()).all()
        return out[pos].cpu(), n_mine

    base, _ = run(1, 0, "uniform")
    assert float(base.float().abs().max()) > 0
    seen = []
    for T, pos, how in ((17, 5, "uniform"), (130, 100, "crowd"),
                        (130, 100, "avoid"), (300, 290, "crowd")):
        got, n_mine = run(T, pos, how)
        seen.append(n_mine)
        assert torch.equal(got, base), (T, pos, how)
    assert max(seen) == 300 and min(seen) == 1    # both extremes were run


def test_default_path_follows_the_cutoff(monkeypatch):
    """fused=None: the grouped kernels from MOE_GROUPED_MIN_T tokens (no host
    sync), the library path just below (its one sync)."""
    assert ops.MOE_GROUPED_MIN_T >= 193
    E, k, H, I = 8, 2, 256, 256
    w13, w2 = _gpu_weights(E, H, I)
    synced = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist",
                        lambda t: synced.append(1) or real(t))
    for T in (ops.MOE_GROUPED_MIN_T, ops.MOE_GROUPED_MIN_T - 1):
        g = torch.Generator().manual_seed(T)
        x = torch.randn(T, H, generator=g).to(torch.bfloat16).to(DEV)
        logits = torch.randn(T, E, generator=g).to(torch.bfloat16).to(DEV)
        synced.clear()
        out = ops.moe_forward(x, logits, w13, w2, k)
        assert bool(synced) == (T < ops.MOE_GROUPED_MIN_T)
        ref = ops.moe_forward(x.cpu(), logits.cpu(), w13.cpu(), w2.cpu(), k)
        mo.assert_wq_close(out.cpu(), ref.double(), 2 * mo.TOL_MOE, f"T={T}")


def test_long_prompt_takes_grouped_prefill_and_fused_decode(monkeypatch):
    """A prompt of MOE_GROUPED_MIN_T + 7 tokens prefills without the library
    path's expert_off.tolist(), decodes with fused=True, and generates the
    tokens of the same model forced onto the library path. The model's rope
    table is sized to the prompt, whatever the cutoff is (tiny-moe's own
    holds 512 positions)."""
    n = ops.MOE_GROUPED_MIN_T + 7
    prompt = [[(3 * i) % 500 + 1 for i in range(n)]]
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    mcfg = dataclasses.replace(get_preset("tiny-moe"), max_position=n + 64)
    model = LlamaForCausalLM(mcfg, 1, 0).to(torch.bfloat16).to(DEV)
    model.init_random(7)

    def engine():
        return LLMEngine(EngineConfig(
            model="tiny-moe", max_model_len=n + 64, max_num_seqs=8,
            kv_cache_blocks=256, eos_token_id=-1, enforce_eager=True),
            device=DEV, model=model)

    calls, syncs, force = [], [], [None]
    real, real_tolist = ops.moe_experts, torch.Tensor.tolist

    def spy(x, w13, w2, ids, w, fused=None, **kw):
        calls.append((x.shape[0], fused))
        if fused is None:
            fused = force[0]
        return real(x, w13, w2, ids, w, fused=fused, **kw)

    monkeypatch.setattr(ops, "moe_experts", spy)
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


def test_host_guards():
    """Each rejected input raises before any launch: the NaN-filled outputs
    stay untouched. The good call with an empty offset table writes nothing."""
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
            ypair=torch.full((P, H), NAN, dtype=torch.float32, device=DEV))

    def gated(d, k=k):
        C.moe_grouped_gated(d["act"], d["x"], d["w13"], d["off"], d["pairs"],
                            k)

    def down(d):
        C.moe_grouped_down(d["ypair"], d["act"], d["w2"], d["tw"], d["off"],
                           d["pairs"])

    def misaligned(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        return buf[1:].view(t.shape)

    def untouched(d):
        torch.cuda.synchronize()
        for n in ("act", "ypair"):               # still all NaN
            assert bool(torch.isnan(d[n].float()).all()), n

    def bad(change, call=None, **shape):
        d = fresh(**shape)
        change(d)
        for fn in ([call] if call else [gated, down]):
            with pytest.raises(RuntimeError):
                fn(d)
        untouched(d)

    d = fresh()
    gated(d), down(d)
    untouched(d)

    bad(lambda d: d.update(x=d["x"].half()), gated)
    bad(lambda d: d.update(x=d["x"].cpu()), gated)
    bad(lambda d: d.update(x=torch.zeros(T, 2 * H, dtype=torch.bfloat16,
                                         device=DEV)[:, :H]), gated)
    bad(lambda d: d.update(x=misaligned(d["x"])), gated)
    bad(lambda d: d.update(w13=d["w13"].float()), gated)
    bad(lambda d: d.update(act=d["act"][:P - 1]), gated)
    bad(lambda d: d.update(act=torch.full((P, 2 * I), NAN, device=DEV,
                                          dtype=torch.bfloat16)), gated)
    bad(lambda d: d.update(w2=d["w2"].half()), down)
    bad(lambda d: d.update(tw=misaligned(d["tw"])), down)
    bad(lambda d: d.update(ypair=d["ypair"].bfloat16()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:, :32].contiguous()), down)
    bad(lambda d: d.update(ypair=d["ypair"][:P - 1]), down)
    bad(lambda d: d.update(tw=d["tw"].cpu()), down)
    bad(lambda d: d.update(off=d["off"][:E]))
    bad(lambda d: d.update(off=d["off"].long()))
    bad(lambda d: d.update(pairs=d["pairs"][:P - 1]))
    bad(lambda d: None, H=48)
    bad(lambda d: None, I=48)
    bad(lambda d: None, E=257)
    bad(lambda d: None, lambda d: gated(d, k=9), k=9, E=16)
    bad(lambda d: None, down, k=9, E=16)
