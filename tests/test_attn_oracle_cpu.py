"""Proof, on the CPU, that the attention GPU tests can fail.

For every case of tests/test_attn_gpu.py (and the needle inputs of the
partition-cap test in tests/test_ops_gpu.py):
  * the fp64 oracle agrees with helix_amd/ops/reference.py to fp32
    accuracy (two independent implementations of the same attention);
  * a CPU emulation of the kernels' rounding passes assert_attn_close at
    the tolerance the GPU tests use;
  * every mutant that applies to the case (the reference with one
    deliberate error) fails it. In the plain-randn family only the
    all-zeros mutant is asked to fail: that an off-by-one among random
    tokens is invisible is why the needle family exists.
test_tolerances re-derives the two tolerance constants from these runs.
"""
import functools
import math

import pytest
import torch

import attn_oracle as ao
import helix_amd.ops as ops
import helix_amd.ops.reference as ref

DECODE = ao.DECODE_CASES + ao.ENGINE_CASES
PREFILL = ao.PREFILL_CASES

# Two fp32 evaluations of a softmax-weighted sum of up to 65 600 terms
# against fp64: a few hundred fp32 ulps (6e-8 each) at the very worst.
REF_AGREEMENT = 2e-5

DECODE_MUTANTS = {"zeros", "drop_last", "drop_first_in_window",
                  "include_kv_lo_minus_1", "read_past_len",
                  "drop_last_partition", "drop_phase_c_tail",
                  "ignore_block_table", "head_mod_hkv", "ignore_window"}
PREFILL_MUTANTS = {"zeros", "causal_plus_1", "causal_minus_1", "ignore_ctx",
                   "attend_past_klen", "ignore_window",
                   "include_kv_lo_minus_1", "drop_first_in_window",
                   "drop_last", "head_mod_hkv"}


def _fp32_reference(kind, b):
    if kind == "decode":
        kc, vc = (ops.kv_fp8_dequant(t) if t.dtype == torch.uint8 else t
                  for t in (b.kc, b.vc))
        return ref.paged_attn_decode(b.q.float(), kc.float(), vc.float(),
                                     b.bt, b.lens, b.scale, b.window)
    return ref.attn_prefill(b.q.float(), b.k.float(), b.v.float(), b.cu_q,
                            b.max_seqlen, b.scale, b.causal, b.window, b.cu_k)


@functools.lru_cache(maxsize=None)
def _result(kind, case):
    """(oracle-vs-reference error, emulation output error, {mutant: its
    error}) of one case; floats only, so every case stays cached."""
    if kind == "decode":
        b = ao.build_decode(case)
        emul, mutants = ao.decode_emulation(b), ao.decode_mutants(b)
    else:
        b = ao.build_prefill(case)
        emul, mutants = ao.prefill_emulation(b), ao.prefill_mutants(b)
    ao.assert_attn_close(emul, b.want, b.tol, f"{case.id} emulation")
    if case.family != "needle":
        mutants = {"zeros": mutants["zeros"]}
    errs = {}
    for name, got in mutants.items():
        with pytest.raises(AssertionError):
            ao.assert_attn_close(got, b.want, b.tol, f"{case.id} {name}")
        errs[name] = float(ao.attn_error(got, b.want).max())
    agree = float(ao.attn_error(_fp32_reference(kind, b), b.want).max())
    e = float(ao.attn_error(emul, b.want).max())
    print(f"{case.id}: oracle vs fp32 reference {agree:.2e}; emulation "
          f"{e:.5f} passes tol {b.tol}; rejected: " +
          ", ".join(f"{n} {v:.3f}" for n, v in sorted(errs.items())))
    return agree, e, errs


@pytest.mark.parametrize("case", DECODE, ids=lambda c: c.id)
def test_decode_case(case):
    agree, _, _ = _result("decode", case)
    assert agree <= REF_AGREEMENT


@pytest.mark.parametrize("case", PREFILL, ids=lambda c: c.id)
def test_prefill_case(case):
    agree, _, _ = _result("prefill", case)
    assert agree <= REF_AGREEMENT


def _applicable(kind, name):
    cases = DECODE if kind == "decode" else PREFILL
    return {c.name for c in cases if c.family == "needle"
            and name in _result(kind, c)[2]}


def test_mutants_apply_where_they_should():
    """A mutant that silently applied nowhere would prove nothing."""
    for name in DECODE_MUTANTS:
        assert _applicable("decode", name), name
    for name in PREFILL_MUTANTS:
        assert _applicable("prefill", name), name
    dec = {c.name: set(_result("decode", c)[2]) for c in DECODE
           if c.family == "needle"}
    # every case reads a block table, has a last token and a slot past it
    for name, got in dec.items():
        assert {"zeros", "read_past_len"} <= got, name
        if not name.startswith("window1-"):
            assert "drop_last" in got, name
    for name in ("splitk-129-700-g1", "splitk-2048-g8", "splitk-multiples",
                 "splitk-cap-65600", "engine"):
        assert {"drop_last_partition", "ignore_block_table",
                "drop_first_in_window"} <= dec[name], name
    for name in ("window256-700-bf16", "window300-700-fp8",
                 "window512-2048-bf16", "window256-100-700-fp8",
                 "window1-700-bf16"):
        assert {"ignore_window", "include_kv_lo_minus_1"} <= dec[name], name
    assert "ignore_window" not in dec["window700-700-bf16"]
    assert "ignore_window" not in dec["window4096-700-bf16"]
    for d, g in ao.DG_PAIRS:
        for name in (f"pairs-d{d}-g{g}-bf16", f"pairs-d{d}-g{g}-fp8",
                     f"fullgrid-d{d}-g{g}"):
            assert "drop_phase_c_tail" in dec[name], name
            assert ("head_mod_hkv" in dec[name]) == (g > 1), name
    pre = {c.name: set(_result("prefill", c)[2]) for c in PREFILL
           if c.family == "needle"}
    for name, got in pre.items():
        if name.startswith("noncausal"):
            assert {"attend_past_klen", "drop_last"} <= got, name
        else:
            assert {"causal_plus_1", "causal_minus_1"} <= got, name
        if "prefix" in name:
            assert "ignore_ctx" in got, name
        if name.startswith("window") and name != "window200":
            assert {"ignore_window", "include_kv_lo_minus_1"} <= got, name
    assert "ignore_window" not in pre["window200"]   # as long as the rows
    assert "head_mod_hkv" in pre["noncausal-8-2-64"]


def test_partition_cap_can_fail():
    """What tests/test_ops_gpu.py::test_paged_attn_decode_partition_cap
    checks is failed by an all-zeros output and by a lost partition."""
    errs = _result("decode", ao.PARTITION_CAP_CASE)[2]
    b = ao.build_decode(ao.PARTITION_CAP_CASE)
    assert (b.geom.part, b.geom.nparts) == (256, 257)
    for name in ("zeros", "drop_last_partition"):
        assert errs[name] > 4 * ao.TOL_DECODE, (name, errs[name])


def test_tolerances():
    """tol = 4 x the worst emulation error (within rounding of the
    constant), and at most 1/4 of the smallest mutant error."""
    for kind, cases, tol in (("decode", DECODE, ao.TOL_DECODE),
                             ("prefill", PREFILL, ao.TOL_PREFILL)):
        res = [_result(kind, c) for c in cases]
        worst = max(r[1] for r in res)
        smallest = min((v for r in res for v in r[2].values()),
                       default=math.inf)
        print(f"{kind}: worst emulation error {worst:.5f}, tol {tol}, "
              f"smallest mutant error {smallest:.4f}")
        assert 4 * worst <= tol * 1.02, (kind, worst)
        assert tol <= 4 * worst * 1.10, (kind, worst)
        assert tol <= smallest / 4, (kind, smallest)


def test_metric_reports_the_worst_pair():
    want = torch.randn(3, 4, 8, dtype=torch.float64)
    got = want.clone()
    assert ao.assert_attn_close(got, want, 1e-9) == 0.0
    got[2, 1, 5] += 1.0
    with pytest.raises(AssertionError, match=r"row 2, head 1 .*element 5"):
        ao.assert_attn_close(got, want, 1e-3)
    got = want.clone()
    got[0, 0, 0] = math.nan
    with pytest.raises(AssertionError, match="non-finite"):
        ao.assert_attn_close(got, want, 1e-3)
