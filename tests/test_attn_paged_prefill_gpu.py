"""attn_prefill_paged.hip: prefill attention read through the block table,
against the fp64 oracle and, bit for bit, against the gather (+ dequant) +
attn_prefill composition it replaces. Cases and paging:
tests/test_attn_paged_prefill_cpu.py.

TOL_PAGED_PREFILL is the project's tolerance rule (tests/attn_oracle.py):
4 x the worst error of attn_oracle.prefill_emulation over exactly these
cases, measured on the CPU:
  bf16 cache 0.00673 (paged-edges-d64-randn), fp8 cache 0.00558
  TOL_PAGED_PREFILL = 4 * 0.00673 = 0.0269
  smallest applicable prefill_mutants error on these inputs: 0.44
      (causal_plus_1, paged-long-d64), about 16 x the tolerance.
Re-derive the three numbers if a case changes.
"""
import pytest
import torch

import attn_oracle as ao
import helix_amd.ops as ops
from test_attn_paged_prefill_cpu import (PAGED_CASES, page_case, run_gathered,
                                         run_paged)

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL_PAGED_PREFILL = 0.0269

COMBOS = [pytest.param(c, kv8, bs,
                       id=f"{c.id}-{'fp8' if kv8 else 'bf16'}-bs{bs}")
          for c in PAGED_CASES for kv8 in (False, True) for bs in (8, 16, 128)]


@pytest.mark.parametrize("case,kv8,bs", COMBOS)
def test_matches_fp64(case, kv8, bs):
    p = page_case(case, kv8, bs)
    err = ao.assert_attn_close(run_paged(p, DEV), p.want, TOL_PAGED_PREFILL,
                               case.id)
    print(f"{case.id}: error {err:.5f} (tol {TOL_PAGED_PREFILL})")


@pytest.mark.parametrize("case,kv8,bs", COMBOS)
def test_bit_identical_to_gather(case, kv8, bs):
    p = page_case(case, kv8, bs)
    assert torch.equal(run_paged(p, DEV), run_gathered(p, DEV))


def _d96(a):
    a["q"] = a["q"].new_zeros(4, 8, 96)
    a["kc"] = a["vc"] = a["kc"].new_zeros(4, 2, 16, 96)


def _bs24(a):
    a["kc"] = a["vc"] = a["kc"].new_zeros(4, 2, 24, 128)


def _two_dtypes(a):
    a["vc"] = a["vc"].to(torch.uint8)


def _int64_tables(a):
    a["bt"] = a["bt"].long()


def _short_table(a):
    a["max_klen"] = 33


def _seq_lens_length(a):
    a["seq_lens"] = a["seq_lens"].new_zeros(2)


def _strided_cache(a):
    a["kc"] = a["kc"].new_zeros(4, 2, 16, 256)[..., :128]


@pytest.mark.parametrize("break_it", [
    _d96, _bs24, _two_dtypes, _int64_tables, _short_table, _seq_lens_length,
    _strided_cache], ids=lambda f: f.__name__.strip("_"))
def test_host_checks(break_it):
    """Every check runs before any launch: the call raises and `out` keeps
    its bits."""
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    a = dict(q=z(4, 8, 128), kc=z(4, 2, 16, 128), vc=z(4, 2, 16, 128),
             bt=z(1, 2, dt=torch.int32),
             cu=torch.tensor([0, 4], dtype=torch.int32, device=DEV),
             seq_lens=torch.tensor([20], dtype=torch.int32, device=DEV),
             max_klen=20)
    break_it(a)
    out = torch.full_like(a["q"], 7.0)
    with pytest.raises(RuntimeError):
        ops._native().attn_prefill_paged(
            out, a["q"], a["kc"], a["vc"], a["bt"], a["cu"], a["seq_lens"],
            4, a["max_klen"], 0.1, 0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
