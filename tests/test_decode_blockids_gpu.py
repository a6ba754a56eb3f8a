"""paged_attn_decode with its block ids staged in LDS, against the fp64
oracle of tests/attn_oracle.py: the cases of tests/decode_blockids_cases.py
(block sizes 8 to 256, windows that start the chunks off the block grid,
split-K, fp8, the full-grid kernel, the engine's calling convention), on
needle and on randn inputs. tests/test_decode_blockids_cpu.py shows that
each case fails a kernel that mixes up its staged ids.
"""
import pytest
import torch

import attn_oracle as ao
import decode_blockids_cases as dc
import helix_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _decode(b, **kw):
    return ops.paged_attn_decode(b.q.to(DEV), b.kc.to(DEV), b.vc.to(DEV),
                                 b.bt.to(DEV), b.lens.to(DEV), b.scale,
                                 window=b.window, **kw)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.id)
def test_decode_blockids(case):
    b = ao.build_decode(case)
    kw = {}
    if case.ws_len:     # a workspace that holds fewer partitions
        kw["workspace"] = ops.decode_workspace(
            b.q.shape[0], b.q.shape[1], b.q.shape[2], case.ws_len, DEV)
    got = _decode(b, **kw)
    err = ao.assert_attn_close(got, b.want, ao.TOL_DECODE, case.id)
    print(f"{case.id}: error {err:.5f} (tol {ao.TOL_DECODE})")


def test_decode_blockids_engine_convention():
    """A persistent workspace for 8 rows of 4096 tokens, filled with NaN
    and used for both calls; max_len rounded up to the buckets 512 and
    4096; block tables 4096 / 32 + 1 wide; block size 32."""
    first = ao.build_decode(dc.ENGINE_CASES[0])
    hq, d = first.q.shape[1], first.q.shape[2]
    ws = ops.decode_workspace(8, hq, d, 4096, DEV)
    for t in ws:
        t.fill_(float("nan"))
    for case in dc.ENGINE_CASES:
        b = ao.build_decode(case)
        assert b.bs == 32 and b.bt.shape[1] == 4096 // 32 + 1
        assert b.max_len == case.max_len
        got = _decode(b, workspace=ws, max_len=case.max_len)
        err = ao.assert_attn_close(got, b.want, ao.TOL_DECODE, case.id)
        print(f"{case.id}: error {err:.5f} (tol {ao.TOL_DECODE})")


@pytest.mark.parametrize("bs", [24, 4])
def test_decode_rejects_block_size(bs):
    """A block size that is no power of two, or below 8, is refused by
    the host's argument checks, which run before any launch."""
    B, hq, hkv, d = 2, 4, 2, 128
    q = torch.zeros(B, hq, d, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(8, hkv, bs, d, dtype=torch.bfloat16, device=DEV)
    bt = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    lens = torch.full((B,), 5, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="power of two and at least 8"):
        ops.paged_attn_decode(q, kc, kc.clone(), bt, lens, d ** -0.5,
                              max_len=5)
