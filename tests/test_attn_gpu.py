"""The two attention kernels against the fp64 oracle of tests/attn_oracle.py.

Every case runs on needle inputs (loud keys on the chunk, partition, tile,
window and causal edges; poison in every slot a row must not read;
shuffled, over-wide block tables) and, up to 2048 tokens, on plain randn
inputs. The metric is relative per (row, head); its tolerance comes from a
CPU emulation of the kernels' rounding, and tests/test_attn_oracle_cpu.py
shows for each case that a wrong kernel would fail it.
"""
import pytest

import attn_oracle as ao
import helix_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _decode(b, **kw):
    return ops.paged_attn_decode(b.q.to(DEV), b.kc.to(DEV), b.vc.to(DEV),
                                 b.bt.to(DEV), b.lens.to(DEV), b.scale,
                                 window=b.window, **kw)


@pytest.mark.parametrize("case", ao.DECODE_CASES, ids=lambda c: c.id)
def test_paged_attn_decode(case):
    """All 8 (D, G) pairs on bf16 (VPS=8) and fp8 caches, one of them at
    block size 32; the full-grid VPS=4 kernels (B * Hkv = 2048); split-K
    with dead, exactly full and capped (MAX_PARTS) partitions; sliding
    windows inside, on the edge of and beyond a partition."""
    b = ao.build_decode(case)
    got = _decode(b)
    err = ao.assert_attn_close(got, b.want, b.tol, case.id)
    print(f"{case.id}: error {err:.5f} (tol {b.tol})")


def test_paged_attn_decode_engine_convention():
    """As graph_runner and engine._run_decode call it: a persistent
    workspace for 8 rows of 4096 tokens sliced to the batch, three short
    rows, max_len rounded up to a bucket, block tables 4096 / 16 + 1
    wide. The workspace starts as NaN and is reused for the second call
    with the largest bucket: no dead partition may leak into the output."""
    first = ao.build_decode(ao.ENGINE_CASES[0])
    hq, d = first.q.shape[1], first.q.shape[2]
    ws = ops.decode_workspace(8, hq, d, 4096, DEV)
    for t in ws:
        t.fill_(float("nan"))
    for case in ao.ENGINE_CASES:
        b = ao.build_decode(case)
        assert b.bt.shape[1] == 4096 // 16 + 1 and b.max_len == case.max_len
        got = _decode(b, workspace=ws, max_len=case.max_len)
        err = ao.assert_attn_close(got, b.want, b.tol, case.id)
        print(f"{case.id}: error {err:.5f} (tol {b.tol})")


@pytest.mark.parametrize("case", ao.PREFILL_CASES, ids=lambda c: c.id)
def test_attn_prefill(case):
    """Non-causal (encoder) prefill at D=64 and D=128; causal tile edges
    with and without extra early-exit q-tiles; windows below, at and above
    KTILE; window and cached prefix together; cached-prefix edges; GQA at
    D=64."""
    b = ao.build_prefill(case)
    got = ops.attn_prefill(b.q.to(DEV), b.k.to(DEV), b.v.to(DEV),
                           b.cu_q.to(DEV), b.max_seqlen, b.scale,
                           causal=b.causal, window=b.window,
                           cu_seqlens_k=b.cu_k.to(DEV))
    err = ao.assert_attn_close(got, b.want, b.tol, case.id)
    print(f"{case.id}: error {err:.5f} (tol {b.tol})")
