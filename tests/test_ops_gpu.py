"""GPU numerics tests: every CDNA4 HIP kernel vs the fp32 torch reference.

All marked `gpu`; run on an MI355X via gpurun. Tolerances are bf16-scale.
"""
import pytest
import torch

import attn_oracle as ao
import helix_amd.ops as ops
import helix_amd.ops.reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def assert_close_bf16(a, b, atol=2e-2, rtol=2e-2, msg=""):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol,
                               rtol=rtol, msg=msg)


def test_native_loaded():
    assert ops.have_native(), "HIP extension must be loaded on a GPU box"


def test_mfma_probe_layout():
    """Verify the assumed 16x16x32 bf16 MFMA fragment layouts with
    asymmetric random operands (guide §3)."""
    torch.manual_seed(0)
    a = torch.randn(16, 32, dtype=torch.bfloat16, device=DEV)
    b = torch.randn(32, 16, dtype=torch.bfloat16, device=DEV)
    d = ops.mfma_probe(a, b)
    want = a.float() @ b.float()
    assert_close_bf16(d, want, atol=5e-2, rtol=5e-2,
                      msg="MFMA fragment layout mismatch")


@pytest.mark.parametrize("H", [768, 4096, 8192])
def test_rms_norm(H):
    torch.manual_seed(0)
    x = torch.randn(33, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    got = ops.rms_norm(x, w, 1e-5)
    want = ref.rms_norm(x.cpu(), w.cpu(), 1e-5)
    assert_close_bf16(got, want)


def test_fused_add_rms_norm():
    torch.manual_seed(1)
    x = torch.randn(17, 4096, dtype=torch.bfloat16, device=DEV)
    r = torch.randn(17, 4096, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(4096, dtype=torch.bfloat16, device=DEV)
    want_out, want_res = ref.fused_add_rms_norm(x.cpu(), r.cpu(), w.cpu(), 1e-5)
    got_out, got_res = ops.fused_add_rms_norm(x, r, w, 1e-5)
    assert_close_bf16(got_res, want_res)
    assert_close_bf16(got_out, want_out)


def test_layer_norm():
    torch.manual_seed(2)
    x = torch.randn(9, 768, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(768, dtype=torch.bfloat16, device=DEV)
    b = torch.randn(768, dtype=torch.bfloat16, device=DEV)
    got = ops.layer_norm(x, w, b, 1e-5)
    want = ref.layer_norm(x.cpu(), w.cpu(), b.cpu(), 1e-5)
    assert_close_bf16(got, want)


@pytest.mark.parametrize("hq,hk,d", [(32, 8, 128), (12, 12, 64)])
def test_rope(hq, hk, d):
    torch.manual_seed(3)
    T = 21
    q = torch.randn(T, hq * d, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(T, hk * d, dtype=torch.bfloat16, device=DEV)
    pos = torch.randint(0, 500, (T,), dtype=torch.int64, device=DEV)
    cs = ref.make_cos_sin_cache(d, 512).to(DEV)
    want_q, want_k = ref.rotary_embedding(pos.cpu(), q.cpu(), k.cpu(),
                                          cs.cpu(), d)
    got_q, got_k = ops.rotary_embedding(pos, q, k, cs, d)
    assert_close_bf16(got_q, want_q)
    assert_close_bf16(got_k, want_k)


def test_silu_and_mul():
    torch.manual_seed(4)
    x = torch.randn(13, 2 * 14336, dtype=torch.bfloat16, device=DEV)
    got = ops.silu_and_mul(x)
    want = ref.silu_and_mul(x.cpu())
    assert_close_bf16(got, want)


def test_gelu_tanh():
    torch.manual_seed(5)
    x = torch.randn(13, 3072, dtype=torch.bfloat16, device=DEV)
    got = ops.gelu_tanh(x)
    want = ref.gelu_tanh(x.cpu())
    assert_close_bf16(got, want)


def test_reshape_and_cache():
    torch.manual_seed(6)
    T, Hkv, D, bs, nb = 10, 8, 128, 16, 4
    k = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(nb, Hkv, bs, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    slots = torch.tensor([0, 1, 17, 18, 19, 35, 36, 63, 5, 40],
                         dtype=torch.int64, device=DEV)
    kc_ref, vc_ref = kc.cpu().clone(), vc.cpu().clone()
    ref.reshape_and_cache(k.cpu(), v.cpu(), kc_ref, vc_ref, slots.cpu())
    ops.reshape_and_cache(k, v, kc, vc, slots)
    assert_close_bf16(kc, kc_ref, atol=0, rtol=0)
    assert_close_bf16(vc, vc_ref, atol=0, rtol=0)


@pytest.mark.parametrize("hq,hkv,d,lens", [
    (32, 8, 128, [1, 17, 128, 63]),
    (8, 8, 128, [200]),
    (12, 12, 64, [33, 64]),
    (32, 8, 128, [512, 300]),
])
def test_attn_prefill(hq, hkv, d, lens):
    torch.manual_seed(7)
    T = sum(lens)
    q = torch.randn(T, hq, d, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(T, hkv, d, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(T, hkv, d, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)),
                      dtype=torch.int32, device=DEV)
    scale = d ** -0.5
    got = ops.attn_prefill(q, k, v, cu, max(lens), scale)
    want = ref.attn_prefill(q.cpu(), k.cpu(), v.cpu(), cu.cpu(), max(lens),
                            scale)
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, ao.prefill_ref64(q, k, v, cu, scale),
                         ao.TOL_PREFILL)


@pytest.mark.parametrize("hq,hkv,d,lens", [
    (32, 8, 128, [1, 16, 100, 333]),
    (8, 8, 128, [257]),
    (64, 8, 128, [90, 1024]),
    (12, 12, 64, [50]),
    (32, 8, 128, [2048]),   # exercises split-K partitions
    # G=2; split-K into 6 partitions with a 60-token last one; the short
    # row leaves dead partitions
    (16, 8, 128, [129, 700]),
    (8, 2, 64, [129, 700]),     # G=4 at D=64
    (16, 2, 64, [300]),         # G=8 at D=64
])
def test_paged_attn_decode(hq, hkv, d, lens):
    torch.manual_seed(8)
    B = len(lens)
    bs = 16
    max_blocks = (max(lens) + bs - 1) // bs
    total_blocks = sum((l + bs - 1) // bs for l in lens) + 1
    q = torch.randn(B, hq, d, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(total_blocks, hkv, bs, d, dtype=torch.bfloat16,
                     device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.zeros(B, max_blocks, dtype=torch.int32, device=DEV)
    nxt = 1
    for b, l in enumerate(lens):
        n = (l + bs - 1) // bs
        bt[b, :n] = torch.arange(nxt, nxt + n, dtype=torch.int32)
        nxt += n
    seq_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = d ** -0.5
    got = ops.paged_attn_decode(q, kc, vc, bt, seq_lens, scale)
    want = ref.paged_attn_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(),
                                 seq_lens.cpu(), scale)
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, ao.decode_ref64(q, kc, vc, bt, seq_lens, scale),
                         ao.TOL_DECODE)


def _paged_case(lens, hq, hkv, d, bs=16):
    """Random q and bf16 paged caches with each row's blocks laid out
    back to back from block 1."""
    B = len(lens)
    nblk = [(l + bs - 1) // bs for l in lens]
    q = torch.randn(B, hq, d, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(sum(nblk) + 1, hkv, bs, d, dtype=torch.bfloat16,
                     device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.zeros(B, max(nblk), dtype=torch.int32)
    nxt = 1
    for b, n in enumerate(nblk):
        bt[b, :n] = torch.arange(nxt, nxt + n, dtype=torch.int32)
        nxt += n
    seq_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    return q, kc, vc, bt.to(DEV), seq_lens


def test_paged_attn_decode_full_grid():
    """The kernel the B=512 headline runs. B*Hkv = 2048 leaves nparts = 1,
    so the grid is 2048 workgroups and the host picks the VPS=4 variant
    (every smaller case in this file gets VPS=8). G=2. Lengths: a
    one-token row, an exactly full chunk, and second chunks of 1 and 44
    tokens (the chunk-2 K prefetch issues; the batch-of-4 V loop has a
    tail)."""
    torch.manual_seed(16)
    hq, hkv, d = 16, 8, 128
    lens = [[1, 127, 128, 129, 300][i % 5] for i in range(256)]
    q, kc, vc, bt, seq_lens = _paged_case(lens, hq, hkv, d)
    scale = d ** -0.5
    got = ops.paged_attn_decode(q, kc, vc, bt, seq_lens, scale)
    want = ref.paged_attn_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(),
                                 seq_lens.cpu(), scale)
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, ao.decode_ref64(q, kc, vc, bt, seq_lens, scale),
                         ao.TOL_DECODE)


def test_decode_partition_constant():
    """The Python workspace sizing and the kernel's split-K quantum are
    one number."""
    assert ops.DECODE_PARTITION == ops._native().DECODE_PART_QUANT


def test_paged_attn_decode_rejects_bad_args():
    """Host checks fire before any launch: a zero max_len (it used to
    divide by zero) and a workspace sized for a smaller batch."""
    torch.manual_seed(17)
    hq, hkv, d = 8, 8, 128
    q, kc, vc, bt, seq_lens = _paged_case([40, 40], hq, hkv, d)
    scale = d ** -0.5
    with pytest.raises(RuntimeError, match="max_len"):
        ops.paged_attn_decode(q, kc, vc, bt, seq_lens, scale, max_len=0)
    ws1 = ops.decode_workspace(1, hq, d, 40, DEV)
    with pytest.raises(RuntimeError, match="tmp_out"):
        ops.paged_attn_decode(q, kc, vc, bt, seq_lens, scale, workspace=ws1,
                              max_len=40)
    torch.cuda.synchronize()
    # the same arguments with a matching workspace are accepted
    ws2 = ops.decode_workspace(2, hq, d, 40, DEV)
    got = ops.paged_attn_decode(q, kc, vc, bt, seq_lens, scale,
                                workspace=ws2, max_len=40)
    want = ref.paged_attn_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(),
                                 seq_lens.cpu(), scale)
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, ao.decode_ref64(q, kc, vc, bt, seq_lens, scale),
                         ao.TOL_DECODE)


def test_paged_attn_decode_partition_cap():
    """One kv head at batch 1 with a 65 600-token context: split-K sizing
    asks for 1024 partitions and the workspace allows 513; the cap of 512
    (the reduce kernel's weight array) makes it 257 partitions of 256
    tokens. The inputs are the needle case of tests/attn_oracle.py: loud
    keys on the edges of the first, last and two middle partitions, so a
    lost partition or an all-zeros output fails the relative check
    (tests/test_attn_oracle_cpu.py::test_partition_cap_can_fail)."""
    b = ao.build_decode(ao.PARTITION_CAP_CASE)
    assert tuple(b.q.shape) == (1, 1, 128) and int(b.lens[0]) == 65600
    q, kc, vc, bt, seq_lens = (t.to(DEV) for t in
                               (b.q, b.kc, b.vc, b.bt, b.lens))
    got = ops.paged_attn_decode(q, kc, vc, bt, seq_lens, b.scale)
    want = ref.paged_attn_decode(b.q, b.kc, b.vc, b.bt, b.lens, b.scale)
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, b.want, ao.TOL_DECODE)


def test_sample_greedy():
    torch.manual_seed(9)
    logits = torch.randn(64, 32000, dtype=torch.bfloat16, device=DEV)
    temps = torch.zeros(64, dtype=torch.float32, device=DEV)
    seeds = torch.arange(64, dtype=torch.int64, device=DEV)
    got = ops.sample_tokens(logits, temps, seeds)
    want = logits.float().argmax(-1)
    assert torch.equal(got.cpu(), want.cpu())


def test_sample_gumbel_distribution():
    """Gumbel-max sampling should land near the softmax distribution."""
    torch.manual_seed(10)
    V = 8
    logits_row = torch.tensor([0.0, 1.0, 2.0, 0.5, -1.0, 0.0, 3.0, -2.0])
    N = 4096
    logits = logits_row.expand(N, V).contiguous().bfloat16().to(DEV)
    temps = torch.ones(N, dtype=torch.float32, device=DEV)
    seeds = torch.arange(N, dtype=torch.int64, device=DEV) * 7919
    got = ops.sample_tokens(logits, temps, seeds)
    counts = torch.bincount(got.cpu(), minlength=V).float() / N
    want = torch.softmax(logits_row, -1)
    assert (counts - want).abs().max() < 0.05, (counts, want)


@pytest.mark.parametrize("m,n,k", [(128, 128, 64), (200, 768, 768),
                                   (512, 3072, 768), (1000, 768, 3072)])
def test_gemm_bf16(m, n, k):
    torch.manual_seed(11)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) / (k ** 0.25)
    w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) / (k ** 0.25)
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    got = ops.gemm_bf16(x, w, bias)
    want = ref.gemm_bf16(x.cpu(), w.cpu(), bias.cpu())
    assert_close_bf16(got, want, atol=5e-2, rtol=5e-2)


def test_gemm_bf16_gelu():
    torch.manual_seed(12)
    x = torch.randn(100, 768, dtype=torch.bfloat16, device=DEV) / 5
    w = torch.randn(3072, 768, dtype=torch.bfloat16, device=DEV) / 5
    got = ops.gemm_bf16(x, w, None, act=1)
    want = ref.gemm_bf16(x.cpu(), w.cpu(), None, act=1)
    assert_close_bf16(got, want, atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("window,lens", [(64, [200]), (128, [100, 400])])
def test_attn_prefill_sliding_window(window, lens):
    torch.manual_seed(13)
    hq, hkv, d = 32, 8, 128
    T = sum(lens)
    q = torch.randn(T, hq, d, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(T, hkv, d, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(T, hkv, d, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)),
                      dtype=torch.int32, device=DEV)
    scale = d ** -0.5
    got = ops.attn_prefill(q, k, v, cu, max(lens), scale, window=window)
    want = ref.attn_prefill(q.cpu(), k.cpu(), v.cpu(), cu.cpu(), max(lens),
                            scale, window=window)
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, ao.prefill_ref64(q, k, v, cu, scale,
                                               window=window),
                         ao.TOL_PREFILL)


@pytest.mark.parametrize("window,lens", [(64, [200]), (256, [100, 700]),
                                         (512, [2048])])
def test_paged_attn_decode_sliding_window(window, lens):
    torch.manual_seed(14)
    hq, hkv, d, bs = 32, 8, 128, 16
    B = len(lens)
    max_blocks = (max(lens) + bs - 1) // bs
    total_blocks = sum((l + bs - 1) // bs for l in lens) + 1
    q = torch.randn(B, hq, d, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(total_blocks, hkv, bs, d, dtype=torch.bfloat16,
                     device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.zeros(B, max_blocks, dtype=torch.int32, device=DEV)
    nxt = 1
    for b, l in enumerate(lens):
        n = (l + bs - 1) // bs
        bt[b, :n] = torch.arange(nxt, nxt + n, dtype=torch.int32)
        nxt += n
    seq_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = d ** -0.5
    got = ops.paged_attn_decode(q, kc, vc, bt, seq_lens, scale,
                                window=window)
    want = ref.paged_attn_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(),
                                 seq_lens.cpu(), scale, window=window)
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, ao.decode_ref64(q, kc, vc, bt, seq_lens, scale,
                                              window=window),
                         ao.TOL_DECODE)


@pytest.mark.parametrize("qlens,klens", [([32], [160]), ([7, 64], [7, 200]),
                                         ([128], [128])])
def test_attn_prefill_cached_prefix(qlens, klens):
    """Query-offset prefill: q is the suffix, kv covers full context."""
    torch.manual_seed(15)
    hq, hkv, d = 32, 8, 128
    Tq, Tk = sum(qlens), sum(klens)
    q = torch.randn(Tq, hq, d, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(Tk, hkv, d, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(Tk, hkv, d, dtype=torch.bfloat16, device=DEV)
    cu_q = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0)),
                        dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0] + list(torch.tensor(klens).cumsum(0)),
                        dtype=torch.int32, device=DEV)
    scale = d ** -0.5
    got = ops.attn_prefill(q, k, v, cu_q, max(qlens), scale,
                           cu_seqlens_k=cu_k)
    want = ref.attn_prefill(q.cpu(), k.cpu(), v.cpu(), cu_q.cpu(),
                            max(qlens), scale, cu_seqlens_k=cu_k.cpu())
    assert_close_bf16(got, want, atol=3e-2, rtol=3e-2)
    ao.assert_attn_close(got, ao.prefill_ref64(q, k, v, cu_q, scale,
                                               cu_k=cu_k),
                         ao.TOL_PREFILL)


@pytest.mark.parametrize("want_kv,use_cache", [(True, True), (False, True),
                                               (True, False)])
def test_rope_qkv_cache_fused(want_kv, use_cache):
    """Fused strided-QKV rope+cache kernel vs the unfused composition."""
    torch.manual_seed(0)
    T, hq, hkv, d, bs = 33, 8, 2, 64, 16
    qkv = torch.randn(T, (hq + 2 * hkv) * d, dtype=torch.bfloat16,
                      device="cuda")
    pos = torch.randint(0, 100, (T,), dtype=torch.int64, device="cuda")
    cs = ref.make_cos_sin_cache(d, 128).cuda()
    nb = 8
    slots = torch.arange(bs, bs + T, dtype=torch.int64, device="cuda") \
        if use_cache else torch.full((T,), -1, dtype=torch.int64,
                                     device="cuda")
    kc = torch.zeros(nb, hkv, bs, d, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    cache = (kc, vc) if use_cache else None
    q, k, v = ops.rope_qkv_cache(pos, qkv, cs, hq, hkv, d,
                                 kv_cache=cache, slot_mapping=slots,
                                 want_kv=want_kv)
    # unfused reference path
    q_sz, kv_sz = hq * d, hkv * d
    q2, k2, v2 = qkv.split([q_sz, kv_sz, kv_sz], dim=-1)
    q2, k2 = q2.contiguous(), k2.contiguous()
    q2, k2 = ops.rotary_embedding(pos, q2.clone(), k2.clone(), cs, d)
    v2 = v2.contiguous()
    torch.testing.assert_close(q.reshape(T, -1), q2, atol=2e-2, rtol=2e-2)
    if want_kv:
        torch.testing.assert_close(k.reshape(T, -1), k2, atol=2e-2,
                                   rtol=2e-2)
        torch.testing.assert_close(v.reshape(T, -1), v2, atol=0, rtol=0)
    if use_cache:
        kc2 = torch.zeros_like(kc)
        vc2 = torch.zeros_like(vc)
        ops.reshape_and_cache(k2.view(T, hkv, d), v2.view(T, hkv, d),
                              kc2, vc2, slots)
        torch.testing.assert_close(kc, kc2, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(vc, vc2, atol=0, rtol=0)


def test_mfma_probe_fp8_layout():
    """16x16x128 MX-fp8 MFMA fragment layout vs torch e4m3 reference
    (asymmetric operands; unity e8m0 scales 0x7F = 2^0)."""
    torch.manual_seed(1)
    a = (torch.randn(16, 128) * 0.5).to(torch.float8_e4m3fn)
    b = (torch.randn(128, 16) * 0.5).to(torch.float8_e4m3fn)
    want = a.float() @ b.float()
    d = torch.zeros(16, 16, dtype=torch.float32, device="cuda")
    from helix_amd.ops import _native
    _native().mfma_probe_fp8(d, a.view(torch.uint8).cuda(),
                             b.view(torch.uint8).cuda(),
                             0x7F7F7F7F, 0x7F7F7F7F)
    torch.cuda.synchronize()
    torch.testing.assert_close(d.cpu(), want, atol=1e-2, rtol=1e-2)


def test_mfma_probe_fp8_scale_doubles():
    """e8m0 scale byte 0x80 (=2^1) on A must exactly double the result
    relative to 0x7F (=2^0) — validates the unity-scale trick the fp8
    GEMM epilogue-dequant design relies on."""
    torch.manual_seed(2)
    a = (torch.randn(16, 128) * 0.5).to(torch.float8_e4m3fn)
    b = (torch.randn(128, 16) * 0.5).to(torch.float8_e4m3fn)
    from helix_amd.ops import _native
    d1 = torch.zeros(16, 16, dtype=torch.float32, device="cuda")
    d2 = torch.zeros_like(d1)
    au, bu = a.view(torch.uint8).cuda(), b.view(torch.uint8).cuda()
    _native().mfma_probe_fp8(d1, au, bu, 0x7F7F7F7F, 0x7F7F7F7F)
    _native().mfma_probe_fp8(d2, au, bu, 0x80808080, 0x7F7F7F7F)
    torch.cuda.synchronize()
    torch.testing.assert_close(d2, d1 * 2.0)


def test_gemm_fp8_numerics():
    """fp8 GEMM with epilogue dequant vs fp32 reference of the quantized
    operands (exact modulo fp32 accumulation order)."""
    torch.manual_seed(0)
    M, N, K = 96, 200, 256
    x = torch.randn(M, K) * 2.0
    w = torch.randn(N, K) * 0.05
    x8, xs = ops.quantize_fp8(x)
    w8, ws = ops.quantize_fp8(w)
    want = ops.gemm_fp8(x8, w8, xs, ws)            # CPU reference path
    got = ops.gemm_fp8(x8.cuda(), w8.cuda(), xs.cuda(), ws.cuda()).cpu()
    torch.testing.assert_close(got.float(), want.float(), atol=0.05,
                               rtol=0.05)
    # and it approximates the bf16 matmul (quantization error bounded)
    ref = (x @ w.t()).float()
    rel = (got.float() - ref).norm() / ref.norm()
    assert rel < 0.05, f"fp8 rel error {rel}"


def test_gemm_fp8_bias_gelu():
    torch.manual_seed(1)
    M, N, K = 64, 64, 128
    x = torch.randn(M, K)
    w = torch.randn(N, K) * 0.1
    bias = torch.randn(N).bfloat16()
    x8, xs = ops.quantize_fp8(x)
    w8, ws = ops.quantize_fp8(w)
    want = ops.gemm_fp8(x8, w8, xs, ws, bias=bias, act=1)
    got = ops.gemm_fp8(x8.cuda(), w8.cuda(), xs.cuda(), ws.cuda(),
                       bias=bias.cuda(), act=1).cpu()
    torch.testing.assert_close(got.float(), want.float(), atol=0.08,
                               rtol=0.08)


@pytest.mark.parametrize("d,lens,window", [
    (128, [77] * 4, 0),         # one partial chunk
    (128, [129, 1100], 0),      # next-chunk K prefetch; split-K, 9 parts
    (64, [129, 700], 0),        # D=64
    (128, [700], 256),          # sliding window over split-K
])
def test_fp8_kv_decode_gpu(d, lens, window):
    """Decode kernel over an fp8 (e4m3) cache matches the dequantized
    reference, and the HW cvt encodings match torch float8_e4m3fn."""
    torch.manual_seed(0)
    B, hq, hkv, bs, L = len(lens), 8, 2, 16, max(lens)
    nb = (L + bs - 1) // bs
    k = torch.randn(L, hkv, d, dtype=torch.bfloat16, device="cuda")
    v = torch.randn(L, hkv, d, dtype=torch.bfloat16, device="cuda")
    q = torch.randn(B, hq, d, dtype=torch.bfloat16, device="cuda")
    kc = torch.zeros(B * nb + 1, hkv, bs, d, dtype=torch.uint8,
                     device="cuda")
    vc = torch.zeros_like(kc)
    bt = (torch.arange(B * nb, dtype=torch.int32, device="cuda")
          .reshape(B, nb) + 1)
    lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for b in range(B):
        n = int(lens[b])
        slots = (torch.arange(n, dtype=torch.int64, device="cuda")
                 + (1 + b * nb) * bs)
        ops.reshape_and_cache(ops.kv_fp8_quant(k[:n]),
                              ops.kv_fp8_quant(v[:n]), kc, vc, slots)
    scale = d ** -0.5
    out = ops.paged_attn_decode(q, kc, vc, bt, lens, scale, window=window)
    # fp32 torch reference on the dequantized cache (CPU)
    want = ops.paged_attn_decode(q.cpu(), ops.kv_fp8_dequant(kc).cpu(),
                                 ops.kv_fp8_dequant(vc).cpu(), bt.cpu(),
                                 lens.cpu(), scale, window=window)
    torch.testing.assert_close(out.cpu().float(), want.float(), atol=3e-2,
                               rtol=3e-2)
    ao.assert_attn_close(out, ao.decode_ref64(q, kc, vc, bt, lens, scale,
                                              window=window),
                         ao.TOL_DECODE)


def test_fp8_kv_fused_rope_write_gpu():
    """rope_qkv_cache writing an fp8 cache matches quantizing the bf16
    path's cache (HW v_cvt_fp8 == torch e4m3fn encodings)."""
    torch.manual_seed(1)
    T, hq, hkv, d, bs = 21, 8, 2, 64, 16
    qkv = torch.randn(T, (hq + 2 * hkv) * d, dtype=torch.bfloat16,
                      device="cuda")
    pos = torch.randint(0, 60, (T,), dtype=torch.int64, device="cuda")
    cs = ref.make_cos_sin_cache(d, 128).cuda()
    slots = torch.arange(bs, bs + T, dtype=torch.int64, device="cuda")
    kc16 = torch.zeros(8, hkv, bs, d, dtype=torch.bfloat16, device="cuda")
    vc16 = torch.zeros_like(kc16)
    ops.rope_qkv_cache(pos, qkv, cs, hq, hkv, d, kv_cache=(kc16, vc16),
                       slot_mapping=slots)
    kc8 = torch.zeros(8, hkv, bs, d, dtype=torch.uint8, device="cuda")
    vc8 = torch.zeros_like(kc8)
    ops.rope_qkv_cache(pos, qkv, cs, hq, hkv, d, kv_cache=(kc8, vc8),
                       slot_mapping=slots)
    # quantization of the bf16-cache contents must match the direct
    # fp8 write within one quantization step: the HW cvt_pk_fp8_f32
    # rounding can differ from torch's cast by 1 ulp on ties
    torch.testing.assert_close(ops.kv_fp8_dequant(vc8).float(),
                               ops.kv_fp8_dequant(
                                   ops.kv_fp8_quant(vc16)).float(),
                               atol=0.06, rtol=0.07)
    # K goes f32->fp8 directly in the fused kernel but f32->bf16->fp8
    # via the bf16 cache: double rounding may move ~0.1% of elements by
    # one e4m3 ulp (rel 0.125). Assert exactly that: almost all equal,
    # none off by more than one quantization step.
    ka = ops.kv_fp8_dequant(kc8).float()
    kb = ops.kv_fp8_dequant(ops.kv_fp8_quant(kc16)).float()
    exact = (ka == kb).float().mean().item()
    assert exact > 0.99, f"only {exact:.3f} exact"
    # one e4m3 ulp is ~2^-3 of the magnitude (plus a small absolute
    # floor for the denormal range)
    bound = 0.135 * torch.maximum(ka.abs(), kb.abs()) + 0.02
    bad = ((ka - kb).abs() > bound).sum().item()
    assert bad == 0, f"{bad} K elements off by more than one e4m3 ulp"


@pytest.mark.parametrize("m,n,k", [
    (1, 128, 64),                 # tiny decode batch, BM=64 path
    (64, 4096, 4096),             # o_proj shape, small batch
    (512, 4096, 4096),            # o_proj @ B=512 (split-K path)
    (512, 6144, 4096),            # qkv_proj
    (512, 4096, 14336),           # down_proj (deep split-K)
    (200, 1024, 512),             # odd M tail
])
def test_gemm_skinny_bf16(m, n, k):
    torch.manual_seed(21)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) / (k ** 0.25)
    w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) / (k ** 0.25)
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    got = ops.gemm_skinny_bf16(x, w, bias)
    want = ref.gemm_bf16(x.cpu(), w.cpu(), bias.cpu())
    assert_close_bf16(got, want, atol=5e-2, rtol=5e-2)
    # no-bias path
    got2 = ops.gemm_skinny_bf16(x, w, None)
    want2 = ref.gemm_bf16(x.cpu(), w.cpu(), None)
    assert_close_bf16(got2, want2, atol=5e-2, rtol=5e-2)


def test_linear_dispatch_matches_torch():
    """ops.linear (the HLinear route) must agree with F.linear on the
    decode shapes it owns."""
    torch.manual_seed(22)
    for m, n, k in [(17, 512, 256), (512, 1024, 512)]:
        x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) / (k ** .25)
        w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) / (k ** .25)
        got = ops.linear(x, w, None)
        want = torch.nn.functional.linear(x.cpu().float(), w.cpu().float())
        assert_close_bf16(got, want.to(torch.bfloat16), atol=5e-2, rtol=5e-2)


def _ext_sample(logits, temps, seeds, top_p=None, top_k=None,
                rep=None, pres=None, freq=None, counts=None, seen=None,
                row_map=None):
    B = logits.shape[0]
    dev = logits.device
    f = lambda v, d: torch.full((B,), v, dtype=d, device=dev)  # noqa: E731
    return ops.sample_tokens_ext(
        logits, temps, seeds,
        top_p if top_p is not None else f(1.0, torch.float32),
        top_k if top_k is not None else f(0, torch.int32),
        rep if rep is not None else f(1.0, torch.float32),
        pres if pres is not None else f(0.0, torch.float32),
        freq if freq is not None else f(0.0, torch.float32),
        counts, seen, row_map)


def test_sample_ext_topp_support():
    """Every sampled token must lie in the exact torch top-p set (plus
    at most the histogram boundary bin, 16/2048 logit units wide)."""
    torch.manual_seed(31)
    V, N, p = 8192, 512, 0.9
    row = torch.randn(V) * 3
    logits = row.expand(N, V).contiguous().bfloat16().cuda()
    temps = torch.full((N,), 0.8, device="cuda")
    seeds = (torch.arange(N, dtype=torch.int64, device="cuda") * 7919 + 3)
    top_p = torch.full((N,), p, device="cuda")
    toks = _ext_sample(logits, temps, seeds, top_p=top_p).cpu()

    srt, idx = torch.sort(row.bfloat16().float(), descending=True)
    probs = torch.softmax(srt, -1)
    cum = probs.cumsum(-1)
    keep_n = int((cum - probs < p).sum())      # exact "first past p" set
    # boundary-bin slack: tokens whose logit >= kept_min - bin_width
    bin_w = 16.0 / 2048
    thresh = srt[keep_n - 1] - bin_w
    allowed = set(idx[(srt >= thresh)].tolist())
    exact = set(idx[:keep_n].tolist())
    in_exact = sum(int(t) in exact for t in toks.tolist())
    assert all(int(t) in allowed for t in toks.tolist())
    assert in_exact >= 0.98 * N, f"only {in_exact}/{N} inside exact set"


def test_sample_ext_topk_support():
    torch.manual_seed(32)
    V, N, k = 8192, 512, 40
    row = torch.randn(V) * 3
    logits = row.expand(N, V).contiguous().bfloat16().cuda()
    temps = torch.full((N,), 1.0, device="cuda")
    seeds = (torch.arange(N, dtype=torch.int64, device="cuda") * 104729 + 7)
    top_k = torch.full((N,), k, dtype=torch.int32, device="cuda")
    toks = _ext_sample(logits, temps, seeds, top_k=top_k).cpu()
    srt, idx = torch.sort(row.bfloat16().float(), descending=True)
    bin_w = 16.0 / 2048
    allowed = set(idx[(srt >= srt[k - 1] - bin_w)].tolist())
    exact = set(idx[:k].tolist())
    assert all(int(t) in allowed for t in toks.tolist())
    assert sum(int(t) in exact for t in toks.tolist()) >= 0.98 * N


def test_sample_ext_penalties_greedy_exact():
    """Greedy + penalties is deterministic: the kernel's adjusted argmax
    must equal the host reference (engine._process_logits semantics)."""
    torch.manual_seed(33)
    B, V = 16, 4096
    logits = (torch.randn(B, V) * 2).bfloat16()
    counts = torch.zeros(B, V, dtype=torch.int32)
    seen = torch.zeros(B, V, dtype=torch.uint8)
    g = torch.Generator().manual_seed(5)
    for b in range(B):
        pid = torch.randint(0, V, (50,), generator=g)
        oid = torch.randint(0, V, (30,), generator=g)
        seen[b][pid] = 1
        counts[b].index_put_((oid,), torch.ones(30, dtype=torch.int32),
                             accumulate=True)
    rep, pres, freq = 1.3, 0.5, 0.2
    # host reference
    want = []
    for b in range(B):
        rowv = logits[b].float().clone()
        seen_any = (seen[b] > 0) | (counts[b] > 0)
        vals = rowv[seen_any]
        rowv[seen_any] = torch.where(vals > 0, vals / rep, vals * rep)
        rowv[seen_any] -= pres
        rowv -= freq * counts[b].float()
        want.append(int(rowv.argmax()))
    dev = "cuda"
    B_t = lambda v, d: torch.full((B,), v, dtype=d, device=dev)  # noqa
    toks = ops.sample_tokens_ext(
        logits.cuda(), B_t(0.0, torch.float32),
        torch.arange(B, dtype=torch.int64, device=dev),
        B_t(1.0, torch.float32), B_t(0, torch.int32),
        B_t(rep, torch.float32), B_t(pres, torch.float32),
        B_t(freq, torch.float32),
        counts.cuda(), seen.cuda(),
        torch.arange(B, dtype=torch.int32, device=dev))
    assert toks.cpu().tolist() == want


def test_engine_gpu_topp_penalties_e2e():
    """End-to-end: engine decodes with top-p + penalties on the GPU fast
    path; output must avoid immediate heavy repetition vs counts and stay
    valid (smoke-level semantic check)."""
    from helix_amd.engine.engine import EngineConfig, LLMEngine
    from helix_amd.engine.sampling_params import SamplingParams
    cfg = EngineConfig(model="tiny-gqa", max_num_seqs=4, max_model_len=256,
                       kv_cache_blocks=256, eos_token_id=-1)
    eng = LLMEngine(cfg, device="cuda:0")
    sp = SamplingParams(temperature=0.8, top_p=0.9, max_tokens=24,
                        repetition_penalty=1.3, presence_penalty=0.2,
                        ignore_eos=True, seed=7)
    out = eng.generate([[1, 2, 3, 4, 5, 6, 7, 8]], sp)
    assert len(out[0]) == 24
    assert eng._pen_counts is not None   # GPU penalty tables engaged
