"""Decode cases for the block ids that paged_attn_decode.hip stages in LDS.

Shared by tests/test_decode_blockids_gpu.py and
tests/test_decode_blockids_cpu.py. The kernel keeps, per 128-token chunk,
the physical ids of the blocks the chunk touches in a small LDS buffer and
addresses a token with shift and mask. What can go wrong there is a matter
of block size and of where a chunk starts:
  * block sizes 8 .. 256: 17 ids per chunk at the low end; one id that
    serves several chunks at the high end (bs > CHUNK);
  * windows 131 and 203 at block sizes 16 and 8: kv_lo is then no multiple
    of the block size, every chunk starts off the block grid and straddles
    CHUNK / bs + 1 blocks (9 and 17);
  * split-K at block size 64, fp8 at D = 64 / G = 8, the full-grid VPS = 4
    kernel at block size 32, and the engine's calling convention (a
    persistent workspace, max_len rounded up to a bucket) at block size 32;
  * the same block sizes and windows with a workspace of one partition
    (ws_len = 128). The short batches above are split into partitions of
    one chunk each, so only the full-grid rows walk several chunks; with
    a single partition every row does, and the ids staged two chunks
    ahead are used.
"""
import attn_oracle as ao

LENS6 = (1, 127, 128, 129, 300, 700)


def _cases():
    cs = []
    for bs in (8, 32, 64, 128, 256):
        cs.append(ao.DecodeCase(f"ids-bs{bs}", 128, 4, LENS6, bs=bs))
    for bs in (16, 8):
        for w in (131, 203):
            cs.append(ao.DecodeCase(f"ids-window{w}-bs{bs}", 128, 4,
                                    (300, 700), window=w, bs=bs))
    cs.append(ao.DecodeCase("ids-splitk-bs64", 128, 1, (129, 700, 2048),
                            bs=64))
    cs.append(ao.DecodeCase("ids-fp8-d64-g8-bs32", 64, 8, (129, 700),
                            kv8=True, bs=32))
    cs.append(ao.DecodeCase("ids-fullgrid-bs32", 128, 4,
                            tuple(ao.FIVE[i % 5] for i in range(256)),
                            hkv=8, bs=32))
    for bs in (8, 64, 256):
        cs.append(ao.DecodeCase(f"ids-onepart-bs{bs}", 128, 4,
                                (129, 300, 700), bs=bs, ws_len=128))
    for bs in (16, 8):
        cs.append(ao.DecodeCase(f"ids-onepart-window203-bs{bs}", 128, 4,
                                (300, 700), window=203, bs=bs, ws_len=128))
    return ao._both(cs)


def _engine_cases():
    return [ao.DecodeCase("ids-engine-bs32", 128, 4, (1, 127, 300), bs=32,
                          max_len=m, ws_len=4096, table_cols=4096 // 32 + 1,
                          tag=f"-maxlen{m}")
            for m in (512, 4096)]


CASES = _cases()
ENGINE_CASES = _engine_cases()
