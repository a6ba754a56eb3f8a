"""ops.lora_group's contract and ops.lora_apply(groups=...) on the CPU."""
import pytest
import torch

import helix_amd.ops as ops
import helix_amd.ops.reference as ref


def test_lora_group_contract():
    S = 5                                        # slots 3 and 4 stay empty
    slot = torch.tensor([2, -1, 0, 2, 5, 0, 2, 7, 1, 0], dtype=torch.int32)
    off, rows = ops.lora_group(slot, S)
    assert off.dtype == rows.dtype == torch.int32
    assert tuple(off.shape) == (S + 1,) and tuple(rows.shape) == (10,)
    lists = [rows[off[s]:off[s + 1]].tolist() for s in range(S)]
    assert lists == [[2, 5, 9], [8], [0, 3, 6], [], []]
    assert off[0] == 0 and off[S] == 7           # rows 1, 4, 7 are in no list
    with pytest.raises(ValueError):
        ops.lora_group(slot, 257)
    with pytest.raises(ValueError):
        ops.lora_group(slot.long(), S)


def test_lora_apply_with_groups_equals_reference():
    g = torch.Generator().manual_seed(0)
    T, K, S, R, n_off = 21, 64, 3, 8, [0, 32, 48]
    x = torch.randn(T, K, generator=g)
    A = torch.randn(S, 2 * R, K, generator=g) / 8
    B = torch.randn(S, 48, R, generator=g)
    scale = torch.tensor([0.5, 2.0, 1.0])
    base = torch.randn(T, 48, generator=g)
    slot = torch.tensor([[-1, 0, 2, 1, S, -1][t % 6] for t in range(T)],
                        dtype=torch.int32)
    y = torch.zeros(T, 2 * R)
    ref.lora_shrink(y, x, A, slot)
    want = ref.lora_expand(base.clone(), y, B, slot, scale, n_off)
    got = ops.lora_apply(base.clone(), x, A, B, slot, scale, n_off,
                         groups=ops.lora_group(slot, S))
    assert torch.equal(got, want)
    assert not torch.equal(got, base)
