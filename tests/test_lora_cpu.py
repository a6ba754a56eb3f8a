"""Multi-LoRA serving on the CPU reference path: PEFT loader and packing,
dynamic adapter vs merged weights, mixed batches, prefix cache, slots."""
import json
import os

import pytest
import torch

from helix_amd.engine.engine import EngineConfig, LLMEngine, SeqStatus
from helix_amd.engine.sampling_params import SamplingParams
from helix_amd.models import lora as L
from helix_amd.models.llama import LlamaForCausalLM, PRESETS, PrefillMeta

CFG = PRESETS["tiny-gqa"]
R = 16
SP = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
PROMPT = [(7 * i + 3) % 1000 + 1 for i in range(19)]


def fp32_model(seed=0):
    return LlamaForCausalLM(CFG).float().init_random(seed)


def make_adapter(path, seed, r=R, targets=L.ALL_TARGETS, zero_b=False):
    """B ~ N(0, 0.05), alpha = 4r: a delta as large as the base output."""
    t = L.random_adapter_tensors(CFG, r, targets, seed=seed, b_std=0.05,
                                 zero_b=zero_b)
    L.save_peft_adapter(str(path), t, r=r, lora_alpha=4 * r,
                        target_modules=targets)
    return t


def make_engine(max_loras=2, model=None, **kw):
    cfg = EngineConfig(model="tiny-gqa", max_model_len=256, max_num_seqs=8,
                       kv_cache_blocks=128, eos_token_id=-1,
                       max_loras=max_loras, max_lora_rank=R, **kw)
    return LLMEngine(cfg, device="cpu",
                     model=model if model is not None else fp32_model())


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    d = tmp_path_factory.mktemp("loras")
    return {
        "a1": (str(d / "a1"), make_adapter(d / "a1", seed=1)),
        "a2": (str(d / "a2"), make_adapter(d / "a2", seed=2)),
        "a3": (str(d / "a3"), make_adapter(d / "a3", seed=3, r=8)),
        "zero": (str(d / "zero"), make_adapter(d / "zero", seed=4,
                                               zero_b=True)),
    }


def engine_with(adapters, names, **kw):
    eng = make_engine(**kw)
    for n in names:
        eng.add_lora(n, adapters[n][0])
    return eng


def merged_model(tensors, r, alpha):
    """Twin with W + (alpha/r) * B @ A merged into each fused slice."""
    m = fp32_model()
    q, kv, inter = CFG.q_size, CFG.kv_size, CFG.intermediate_size
    rows = {"q_proj": (0, q), "k_proj": (q, q + kv),
            "v_proj": (q + kv, q + 2 * kv), "o_proj": (0, CFG.hidden_size),
            "gate_proj": (0, inter), "up_proj": (inter, 2 * inter),
            "down_proj": (0, CFG.hidden_size)}
    for i, layer in enumerate(m.layers):
        for mod, (lo, hi) in rows.items():
            sub, proj, _ = L.HF_TARGETS[mod]
            w = getattr(getattr(layer, sub), proj).weight.data
            delta = (alpha / r) * (tensors[L.hf_key(i, mod, "B")]
                                   @ tensors[L.hf_key(i, mod, "A")])
            w[lo:hi] += delta
    return m


def prefill_logits(model, slot=None):
    T = len(PROMPT)
    meta = PrefillMeta(
        cu_seqlens=torch.tensor([0, T], dtype=torch.int32), max_seqlen=T,
        slot_mapping=torch.zeros(T, dtype=torch.int64),
        positions=torch.arange(T, dtype=torch.int64),
        lora_slots=(torch.full((T,), slot, dtype=torch.int32)
                    if slot is not None else None))
    hidden = model(torch.tensor(PROMPT), None, meta)
    return model.compute_logits(hidden)


def test_dynamic_adapter_matches_merged_weights(adapters):
    path, tensors = adapters["a1"]
    dyn = fp32_model()
    eng = make_engine(model=dyn)
    eng.add_lora("a1", path)
    slot = eng.lora.acquire("a1")
    twin = merged_model(tensors, R, 4 * R)
    got = prefill_logits(dyn, slot)
    want = prefill_logits(twin)
    base = prefill_logits(fp32_model())
    assert (want - base).abs().max() > 0.1        # the adapter matters
    torch.testing.assert_close(got, want, atol=1e-4, rtol=1e-4)
    # no slots on the meta => the base model, manager or not
    assert torch.equal(prefill_logits(dyn), base)

    out = eng.generate([PROMPT], SP, loras=["a1"])
    want_out = make_engine(max_loras=0, model=twin).generate([PROMPT], SP)
    assert out == want_out


def test_zero_b_adapter_equals_base(adapters):
    eng = engine_with(adapters, ["zero"])
    base = make_engine(max_loras=0)
    prompts = [PROMPT, PROMPT[:7]]
    assert eng.generate(prompts, SP, loras=["zero", "zero"]) == \
        base.generate(prompts, SP)


def test_mixed_batch_rows_match_solo(adapters):
    names = [None, "a1", "a2", "a1"]
    prompts = [PROMPT, PROMPT[:11], PROMPT[3:], PROMPT[:11]]
    mixed = engine_with(adapters, ["a1", "a2"]).generate(
        prompts, SP, loras=names)
    for p, n, got in zip(prompts, names, mixed):
        solo = engine_with(adapters, ["a1", "a2"]).generate(
            [p], SP, loras=[n])[0]
        assert got == solo, n
    base = make_engine(max_loras=0).generate(prompts, SP)
    assert mixed[0] == base[0]
    assert mixed[1] != base[1] and mixed[2] != base[2]
    assert mixed[1] == mixed[3]


def test_prefix_cache_is_keyed_by_adapter_and_generation(adapters):
    eng = engine_with(adapters, ["a1"])
    prompt = [(5 * i) % 900 + 1 for i in range(40)]

    def run(name):
        eng._n = getattr(eng, "_n", 0) + 1
        seq = eng.add_request(f"r{eng._n}", prompt, SP, lora=name)
        while eng.has_work:
            eng.step()
        return seq.cached_prefix

    assert run(None) == 0
    assert run("a1") == 0
    assert run("a1") > 0
    eng.remove_lora("a1")
    assert eng.list_loras() == []
    eng.add_lora("a1", adapters["a2"][0])
    assert run("a1") == 0
    assert run(None) > 0          # base-model hashes are untouched


def test_slot_eviction_and_pinned_stall(adapters):
    eng = engine_with(adapters, ["a1", "a2", "a3"], max_loras=1)
    solo = {n: engine_with(adapters, [n]).generate([PROMPT], SP,
                                                    loras=[n])[0]
            for n in ("a1", "a2", "a3")}
    # three adapters through one slot, one after the other
    for n in ("a1", "a2", "a3", "a1"):
        assert eng.generate([PROMPT], SP, loras=[n])[0] == solo[n]
    # a2 queued behind a running a1: its eviction would hit a pinned slot
    s1 = eng.add_request("p1", PROMPT, SP, lora="a1")
    s2 = eng.add_request("p2", PROMPT, SP, lora="a2")
    eng.step()
    assert s1.status == SeqStatus.RUNNING
    assert s2.status == SeqStatus.WAITING and not s2.block_table
    assert eng.lora.slots == ["a1"]
    with pytest.raises(ValueError):
        eng.remove_lora("a1")                      # still referenced
    while eng.has_work:
        eng.step()
        if s1.status == SeqStatus.RUNNING:
            assert eng.lora.slots == ["a1"]
    assert s1.output_ids == solo["a1"]
    assert s2.output_ids == solo["a2"]
    assert eng.num_free_blocks() == 128


def test_request_errors(adapters):
    eng = engine_with(adapters, ["a1"])
    with pytest.raises(ValueError, match="unknown LoRA"):
        eng.add_request("x", PROMPT, SP, lora="nope")
    off = make_engine(max_loras=0)
    with pytest.raises(ValueError, match="max_loras=0"):
        off.add_request("x", PROMPT, SP, lora="a1")
    with pytest.raises(ValueError):
        off.add_lora("a1", adapters["a1"][0])
    with pytest.raises(ValueError, match="tp_size"):
        LLMEngine(EngineConfig(model="tiny-gqa", kv_cache_blocks=16,
                               max_loras=1), device="cpu",
                  model=fp32_model(), tp_size=2)


def test_loader_pads_rank_and_zero_fills_missing_targets(tmp_path):
    targets = ("q_proj", "v_proj", "down_proj")
    t = make_adapter(tmp_path / "part", seed=9, r=8, targets=targets)
    ad = L.load_peft_adapter(str(tmp_path / "part"), CFG, max_lora_rank=16)
    assert ad.r == 8 and ad.scale == 4.0
    q, kv = CFG.q_size, CFG.kv_size
    A, B = ad.packed[(1, "qkv_proj")]
    assert A.shape == (48, CFG.hidden_size) and B.shape == (q + 2 * kv, 16)
    assert torch.equal(A[0:8], t[L.hf_key(1, "q_proj", "A")])
    assert not A[8:32].any()                  # rank padding + absent k_proj
    assert torch.equal(A[32:40], t[L.hf_key(1, "v_proj", "A")])
    assert not A[40:48].any()
    assert torch.equal(B[:q, :8], t[L.hf_key(1, "q_proj", "B")])
    assert not B[:, 8:].any() and not B[q:q + kv].any()
    assert torch.equal(B[q + kv:, :8], t[L.hf_key(1, "v_proj", "B")])
    for proj in ("o_proj", "gate_up_proj"):
        A, B = ad.packed[(0, proj)]
        assert not A.any() and not B.any()
    A, B = ad.packed[(3, "down_proj")]
    assert torch.equal(A[:8], t[L.hf_key(3, "down_proj", "A")])
    assert torch.equal(B[:, :8], t[L.hf_key(3, "down_proj", "B")])


def test_loader_rejects_bad_adapters(tmp_path):
    make_adapter(tmp_path / "big", seed=1, r=32)
    with pytest.raises(ValueError, match="max_lora_rank"):
        L.load_peft_adapter(str(tmp_path / "big"), CFG, max_lora_rank=16)
    # unsupported target module
    make_adapter(tmp_path / "emb", seed=1)
    cfg_path = os.path.join(tmp_path / "emb", "adapter_config.json")
    with open(cfg_path) as f:
        c = json.load(f)
    c["target_modules"].append("lm_head")
    with open(cfg_path, "w") as f:
        json.dump(c, f)
    with pytest.raises(ValueError, match="unsupported"):
        L.load_peft_adapter(str(tmp_path / "emb"), CFG)
    # shapes of another model
    t = L.random_adapter_tensors(PRESETS["tiny"], R, seed=1)
    L.save_peft_adapter(str(tmp_path / "other"), t, r=R, lora_alpha=R)
    with pytest.raises(ValueError, match="shape"):
        L.load_peft_adapter(str(tmp_path / "other"), CFG)


def test_ops_reference_semantics():
    """ref.lora_* against the written-out formula, incl. untouched rows."""
    import helix_amd.ops as ops
    torch.manual_seed(0)
    T, K, Rm, S = 6, 32, 8, 2
    widths = (16, 8, 8)
    n_off = (0, 16, 24, 32)
    x = torch.randn(T, K)
    A = torch.randn(S, 3 * Rm, K)
    B = torch.randn(S, 32, Rm)
    scale = torch.tensor([0.5, 2.0])
    slot = torch.tensor([0, -1, 1, 2, 1, 0], dtype=torch.int32)
    base = torch.randn(T, 32)
    out = ops.lora_apply(base.clone(), x, A, B, slot, scale, n_off)
    for t in range(T):
        s = int(slot[t])
        if not 0 <= s < S:
            assert torch.equal(out[t], base[t])
            continue
        y = A[s] @ x[t]
        for i, w in enumerate(widths):
            lo, hi = n_off[i], n_off[i + 1]
            want = base[t, lo:hi] + scale[s] * (
                B[s, lo:hi] @ y[i * Rm:(i + 1) * Rm])
            torch.testing.assert_close(out[t, lo:hi], want, atol=1e-5,
                                       rtol=1e-5)
