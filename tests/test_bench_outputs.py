"""bench.py --dump-outputs: the tap must hand back exactly what the last
engine step returned, indexed by request, in float .npy files."""
import numpy as np

import bench
from helix_amd.engine.engine import EngineConfig, LLMEngine
from helix_amd.engine.sampling_params import SamplingParams


def _tiny_engine(n_req):
    eng = LLMEngine(EngineConfig(model="tiny-gqa", max_model_len=64,
                                 max_num_seqs=n_req, kv_cache_blocks=64,
                                 eos_token_id=-1), device="cpu")
    sp = SamplingParams(temperature=0.0, max_tokens=10 ** 9, ignore_eos=True)
    for i in range(n_req):
        eng.add_request(f"bench-{i}", [3 + i, 5, 7 + i], sp)
    return eng


def test_dump_outputs_matches_last_step(tmp_path):
    eng = _tiny_engine(3)
    tap = bench.OutputTap(eng)
    while eng.waiting:
        eng.step()
    for _ in range(2):
        events = eng.step()
    tap.events = events
    tap.dump(str(tmp_path))

    tokens = np.load(tmp_path / "tokens.npy")
    logits = np.load(tmp_path / "logits.npy")
    cols = np.load(tmp_path / "logits_cols.npy")
    assert tokens.dtype == np.float64 and logits.dtype == np.float32
    V = eng.model_cfg.vocab_size
    assert tokens.shape == (3,) and logits.shape == (3, V)
    assert np.array_equal(cols, np.arange(V))
    want = {int(s.seq_id.rsplit("-", 1)[1]): t for s, t, _ in events}
    assert [int(t) for t in tokens] == [want[i] for i in range(3)]
    # greedy: every returned token is the argmax of its dumped row
    assert np.array_equal(logits.argmax(1), tokens.astype(np.int64))


def test_dump_outputs_samples_wide_logits(tmp_path, monkeypatch):
    eng = _tiny_engine(2)
    tap = bench.OutputTap(eng)
    while eng.waiting:
        eng.step()
    tap.events = eng.step()
    V = eng.model_cfg.vocab_size
    ncols = V // 4
    monkeypatch.setattr(bench, "DUMP_LOGITS_BYTES", 4 * 2 * ncols)
    tap.dump(str(tmp_path / "a"))
    tap.dump(str(tmp_path / "b"))
    cols = np.load(tmp_path / "a" / "logits_cols.npy").astype(np.int64)
    assert cols.shape == (ncols,) and np.all(np.diff(cols) > 0)
    assert np.array_equal(cols, np.load(tmp_path / "b" / "logits_cols.npy"))
    sample = np.load(tmp_path / "a" / "logits.npy")
    full = tap.logits.float().numpy()
    assert np.array_equal(sample, full[:, cols])
