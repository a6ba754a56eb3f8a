"""lora_id through the serving stack on CPU: runner OpenAI surface,
adapter directory resolution, and an assistant's lora_id from helix.yaml."""
import json

import pytest
from fastapi.testclient import TestClient

from helix_amd.models import lora as L
from helix_amd.models.llama import PRESETS
from helix_amd.runner.http import create_runner_app
from helix_amd.runner.service import (ModelNotFoundError, ModelSpec,
                                      RunnerService, estimate_model_bytes)

CFG = PRESETS["tiny"]
MSG = [{"role": "user", "content": "hello adapters"}]


def tiny_spec(lora_dir, max_loras=2):
    return ModelSpec("tiny", "llm", "tiny", max_model_len=256,
                     kv_cache_blocks=256, max_loras=max_loras,
                     max_lora_rank=16, lora_dir=lora_dir)


@pytest.fixture(scope="module")
def service(tmp_path_factory):
    d = tmp_path_factory.mktemp("loras")
    for seed, (name, zero) in enumerate([("tuned", False), ("zero", True)],
                                        start=1):
        t = L.random_adapter_tensors(CFG, 16, seed=seed, b_std=0.05,
                                     zero_b=zero)
        L.save_peft_adapter(str(d / name), t, r=16, lora_alpha=64)
    (d / "empty").mkdir()
    svc = RunnerService(device="cpu", memory_budget=64 << 30,
                        specs={"tiny": tiny_spec(str(d)),
                               "tiny-nolora": tiny_spec(str(d), 0)})
    yield svc
    svc.shutdown()


@pytest.fixture(scope="module")
def client(service):
    with TestClient(create_runner_app(service)) as c:
        yield c


def chat(client, lora_id=None, model="tiny", stream=False):
    body = {"model": model, "messages": MSG, "max_tokens": 12,
            "temperature": 0}
    if lora_id is not None:
        body["lora_id"] = lora_id
    if not stream:
        return client.post("/v1/chat/completions", json=body)
    with client.stream("POST", "/v1/chat/completions",
                       json={**body, "stream": True}) as r:
        assert r.status_code == 200
        lines = [l for l in r.iter_lines() if l.startswith("data: ")]
    chunks = [json.loads(l[6:]) for l in lines[:-1]]
    return "".join(c["choices"][0]["delta"].get("content") or ""
                   for c in chunks)


def tokens_of(service, lora=None):
    """Greedy token ids for MSG straight from the loaded engine's records
    (text can hide differences between undecodable byte tokens)."""
    eng = service.instances["tiny"].engine
    seqs = [s for s in eng.seqs.values() if s.lora == lora]
    return seqs[-1].output_ids


def test_lora_id_changes_output_and_zero_b_does_not(client, service):
    base = chat(client)
    assert base.status_code == 200, base.text
    tuned = chat(client, "tuned")
    assert tuned.status_code == 200, tuned.text
    assert tuned.json()["model"] == "tiny"
    zero = chat(client, "zero")
    assert zero.status_code == 200, zero.text
    text = lambda r: r.json()["choices"][0]["message"]["content"]  # noqa: E731
    assert tokens_of(service, "tuned") != tokens_of(service, None)
    assert text(tuned) != text(base)
    assert tokens_of(service, "zero") == tokens_of(service, None)
    assert text(zero) == text(base)
    assert sorted(service.instances["tiny"].engine.list_loras()) == \
        ["tuned", "zero"]


def test_lora_id_streaming(client):
    assert chat(client, "tuned", stream=True) == \
        chat(client, "tuned").json()["choices"][0]["message"]["content"]
    assert chat(client, "tuned", stream=True) != chat(client, stream=True)


@pytest.mark.parametrize("bad", ["nope", "../tuned", "a/b", "..", "empty"])
def test_unknown_lora_id_is_rejected_like_unknown_model(client, bad):
    want = client.post("/v1/chat/completions",
                       json={"model": "no-such-model", "messages": MSG})
    r = chat(client, bad)
    assert r.status_code == want.status_code == 404
    assert r.json()["error"]["type"] == want.json()["error"]["type"]
    assert bad in r.json()["error"]["message"]


def test_model_without_slots_rejects_lora_id(client, service):
    r = chat(client, "tuned", model="tiny-nolora")
    assert r.status_code == 404
    with pytest.raises(ModelNotFoundError):
        service.instances["tiny-nolora"].resolve_lora("tuned")


def test_estimate_counts_slot_stacks(tmp_path):
    off = estimate_model_bytes(tiny_spec(str(tmp_path), 0))
    on = estimate_model_bytes(tiny_spec(str(tmp_path), 2))
    assert on - off == L.lora_stack_bytes(CFG, 2, 16) > 0


def test_assistant_lora_id_from_yaml_reaches_engine(service, tmp_path):
    from helix_amd.server.app import create_app
    from helix_amd.server.apps import parse_helix_yaml
    from helix_amd.server.config import ServerConfig
    from helix_amd.store import Store
    cfg = ServerConfig()
    cfg.filestore.path = str(tmp_path / "fs")
    cfg.inference.default_provider = "helix"
    cfg.inference.default_model = "tiny"
    app = create_app(cfg, store=Store(":memory:"), runner_service=service)
    client = TestClient(app)
    H = {"Authorization": "Bearer admin-key"}
    helix = parse_helix_yaml("""
name: tuned-bot
assistants:
  - name: default
    model: tiny
    lora_id: tuned
    temperature: 0
    max_tokens: 12
""")
    assert helix.assistants[0].lora_id == "tuned"
    r = client.post("/api/v1/apps",
                    json={"config": helix.model_dump(by_alias=True)},
                    headers=H)
    assert r.status_code == 200, r.text
    app_id = r.json()["id"]
    eng = service.ensure_loaded("tiny").engine
    before = set(eng.seqs)
    r = client.post("/v1/chat/completions",
                    json={"app_id": app_id, "messages": MSG}, headers=H)
    assert r.status_code == 200, r.text
    new = [eng.seqs[k] for k in set(eng.seqs) - before]
    assert new and all(s.lora == "tuned" for s in new)
    # an explicit lora_id on the request wins over the assistant's
    before = set(eng.seqs)
    r = client.post("/v1/chat/completions",
                    json={"app_id": app_id, "messages": MSG,
                          "lora_id": "zero"}, headers=H)
    assert r.status_code == 200, r.text
    new = [eng.seqs[k] for k in set(eng.seqs) - before]
    assert new and all(s.lora == "zero" for s in new)
