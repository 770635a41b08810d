"""CPU: the host half of cross-encoder re-ranking -- pair tokenisation (Python restatement and native batch routine vs
BertTokenizerFast goldens), the C-ABI's argument checks, EmbeddingManager.rerank_results and POST /query with
"rerank"."""
import asyncio
import ctypes
import json
import os

import numpy as np
import pytest
from starlette.testclient import TestClient

from multimodal_rag_amd import embedder as emb_mod
from multimodal_rag_amd.embedder import RESULT_KEYS, EmbeddingManager
from multimodal_rag_amd.server import create_app
from multimodal_rag_amd.tokenizer import NativeWordPieceTokenizer, WordPieceTokenizer, longest_first
from tests.fakes import FakeEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def vocab():
    with open(os.path.join(GOLDEN, "cross_encoder_vocab.txt"), encoding="utf-8") as f:
        return {line.rstrip("\n"): i for i, line in enumerate(f)}


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(GOLDEN, "cross_encoder_pairs.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def test_python_pair_encoding_matches_golden(vocab, cases):
    tk = WordPieceTokenizer(vocab)
    for c in cases:
        assert tk.encode_pair(c["a"], c["b"], c["max_length"]) == (c["ids"], c["type_ids"]), c


def test_native_pair_encoding_matches_golden(vocab, cases):
    tk = NativeWordPieceTokenizer(vocab, n_threads=4)
    for c in cases:
        ids, types, lens = tk.encode_pairs_arrays([c["a"]] * 3, [c["b"]] * 3, c["max_length"])
        for i in range(3):
            assert ids[i, : lens[i]].tolist() == c["ids"] and types[i, : lens[i]].tolist() == c["type_ids"], c


def test_pair_encoding_matches_live_fast_tokenizer(vocab, cases):
    tf = pytest.importorskip("transformers")
    fast = tf.BertTokenizerFast(os.path.join(GOLDEN, "cross_encoder_vocab.txt"), do_lower_case=True)
    nat = NativeWordPieceTokenizer(vocab)
    g = np.random.default_rng(3)
    words = [w for w in vocab if not w.startswith("[")] + ["xyz", "Über", "naïve", "日本"]
    for _ in range(60):
        a = " ".join(g.choice(words, int(g.integers(0, 30))))
        b = " ".join(g.choice(words, int(g.integers(0, 40))))
        ml = int(g.integers(3, 40))
        e = fast([a], [b], truncation="longest_first", max_length=ml)
        ids, types, lens = nat.encode_pairs_arrays([a], [b], ml)
        assert ids[0, : lens[0]].tolist() == e["input_ids"][0] and types[0, : lens[0]].tolist() == e["token_type_ids"][0]


def test_native_equals_python_on_fuzzed_pairs(vocab):
    py, nat = WordPieceTokenizer(vocab), NativeWordPieceTokenizer(vocab, n_threads=8)
    g = np.random.default_rng(11)
    alphabet = list("abcdefghij klmnop qrstuvwxyz.,!?'-0123456789") + ["é", "中", "日", "\t", " ", "Ü"]
    q = "what is the quick fox"
    firsts, seconds = [], []
    for i in range(400):
        firsts.append(q if i % 3 else "".join(g.choice(alphabet, int(g.integers(0, 60)))))   # repeated queries
        seconds.append("".join(g.choice(alphabet, int(g.integers(0, 400)))))
    for ml in (3, 7, 64, 512):
        ids, types, lens = nat.encode_pairs_arrays(firsts, seconds, ml)
        for i in range(len(firsts)):
            r, t = py.encode_pair(firsts[i], seconds[i], ml)
            assert ids[i, : lens[i]].tolist() == r and types[i, : lens[i]].tolist() == t, (ml, i)


def test_longest_first_rule():
    assert longest_first(3, 4, 10) == (3, 4)          # fits
    assert longest_first(2, 20, 10) == (2, 8)         # the shorter side fits: the longer gets the rest
    assert longest_first(20, 2, 10) == (8, 2)
    assert longest_first(8, 20, 10) == (5, 5)         # both overflow: half each
    assert longest_first(20, 8, 11) == (6, 5)         # the odd token to the longer side
    assert longest_first(8, 20, 11) == (5, 6)
    assert longest_first(9, 9, 11) == (5, 6)          # equal: to the second side
    assert longest_first(5, 5, 0) == (0, 0)


def test_abi_argument_errors_without_gpu():
    from multimodal_rag_amd import _native

    L = _native.lib()
    d = _native.EncoderDesc(arch=_native.ARCH_BERT, n_layers=2, hidden=128, n_heads=4, intermediate=256, vocab=1000,
                            max_pos=64, pool=0, act=_native.ACT_GELU, causal=0, normalize=1, out_dim=128, ln_eps=1e-12)
    dp = ctypes.byref(d)
    w = (ctypes.c_void_p * 40)(*([16] * 40))
    x = ctypes.c_void_p(256)
    for fwd, wsb in ((L.mmrag_cross_encoder_forward, L.mmrag_cross_encoder_workspace_bytes),
                     (L.mmrag_cross_encoder_forward_f32, L.mmrag_cross_encoder_f32_workspace_bytes)):
        need = wsb(dp, 100, 2)
        assert need > wsb(dp, 10, 2) > 0 and wsb(dp, 0, 2) == 0
        call = lambda nl=1, ws=need, desc=dp, t=x: fwd(desc, w, nl, t, x, x, x, 100, 2, 64, x, x, ws, None)  # noqa: E731
        assert call(nl=0) == 1 and call(nl=17) == 1                        # MMRAG_EINVAL
        assert call(t=None) == 1                                           # null type_ids
        assert call(ws=need - 1) == 2                                      # MMRAG_EWORKSPACE
        pre = _native.EncoderDesc(**{f: getattr(d, f) for f, _ in d._fields_})
        pre.arch = _native.ARCH_PRELN
        assert call(desc=ctypes.byref(pre)) == 1
        odd = _native.EncoderDesc(**{f: getattr(d, f) for f, _ in d._fields_})
        odd.n_heads = 1                                                    # head dim 128: not built
        assert call(desc=ctypes.byref(odd)) == 1
        assert fwd(dp, w, 1, x, x, x, x, 0, 2, 64, x, x, need, None) == 1  # T = 0
    # pool / normalize are ignored: the workspace does not depend on them
    d2 = _native.EncoderDesc(**{f: getattr(d, f) for f, _ in d._fields_})
    d2.pool, d2.normalize = 2, 0
    assert L.mmrag_cross_encoder_workspace_bytes(ctypes.byref(d2), 100, 2) == L.mmrag_cross_encoder_workspace_bytes(dp, 100, 2)
    tk = NativeWordPieceTokenizer({"[CLS]": 0, "[SEP]": 1, "[UNK]": 2, "a": 3})
    arr = np.zeros(8, np.int32)
    off = np.zeros(2, np.int64)
    assert L.mmrag_wordpiece_encode_pairs(tk._h, None, off.ctypes.data, None, off.ctypes.data, 1, 2, arr.ctypes.data,
                                          arr.ctypes.data, arr.ctypes.data, 1) == 1         # max_length < 3


# ---------------------------------------------------------------- rerank_results with a fake scorer
class FakeScorer:
    def __init__(self, table):
        self.table, self.calls = table, []

    def predict(self, pairs, batch_size=32, apply_sigmoid=None):
        self.calls.append(list(pairs))
        return np.array([self.table.get(d, 0.0) for _, d in pairs], np.float32)


def results(docs):
    n = len(docs)
    return {"ids": [f"id{i}" for i in range(n)], "distances": [0.1 * i for i in range(n)],
            "metadatas": [{"i": i} for i in range(n)], "documents": list(docs)}


def test_rerank_orders_by_score_stable_and_truncates(monkeypatch):
    m = EmbeddingManager(engine=FakeEngine())
    m._reranker = FakeScorer({"b": 3.0, "c": 1.0, "d": 3.0, "e": -1.0})
    res = results(["a", "b", "c", "d", None, "e"])
    out = asyncio.run(m.rerank_results("q", res, top_k=4))
    assert out["ids"] == ["id1", "id3", "id2", "id0"]          # 3.0 (b before d: ties keep search order), 1.0, 0.0
    assert out["rerank_scores"] == [3.0, 3.0, 1.0, 0.0]
    assert out["documents"] == ["b", "d", "c", "a"] and out["metadatas"] == [{"i": 1}, {"i": 3}, {"i": 2}, {"i": 0}]
    assert out["distances"] == [res["distances"][i] for i in (1, 3, 2, 0)]
    assert set(out) == set(RESULT_KEYS) | {"rerank_scores"}
    assert m._reranker.calls[-1] == [("q", d if d is not None else "") for d in res["documents"]]   # None -> ""
    full = asyncio.run(m.rerank_results("q", res))
    assert len(full["ids"]) == 6 and full["ids"][-1] == "id5" and full["ids"][3:5] == ["id0", "id4"]
    empty = asyncio.run(m.rerank_results("q", results([]), top_k=3))
    assert empty["ids"] == [] and empty["rerank_scores"] == []


def test_rerank_loads_once_from_configured_dir(monkeypatch):
    loads = []

    class Fake:
        @classmethod
        def from_local_dir(cls, path, device="cuda:0", **kw):
            loads.append((path, device))
            return FakeScorer({"x": 1.0})

    import multimodal_rag_amd.reranker as rr

    monkeypatch.setattr(rr, "DeviceCrossEncoder", Fake)
    monkeypatch.setattr(emb_mod.settings, "MMRAG_RERANKER_DIR", "/models/ce")
    m = EmbeddingManager(engine=FakeEngine())
    assert m.has_reranker()
    for _ in range(3):
        out = asyncio.run(m.rerank_results("q", results(["y", "x"]), top_k=1))
        assert out["ids"] == ["id1"] and out["rerank_scores"] == [1.0]
    assert len(loads) == 1 and loads[0][0] == "/models/ce"


def test_unconfigured_rerank_is_the_reference_stub(monkeypatch, caplog):
    monkeypatch.setattr(emb_mod.settings, "MMRAG_RERANKER_DIR", "")
    m = EmbeddingManager(engine=FakeEngine())
    assert not m.has_reranker()
    res = results(["a", "b", "c"])
    with caplog.at_level("WARNING"):
        out = asyncio.run(m.rerank_results("q", res, top_k=2))
    assert out == {k: res[k][:2] for k in RESULT_KEYS} and "rerank_scores" not in out
    assert "Re-ranking not implemented yet" in caplog.text
    assert asyncio.run(m.rerank_results("q", res)) is res
    assert asyncio.run(m.rerank_results("q", res, top_k=5)) is res


# ---------------------------------------------------------------- POST /query with "rerank"
def upload_docs(client):
    for i, body in enumerate(["alpha beta gamma. " * 3, "delta epsilon. " * 3, "zeta eta theta. " * 3]):
        r = client.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
        assert r.status_code == 200, r.text


def test_query_rerank_flag(monkeypatch):
    from multimodal_rag_amd import server

    monkeypatch.setattr(server.settings, "MMRAG_RERANK_CANDIDATES", 20)
    m = EmbeddingManager(engine=FakeEngine())
    asked = []
    orig_query = m.query

    async def spy(q, n_results=5, filter_dict=None):
        asked.append(n_results)
        return await orig_query(q, n_results, filter_dict)

    m.query = spy
    app = create_app(embedder=m)
    with TestClient(app) as c:
        upload_docs(c)
        plain = c.post("/query", json={"query": "delta", "top_k": 2}).json()
        assert asked[-1] == 2 and all("rerank_score" not in s for s in plain["sources"])
        assert c.post("/query", json={"query": "delta", "top_k": 2, "rerank": False}).json()["sources"] == plain["sources"]
        # no cross-encoder configured: 400 with a plain message
        monkeypatch.setattr(server.settings, "MMRAG_RERANKER_DIR", "")
        r = c.post("/query", json={"query": "delta", "top_k": 2, "rerank": True})
        assert r.status_code == 400 and "MMRAG_RERANKER_DIR" in r.json()["detail"]
        # configured: candidates = max(top_k, MMRAG_RERANK_CANDIDATES), best top_k by score, rerank_score per source
        m._reranker = FakeScorer({})
        m._reranker.predict = lambda pairs, **kw: np.array([7.0 if "zeta" in d else 0.0 for _, d in pairs], np.float32)
        r = c.post("/query", json={"query": "delta", "top_k": 2, "rerank": True})
        assert r.status_code == 200, r.text
        body = r.json()
        assert asked[-1] == 20 and len(body["sources"]) == 2
        assert body["sources"][0]["rerank_score"] == 7.0 and body["sources"][1]["rerank_score"] == 0.0
        assert [s["rank"] for s in body["sources"]] == [1, 2]
        assert set(body["sources"][0]) == {"rank", "doc_id", "relevance_score", "type", "rerank_score"}
        monkeypatch.setattr(server.settings, "MMRAG_RERANK_CANDIDATES", 1)
        c.post("/query", json={"query": "delta", "top_k": 3, "rerank": True})
        assert asked[-1] == 3
