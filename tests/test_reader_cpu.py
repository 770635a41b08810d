"""CPU: the host half of the extractive reader -- the selection rule's two Python statements against each other, the
C ABI's surface and argument checks, window cutting and character mapping, the answerable rule, checkpoint refusal and
POST /query with "reader" / "reader_answer"."""
import asyncio
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
from starlette.testclient import TestClient

from multimodal_rag_amd import embedder as emb_mod
from multimodal_rag_amd import reader as RD
from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.server import NO_ANSWER_FOUND, create_app
from multimodal_rag_amd.tokenizer import WordPieceTokenizer
from tests import reader_ref as Q
from tests.fakes import FakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the selection rule
@pytest.mark.parametrize("kind", ["random", "ties", "binary"])
def test_reference_equals_brute_force(kind):
    g = np.random.default_rng({"random": 1, "ties": 2, "binary": 3}[kind])
    for _ in range(40):
        n_tok = int(g.integers(3, 40))
        cs = int(g.integers(1, n_tok))
        cl = int(g.integers(0, n_tok - cs + 1))
        if kind == "random":
            ls, le = g.standard_normal(n_tok).astype(np.float32), g.standard_normal(n_tok).astype(np.float32)
        else:
            hi = 4 if kind == "ties" else 2
            ls, le = g.integers(0, hi, n_tok).astype(np.float32), g.integers(0, hi, n_tok).astype(np.float32)
        L, n = int(g.integers(1, 9)), int(g.integers(1, 9))
        a, b = Q.select_spans(ls, le, cs, cl, L, n), Q.select_spans_brute(ls, le, cs, cl, L, n)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (kind, cs, cl, L, n)
        real = a[0][:, 0] >= 0
        assert np.all(a[0][real, 0] >= cs) and np.all(a[0][real, 1] < cs + cl)
        assert np.all(a[0][real, 1] - a[0][real, 0] < L) and np.all(np.diff(a[1][real]) <= 0)
        assert np.all(a[1][~real] == -np.inf) and np.all(np.diff(real.astype(np.int8)) <= 0)   # padding at the end


def test_reference_rule_on_planted_cases():
    # all equal: lowest i, then lowest j, one token at a time
    z = np.zeros(8, np.float32)
    s, _ = Q.select_spans(z, z, 2, 5, 3, 3)
    assert s.tolist() == [[2, 2], [3, 3], [4, 4]]
    # the runner-up (3, 5) overlaps the winner (3, 4): skipped for (6, 6)
    ls = np.array([0, 0, 0, 5, 0, -3, 1, 0], np.float32)
    le = np.array([0, 0, 0, 0, 5, 4, 2, 0], np.float32)
    s, v = Q.select_spans(ls, le, 1, 7, 4, 2)
    assert s.tolist() == [[3, 4], [6, 6]] and v.tolist() == [10.0, 3.0]
    # more rounds than disjoint spans
    s, v = Q.select_spans(z, z, 1, 2, 64, 8)
    assert s[:2].tolist() == [[1, 1], [2, 2]] and (s[2:] == -1).all() and (v[2:] == -np.inf).all()
    assert (Q.select_spans(z, z, 2, 0, 5, 2)[0] == -1).all()
    a, b = Q.lse_f64(z, z, 3, 4)
    assert abs(a - math.log(5)) < 1e-12 and abs(b - math.log(5)) < 1e-12


# ---------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def N():
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def test_symbols_limits_and_header(N):
    L = ctypes.CDLL(N.LIB_PATH)
    for name in ("mmrag_span_select", "mmrag_reader_workspace_bytes", "mmrag_reader_forward"):
        assert hasattr(L, name), name
    assert N.lib().mmrag_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "mmrag.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define (MMRAG_MAX_READER_TOKENS|MMRAG_MAX_ANSWER_TOKENS|"
                                               r"MMRAG_MAX_READER_SPANS) (\d+)", text)}
    assert limits == {"MMRAG_MAX_READER_TOKENS": 512, "MMRAG_MAX_ANSWER_TOKENS": 64, "MMRAG_MAX_READER_SPANS": 8}
    assert (N.MAX_READER_TOKENS, N.MAX_ANSWER_TOKENS, N.MAX_READER_SPANS) == (512, 64, 8)
    assert (RD.MAX_READER_TOKENS, RD.MAX_ANSWER_TOKENS, RD.MAX_READER_SPANS) == (512, 64, 8)


def test_bad_arguments_are_einval_without_a_gpu(N):
    L = N.lib()
    x = ctypes.c_void_p(256)

    def select(hidden=x, ld=128, H=128, w=x, T=100, B=2, ml=30, n=3, span=x, logits=None):
        return L.mmrag_span_select(hidden, ld, H, w, x, x, x, x, T, B, ml, n, span, x, x, x, logits, None)

    for bad in (dict(ml=0), dict(ml=65), dict(n=0), dict(n=9), dict(H=96), dict(H=1088, ld=1088), dict(H=0, ld=0),
                dict(ld=64), dict(ld=132), dict(T=0), dict(B=0), dict(hidden=None), dict(w=None), dict(span=None),
                dict(hidden=ctypes.c_void_p(264))):
        assert select(**bad) == 1, bad                                     # MMRAG_EINVAL
    d = N.EncoderDesc(arch=N.ARCH_BERT, n_layers=2, hidden=128, n_heads=4, intermediate=256, vocab=1000, max_pos=64,
                      pool=0, act=N.ACT_GELU, causal=0, normalize=1, out_dim=128, ln_eps=1e-12)
    dp = ctypes.byref(d)
    w = (ctypes.c_void_p * 40)(*([16] * 40))
    need = L.mmrag_reader_workspace_bytes(dp, 100, 2)
    assert need > L.mmrag_reader_workspace_bytes(dp, 10, 2) > 0 and L.mmrag_reader_workspace_bytes(dp, 0, 2) == 0
    assert need == L.mmrag_encoder_workspace_bytes(dp, 100, 2)              # no tail buffers: the head has no workspace

    def forward(desc=dp, table=w, t=x, T=100, ml=30, n=3, ws=need, span=x):
        return L.mmrag_reader_forward(desc, table, x, t, x, x, x, x, T, 2, 64, ml, n, span, x, x, x, None, x, ws, None)

    for bad in (dict(ml=0), dict(ml=65), dict(n=0), dict(n=9), dict(t=None), dict(T=0), dict(span=None)):
        assert forward(**bad) == 1, bad
    assert forward(ws=need - 1) == 2                                        # MMRAG_EWORKSPACE
    clone = lambda: N.EncoderDesc(**{f: getattr(d, f) for f, _ in d._fields_})  # noqa: E731
    pre = clone()
    pre.arch = N.ARCH_PRELN
    odd = clone()
    odd.n_heads = 1                                                         # head dim 128: not built
    assert forward(desc=ctypes.byref(pre)) == 1 and forward(desc=ctypes.byref(odd)) == 1
    no_head = (ctypes.c_void_p * 40)(*([16] * 29 + [None] * 11))            # w[5 + 12 * 2] is qa_w
    assert forward(table=no_head) == 1


# ---------------------------------------------------------------- windows and characters
WORDS = ["alpha", "beta", "gamma", "delta", "paris", "berlin", "march", "2019", "the", "capital", "of", "france", "is"]
VOCAB = {t: i for i, t in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ".", ","] + WORDS)}


def test_cut_windows():
    assert RD.cut_windows(0, 10, 4) == [(0, 0)] and RD.cut_windows(10, 10, 4) == [(0, 10)]
    assert RD.cut_windows(11, 10, 4) == [(0, 10), (6, 5)]
    assert RD.cut_windows(25, 10, 4) == [(0, 10), (6, 10), (12, 10), (18, 7)]
    assert RD.cut_windows(20, 4, 128) == [(2 * i, 4) for i in range(9)]         # overlap capped at half a window
    for n, w, s in ((1300, 500, 128), (513, 505, 128), (37, 5, 0), (100, 7, 3)):
        cuts = RD.cut_windows(n, w, s)
        seen = set()
        for a, k in cuts:
            assert 1 <= k <= w
            seen.update(range(a, a + k))
        assert seen == set(range(n)) and cuts[-1][0] + cuts[-1][1] == n
    assert RD.chunk_rows([5, 5, 5, 20, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 5)] and RD.chunk_rows([], 10) == []


def test_windows_map_spans_to_characters_and_merge():
    tk = WordPieceTokenizer(VOCAB)
    g = np.random.default_rng(4)
    body = [str(w) for w in g.choice(WORDS[:4], 1300)]
    body[800:803] = ["paris", ",", "france"]                    # tokens 800..802
    long_text = "  ".join(body)                                # two spaces: characters are not 6 per token
    short = "the capital of france is paris."
    question = "the capital of france"
    rows, spans = RD.plan_rows(tk, [question, question], [long_text, short], 512, 128, 64)
    mine = [r for r in rows if r["passage"] == 0]
    assert len(mine) >= 3 and len(rows) == len(mine) + 1 and len(spans[0]) == 1300
    q_len = 4
    for r in rows:
        assert len(r["ids"]) <= 512 and len(r["ids"]) == len(r["type_ids"]) == r["ctx_start"] + r["ctx_len"] + 1
        assert r["ids"][0] == VOCAB["[CLS]"] and r["ids"][-1] == r["ids"][q_len + 1] == VOCAB["[SEP]"]
        assert r["ctx_start"] == q_len + 2 and r["type_ids"] == [0] * (q_len + 2) + [1] * (r["ctx_len"] + 1)
    assert [r["offset"] for r in mine][:3] == [0, 505 - 128, 2 * (505 - 128)]
    # windows 1 and 2 both hold tokens 800..802; fake the kernel: window 1 finds "paris , france" (score 5) and
    # something else, window 2 finds the same span with a higher score and "paris" alone, which overlaps it
    n = 3
    span = np.full((len(rows), n, 2), -1, np.int32)
    score = np.full((len(rows), n), -np.inf, np.float32)
    null = np.arange(len(rows), dtype=np.float32) + 1.0
    null[2] = -3.0
    lse = np.full((len(rows), 2), 4.0, np.float32)
    at = lambda r, tok: tok - rows[r]["offset"] + rows[r]["ctx_start"]  # noqa: E731
    assert rows[1]["offset"] <= 800 and rows[2]["offset"] <= 800 < rows[1]["offset"] + rows[1]["ctx_len"]
    span[1, 0], score[1, 0] = (at(1, 800), at(1, 802)), 5.0
    span[1, 1], score[1, 1] = (at(1, 400), at(1, 401)), 2.0
    span[2, 0], score[2, 0] = (at(2, 800), at(2, 802)), 6.0
    span[2, 1], score[2, 1] = (at(2, 800), at(2, 800)), 5.5
    span[2, 2], score[2, 2] = (at(2, 900), at(2, 900)), 1.0
    last = len(rows) - 1
    span[last, 0], score[last, 0] = (rows[last]["ctx_start"] + 5, rows[last]["ctx_start"] + 5), 7.0
    out = RD.assemble([long_text, short], rows, spans, span, score, null, lse, n)
    got = out[0]["spans"]
    assert [s["text"] for s in got[:1]] == ["paris  ,  france"] and got[0]["score"] == 6.0       # merged: the higher
    assert all(s["text"] == long_text[s["start"]: s["end"]] for s in got)
    assert [s["score"] for s in got] == [6.0, 2.0, 1.0]                                          # 5.5 overlaps the best
    assert got[1]["text"] == "  ".join(body[400:402]) and got[2]["text"] == body[900]
    assert got[0]["probability"] == pytest.approx(math.exp(6.0 - 8.0)) and out[0]["null_score"] == -3.0
    assert out[1]["spans"] == [{"text": "paris", "start": short.index("paris"), "end": short.index("paris") + 5,
                                "score": 7.0, "probability": pytest.approx(math.exp(-1.0))}]
    assert out[1]["null_score"] == float(null[last])
    # a truncated question, an empty passage
    rows, spans = RD.plan_rows(tk, ["alpha " * 100, "beta"], ["gamma delta", ""], 64, 16, 10)
    assert rows[0]["ctx_start"] == 12 and rows[1]["ctx_len"] == 0 and rows[1]["ids"] == [2, VOCAB["beta"], 3, 3]
    with pytest.raises(ValueError):
        RD.plan_rows(tk, ["a"], ["b", "c"], 64, 16, 10)


# ---------------------------------------------------------------- answerable
def test_answerable_and_merged_answers():
    read = [{"spans": [{"text": "Paris", "start": 3, "end": 8, "score": 4.0, "probability": 0.5},
                       {"text": "France", "start": 12, "end": 18, "score": 1.0, "probability": 0.1}], "null_score": 2.5},
            {"spans": [{"text": "Paris", "start": 0, "end": 5, "score": 6.0, "probability": 0.7}], "null_score": 3.5},
            {"spans": [], "null_score": 9.0}]
    out = RD.best_answers(read, [0, 1, 1], 3, 0.0)
    assert [(a["text"], a["score"], a["hit"], a["passage"], a["start"], a["end"]) for a in out["answers"]] == \
        [("Paris", 6.0, 1, 1, 0, 5), ("France", 1.0, 0, 0, 12, 18)]
    assert out["null_score"] == 2.5 and out["answerable"] is True            # 6.0 - 2.5 > 0
    assert RD.best_answers(read, [0, 1, 1], 3, 3.5)["answerable"] is False   # 3.5 > 3.5 is false
    assert RD.best_answers(read, [0, 1, 1], 3, 3.4)["answerable"] is True
    assert len(RD.best_answers(read, [0, 1, 1], 1, 0.0)["answers"]) == 1
    none = RD.best_answers([{"spans": [], "null_score": 1.0}], [0], 3, -100.0)
    assert none == {"answers": [], "answerable": False, "null_score": 1.0}


# ---------------------------------------------------------------- checkpoints
def test_from_local_dir_refuses_other_heads_and_fp32(tmp_path):
    cfg = {"architectures": ["BertForSequenceClassification"], "model_type": "bert", "vocab_size": 100,
           "hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 4, "intermediate_size": 256,
           "max_position_embeddings": 64}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="BertForQuestionAnswering"):
        RD.DeviceReader.from_local_dir(str(tmp_path))
    for change in ({"model_type": "roberta"}, {"hidden_act": "gelu_new"}, {"position_embedding_type": "relative_key"}):
        (tmp_path / "config.json").write_text(json.dumps({**cfg, "architectures": ["BertForQuestionAnswering"], **change}))
        with pytest.raises(ValueError):
            RD.DeviceReader.from_local_dir(str(tmp_path))
    (tmp_path / "config.json").write_text(json.dumps({**cfg, "architectures": ["BertForQuestionAnswering"]}))
    with pytest.raises(ValueError, match="fp16 is the only"):
        RD.DeviceReader.from_local_dir(str(tmp_path), precision="fp32")


# ---------------------------------------------------------------- EmbeddingManager and POST /query with a fake reader
class FakeReader:
    """finds the word "zebra" (score 5, or 9 in a text that shouts it) and the first word (score 1) of every passage"""

    def __init__(self):
        self.calls = []

    def read(self, question, passages, n_best=3, max_answer_tokens=30, doc_stride=128, max_query_tokens=64):
        self.calls.append((list(question), list(passages), n_best, max_answer_tokens, doc_stride))
        out = []
        for text in passages:
            spans = []
            at = text.lower().find("zebra")
            if at >= 0:
                loud = text[at: at + 5] == "ZEBRA"
                spans.append({"text": text[at: at + 5], "start": at, "end": at + 5, "score": 9.0 if loud else 5.0,
                              "probability": 0.9 if loud else 0.5})
            first = text.split()[0] if text.split() else ""
            if first:
                spans.append({"text": first, "start": text.index(first), "end": text.index(first) + len(first),
                              "score": 1.0, "probability": 0.1})
            out.append({"spans": spans[:n_best], "null_score": 2.0 if at >= 0 else 8.0})
        return out


def results(docs):
    n = len(docs)
    return {"ids": [f"id{i}" for i in range(n)], "distances": [0.1 * i for i in range(n)],
            "metadatas": [{"i": i} for i in range(n)], "documents": list(docs)}


def test_read_answers_with_a_fake_reader(monkeypatch):
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_DIR", "")
    m = EmbeddingManager(engine=FakeEngine())
    assert not m.has_reader()
    with pytest.raises(ValueError, match="MMRAG_READER_DIR"):
        asyncio.run(m.read_answers("q", results(["a"])))
    m._reader = FakeReader()
    assert m.has_reader()
    res = results(["the zebra crossing", None, "a ZEBRA here", "nothing striped"])
    out = asyncio.run(m.read_answers("which animal", res, n_answers=3))
    assert {k: out[k] for k in res} == res
    assert [(a["text"], a["hit"], a["score"]) for a in out["answers"]] == [("ZEBRA", 2, 9.0), ("zebra", 0, 5.0),
                                                                           ("the", 0, 1.0)]
    assert out["answerable"] is True and out["null_score"] == 2.0
    assert [len(s) for s in out["answer_spans"]] == [2, 0, 2, 1]
    assert m._reader.calls[-1] == (["which animal"] * 4, ["the zebra crossing", "", "a ZEBRA here", "nothing striped"],
                                   3, 30, 128)
    # the threshold: 9 - 2 = 7
    assert asyncio.run(m.read_answers("q", res, null_threshold=7.0))["answerable"] is False
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_NULL_THRESHOLD", 6.5)
    assert asyncio.run(m.read_answers("q", res))["answerable"] is True
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_NULL_THRESHOLD", 1e9)
    assert asyncio.run(m.read_answers("q", res))["answerable"] is False
    # raw texts with owners; two questions in ONE read call
    calls = len(m._reader.calls)
    both = asyncio.run(m.batch_read_answers(["q0", "q1"], [results(["x", "y"]), results(["z"])],
                                            texts_list=[["no stripes", "a zebra", "zebra again"], None],
                                            owners_list=[[0, 1, 1], None]))
    assert len(m._reader.calls) == calls + 1 and m._reader.calls[-1][0] == ["q0"] * 3 + ["q1"]
    assert [(a["text"], a["hit"], a["passage"]) for a in both[0]["answers"]] == [("zebra", 1, 1), ("no", 0, 0), ("a", 1, 1)]
    assert [len(s) for s in both[0]["answer_spans"]] == [1, 4] and both[1]["answers"][0]["text"] == "z"
    empty = asyncio.run(m.read_answers("q", results([])))
    assert empty["answers"] == [] and empty["answerable"] is False and empty["null_score"] is None


def test_reader_loads_once_from_configured_dir(monkeypatch):
    loads = []

    class Fake:
        @classmethod
        def from_local_dir(cls, path, device="cuda:0", **kw):
            loads.append((path, device))
            return FakeReader()

    monkeypatch.setattr(RD, "DeviceReader", Fake)
    monkeypatch.setattr(emb_mod.settings, "MMRAG_READER_DIR", "/models/qa")
    m = EmbeddingManager(engine=FakeEngine())
    assert m.has_reader()
    for _ in range(3):
        assert asyncio.run(m.read_answers("q", results(["a zebra"])))["answers"][0]["text"] == "zebra"
    assert len(loads) == 1 and loads[0][0] == "/models/qa"


def test_query_reader_flags(monkeypatch):
    from multimodal_rag_amd import server

    monkeypatch.setattr(server.settings, "MMRAG_READER_DIR", "")
    m = EmbeddingManager(engine=FakeEngine())
    bodies = ["The zebra crossing is on Main Street. " * 3, "Nothing striped lives here. " * 3]
    with TestClient(create_app(embedder=m)) as c:
        for i, body in enumerate(bodies):
            assert c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")}).status_code == 200
        plain = c.post("/query", json={"query": "which animal", "top_k": 2}).json()
        assert set(plain) == {"answer", "sources", "processing_time"}
        assert c.post("/query", json={"query": "which animal", "top_k": 2, "reader": False}).json()["sources"] == \
            plain["sources"]
        for flag in ("reader", "reader_answer"):                 # no reader configured: 400 with a plain message
            r = c.post("/query", json={"query": "which animal", "top_k": 2, flag: True})
            assert r.status_code == 400 and "MMRAG_READER_DIR" in r.json()["detail"]
        assert c.post("/query", json={"query": "q", "reader": "yes please"}).status_code == 422
        m._reader = FakeReader()
        on = c.post("/query", json={"query": "which animal", "top_k": 2, "reader": True})
        assert on.status_code == 200, on.text
        on = on.json()
        assert set(on) == {"answer", "sources", "processing_time", "answers", "answerable"}
        assert on["answer"] == plain["answer"]                   # the generator's answer, unchanged
        assert [{k: v for k, v in s.items() if k != "answer_spans"} for s in on["sources"]] == plain["sources"]
        assert on["answerable"] is True and on["answers"][0]["text"] == "zebra" and on["answers"][0]["score"] == 5.0
        assert set(on["answers"][0]) == {"text", "score", "probability", "hit", "passage", "start", "end"}
        zebra_hit = on["answers"][0]["hit"]
        assert plain["sources"][zebra_hit]["doc_id"] == on["sources"][zebra_hit]["doc_id"]
        assert on["sources"][zebra_hit]["answer_spans"][0]["text"] == "zebra"
        assert all("answer_spans" in s for s in on["sources"])
        assert m._reader.calls[-1][0] == ["which animal"] * len(m._reader.calls[-1][1])
        # reader_answer implies reader: the best span is the answer, no generator call
        ans = c.post("/query", json={"query": "which animal", "top_k": 2, "reader_answer": True}).json()
        assert ans["answer"] == "zebra" and ans["answerable"] is True and ans["answers"] == on["answers"]
        monkeypatch.setattr(server.settings, "MMRAG_READER_NULL_THRESHOLD", 1e9)
        ans = c.post("/query", json={"query": "which animal", "top_k": 2, "reader_answer": True}).json()
        assert ans["answer"] == NO_ANSWER_FOUND and ans["answerable"] is False and ans["answers"][0]["text"] == "zebra"
        # refused the way `passages` is refused with learned sparse retrieval
        with_passages = c.post("/query", json={"query": "q", "sparse": True, "passages": True})
        for flag in ("reader", "reader_answer"):
            r = c.post("/query", json={"query": "q", "sparse": True, flag: True})
            assert r.status_code == 400 and r.json()["detail"] == with_passages.json()["detail"]
        r = c.post("/query", json={"query": "q", "reader_answer": True, "extractive_answer": True})
        assert r.status_code == 400
