"""CPU: extractive summaries -- the sentence splitter's known answers, the invariants of the float64 reference
(tests/summary_ref.py), the header constant, and the server / settings wiring over a fake embedder."""
import asyncio
import os
import re

import numpy as np
import pytest
from starlette.testclient import TestClient

from multimodal_rag_amd import _native, config
from multimodal_rag_amd import summarize as SM
from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.ingest import PassthroughSummarizer, fallback_summary
from multimodal_rag_amd.server import EXTRACT_NEEDS, create_app
from tests import summary_ref as R
from tests.fakes import FakeEngine


def pieces(text, max_chars=None):
    return [text[a:b] for a, b in SM.split_sentences(text, max_chars)]


# ---------------------------------------------------------------- the splitter
def test_splitter_on_the_vietnamese_sample(golden_dir):
    text = open(os.path.join(golden_dir, "sample_document.txt"), encoding="utf-8").read()
    got = pieces(text)
    # blank lines end a span; "1." "2." "3." are enumerators, not ends; the list lines carry no punctuation, so each
    # list is one span (single line breaks do not end a sentence)
    assert got == [
        "# Giới Thiệu về Machine Learning",
        "Machine Learning (Học máy) là một nhánh của trí tuệ nhân tạo cho phép máy tính học từ dữ liệu mà không cần "
        "lập trình cụ thể.",
        "## Các Loại Machine Learning",
        "1. **Supervised Learning** (Học có giám sát): Học từ dữ liệu có nhãn\n"
        "2. **Unsupervised Learning** (Học không giám sát): Tìm patterns trong dữ liệu không có nhãn\n"
        "3. **Reinforcement Learning** (Học tăng cường): Học thông qua thử và sai",
        "## Ứng Dụng",
        "- Y tế: Chẩn đoán bệnh, dự đoán\n- Tài chính: Phát hiện gian lận\n- Giao thông: Xe tự lái\n"
        "- Thương mại điện tử: Hệ thống gợi ý"]
    spans = SM.split_sentences(text)
    assert spans == sorted(spans) and all(b <= a2 for (_, b), (a2, _) in zip(spans, spans[1:]))
    # with a limit every span fits and is cut at whitespace
    for a, b in SM.split_sentences(text, 60):
        assert 0 < b - a <= 60 and text[a:b] == text[a:b].strip()
        assert b == len(text) or text[b].isspace() or text[b - 1] in ".?!…"


def test_splitter_rules():
    assert pieces("Xin chào. Đây là câu thứ hai? Vâng!  Số 3.14 không bị cắt… Hết") == [
        "Xin chào.", "Đây là câu thứ hai?", "Vâng!", "Số 3.14 không bị cắt…", "Hết"]
    # abbreviations are not special-cased: a terminator followed by whitespace ends a sentence, whatever precedes it
    assert pieces("We saw Dr. Smith, e.g. at noon.") == ["We saw Dr.", "Smith, e.g.", "at noon."]
    # ... except after a word of digits only that begins a span or a line (an enumerator); dotted names and decimals
    # have no whitespace after the dot
    assert pieces("1. First item. 2. Second item\n 3. Third") == ["1. First item.", "2. Second item\n 3. Third"]
    assert pieces("Built in 1999. Sold for 5. Gone") == ["Built in 1999.", "Sold for 5.", "Gone"]
    assert pieces("See www.example.com now?! Yes... maybe.") == ["See www.example.com now?!", "Yes...", "maybe."]
    assert pieces("one\n\n\ntwo\n \nthree\nfour") == ["one", "two", "three\nfour"]
    assert pieces("") == [] and pieces("  \n\t ") == [] and pieces("...") == ["..."] and pieces(None) == []


def test_over_long_spans_are_cut_at_whitespace():
    assert pieces("aaa bbb ccc ddd eee fff", 8) == ["aaa bbb", "ccc ddd", "eee fff"]
    assert pieces("abcdefghijkl", 5) == ["abcde", "fghij", "kl"]           # no whitespace: cut at the limit
    text = "word " * 30 + "end. Next one."
    got = SM.split_sentences(text, 40)
    assert all(b - a <= 40 for a, b in got) and [text[a:b] for a, b in got][-1] == "Next one."
    assert " ".join(text[a:b] for a, b in got) == " ".join(text.split())    # nothing lost, nothing twice
    lines = "a | b\n\n  c | d  \nlong line " + "x" * 30
    assert [lines[a:b] for a, b in SM.split_lines(lines, 20)] == ["a | b", "c | d", "long line", "x" * 20, "x" * 10]


# ---------------------------------------------------------------- the reference's invariants
def unit_rows(rng, n, d=24):
    x = rng.standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize("n", (1, 2, 7, 40, 128))
def test_reference_never_exceeds_the_budget(n):
    rng = np.random.default_rng(n)
    X, cost = unit_rows(rng, n), rng.integers(1, 30, n)
    for budget in (0, 1, 29, 100):
        rel, pos, val, used = R.summarize(X, cost, budget, 16, 0.1, 0.15, 32, 0.7)
        assert used == cost[pos].sum() <= budget and len(set(pos)) == len(pos) <= 16
        assert rel.max() == 1.0 and (rel > 0).all()
        left = budget - used
        if len(pos) < 16:
            assert all(cost[i] > left for i in range(n) if i not in pos)


def test_reference_lambda_one_picks_by_rel_alone():
    rng = np.random.default_rng(11)
    X = unit_rows(rng, 30)
    rel, pos, val, _ = R.summarize(X, np.ones(30, int), 1000, 10, 0.0, 0.15, 32, 1.0)
    assert pos == list(np.argsort(-rel, kind="stable")[:10]) and np.allclose(val, rel[pos])


def test_reference_without_iterations_rel_is_the_prior():
    rng = np.random.default_rng(12)
    X, q = unit_rows(rng, 20), unit_rows(rng, 1)[0]
    S, s = R.similarities(X, q)
    assert np.array_equal(R.centrality(S, None, 0.1, 0.15, 0), np.ones(20))
    b = R.prior(20, s)
    assert np.allclose(R.centrality(S, s, 0.1, 0.15, 0), b / b.max()) and (b >= 0).all() and np.isclose(b.sum(), 1.0)
    assert np.array_equal(R.prior(3, np.array([-1.0, 0.0, -2.0])), np.full(3, 1 / 3))      # no positive mass: uniform


def test_reference_picks_a_duplicated_sentence_once():
    # ten sentences that share one direction (every cosine 0.2) and sentence 7 repeating sentence 2 (cosine 1): the
    # pair is the most central, so one of them is picked first; its twin then carries the full redundancy penalty and
    # waits until every other sentence is gone
    X = np.eye(10, 11)
    X[:, 10] = 0.5
    X[7] = X[2]
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    rel, pos, _, _ = R.summarize(X, np.ones(10, int), 1000, 9, 0.1, 0.15, 32, 0.7)
    assert pos[0] == 2 and 7 not in pos and len(pos) == 9
    assert R.summarize(X, np.ones(10, int), 1000, 10, 0.1, 0.15, 32, 0.7)[1][-1] == 7
    # ... while rel alone (lambda = 1) takes both at once
    rel1, pos1, _, _ = R.summarize(X, np.ones(10, int), 1000, 10, 0.1, 0.15, 32, 1.0)
    assert pos1[:2] == [2, 7] and rel1[2] == rel1[7] == 1.0


def test_reference_single_sentence():
    x = np.array([[0.6, 0.8]])
    assert R.summarize(x, [5], 5, 3, 0.1, 0.15, 32, 0.7)[1:] == ([0], [float(np.float32(0.7))], 5)
    assert R.summarize(x, [5], 4, 3, 0.1, 0.15, 32, 0.7)[1:] == ([], [], 0)
    assert np.array_equal(R.summarize(x, [5], 4, 3, 0.1, 0.15, 32, 0.7, q=np.array([-1.0, 0.0]))[0], [1.0])


# ---------------------------------------------------------------- header and binding
def test_header_constant_equals_the_binding():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mmrag.h"), encoding="utf-8").read()
    assert "#define MMRAG_MAX_SUMMARY_SENTENCES 128" in header
    found = re.search(r"#define MMRAG_MAX_SUMMARY_ITERATIONS (\d+)", header)
    assert _native.MAX_SUMMARY_SENTENCES == 128 and int(found.group(1)) == _native.MAX_SUMMARY_ITERATIONS
    assert "int mmrag_summary_select(" in header
    assert "summarize.hip" in __import__("multimodal_rag_amd.build", fromlist=["SOURCES"]).SOURCES


def test_summary_select_refuses_host_tensors():
    import torch

    rows = torch.zeros((4, 64), dtype=torch.float16)
    table = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_native.MMRagNativeError, match="device"):
        _native.summary_select(rows, 64, table, table, torch.ones(4, dtype=torch.int32), table, 1, 0.1, 0.15, 32, 0.7)


# ---------------------------------------------------------------- settings
def test_summarizer_setting_is_checked(monkeypatch):
    assert config.settings.summarizer() == "fallback" and config.Settings().MMRAG_SUMMARY_ITERATIONS == 32
    assert (config.Settings().MMRAG_SUMMARY_EDGE_THRESHOLD, config.Settings().MMRAG_SUMMARY_ALPHA,
            config.Settings().MMRAG_SUMMARY_LAMBDA) == (0.1, 0.15, 0.7)
    monkeypatch.setenv("MMRAG_SUMMARIZER", "abstractive")
    with pytest.raises(ValueError, match="MMRAG_SUMMARIZER"):
        config.Settings()
    monkeypatch.setenv("MMRAG_SUMMARIZER", "extractive")
    assert config.Settings().summarizer() == "extractive"
    monkeypatch.setattr(config.settings, "MMRAG_SUMMARIZER", "nonsense")
    with pytest.raises(ValueError):
        config.settings.summarizer()
    monkeypatch.setattr(config.settings, "MMRAG_SUMMARY_ALPHA", 0.0)
    with pytest.raises(ValueError, match="MMRAG_SUMMARY_ALPHA"):
        SM.summary_parameters()


# ---------------------------------------------------------------- the summariser stage and the server
class SummarizingManager(EmbeddingManager):
    """an embedder whose summaries and answers are recognisable: the LAST 50 characters of a text, the first 12
    characters of every passage"""

    calls = None

    def supports_summaries(self):
        return True

    async def summarize_texts(self, texts, max_length=300, by_lines=False, questions=None):
        self.calls = (self.calls or []) + [("summarize", len(texts), max_length, by_lines)]
        return [{"summary": ("ROWS " if by_lines else "TAIL ") + t[-50:].strip(), "spans": [(max(len(t) - 50, 0), len(t))],
                 "scores": [1.0]} for t in texts]

    async def extract_answer(self, question, passages, max_chars=600, top_sentences=8):
        quotes = [{"passage": i, "start": 0, "end": min(12, len(p)), "text": p[:12], "score": 1.0 / (i + 1)}
                  for i, p in enumerate(passages)]
        return {"answer": " ".join(q["text"] for q in quotes), "quotes": quotes, "considered": len(quotes)}


def test_extractive_summarizer_keeps_the_stage_contract():
    tree = {"text_chunks": [{"content": "alpha " * 80, "metadata": {"page": 1}}, {"content": "short"}],
            "tables": [{"id": "table_3", "content": "a | b\nc | d"}, {"content": "x"}],
            "images": [{"id": "image_1", "description": "a chart", "base64": "QUJD", "path": "/p.png"}, {}]}
    fake = SummarizingManager(engine=FakeEngine())
    ours = SM.ExtractiveSummarizer(lambda: fake)           # resolved at the first document
    got = asyncio.run(ours.summarize_parsed_document(tree, max_length=120))
    want = asyncio.run(PassthroughSummarizer().summarize_parsed_document(tree, max_length=120))
    assert [(g["id"], g["type"], sorted(g)) for g in got] == [(w["id"], w["type"], sorted(w)) for w in want]
    assert [g["raw"] for g in got] == [w["raw"] for w in want] and got[4:] == want[4:]       # images: unchanged
    assert got[0]["summary"].startswith("TAIL ") and got[2]["summary"] == "ROWS a | b\nc | d"
    assert fake.calls == [("summarize", 2, 120, False), ("summarize", 2, 120, True)]
    assert asyncio.run(ours.get_stats()) == {"total_summaries": 6, "cache": {"hit_rate": 0}}
    assert asyncio.run(SM.ExtractiveSummarizer(fake).summarize_parsed_document({})) == []


def chunk_text():
    head = "The opening sentence says little. " * 12
    return head + "Only the end of this chunk names the zebra crossing."


def test_upload_embeds_the_extractive_summaries(monkeypatch):
    text = chunk_text()
    assert 300 < len(text) <= 1000
    stored = {}
    for setting in ("extractive", "fallback"):
        monkeypatch.setattr(config.settings, "MMRAG_SUMMARIZER", setting)
        manager = SummarizingManager(engine=FakeEngine())
        with TestClient(create_app(embedder=manager)) as client:
            up = client.post("/upload", files={"file": ("zebra.txt", text.encode("utf-8"), "text/plain")})
            assert up.status_code == 200, up.text
            assert set(up.json()) == {"doc_id", "filename", "doc_type", "chunks_processed", "message", "processing_time"}
            stored[setting] = manager.collection.get(where={"doc_id": up.json()["doc_id"]})["documents"]
            assert client.get("/stats").status_code == 200
    assert stored["extractive"] == ["TAIL " + text[-50:].strip()] and "zebra" in stored["extractive"][0]
    assert stored["fallback"] == [fallback_summary(text, 300)] and "zebra" not in stored["fallback"][0]


def test_query_with_an_extractive_answer_carries_quotes(monkeypatch):
    text = chunk_text()
    manager = SummarizingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=manager)) as client:
        for name in ("a.txt", "b.txt"):
            assert client.post("/upload", files={"file": (name, text.encode("utf-8"), "text/plain")}).status_code == 200
        plain = client.post("/query", json={"query": "zebra", "top_k": 2}).json()
        off = client.post("/query", json={"query": "zebra", "top_k": 2, "extractive_answer": False}).json()
        on = client.post("/query", json={"query": "zebra", "top_k": 2, "extractive_answer": True}).json()
    # without the field: the generator's answer over the raw chunks and the four columns of a source, nothing else
    assert set(plain) == {"answer", "sources", "processing_time"}
    assert plain["answer"] == "\n\n".join([text, text]) and plain["answer"] == off["answer"]
    assert all(set(s) == {"rank", "doc_id", "relevance_score", "type"} for s in plain["sources"])
    assert plain["sources"] == off["sources"]
    # with it: the embedder's extract, and its quotes on the sources they come from
    assert on["answer"] == " ".join([text[:12]] * 2)
    assert [{k: v for k, v in s.items() if k != "quotes"} for s in on["sources"]] == plain["sources"]
    assert [s["quotes"] for s in on["sources"]] == [[{"start": 0, "end": 12, "text": text[:12], "score": 1.0}],
                                                   [{"start": 0, "end": 12, "text": text[:12], "score": 0.5}]]


def test_an_embedder_without_extractive_answers_gets_a_400():
    with TestClient(create_app(embedder=EmbeddingManager(engine=FakeEngine()))) as client:
        r = client.post("/query", json={"query": "zebra", "extractive_answer": True})
        assert r.status_code == 400 and r.json()["detail"] == EXTRACT_NEEDS[2]
        assert client.post("/query", json={"query": "zebra", "extractive_answer": "yes please"}).status_code == 422
        assert client.post("/query", json={"query": "zebra"}).status_code == 200
    manager = EmbeddingManager(engine=FakeEngine())
    assert not manager.supports_summaries()
    with pytest.raises(ValueError, match="encode_device"):
        asyncio.run(manager.summarize_texts(["x" * 400]))
