"""CPU: answer citations -- the invariants of the float64 reference (tests/attribution_ref.py), the header constants, the
host layer of attribution.py over an attributor whose device part is the reference, the settings, and the server wiring
(POST /query "citations", POST /attribute) over a fake embedder."""
import asyncio
import os
import re

import numpy as np
import pytest
from starlette.testclient import TestClient

from multimodal_rag_amd import _native, config
from multimodal_rag_amd import attribution as AT
from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.server import CITATION_NEEDS, create_app
from multimodal_rag_amd.summarize import split_sentences
from tests import attribution_ref as R
from tests.fakes import FakeEngine


# ---------------------------------------------------------------- the reference's invariants
def unit_rows(rng, n, d=24):
    x = rng.standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_reference_small_known_answer():
    X = np.array([[1.0, 0.0], [0.0, 1.0]])
    E = np.array([[0.5, 0.0], [1.0, 0.0], [0.0, 0.25], [1.0, 0.0], [0.0, -1.0]])
    src, ev, score, M = R.attribute(X, E, [2, 0, 2, 0, 7], 4, 3)
    assert M.tolist() == [[1.0, -np.inf, 0.5, -np.inf], [0.0, -np.inf, 0.25, -np.inf]]
    # claim 0: source 0 by rows 1 and 3 (the lowest j), then source 2; claim 1: source 2, then source 0 (row 1 of 0, 0)
    assert src.tolist() == [[0, 2, -1], [2, 0, -1]] and ev.tolist() == [[1, 0, -1], [2, 1, -1]]
    assert score.tolist() == [[1.0, 0.5, -np.inf], [0.25, 0.0, -np.inf]]
    # no evidence at all: every entry is padding
    src, ev, score, M = R.attribute(X, np.zeros((0, 2)), [], 2, 2)
    assert np.all(src == -1) and np.all(ev == -1) and np.all(np.isneginf(score)) and np.all(np.isneginf(M))


def test_reference_permuting_the_evidence_changes_only_j():
    rng = np.random.default_rng(1)
    X, E, sources = unit_rows(rng, 9), unit_rows(rng, 50), rng.integers(-1, 7, 50)
    src, ev, score, M = R.attribute(X, E, sources, 6, 4)
    perm = rng.permutation(50)                         # new row t holds old row perm[t]
    src2, ev2, score2, M2 = R.attribute(X, E[perm], sources[perm], 6, 4)
    assert np.array_equal(src2, src) and np.array_equal(score2, score) and np.array_equal(M2, M)
    assert np.array_equal(np.where(ev2 >= 0, perm[ev2], -1), ev) and not np.array_equal(ev2, ev)


def test_reference_relabelling_the_sources_permutes_the_output():
    rng = np.random.default_rng(2)
    X, E, sources = unit_rows(rng, 9), unit_rows(rng, 50), rng.integers(0, 6, 50)
    src, ev, score, M = R.attribute(X, E, sources, 6, 6)
    label = rng.permutation(6)                         # source s is now called label[s]
    src2, ev2, score2, M2 = R.attribute(X, E, label[sources], 6, 6)
    assert np.array_equal(src2, label[src]) and np.array_equal(ev2, ev) and np.array_equal(score2, score)
    assert np.array_equal(M2[:, label], M)


def test_reference_ties():
    rng = np.random.default_rng(3)
    X, E = unit_rows(rng, 5), unit_rows(rng, 12)
    E[9] = E[4]                                        # one sentence in two sources: the lower ordinal comes first
    sources = np.array([3, 3, 3, 3, 5, 5, 5, 5, 2, 2, 2, 2])
    src, ev, score, M = R.attribute(X, E, sources, 6, 3)
    for i in range(5):
        if M[i, 2] == M[i, 5]:                         # the duplicate is the best of both: 2 before 5, at equal scores
            order = src[i].tolist()
            assert order.index(2) + 1 == order.index(5) and score[i, order.index(2)] == score[i, order.index(5)]
    twin = np.argmax(X @ E[4])                         # make it the best of both for one claim at least
    X[twin] = E[4]
    src, ev, score, _ = R.attribute(X, E, sources, 6, 3)
    assert src[twin, :2].tolist() == [2, 5] and ev[twin, :2].tolist() == [9, 4] and score[twin, 0] == score[twin, 1]
    E[6] = E[4]                                        # ... and twice inside source 5: the lowest j
    assert R.attribute(X, E, sources, 6, 3)[1][twin, :2].tolist() == [9, 4]


def test_reference_m_above_the_sources_and_ordinals_out_of_range():
    rng = np.random.default_rng(4)
    X, E = unit_rows(rng, 3), unit_rows(rng, 20)
    sources = np.array([0, 64, -1, 1, 1000] * 4)
    src, ev, score, M = R.attribute(X, E, sources, 2, 8)
    assert np.all((src[:, :2] >= 0)) and np.all(src[:, 2:] == -1) and np.all(np.isneginf(score[:, 2:]))
    assert set(ev[:, :2].ravel()) <= {0, 3, 5, 8, 10, 13, 15, 18}
    got, left = R.margins((X @ E.T)[0], sources, 2, src[0], ev[0])
    assert left == 0 and len(got) == 2 and all(mine for *_, mine in got)
    assert got[0][0] == got[0][1] == got[0][2] == score[0, 0] and got[0][4] == src[0, 0]
    assert got[0][3] == score[0, 0] - score[0, 1] and got[1][3] == float("inf")


# ---------------------------------------------------------------- header and binding
def test_header_constants_equal_the_binding():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mmrag.h"), encoding="utf-8").read()
    for name, value in (("MMRAG_MAX_CLAIMS", _native.MAX_CLAIMS), ("MMRAG_MAX_EVIDENCE", _native.MAX_EVIDENCE),
                        ("MMRAG_MAX_ATTR_SOURCES", _native.MAX_ATTR_SOURCES),
                        ("MMRAG_MAX_CITATIONS", _native.MAX_CITATIONS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    assert (_native.MAX_CLAIMS, _native.MAX_EVIDENCE, _native.MAX_ATTR_SOURCES, _native.MAX_CITATIONS) == \
        (128, 4096, 64, 8)
    assert "int mmrag_attribute(" in header and "not entailment" in header
    for promise in ("no workspace", "no host synchronisation", "captured into a graph", "do not depend on the batch"):
        assert promise in header[header.index("csrc/attribute.hip"): header.index("int mmrag_attribute(")]
    assert "attribute.hip" in __import__("multimodal_rag_amd.build", fromlist=["SOURCES"]).SOURCES


def test_attribute_refuses_host_tensors():
    import torch

    rows = torch.zeros((4, 64), dtype=torch.float16)
    table = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_native.MMRagNativeError, match="device"):
        _native.attribute(rows, 64, table, table, table, table, torch.zeros(4, dtype=torch.int32), 2, 1, 4)


# ---------------------------------------------------------------- the host side
def embed(texts, words):
    """bags of words as unit vectors over the vocabulary `words` (a dict that grows): identical sentences have cosine
    1, sentences without a common word 0"""
    bags = [re.findall(r"\w+", text.lower()) for text in texts]
    for bag in bags:
        for word in bag:
            words.setdefault(word, len(words))
    out = np.zeros((len(texts), len(words)))
    for row, bag in zip(out, bags):
        for word in bag:
            row[words[word]] += 1.0
    return out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-30)


class RefAttributor(AT.DeviceAttributor):
    """an attributor whose device part is the float64 reference over bag-of-words vectors"""

    def __init__(self):
        self.calls = []

    def rank(self, sections, evidence, n_sources, m):
        self.calls.append(([len(c) for c, _ in sections], [e for _, e in sections], [len(s) for s, _ in evidence],
                           n_sources, m))
        out = []
        for claims, e in sections:
            sents, ords = evidence[e]
            words = {}
            E = embed(sents, words)
            X = embed(claims, words)
            E = np.pad(E, ((0, 0), (0, X.shape[1] - E.shape[1])))
            src, ev, score, _ = R.attribute(X, E, ords, n_sources, m)
            out.append([[(int(s), int(j), float(v)) for s, j, v in zip(src[i], ev[i], score[i]) if s >= 0]
                        for i in range(len(claims))])
        return out


SOLAR = "Solar panels turn sunlight into power. A panel holds many silicon cells.  Each cell frees electrons."
BREAD = "Sourdough starts from flour and water.\nThe dough proofs overnight! A hot pot gives the crust."
ALIEN = "Quarterly invoices were mailed yesterday."


def test_offsets_map_back_to_the_texts():
    worker = RefAttributor()
    answer = "  A hot pot gives the crust. Solar panels turn sunlight into power.  " + ALIEN + " The dough proofs overnight!"
    got = worker.attribute([answer], [[SOLAR, "", BREAD]], threshold=0.9, max_citations=2)[0]
    assert worker.calls == [([4], [0], [6], 3, 2)]
    assert got["considered"] == {"claims": 4, "evidence": 6}
    assert [c["text"] for c in got["citations"]] == [answer[a:b] for a, b in split_sentences(answer)]
    for c in got["citations"]:
        assert answer[c["start"]: c["end"]] == c["text"]
        for s in c["sources"]:
            text = [SOLAR, "", BREAD][s["passage"]]
            assert text[s["start"]: s["end"]] == s["text"] and s["score"] >= 0.9 and s["source"] == s["passage"]
    assert [c["supported"] for c in got["citations"]] == [True, True, False, True]
    assert [[s["source"] for s in c["sources"]] for c in got["citations"]] == [[2], [0], [], [2]]
    assert [c["sources"][0]["text"] for c in got["citations"] if c["sources"]] == \
        ["A hot pot gives the crust.", "Solar panels turn sunlight into power.", "The dough proofs overnight!"]
    assert got["citations"][0]["score"] == pytest.approx(1.0) and got["citations"][2]["score"] < 0.5
    chars = [c["end"] - c["start"] for c in got["citations"]]
    assert got["groundedness"] == pytest.approx((chars[0] + chars[1] + chars[3]) / sum(chars))
    assert got["support"] == pytest.approx([chars[1] / sum(chars), 0.0, (chars[0] + chars[3]) / sum(chars)])
    assert sum(got["support"]) == pytest.approx(got["groundedness"])
    # a low threshold lists every source with evidence, best first, at most max_citations of them
    loose = worker.attribute([answer], [[SOLAR, "", BREAD]], threshold=-0.5, max_citations=8)[0]
    assert all([s["source"] for s in c["sources"]] in ([0, 2], [2, 0]) for c in loose["citations"])
    assert all(c["sources"][0]["score"] >= c["sources"][1]["score"] for c in loose["citations"])
    assert loose["groundedness"] == 1.0
    assert all(len(c["sources"]) == 1 for c in
               worker.attribute([answer], [[SOLAR, "", BREAD]], threshold=-0.5, max_citations=1)[0]["citations"])


def test_a_long_answer_is_cut_into_sections_over_the_same_evidence():
    worker = RefAttributor()
    facts = [f"Fact number {i} is about topic {i}." for i in range(300)]
    answer = " ".join(facts[:290])
    got = worker.attribute([answer, "Fact number 7 is about topic 7."], [[" ".join(facts[:150]), " ".join(facts[150:])],
                                                                      [" ".join(facts[:10])]], threshold=0.99)
    # three sections (128 + 128 + 34 claims) share evidence set 0, which is in the call once; one launch for both answers
    assert worker.calls == [([128, 128, 34, 1], [0, 0, 0, 1], [300, 10], 2, 3)]
    assert got[0]["considered"] == {"claims": 290, "evidence": 300} and got[0]["groundedness"] == 1.0
    for i, c in enumerate(got[0]["citations"]):
        assert c["text"] == facts[i] and c["sources"][0]["text"] == facts[i]
        assert c["sources"][0]["source"] == c["sources"][0]["passage"] == (0 if i < 150 else 1)
    assert got[1]["citations"][0]["sources"][0]["text"] == facts[7] and got[1]["support"] == [1.0]


def test_the_evidence_cap_and_considered():
    worker = RefAttributor()
    passages = [" ".join(f"Item {p} {i}." for i in range(1500)) for p in range(3)]
    got = worker.attribute(["Item 0 3. Item 2 1499. Item 2 1000."], [passages], threshold=0.99)[0]
    assert worker.calls[-1][2] == [_native.MAX_EVIDENCE]
    assert got["considered"] == {"claims": 3, "evidence": 4096}
    # passage 2 takes part with its first 4096 - 3000 sentences only
    assert [c["supported"] for c in got["citations"]] == [True, False, True]
    assert got["citations"][2]["sources"][0]["passage"] == 2


def test_empty_inputs_need_no_launch():
    worker = RefAttributor()
    empty = {"citations": [], "groundedness": 0.0, "support": [0.0], "considered": {"claims": 0, "evidence": 0}}
    assert worker.attribute(["", "  \n ", "An answer.", "An answer.", None], [[SOLAR], [SOLAR], [], [" \n"], [SOLAR]],
                            threshold=0.5) == [empty] * 5
    assert worker.calls == [] and worker.attribute([], []) == []
    # ... and beside a real one they do not disturb it
    got = worker.attribute(["", "Each cell frees electrons."], [[SOLAR], [BREAD, SOLAR]], threshold=0.9)
    assert got[0] == empty and got[1]["citations"][0]["sources"][0]["passage"] == 1 and got[1]["support"] == [0.0, 1.0]
    assert worker.calls == [([1], [0], [6], 2, 3)]


def test_owners_and_the_source_limit():
    worker = RefAttributor()
    answer = "Each cell frees electrons. A hot pot gives the crust."
    got = worker.attribute([answer], [[SOLAR, BREAD, ALIEN]], owners=[[5, 1, 5]], threshold=0.9)[0]
    assert [c["sources"][0]["source"] for c in got["citations"]] == [5, 1]
    assert [c["sources"][0]["passage"] for c in got["citations"]] == [0, 1]
    assert len(got["support"]) == 6 and got["support"][5] > 0 and got["support"][1] > 0 and got["support"][0] == 0
    assert len(worker.attribute([answer], [[SOLAR]], n_sources=9, threshold=0.9)[0]["support"]) == 9
    many = [f"Passage {i} says something." for i in range(65)]
    assert worker.attribute([answer], [many[:64]], threshold=0.9)[0]["considered"]["evidence"] == 64
    with pytest.raises(ValueError, match="64 sources"):
        worker.attribute([answer], [many], threshold=0.9)
    with pytest.raises(ValueError, match="64 sources"):
        worker.attribute([answer], [[SOLAR]], owners=[[64]], threshold=0.9)
    with pytest.raises(ValueError):
        worker.attribute([answer], [[SOLAR]], owners=[[-1]], threshold=0.9)
    with pytest.raises(ValueError):
        worker.attribute([answer], [[SOLAR, BREAD]], owners=[[0]], threshold=0.9)
    with pytest.raises(ValueError):
        worker.attribute([answer], [[SOLAR, BREAD]], n_sources=1, threshold=0.9)
    with pytest.raises(ValueError):
        worker.attribute([answer], [[SOLAR]], n_sources=65)
    with pytest.raises(ValueError):
        worker.attribute([answer, answer], [[SOLAR]])
    for bad in ({"threshold": 1.5}, {"threshold": -1.0}, {"threshold": float("nan")}, {"max_citations": 0},
                {"max_citations": 9}, {"max_citations": True}):
        with pytest.raises(ValueError):
            worker.attribute([answer], [[SOLAR]], **bad)


# ---------------------------------------------------------------- settings
def test_citation_settings_are_checked(monkeypatch):
    fresh = config.Settings()
    assert (fresh.MMRAG_CITATIONS, fresh.MMRAG_CITATION_THRESHOLD, fresh.MMRAG_CITATION_MAX) == (0, 0.6, 3)
    assert fresh.citation_parameters() == {"default": False, "threshold": 0.6, "max_citations": 3}
    for name, value in (("MMRAG_CITATION_MAX", "9"), ("MMRAG_CITATION_MAX", "0"), ("MMRAG_CITATION_THRESHOLD", "1.5"),
                        ("MMRAG_CITATION_THRESHOLD", "nan"), ("MMRAG_CITATIONS", "2")):
        monkeypatch.setenv(name, value)
        with pytest.raises(ValueError, match="MMRAG_CITATION"):
            config.Settings()
        monkeypatch.delenv(name)
    monkeypatch.setenv("MMRAG_CITATIONS", "1")
    monkeypatch.setenv("MMRAG_CITATION_MAX", "8")
    assert config.Settings().citation_parameters() == {"default": True, "threshold": 0.6, "max_citations": 8}
    monkeypatch.setattr(config.settings, "MMRAG_CITATION_THRESHOLD", 0.25)
    assert AT.citation_parameters() == {"threshold": 0.25, "max_citations": 3}
    assert AT.citation_parameters(0.5, 2) == {"threshold": 0.5, "max_citations": 2}
    monkeypatch.setattr(config.settings, "MMRAG_CITATION_MAX", 12)
    with pytest.raises(ValueError, match="MMRAG_CITATION_MAX"):
        AT.citation_parameters()


# ---------------------------------------------------------------- the server
class CitingManager(EmbeddingManager):
    """an embedder that attributes through the reference and answers by quoting the first sentence of every passage"""

    def supports_summaries(self):
        return True

    def _attributor(self):
        self.attributor = RefAttributor()
        return self.attributor

    async def extract_answer(self, question, passages, max_chars=600, top_sentences=8):
        quotes = []
        for i, p in enumerate(passages):
            a, b = split_sentences(p)[0]
            quotes.append({"passage": i, "start": a, "end": b, "text": p[a:b], "score": 1.0})
        return {"answer": " ".join(q["text"] for q in quotes), "quotes": quotes, "considered": len(quotes)}


ZEBRA = ("The zebra crossing is on Main Street. It was painted in spring. " * 3).strip()
HERON = ("Herons nest in the reeds. The river floods the meadows. " * 3).strip()


def uploaded(client):
    for name, body in (("zebra.txt", ZEBRA), ("heron.txt", HERON)):
        assert client.post("/upload", files={"file": (name, body.encode("utf-8"), "text/plain")}).status_code == 200


def test_query_without_the_flag_is_what_it_was_and_with_it_carries_citations():
    manager = CitingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=manager)) as client:
        uploaded(client)
        plain = client.post("/query", json={"query": "zebra", "top_k": 2})
        off = client.post("/query", json={"query": "zebra", "top_k": 2, "citations": False})
        on = client.post("/query", json={"query": "zebra", "top_k": 2, "citations": True, "citation_threshold": 0.9,
                                         "max_citations": 2})
        assert on.status_code == 200, on.text
        plain, off, on = plain.json(), off.json(), on.json()
        # without the flag: the keys and the sources of before, and no attributor was made
        assert set(plain) == set(off) == {"answer", "sources", "processing_time"}
        assert all(set(s) == {"rank", "doc_id", "relevance_score", "type"} for s in plain["sources"])
        assert {k: v for k, v in off.items() if k != "processing_time"} == \
            {k: v for k, v in plain.items() if k != "processing_time"}
        # with it: the generator's answer (the raw chunks joined) unchanged, every sentence cites the hit it came from
        assert set(on) == {"answer", "sources", "processing_time", "citations", "groundedness"}
        assert on["answer"] == plain["answer"] and on["groundedness"] == 1.0
        assert [{k: v for k, v in s.items() if k not in ("cited_by", "support")} for s in on["sources"]] == \
            plain["sources"]
        assert len(on["citations"]) == 12 and all(c["supported"] for c in on["citations"])
        for at, c in enumerate(on["citations"]):
            assert on["answer"][c["start"]: c["end"]] == c["text"]
            assert [s["source"] for s in c["sources"]] == [at // 6] and c["sources"][0]["text"] == c["text"]
        assert [s["cited_by"] for s in on["sources"]] == [list(range(6)), list(range(6, 12))]
        assert sum(s["support"] for s in on["sources"]) == pytest.approx(1.0)
        direct = asyncio.run(manager.attribute_answer(on["answer"], on["answer"].split("\n\n"), threshold=0.9,
                                                      max_citations=2))
        assert direct["citations"] == on["citations"]
        # the parameters alone are refused, and so is a flag that is no boolean
        r = client.post("/query", json={"query": "zebra", "citation_threshold": 0.5})
        assert r.status_code == 400 and "`citations`" in r.json()["detail"]
        assert client.post("/query", json={"query": "zebra", "max_citations": 2}).status_code == 400
        assert client.post("/query", json={"query": "zebra", "citations": "yes please"}).status_code == 422
        assert client.post("/query", json={"query": "zebra", "citations": True, "max_citations": 9}).status_code == 422
        assert client.post("/query", json={"query": "zebra", "citations": True,
                                           "citation_threshold": 1.5}).status_code == 422


def test_the_flag_defaults_to_the_setting_and_a_bad_setting_is_a_400(monkeypatch):
    manager = CitingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=manager)) as client:
        uploaded(client)
        monkeypatch.setattr(config.settings, "MMRAG_CITATIONS", 1)
        monkeypatch.setattr(config.settings, "MMRAG_CITATION_THRESHOLD", 0.9)
        assert "citations" in client.post("/query", json={"query": "zebra"}).json()
        assert "citations" not in client.post("/query", json={"query": "zebra", "citations": False}).json()
        monkeypatch.setattr(config.settings, "MMRAG_CITATION_MAX", 12)
        r = client.post("/query", json={"query": "zebra", "citations": True})
        assert r.status_code == 400 and "MMRAG_CITATION_MAX" in r.json()["detail"]


def test_citations_with_an_extractive_and_a_reader_answer(monkeypatch):
    from tests.test_reader_cpu import FakeReader

    manager = CitingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=manager)) as client:
        uploaded(client)
        got = client.post("/query", json={"query": "zebra", "top_k": 2, "extractive_answer": True, "citations": True,
                                          "citation_threshold": 0.9})
        assert got.status_code == 200, got.text
        got = got.json()
        assert set(got) == {"answer", "sources", "processing_time", "citations", "groundedness"}
        assert [c["text"] for c in got["citations"]] == [s["quotes"][0]["text"] for s in got["sources"]]
        assert [s["cited_by"] for s in got["sources"]] == [[0], [1]] and got["groundedness"] == 1.0
        # each quoted sentence is found where the quote says it is
        for c, s in zip(got["citations"], got["sources"]):
            assert (c["sources"][0]["start"], c["sources"][0]["end"]) == (s["quotes"][0]["start"], s["quotes"][0]["end"])
        manager._reader = FakeReader()
        read = client.post("/query", json={"query": "which animal", "top_k": 2, "reader_answer": True,
                                           "citations": True, "citation_threshold": 0.2})
        assert read.status_code == 200, read.text
        read = read.json()
        assert set(read) == {"answer", "sources", "processing_time", "answers", "answerable", "citations",
                             "groundedness"}
        assert read["answer"] == "zebra" and [c["text"] for c in read["citations"]] == ["zebra"]
        zebra_hit = read["answers"][0]["hit"]
        assert read["citations"][0]["sources"][0]["source"] == zebra_hit
        assert read["sources"][zebra_hit]["cited_by"] == [0] and read["sources"][1 - zebra_hit]["cited_by"] == []
        assert all("answer_spans" in s and "support" in s for s in read["sources"])


def test_an_embedder_without_citations_gets_a_400():
    with TestClient(create_app(embedder=EmbeddingManager(engine=FakeEngine()))) as client:
        r = client.post("/query", json={"query": "zebra", "citations": True})
        assert r.status_code == 400 and r.json()["detail"] == CITATION_NEEDS[2]
        r = client.post("/attribute", json={"answer": "x.", "passages": ["x."]})
        assert r.status_code == 400 and r.json()["detail"] == CITATION_NEEDS[2]
        assert client.post("/query", json={"query": "zebra"}).status_code == 200
    manager = EmbeddingManager(engine=FakeEngine())
    assert not manager.supports_citations()
    with pytest.raises(ValueError, match="encode_device"):
        asyncio.run(manager.attribute_answer("An answer.", ["A passage."]))


def test_post_attribute_with_passages_and_with_stored_ids():
    manager = CitingManager(engine=FakeEngine())
    answer = "It was painted in spring. Herons nest in the reeds. " + ALIEN
    with TestClient(create_app(embedder=manager)) as client:
        uploaded(client)
        got = client.post("/attribute", json={"answer": answer, "passages": [HERON, ZEBRA], "citation_threshold": 0.9})
        assert got.status_code == 200, got.text
        got = got.json()
        assert set(got) == {"citations", "groundedness", "support", "considered", "processing_time"}
        assert [[s["source"] for s in c["sources"]] for c in got["citations"]] == [[1], [0], []]
        assert got["considered"] == {"claims": 3, "evidence": 12} and 0.0 < got["groundedness"] < 1.0
        direct = asyncio.run(manager.attribute_answer(answer, [HERON, ZEBRA], threshold=0.9))
        assert {k: v for k, v in got.items() if k != "processing_time"} == direct
        # by stored ids: source i is ids[i]
        hits = client.post("/query", json={"query": "zebra", "top_k": 2, "extractive_answer": True}).json()["sources"]
        ids = [s["doc_id"] for s in hits]
        by_id = client.post("/attribute", json={"answer": answer, "ids": ids, "citation_threshold": 0.9})
        assert by_id.status_code == 200, by_id.text
        by_id = by_id.json()
        zebra_at = 0 if "zebra" in hits[0]["quotes"][0]["text"] else 1
        assert [[s["source"] for s in c["sources"]] for c in by_id["citations"]] == [[zebra_at], [1 - zebra_at], []]
        assert by_id["groundedness"] == got["groundedness"]
        # one of the two, not both and not neither; an unknown id has no passages: nothing is supported
        assert client.post("/attribute", json={"answer": answer}).status_code == 400
        assert client.post("/attribute", json={"answer": answer, "passages": [HERON], "ids": ids}).status_code == 400
        assert client.post("/attribute", json={"answer": answer, "passages": ["x"] * 65}).status_code == 422
        none = client.post("/attribute", json={"answer": answer, "ids": ["no-such-id"]}).json()
        assert none["citations"] == [] and none["groundedness"] == 0.0

