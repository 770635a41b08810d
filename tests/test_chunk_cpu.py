"""CPU: semantic chunking -- the NumPy model (tests/chunk_ref.py) against brute force, the host side of chunking.py with
a chunker whose cuts are fixed, the settings, the parser stage and POST /chunk."""
import asyncio
import os

import numpy as np
import pytest
from starlette.testclient import TestClient

from multimodal_rag_amd import _native, config
from multimodal_rag_amd import chunking as CK
from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.ingest import TextDocumentParser, basic_chunk_text
from multimodal_rag_amd.server import CHUNK_NEEDS, create_app
from multimodal_rag_amd.summarize import split_sentences
from tests import chunk_ref as R
from tests.fakes import FakeEngine


# ---------------------------------------------------------------- the model
def exact_case(rng, n, d=16):
    """rows of multiples of 1/8 with few non-zeros: every S_ij, every partial sum and every objective is exact in
    float32 and float64 alike"""
    x = np.zeros((n, d))
    for i in range(n):
        cols = rng.choice(d, 6, replace=False)
        x[i, cols] = rng.integers(-1, 5, 6) / 8.0
    return R.similarities(x)


# (W, max_cost, the cost range): the cap binds / W binds / W = 1 / sentences above the cap / nothing binds
REGIMES = {"cap": (9, 9, (1, 6)), "W": (3, 10 ** 6, (1, 6)), "W1": (1, 10 ** 6, (1, 6)), "over": (9, 4, (1, 9)),
           "free": (9, 10 ** 6, (1, 6))}


@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_model_equals_brute_force_on_exact_cases(regime):
    W, max_cost, (lo, hi) = REGIMES[regime]
    binds = over = 0
    for seed in range(20):
        rng = np.random.default_rng([seed, len(regime)])
        n = 9
        S = exact_case(rng, n)
        cost = rng.integers(lo, hi + 1, n)
        tau, beta = rng.integers(0, 9) / 64.0, rng.integers(0, 9) / 64.0
        prev, best = R.segment(S, cost, max_cost, W, tau, beta)
        cuts = R.cuts_of(prev)
        assert cuts[0] == 0 and R.admissible(cuts, n, cost, max_cost, W)
        top, found = R.brute_force(S, cost, max_cost, W, tau, beta)
        assert best[-1] == top == R.objective(S, cuts, tau, beta), (seed, best[-1], top)
        assert cuts in found
        # ties to the lowest a at every step: the LAST chunk of the model's answer is the longest among the optima's
        assert cuts[-1] == min(c[-1] for c in found)
        free_top, _ = R.brute_force(S, cost, 10 ** 9, n, tau, beta)
        binds += free_top > top
        if regime == "W1":
            assert cuts == list(range(n))
        over += bool((cost > max_cost).any())
    assert over >= 15 if regime == "over" else over == 0
    if regime in ("cap", "W", "W1", "over"):
        assert binds >= 5, f"the limit of regime {regime!r} changed the optimum in only {binds} of 20 cases"


def test_float32_model_equals_the_float64_model_bit_for_bit_on_exact_data():
    for seed in range(10):
        rng = np.random.default_rng(100 + seed)
        n = int(rng.integers(1, 150))
        S = exact_case(rng, n, d=32)
        cost = rng.integers(1, 9, n)
        W = int(rng.choice([1, 2, 17, 64]))
        tau, beta = rng.integers(0, 17) / 64.0, rng.integers(0, 9) / 64.0
        p64, b64 = R.segment(S, cost, 40, W, tau, beta, np.float64)
        p32, b32 = R.segment(S, cost, 40, W, tau, beta, np.float32)
        assert b32.dtype == np.float32 and np.array_equal(p32, p64) and np.array_equal(b32.astype(np.float64), b64)
        t64, t32 = R.auto_tau(S, 0.5), R.auto_tau(S, 0.5, np.float32)
        # the mean's division is the one operation that rounds: the two agree when (n - 1) divides exactly
        if n == 1 or (n - 1) & (n - 2) == 0:
            assert float(t32) == float(t64)
    assert R.auto_tau(np.ones((1, 1)), 0.5) == 0.0
    assert R.auto_tau(np.array([[1.0, 0.5, 9.0], [0.5, 1.0, 0.25], [9.0, 0.25, 1.0]]), 2.0) == 0.75


def test_model_edges():
    S = np.full((5, 5), 0.5)
    assert R.cuts_of(R.segment(S, [1] * 5, 100, 64, 0.25, 0.0)[0]) == [0]               # everything attracts
    assert R.cuts_of(R.segment(S, [1] * 5, 100, 64, 0.75, 0.0)[0]) == [0, 1, 2, 3, 4]   # everything repels
    assert R.cuts_of(R.segment(S, [1] * 5, 100, 64, 0.5, 0.0)[0]) == [0]                # all ties: the lowest a
    assert R.cuts_of(R.segment(S, [1] * 5, 2, 64, 0.25, 0.0)[0]) == [0, 1, 3]           # the cap: the last is longest
    assert R.cuts_of(R.segment(S, [7] * 5, 2, 64, 0.25, 0.0)[0]) == [0, 1, 2, 3, 4]     # every cost above the cap
    prev, best = R.segment(np.ones((1, 1)), [3], 1, 1, 0.0, 0.25)
    assert prev.tolist() == [0] and best.tolist() == [-0.25]


# ---------------------------------------------------------------- header and binding
def test_header_constant_equals_the_binding():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mmrag.h"), encoding="utf-8").read()
    assert "#define MMRAG_MAX_CHUNK_SENTENCES 64" in header and _native.MAX_CHUNK_SENTENCES == 64
    assert "int mmrag_chunk_boundaries(" in header and "parser.py:1702-1736" in header
    assert "chunk.hip" in __import__("multimodal_rag_amd.build", fromlist=["SOURCES"]).SOURCES


def test_chunk_boundaries_refuses_host_tensors():
    import torch

    rows = torch.zeros((4, 64), dtype=torch.float16)
    table = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_native.MMRagNativeError, match="device"):
        _native.chunk_boundaries(rows, 64, table, table, torch.ones(4, dtype=torch.int32), 10, 4)


# ---------------------------------------------------------------- the host side
TEXT = ("Solar panels turn light into power.  A panel holds many cells!\nEach cell frees electrons. "
        "Bread starts from flour and water. The dough proofs overnight?   A hot pot gives the crust. "
        "Steam lets the loaf rise.")


class FixedChunker(CK.DeviceChunker):
    """a chunker whose cuts are given: chunks of `size` sentences"""

    def __init__(self, size=3):
        self.size, self.calls = size, []

    def segment(self, units, costs, max_cost, max_sentences, threshold=None, auto_scale=0.5, penalty=0.0):
        self.calls.append((len(units), [list(c) for c in costs], max_cost, max_sentences, threshold, auto_scale, penalty))
        return [{"runs": [(a, min(a + self.size, len(u)), 1.5) for a in range(0, len(u), self.size)], "tau": 0.25,
                 "score": 0.0} for u in units]


def test_semantic_costs_bound_every_slice():
    spans = split_sentences(TEXT)
    costs = CK.semantic_costs(TEXT, spans)
    assert len(spans) == 7 and len(costs) == 7 and all(c >= 1 for c in costs)
    assert costs[0] == spans[1][0] - spans[0][0] and costs[-1] == spans[-1][1] - spans[-1][0]
    for a in range(7):
        for b in range(a + 1, 8):
            assert spans[b - 1][1] - spans[a][0] <= sum(costs[a:b])
    assert CK.semantic_costs("", []) == [] and CK.semantic_costs("One.", [(0, 4)]) == [4]


def check_chunks(text, chunks, chunk_size, overlap=0):
    spans = split_sentences(text, chunk_size)
    assert sum(c["sentences"] for c in chunks) == len(spans)                                 # coverage
    at = 0
    for i, c in enumerate(chunks):
        assert (c["start"], c["end"]) == (spans[at][0], spans[at + c["sentences"] - 1][1])
        at += c["sentences"]
        lo = c.get("overlap_start", c["start"])
        assert c["content"] == text[lo: c["end"]] == c["content"].strip() and len(c["content"]) <= chunk_size
        assert text[c["start"]: c["end"]] == text[c["start"]: c["end"]].strip()
        if "overlap_start" in c:
            assert i > 0 and overlap > 0 and chunks[i - 1]["start"] <= lo < c["start"] and c["start"] - lo <= overlap
            assert lo in [a for a, _ in spans]                                               # whole sentences
    assert all(p["end"] <= c["start"] for p, c in zip(chunks, chunks[1:]))                   # order, no overlap


def test_chunk_texts_covers_the_text_in_order():
    fake = FixedChunker(3)
    got = fake.chunk_texts([TEXT, "One sentence only.", "", "   \n "], chunk_size=1000, overlap=0)
    assert [len(g) for g in got] == [3, 1, 0, 0]
    check_chunks(TEXT, got[0], 1000)
    assert [c["sentences"] for c in got[0]] == [3, 3, 1] and all(c["gain"] == 1.5 for c in got[0])
    assert not any("overlap_start" in c for c in got[0])
    assert got[1] == [{"content": "One sentence only.", "start": 0, "end": 18, "sentences": 1, "gain": -0.0}]
    # one launch for the one text of more than one sentence, with its costs and the settings' parameters
    assert len(fake.calls) == 1
    n_units, costs, max_cost, most, threshold, scale, penalty = fake.calls[0]
    assert (n_units, costs, max_cost) == (1, [CK.semantic_costs(TEXT, split_sentences(TEXT))], 1000)
    assert (most, threshold, scale, penalty) == (64, None, 0.5, 0.0)
    # texts of one sentence or none: no launch at all
    quiet = FixedChunker(3)
    assert [len(g) for g in quiet.chunk_texts(["Just this.", ""], chunk_size=50)] == [1, 0] and quiet.calls == []


def test_chunk_texts_overlap_prefixes_whole_sentences():
    fake = FixedChunker(2)
    got = fake.chunk_texts([TEXT], chunk_size=120, overlap=40)[0]
    check_chunks(TEXT, got, 120, overlap=40)
    assert fake.calls[0][2] == 80                                   # the kernel's cap leaves room for the prefix
    spans = split_sentences(TEXT, 120)
    assert "overlap_start" not in got[0]
    # chunk 1 = sentences 2, 3: sentence 1 (27 characters and a gap) fits in 40, sentences 0 + 1 do not
    assert got[1]["overlap_start"] == spans[1][0] and got[1]["content"].startswith("A panel holds many cells!")
    assert any("overlap_start" in c for c in got[2:])
    with pytest.raises(ValueError):
        fake.chunk_texts([TEXT], chunk_size=100, overlap=100)
    with pytest.raises(ValueError):
        fake.chunk_texts([TEXT], chunk_size=0)


def test_long_sentences_are_cut_to_the_chunk_size():
    text = "word " * 100 + "end. Short one."
    got = FixedChunker(1).chunk_texts([text], chunk_size=60)[0]
    check_chunks(text, got, 60)
    assert len(got) > 8


# ---------------------------------------------------------------- settings
def test_chunker_settings_are_checked(monkeypatch):
    fresh = config.Settings()
    assert config.settings.chunker() == "basic" and fresh.MMRAG_CHUNKER == "basic"
    assert (fresh.MMRAG_CHUNK_THRESHOLD, fresh.MMRAG_CHUNK_AUTO_SCALE, fresh.MMRAG_CHUNK_PENALTY,
            fresh.MMRAG_CHUNK_MAX_SENTENCES, fresh.MMRAG_CHUNK_SEMANTIC_OVERLAP) == ("", 0.5, 0.0, 64, 0)
    assert fresh.chunk_parameters() == {"threshold": None, "auto_scale": 0.5, "penalty": 0.0, "max_sentences": 64,
                                        "overlap": 0}
    monkeypatch.setenv("MMRAG_CHUNKER", "recursive")
    with pytest.raises(ValueError, match="MMRAG_CHUNKER"):
        config.Settings()
    monkeypatch.setenv("MMRAG_CHUNKER", "semantic")
    monkeypatch.setenv("MMRAG_CHUNK_THRESHOLD", "0.3")
    monkeypatch.setenv("MMRAG_CHUNK_SEMANTIC_OVERLAP", "1")
    got = config.Settings()
    assert got.chunker() == "semantic"
    assert got.chunk_parameters()["threshold"] == 0.3 and got.chunk_parameters()["overlap"] == got.CHUNK_OVERLAP
    for name, bad in (("MMRAG_CHUNK_THRESHOLD", "warm"), ("MMRAG_CHUNK_THRESHOLD", "inf"),
                      ("MMRAG_CHUNK_AUTO_SCALE", "0"), ("MMRAG_CHUNK_AUTO_SCALE", "nan"), ("MMRAG_CHUNK_PENALTY", "-1"),
                      ("MMRAG_CHUNK_MAX_SENTENCES", "65"), ("MMRAG_CHUNK_MAX_SENTENCES", "0"),
                      ("MMRAG_CHUNK_SEMANTIC_OVERLAP", "2")):
        with monkeypatch.context() as m:
            m.setenv(name, bad)
            with pytest.raises(ValueError, match="MMRAG_CHUNK"):
                config.Settings()
    monkeypatch.setattr(config.settings, "MMRAG_CHUNKER", "nonsense")
    with pytest.raises(ValueError):
        config.settings.chunker()
    with pytest.raises(ValueError):
        CK.make_parser(lambda: None)


# ---------------------------------------------------------------- the parser stage and the server
class ChunkingManager(EmbeddingManager):
    """an embedder whose chunks are recognisable: two sentences each"""

    def supports_chunking(self):
        return True

    async def chunk_texts(self, texts, chunk_size=None):
        return FixedChunker(2).chunk_texts(list(texts), chunk_size=chunk_size, overlap=0)


def test_semantic_parser_keeps_the_stage_contract():
    fake = ChunkingManager(engine=FakeEngine())
    ours = CK.SemanticDocumentParser(lambda: fake)          # resolved at the first document
    got = asyncio.run(ours.parse_document(TEXT.encode("utf-8"), "solar.txt", "text/plain", doc_id="doc_1"))
    want = asyncio.run(TextDocumentParser().parse_document(TEXT.encode("utf-8"), "solar.txt", "text/plain",
                                                           doc_id="doc_1"))
    assert sorted(got) == sorted(want) and {k: v for k, v in got.items() if k != "text_chunks"} == \
        {k: v for k, v in want.items() if k != "text_chunks"}
    assert len(got["text_chunks"]) == 4 and len(want["text_chunks"]) == 1
    for i, chunk in enumerate(got["text_chunks"]):
        assert sorted(chunk) == sorted(want["text_chunks"][0])
        assert chunk["chunk_id"].startswith(f"doc_1_chunk_{i}_") and len(chunk["chunk_id"]) == len(f"doc_1_chunk_{i}_") + 8
        meta = chunk["metadata"]
        assert set(meta) == set(want["text_chunks"][0]["metadata"]) | {"char_start", "char_end", "sentence_count",
                                                                        "chunker"}
        assert TEXT[meta["char_start"]: meta["char_end"]] == chunk["content"] and meta["chunker"] == "semantic"
        assert meta["char_count"] == len(chunk["content"]) and meta["sentence_count"] == (2 if i < 3 else 1)
        assert (meta["filename"], meta["doc_type"], meta["doc_id"]) == ("solar.txt", "text", "doc_1")
    refusals = []
    for parser in (ours, TextDocumentParser()):
        with pytest.raises(ValueError) as e:
            asyncio.run(parser.parse_document(b"%PDF", "paper.pdf", "application/pdf", doc_id="d"))
        refusals.append(str(e.value))
    assert refusals[0] == refusals[1]
    assert asyncio.run(ours.parse_document(b"  \n", "empty.txt", doc_id="d"))["text_chunks"] == []


def test_upload_under_both_settings_and_the_chunk_route(monkeypatch):
    stored = {}
    for setting in ("semantic", "basic"):
        monkeypatch.setattr(config.settings, "MMRAG_CHUNKER", setting)
        manager = ChunkingManager(engine=FakeEngine())
        with TestClient(create_app(embedder=manager)) as client:
            up = client.post("/upload", files={"file": ("solar.txt", TEXT.encode("utf-8"), "text/plain")})
            assert up.status_code == 200, up.text
            assert set(up.json()) == {"doc_id", "filename", "doc_type", "chunks_processed", "message", "processing_time"}
            got = manager.collection.get(where={"doc_id": up.json()["doc_id"]})
            stored[setting] = (got["documents"], got["metadatas"])
            # the preview route does not depend on the setting
            r = client.post("/chunk", json={"text": TEXT, "chunk_size": 500})
            assert r.status_code == 200 and r.json()["chunker"] == "semantic"
            assert [c["sentences"] for c in r.json()["chunks"]] == [2, 2, 2, 1]
            check_chunks(TEXT, r.json()["chunks"], 500)
            assert client.post("/chunk", json={"text": ""}).json()["chunks"] == []
            assert client.post("/chunk", json={"chunk_size": 5}).status_code == 422
            assert client.post("/chunk", json={"text": "x", "chunk_size": 0}).status_code == 422
    docs, metas = stored["semantic"]
    assert len(docs) == 4 and all(m["chunker"] == "semantic" and m["sentence_count"] in (1, 2) for m in metas)
    assert sorted(TEXT[m["char_start"]: m["char_end"]] for m in metas) == sorted(docs)     # (short chunks: summary = raw)
    # "basic" is the parse the pipeline gives today: one chunk, the window's, and no new metadata key
    docs, metas = stored["basic"]
    assert len(docs) == 1 and basic_chunk_text(TEXT) == [TEXT] and "chunker" not in metas[0]
    assert "char_start" not in metas[0]


def test_basic_setting_gives_the_parse_it_gives_today():
    assert CK.make_parser(lambda: None) is None                     # the pipeline keeps TextDocumentParser
    text = ("A sentence that fills the window. " * 70).strip()
    got = asyncio.run(TextDocumentParser().parse_document(text.encode("utf-8"), "w.txt", doc_id="d"))
    assert [c["content"] for c in got["text_chunks"]] == [c.strip() for c in basic_chunk_text(text, 1000, 200)]
    assert all(set(c["metadata"]) == {"char_count", "filename", "doc_type", "doc_id"} for c in got["text_chunks"])


def test_an_embedder_without_chunking_gets_a_400():
    with TestClient(create_app(embedder=EmbeddingManager(engine=FakeEngine()))) as client:
        r = client.post("/chunk", json={"text": TEXT})
        assert r.status_code == 400 and r.json()["detail"] == CHUNK_NEEDS[2]
    manager = EmbeddingManager(engine=FakeEngine())
    assert not manager.supports_chunking()
    with pytest.raises(ValueError, match="encode_device"):
        asyncio.run(manager.chunk_texts([TEXT]))
