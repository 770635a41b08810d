"""Host side of the BM25 lexical leg: the native analyzer against its Python twin and tests/bm25_ref.py, the lexicon's
id rules, rrf_fuse, the C-ABI size queries, POST /query with "hybrid", and the lexical kernels' resource usage."""
import asyncio
import os
import random
import re
import shutil
import subprocess
import unicodedata

import numpy as np
import pytest
from fastapi.testclient import TestClient

from multimodal_rag_amd import lexical as L
from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.server import create_app
from tests import bm25_ref as R
from tests.fakes import FakeCollection, FakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAND = [
    "Những khái niệm cơ bản về ngôn ngữ C",
    "Học HỌC học hoc hóc",                                 # NFC upper / lower, NFD spelling, no marks
    "Học",                                                  # NFD
    "C++, printf(\"%d\\n\", x); a.b-c_d 'quoted' [x]",
    "中文字 mixed中文text 日本語",
    "ΣΊΣΥΦΟΣ ὈΔΥΣΣΕΎΣ Σ aΣ aΣb",                            # final sigma in and out of context
    "",
    "   \t\n  ",
    "İstanbul ǅemal ﬁle ß ẞ",                               # lower() that grows, ligature, sharp s
    "ắ ẵ ẳ ặ ỗ ữ ự Ð đ",
    "tab\tsep nbsp em​zero-width\x00nul�repl",
    "emoji 🙂 end. ... !!! ??",
]


def _native_terms(texts):
    lx = L.Lexicon()
    off, ids, tfs, dl = lx.analyze_batch(texts, L.LEX_DOCUMENTS)
    return lx, off, ids, tfs, dl


def test_analyzer_hand_cases():
    hoc = unicodedata.normalize("NFD", "học")
    assert L.analyze("Học HỌC " + hoc + " hoc") == [hoc] * 3 + ["hoc"]
    assert L.analyze("C++, printf(x);") == ["c", "printf", "x"]
    assert L.analyze("中文a") == ["中", "文", "a"]
    assert L.analyze(None) == [] and L.analyze("  \n") == []
    for t in HAND:
        assert L.analyze(t) == R.analyze(t), t


def _check_batch_against_twin(texts):
    """native (term id, tf) pairs and dl of every text == the Python twin's terms counted, ids first-seen"""
    lx, off, ids, tfs, dl = _native_terms(texts)
    vocab = {}
    for i, t in enumerate(texts):
        terms = L.analyze(t)
        assert dl[i] == len(terms), (t, dl[i], terms)
        counts = {}
        for term in terms:
            tid = vocab.setdefault(term, len(vocab))
            counts[tid] = counts.get(tid, 0) + 1
        got = list(zip(ids[off[i]:off[i + 1]].tolist(), tfs[off[i]:off[i + 1]].tolist()))
        assert got == sorted(counts.items()), (t, got, counts)
    assert len(lx) == len(vocab)


def test_native_analyzer_equals_twin_hand_cases():
    _check_batch_against_twin(HAND + [None])


def _fuzz_strings(n, seed):
    rng = random.Random(seed)
    pools = [
        "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789",
        "àáảãạăắằẳẵặâấầẩẫậèéẻẽẹêếềểễệìíỉĩịòóỏõọôốồổỗộơớờởỡợùúủũụưứừửữựỳýỷỹỵđĐ",
        "ÀÁẢÃẠĂẮẰẲẴẶÂẤẦẨẪẬÈÉẺẼẸÊẾỀỂỄỆÌÍỈĨỊÒÓỎÕỌÔỐỒỔỖỘƠỚỜỞỠỢÙÚỦŨỤƯỨỪỬỮỰỲÝỶỸỴ",
        "̛̣̀́̃̉̂̆",          # combining marks (NFD input)
        " \t\n\r  　",
        ".,;:!?()[]{}<>\"'`~@#$%^&*-_+=/\\|–—“”¿¡。",
        "中文字日本語한국어가나다",
        "ΣσςΑαΩωΆΈΉΊΌΎΏ",
        "İıẞßǅǄǆﬁﬂİK",
        "\x00\x01\x7f​‍﻿�\U0001F642",
    ]
    out = []
    for _ in range(n):
        s = []
        for _ in range(rng.randint(0, 40)):
            s.append(rng.choice(rng.choice(pools)))
        out.append("".join(s))
    return out


def test_native_analyzer_equals_twin_fuzzed():
    texts = _fuzz_strings(2500, 1234)
    _check_batch_against_twin(texts)
    # the same batch on one thread and on many gives the same ids
    a = L.Lexicon(n_threads=1).analyze_batch(texts * 8, L.LEX_DOCUMENTS)
    b = L.Lexicon(n_threads=8).analyze_batch(texts * 8, L.LEX_DOCUMENTS)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_lexicon_first_seen_and_queries_add_nothing():
    lx = L.Lexicon()
    off, ids, tfs, dl = lx.analyze_batch(["b a b", "a c", None], L.LEX_DOCUMENTS)
    assert off.tolist() == [0, 2, 4, 4] and ids.tolist() == [0, 1, 1, 2] and tfs.tolist() == [2, 1, 1, 1]
    assert dl.tolist() == [3, 2, 0] and len(lx) == 3
    off, ids, tfs, dl = lx.analyze_batch(["c zz b c a", "unknown only", ""], L.LEX_QUERIES)
    assert off.tolist() == [0, 3, 3, 3] and ids.tolist() == [2, 0, 1] and tfs.tolist() == [2, 1, 1]
    assert dl.tolist() == [5, 2, 0] and len(lx) == 3
    lx.analyze_batch(["zz b"], L.LEX_DOCUMENTS)
    assert len(lx) == 4 and lx.analyze_batch(["zz"], L.LEX_QUERIES)[1].tolist() == [3]


def test_rrf_fuse_hand_cases():
    # row 5: dense rank 1 only; row 7: lexical rank 1 only -> equal scores, the dense one wins; then the lower row
    assert L.rrf_fuse([5], [7], k=60) == [(5, 1 / 61), (7, 1 / 61)]
    assert L.rrf_fuse([], [9, 3], k=60) == [(9, 1 / 61), (3, 1 / 62)]
    # both legs: 1/61 + 1/63 for row 1 (dense 1, lexical 3) vs 1/62 + 1/62 for row 2 -> compare exact floats
    got = L.rrf_fuse([1, 2, 4], [8, 2, 1], k=60)
    want = R.rrf([1, 2, 4], [8, 2, 1], k=60)
    assert got == want
    # lexical-only rows tie among themselves at the same rank only if in different legs: lower row after dense rank
    assert [r for r, _ in L.rrf_fuse([10, 11], [11, 10], k=1)] == [10, 11]
    rng = np.random.default_rng(0)
    for _ in range(200):
        d = rng.permutation(30)[: rng.integers(0, 12)].tolist()
        lx = rng.permutation(30)[: rng.integers(0, 12)].tolist()
        k = int(rng.integers(1, 80))
        assert L.rrf_fuse(d, lx, k) == R.rrf(d, lx, k)


def test_workspace_sizes_without_gpu():
    assert L.bm25_workspace_bytes(1, 1000, 5) > 0
    assert L.bm25_workspace_bytes(0, 1000, 5) == 0 and L.bm25_workspace_bytes(1, 1000, 4097) == 0
    assert L.bm25_workspace_bytes(1, 10**6, 4096) >= 8 * 10**6        # one query x n overflow slots
    assert L.bm25_workspace_bytes(256, 10**6, 50) >= L.bm25_workspace_bytes(1, 10**6, 50)
    assert L.csr_build_workspace_bytes(10**6, 200000) >= 200000 * 12
    assert L.csr_build_workspace_bytes(-1, 5) == 0


class HybridCollection(FakeCollection):
    """the fake collection plus a hybrid_query: the dense hits with made-up fused scores"""

    def hybrid_query(self, query_embeddings, query_texts, n_results=10, where=None, include=()):
        res = self.query(query_embeddings, n_results=n_results, where=where)
        res["hybrid_scores"] = [[1.0 / (61 + i) for i in range(len(ids))] for ids in res["ids"]]
        res["lexical_scores"] = [[0.0] * len(ids) for ids in res["ids"]]
        return res


def _upload(client):
    for i, body in enumerate(["alpha beta gamma. " * 3, "delta epsilon. " * 3, "zeta eta theta. " * 3]):
        r = client.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
        assert r.status_code == 200, r.text


def test_query_hybrid_400_without_hybrid_collection():
    m = EmbeddingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=m)) as c:
        _upload(c)
        plain = c.post("/query", json={"query": "delta", "top_k": 2})
        assert plain.status_code == 200
        assert c.post("/query", json={"query": "delta", "top_k": 2, "hybrid": False}).json()["sources"] == \
            plain.json()["sources"]
        r = c.post("/query", json={"query": "delta", "top_k": 2, "hybrid": True})
        assert r.status_code == 400 and "Hybrid" in r.json()["detail"]


def test_query_hybrid_with_fake_collection(monkeypatch):
    eng = FakeEngine()
    orig = eng.new_collection

    def new_collection(*a, **kw):
        c = orig(*a, **kw)
        c.__class__ = HybridCollection
        return c

    monkeypatch.setattr(eng, "new_collection", new_collection)
    m = EmbeddingManager(engine=eng)
    with TestClient(create_app(embedder=m)) as c:
        _upload(c)
        before = m.stats["total_queries"]
        r = c.post("/query", json={"query": "delta", "top_k": 2, "hybrid": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert len(src) == 2 and [s["hybrid_score"] for s in src] == [1 / 61, 1 / 62]
        assert set(src[0]) == {"rank", "doc_id", "relevance_score", "type", "hybrid_score"}
        assert m.stats["total_queries"] == before + 1
        assert all("hybrid_score" not in s for s in c.post("/query", json={"query": "delta", "top_k": 2}).json()["sources"])
    with pytest.raises(ValueError):
        asyncio.run(m.hybrid_query("   "))


def test_lexical_kernels_no_scratch_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", "-I",
                        os.path.join(ROOT, "include"), os.path.join(ROOT, "multimodal_rag_amd", "csrc", "lexical.hip"),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern in ("bm25_score_kernel", "csr_sort_kernel", "csr_scatter_kernel", "csr_scan_kernel", "csr_hist_kernel",
                 "df_update_kernel", "rows_dot_kernel", "deep_select_kernel"):
        assert any(kern in n for n in names), kern
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] + \
        [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    assert len(scratch) == len(names) and not any(scratch) and not any(spills)
