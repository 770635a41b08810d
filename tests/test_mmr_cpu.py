"""Host side of MMR retrieval: tests/mmr_ref.py on hand-made inputs, the C-ABI entry's exports and argument checks
(no GPU: they come before any HIP call), POST /query with "mmr", and the MMR kernels' resource usage."""
import asyncio
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from fastapi.testclient import TestClient

from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.server import create_app
from tests import mmr_ref as R
from tests.fakes import FakeCollection, FakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference on known answers
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def test_ref_lambda_one_is_the_dense_order():
    g = np.random.default_rng(0)
    M = g.standard_normal((30, 8))
    rel = -np.sort(-g.random(12))
    rows = g.permutation(30)[:12]
    pos, val = R.select(rel, rows, M, 7, 1.0)
    assert pos == list(range(7)) and val == rel[:7].tolist()


def test_ref_planted_duplicate_of_the_top_hit_goes_last():
    # rows 0 and 1 are the same vector (sim 1): at lambda 0.5 the copy waits until every other candidate is taken
    M = np.stack([_unit([1, 0, 0, 0]), _unit([1, 0, 0, 0]), _unit([0.8, 0.6, 0, 0]), _unit([0.7, 0, 0.7, 0.1]),
                  _unit([0.6, 0.1, 0.1, 0.78])])
    q = _unit([1, 0.05, 0.02, 0.01])
    rel = M @ q
    order = np.lexsort((np.arange(5), -rel))
    assert order[:2].tolist() == [0, 1]
    pos, val = R.select(rel[order], order, M, 5, 0.5)
    assert pos[0] == 0 and pos[-1] == 1 and sorted(pos) == [0, 1, 2, 3, 4]
    assert val[-1] == pytest.approx(0.5 * rel[1] - 0.5 * 1.0)
    assert R.select(rel[order], order, M, 5, 1.0)[0] == [0, 1, 2, 3, 4]


def test_ref_ties_go_to_the_lower_position_and_values():
    # candidates 1, 2, 3 are the same row with the same relevance: picked in position order
    M = np.array([[2.0, 0.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [1.0, 1.0]])
    rows = np.array([0, 1, 2, 3, 4])
    rel = np.array([4.0, 2.0, 2.0, 2.0, 2.0])
    pos, val = R.select(rel, rows, M, 5, 0.5)
    # step 1: v = 1 - 0.5 * sim(i, 0): rows 1..3 have sim 0 -> v = 1 (lowest position 1); row 4 sim 2 -> 0
    # step 2: rows 2, 3 now have maxsim 1 -> v = 0.5; row 4: max(2, 1) -> 0
    assert pos == [0, 1, 2, 3, 4] and val == [4.0, 1.0, 0.5, 0.5, 0.0]
    # lambda 0: pure diversity after the first pick
    pos0, val0 = R.select(rel, rows, M, 3, 0.0)
    assert pos0 == [0, 1, 2] and val0 == [4.0, 0.0, -1.0]


def test_ref_short_candidate_lists():
    M = np.eye(4)
    rel = np.array([0.9, 0.5, -np.inf, -np.inf])
    rows = np.array([2, 0, -1, -1])
    s, r, p, v = R.select_padded(rel, rows, M, 3, 0.5)
    assert r.tolist() == [2, 0, -1] and p.tolist() == [0, 1, -1]
    assert s.tolist() == [np.float32(0.9), 0.5, -math.inf] and v.tolist() == [np.float32(0.9), 0.25, -math.inf]
    s, r, p, v = R.select_padded(np.full(3, -np.inf), np.full(3, -1), M, 2, 0.5)
    assert r.tolist() == [-1, -1] and p.tolist() == [-1, -1] and np.isneginf(s).all() and np.isneginf(v).all()
    assert R.select([1.0], [3], M, 1, 0.3) == ([0], [1.0])


# ---------------------------------------------------------------- C-ABI
@pytest.fixture(scope="module")
def lib():
    from multimodal_rag_amd import _native, build

    build.build(verbose=False)
    return _native.lib()


def _call(lib, dtype=1, C=50, k=5, lam=0.5, B=2, d=64, ld=64):
    """mmrag_mmr_select with host buffers standing in for device memory: only for calls the argument checks reject"""
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    return lib.mmrag_mmr_select(p, ld, dtype, d, p, p, B, C, k, lam, p, p, p, p, None, 0, None)


def test_abi_exports_and_size_query(lib):
    raw = ctypes.CDLL(lib._name)
    assert hasattr(raw, "mmrag_mmr_select") and hasattr(raw, "mmrag_mmr_select_workspace_bytes")
    header = open(os.path.join(ROOT, "include", "mmrag.h")).read()
    assert "#define MMRAG_MAX_MMR_CANDIDATES 1024" in header
    from multimodal_rag_amd import _native

    assert _native.MAX_MMR_CANDIDATES == 1024 and lib.mmrag_abi_version() == 1
    for dt in (0, 1, 2):
        assert lib.mmrag_mmr_select_workspace_bytes(256, 50, 768, dt) >= 0


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=6, C=5), dict(C=1025, k=5), dict(C=0, k=0), dict(k=-1),
                                 dict(lam=-0.01), dict(lam=1.5), dict(lam=float("nan")), dict(lam=float("inf")),
                                 dict(dtype=3), dict(dtype=-1)])
def test_abi_bad_arguments_are_einval_without_a_gpu(lib, bad):
    assert _call(lib, **bad) == 1                                    # MMRAG_EINVAL
    assert b"mmr_select" in lib.mmrag_last_error()


# ---------------------------------------------------------------- POST /query with "mmr"
class MmrCollection(FakeCollection):
    """the fake collection plus an mmr_query: the reference selection over the fake's own vectors"""
    calls = []

    def mmr_query(self, query_embeddings, n_results=10, fetch_k=None, lambda_mult=None, where=None, include=()):
        type(self).calls.append({"n_results": n_results, "fetch_k": fetch_k, "lambda_mult": lambda_mult})
        lam = 0.5 if lambda_mult is None else lambda_mult
        C = max(n_results, 50 if fetch_k is None else fetch_k)
        s, r = self.search(query_embeddings, min(C, max(len(self.ids), 1)), where)
        out = {"ids": [], "distances": [], "metadatas": [], "documents": [], "mmr_scores": []}
        for b in range(len(s)):
            pos, val = R.select(s[b], r[b], self.vecs, n_results, lam) if len(self.ids) else ([], [])
            hit = [int(r[b][p]) for p in pos]
            out["ids"].append([self.ids[i] for i in hit])
            out["distances"].append([float(1.0 - s[b][p]) for p in pos])
            out["metadatas"].append([dict(self.metas[i]) for i in hit])
            out["documents"].append([self.docs[i] for i in hit])
            out["mmr_scores"].append(val)
        return out


def _mmr_manager(monkeypatch):
    eng = FakeEngine()
    orig = eng.new_collection

    def new_collection(*a, **kw):
        c = orig(*a, **kw)
        c.__class__ = MmrCollection
        return c

    monkeypatch.setattr(eng, "new_collection", new_collection)
    MmrCollection.calls = []
    return EmbeddingManager(engine=eng)


def _upload(client):
    bodies = ["alpha beta gamma. " * 3, "delta epsilon. " * 3, "zeta eta theta. " * 3, "delta epsilon. " * 3]
    for i, body in enumerate(bodies):
        r = client.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
        assert r.status_code == 200, r.text


def test_query_mmr_with_fake_collection(monkeypatch):
    m = _mmr_manager(monkeypatch)
    assert m.supports_mmr()
    with TestClient(create_app(embedder=m)) as c:
        _upload(c)
        before = m.stats["total_queries"]
        plain = c.post("/query", json={"query": "delta epsilon", "top_k": 3})
        assert plain.status_code == 200 and all("mmr_score" not in s for s in plain.json()["sources"])
        assert c.post("/query", json={"query": "delta epsilon", "top_k": 3, "mmr": False}).json()["sources"] == \
            plain.json()["sources"]
        assert not MmrCollection.calls
        r = c.post("/query", json={"query": "delta epsilon", "top_k": 3, "mmr": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert len(src) == 3 and set(src[0]) == {"rank", "doc_id", "relevance_score", "type", "mmr_score"}
        assert all(isinstance(s["mmr_score"], float) for s in src)
        assert MmrCollection.calls[-1] == {"n_results": 3, "fetch_k": None, "lambda_mult": None}
        assert m.stats["total_queries"] == before + 3
        # lambda 1 through the route: the plain order; the value arrives at the collection
        r1 = c.post("/query", json={"query": "delta epsilon", "top_k": 3, "mmr": True, "mmr_lambda": 1.0})
        assert r1.status_code == 200 and MmrCollection.calls[-1]["lambda_mult"] == 1.0
        assert [s["doc_id"] for s in r1.json()["sources"]] == [s["doc_id"] for s in plain.json()["sources"]]
        # the two uploads with the same text: the plain hits hold both, the diversified ones put the copy last
        assert [s["doc_id"] for s in src] != [s["doc_id"] for s in plain.json()["sources"]]
        assert c.post("/query", json={"query": "delta", "top_k": 2, "mmr": True, "hybrid": True}).status_code == 400
        bad = c.post("/query", json={"query": "delta", "top_k": 2, "mmr": True, "hybrid": True})
        assert "not combined" in bad.json()["detail"]
        assert c.post("/query", json={"query": "delta", "top_k": 2, "mmr": True, "mmr_lambda": 1.5}).status_code == 422
        assert c.post("/query", json={"query": "delta", "top_k": 2, "mmr": True, "mmr_lambda": -0.1}).status_code == 422
    with pytest.raises(ValueError):
        asyncio.run(m.mmr_query("   "))


def test_query_mmr_400_without_mmr_collection():
    m = EmbeddingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=m)) as c:
        _upload(c)
        assert not m.supports_mmr()
        r = c.post("/query", json={"query": "delta", "top_k": 2, "mmr": True})
        assert r.status_code == 400 and "MMR" in r.json()["detail"]
        assert c.post("/query", json={"query": "delta", "top_k": 2}).status_code == 200


def test_manager_mmr_query_and_batch(monkeypatch):
    m = _mmr_manager(monkeypatch)
    asyncio.run(m.initialize())
    items = [{"id": f"t{i}", "type": "text", "summary": t} for i, t in
             enumerate(["alpha beta", "beta alpha", "gamma delta", "epsilon", "alpha gamma"])]
    asyncio.run(m.embed_and_store(items, "doc"))
    one = asyncio.run(m.mmr_query("alpha beta", n_results=3, fetch_k=5, lambda_mult=0.5))
    assert set(one) == {"ids", "distances", "metadatas", "documents", "mmr_scores"} and len(one["ids"]) == 3
    assert MmrCollection.calls[-1] == {"n_results": 3, "fetch_k": 5, "lambda_mult": 0.5}
    n_calls, encodes = len(MmrCollection.calls), len(m._engine.calls)
    many = asyncio.run(m.batch_mmr_query(["alpha beta", "", "gamma"], n_results=3, fetch_k=5, lambda_mult=0.5))
    assert len(MmrCollection.calls) == n_calls + 1                    # one collection call for the whole batch
    assert len(m._engine.calls) == encodes + 1 and m._engine.calls[-1] == 1   # "alpha beta" came from the cache
    # (the fake's CPU scores move in the last bit with the batch size: ids exactly, values to 1e-6)
    assert many[0]["ids"] == one["ids"] and many[0]["mmr_scores"] == pytest.approx(one["mmr_scores"], abs=1e-6)
    assert many[1]["error"] == "Query text cannot be empty" and many[1]["mmr_scores"] == []
    assert len(many[2]["ids"]) == 3


def test_query_mmr_with_rerank(monkeypatch):
    m = _mmr_manager(monkeypatch)

    class Scorer:
        def predict(self, pairs):
            return [float(len(doc) % 7) for _, doc in pairs]

    m._reranker = Scorer()
    with TestClient(create_app(embedder=m)) as c:
        _upload(c)
        r = c.post("/query", json={"query": "delta epsilon", "top_k": 2, "mmr": True, "rerank": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert len(src) == 2 and all("mmr_score" in s and "rerank_score" in s for s in src)
        assert MmrCollection.calls[-1]["n_results"] == 20              # max(top_k, MMRAG_RERANK_CANDIDATES)


# ---------------------------------------------------------------- the kernels
def test_mmr_kernels_no_scratch_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", "-I",
                        os.path.join(ROOT, "include"), os.path.join(ROOT, "multimodal_rag_amd", "csrc", "mmr.hip"),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 6 and all("mmr_select_kernel" in n for n in names), names   # 3 dtypes x (staged, streamed)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] + \
        [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stderr)]
    assert len(scratch) == len(names) and not any(scratch) and not any(spills)
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(lds) == len(names) and max(lds) <= 160 * 1024
