"""Host side of multi-query retrieval: tests/fuse_ref.py against answers written out by hand and a float64 brute force,
the C-ABI entry's exports and argument checks (no GPU: they come before any HIP call), POST /query with "variants" /
"expand" and EmbeddingManager.multi_query through a fake collection, the query expander, and the kernel's resource
usage."""
import asyncio
import ctypes
import os
import re

import numpy as np
import pytest
from fastapi.testclient import TestClient

from multimodal_rag_amd.embedder import EmbeddingManager
from multimodal_rag_amd.server import create_app
from tests import asm_util
from tests import fuse_ref as R
from tests.fakes import FakeCollection, FakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NINF = F(-np.inf)


# ---------------------------------------------------------------- the reference: known answers
def test_reference_known_answers_rrf():
    rows = np.array([[7, 3, 9, -1], [3, 7, 5, 11], [9, 9, 2, 3]], np.int64)      # list 2 holds row 9 twice
    scores = np.array([[.9, .8, .7, -np.inf], [.95, .6, .5, .4], [.3, .3, .2, .1]], F)
    f, r, b, bl, cnt, info = R.fuse_group(scores, rows, None, R.RRF, 60, 8)
    one = lambda rank: F(1) / F(60 + rank)                                       # noqa: E731
    want = {7: (one(1) + one(2), F(.9), 0, 2), 3: ((one(2) + one(1)) + one(4), F(.95), 1, 3),
            9: (one(3) + one(1), F(.7), 0, 2), 5: (one(3), F(.5), 1, 1), 11: (one(4), F(.4), 1, 1),
            2: (one(3), F(.2), 2, 1)}
    assert info.tolist() == [6, 11]                                              # 3 + 4 + 4 entries before a list's end
    assert r.tolist() == [3, 7, 9, 5, 2, 11, -1, -1]                             # 5 and 2 tie on fused: best decides
    for j, row in enumerate(r[:6].tolist()):
        assert (f[j], b[j], bl[j], cnt[j]) == want[row], (row, f[j], want[row])
        assert f[j].dtype == F
    assert np.isneginf(f[6:]).all() and np.isneginf(b[6:]).all() and bl[6:].tolist() == [-1, -1] and cnt[6:].tolist() == [0, 0]
    # n smaller than what exists; weights: list 1 counts double, list 2 not at all, list 0 against
    f, r, *_ = R.fuse_group(scores, rows, np.array([-1, 2, 0], F), R.RRF, 0, 3)
    assert r.tolist() == [3, 5, 11]
    assert f.tolist() == [(F(-1) / F(2) + F(2) / F(1)) + F(0) / F(4), F(2) / F(3), F(2) / F(4)]


def test_reference_known_answers_max_and_tie_keys():
    rows = np.array([[1, 2, 3], [3, 2, 4]], np.int64)
    scores = np.array([[.5, .25, .125], [.5, .25, .0625]], F)
    f, r, b, bl, cnt, info = R.fuse_group(scores, rows, np.array([1, 2], F), R.MAX, 60, 5)
    assert r.tolist() == [3, 1, 2, 4, -1] and f[:4].tolist() == [1.0, .5, .5, .125]     # 1 and 2 tie: best .5 > .25
    assert bl[:4].tolist() == [1, 0, 0, 1] and cnt[:4].tolist() == [2, 1, 2, 1] and b[0] == F(.5) and info.tolist() == [4, 6]
    # all three keys: equal fused and equal best fall to the lower row; -0.0 ties with 0.0 and falls through
    rows = np.array([[40, 30, 20, 10]], np.int64)
    f, r, b, *_ = R.fuse_group(np.array([[0.0, -0.0, 0.0, -0.0]], F), rows, None, R.MAX, 60, 4)
    assert r.tolist() == [10, 20, 30, 40] and np.signbit(f).tolist() == [True, False, True, False]
    assert np.signbit(b).tolist() == [True, False, True, False]                  # bits copied, not canonicalised
    # an empty group, an entirely empty list, ties of best go to the lower list
    out = R.fuse_group(np.zeros((0, 4), F), np.zeros((0, 4), np.int64), None, R.RRF, 60, 2)
    assert out[1].tolist() == [-1, -1] and out[5].tolist() == [0, 0]
    out = R.fuse_group(np.array([[1, 1], [.5, .25]], F), np.array([[-1, 8], [8, 9]], np.int64), None, R.RRF, 60, 2)
    assert out[1].tolist() == [8, 9] and out[4].tolist() == [1, 1] and out[5].tolist() == [2, 2] and out[3].tolist() == [1, 1]
    out = R.fuse_group(np.array([[.5], [.5]], F), np.array([[8], [8]], np.int64), None, R.MAX, 60, 1)
    assert out[3].tolist() == [0] and out[4].tolist() == [2]
    # the stacked form: ragged groups, one of them without lists
    rows = np.array([[1, 2], [2, 3], [5, 6]], np.int64)
    scores = np.array([[.9, .8], [.7, .6], [.5, .4]], F)
    f, r, *_, info = R.fuse_select(scores, rows, [0, 2, 2, 3], 2, method="rrf", rrf_k=1)
    assert r.tolist() == [[2, 1], [-1, -1], [5, 6]] and info.tolist() == [[3, 4], [0, 0], [2, 2]]
    assert f[0, 0] == F(1) / F(3) + F(1) / F(2)


def random_group(g, nl, C, pool, ties):
    rows = np.stack([g.choice(pool, C, replace=False) for _ in range(nl)]).astype(np.int64) if nl else \
        np.zeros((0, C), np.int64)
    scores = -np.sort(-g.standard_normal((nl, C)).astype(F), axis=1)
    if ties:
        scores = (np.round(scores * 2) / 2).astype(F)
    for l in range(nl):
        kind = int(g.integers(0, 5))
        if kind == 0:
            cut = int(g.integers(0, C + 1))
            rows[l, cut:], scores[l, cut:] = -1, -np.inf
        elif kind == 1 and C > 2:
            rows[l, C - 1] = rows[l, 0]                                          # a duplicate inside one list
    return scores, rows


@pytest.mark.parametrize("seed", range(10))
def test_reference_agrees_with_the_float64_brute_force(seed):
    g = np.random.default_rng(seed)
    for _ in range(20):
        nl, C = int(g.integers(0, 7)), int(g.integers(1, 40))
        scores, rows = random_group(g, nl, C, int(g.integers(C, 4 * C + 2)), bool(g.integers(0, 2)))
        weights = [None, g.integers(-1, 3, nl).astype(F), g.random(nl).astype(F)][int(g.integers(0, 3))]
        for method in (R.RRF, R.MAX):
            for n in (1, 5, 4096):
                f, r, b, bl, cnt, info = R.fuse_group(scores, rows, weights, method, 60, n)
                exact = R.brute_force(scores, rows, weights, method, 60)
                found = int(info[0])
                assert found == len(exact) and (r[min(found, n):] == -1).all()
                got = r[: min(found, n)].tolist()
                assert len(set(got)) == len(got) and set(got) <= set(exact)
                for j, row in enumerate(got):
                    ef, eb, el, ec = exact[row]
                    assert abs(float(f[j]) - ef) <= 1e-5 * max(1.0, abs(ef)) and float(b[j]) == eb
                    assert (int(bl[j]), int(cnt[j])) == (el, ec)
                # ordered by the definition's own keys, and nothing left out outranks what was returned
                keys = [(-float(f[j]), -float(b[j]), row) for j, row in enumerate(got)]
                assert keys == sorted(keys)
                if got and found > n:
                    worst = float(f[len(got) - 1])
                    assert all(exact[row][0] <= worst + 1e-5 * max(1.0, abs(worst)) for row in set(exact) - set(got))


# ---------------------------------------------------------------- C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from multimodal_rag_amd import _native, build

    build.build(verbose=False)
    return _native.lib()


def _call(lib, L=4, C=50, G=2, method=0, rrf_k=60, n=5, null_out=False, null_off=False, null_lists=False):
    """mmrag_fuse_select with host buffers standing in for device memory: only for calls the argument checks reject"""
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    return lib.mmrag_fuse_select(None if null_lists else p, p, L, C, None if null_off else p, G, None, method, rrf_k,
                                 n, None if null_out else p, p, p, p, p, p, None)


def test_abi_exports_and_limits(lib):
    from multimodal_rag_amd import _native

    assert hasattr(ctypes.CDLL(lib._name), "mmrag_fuse_select") and lib.mmrag_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "mmrag.h")).read()
    for line in ("#define MMRAG_MAX_FUSE_LISTS 16", "#define MMRAG_MAX_FUSE_CANDIDATES 256",
                 "#define MMRAG_MAX_FUSE_RESULTS 4096", "#define MMRAG_FUSE_RRF 0", "#define MMRAG_FUSE_MAX 1"):
        assert line in header
    assert (_native.MAX_FUSE_LISTS, _native.MAX_FUSE_CANDIDATES, _native.MAX_FUSE_RESULTS) == (16, 256, 4096)
    assert _native.FUSE_METHODS == {"rrf": 0, "max": 1} == R.METHODS
    assert (R.MAX_LISTS, R.MAX_CANDIDATES, R.MAX_RESULTS) == (16, 256, 4096)


@pytest.mark.parametrize("bad", [dict(G=0), dict(G=-3), dict(C=0), dict(C=257), dict(C=-1), dict(n=0), dict(n=4097),
                                 dict(n=-1), dict(rrf_k=-1), dict(method=2), dict(method=-1), dict(L=-1),
                                 dict(null_out=True), dict(null_off=True), dict(null_lists=True)])
def test_abi_bad_arguments_are_einval_without_a_gpu(lib, bad):
    assert _call(lib, **bad) == 1                                    # MMRAG_EINVAL
    assert b"fuse_select" in lib.mmrag_last_error()


def test_native_wrapper_refuses_host_tensors(lib):
    import torch

    from multimodal_rag_amd import _native

    s, r = torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(_native.MMRagNativeError):
        _native.fuse_select(s, r, [0, 2], 3)
    with pytest.raises(_native.MMRagNativeError):
        _native.fuse_select(s, r, [0, 2], 3, weights=torch.ones(2))


# ---------------------------------------------------------------- the manager and POST /query over a fake collection
class FusedCollection(FakeCollection):
    """the fake collection plus a fused_query: the reference over the fake's own exact per-variant rankings"""
    calls = []

    def fused_query(self, query_embeddings, list_off, n_results=10, fetch_k=None, weights=None, method=None,
                    where=None, include=()):
        q = np.asarray(query_embeddings, np.float32).reshape(-1, self.dim)
        type(self).calls.append({"rows": len(q), "list_off": list(list_off), "n_results": n_results,
                                 "weights": None if weights is None else list(weights), "method": method})
        C = min(max(n_results, 50) if fetch_k is None else fetch_k, 256)
        s, r = self.search(q, C, where)
        f, rows, best, bl, cnt, _ = R.fuse_select(s.astype(F), r, list_off, n_results,
                                                  None if weights is None else np.asarray(weights, F),
                                                  method or "rrf", 60)
        out = {key: [] for key in ("ids", "distances", "metadatas", "documents", "fused_scores", "matched_queries",
                                   "best_query")}
        for g in range(len(list_off) - 1):
            hit = [int(x) for x in rows[g] if x >= 0]
            k = len(hit)
            out["ids"].append([self.ids[i] for i in hit])
            out["distances"].append([float(1.0 - x) for x in best[g][:k]])
            out["metadatas"].append([dict(self.metas[i]) for i in hit])
            out["documents"].append([self.docs[i] for i in hit])
            out["fused_scores"].append([float(x) for x in f[g][:k]])
            out["matched_queries"].append([int(x) for x in cnt[g][:k]])
            out["best_query"].append([int(x) for x in bl[g][:k]])
        return out


def _fused_manager(monkeypatch):
    eng = FakeEngine()
    orig = eng.new_collection

    def new_collection(*a, **kw):
        c = orig(*a, **kw)
        c.__class__ = FusedCollection
        return c

    monkeypatch.setattr(eng, "new_collection", new_collection)
    FusedCollection.calls = []
    return EmbeddingManager(engine=eng)


def _upload(client):
    bodies = [" ".join(f"alpha beta gamma number {i}." for i in range(40)), "delta epsilon. " * 3,
              "alpha beta once. " * 3, "zeta eta theta. " * 3]
    for i, body in enumerate(bodies):
        r = client.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
        assert r.status_code == 200, r.text


class StubExpander:
    def __init__(self, lines):
        self.lines, self.asked = lines, []

    async def expand(self, question, n):
        self.asked.append((question, n))
        return self.lines[:n]


class StubReranker:
    def __init__(self):
        self.pairs = []

    def predict(self, pairs):
        self.pairs.append(list(pairs))
        return [float(len(d)) for _, d in pairs]


PLAIN_KEYS = {"rank", "doc_id", "relevance_score", "type"}


def test_query_with_variants_through_a_fake_collection(monkeypatch):
    m = _fused_manager(monkeypatch)
    assert m.supports_multi_query()
    expander = StubExpander(["delta epsilon", "alpha beta gamma", "zeta eta"])
    with TestClient(create_app(embedder=m, query_expander=expander)) as c:
        _upload(c)
        before = m.stats["total_queries"]
        plain = c.post("/query", json={"query": "alpha beta gamma", "top_k": 3})
        assert plain.status_code == 200 and all(set(s) == PLAIN_KEYS for s in plain.json()["sources"])
        assert not FusedCollection.calls
        r = c.post("/query", json={"query": "alpha beta gamma", "top_k": 4,
                                   "variants": ["delta epsilon", "zeta eta theta"]})
        assert r.status_code == 200, r.text
        call = FusedCollection.calls[-1]
        assert call == {"rows": 3, "list_off": [0, 3], "n_results": 4, "weights": None, "method": None}
        src = r.json()["sources"]
        assert len(src) == 4 and all(set(s) == PLAIN_KEYS | {"fused_score", "matched_queries"} for s in src)
        assert [s["fused_score"] for s in src] == sorted((s["fused_score"] for s in src), reverse=True)
        assert all(1 <= s["matched_queries"] <= 3 for s in src) and [s["rank"] for s in src] == [1, 2, 3, 4]
        # `query` is list 0 and weighs 1.0; the further phrasings get `variant_weight`; `fusion` is handed on
        enc = m._engine.calls[:]
        r = c.post("/query", json={"query": "alpha beta gamma", "top_k": 2, "variants": ["delta epsilon"],
                                   "variant_weight": 0.25, "fusion": "max"})
        assert r.status_code == 200, r.text
        assert FusedCollection.calls[-1] == {"rows": 2, "list_off": [0, 2], "n_results": 2, "weights": [1.0, 0.25],
                                             "method": "max"}
        assert m._engine.calls == enc                                             # both phrasings came from the cache
        only = c.post("/query", json={"query": "alpha beta gamma", "top_k": 2, "variants": ["delta epsilon"],
                                      "variant_weight": 0.0, "fusion": "max"}).json()["sources"]
        assert [s["doc_id"] for s in only] == [s["doc_id"] for s in plain.json()["sources"][:2]]
        # an empty list is multi-query retrieval over `query` alone; a phrasing equal to `query` is searched once
        r = c.post("/query", json={"query": "alpha beta gamma", "top_k": 2, "variants": []})
        assert r.status_code == 200 and FusedCollection.calls[-1]["list_off"] == [0, 1]
        assert all(s["matched_queries"] == 1 for s in r.json()["sources"])
        r = c.post("/query", json={"query": "alpha beta gamma", "top_k": 2, "variants": ["alpha beta gamma", "x y"]})
        assert r.status_code == 200 and FusedCollection.calls[-1]["list_off"] == [0, 2]
        # unsupported combinations and bad fields
        for other in ("mmr", "hybrid", "group_by_document"):
            bad = c.post("/query", json={"query": "alpha", "top_k": 2, "variants": ["beta"], other: True})
            assert bad.status_code == 400 and "not combined" in bad.json()["detail"], other
            bad = c.post("/query", json={"query": "alpha", "top_k": 2, "expand": 2, other: True})
            assert bad.status_code == 400 and "not combined" in bad.json()["detail"], other
        for body in ({"variants": ["v"] * 16}, {"variants": [""]}, {"variants": ["x" * 2001]}, {"fusion": "sum"},
                     {"expand": 16}, {"expand": -1}, {"variants": "beta"}):
            assert c.post("/query", json={"query": "alpha", **body}).status_code == 422, body
        # expansion through the application's expander; its repeat of the question is dropped
        r = c.post("/query", json={"query": "alpha beta gamma", "top_k": 3, "expand": 3})
        assert r.status_code == 200, r.text
        assert expander.asked == [("alpha beta gamma", 3)] and FusedCollection.calls[-1]["list_off"] == [0, 3]
        r = c.post("/query", json={"query": "alpha beta gamma", "top_k": 3, "expand": 1, "variants": ["zeta eta"]})
        assert r.status_code == 200 and FusedCollection.calls[-1]["list_off"] == [0, 3]
        assert all("fused_score" in s for s in r.json()["sources"])
        assert m.stats["total_queries"] == before + 8
    with TestClient(create_app(embedder=m)) as c:                                 # no expander installed
        r = c.post("/query", json={"query": "alpha", "expand": 2})
        assert r.status_code == 400 and "expansion is not configured" in r.json()["detail"]
        assert c.post("/query", json={"query": "alpha", "expand": 0}).status_code == 200


def test_variants_with_rerank_reranks_against_query(monkeypatch):
    m = _fused_manager(monkeypatch)
    m._reranker = StubReranker()
    with TestClient(create_app(embedder=m)) as c:
        _upload(c)
        r = c.post("/query", json={"query": "alpha beta gamma", "top_k": 3, "variants": ["delta epsilon"],
                                   "rerank": True})
        assert r.status_code == 200, r.text
        from multimodal_rag_amd.config import settings

        assert FusedCollection.calls[-1]["n_results"] == max(3, settings.MMRAG_RERANK_CANDIDATES)
        pairs = m._reranker.pairs[-1]
        assert pairs and {q for q, _ in pairs} == {"alpha beta gamma"}            # never a variant
        src = r.json()["sources"]
        assert len(src) == 3 and all(set(s) == PLAIN_KEYS | {"fused_score", "matched_queries", "rerank_score"} for s in src)
        assert [s["rerank_score"] for s in src] == sorted((s["rerank_score"] for s in src), reverse=True)
        fused = asyncio.run(m.multi_query(["alpha beta gamma", "delta epsilon"],
                                          n_results=max(3, settings.MMRAG_RERANK_CANDIDATES)))
        of_id = dict(zip(fused["ids"], zip(fused["fused_scores"], fused["matched_queries"])))
        assert all((s["fused_score"], s["matched_queries"]) == of_id[s["doc_id"]] for s in src)


def test_variants_400_without_a_multi_query_embedder():
    m = EmbeddingManager(engine=FakeEngine())                                    # a collection without fused_query
    with TestClient(create_app(embedder=m, query_expander=StubExpander(["x"]))) as c:
        _upload(c)
        assert not m.supports_multi_query()
        for body in ({"variants": ["epsilon"]}, {"expand": 1}, {"variants": []}):
            r = c.post("/query", json={"query": "delta", "top_k": 2, **body})
            assert r.status_code == 400 and "Multi-query retrieval is not available" in r.json()["detail"]
        assert c.post("/query", json={"query": "delta", "top_k": 2}).status_code == 200

    class NoMulti:                                                      # an embedder without multi_query at all
        def __getattr__(self, name):
            if name in ("multi_query", "supports_multi_query"):
                raise AttributeError(name)
            return getattr(m, name)

    with TestClient(create_app(embedder=NoMulti())) as c:
        r = c.post("/query", json={"query": "delta", "top_k": 2, "variants": ["epsilon"]})
        assert r.status_code == 400 and "Multi-query retrieval is not available" in r.json()["detail"]
    with pytest.raises(ValueError, match="single-GPU collection"):
        asyncio.run(m.multi_query(["delta", "epsilon"]))


def test_manager_multi_query_and_batch(monkeypatch):
    m = _fused_manager(monkeypatch)
    asyncio.run(m.initialize())
    for doc, texts in (("docA", ["alpha beta", "beta alpha", "alpha gamma"]), ("docB", ["gamma delta", "epsilon"])):
        items = [{"id": f"{doc}_t{i}", "type": "text", "summary": t} for i, t in enumerate(texts)]
        asyncio.run(m.embed_and_store(items, doc))
    before = m.stats["total_queries"]
    one = asyncio.run(m.multi_query(["alpha beta", "epsilon"], n_results=4))
    assert set(one) == {"ids", "distances", "metadatas", "documents", "fused_scores", "matched_queries", "best_query"}
    assert len(one["ids"]) == 4 == len(one["fused_scores"]) == len(one["matched_queries"]) == len(one["best_query"])
    assert one["matched_queries"] == [2] * 4 and set(one["best_query"]) <= {0, 1}    # 5 rows, both lists hold them all
    assert one["fused_scores"] == sorted(one["fused_scores"], reverse=True)
    assert m.stats["total_queries"] == before + 1
    # the same through the reference over the manager's own per-variant hits
    per = asyncio.run(m.batch_query(["alpha beta", "epsilon"], n_results=5))
    rrf = {}
    for hits in per:
        for rank, i in enumerate(hits["ids"], 1):
            rrf[i] = rrf.get(i, F(0)) + F(1) / F(60 + rank) if i in rrf else F(1) / F(60 + rank)
    assert [rrf[i] for i in one["ids"]] == one["fused_scores"]
    # the batch: one encoder pass for the misses, one collection call; failures are 'error' dicts
    n_calls, encodes = len(FusedCollection.calls), len(m._engine.calls)
    many = asyncio.run(m.batch_multi_query([["alpha beta", "epsilon"], [], ["gamma", " "], ["gamma", "delta", "beta"]],
                                           n_results=4, weights=[None, None, None, [1.0, 0.5, 0.5]]))
    assert len(FusedCollection.calls) == n_calls + 1 and len(m._engine.calls) == encodes + 1
    assert m._engine.calls[-1] == 3                                               # gamma, delta, beta; two were cached
    assert FusedCollection.calls[-1]["list_off"] == [0, 2, 5]
    assert FusedCollection.calls[-1]["weights"] == [1.0, 1.0, 1.0, 0.5, 0.5]
    assert {k: v for k, v in many[0].items() if k != "distances"} == {k: v for k, v in one.items() if k != "distances"}
    assert np.allclose(many[0]["distances"], one["distances"], atol=1e-6)        # the fake's matmul varies with the batch
    for at in (1, 2):
        assert many[at]["error"] == "Query text cannot be empty" and many[at]["ids"] == [] == many[at]["fused_scores"]
    assert len(many[3]["ids"]) == 4 and max(many[3]["matched_queries"]) == 3
    assert m.stats["total_queries"] == before + 1 + 2 + 2                         # batch_query's two and the two live
    # empty input: query()'s own error
    for bad in ([], [""], ["alpha", "  "], "alpha"):
        with pytest.raises(ValueError, match="Query text cannot be empty"):
            asyncio.run(m.multi_query(bad))
    with pytest.raises(ValueError, match="Query text cannot be empty"):
        asyncio.run(m.query(""))
    with pytest.raises(ValueError, match="at most 16"):
        asyncio.run(m.multi_query(["q%d" % i for i in range(17)]))
    # a failing collection call: every live question of the batch carries the reason
    m.collection.fused_query = lambda *a, **kw: (_ for _ in ()).throw(RuntimeError("boom"))
    m.max_retries, m._sleep = 1, (lambda s: None)
    failed = asyncio.run(m.batch_multi_query([["alpha"], []]))
    assert "boom" in failed[0]["error"] and failed[1]["error"] == "Query text cannot be empty"


def test_llm_query_expander_parses_lines():
    from multimodal_rag_amd.ingest import LLMQueryExpander

    class Gen:
        prompts = []

        async def generate_text(self, prompt, max_tokens=1000, temperature=0.7):
            self.prompts.append(prompt)
            return "1. What is ML?\n\n- how do machines learn\nWhat is ML?\nwhat is machine learning\n  \n* Fourth one\nfifth"

    gen = Gen()
    ex = LLMQueryExpander(gen)
    got = asyncio.run(ex.expand("What is machine learning", 4))
    assert got == ["What is ML?", "how do machines learn", "Fourth one", "fifth"]     # blank, repeat, the question: gone
    assert len(gen.prompts) == 1 and "What is machine learning" in gen.prompts[0] and "4" in gen.prompts[0]
    assert asyncio.run(ex.expand("q", 2)) == ["What is ML?", "how do machines learn"]
    assert asyncio.run(ex.expand("q", 0)) == [] and len(gen.prompts) == 2


# ---------------------------------------------------------------- the kernel
def test_fuse_kernel_no_scratch_no_spills(tmp_path):
    asm = asm_util.compile_asm("fuse.hip", tmp_path)
    names = [n for n in asm_util.bodies(asm) if "kernel" in n]
    assert len(names) == 1 and "fuse_select_kernel" in names[0], names
    body = asm_util.bodies(asm)[names[0]]
    assert not [l for l in body if re.match(r"(scratch_|buffer_(load|store)\S* .*offen)", l)]
    for field, want in (("private_segment_fixed_size", 0), ("sgpr_spill_count", 0), ("vgpr_spill_count", 0)):
        vals = [int(x) for x in re.findall(r"\.%s:\s*(\d+)" % field, asm)]
        assert vals == [want], (field, vals)
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)]
    assert len(lds) == 1 and lds[0] <= 64 * 1024                       # two workgroups per CU
