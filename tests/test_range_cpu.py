"""No GPU: range retrieval's reference (tests/range_ref.py) against a brute-force loop, the argument refusals of
_native.range_scan, and the host side -- VectorIndex's facet formatting, EmbeddingManager.range_query and POST /explore
over a fake collection."""
import asyncio

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

from multimodal_rag_amd.index import match_where
from tests import range_ref as R
from tests.fakes import FakeCollection, FakeEngine


# ---------------------------------------------------------------- the reference
def brute(q, rows, thr, limit, vis, codes, sizes):
    B, n = len(q), len(rows)
    counts, tables, hits = [], [np.zeros((B, G + 1), np.int64) for G in sizes], []
    for b in range(B):
        passing = []
        for r in range(n):
            s = float(np.dot(q[b].astype(np.float64), rows[r].astype(np.float64)))
            if (vis is None or vis[b][r]) and s >= thr[b]:
                passing.append((-s, r))
                for c, G in enumerate(sizes):
                    g = int(codes[c][r])
                    tables[c][b, g if 0 <= g < G else G] += 1
        counts.append(len(passing))
        hits.append([(r, -s) for s, r in sorted(passing)[:limit]])
    return counts, tables, hits


@pytest.mark.parametrize("n,B,limit", [(1, 1, 3), (37, 4, 5), (200, 3, 0), (200, 3, 250)])
def test_reference_equals_a_brute_force_loop(n, B, limit):
    g = np.random.default_rng(n + limit)
    rows = g.integers(-2, 3, (n, 8)).astype(np.float32)
    q = g.integers(-2, 3, (B, 8)).astype(np.float32)
    thr = np.array([0.0, -3.0, 2.0, 100.0][:B])           # on values many rows hit exactly; one above every score
    vis = g.random((B, n)) > 0.3
    codes = [g.integers(-1, 5, n), g.integers(0, 2, n)]    # -1 and codes at and past G among them
    sizes = [3, 1]
    for v in (None, vis):
        counts, tables, s, r = R.range_ref(q, rows, thr, limit, v, codes, sizes)
        bc, bt, bh = brute(q, rows, thr, limit, v, codes, sizes)
        assert counts.tolist() == bc
        for t, e in zip(tables, bt):
            assert np.array_equal(t, e)
            assert np.array_equal(t.sum(axis=1), counts)    # every column's slots sum to the count
        for b in range(B):
            m = len(bh[b])
            assert r[b, :m].tolist() == [x for x, _ in bh[b]] and np.all(r[b, m:] == -1)
            assert np.allclose(s[b, :m], [y for _, y in bh[b]]) and np.all(np.isneginf(s[b, m:]))
    assert R.range_ref(q, rows, 100.0, 4)[0].tolist() == [0] * B
    assert R.range_ref(q, rows, -1e9, 0, None, [codes[0]], [3])[1][0].sum() == B * n


def test_reference_ties_go_to_the_lower_row_and_row_offset():
    rows = np.array([[1.0, 0], [0, 1], [1, 0], [1, 0]], np.float32)
    counts, _, s, r = R.range_ref(np.array([[1.0, 0]], np.float32), rows, 1.0, 2, row_offset=10)
    assert counts.tolist() == [3] and r.tolist() == [[10, 12]] and s.tolist() == [[1.0, 1.0]]


def test_gap_threshold_picks_the_nearest_wide_gap():
    s = np.array([0.9, 0.5, 0.4999, 0.3, 0.2999, 0.1])
    t = R.gap_threshold(s, 2)
    assert 0.5 < t < 0.9 and (s >= t).sum() == 1           # the gap after 2 rows is too narrow: the one after 1 is nearest
    assert (s >= R.gap_threshold(s, 3)).sum() == 3
    assert (s >= R.gap_threshold(s, 6)).sum() == 5
    with pytest.raises(AssertionError):
        R.gap_threshold(np.array([0.5, 0.4999, 0.4998]), 1)


# ---------------------------------------------------------------- _native.range_scan refuses before the device is asked
def test_native_range_scan_refusals():
    from multimodal_rag_amd import _native as N

    q, rows = torch.zeros((2, 64)), torch.zeros((8, 64))
    assert N.MAX_FACET_COLUMNS == 4
    with pytest.raises(N.MMRagNativeError, match="device"):          # no CPU fallback
        N.range_scan(q, rows, 8, 64, 0.5, 5)
    with pytest.raises(N.MMRagNativeError, match="device"):
        N.range_scan(q, rows, 8, 64, 0.5, 0, [torch.zeros(8, dtype=torch.int32)], [3])
    for limit in (-1, N.MAX_K_DEEP + 1):
        with pytest.raises(ValueError, match="limit"):
            N.range_scan(q, rows, 8, 64, 0.5, limit)
    cols = [torch.zeros(8, dtype=torch.int32)] * 5
    with pytest.raises(N.MMRagNativeError, match="at most 4"):
        N.range_scan(q, rows, 8, 64, 0.5, 5, cols, [1] * 5)
    with pytest.raises(N.MMRagNativeError, match="facet_sizes"):
        N.range_scan(q, rows, 8, 64, 0.5, 5, cols[:2], [1])
    with pytest.raises(N.MMRagNativeError, match="facet_sizes"):
        N.range_scan(q, rows, 8, 64, 0.5, 5, cols[:1], [-1])


def test_workspace_bytes_is_zero_out_of_range():
    from multimodal_rag_amd import _native as N, build

    build.build(verbose=False)
    assert N.range_scan_workspace_bytes(4, 1000, 10, 7) > 0
    assert N.range_scan_workspace_bytes(4, 1000, 0, 0) > 0
    assert N.range_scan_workspace_bytes(4, 1000, 0) < N.range_scan_workspace_bytes(4, 1000, 1)    # no candidate slots
    for bad in ((0, 1000, 10, 0), (4, -1, 10, 0), (4, 1 << 31, 10, 0), (4, 1000, -1, 0), (4, 1000, 4097, 0),
                (4, 1000, 10, -1)):
        assert N.range_scan_workspace_bytes(*bad) == 0


def test_setting_is_a_budget_with_a_default():
    from multimodal_rag_amd.config import Settings

    assert Settings().MMRAG_RANGE_TABLE_BYTES == 256 << 20


# ---------------------------------------------------------------- VectorIndex's facet lists
def test_facet_lists_order_and_missing_slot():
    from multimodal_rag_amd.index import VectorIndex

    table = np.array([[2, 0, 5, 2, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 3]])
    out = VectorIndex._facet_lists(table, ["a", "b", "c", "d"])
    assert out[0] == [{"value": "c", "count": 5}, {"value": "a", "count": 2}, {"value": "d", "count": 2},
                      {"value": None, "count": 1}]                     # count descending, then first appearance
    assert out[1] == [] and out[2] == [{"value": None, "count": 3}]


# ---------------------------------------------------------------- EmbeddingManager and POST /explore over a stand-in
class RangeCollection(FakeCollection):
    """FakeCollection with VectorIndex.range_query's result, from the reference"""

    def range_query(self, query_embeddings, threshold, limit=100, wheres=None, facets=(),
                    include=("metadatas", "documents", "distances")):
        q = np.asarray(query_embeddings, np.float32).reshape(-1, self.dim)
        B, n = len(q), len(self.ids)
        wheres = [wheres] * B if wheres is None or isinstance(wheres, dict) else list(wheres)
        vis = np.array([[match_where(m, w) for m in self.metas] for w in wheres], bool).reshape(B, n)
        values, codes = [], []
        for key in facets:
            seen = {}
            codes.append(np.array([seen.setdefault(m[key], len(seen)) if key in m else -1 for m in self.metas], np.int64))
            values.append(list(seen))
        counts, tables, s, r = R.range_ref(q, self.vecs, threshold, limit, vis, codes, [len(v) for v in values])
        out = {"ids": [], "distances": [], "metadatas": [], "documents": [], "total": counts.tolist(),
               "truncated": [int(c) > limit for c in counts], "facets": []}
        for b in range(B):
            hit = [int(x) for x in r[b] if x >= 0]
            out["ids"].append([self.ids[i] for i in hit])
            out["distances"].append([float(1.0 - s[b, j]) for j in range(len(hit))])
            out["metadatas"].append([dict(self.metas[i]) for i in hit])
            out["documents"].append([self.docs[i] for i in hit])
            per_key = {}
            for key, vals, t in zip(facets, values, tables):
                nz = [g for g in np.argsort(-t[b], kind="stable").tolist() if t[b, g]]
                per_key[key] = [{"value": vals[g] if g < len(vals) else None, "count": int(t[b, g])} for g in nz]
            out["facets"].append(per_key)
        return out


class RangeEngine(FakeEngine):
    def new_collection(self, name, metadata=None):
        c = RangeCollection(self.dim, name, metadata)
        self.collections.append(c)
        return c


def make_manager(engine):
    from multimodal_rag_amd.embedder import EmbeddingManager

    async def no_sleep(_):
        return None

    manager = EmbeddingManager(engine=engine)
    manager._sleep = no_sleep
    return manager


def store(engine, col):
    """doc "da": 6 text chunks and one table that all say the same; doc "db": 2 of them again, one without a type"""
    same = ["the same words"] * 9
    metas = ([{"doc_id": "da", "type": "text"}] * 6 + [{"doc_id": "da", "type": "table"}]
             + [{"doc_id": "db", "type": "text"}, {"doc_id": "db"}])
    col.add(engine.encode(same), documents=same, metadatas=metas, ids=[f"same{i}" for i in range(9)])
    other = [f"something else {i}" for i in range(5)]
    col.add(engine.encode(other), documents=other, metadatas=[{"doc_id": "dc", "type": "text"}] * 5,
            ids=[f"other{i}" for i in range(5)])


def test_manager_range_query(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    engine = RangeEngine()
    m = make_manager(engine)

    async def go():
        await m.initialize()
        assert m.supports_range()
        store(engine, engine.collections[-1])
        with pytest.raises(ValueError, match="empty"):
            await m.range_query(" ", 0.5)
        out = await m.range_query("the same words", 0.9, limit=4, facets=["doc_id", "type"])
        assert out["total"] == 9 and out["truncated"] is True and out["ids"] == [f"same{i}" for i in range(4)]
        assert out["facets"] == {"doc_id": [{"value": "da", "count": 7}, {"value": "db", "count": 2}],
                                 "type": [{"value": "text", "count": 7}, {"value": "table", "count": 1},
                                          {"value": None, "count": 1}]}
        none = await m.range_query("the same words", 0.9, limit=0, facets=["type"], filter_dict={"doc_id": "db"})
        assert none["total"] == 2 and none["ids"] == [] and none["truncated"] is True
        assert none["facets"] == {"type": [{"value": "text", "count": 1}, {"value": None, "count": 1}]}
        low = await m.range_query("the same words", -1.0, limit=20)
        assert low["total"] == 14 and low["truncated"] is False and low["facets"] == {}
        calls = len(engine.calls)
        many = await m.batch_range_query(["the same words", "", "something else 0"], [0.9, 0.9, 0.99], limit=3,
                                         facets=["doc_id"])
        assert len(engine.calls) == calls + 1 and engine.calls[-1] == 1      # one encode call; the first text was cached
        assert [a["total"] for a in many] == [9, 0, 1] and "empty" in many[1]["error"] and many[1]["facets"] == {}
        assert many[2]["facets"] == {"doc_id": [{"value": "dc", "count": 1}]}
        await m.cleanup()

    asyncio.run(go())
    plain = make_manager(FakeEngine())      # a collection without range_query (the sharded path's): refused

    async def refused():
        await plain.initialize()
        assert not plain.supports_range()
        with pytest.raises(ValueError, match="single-GPU"):
            await plain.range_query("x", 0.5)
        await plain.cleanup()

    asyncio.run(refused())


def test_explore_route(monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.server import create_app

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    engine = RangeEngine()
    with TestClient(create_app(embedder=make_manager(engine))) as c:
        store(engine, engine.collections[-1])
        r = c.post("/explore", json={"query": "the same words", "min_score": 0.9, "limit": 3,
                                     "facets": ["doc_id", "type"]})
        assert r.status_code == 200, r.text
        body = r.json()
        assert set(body) == {"total", "truncated", "hits", "facets", "processing_time"}
        assert body["total"] == 9 and body["truncated"] is True
        assert [h["doc_id"] for h in body["hits"]] == ["same0", "same1", "same2"]
        assert all(set(h) == {"rank", "doc_id", "relevance_score", "type"} and h["relevance_score"] == 1.0
                   for h in body["hits"])
        assert body["facets"]["doc_id"] == [{"value": "da", "count": 7}, {"value": "db", "count": 2}]
        assert body["facets"]["type"][-1] == {"value": None, "count": 1}
        # nothing relevant: a count of zero, no hits, empty facet lists
        r = c.post("/explore", json={"query": "never stored", "min_score": 0.99, "facets": ["type"]})
        assert r.status_code == 200 and r.json()["total"] == 0 and r.json()["hits"] == []
        assert r.json()["facets"] == {"type": []} and r.json()["truncated"] is False
        # the numbers alone, restricted by a filter and by documents
        r = c.post("/explore", json={"query": "the same words", "min_score": 0.9, "limit": 0, "facets": ["type"],
                                     "filter": {"type": "text"}, "doc_ids": ["da", "dc"]})
        assert r.status_code == 200 and r.json()["total"] == 6 and r.json()["hits"] == []
        assert r.json()["facets"] == {"type": [{"value": "text", "count": 6}]}
        ok = {"query": "q", "min_score": 0.5}
        for bad in ({"min_score": 1.5}, {"min_score": -1.0}, {"facets": ["a", "b", "c", "d", "e"]}, {"limit": 101},
                    {"limit": -1}, {"query": ""}):
            assert c.post("/explore", json={**ok, **bad}).status_code == 422, bad
        assert c.post("/explore", json={"query": "q"}).status_code == 422        # min_score is required
        assert c.post("/explore", json={**ok, "facets": ["a", "a"]}).status_code == 400
        assert c.post("/explore", json={**ok, "filter": {"page": {"$between": 1}}}).status_code == 400
    # an embedder whose collection cannot: 400 with a clear message, no other way of answering
    with TestClient(create_app(embedder=make_manager(FakeEngine()))) as c:
        r = c.post("/explore", json={"query": "q", "min_score": 0.5})
        assert r.status_code == 400 and "Range retrieval is not available" in r.json()["detail"]
