"""No GPU: related-document retrieval's reference (tests/related_ref.py) on hand-made cases, the case that pins why the
feature exists, the library's exports and argument checks, EmbeddingManager.related_documents' refusals, and the two
routes (GET /documents/{doc_id}/related, POST /related) over a fake collection."""
import asyncio
import ctypes

import numpy as np
import pytest
from fastapi.testclient import TestClient

from tests import related_ref as R
from tests.fakes import FakeCollection, FakeEngine


# ---------------------------------------------------------------- 1. the reference on a hand-worked case
def test_reference_on_a_hand_worked_case():
    """6 rows, 3 documents, sets of 2 and 1 vectors, everything on two axes so every number can be read off"""
    rows = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0], [0.5, 0.0], [0.5, 0.0], [0.0, 0.25]], np.float32)
    col = np.array([0, 0, 1, 2, 2, 1], np.int32)
    sets = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]], np.float32)
    # best[a][g]:   a0: g0 = 1 (row 0), g1 = 0 (row 2, the lower of two zeros), g2 = 0.5 (row 3, the lower of a tie)
    #               a1: g0 = 0.5 (row 1), g1 = 1 (row 2), g2 = 0 (row 3)
    (sim, grp, cov, best, row), _ = R.related_groups(sets, [0, 2, 3], rows, col, 3, 4, 0.5)
    assert grp.tolist() == [[0, 1, 2, -1], [1, 0, 2, -1]]
    assert sim[0].tolist() == [0.75, 0.5, 0.25, -np.inf] and sim[1].tolist() == [1.0, 0.5, 0.0, -np.inf]
    assert cov.tolist() == [[2, 1, 1, 0], [1, 1, 0, 0]]
    assert best[:, :3].tolist() == [[1.0, 0.0, 0.5], [0.5, 1.0, 0.0], [1.0, 0.5, 0.0]]
    assert row[:, :3].tolist() == [[0, 2, 3], [1, 2, 3], [2, 1, 3]]
    assert np.all(np.isneginf(best[:, 3])) and np.all(row[:, 3] == -1)
    # the excluded group and a dead row: document 0 is gone for set 0, row 2 is dead so document 1 rests on row 5
    alive = np.array([1, 1, 0, 1, 1, 1], bool)
    (sim, grp, cov, best, row), _ = R.related_groups(sets, [0, 2, 3], rows, col, 3, 2, 0.5, exclude=[0, -1], alive=alive)
    assert grp.tolist() == [[2, 1], [0, 1]] and sim.tolist() == [[0.25, 0.125], [0.5, 0.25]]
    assert row[:2].tolist() == [[3, 5], [3, 5]] and cov.tolist() == [[1, 0], [1, 0]]
    # two documents with the same similarity: the lower ordinal first; an empty set is padding only
    (sim, grp, _, _, _), _ = R.related_groups(sets[:1], [0, 0, 1], np.array([[0.5, 0], [0.5, 0]], np.float32),
                                             np.array([1, 0], np.int32), 2, 2, 0.5)
    assert grp.tolist() == [[-1, -1], [0, 1]] and sim[1].tolist() == [0.5, 0.5]
    # ordinals outside 0..n_groups-1 are rows of no document
    (_, grp, _, _, _), _ = R.related_groups(sets[:1], [0, 1], rows, np.array([-1, 7, 1, -1, 3, 1], np.int32), 3, 3, 0.5)
    assert grp.tolist() == [[1, -1, -1]]


# ---------------------------------------------------------------- 2. why the feature exists
def test_best_document_is_in_no_chunk_list_at_depth_10():
    """A set of 4 orthogonal chunks.  For every chunk 12 one-row documents hold a 0.9 match of it and nothing of the
    others; one document holds a 0.6 match of EVERY chunk.  That document is the 13th hit of each chunk, so no merge
    of per-chunk top-10 lists can see it -- and it is the most similar document by far (0.6 against 0.9 / 4)."""
    m, per = 4, 12
    d = m + m + m * per
    sets = np.eye(m, d, dtype=np.float64)
    rows, col = [], []
    for i in range(m):                                   # the document that holds all of the set: ordinal 0
        v = np.zeros(d)
        v[i], v[m + i] = 0.6, 0.8
        rows.append(v)
        col.append(0)
    for i in range(m):
        for j in range(per):
            v = np.zeros(d)
            v[i], v[2 * m + i * per + j] = 0.9, np.sqrt(1 - 0.81)
            rows.append(v)
            col.append(1 + i * per + j)
    rows, col = np.array(rows), np.array(col, np.int32)
    assert np.allclose(np.linalg.norm(rows, axis=1), 1.0)
    n_groups = 1 + m * per
    (sim, grp, cov, _, _), _ = R.related_groups(sets, [0, m], rows, col, n_groups, 3, 0.5)
    assert grp[0, 0] == 0 and abs(sim[0, 0] - 0.6) < 1e-6 and cov[0, 0] == m
    assert abs(sim[0, 1] - 0.225) < 1e-6 and cov[0, 1] == 1
    seen = R.chunk_topk_groups(sets, rows, col, 10)
    assert all(0 not in groups and len(groups) == 10 for groups in seen)


# ---------------------------------------------------------------- 3. exports and argument checks of the library
def test_exports_and_argument_checks_need_no_device():
    from multimodal_rag_amd import _native

    L = _native.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)       # never dereferenced: every call below returns before anything is launched
    EINVAL, EUNSUPPORTED = 1, 4
    assert L.mmrag_abi_version() == 1
    assert _native.MAX_RELATED_ROWS == 8192 and _native.MAX_RELATED_SETS == 64
    assert hasattr(L, "mmrag_related_groups") and hasattr(L, "mmrag_internal_related_groups_ex")
    wb = _native.related_groups_workspace_bytes
    assert wb(128, 1, 1 << 20, 20000, 5) >= 8 * 128 * 20000
    assert wb(128, 1, 1000, 100, 5) <= wb(256, 1, 1000, 100, 5) <= wb(256, 1, 1000, 200, 5) <= wb(256, 2, 1000, 200, 5)
    assert wb(256, 2, 1000, 200, 5) <= wb(256, 2, 1000, 200, 50) and wb(0, 1, 0, 0, 1) > 0
    for bad in ((-1, 1, 10, 10, 5), (8193, 1, 10, 10, 5), (4, 0, 10, 10, 5), (4, 65, 10, 10, 5), (4, 1, -1, 10, 5),
                (4, 1, 1 << 31, 10, 5), (4, 1, 10, -1, 5), (4, 1, 10, 10, 0), (4, 1, 10, 10, 4097)):
        assert wb(*bad) == 0, bad

    def call(sets=p, M=4, off=p, S=2, rows=p, n=100, d=64, ld=64, dtype=_native.F16, group=p, n_groups=10, excl=p,
             threshold=0.9, k=5, out_sim=p, out_grp=p, out_cov=p, out_best=p, out_row=p, ws=p, ws_bytes=1 << 30):
        return L.mmrag_related_groups(sets, M, off, S, rows, n, d, ld, dtype, None, group, n_groups, excl, threshold, k,
                                      out_sim, out_grp, out_cov, out_best, out_row, ws, ws_bytes, None)

    for name in ("out_sim", "out_grp", "out_cov", "out_best", "out_row"):
        assert call(**{name: None}) == EINVAL and b"null output" in L.mmrag_last_error(), name
    for name in ("sets", "off", "rows", "group", "excl"):
        assert call(**{name: None}) == EINVAL and b"null pointer" in L.mmrag_last_error(), name
    assert call(M=-1) == EINVAL and call(M=8193) == EINVAL and call(S=0) == EINVAL and call(S=65) == EINVAL
    assert call(n=-1) == EINVAL and call(n=1 << 31) == EINVAL and call(k=0) == EINVAL and call(k=4097) == EINVAL
    assert call(d=0) == EINVAL and call(ld=63) == EINVAL and call(n_groups=-1) == EINVAL and call(dtype=9) == EINVAL
    assert call(threshold=float("nan")) == EINVAL
    assert call(dtype=_native.F8E4M3, ld=128) == EUNSUPPORTED and b"re-scoring plane" in L.mmrag_last_error()
    assert call(ws=None) == EINVAL and call(ws_bytes=16) == EINVAL and b"workspace" in L.mmrag_last_error()
    assert L.mmrag_abi_version() == 1


# ---------------------------------------------------------------- 4. EmbeddingManager and the routes over a fake collection
class RelatedCollection(FakeCollection):
    """FakeCollection plus VectorIndex.related_query, answered by the reference"""

    def related_query(self, sets, n_results=5, key="doc_id", threshold=None, exclude=None, where=None,
                      include=("metadatas", "documents"), check_norm=True):
        from multimodal_rag_amd.index import match_where

        values = list(dict.fromkeys(m[key] for m in self.metas if key in m))
        col = np.array([values.index(m[key]) if key in m else -1 for m in self.metas], np.int32)
        alive = np.array([match_where(m, where) for m in self.metas], bool) if where else None
        out = []
        for entry in sets:
            if isinstance(entry, dict):
                mine = [i for i, m in enumerate(self.metas) if m.get(key) == entry["value"]]
                if not mine:
                    raise ValueError(f"no stored row has {key}={entry['value']!r}")
                vecs, items, excl = self.vecs[mine], [self.ids[i] for i in mine], values.index(entry["value"])
            else:
                vecs = np.asarray(entry, np.float32).reshape(-1, self.dim)
                items, excl = list(range(len(vecs))), -1
            m = len(vecs)
            (sim, grp, cov, best, row), _ = R.related_groups(vecs, [0, m], self.vecs, col, len(values), n_results,
                                                             threshold, exclude=[excl], alive=alive)
            out.append([{"key": values[g], "similarity": float(sim[0, j]), "coverage": int(cov[0, j]) / m,
                         "matched": int(cov[0, j]), "rows_in_group": int(np.sum(col == g)),
                         "pairs": [{"item": items[a], "match_id": self.ids[row[a, j]], "score": float(best[a, j])}
                                   for a in range(m)]}
                        for j, g in enumerate(grp[0].tolist()) if g >= 0])
        return out


class RelatedEngine(FakeEngine):
    def new_collection(self, name, metadata=None):
        c = RelatedCollection(self.dim, name, metadata)
        self.collections.append(c)
        return c


def make_manager(engine):
    from multimodal_rag_amd.embedder import EmbeddingManager

    async def no_sleep(_):
        return None

    manager = EmbeddingManager(engine=engine)
    manager._sleep = no_sleep
    return manager


def store(engine, col, doc, texts):
    col.add(engine.encode(texts), documents=texts, metadatas=[{"doc_id": doc, "type": "text"}] * len(texts),
            ids=[f"{doc}_{i}" for i in range(len(texts))])


def test_related_documents_refusals_and_answer(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    engine = RelatedEngine()
    m = make_manager(engine)

    async def go():
        with pytest.raises(ValueError, match="exactly one"):
            await m.related_documents()
        with pytest.raises(ValueError, match="exactly one"):
            await m.related_documents(doc_id="a", texts=["x"])
        await m.initialize()
        assert m.supports_related()
        col = engine.collections[-1]
        shared = [f"shared passage {i}" for i in range(6)]
        store(engine, col, "da", shared + ["only in a"])
        store(engine, col, "db", shared[:4] + ["only in b", "also only in b"])
        store(engine, col, "dc", ["nothing alike", "something else"])
        with pytest.raises(LookupError, match="nowhere"):
            await m.related_documents(doc_id="nowhere")
        for bad in ([], ["ok", " "], ["ok", 3]):
            with pytest.raises(ValueError, match="non-empty"):
                await m.related_documents(texts=bad)
        with pytest.raises(ValueError, match="at most 8192"):
            await m.related_documents(texts=["x"] * 8193)
        out = await m.related_documents(doc_id="da", n_results=5)
        assert out["chunks"] == 7 and out["threshold"] == config.settings.MMRAG_DEDUP_REPORT_THRESHOLD
        assert [r["key"] for r in out["related"]] == ["db", "dc"]            # "da" itself is no candidate
        top = out["related"][0]
        assert top["matched"] == 4 and top["coverage"] == 4 / 7 and top["rows_in_group"] == 6
        assert [p["item"] for p in top["pairs"]] == [f"da_{i}" for i in range(7)]
        assert [p["match_id"] for p in top["pairs"][:4]] == [f"db_{i}" for i in range(4)]
        calls = len(engine.calls)
        out = await m.related_documents(texts=shared[2:5] + ["new words"], n_results=2, threshold=0.5)
        assert len(engine.calls) == calls + 1 and engine.calls[-1] == 4        # ONE encode call for the four texts
        assert out["chunks"] == 4 and out["threshold"] == 0.5
        assert [r["key"] for r in out["related"]] == ["da", "db"] and [r["matched"] for r in out["related"]] == [3, 2]
        assert [p["item"] for p in out["related"][0]["pairs"]] == [0, 1, 2, 3]
        only_c = await m.related_documents(texts=shared[:2], filter_dict={"doc_id": "dc"})
        assert [r["key"] for r in only_c["related"]] == ["dc"]
        await m.cleanup()

    asyncio.run(go())
    # a collection without related_query (the sharded path's, the plain fake): refused, not answered another way
    plain = make_manager(FakeEngine())

    async def refused():
        await plain.initialize()
        assert not plain.supports_related()
        with pytest.raises(ValueError, match="single-GPU"):
            await plain.related_documents(texts=["x"])
        await plain.cleanup()

    asyncio.run(refused())


def test_related_routes(monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.server import create_app

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    engine = RelatedEngine()
    manager = make_manager(engine)
    with TestClient(create_app(embedder=manager)) as c:
        col = engine.collections[-1]
        shared = [f"shared passage {i}" for i in range(8)]
        store(engine, col, "da", shared)
        store(engine, col, "db", shared[:7] + ["only in b"])
        store(engine, col, "dc", ["nothing alike"])
        r = c.get("/documents/da/related", params={"top_k": 2})
        assert r.status_code == 200, r.text
        body = r.json()
        assert set(body) == {"doc_id", "chunks", "threshold", "related", "processing_time"}
        assert body["doc_id"] == "da" and body["chunks"] == 8
        assert body["threshold"] == config.settings.MMRAG_DEDUP_REPORT_THRESHOLD
        assert [d["key"] for d in body["related"]] == ["db", "dc"]
        first = body["related"][0]
        assert set(first) == {"key", "similarity", "coverage", "matched", "rows_in_group", "pairs"}
        assert first["matched"] == 7 and first["coverage"] == 7 / 8 and first["rows_in_group"] == 8
        assert len(first["pairs"]) == 5 and all(abs(p["score"] - 1.0) < 1e-5 for p in first["pairs"])   # the 5 best
        assert all(set(p) == {"item", "match_id", "score"} for p in first["pairs"])
        scores = [p["score"] for p in body["related"][1]["pairs"]]
        assert len(scores) == 5 and scores == sorted(scores, reverse=True)
        assert c.get("/documents/da/related", params={"threshold": 0.5}).json()["threshold"] == 0.5
        assert c.get("/documents/nowhere/related").status_code == 404
        assert "nowhere" in c.get("/documents/nowhere/related").json()["detail"]
        assert c.get("/documents/da/related", params={"top_k": 0}).status_code == 400
        r = c.post("/related", json={"texts": shared[:3] + ["only in b"], "top_k": 3})
        assert r.status_code == 200, r.text
        body = r.json()
        assert set(body) == {"chunks", "threshold", "related", "processing_time"} and body["chunks"] == 4
        assert [(d["key"], d["matched"]) for d in body["related"]] == [("db", 4), ("da", 3), ("dc", 0)]
        assert sorted(p["item"] for p in body["related"][0]["pairs"]) == [0, 1, 2, 3]
        assert c.post("/related", json={"texts": []}).status_code == 422
        assert c.post("/related", json={"texts": ["a"], "top_k": 0}).status_code == 422
        assert c.post("/related", json={"texts": ["a", " "]}).status_code == 400
    # an embedder whose collection cannot: 400 with a clear message, on both routes
    with TestClient(create_app(embedder=make_manager(FakeEngine()))) as c:
        for r in (c.get("/documents/da/related"), c.post("/related", json={"texts": ["a"]})):
            assert r.status_code == 400 and "Related-document retrieval is not available" in r.json()["detail"]
