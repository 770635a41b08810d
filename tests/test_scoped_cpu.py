"""No GPU: document-scoped retrieval's reference (tests/scoped_ref.py), the library's exports and argument checks, the
dispatcher's one-batch-per-k rule for requests with doc_ids, EmbeddingManager over a collection without scoped_query,
and the `doc_ids` field of POST /query over a fake embedder."""
import asyncio
import ctypes

import numpy as np
import pytest
from fastapi.testclient import TestClient

from tests import scoped_ref as R
from tests.fakes import FakeCollection, FakeEngine


# ---------------------------------------------------------------- 1. the reference on a hand-made case
def test_reference_on_a_hand_made_case():
    rows = np.zeros((6, 4), np.float32)
    rows[:, 0] = [1.0, 0.5, 0.5, 0.25, 0.75, 1.0]
    col = np.array([0, 1, 1, -1, 2, 0], np.int32)
    q = np.array([[1, 0, 0, 0], [-1, 0, 0, 0]], np.float32)
    scopes = [[1, 2], [0], [], [7]]
    s, r = R.scoped_topk(np.concatenate([q, q]), rows, 3, col, [0, 0, 1, 2], scopes)
    assert r.tolist() == [[4, 1, 2], [1, 2, 4], [0, 5, -1], [-1, -1, -1]]       # ties to the lower row, padding
    assert s[0].tolist() == [0.75, 0.5, 0.5] and s[1].tolist() == [-0.5, -0.5, -0.75]
    assert s[2].tolist() == [1.0, 1.0, -np.inf] and np.all(np.isneginf(s[3]))
    alive = np.array([0, 1, 0, 1, 1, 1], bool)
    s, r = R.scoped_topk(q[:1], rows, 2, col, [0], [[0, 1]], alive, row_offset=100)
    assert r.tolist() == [[105, 101]] and s.tolist() == [[1.0, 0.5]]
    assert R.visible_rows(col, [7]).size == 0 and R.visible_rows(col, [-1]).size == 0   # -1 is in no scope
    s, r = R.scoped_topk(q[:1], rows, 2, col, [0], [[-1]])
    assert r.tolist() == [[-1, -1]]


# ---------------------------------------------------------------- 2. exports and argument checks of the library
def test_exports_and_argument_checks_need_no_device():
    from multimodal_rag_amd import _native

    L = _native.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)       # never dereferenced: every call below returns before anything is launched
    EINVAL, EUNSUPPORTED = 1, 4
    assert L.mmrag_abi_version() == 1 and _native.MAX_SCOPE_GROUPS == 64
    assert _native.scoped_topk_workspace_bytes(256, 1 << 20, 5, 2000) > 256 * 16384 * 8
    assert _native.scoped_topk_workspace_bytes(0, 100, 5, 10) == 0
    assert _native.scoped_topk_workspace_bytes(1, 100, 4097, 10) == 0
    assert _native.candidate_capacity(5) == 16384 and _native.candidate_capacity(4096) == 32 * 4096
    assert hasattr(L, "mmrag_internal_scoped_topk_ex")

    def call(q=p, rows=p, B=4, n=100, d=64, ld=64, dtype=_native.F16, k=5, group=p, n_groups=10, soq=p, S=2, off=p,
             groups=p, max_candidates=100, out_s=p, out_r=p, ws=p, ws_bytes=4096):
        return L.mmrag_scoped_topk(q, rows, B, n, d, ld, dtype, k, 0, None, group, n_groups, soq, S, off, groups,
                                   max_candidates, out_s, out_r, ws, ws_bytes, None)

    assert call(out_s=None) == EINVAL and b"null output" in L.mmrag_last_error()
    assert call(out_r=None) == EINVAL
    for name in ("q", "rows", "group", "soq", "off", "groups"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=0) == EINVAL and call(S=0) == EINVAL and call(n=-1) == EINVAL and call(n=1 << 31) == EINVAL
    assert call(k=0) == EINVAL and call(k=4097) == EINVAL and call(d=0) == EINVAL and call(ld=63) == EINVAL
    assert call(n_groups=-1) == EINVAL and call(max_candidates=-1) == EINVAL and call(dtype=9) == EINVAL
    assert call(dtype=_native.F8E4M3, ld=128) == EUNSUPPORTED
    assert b"re-scoring plane" in L.mmrag_last_error()
    assert call(ws_bytes=16) == 2 and b"workspace" in L.mmrag_last_error()          # MMRAG_EWORKSPACE
    assert L.mmrag_abi_version() == 1


def test_scope_tables_are_checked_on_the_host():
    """the scope tables live on the device, where the C entry point cannot read them before it launches: the wrapper
    checks the host copies it is given"""
    from multimodal_rag_amd import _native

    ok = _native.check_scopes(3, 100, [0, 1, 0], [0, 2, 2], [5, 9])
    assert ok == 2
    assert _native.check_scopes(1, 100, [0], [0, 64], list(range(64))) == 1
    with pytest.raises(_native.MMRagNativeError, match="at most 64"):
        _native.check_scopes(1, 100, [0], [0, 65], list(range(65)))
    with pytest.raises(_native.MMRagNativeError, match="outside 0..1"):
        _native.check_scopes(3, 100, [0, 2, 0], [0, 2, 2], [5, 9])
    with pytest.raises(_native.MMRagNativeError, match="outside 0..1"):
        _native.check_scopes(3, 100, [0, -1, 0], [0, 2, 2], [5, 9])
    with pytest.raises(_native.MMRagNativeError, match="ascending"):
        _native.check_scopes(1, 100, [0], [0, 2], [9, 5])
    with pytest.raises(_native.MMRagNativeError, match="ascending"):
        _native.check_scopes(1, 100, [0], [0, 1], [100])
    with pytest.raises(_native.MMRagNativeError, match="offsets"):
        _native.check_scopes(1, 100, [0], [0, 3], [1, 2])
    with pytest.raises(_native.MMRagNativeError, match="2 entries for 3"):
        _native.check_scopes(3, 100, [0, 0], [0, 1], [1])


# ---------------------------------------------------------------- 3. dispatcher
def test_dispatcher_serves_different_documents_in_one_call():
    from multimodal_rag_amd.dispatcher import QueryDispatcher

    calls = {"batch": [], "scoped": []}

    async def batch_fn(texts, k, flt):
        calls["batch"].append((list(texts), k, flt))
        return [{"ids": [t], "flt": flt} for t in texts]

    async def scoped_fn(texts, k, docs):
        calls["scoped"].append((list(texts), k, [list(d) for d in docs]))
        return [{"ids": [t], "docs": d} for t, d in zip(texts, docs)]

    async def go():
        disp = QueryDispatcher(batch_fn, max_batch=64, max_wait_ms=200.0, idle_ms=50.0, scoped_fn=scoped_fn)
        try:
            out = await asyncio.gather(*[disp.submit(f"q{i}", 5, None, [f"doc{i}"]) for i in range(8)])
            assert calls["batch"] == [] and len(calls["scoped"]) == 1
            texts, k, docs = calls["scoped"][0]
            assert texts == [f"q{i}" for i in range(8)] and k == 5 and docs == [[f"doc{i}"] for i in range(8)]
            assert [o["docs"] for o in out] == docs and [o["ids"] for o in out] == [[t] for t in texts]
            # two k: one scoped call each; filters group as before; doc_ids next to a filter become part of it
            calls["scoped"].clear()
            flt = {"type": "text"}
            mixed = await asyncio.gather(
                disp.submit("a", 5, None, ["d1"]), disp.submit("b", 7, None, ["d2"]), disp.submit("c", 5, None, ["d3"]),
                disp.submit("d", 5), disp.submit("e", 5, flt), disp.submit("f", 5, flt), disp.submit("g", 5),
                disp.submit("h", 5, flt, ["d4"]))
            assert sorted((t, k) for t, k, _ in calls["scoped"]) == [(["a", "c"], 5), (["b"], 7)]
            both = {"$and": [flt, {"doc_id": {"$in": ["d4"]}}]}
            assert sorted(calls["batch"], key=repr) == sorted(
                [(["d", "g"], 5, None), (["e", "f"], 5, flt), (["h"], 5, both)], key=repr)
            assert mixed[7]["flt"] == both and mixed[0]["docs"] == ["d1"]
        finally:
            await disp.stop()
        # no scoped_fn: the documents become the filter, and requests are grouped by it as by any other
        calls["batch"].clear()
        plain = QueryDispatcher(batch_fn, max_batch=64, max_wait_ms=200.0, idle_ms=50.0)
        try:
            await asyncio.gather(plain.submit("x", 5, None, ["d1"]), plain.submit("y", 5, None, ["d1"]),
                                 plain.submit("z", 5, None, ["d2"]))
            assert sorted(calls["batch"], key=repr) == sorted(
                [(["x", "y"], 5, {"doc_id": {"$in": ["d1"]}}), (["z"], 5, {"doc_id": {"$in": ["d2"]}})], key=repr)
        finally:
            await plain.stop()

    asyncio.run(go())


# ---------------------------------------------------------------- 4. EmbeddingManager over a collection without scoped_query
def make_manager(engine):
    from multimodal_rag_amd.embedder import EmbeddingManager

    async def no_sleep(_):
        return None

    manager = EmbeddingManager(engine=engine)
    manager._sleep = no_sleep
    return manager


def test_manager_answers_by_filter_where_the_collection_has_no_scoped_query(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    engine = FakeEngine()
    m = make_manager(engine)

    async def go():
        await m.initialize()
        assert not m.supports_scoped()
        for doc in ("da", "db", "dc"):
            await m.embed_and_store([{"id": f"{doc}_{i}", "type": "text", "summary": f"{doc} passage {i}"}
                                     for i in range(6)], doc)
        one = await m.scoped_query("passage 3", ["db"], n_results=4)
        assert len(one["ids"]) == 4 and all(meta["doc_id"] == "db" for meta in one["metadatas"])
        assert one == await m.query("passage 3", n_results=4, filter_dict={"doc_id": {"$in": ["db"]}})
        assert (await m.scoped_query("passage 3", ["nowhere"]))["ids"] == []
        with pytest.raises(ValueError, match="empty"):
            await m.scoped_query("  ", ["db"])
        before, encodes = m.stats["total_queries"], len(engine.calls)
        many = await m.batch_scoped_query(["passage 1", " ", "passage 2", "passage 5"],
                                          [["da"], ["da"], ["dc", "db"], ["da"]], n_results=3)
        assert m.stats["total_queries"] == before + 3 and len(engine.calls) == encodes + 1      # ONE encode
        assert many[1]["error"] == "Query text cannot be empty" and many[1]["ids"] == []
        assert {meta["doc_id"] for meta in many[0]["metadatas"]} == {"da"} == {meta["doc_id"] for meta in many[3]["metadatas"]}
        assert {meta["doc_id"] for meta in many[2]["metadatas"]} <= {"dc", "db"} and len(many[2]["ids"]) == 3
        assert many[2] == await m.query("passage 2", n_results=3, filter_dict={"doc_id": {"$in": ["dc", "db"]}})
        with pytest.raises(ValueError, match="document lists"):
            await m.batch_scoped_query(["a", "b"], [["da"]])
        # through the dispatcher: no scoped_fn is wired for this collection, the documents travel as the filter
        disp = m.enable_dynamic_batching(max_batch=16, max_wait_ms=50.0)
        try:
            assert disp.scoped_fn is None
            out = await asyncio.gather(*[m.scoped_query("passage 3", [doc], n_results=2) for doc in ("da", "db", "dc")])
            for res, doc in zip(out, ("da", "db", "dc")):
                assert len(res["ids"]) == 2 and all(meta["doc_id"] == doc for meta in res["metadatas"])
        finally:
            await disp.stop()
            m._dispatcher = None
        await m.cleanup()

    asyncio.run(go())


class ScopedCollection(FakeCollection):
    """FakeCollection plus VectorIndex.scoped_query, answered query by query through the `where` filter"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.scoped_calls = []

    def scoped_query(self, query_embeddings, n_results=10, scopes=(), key="doc_id", where=None,
                     include=("metadatas", "documents", "distances"), check_norm=True):
        q = np.asarray(query_embeddings, np.float32).reshape(-1, self.dim)
        self.scoped_calls.append([list(s) for s in scopes])
        out = {"ids": [], "distances": [], "metadatas": [], "documents": []}
        for b, entry in enumerate(scopes):
            one = self.query(q[b: b + 1], n_results, where={key: {"$in": list(entry)}}, include=include)
            for name in out:
                out[name].append(one[name][0])
        return out


class ScopedEngine(FakeEngine):
    def new_collection(self, name, metadata=None):
        c = ScopedCollection(self.dim, name, metadata)
        self.collections.append(c)
        return c


def test_manager_and_dispatcher_make_one_collection_call(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    engine = ScopedEngine()
    m = make_manager(engine)

    async def go():
        await m.initialize()
        assert m.supports_scoped()
        docs = [f"d{i}" for i in range(8)]
        for doc in docs:
            await m.embed_and_store([{"id": f"{doc}_{i}", "type": "text", "summary": f"{doc} passage {i}"}
                                     for i in range(5)], doc)
        col = engine.collections[-1]
        many = await m.batch_scoped_query([f"passage {i}" for i in range(8)], [[doc] for doc in docs], n_results=3)
        assert col.scoped_calls == [[[doc] for doc in docs]]                     # ONE call for eight scopes
        encodes = len(engine.calls)
        disp = m.enable_dynamic_batching(max_batch=16, max_wait_ms=200.0)
        try:
            assert disp.scoped_fn is not None
            out = await asyncio.gather(*[m.scoped_query(f"passage {i}", [doc], n_results=3)
                                         for i, doc in enumerate(docs)])
        finally:
            await disp.stop()
            m._dispatcher = None
        assert len(col.scoped_calls) == 2 and col.scoped_calls[1] == col.scoped_calls[0]
        assert len(engine.calls) == encodes                                      # every text was cached by then
        assert out == many and all(meta["doc_id"] == doc for res, doc in zip(out, docs) for meta in res["metadatas"])
        await m.cleanup()

    asyncio.run(go())


# ---------------------------------------------------------------- 5. POST /query with doc_ids over a fake embedder
def test_query_endpoint_doc_ids(monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.server import create_app

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    seen = []

    class RecordingManager(EmbeddingManager):
        """records how a restriction to documents arrives; hybrid retrieval is the dense one with a score column"""

        async def scoped_query(self, query_text, doc_ids, n_results=5):
            seen.append(("scoped", list(doc_ids), n_results))
            return await super().scoped_query(query_text, doc_ids, n_results=n_results)

        async def query(self, query_text, n_results=5, filter_dict=None):
            seen.append(("query", filter_dict, n_results))
            return await super().query(query_text, n_results=n_results, filter_dict=filter_dict)

        def supports_hybrid(self):
            return True

        async def hybrid_query(self, query_text, n_results=5, filter_dict=None):
            seen.append(("hybrid", filter_dict, n_results))
            hits = await super().query(query_text, n_results=n_results, filter_dict=filter_dict)
            return {**hits, "hybrid_scores": [1.0] * len(hits["ids"]), "lexical_scores": [0.0] * len(hits["ids"])}

    manager = RecordingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=manager)) as c:
        docs = []
        for word in ("alpha", "beta", "gamma"):
            body = "\n\n".join(f"{word} paragraph number {i} about {word} engines. " * 25 for i in range(4)).encode()
            r = c.post("/upload", files={"file": (f"{word}.txt", body, "text/plain")})
            assert r.status_code == 200, r.text
            docs.append(r.json()["doc_id"])
        seen.clear()
        plain = c.post("/query", json={"query": "engines", "top_k": 3})
        assert plain.status_code == 200 and seen == [("query", None, 3)]            # nothing changes without doc_ids
        seen.clear()
        r = c.post("/query", json={"query": "engines", "top_k": 3, "doc_ids": [docs[1]]})
        assert r.status_code == 200, r.text
        assert seen[0] == ("scoped", [docs[1]], 3)
        src = r.json()["sources"]
        assert len(src) == 3 and all(s["doc_id"].startswith(docs[1]) for s in src)
        assert set(src[0]) == set(plain.json()["sources"][0])                        # sources unchanged in shape
        seen.clear()
        r = c.post("/query", json={"query": "engines", "top_k": 2, "doc_ids": [docs[0], docs[2]], "hybrid": True})
        assert r.status_code == 200, r.text
        assert seen[0] == ("hybrid", {"doc_id": {"$in": [docs[0], docs[2]]}}, 2)
        assert all(s["doc_id"].startswith((docs[0], docs[2])) and "hybrid_score" in s for s in r.json()["sources"])
        r = c.post("/query", json={"query": "engines", "doc_ids": ["doc_unknown"]})
        assert r.status_code == 200 and r.json()["sources"] == []                   # as an empty collection answers
        assert r.json()["answer"] == c.post("/query", json={"query": "engines", "doc_ids": ["x"]}).json()["answer"]
        assert c.post("/query", json={"query": "engines", "doc_ids": []}).status_code == 422
        assert c.post("/query", json={"query": "engines", "doc_ids": [""]}).status_code == 422
        assert c.post("/query", json={"query": "engines", "doc_ids": [f"d{i}" for i in range(65)]}).status_code == 422
        assert c.post("/query", json={"query": "engines", "doc_ids": [f"d{i}" for i in range(64)]}).status_code == 200
