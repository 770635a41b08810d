"""No GPU: the filter compiler and its numpy interpreter against index.match_where (tests/filter_ref.py), the metadata
columns' append / compact paths, the library's exports and argument checks, the dispatcher's one-batch-per-k rule for
requests with filters, EmbeddingManager over a collection without filtered_query, and the `filter` field of POST /query
over a fake embedder."""
import asyncio
import ctypes

import numpy as np
import pytest
from fastapi.testclient import TestClient

from multimodal_rag_amd import filters as F
from tests import filter_ref as R
from tests.fakes import FakeEngine

N_ROWS = 400


@pytest.fixture(scope="module")
def table():
    metas, times = R.metadata(N_ROWS, 1)
    return metas, times, F.ColumnRegistry.from_metadatas(metas, times)


# ---------------------------------------------------------------- 1. the compiler against match_where
def test_every_covered_filter_compiles_and_equals_match_where(table):
    metas, times, reg = table
    family = R.covered_filters(N_ROWS, 2)
    assert len(family) >= 300
    longest, ops_seen = 0, set()
    for where in family:
        prog, why = F.try_compile(where, reg)
        assert prog is not None, (where, why)            # no share of the family may be left out
        assert 1 <= len(prog.instrs) <= F.MAX_FILTER_OPS
        longest = max(longest, len(prog.instrs))
        ops_seen |= {(ins.code, reg.get(ins.key).kind) for ins in prog.instrs if ins.key is not None}
        got = F.run_program_host(prog, reg.host_columns(prog.keys), N_ROWS)
        want = R.visible(metas, where, times=times)
        assert got.dtype == bool and np.array_equal(got, want), where
    # the largest program there is: 16 leaves and 15 combinators (binary postfix programs hold an odd number)
    assert longest == F.MAX_FILTER_OPS - 1
    assert {(c, F.NUMBER) for c in range(F.EQ, F.NIN + 1)} <= ops_seen
    assert {(c, F.STRING) for c in (F.EQ, F.NE, F.IN, F.NIN)} <= ops_seen
    kinds = {k: reg.get(k).kind for k in ("doc_id", "type", "page", "score", "flag", "ghost", "$added_at")}
    assert kinds == {"doc_id": F.STRING, "type": F.STRING, "page": F.NUMBER, "score": F.NUMBER, "flag": F.NUMBER,
                     "ghost": F.ABSENT, "$added_at": F.NUMBER}
    assert reg.get("page").host.dtype == np.float64 and np.isnan(reg.get("page").host[:N_ROWS]).any()
    assert reg.get("type").host.dtype == np.int32 and list(reg.get("doc_id").ordinals)[:2] == ["doc0", "doc1"]


def test_uncovered_forms_are_refused_with_a_reason(table):
    _, _, reg = table
    for what, where in R.uncovered_filters():
        prog, why = F.try_compile(where, reg)
        assert prog is None and why, what
        assert F.compile_where(where, reg) is None
        plan = reg.plan(where)
        assert plan == {"device": False, "reason": why, "columns": []}
    for key in ("mixed", "big", "nan"):
        assert reg.get(key).kind == F.UNSUPPORTED and reg.get(key).reason
    assert reg.plan({"page": {"$gt": 3}, "type": "table"}) == {"device": True, "reason": "", "columns": ["page", "type"]}
    # an unknown operator raises as match_where does
    from multimodal_rag_amd.index import match_where

    bad = {"page": {"$between": [1, 2]}}
    with pytest.raises(ValueError) as mine:
        F.try_compile(bad, reg)
    with pytest.raises(ValueError) as theirs:
        match_where({"page": 1}, bad)
    assert str(mine.value) == str(theirs.value)
    # 16 leaves compile, 17 do not: the instruction limit sits between 31 and 33
    assert len(F.compile_where({"$and": [{"page": {"$ne": p}} for p in range(16)]}, reg).instrs) == 31


def test_equal_filters_are_one_program(table):
    _, _, reg = table
    a = F.compile_where({"type": "table", "page": {"$gte": 3, "$lt": 9}, "doc_id": {"$in": ["doc3", "doc1", "doc3"]}}, reg)
    b = F.compile_where({"doc_id": {"$in": ["doc1", "doc3"]}, "page": {"$lt": 9, "$gte": 3}, "type": "table"}, reg)
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a != F.compile_where({"type": "table", "page": {"$gte": 3, "$lt": 10}, "doc_id": {"$in": ["doc1", "doc3"]}}, reg)
    assert F.names_added_at({"$or": [{"a": 1}, {"$and": [{"$added_at": {"$gt": 0}}]}]}) and not F.names_added_at({"a": 1})
    ops, off, sets, keys = F.pack_programs([a, F.compile_where(None, reg)])
    assert ops.dtype.itemsize == 24 and off.tolist() == [0, len(a.instrs), len(a.instrs) + 1]
    assert keys == a.keys and sets.tolist() == sorted(sets.tolist()) and len(sets) == 2


def test_columns_follow_appends_and_compaction():
    metas, times = R.metadata(N_ROWS, 3)
    grown_metas = list(metas[:150])
    grown = F.ColumnRegistry(lambda: (grown_metas, len(grown_metas), times))
    keys = ("doc_id", "type", "page", "score", "flag", "ghost", "mixed", "late")
    for key in keys:
        grown.get(key)
    for lo in (150, 151, 300):
        hi = {150: 151, 151: 300, 300: N_ROWS}[lo]
        batch = [dict(m) for m in metas[lo:hi]]
        if lo == 300:
            for i, m in enumerate(batch):
                m["late"] = i            # a key that appears only now: earlier rows are missing it
        grown_metas.extend(batch)
        grown.appended(batch, lo)
    whole = F.ColumnRegistry.from_metadatas(grown_metas, times)      # the same rows, built in one pass
    for key in keys:
        a, b = whole.get(key), grown.get(key)
        assert a.kind == b.kind and a.ordinals == b.ordinals, key
        if a.kind in (F.NUMBER, F.STRING):
            assert np.array_equal(a.host[:N_ROWS], b.host[:N_ROWS], equal_nan=True), key
    assert grown.get("late").kind == F.NUMBER and np.isnan(grown.get("late").host[:300]).all()
    # a str among the numbers: the key is unsupported from then on, filters on it take the host path
    grown_metas.append({"page": "seven"})
    grown.appended(grown_metas[-1:], N_ROWS)
    assert grown.get("page").kind == F.UNSUPPORTED and not grown.plan({"page": 3})["device"]
    assert grown.plan({"type": "table"})["device"]
    # compaction keeps the kept rows' values in order and the dictionaries' ordinals
    keep = np.arange(0, N_ROWS, 3)
    before = {k: whole.get(k).host[:N_ROWS].copy() for k in ("doc_id", "score")}
    whole.compacted(keep)
    for k, col in before.items():
        assert np.array_equal(whole.get(k).host[: keep.size], col[keep], equal_nan=True)
    whole.reset()
    assert whole._cols == {}


# ---------------------------------------------------------------- 2. exports and argument checks of the library
def test_exports_and_argument_checks_need_no_device():
    from multimodal_rag_amd import _native

    L = _native.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)       # never dereferenced: every call below returns before anything is launched
    EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4
    assert (_native.MAX_FILTER_OPS, _native.MAX_FILTER_SET, _native.MAX_FILTER_COLUMNS) == (32, 64, 16)
    assert [_native.filter_words(n) for n in (0, 1, 127, 128, 129, 1000, 1 << 20)] == [0, 4, 4, 4, 8, 32, 32768]
    assert _native.filter_words(-1) == 0 and _native.filter_words(1 << 31) == 0
    assert _native.filter_words((1 << 31) - 1) == 4 * (1 << 24)
    assert _native.filtered_topk_workspace_bytes(256, 1 << 20, 5) > 256 * 16384 * 8 + 3 * 32768 * 4
    for bad in ((0, 100, 5), (1, 100, 0), (1, 100, 4097), (1, -1, 5), (1, 1 << 31, 5)):
        assert _native.filtered_topk_workspace_bytes(*bad) == 0, bad
    assert hasattr(L, "mmrag_internal_filtered_topk_ex")

    def call(q=p, rows=p, B=4, n=100, d=64, ld=64, dtype=_native.F16, k=5, foq=p, F=2, vis=p, out_s=p, out_r=p, ws=p,
             ws_bytes=4096):
        return L.mmrag_filtered_topk(q, rows, B, n, d, ld, dtype, k, 0, foq, F, vis, out_s, out_r, ws, ws_bytes, None)

    assert call(out_s=None) == EINVAL and b"null output" in L.mmrag_last_error()
    assert call(out_r=None) == EINVAL
    for name in ("q", "rows", "foq", "vis"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=0) == EINVAL and call(F=0) == EINVAL and call(n=-1) == EINVAL and call(n=1 << 31) == EINVAL
    assert call(k=0) == EINVAL and call(k=4097) == EINVAL and call(d=0) == EINVAL and call(ld=63) == EINVAL
    assert call(ld=32) == EINVAL and call(dtype=9) == EINVAL
    assert call(dtype=_native.F8E4M3, ld=128) == EUNSUPPORTED
    assert b"re-scoring plane" in L.mmrag_last_error()
    assert call(ws_bytes=16) == EWORKSPACE and b"workspace" in L.mmrag_last_error()
    assert call(ws=None, ws_bytes=1 << 30) == EWORKSPACE
    assert call(ws=p + 8, ws_bytes=1 << 30) == EWORKSPACE and b"aligned" in L.mmrag_last_error()

    cols = (ctypes.c_void_p * 16)(*([p] * 16))
    kinds = (ctypes.c_int32 * 16)(*([0, 1] * 8))

    def ev(ops=p, n_ops=3, off=p, F=1, sets=p, n_set=2, columns=cols, kind=kinds, n_columns=2, n=100, out=p):
        return L.mmrag_filter_eval(ops, n_ops, off, F, sets, n_set, columns, kind, n_columns, n, None, out, None)

    for name in ("ops", "off", "out", "sets", "columns", "kind"):
        assert ev(**{name: None}) == EINVAL, name
    assert ev(F=0) == EINVAL and ev(n_ops=0) == EINVAL and ev(n_set=-1) == EINVAL
    assert ev(n=-1) == EINVAL and ev(n=1 << 31) == EINVAL and ev(n_columns=17) == EINVAL and ev(n_columns=-1) == EINVAL
    assert ev(kind=(ctypes.c_int32 * 16)(0, 7)) == EINVAL and b"kind" in L.mmrag_last_error()
    assert ev(columns=(ctypes.c_void_p * 16)(p, None)) == EINVAL
    assert ev(n=0) == 0                                  # no rows: no words, nothing launched
    assert L.mmrag_abi_version() == 1


def test_program_tables_are_checked_on_the_host(table):
    """the tables live on the device, where the C entry point cannot read them before it launches: the wrapper checks the
    host copies it is given"""
    from multimodal_rag_amd import _native

    _, _, reg = table
    progs = [F.compile_where(w, reg) for w in ({"page": {"$in": [1, 2]}, "type": "table"}, None, {"score": {"$lt": 0}})]
    ops, off, sets, keys = F.pack_programs(progs)
    assert _native.check_filter_programs(ops, off, sets, len(keys)) == 3

    def broken(**change):
        o, f, s = ops.copy(), off.copy(), sets.copy()
        for name, (i, v) in change.items():
            {"ops_code": lambda: o["code"].__setitem__(i, v), "ops_column": lambda: o["column"].__setitem__(i, v),
             "ops_set_off": lambda: o["set_off"].__setitem__(i, v), "ops_set_len": lambda: o["set_len"].__setitem__(i, v),
             "ops_value": lambda: o["value"].__setitem__(i, v), "off": lambda: f.__setitem__(i, v),
             "sets": lambda: s.__setitem__(i, v)}[name]()
        return o, f, s

    leaf_in = int(np.nonzero(ops["code"] == F.IN)[0][0])
    leaf_lt = int(np.nonzero(ops["code"] == F.LT)[0][0])
    for change, text in (({"off": (1, 99)}, "ascending"), ({"off": (0, 1)}, "ascending"), ({"ops_code": (0, 12)}, "code"),
                         ({"ops_code": (0, -1)}, "code"), ({"ops_column": (leaf_in, len(keys))}, "column"),
                         ({"ops_column": (leaf_lt, -1)}, "column"), ({"ops_set_off": (leaf_in, 1)}, "set"),
                         ({"ops_set_len": (leaf_in, 65)}, "set"), ({"ops_set_off": (leaf_in, -1)}, "set"),
                         ({"ops_value": (leaf_lt, float("nan"))}, "compares"), ({"sets": (0, float("inf"))}, "finite"),
                         ({"ops_code": (0, F.AND)}, "empty stack"), ({"ops_code": (2, F.TRUE)}, "stack")):
        with pytest.raises(_native.MMRagNativeError, match=text):
            _native.check_filter_programs(*broken(**change), len(keys))
    long = F.Program(tuple([F.Instr(F.TRUE)] + [F.Instr(F.TRUE), F.Instr(F.AND)] * 16))     # 33 instructions
    with pytest.raises(_native.MMRagNativeError, match="33 instructions"):
        _native.check_filter_programs(*F.pack_programs([long])[:3], 0)


# ---------------------------------------------------------------- 3. dispatcher
def test_dispatcher_serves_different_filters_in_one_call():
    from multimodal_rag_amd.dispatcher import QueryDispatcher

    calls = {"batch": [], "filtered": [], "scoped": []}

    async def batch_fn(texts, k, flt):
        calls["batch"].append((list(texts), k, flt))
        return [{"ids": [t], "flt": flt} for t in texts]

    async def filtered_fn(texts, k, filters):
        calls["filtered"].append((list(texts), k, list(filters)))
        return [{"ids": [t], "flt": f} for t, f in zip(texts, filters)]

    async def scoped_fn(texts, k, docs):
        calls["scoped"].append((list(texts), k, [list(d) for d in docs]))
        return [{"ids": [t], "docs": d} for t, d in zip(texts, docs)]

    filters = [{"type": "table"}, {"page": {"$gte": 10, "$lte": 40}}, {"doc_id": "d1"}, {"$added_at": {"$gt": 5}},
               {"$or": [{"type": "text"}, {"flag": True}]}]

    async def go():
        disp = QueryDispatcher(batch_fn, max_batch=64, max_wait_ms=200.0, idle_ms=50.0, filtered_fn=filtered_fn,
                               scoped_fn=scoped_fn)
        try:
            out = await asyncio.gather(*[disp.submit(f"q{i}", 5, flt) for i, flt in enumerate(filters)])
            assert calls["batch"] == [] and len(calls["filtered"]) == 1           # five filters, ONE call
            assert calls["filtered"][0] == ([f"q{i}" for i in range(5)], 5, filters)
            assert [o["flt"] for o in out] == filters
            # two k: one call each; no filter: the plain batch; doc_ids alone: the scoped batch; doc_ids next to a
            # filter are folded into it and travel with the filtered batch
            for seen in calls.values():
                seen.clear()
            mixed = await asyncio.gather(
                disp.submit("a", 5, filters[0]), disp.submit("b", 7, filters[1]), disp.submit("c", 5, filters[2]),
                disp.submit("d", 5), disp.submit("e", 5, None, ["d9"]), disp.submit("f", 5, filters[0], ["d4"]))
            both = {"$and": [filters[0], {"doc_id": {"$in": ["d4"]}}]}
            assert sorted(calls["filtered"], key=repr) == sorted(
                [(["a", "c", "f"], 5, [filters[0], filters[2], both]), (["b"], 7, [filters[1]])], key=repr)
            assert calls["batch"] == [(["d"], 5, None)] and calls["scoped"] == [(["e"], 5, [["d9"]])]
            assert mixed[5]["flt"] == both and mixed[4]["docs"] == ["d9"]
        finally:
            await disp.stop()
        # no filtered_fn: today's grouping, one call per (k, filter)
        for seen in calls.values():
            seen.clear()
        plain = QueryDispatcher(batch_fn, max_batch=64, max_wait_ms=200.0, idle_ms=50.0)
        try:
            assert plain.filtered_fn is None
            await asyncio.gather(*[plain.submit(f"q{i}", 5, flt) for i, flt in enumerate(filters + filters[:1])])
            assert calls["filtered"] == [] and len(calls["batch"]) == 5
            assert sorted(calls["batch"], key=repr)[0][2] in filters
            assert (["q0", "q5"], 5, filters[0]) in calls["batch"]
        finally:
            await plain.stop()

    asyncio.run(go())


# ---------------------------------------------------------------- 4. manager fallback and server
def make_manager(engine):
    from multimodal_rag_amd.embedder import EmbeddingManager

    async def no_sleep(_):
        return None

    manager = EmbeddingManager(engine=engine)
    manager._sleep = no_sleep
    return manager


def test_manager_answers_per_distinct_filter_where_the_collection_has_no_filtered_query(monkeypatch):
    from multimodal_rag_amd import config

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    monkeypatch.setattr(config.settings, "MMRAG_DEVICE_FILTERS", True)
    engine = FakeEngine()
    m = make_manager(engine)

    async def go():
        await m.initialize()
        assert not m.supports_device_filters()
        for doc in ("da", "db", "dc"):
            await m.embed_and_store([{"id": f"{doc}_{i}", "type": "text" if i % 2 else "table",
                                      "summary": f"{doc} passage {i}"} for i in range(6)], doc)
        col = engine.collections[-1]
        seen = []
        real = col.query
        monkeypatch.setattr(col, "query", lambda **kw: (seen.append(kw["where"]), real(**kw))[1])
        fa, fb = {"doc_id": "da"}, {"$and": [{"doc_id": "db"}, {"type": "table"}]}
        before, encodes = m.stats["total_queries"], len(engine.calls)
        many = await m.batch_filtered_query(["passage 1", " ", "passage 2", "passage 5", "passage 3"],
                                            [fa, fa, fb, dict(fa), None], n_results=3)
        assert m.stats["total_queries"] == before + 4 and len(engine.calls) == encodes + 1      # ONE encode
        assert len(seen) == 3 and fa in seen and fb in seen and None in seen                    # one query per filter
        assert many[1]["error"] == "Query text cannot be empty" and many[1]["ids"] == []
        assert {meta["doc_id"] for meta in many[0]["metadatas"]} == {"da"} == {meta["doc_id"] for meta in many[3]["metadatas"]}
        assert all(meta["doc_id"] == "db" and meta["type"] == "table" for meta in many[2]["metadatas"]) and many[2]["ids"]
        monkeypatch.undo()
        monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
        assert many[2] == await m.query("passage 2", n_results=3, filter_dict=fb)
        assert many[4] == await m.query("passage 3", n_results=3)
        with pytest.raises(ValueError, match="1 filters for 2"):
            await m.batch_filtered_query(["a", "b"], [fa])
        # through the dispatcher: no filtered_fn is wired for this collection even with the setting on
        monkeypatch.setattr(config.settings, "MMRAG_DEVICE_FILTERS", True)
        disp = m.enable_dynamic_batching(max_batch=16, max_wait_ms=50.0)
        try:
            assert disp.filtered_fn is None
            out = await asyncio.gather(m.query("passage 3", 2, fa), m.query("passage 3", 2, fb))
            assert all(meta["doc_id"] == "da" for meta in out[0]["metadatas"]) and len(out[0]["ids"]) == 2
        finally:
            await disp.stop()
            m._dispatcher = None
        await m.cleanup()

    asyncio.run(go())


def test_query_endpoint_filter(monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.server import check_filter, create_app

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    seen = []

    class RecordingManager(EmbeddingManager):
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
        for word in ("alpha", "beta"):
            body = "\n\n".join(f"{word} paragraph number {i} about {word} engines. " * 25 for i in range(4)).encode()
            r = c.post("/upload", files={"file": (f"{word}.txt", body, "text/plain")})
            assert r.status_code == 200, r.text
            docs.append(r.json()["doc_id"])
        seen.clear()
        flt = {"type": {"$in": ["text", "table"]}}
        r = c.post("/query", json={"query": "engines", "top_k": 3, "filter": flt})
        assert r.status_code == 200 and seen == [("query", flt, 3)] and len(r.json()["sources"]) == 3
        seen.clear()
        r = c.post("/query", json={"query": "engines", "top_k": 3, "filter": {"type": "no such type"}})
        assert r.status_code == 200 and r.json()["sources"] == [] and seen == [("query", {"type": "no such type"}, 3)]
        seen.clear()
        both = {"$and": [flt, {"doc_id": {"$in": [docs[1]]}}]}
        r = c.post("/query", json={"query": "engines", "top_k": 2, "filter": flt, "doc_ids": [docs[1]]})
        assert r.status_code == 200 and seen == [("query", both, 2)]            # AND-ed with the documents
        assert all(s["doc_id"].startswith(docs[1]) for s in r.json()["sources"]) and r.json()["sources"]
        seen.clear()
        r = c.post("/query", json={"query": "engines", "top_k": 2, "filter": flt, "doc_ids": [docs[0]], "hybrid": True})
        assert r.status_code == 200 and seen[0] == ("hybrid", {"$and": [flt, {"doc_id": {"$in": [docs[0]]}}]}, 2)
        seen.clear()
        r = c.post("/query", json={"query": "engines", "top_k": 2, "doc_ids": [docs[0]]})
        assert r.status_code == 200 and seen[0] == ("scoped", [docs[0]], 2)      # unchanged without a filter
        r = c.post("/query", json={"query": "engines", "filter": {"page": {"$between": [1, 2]}}})
        assert r.status_code == 400 and r.json()["detail"] == "unsupported where operator '$between'"
        r = c.post("/query", json={"query": "engines", "filter": {"$added_at": {"$gt": 0}}})
        assert r.status_code == 400 and "$added_at" in r.json()["detail"]        # this embedder has no device filters
        leaves = lambda m: {"$or": [{"page": i} for i in range(m)]}             # noqa: E731
        assert c.post("/query", json={"query": "engines", "filter": leaves(32)}).status_code == 200
        r = c.post("/query", json={"query": "engines", "filter": leaves(33)})
        assert r.status_code == 400 and "32 leaves" in r.json()["detail"]
        deep = {"page": 1}
        for _ in range(7):
            deep = {"$and": [deep]}
        assert c.post("/query", json={"query": "engines", "filter": deep}).status_code == 200       # depth 8
        assert c.post("/query", json={"query": "engines", "filter": {"$or": [deep]}}).status_code == 400
        assert c.post("/query", json={"query": "engines", "filter": "type=table"}).status_code == 422
    assert check_filter({"a": {"$gt": 1, "$lt": 5}, "$or": [{"b": 1}, {"$added_at": {"$gte": 3}}]}) == (4, True)
