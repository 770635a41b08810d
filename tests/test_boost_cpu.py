"""No GPU: boosted retrieval's reference (tests/boost_ref.py), the BoostSpec column math and its cache key, the
persistence of the rows' add times, the request validation of POST /query's "boost" and the library's exports."""
import ctypes
import json
import os

import numpy as np
import pytest
from fastapi.testclient import TestClient

from tests import boost_ref as R
from tests.fakes import FakeEngine


def unit_rows(n, d, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


# ---------------------------------------------------------------- 1. the reference
def test_reference_against_a_naive_loop():
    g = np.random.default_rng(1)
    n, B, d, k = 60, 5, 16, 70
    c, q = unit_rows(n, d, 2), unit_rows(B, d, 3)
    prior = g.random(n).astype(np.float32)
    w = np.array([0.5, -1.0, 0.0, 1.0, 0.25], np.float32)
    alive = g.random(n) > 0.2
    s, r, bo = R.boosted_topk(q, c, k, prior, w, alive, row_offset=1000)
    for b in range(B):
        cand = []
        for row in range(n):
            if alive[row]:
                dot = sum(float(q[b, j]) * float(c[row, j]) for j in range(d))
                cand.append((-float(np.float32(dot + float(w[b]) * float(prior[row]))), row))
        cand.sort()
        m = len(cand)
        assert m < k
        assert r[b, :m].tolist() == [row + 1000 for _, row in cand] and np.all(r[b, m:] == -1)
        assert np.allclose(s[b, :m], [-f for f, _ in cand], rtol=0, atol=1e-6) and np.all(np.isneginf(s[b, m:]))
        assert np.array_equal(bo[b, :m], np.array([np.float32(w[b]) * prior[row] for _, row in cand], np.float32))
        assert np.all(bo[b, m:] == 0.0)
    # weight 0: the plain top-k
    s0, r0, b0 = R.boosted_topk(q, c, 5, prior, 0.0)
    assert np.array_equal(r0, np.argsort(-(q.astype(np.float64) @ c.astype(np.float64).T), axis=1, kind="stable")[:, :5])
    assert np.all(b0 == 0.0)


def test_a_resorted_cosine_top50_is_not_the_boosted_top5():
    """why the prior has to be inside the scan: 5 rows with a large prior and a middling cosine are the boosted top-5,
    and none of them is among the 50 best cosines, so no re-sort of that list can find them"""
    n, d = 400, 8
    q = np.zeros((1, d), np.float32)
    q[0, 0] = 1.0
    c = np.zeros((n, d), np.float32)
    cos = np.linspace(0.9, 0.1, n).astype(np.float32)       # row r: cosine falling with r
    c[:, 0] = cos
    c[:, 1] = np.sqrt(1.0 - cos * cos)
    prior = np.zeros(n, np.float32)
    pinned = [200, 230, 260, 290, 320]
    prior[pinned] = 1.0
    s, r, _ = R.boosted_topk(q, c, 5, prior, 1.0)
    _, plain, _ = R.boosted_topk(q, c, 50, prior, 0.0)
    assert r[0].tolist() == pinned
    assert not set(plain[0].tolist()) & set(r[0].tolist())
    # the best a re-sort of the 50 can do is a different list
    resorted = sorted(plain[0].tolist(), key=lambda row: -(cos[row] + prior[row]))[:5]
    assert not set(resorted) & set(pinned)


# ---------------------------------------------------------------- 2. BoostSpec
def test_spec_column_math():
    from multimodal_rag_amd.boost import BoostSpec

    day = 86400.0
    now = 1_700_000_000.0
    times = np.array([now, now - 10 * day, now - 20 * day, now + 5 * day, np.nan])
    metas = [{"type": "text"}, {"type": "table", "pinned": True}, {}, {"type": "image", "pinned": False}, {"type": "table"}]
    spec = BoostSpec(recency=0.8, half_life_s=10 * day)
    col = spec.column(times, metas, now)
    assert col.dtype == np.float32
    # the half-life halves the term; a future time clamps to age 0; an unknown time gives 0
    assert col.tolist() == [np.float32(0.8), np.float32(0.4), np.float32(0.2), np.float32(0.8), 0.0]
    # value weights add, over keys too; a missing key or an unlisted value adds 0
    spec = BoostSpec(values={"type": {"table": 0.3, "image": -0.1}, "pinned": {True: 0.5}})
    assert spec.column(times, metas, now).tolist() == [0.0, np.float32(0.3 + 0.5), 0.0, np.float32(-0.1), np.float32(0.3)]
    # float64 throughout, rounded to float32 ONCE: the sum of the two float32-rounded terms differs
    spec = BoostSpec(recency=1.0, half_life_s=7 * day, values={"type": {"table": 0.1}})
    got = spec.column(times[1:2], metas[1:2], now)[0]
    exact = 2.0 ** (-10.0 / 7.0) + 0.1
    assert got == np.float32(exact)
    terms = [(a, b) for a in (0.1, 0.3, 0.7) for b in (3.0, 10.0, 17.0)]
    once = [BoostSpec(recency=1.0, half_life_s=7 * day, values={"type": {"table": a}}).column(
        np.array([now - b * day]), [{"type": "table"}], now)[0] for a, b in terms]
    twice = [np.float32(np.float32(2.0 ** (-b / 7.0)) + np.float32(a)) for a, b in terms]
    assert once == [np.float32(2.0 ** (-b / 7.0) + a) for a, b in terms] and once != twice
    with pytest.raises(ValueError):
        BoostSpec(recency=float("nan"))
    with pytest.raises(ValueError):
        BoostSpec(half_life_s=0.0)
    with pytest.raises(ValueError):
        spec.column(times, metas[:2], now)


def test_spec_cache_key_and_floored_now():
    from multimodal_rag_amd.boost import BoostSpec, check_prior_values, floored_now

    a = BoostSpec(recency=0.2, values={"type": {"table": 0.3, "image": 0.1}, "pinned": {True: 1.0}})
    b = BoostSpec(recency=0.2, values={"pinned": {True: 1.0}, "type": {"image": 0.1, "table": 0.3}})
    assert a.key() == b.key() and json.loads(a.key())["recency"] == 0.2
    assert a.key() != BoostSpec(recency=0.3).key() != BoostSpec(recency=0.3, half_life_s=5.0).key()
    assert BoostSpec(values={"k": {"1": 1.0}}).key() != BoostSpec(values={"k": {1: 1.0}}).key()
    assert floored_now(7200.0 + 3599.9, 3600.0) == 7200.0 and floored_now(7200.0, 3600.0) == 7200.0
    assert floored_now(1234.5, 0.0) == 1234.5
    clock = lambda: 10_000.0                                                       # noqa: E731
    assert a.cache_key(3600.0, clock) == (a.key(), 7200.0) == b.cache_key(3600.0, lambda: 10_799.0)
    assert a.cache_key(3600.0, lambda: 10_800.0) == (a.key(), 10_800.0)            # the floored time moved on
    fixed = BoostSpec(recency=0.2, now=555.5)
    assert fixed.cache_key(3600.0, clock) == (fixed.key(), 555.5)                  # an explicit now is kept as it is
    assert fixed.batch_key() != BoostSpec(recency=0.2).batch_key() and fixed.key() == BoostSpec(recency=0.2).key()
    assert check_prior_values([1, 2.5], 2).dtype == np.float32
    for bad in ([1.0], [1.0, float("inf")], [1.0, float("nan")], [1.0, 1e300]):
        with pytest.raises(ValueError):
            check_prior_values(bad, 2)


def test_added_at_round_trip_through_the_tables():
    from multimodal_rag_amd.boost import times_from_tables, times_to_tables

    times = np.array([1.5e9, np.nan, 1.7e9 + 0.25])
    tables = json.loads(json.dumps({"count": 3, "added_at": times_to_tables(times)}))
    assert tables["added_at"][1] is None
    back = times_from_tables(tables, 3)
    assert back.dtype == np.float64 and np.array_equal(back, times, equal_nan=True)
    old = times_from_tables({"count": 3}, 3)                # a directory written before the times existed
    assert old.shape == (3,) and np.all(np.isnan(old))
    with pytest.raises(ValueError):
        times_from_tables({"added_at": [1.0]}, 3)


def test_parse_boost_bounds():
    from multimodal_rag_amd.boost import BoostSpec, parse_boost

    assert parse_boost(None) is None and parse_boost(False) is None
    assert parse_boost(True, 0.25, 7.0) == BoostSpec(recency=0.25, half_life_s=7 * 86400.0)
    spec = parse_boost({"recency": 0.5, "half_life_days": 2, "values": {"type": {"table": 0.3}}})
    assert spec == BoostSpec(recency=0.5, half_life_s=2 * 86400.0, values={"type": {"table": 0.3}})
    assert parse_boost({}, 0.1, 3.0) == BoostSpec(recency=0.1, half_life_s=3 * 86400.0)
    many_keys = {f"k{i}": {"v": 1.0} for i in range(9)}
    many_values = {"k": {f"v{i}": 1.0 for i in range(33)}}
    for bad in ("yes", 3, {"recency": 10.5}, {"recency": -11}, {"recency": "1"}, {"recency": True},
                {"half_life_days": 0}, {"half_life_days": -1}, {"values": []}, {"values": {"type": 1.0}},
                {"values": {"type": {"table": 11}}}, {"values": {"type": {"table": "x"}}}, {"values": many_keys},
                {"values": many_values}, {"recenzy": 1.0}, {"values": {"": {"a": 1.0}}}):
        with pytest.raises(ValueError, match="boost"):
            parse_boost(bad)
    assert parse_boost({"values": {f"k{i}": {"v": 1.0} for i in range(8)}}) is not None
    assert parse_boost({"values": {"k": {f"v{i}": -10 for i in range(32)}}, "recency": -10}) is not None


# ---------------------------------------------------------------- 3. POST /query with "boost" over a fake manager
def test_query_endpoint_boost_validation_and_mode_combinations(monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.boost import BoostSpec
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.server import create_app

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    monkeypatch.setattr(config.settings, "MMRAG_BOOST_RECENCY", 0.25)
    monkeypatch.setattr(config.settings, "MMRAG_BOOST_HALF_LIFE_DAYS", 7.0)
    seen = []
    able = {"boost": True}

    class BoostingManager(EmbeddingManager):
        """boosted retrieval is the dense one with the two score columns; records what arrives"""

        def supports_boost(self):
            return able["boost"]

        def supports_hybrid(self):
            return True

        def supports_mmr(self):
            return True

        def supports_grouping(self):
            return True

        def supports_multi_query(self):
            return True

        async def query(self, query_text, n_results=5, filter_dict=None):
            seen.append(("query", filter_dict, n_results))
            return await super().query(query_text, n_results=n_results, filter_dict=filter_dict)

        async def boosted_query(self, query_text, n_results=5, filter_dict=None, boost=None):
            seen.append(("boosted", boost, n_results))
            hits = await super().query(query_text, n_results=n_results, filter_dict=filter_dict)
            m = len(hits["ids"])
            return {**hits, "scores": [1.0 - d + 0.125 for d in hits["distances"]], "boosts": [0.125] * m}

    manager = BoostingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=manager)) as c:
        for word in ("alpha", "beta"):
            body = "\n\n".join(f"{word} paragraph number {i} about {word} engines. " * 25 for i in range(4)).encode()
            assert c.post("/upload", files={"file": (f"{word}.txt", body, "text/plain")}).status_code == 200
        seen.clear()
        plain = c.post("/query", json={"query": "engines", "top_k": 3})
        assert plain.status_code == 200 and seen == [("query", None, 3)]
        assert c.post("/query", json={"query": "engines", "top_k": 3, "boost": False}).json()["sources"] == \
            plain.json()["sources"]
        assert [s[0] for s in seen] == ["query", "query"]          # a non-zero default changes no plain request
        seen.clear()
        r = c.post("/query", json={"query": "engines", "top_k": 3,
                                   "boost": {"recency": 0.5, "half_life_days": 2, "values": {"type": {"table": 0.3}}}})
        assert r.status_code == 200, r.text
        assert seen == [("boosted", BoostSpec(recency=0.5, half_life_s=2 * 86400.0, values={"type": {"table": 0.3}}), 3)]
        src = r.json()["sources"]
        assert len(src) == 3 and all(s["boost"] == 0.125 for s in src)
        assert set(src[0]) == set(plain.json()["sources"][0]) | {"boost", "score"}
        assert [s["relevance_score"] for s in src] == [s["relevance_score"] for s in plain.json()["sources"]]
        assert all(abs(s["score"] - s["relevance_score"] - 0.125) < 1e-3 for s in src)
        seen.clear()
        assert c.post("/query", json={"query": "engines", "boost": True}).status_code == 200
        assert seen == [("boosted", BoostSpec(recency=0.25, half_life_s=7 * 86400.0), 5)]     # the configured defaults
        # bounds: a 400 with the field's name
        for bad in ({"recency": 11}, {"recency": -10.5}, {"half_life_days": 0}, {"values": {"type": {"table": 10.5}}},
                    {"values": {f"k{i}": {"v": 1.0} for i in range(9)}}, {"values": {"k": {f"v{i}": 1 for i in range(33)}}},
                    {"unknown": 1}):
            r = c.post("/query", json={"query": "engines", "boost": bad})
            assert r.status_code == 400 and "boost" in r.json()["detail"], bad
        assert c.post("/query", json={"query": "engines", "boost": "yes"}).status_code == 422
        # not combined with the other modes
        for extra in ({"hybrid": True}, {"mmr": True}, {"group_by_document": True}, {"variants": ["motors"]},
                      {"doc_ids": ["doc_x"]}):
            r = c.post("/query", json={"query": "engines", "boost": {"recency": 0.5}, **extra})
            assert r.status_code == 400 and "Boosted retrieval is not combined" in r.json()["detail"], extra
        able["boost"] = False
        r = c.post("/query", json={"query": "engines", "boost": {"recency": 0.5}})
        assert r.status_code == 400 and "not available with this embedder" in r.json()["detail"]
        assert c.post("/query", json={"query": "engines", "top_k": 3}).json()["sources"] == plain.json()["sources"]


def test_manager_refuses_to_boost_a_collection_without_boosted_query(monkeypatch):
    import asyncio

    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    m = EmbeddingManager(engine=FakeEngine())

    async def go():
        await m.initialize()
        assert not m.supports_boost()
        await m.embed_and_store([{"id": "a_0", "type": "text", "summary": "alpha passage"}], "a")    # no timestamps kwarg
        with pytest.raises(ValueError, match="boosted retrieval needs"):
            await m.boosted_query("alpha", boost={"recency": 0.5})
        with pytest.raises(ValueError, match="boost.recency"):
            await m.boosted_query("alpha", boost={"recency": 50})
        many = await m.batch_boosted_query(["alpha", " "], boost={"recency": 0.5})
        assert "boosted retrieval needs" in many[0]["error"] and many[0]["scores"] == [] and many[1]["boosts"] == []
        disp = m.enable_dynamic_batching(max_batch=4, max_wait_ms=10.0)
        try:
            assert disp.boosted_fn is None
        finally:
            await disp.stop()
            m._dispatcher = None
        await m.cleanup()

    asyncio.run(go())


def test_row_times_and_a_false_boost_are_refused():
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.index import VectorIndex

    assert VectorIndex._row_times(5.0, 3).tolist() == [5.0] * 3
    assert np.array_equal(VectorIndex._row_times([1.0, np.nan], 2), [1.0, np.nan], equal_nan=True)
    assert np.all(np.isnan(VectorIndex._row_times(float("nan"), 2)))
    for bad, m in ((float("inf"), 2), (-np.inf, 1), ([1.0, np.inf], 2), ([1.0], 2)):
        with pytest.raises(ValueError):
            VectorIndex._row_times(bad, m)
    with pytest.raises(ValueError, match="false"):
        EmbeddingManager._boost_spec(False)          # "no boost" to POST /query: not a boosted query
    assert EmbeddingManager._boost_spec(None) == EmbeddingManager._boost_spec(True)


def test_item_times_take_the_configured_key(monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager

    items = [{"id": "a", "published": 1.5e9}, {"id": "b"}, {"id": "c", "published": "soon"},
             {"id": "d", "metadata": {"published": 1.6e9}}, {"id": "e", "published": float("nan")}]
    monkeypatch.setattr(config.settings, "MMRAG_BOOST_TIME_KEY", "")
    assert EmbeddingManager._item_times(items, 7.0) == [7.0] * 5
    monkeypatch.setattr(config.settings, "MMRAG_BOOST_TIME_KEY", "published")
    assert EmbeddingManager._item_times(items, 7.0) == [1.5e9, 7.0, 7.0, 1.6e9, 7.0]


# ---------------------------------------------------------------- 4. the library's exports and argument checks
def test_exports_header_and_argument_checks_need_no_device():
    from multimodal_rag_amd import _native

    L = _native.lib()
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "mmrag.h"), encoding="utf-8") as f:
        header = f.read()
    assert "int mmrag_boosted_topk(" in header and "size_t mmrag_boosted_topk_workspace_bytes(" in header
    assert "mmrag_internal_boosted_topk_ex" not in header
    for name in ("mmrag_boosted_topk", "mmrag_boosted_topk_workspace_bytes", "mmrag_internal_boosted_topk_ex"):
        assert hasattr(L, name), name
    assert _native.boosted_topk_workspace_bytes(256, 1 << 20, 5) > 256 * 16384 * 8
    assert _native.boosted_topk_workspace_bytes(0, 100, 5) == 0 and _native.boosted_topk_workspace_bytes(1, 100, 4097) == 0
    assert _native.boosted_topk_workspace_bytes(1, 1 << 31, 5) == 0

    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255      # never dereferenced: every call below returns before anything is launched
    EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4

    def call(q=p, rows=p, B=4, n=100, d=64, ld=64, dtype=_native.F16, k=5, prior=p, weight=p, out_s=p, out_r=p,
             out_b=None, ws=p, ws_bytes=4096):
        return L.mmrag_boosted_topk(q, rows, B, n, d, ld, dtype, k, 0, None, prior, weight, out_s, out_r, out_b, ws,
                                    ws_bytes, None)

    assert call(out_s=None) == EINVAL and b"null output" in L.mmrag_last_error()
    assert call(out_r=None) == EINVAL
    for name in ("q", "rows", "prior", "weight"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=0) == EINVAL and call(n=-1) == EINVAL and call(n=1 << 31) == EINVAL
    assert call(k=0) == EINVAL and call(k=4097) == EINVAL and call(d=0) == EINVAL and call(ld=63) == EINVAL
    assert call(ld=96) == EINVAL and call(dtype=9) == EINVAL            # 192-byte rows: not whole 128-byte slabs
    assert call(dtype=_native.F8E4M3, ld=128) == EUNSUPPORTED and b"re-scoring plane" in L.mmrag_last_error()
    assert call(ws_bytes=16) == EWORKSPACE and b"workspace" in L.mmrag_last_error()
    assert call(ws=None) == EWORKSPACE
    big = _native.boosted_topk_workspace_bytes(4, 100, 5)
    assert call(ws=p + 4, ws_bytes=big) == EWORKSPACE and b"aligned" in L.mmrag_last_error()
