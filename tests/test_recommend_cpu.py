"""No GPU: recommend retrieval's reference (tests/recommend_ref.py), why the penalty cannot be applied to a finished
list, pack_examples' layout and refusals, the request validation of POST /query's "like" / "unlike" / "not" and of
POST /recommend, the manager's request rules and the library's exports."""
import asyncio
import ctypes
import os

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

from tests import recommend_ref as R
from tests.fakes import FakeEngine

E = 16


def unit_rows(n, d, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


# ---------------------------------------------------------------- 1. the reference
def test_reference_against_a_naive_loop():
    n, d, k, R_ = 60, 12, 7, 5
    c = unit_rows(n, d, 1)
    counts = [(1, 0), (3, 2), (1, 15), (16, 0), (2, 1)]
    pos = [unit_rows(p, d, 10 + i) for i, (p, _) in enumerate(counts)]
    neg = [unit_rows(m, d, 20 + i) if m else np.zeros((0, d), np.float32) for i, (_, m) in enumerate(counts)]
    neg[1][0] = c[5]                                   # a negative that bites
    ex, sign = R.pack(pos, neg, d)
    assert ex.shape == (E * R_, d) and sign.reshape(R_, E)[2].tolist() == [1] + [-1] * 15
    w = np.array([1.0, 0.5, 0.25, 1.0, 0.0], np.float32)
    alive = np.ones(n, bool)
    alive[[3, 17]] = False
    s, r, po, ne, pa, na = R.recommend_topk(ex, sign, w, c, k, alive, row_offset=100)
    for g in range(R_):
        scored = []
        for row in range(n):
            if not alive[row]:
                continue
            pd = [float(np.dot(p.astype(np.float64), c[row].astype(np.float64))) for p in pos[g]]
            nd = [float(np.dot(q.astype(np.float64), c[row].astype(np.float64))) for q in neg[g]]
            best_n = max(nd) if nd else 0.0
            final = np.float32(max(pd) - float(w[g]) * max(best_n, 0.0))
            scored.append((-final, row, max(pd), best_n, pd.index(max(pd)), len(pd) + nd.index(best_n) if nd else -1))
        scored.sort(key=lambda t: (t[0], t[1]))
        for j, (mf, row, p_, n_, pa_, na_) in enumerate(scored[:k]):
            assert s[g, j] == -mf and r[g, j] == row + 100
            assert po[g, j] == np.float32(p_) and ne[g, j] == np.float32(n_) and pa[g, j] == pa_ and na[g, j] == na_
    # fewer live rows than k: (-inf, -1) and 0 / -1 padding
    s, r, po, ne, pa, na = R.recommend_topk(ex, sign, w, c[:4], 6, np.array([1, 0, 1, 1], bool))
    assert np.all(np.isneginf(s[:, 3:])) and np.all(r[:, 3:] == -1) and np.all(po[:, 3:] == 0) and np.all(pa[:, 3:] == -1)
    assert np.all(na[3] == -1) and np.all(ne[3] == 0)                     # a request without a negative


def half_circle():
    ang = np.deg2rad(np.linspace(-90.0, 90.0, 400))
    return np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32), np.rad2deg(ang)


def test_a_resorted_cosine_top50_is_not_the_recommend_top5():
    """400 unit rows on a half circle, the positive at 0 degrees, one negative at 30 degrees, weight 1: the five best
    finals sit near -60 degrees (cosine 0.5) and none is among the 50 best cosines, so no re-sort of a finished list
    finds them.  Without the negative the result is the plain top-k."""
    c, deg = half_circle()
    p = np.array([[1.0, 0.0]], np.float32)
    q = np.array([[np.cos(np.pi / 6), np.sin(np.pi / 6)]], np.float32)
    ex, sign = R.pack([p], [q], 2)
    s, r, po, ne, pa, na = R.recommend_topk(ex, sign, 1.0, c, 5)
    cos = c.astype(np.float64) @ p[0].astype(np.float64)
    top50 = set(np.lexsort((np.arange(400), -cos))[:50].tolist())
    assert not set(r[0].tolist()) & top50
    assert np.all(np.abs(deg[r[0]] + 60.0) < 2.5) and np.all(np.abs(po[0] - 0.5) < 0.03)
    assert np.all(pa == 0) and np.all(na == 1)
    ex0, sign0 = R.pack([p], None, 2)
    s0, r0, _, ne0, _, na0 = R.recommend_topk(ex0, sign0, 1.0, c, 5)
    plain = np.lexsort((np.arange(400), -cos.astype(np.float32)))[:5]
    assert np.array_equal(r0[0], plain) and np.array_equal(s0[0], cos[plain].astype(np.float32))
    assert np.all(ne0 == 0) and np.all(na0 == -1)
    # a row is never rewarded for being unlike a negative: with the negative opposite the positive nothing changes
    ex1, sign1 = R.pack([p], [-p], 2)
    s1, r1, *_ = R.recommend_topk(ex1, sign1, 1.0, c, 5)
    assert np.array_equal(r1, r0) and np.array_equal(s1, s0)


# ---------------------------------------------------------------- 2. pack_examples
def test_pack_examples_layout_and_refusals():
    from multimodal_rag_amd import _native

    d = 24
    v = unit_rows(8, d, 3)
    ex, sign = _native.pack_examples([[v[0]], [v[1], v[2].tolist(), torch.from_numpy(v[3])]], [None, [v[4], v[5]]], d,
                                     torch.float16, "cpu")
    ld = _native.padded_dim(d, torch.float16)
    assert ex.shape == (2 * E, ld) and ex.dtype == torch.float16 and sign.dtype == torch.int8
    assert sign.reshape(2, E).tolist() == [[1] + [0] * 15, [1, 1, 1, -1, -1] + [0] * 11]
    want = np.zeros((2 * E, ld), np.float32)
    want[0, :d] = v[0]
    want[E: E + 5, :d] = v[1:6]
    assert np.array_equal(ex.float().numpy(), torch.from_numpy(want).to(torch.float16).float().numpy())
    ref_ex, ref_sign = R.pack([v[:1], v[1:4]], [None, v[4:6]], d)
    assert np.array_equal(ref_sign, sign.numpy()) and np.array_equal(ref_ex, want[:, :d])
    # stored rows as examples: ints, gathered from the rows given
    rows = torch.zeros((5, ld), dtype=torch.float16)
    rows[:, :d] = torch.from_numpy(unit_rows(5, d, 4)).to(torch.float16)
    ex2, sign2 = _native.pack_examples([[3, v[0]]], [[1]], d, torch.float16, "cpu", rows=rows)
    assert sign2.tolist() == [1, 1, -1] + [0] * 13
    assert torch.equal(ex2[0], rows[3]) and torch.equal(ex2[2], rows[1]) and torch.equal(ex2[1], ex[0])
    full = [[v[i % 8] for i in range(9)]], [[v[i % 8] for i in range(7)]]
    assert _native.pack_examples(*full, d, torch.float32, "cpu")[1].tolist() == [1] * 9 + [-1] * 7
    for pos, neg in (([], None),                                      # no request
                     ([[]], None), ([[v[0]], []], None),              # a request without a positive
                     ([[]], [[v[0]]]),                                # negatives alone
                     ([[v[i % 8] for i in range(17)]], None),         # 17 examples
                     ([[v[i % 8] for i in range(9)]], [[v[i % 8] for i in range(8)]]),
                     ([[v[0]]], [None, None]),                        # negative lists for other requests
                     ([[v[0][:-1]]], None),                           # a wrong length
                     ([[2.0 * v[0]]], None), ([[v[0]]], [[0.5 * v[1]]]), ([[np.zeros(d)]], None),     # not unit vectors
                     ([[np.full(d, np.nan)]], None),
                     ([[3]], None)):                                  # a stored row without the rows
        with pytest.raises(ValueError):
            _native.pack_examples(pos, neg, d, torch.float16, "cpu")
    with pytest.raises(ValueError):
        _native.pack_examples([[5]], None, d, torch.float16, "cpu", rows=rows)       # past the rows given
    assert _native.MAX_RECOMMEND_EXAMPLES == E


def test_request_check_of_the_wrapper():
    from multimodal_rag_amd import _native

    sign = np.zeros(2 * E, np.int8)
    sign[[0, 1, E]] = 1
    sign[2] = -1
    s, w = _native.check_recommend_request("t", sign, 0.5, 2)
    assert s.dtype == np.int8 and w.dtype == np.float32 and w.tolist() == [0.5, 0.5]
    assert _native.check_recommend_request("t", sign.tolist(), [0.0, 1.0], 2)[1].tolist() == [0.0, 1.0]
    for one in (np.float32(0.25), np.array(0.25), torch.tensor(0.25)):       # 0-d: the same for every request
        assert _native.check_recommend_request("t", sign, one, 2)[1].tolist() == [0.25, 0.25]
    assert _native.check_recommend_request("t", None, None, 2) == (None, None)
    two, none = sign.copy(), sign.copy()
    two[3] = 2
    none[E] = -1
    for s_, w_ in ((two, 1.0), (none, 1.0), (sign[:-1], 1.0), (sign, -0.5), (sign, float("nan")), (sign, [1.0, np.inf]),
                   (sign, [1.0]), (sign, [1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            _native.check_recommend_request("t", s_, w_, 2)


# ---------------------------------------------------------------- 3. the manager's request rules
def test_manager_request_rules_and_a_collection_that_cannot():
    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager

    req = EmbeddingManager._recommend_request
    assert req("q", like=["a"], unlike_texts=["t"]) == {"query_text": "q", "like": ["a"], "unlike": [],
                                                          "unlike_texts": ["t"], "negative_weight": None}
    assert req(None, like=["a"])["query_text"] is None
    for bad in (dict(), dict(query_text=" "), dict(unlike=["a"]), dict(query_text="q", like="a"),
                dict(query_text="q", like=[""]), dict(query_text="q", unlike_texts=[" "]),
                dict(query_text="q", like=["a"] * 8, unlike=["b"] * 8),                        # 17 in all
                dict(like=["a"] * 10, unlike_texts=["t"] * 7), dict(query_text="q", negative_weight=-1.0),
                dict(query_text="q", negative_weight=float("inf"))):
        with pytest.raises(ValueError):
            req(**bad)
    assert len(req("q", like=["a"] * 8, unlike=["b"] * 7)["like"]) == 8                       # 16 in all
    assert config.settings.MMRAG_RECOMMEND_NEGATIVE_WEIGHT == 1.0

    m = EmbeddingManager(engine=FakeEngine())

    async def go():
        await m.initialize()
        assert not m.supports_recommend()
        with pytest.raises(ValueError, match="recommend retrieval needs"):
            await m.recommend("alpha", unlike_texts=["beta"])
        with pytest.raises(ValueError, match="question or at least one"):
            await m.recommend(None)
        many = await m.batch_recommend([{"query_text": "alpha"}, {"unlike": ["x"]}])
        assert "recommend retrieval needs" in many[0]["error"] and "question or at least one" in many[1]["error"]
        assert many[0]["scores"] == [] and many[1]["repelled_by"] == []
        disp = m.enable_dynamic_batching(max_batch=4, max_wait_ms=10.0)
        try:
            assert disp.recommend_fn is None
            with pytest.raises(ValueError):
                await disp.submit("", 5, None, None, recommend={"query_text": "alpha"})
        finally:
            await disp.stop()
            m._dispatcher = None
        await m.cleanup()

    asyncio.run(go())


def test_dispatcher_tells_a_bad_request_from_a_failing_engine():
    """an 'error' dict of a recommend_fn is the request's own fault (ValueError, a 400 of POST /query); what it raises
    reaches the caller as it is (a 500)"""
    from multimodal_rag_amd.dispatcher import QueryDispatcher

    seen = []

    async def plain(texts, k, flt):
        return [{"ids": []} for _ in texts]

    async def recommend_fn(requests, k, flt):
        seen.append((list(requests), k, flt))
        if any(r.get("boom") for r in requests):
            raise RuntimeError("the device fell over")
        return [{"ids": [], "error": "Item not found: x"} if r.get("like") == ["x"] else {"ids": ["ok"]} for r in requests]

    async def go():
        disp = QueryDispatcher(plain, max_batch=8, max_wait_ms=50.0, recommend_fn=recommend_fn)
        try:
            good, bad = await asyncio.gather(disp.submit("", 3, None, None, recommend={"like": ["a"]}),
                                             disp.submit("", 3, None, None, recommend={"like": ["x"]}),
                                             return_exceptions=True)
            assert good == {"ids": ["ok"]} and isinstance(bad, ValueError) and "Item not found" in str(bad)
            assert len(seen) == 1 and len(seen[0][0]) == 2              # one batch for the two
            with pytest.raises(RuntimeError, match="fell over"):
                await disp.submit("", 3, None, None, recommend={"boom": True})
            both = await asyncio.gather(disp.submit("", 3, {"type": "text"}, None, recommend={"like": ["a"]}),
                                        disp.submit("", 3, None, None, recommend={"like": ["b"]}))
            assert both == [{"ids": ["ok"]}] * 2 and len(seen) == 4      # another filter: another alive bitmap, another scan
        finally:
            await disp.stop()

    asyncio.run(go())


# ---------------------------------------------------------------- 4. POST /query and POST /recommend over a fake manager
def test_endpoints_validation_and_mode_combinations(monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.server import create_app

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    seen = []
    able = {"recommend": True}

    class RecommendingManager(EmbeddingManager):
        """recommend retrieval is the dense one with the four columns; records what arrives"""

        def supports_recommend(self):
            return able["recommend"]

        def supports_hybrid(self):
            return True

        def supports_mmr(self):
            return True

        def supports_grouping(self):
            return True

        def supports_multi_query(self):
            return True

        def supports_boost(self):
            return True

        async def query(self, query_text, n_results=5, filter_dict=None):
            seen.append(("query", filter_dict, n_results))
            return await super().query(query_text, n_results=n_results, filter_dict=filter_dict)

        async def recommend(self, query_text=None, like=(), unlike=(), unlike_texts=(), n_results=5, filter_dict=None,
                            negative_weight=None):
            req = self._recommend_request(query_text, like, unlike, unlike_texts, negative_weight)
            seen.append(("recommend", req, n_results, filter_dict))
            if "nobody" in req["like"] + req["unlike"]:
                raise ValueError("Item not found: nobody")
            hits = await super().query(query_text or "engines", n_results=n_results, filter_dict=filter_dict)
            m = len(hits["ids"])
            return {**hits, "scores": [1.0 - d - 0.125 for d in hits["distances"]], "penalties": [0.125] * m,
                    "matched": ["query" if query_text else like[0]] * m,
                    "repelled_by": [(list(unlike) + list(unlike_texts) + [None])[0]] * m}

    manager = RecommendingManager(engine=FakeEngine())
    with TestClient(create_app(embedder=manager)) as c:
        for word in ("alpha", "beta"):
            body = "\n\n".join(f"{word} paragraph number {i} about {word} engines. " * 25 for i in range(4)).encode()
            assert c.post("/upload", files={"file": (f"{word}.txt", body, "text/plain")}).status_code == 200
        seen.clear()
        plain = c.post("/query", json={"query": "engines", "top_k": 3})
        assert plain.status_code == 200 and seen == [("query", None, 3)]
        some_id = plain.json()["sources"][0]["doc_id"]
        seen.clear()
        r = c.post("/query", json={"query": "engines", "top_k": 3, "like": [some_id], "not": ["beta engines"],
                                   "negative_weight": 0.5})
        assert r.status_code == 200, r.text
        assert seen == [("recommend", {"query_text": "engines", "like": [some_id], "unlike": [],
                                       "unlike_texts": ["beta engines"], "negative_weight": 0.5}, 3, None)]
        src = r.json()["sources"]
        assert len(src) == 3 and set(src[0]) == set(plain.json()["sources"][0]) | {"score", "penalty", "matched",
                                                                                   "repelled_by"}
        assert all(s["penalty"] == 0.125 and s["matched"] == "query" and s["repelled_by"] == "beta engines" for s in src)
        assert [s["relevance_score"] for s in src] == [s["relevance_score"] for s in plain.json()["sources"]]
        assert r.json()["answer"]
        seen.clear()
        assert c.post("/query", json={"query": "engines", "unlike": [some_id]}).status_code == 200
        assert seen[0][1]["unlike"] == [some_id] and seen[0][1]["negative_weight"] is None and seen[0][2] == 5
        # malformed: the schema's 422, the rules' 400
        for bad in ({"like": []}, {"not": []}, {"like": "x"}, {"not": [""]}, {"like": ["x"] * 17},
                    {"like": ["x"], "negative_weight": -1}):
            assert c.post("/query", json={"query": "engines", **bad}).status_code == 422, bad
        r = c.post("/query", json={"query": "engines", "like": ["x"] * 8, "unlike": ["y"] * 8})
        assert r.status_code == 400 and "at most 16 examples" in r.json()["detail"]
        r = c.post("/query", json={"query": "engines", "negative_weight": 0.5})
        assert r.status_code == 400 and "negative_weight" in r.json()["detail"]
        r = c.post("/query", json={"query": "engines", "like": ["nobody"]})
        assert r.status_code == 400 and "Item not found" in r.json()["detail"]
        # not combined with the other modes
        for extra in ({"hybrid": True}, {"mmr": True}, {"group_by_document": True}, {"variants": ["motors"]},
                      {"expand": 2}, {"doc_ids": ["doc_x"]}, {"boost": {"recency": 0.5}}):
            for mine in ({"like": [some_id]}, {"unlike": [some_id]}, {"not": ["beta"]}):
                r = c.post("/query", json={"query": "engines", **mine, **extra})
                assert r.status_code == 400 and "not combined" in r.json()["detail"], (mine, extra)
        # POST /recommend: stored items as examples, no question, no answer
        seen.clear()
        r = c.post("/recommend", json={"like": [some_id], "unlike": ["other"], "not": ["beta"], "top_k": 2,
                                       "filter": {"type": "text"}})
        assert r.status_code == 200, r.text
        assert seen == [("recommend", {"query_text": None, "like": [some_id], "unlike": ["other"],
                                       "unlike_texts": ["beta"], "negative_weight": None}, 2, {"type": "text"})]
        out = r.json()
        assert set(out) == {"sources", "processing_time"} and len(out["sources"]) == 2
        assert all(s["matched"] == some_id and s["repelled_by"] == "other" and "score" in s for s in out["sources"])
        for bad in ({}, {"like": []}, {"unlike": ["x"]}, {"like": ["x"], "top_k": 0}, {"like": ["x"], "top_k": 21},
                    {"like": ["x"] * 17}):
            assert c.post("/recommend", json=bad).status_code == 422, bad
        r = c.post("/recommend", json={"like": ["x"] * 9, "not": ["t"] * 8})
        assert r.status_code == 400 and "at most 16 examples" in r.json()["detail"]
        r = c.post("/recommend", json={"like": ["nobody"]})
        assert r.status_code == 400 and "Item not found" in r.json()["detail"]
        able["recommend"] = False
        for path, body in (("/query", {"query": "engines", "not": ["beta"]}), ("/recommend", {"like": [some_id]})):
            r = c.post(path, json=body)
            assert r.status_code == 400 and "not available with this embedder" in r.json()["detail"]
        # a request without these keys is what it was
        after = c.post("/query", json={"query": "engines", "top_k": 3}).json()
        assert after["sources"] == plain.json()["sources"] and after["answer"] == plain.json()["answer"]


# ---------------------------------------------------------------- 5. the library's exports and argument checks
def test_exports_header_and_argument_checks_need_no_device():
    from multimodal_rag_amd import _native

    L = _native.lib()
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "mmrag.h"), encoding="utf-8") as f:
        header = f.read()
    assert "int mmrag_recommend_topk(" in header and "size_t mmrag_recommend_topk_workspace_bytes(" in header
    assert "#define MMRAG_MAX_RECOMMEND_EXAMPLES 16" in header
    assert "mmrag_internal_recommend_topk_ex" not in header
    for name in ("mmrag_recommend_topk", "mmrag_recommend_topk_workspace_bytes", "mmrag_internal_recommend_topk_ex"):
        assert hasattr(L, name), name
    assert _native.recommend_topk_workspace_bytes(64, 1 << 20, 5) > 64 * 16384 * 8
    assert _native.recommend_topk_workspace_bytes(0, 100, 5) == 0
    assert _native.recommend_topk_workspace_bytes(1, 100, 4097) == 0
    assert _native.recommend_topk_workspace_bytes(1, 1 << 31, 5) == 0

    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255      # never dereferenced: every call below returns before anything is launched
    EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4

    def call(ex=p, sign=p, w=p, rows=p, R_=4, n=100, d=64, ld=64, dtype=_native.F16, k=5, out_s=p, out_r=p, ws=p,
             ws_bytes=4096):
        return L.mmrag_recommend_topk(ex, sign, w, rows, R_, n, d, ld, dtype, k, 0, None, out_s, out_r, None, None, None,
                                      None, ws, ws_bytes, None)

    assert call(out_s=None) == EINVAL and b"null output" in L.mmrag_last_error()
    assert call(out_r=None) == EINVAL
    for name in ("ex", "sign", "w", "rows"):
        assert call(**{name: None}) == EINVAL, name
    assert call(R_=0) == EINVAL and call(n=-1) == EINVAL and call(n=1 << 31) == EINVAL
    assert call(k=0) == EINVAL and call(k=4097) == EINVAL and call(d=0) == EINVAL and call(ld=63) == EINVAL
    assert call(ld=96) == EINVAL and call(dtype=9) == EINVAL            # 192-byte rows: not whole 128-byte slabs
    assert call(sign=p + 1) == EINVAL and b"aligned" in L.mmrag_last_error()
    assert call(dtype=_native.F8E4M3, ld=128) == EUNSUPPORTED and b"re-scoring plane" in L.mmrag_last_error()
    assert call(ws_bytes=16) == EWORKSPACE and b"workspace" in L.mmrag_last_error()
    assert call(ws=None) == EWORKSPACE
    big = _native.recommend_topk_workspace_bytes(4, 100, 5)
    assert call(ws=p + 4, ws_bytes=big) == EWORKSPACE and b"aligned" in L.mmrag_last_error()
