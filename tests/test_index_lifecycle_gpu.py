"""GPU: one VectorIndex per storage kind with EVERY side structure enabled at once -- two group keys, lexical, sparse, a
token store, a named prior column and a cached BoostSpec column, typed filter columns -- driven through a fixed script
of adds, capacity doublings, tombstones, lazy and explicit compactions, re-adds, a save / load round trip and a reset,
and compared with tests/index_model.py's NumPy model at every numbered checkpoint in every retrieval mode.

The data is exact (tests/index_model.py): every comparison is on ids and on score bits (`same`: np.array_equal of the
float32 words, a zero's sign aside), except the two modes with inexact arithmetic of their own, which keep the rule of
their own GPU tests: BM25 scores through bm25_ref.assert_topk (tests/test_lexical_gpu.py), hybrid fusion through
check_hybrid's rule there, multi-query fusion by fuse_ref bit for bit (tests/test_fuse_gpu.py).

REFUSED lists the (kind, mode) pairs the index refuses -- the modes that need full-precision rows, in FP8 capacity
mode -- and each is asserted to raise its ValueError at every checkpoint.  No checkpoint is thinned for any kind."""
import numpy as np
import pytest
import torch

from tests import bm25_ref, fuse_ref
from tests import index_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F8 = torch.float8_e4m3fn
KINDS = {
    "f16": dict(dtype=torch.float16),
    "bf16": dict(dtype=torch.bfloat16),
    "f32": dict(dtype=torch.float32),
    "f8+f16": dict(dtype=F8, rescore_dtype=torch.float16),
    "f8": dict(dtype=F8, rescore_dtype=None),
}
TOKEN_DTYPE = {"f8+f16": "float8_e4m3fn"}            # every other kind keeps fp16 token rows

NEEDS_PLANE = "needs full-precision rows"
# (kind, mode) -> the message of the documented ValueError; every other pair must answer
REFUSED = {
    ("f8", "mmr_search"): NEEDS_PLANE,
    ("f8", "scoped_search"): NEEDS_PLANE,
    ("f8", "filtered_search"): NEEDS_PLANE,
    ("f8", "range_search"): NEEDS_PLANE,
    ("f8", "related_search"): NEEDS_PLANE,
    ("f8", "boosted_search"): NEEDS_PLANE,
    ("f8", "recommend_search"): NEEDS_PLANE,
    ("f8", "hybrid_query"): NEEDS_PLANE,
    ("f8", "sparse_hybrid_query"): NEEDS_PLANE,
    ("f8", "near_duplicates"): NEEDS_PLANE,
    ("f8", "cluster"): NEEDS_PLANE,
}

W_PLAIN = {"$and": [{"n": {"$gte": 2}}, {"tag": {"$in": ["a", "b"]}}]}           # a numeric and a string-set column
W_TIME = {"$and": [{"n": {"$gte": 2}}, {"tag": {"$in": ["a", "b", "c"]}},        # ... and the time column
                   {"$added_at": {"$gte": M.NOW - 1.5 * M.HOUR}}]}
SPEC = (1.0, M.HOUR, {"tag": {"a": 0.5, "b": -0.25}}, M.NOW)
TEXTS = ["học máy gpu", "vector index tìm kiếm", "zzzz qqqq"]
GROUP_KEYS = ("doc_id", "sec")


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same(got, want) -> bool:
    """equal shape and, number for number, equal float32 / integer words (+0.0 and -0.0 are one number)"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    if got.shape != want.shape:
        return False
    if want.dtype.kind == "f":
        return got.dtype == np.float32 and np.array_equal((got + np.float32(0)).view(np.int32),
                                                          (want.astype(np.float32) + np.float32(0)).view(np.int32))
    return np.array_equal(got.astype(np.int64), want.astype(np.int64))


def raw_equal(got, want) -> bool:
    """tests/test_fuse_gpu.py's bits_equal"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


class Pair:
    """the index of one storage kind and its model, changed in step"""

    def __init__(self, kind: str):
        from multimodal_rag_amd.index import VectorIndex

        self.kind = kind
        self.gen = M.Generator(17)
        self.model = M.IndexModel()
        self.idx = VectorIndex(dim=M.DIM, device=DEV, capacity=256, **KINDS[kind])
        self.deleted: list = []
        self.enable()

    # ---------------------------------------------------------------- the side structures
    def enable(self):
        """everything the kind supports, at once; on a loaded index: what is not persisted, re-filled from the model"""
        from multimodal_rag_amd.boost import BoostSpec

        idx, model = self.idx, self.model
        for key in GROUP_KEYS:
            idx.enable_grouping(key)
            model.enable_grouping(key)
        idx.enable_lexical()
        idx.enable_sparse(M.N_TERMS)
        idx.enable_token_store(M.TOKEN_DIM, 40, dtype=TOKEN_DTYPE.get(self.kind, "float16"))
        self.spec = BoostSpec(recency=SPEC[0], half_life_s=SPEC[1], values=SPEC[2], now=SPEC[3])
        idx.set_prior("fresh", spec=self.spec)
        if model.n:
            live = [i for i, r in enumerate(model.rows) if r["live"]]
            off, terms, imps = M.batch_arrays([model.rows[i] for i in live])[5]
            idx.set_sparse(np.asarray(live, np.int64), off, terms, imps)
            self.set_tokens([model.rows[i] for i in live])
        self.set_pin()

    def set_pin(self):
        values = [((7 * i) % 9 - 4) / 8 for i in range(self.model.count())]
        self.idx.set_prior("pin", values=values)
        self.model.set_prior("pin", values)

    def set_tokens(self, rows):
        toks = np.concatenate([r["tok"] for r in rows] + [np.zeros((0, M.TOKEN_DIM))]).astype(np.float16)
        wrote = self.idx.set_tokens_for_ids([r["id"] for r in rows], toks, [r["tok"].shape[0] for r in rows])
        assert wrote == len(rows)

    # ---------------------------------------------------------------- the operations
    def add(self, m: int, ids=None):
        batch = self.gen.rows(m, ids)
        vecs, docs, metas, ids_, times, sparse = M.batch_arrays(batch)
        self.idx.add(vecs, documents=docs, metadatas=metas, ids=ids_, timestamps=times, sparse=sparse)
        kept = self.model.add(batch)
        self.set_tokens([batch[i] for i in kept])
        return batch

    def delete(self, ids=None, where=None):
        got = self.idx.delete(ids=ids, where=where)
        want = self.model.delete(ids=ids, where=where)
        assert got == want and got
        self.deleted += got

    def stored(self, j: int = 0):
        """the vector of a live row, for a query that scores exactly 1 against it and its twins"""
        live = [r for r in self.model.rows if r["live"]]
        return [live[(11 * j + 3) % len(live)]["vec"]] if live else []


# ------------------------------------------------------------------------------------------------------------------
# one checkpoint: every mode against the model
# ------------------------------------------------------------------------------------------------------------------
def ids_of(idx, rows):
    rows = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    return [idx._ids[int(r)] if r >= 0 else None for r in rows.reshape(-1)]


def refused(kind, mode, call):
    why = REFUSED.get((kind, mode))
    if why is None:
        return False
    with pytest.raises(ValueError, match=why):
        call()
    return True


def check_query(p, q, tag):
    idx, model = p.idx, p.model
    for k in (5, 21):
        for where, flags in ((None, (False, True)), (W_PLAIN, (False, True)), (W_TIME, (True,))):
            s, r = model.search(q, k, where)
            for flag in flags:
                idx.device_filters = flag
                res = idx.query(q, n_results=k, where=where)
                for b in range(len(q)):
                    m = int((r[b] >= 0).sum())
                    ctx = (tag, "query", k, where is not None, flag, b)
                    assert res["ids"][b] == model.ids_of(r[b][:m]), ctx
                    assert res["distances"][b] == (np.float32(1.0) - s[b][:m]).tolist(), ctx
                    assert res["documents"][b] == [model.rows[i]["doc"] for i in r[b][:m]], ctx
                    assert res["metadatas"][b] == [model.rows[i]["meta"] for i in r[b][:m]], ctx
        idx.device_filters = False
        gs, gr = idx.search(q, k, where=W_PLAIN)
        s, r = model.search(q, k, W_PLAIN)
        assert same(gs, s) and ids_of(idx, gr) == model.ids_of(r), (tag, "search", k)


def check_mmr(p, q, tag):
    if refused(p.kind, "mmr_search", lambda: p.idx.mmr_search(q, 5, fetch_k=32, lambda_mult=0.5)):
        return
    for where in (None, W_PLAIN):
        got = p.idx.mmr_search(q, 5, fetch_k=32, lambda_mult=0.5, where=where)
        s, r, pos, val = p.model.mmr(q, 5, 32, 0.5, where)
        assert same(got[0], s) and ids_of(p.idx, got[1]) == p.model.ids_of(r), (tag, "mmr")
        assert same(got[2], pos) and same(got[3], val), (tag, "mmr values")


def check_grouped(p, q, tag):
    from multimodal_rag_amd.config import settings

    idx, model = p.idx, p.model
    for key, G, S, fetch_k, where in (("doc_id", 8, 2, None, None), ("sec", 4, 2, None, W_PLAIN), ("sec", 3, 3, 40, None)):
        got = idx.grouped_search(q, G, S, group_by=key, fetch_k=fetch_k, where=where)
        want = model.grouped(q, G, S, key, fetch_k, where, base=int(settings.MMRAG_GROUP_CANDIDATES))
        assert idx._groups[key]["values"] == model.groups[key], (tag, key)
        for b, (depth, (ws, wr, wp, wg, winfo)) in enumerate(want):
            ctx = (tag, "grouped", key, b)
            assert got[5][b] == depth, ctx
            assert same(got[0][b], ws) and ids_of(idx, got[1][b]) == model.ids_of(wr), ctx
            assert same(got[2][b], wp) and same(got[3][b], wg) and same(got[4][b], winfo), ctx


def some_documents(model, n):
    docs = [v for v, c in zip(model.groups["doc_id"], model.group_counts("doc_id")) if c]
    return [docs[(5 * j + 1) % len(docs)] for j in range(n)] if docs else ["none"] * n


def check_scoped(p, q, tag):
    docs = some_documents(p.model, 3)
    scopes = [[docs[0], docs[1]], [docs[2]], ["no such document"]][: len(q)]
    if refused(p.kind, "scoped_search", lambda: p.idx.scoped_search(q, 5, scopes)):
        return
    for where in (None, W_PLAIN):
        gs, gr = p.idx.scoped_search(q, 5, scopes, key="doc_id", where=where)
        s, r = p.model.scoped(q, 5, scopes, "doc_id", where)
        assert same(gs, s) and ids_of(p.idx, gr) == p.model.ids_of(r), (tag, "scoped", where is not None)


def check_filtered(p, q, tag):
    wheres = [W_TIME, None, W_PLAIN][: len(q)]
    if refused(p.kind, "filtered_search", lambda: p.idx.filtered_search(q, 5, wheres)):
        return
    for k in (5, 21):
        gs, gr = p.idx.filtered_search(q, k, wheres)
        s, r = p.model.filtered(q, k, wheres)
        assert same(gs, s) and ids_of(p.idx, gr) == p.model.ids_of(r), (tag, "filtered", k)


def check_range(p, q, tag):
    wheres = [None, W_TIME, W_PLAIN][: len(q)]
    thr = [0.25, 0.125, 0.125][: len(q)]
    if refused(p.kind, "range_search", lambda: p.idx.range_search(q, thr, 10, wheres, GROUP_KEYS)):
        return
    counts, tables, gs, gr, values = p.idx.range_search(q, thr, limit=10, wheres=wheres, facets=GROUP_KEYS)
    wc, wt, s, r = p.model.range(q, thr, 10, wheres, GROUP_KEYS)
    assert same(counts, wc), (tag, "range counts", counts.tolist(), wc.tolist())
    for key, got_t, want_t, vals in zip(GROUP_KEYS, tables, wt, values):
        assert vals == p.model.groups[key] and same(got_t, want_t), (tag, "range facets", key)
    assert same(gs, s) and ids_of(p.idx, gr) == p.model.ids_of(r), (tag, "range hits")


def check_related(p, q, tag):
    model = p.model
    docs = model.power_of_two_documents()
    sets = ([{"value": docs[len(docs) // 2]}] if docs else []) + [q[:2].astype(np.float64) if len(q) > 1 else q.astype(np.float64)]
    if len(q) > 1:
        sets.append(q[2:3].astype(np.float64))
    call = lambda where=None: p.idx.related_search([s if isinstance(s, dict) else s.astype(np.float32) for s in sets], 4,  # noqa: E731
                                                   key="doc_id", threshold=0.75, where=where)
    if refused(p.kind, "related_search", call):
        return
    for where in (None, W_PLAIN):
        sim, grp, cov, best, brow = call(where)
        want = model.related(sets, 4, "doc_id", 0.75, where)
        ctx = (tag, "related", where is not None)
        assert same(sim, want[0]) and same(grp, want[1]) and same(cov, want[2]), ctx
        assert same(best, want[3]) and ids_of(p.idx, brow) == model.ids_of(want[4]), ctx


def check_boosted(p, q, tag):
    weights = [1.0, 0.25, 2.0][: len(q)]
    if refused(p.kind, "boosted_search", lambda: p.idx.boosted_search(q, 7, prior="pin")):
        return
    for prior, mprior, w, where in (("pin", "pin", weights, None), ("fresh", SPEC, 0.5, W_PLAIN), (p.spec, SPEC, weights, None)):
        gs, gr, gb = p.idx.boosted_search(q, 7, prior=prior, weight=w, where=where)
        s, r, b = p.model.boosted(q, 7, mprior, w, where)
        assert same(gs, s) and ids_of(p.idx, gr) == p.model.ids_of(r) and same(gb, b), (tag, "boosted", str(prior)[:12])
    assert len(p.idx._spec_cols) == 1                    # the name and the spec itself share one cached column


def check_recommend(p, q, tag):
    live = p.model.live_ids()
    named = [live[len(live) // 3], live[-1]] if live else []
    pos = [[*named[:1], q[0]], [q[-1], *named[1:]], [q[1 % len(q)]]][: len(q)]
    neg = [[q[-1]], [], [*named[:1]]][: len(q)]
    if refused(p.kind, "recommend_search", lambda: p.idx.recommend_search(pos, neg, 6, negative_weight=0.5)):
        return
    for where in (None, W_PLAIN):
        got = p.idx.recommend_search(pos, neg, n_results=6, negative_weight=0.5, where=where)
        want = p.model.recommend(pos, neg, 6, 0.5, where)
        ctx = (tag, "recommend", where is not None)
        assert same(got[0], want[0]) and ids_of(p.idx, got[1]) == p.model.ids_of(want[1]), ctx
        hit = want[1] >= 0
        for g_, w_ in zip(got[2:], want[2:]):
            g_ = g_.cpu().numpy()
            assert same(g_[hit], w_[hit]), ctx


def check_fused(p, q, tag):
    from multimodal_rag_amd.config import settings

    off = [0, 2, 3] if len(q) == 3 else [0, 1]
    depth = int(settings.MMRAG_FUSE_CANDIDATES)
    weights = np.array([1.0, 0.5, 2.0][: len(q)], np.float32)
    for method, w, where in (("rrf", None, None), ("max", weights, W_PLAIN)):
        got = p.idx.fused_search(q, off, 8, weights=w, method=method, where=where)
        want = p.model.fused(q, off, 8, depth, w, method, int(settings.MMRAG_FUSE_RRF_K), where)
        for name, g_, w_ in zip(("fused", "rows", "best", "best_list", "count", "info"), got, want):
            if name == "rows":
                assert ids_of(p.idx, g_) == p.model.ids_of(w_), (tag, "fused", method)
            else:
                assert raw_equal(g_, w_), (tag, "fused", method, name)


def check_late(p, q, tag):
    lens = [3, 4, 2][: len(q)]
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1].tolist()
    qt = M.exact_rows(np.random.default_rng(len(tag) + len(q)), int(sum(lens)), M.TOKEN_DIM)
    q_dev = torch.from_numpy(qt.astype(np.float16)).to(DEV)
    for where in (None, W_PLAIN):
        gs, gr = p.idx.late_search(q_dev, starts, lens, 6, where=where)
        s, r = p.model.late(qt, starts, lens, 6, where, f8=p.kind in TOKEN_DTYPE)
        assert same(gs, s) and ids_of(p.idx, gr) == p.model.ids_of(r), (tag, "late", where is not None)


def check_lexical(p, q, tag):
    idx, model = p.idx, p.model
    texts = TEXTS[: len(q)]
    k = 10
    for where in (None, W_PLAIN):
        res = idx.lexical_query(texts, n_results=k, where=where)
        allowed = model.visible(where) if model.n else np.zeros(0, bool)
        for b, text in enumerate(texts):
            acc, matched = model.lexical(text)
            rows = [model.row_of(i) for i in res["ids"][b]]
            assert all(r >= 0 for r in rows), (tag, "lexical returned a dead id")
            got_s = np.full(k, -np.inf, np.float32)
            got_r = np.full(k, -1, np.int64)
            got_s[: len(rows)] = res["lexical_scores"][b]
            got_r[: len(rows)] = rows
            bm25_ref.assert_topk(got_s, got_r, acc, matched, allowed, k)
            assert res["documents"][b] == [model.rows[r]["doc"] for r in rows]


def check_hybrid(p, q, tag):
    from multimodal_rag_amd.config import settings

    idx, model = p.idx, p.model
    texts = TEXTS[: len(q)]
    n_results = 7
    if refused(p.kind, "hybrid_query", lambda: idx.hybrid_query(q, texts, n_results=n_results)):
        return
    C = max(n_results, settings.MMRAG_HYBRID_CANDIDATES)
    res = idx.hybrid_query(q, texts, n_results=n_results)
    ds, dr = model.search(q, C)
    X = model.matrix().astype(np.float64)
    for b, text in enumerate(texts):
        lex_rows = model.lexical_rows(text, C).tolist()
        d_rows = [int(r) for r in dr[b] if r >= 0]
        want = bm25_ref.rrf(d_rows, lex_rows, settings.MMRAG_HYBRID_RRF_K)[:n_results]
        got = [model.row_of(i) for i in res["ids"][b]]
        assert got == [r for r, _ in want], (tag, "hybrid", b)
        assert res["hybrid_scores"][b] == [s for _, s in want]
        cos = X[got] @ q[b].astype(np.float64) if got else np.zeros(0)
        np.testing.assert_allclose(res["distances"][b], 1.0 - cos, rtol=0, atol=1e-6)
        for r, s in zip(got, res["lexical_scores"][b]):
            assert (s > 0) == (r in lex_rows)


def check_sparse(p, q, tag):
    from multimodal_rag_amd.config import settings

    idx, model = p.idx, p.model
    sq = M.Generator(len(tag) * 7 + len(q)).sparse_queries(len(q))
    for where in (None, W_PLAIN):
        gs, gr = idx.sparse_search(sq, 7, where=where)
        s, r = model.sparse(sq, 7, where)
        assert same(gs, s) and ids_of(idx, gr) == model.ids_of(r), (tag, "sparse", where is not None)
    if refused(p.kind, "sparse_hybrid_query", lambda: idx.sparse_hybrid_query(q, sq, n_results=7)):
        return
    C = max(7, settings.MMRAG_HYBRID_CANDIDATES)
    res = idx.sparse_hybrid_query(q, sq, n_results=7)
    ds, dr = model.search(q, C)
    ss, sr = model.sparse(sq, C)
    norm = idx._sparse_norm(None)
    X = model.matrix().astype(np.float64)
    for b in range(len(q)):
        d_rows = [int(r) for r in dr[b] if r >= 0]
        s_rows = [int(r) for r in sr[b] if r >= 0]
        want = bm25_ref.rrf(d_rows, s_rows, settings.MMRAG_HYBRID_RRF_K)[:7]
        got = [model.row_of(i) for i in res["ids"][b]]
        assert got == [r for r, _ in want], (tag, "sparse hybrid", b)
        assert res["hybrid_scores"][b] == [s for _, s in want]
        by_row = {r: float(ss[b][i]) / norm for i, r in enumerate(s_rows)}
        assert res["sparse_scores"][b] == [by_row.get(r, 0.0) for r in got]
        cos = (X[got] @ q[b].astype(np.float64)).astype(np.float32) if got else np.zeros(0, np.float32)
        assert res["distances"][b] == (np.float32(1.0) - cos).tolist()


def check_duplicates(p, tag):
    idx, model = p.idx, p.model
    if refused(p.kind, "near_duplicates", lambda: idx.near_duplicates(threshold=1.0)):
        return
    for t, where in ((1.0, None), (0.75, W_PLAIN)):
        rep = idx.near_duplicates(threshold=t, where=where)
        pairs, groups = model.near_duplicates(t, where)
        want = [(model.rows[a]["id"], model.rows[b]["id"], v) for (a, b), v in sorted(pairs.items())]
        assert rep["total_pairs"] == len(want) and not rep["truncated"], (tag, "duplicates", t)
        assert [(a, b, float(np.float32(v))) for a, b, v in rep["pairs"]] == want, (tag, "duplicate pairs", t)
        assert rep["groups"] == [model.ids_of(g_) for g_ in groups], (tag, "duplicate groups", t)
    if model.count() > 20:
        assert idx.near_duplicates(threshold=1.0)["total_pairs"] > 0          # the planted twins are there


def check_cluster_assign(p, tag):
    """k-means for its assign step only: one iteration from seed rows of distinct vectors, so the centroids are stored
    rows and every score is exact"""
    idx, model = p.idx, p.model
    seeds, seen = [], set()
    for r in model.rows:
        if r["live"] and r["vec"].tobytes() not in seen and len(seeds) < 4:
            seen.add(r["vec"].tobytes())
            seeds.append(r["id"])
    if refused(p.kind, "cluster", lambda: idx.cluster(init=seeds or None, n_clusters=None if seeds else 1)):
        return
    for where in (None, W_PLAIN):
        vis = model.visible(where) if model.n else np.zeros(0, bool)
        mine = [i for i in seeds if vis[model.row_of(i)]]
        if not mine:
            assert idx.cluster(n_clusters=1, where={"n": -1})["n_clusters"] == 0, (tag, "cluster of nothing")
            continue
        out = idx.cluster(init=mine, where=where, max_iter=1, tol=1.0, return_labels=True)
        arg, best = model.assign(mine, where)
        assert out["converged"] and out["iterations"] == 1, (tag, "cluster")
        assert out["labels"] == {model.rows[i]["id"]: int(arg[i]) for i in np.nonzero(vis)[0]}, (tag, "cluster labels")
        assert out["objective"] == [float(best[vis].sum()) / int(vis.sum())], (tag, "cluster objective")


def check_tables(p, tag):
    idx, model = p.idx, p.model
    assert idx.count() == model.count() and idx.rows_in_use == model.n, (tag, idx.count(), idx.rows_in_use)
    live = model.live_ids()
    ask = live[:3] + p.deleted[:2] + ["never stored"] + live[-2:]
    for where in (None, W_PLAIN):
        got = idx.get(ids=ask, where=where, include=("metadatas", "documents", "embeddings"))
        want = model.get(ids=ask, where=where)
        for key in ("ids", "documents", "metadatas", "embeddings"):
            assert got[key] == want[key], (tag, "get", key)
    got, want = idx.get(where=W_PLAIN), model.get(where=W_PLAIN)
    assert got["ids"] == want["ids"] and got["documents"] == want["documents"], (tag, "get where")
    assert [i for i in idx.rows_of_ids(live)] == [model.row_of(i) for i in live]
    assert np.array_equal(idx.row_times().view(np.int64), model.row_times().view(np.int64)), (tag, "row_times")


def check_invariants(p, tag):
    """what ties the structures together"""
    idx, model = p.idx, p.model
    cap, n = idx.matrix.shape[0], idx.rows_in_use
    dev_words = idx._alive_dev.cpu().numpy()
    assert np.array_equal(idx._alive_host.view(np.int32), dev_words), (tag, "alive words: host != device")
    flags = np.zeros(dev_words.size * 32, bool)
    flags[:n] = model.alive()
    assert np.array_equal(np.packbits(flags, bitorder="little").view(np.int32), dev_words), (tag, "alive words")
    assert dev_words.size == idx._n_words(cap) and idx._added_at.size == cap
    per_row = [st["col"] for st in idx._groups.values()] + [st["col"] for st in idx._spec_cols.values()]
    per_row += [c for c in idx._priors.values() if isinstance(c, torch.Tensor)]
    if idx.plane is not None:
        per_row.append(idx.plane)
    # two group columns, the named prior, the spec's cached column once a boosted search built it, the FP8 plane
    expect = 3 + ((p.kind, "boosted_search") not in REFUSED) + (idx.plane is not None)
    assert len(per_row) == expect and all(t.shape[0] == cap for t in per_row), (tag, cap, [t.shape[0] for t in per_row])
    for key in GROUP_KEYS:
        st = idx._groups[key]
        col = st["col"].cpu().numpy()
        assert np.array_equal(col[:n], model.group_column(key)) and np.all(col[n:] == -1), (tag, "group column", key)
        in_use = np.bincount(col[:n][col[:n] >= 0], minlength=len(st["values"])).tolist()
        assert st["counts"] == in_use, (tag, "group counts", key)          # dead rows count until a compaction
        if idx.count() == n:
            assert st["counts"] == model.group_counts(key), (tag, "group counts over live rows", key)
    assert np.array_equal(idx._priors["pin"].cpu().numpy()[:n], model.prior_column("pin")), (tag, "prior column")
    for st in idx._spec_cols.values():
        assert np.array_equal(st["col"].cpu().numpy()[:n], model.prior_column(SPEC)), (tag, "spec column")
    off = idx.token_store.device_offsets(n).cpu().numpy()
    assert off.shape == (n + 1,) and np.array_equal(off, model.token_plane()[1]), (tag, "token offsets")
    assert idx._lex.n == n and idx._sparse.n == n, (tag, "postings rows", idx._lex.n, idx._sparse.n)
    s_off, s_terms, s_imps = model.sparse_log()
    assert np.array_equal(idx._sparse._off_host, s_off) and np.array_equal(idx._sparse._term_host, s_terms)
    assert np.array_equal(idx._sparse._imp_host, s_imps), (tag, "sparse log")


def checkpoint(p: Pair, number):
    tag = f"{p.kind}#{number}"
    check_tables(p, tag)
    for B in (1, 3):
        q = M.Generator(1000 + 10 * (number if isinstance(number, int) else 99) + B).queries(B, p.stored(B))
        check_query(p, q, tag)
        check_mmr(p, q, tag)
        check_grouped(p, q, tag)
        check_scoped(p, q, tag)
        check_filtered(p, q, tag)
        check_range(p, q, tag)
        check_related(p, q, tag)
        check_boosted(p, q, tag)
        check_recommend(p, q, tag)
        check_fused(p, q, tag)
        check_late(p, q, tag)
        check_lexical(p, q, tag)
        check_hybrid(p, q, tag)
        check_sparse(p, q, tag)
    check_duplicates(p, tag)
    check_cluster_assign(p, tag)
    check_invariants(p, tag)


# ------------------------------------------------------------------------------------------------------------------
# the script
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_mode_follows_the_model_through_the_lifecycle(kind, tmp_path):
    from multimodal_rag_amd.persistence import load_index, save_index

    p = Pair(kind)
    idx, model = p.idx, p.model

    # 1. 200 rows, nothing deleted
    p.add(200)
    p.set_pin()
    assert idx.matrix.shape[0] == 256
    checkpoint(p, 1)

    # 2. the add that crosses 256: _reserve doubles mid-script; the batch repeats ids inside itself and names ids that exist
    ids = [f"r{200 + i}" for i in range(100)]
    ids[5], ids[40], ids[41], ids[97] = "r3", "r210", "r210", "r199"
    ids[60] = ids[59]
    p.add(100, ids)
    assert idx.rows_in_use == model.n == 295 and idx.matrix.shape[0] == 512
    checkpoint(p, 2)

    # 3. 512 and 1024 crossed in one large add, then on to about 1 500 rows
    p.add(900, [f"r{300 + i}" for i in range(900)])
    assert idx.rows_in_use == 1195 and idx.matrix.shape[0] == 1195
    p.add(305, [f"r{1200 + i}" for i in range(305)])
    assert idx.rows_in_use == 1500 and idx.matrix.shape[0] == 2390
    checkpoint(p, 3)

    # 4. scattered tombstones, below the lazy-compaction threshold: the first row, the last row, a whole document, rows
    # whose exact twin stays alive (one on each side), every 37th row, and a delete by `where`
    twin = next(i for i in range(400, 500) if np.array_equal(model.rows[i]["vec"], model.rows[i - 9]["vec"]))
    p.delete(ids=[model.rows[0]["id"], model.rows[-1]["id"], model.rows[twin]["id"], model.rows[twin + 5 - 9]["id"]])
    p.delete(where={"doc_id": model.rows[333]["meta"]["doc_id"]})
    p.delete(ids=[model.rows[i]["id"] for i in range(7, 1500, 37)])
    p.delete(where={"$and": [{"n": 9}, {"tag": "d"}]})
    assert idx.rows_in_use == 1500 and 40 < 1500 - idx.count() < 375
    checkpoint(p, 4)

    # 5. the lazy compaction, from inside delete (the threshold lowered on the instance, the class untouched)
    idx.COMPACT_MIN_DEAD = model.compact_min_dead = 8
    p.delete(where={"tag": "b"})
    assert type(idx).COMPACT_MIN_DEAD == 4096 and idx.rows_in_use == idx.count() == model.n < 1125
    assert idx.matrix.shape[0] == 2390
    checkpoint(p, 5)

    # 6. an explicit compact() with fewer than a quarter of the capacity alive shrinks it; the next add grows it again
    del idx.COMPACT_MIN_DEAD
    model.compact_min_dead = 4096
    p.delete(where={"n": {"$gte": 5}})
    assert idx.rows_in_use > idx.count() and idx.count() < 2390 // 4
    idx.compact()
    model.compact()
    assert idx.matrix.shape[0] == 1195 and idx.rows_in_use == idx.count() == model.n
    p.add(700, [f"r{2000 + i}" for i in range(700)])
    assert idx.matrix.shape[0] == 2390
    checkpoint(p, 6)

    # 7. deleted ids come back with new vectors, text, tokens and sparse vectors, as new rows at the end; live ids among
    # them are ignored
    back = p.deleted[::9][:60] + model.live_ids()[:5]
    before = model.n
    p.add(len(back), back)
    assert model.n == before + len(back) - 5 and idx.rows_in_use == model.n
    p.delete(ids=back[:3])                                    # and tombstones again, so the save below has to compact
    checkpoint(p, 7)

    # 8. save -> load: the rows, their tables and their add times persist; everything else is re-enabled and re-filled
    times_before = idx.row_times()
    save_index(idx, str(tmp_path / kind))
    model.compact()                                           # save_index compacts
    loaded = load_index(str(tmp_path / kind), device=DEV)
    assert loaded.dtype == idx.dtype and loaded.rescore_dtype == idx.rescore_dtype
    assert np.array_equal(loaded.row_times().view(np.int64), times_before.view(np.int64))      # bit for bit
    assert np.array_equal(times_before.view(np.int64), model.row_times().view(np.int64))
    p.idx = idx = loaded
    model.groups, model.prior_names = {}, []                  # derived state is rebuilt from the rows as they are now
    for r in model.rows:
        r["priors"] = {}
    p.enable()
    checkpoint(p, 8)

    # 9. reset: the empty index gives every mode's empty answer; then a small add
    cap = idx.matrix.shape[0]
    idx.reset()
    model.reset()
    p.deleted = []
    assert not idx._groups and not idx._priors and not idx._spec_cols            # reset drops what is derived
    assert idx.matrix.shape[0] == cap and idx.count() == idx.rows_in_use == 0
    assert idx._lex.n == idx._sparse.n == 0 and idx.token_store.n_rows == 0 and idx.token_store.n_items == 0
    p.enable()
    checkpoint(p, "empty")
    p.add(40, [f"z{i}" for i in range(40)])
    p.set_pin()
    p.delete(ids=["z7"])
    checkpoint(p, 9)
