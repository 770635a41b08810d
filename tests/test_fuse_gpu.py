"""GPU: multi-query fusion (csrc/fuse.hip through _native.fuse_select, VectorIndex, EmbeddingManager and POST /query)
against tests/fuse_ref.py.  Every comparison with the reference is exact, floats bit for bit: the definition fixes the
order of every float32 operation, and the index-level tests feed both sides the same lists."""
import asyncio

import numpy as np
import pytest
import torch

from tests import fuse_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("fused", "rows", "best", "best_list", "count", "info")
CS = [1, 63, 64, 65, 256]
NS = [1, 5, 64, 4096]
PATTERNS = ["identical", "disjoint", "overlap", "tails", "dup", "special", "bigrows", "tiekeys"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


def bits_equal(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def make_group(g, nl, C, pattern):
    """one group's lists: scores [nl, C] float32 descending, rows [nl, C] int64"""
    if nl == 0:
        return np.zeros((0, C), F), np.zeros((0, C), np.int64)
    if pattern == "identical":
        rows = np.tile(g.choice(5 * C + 5, C, replace=False), (nl, 1))
    elif pattern in ("disjoint", "tiekeys"):
        rows = g.permutation(nl * C + 7)[: nl * C].reshape(nl, C)
    else:
        rows = np.stack([g.choice(2 * C + 3, C, replace=False) for _ in range(nl)])
    rows = rows.astype(np.int64)
    scores = -np.sort(-g.standard_normal((nl, C)).astype(F), axis=1)
    if pattern == "identical":
        scores = np.tile(scores[0], (nl, 1))
    if pattern == "tiekeys":
        # equal weights and disjoint lists: all rows of one rank tie on fused under rrf; long runs of equal scores,
        # and two lists with the same scores, make many of them tie on best too, so the row decides
        scores = (np.round(scores * 1.5) / 1.5).astype(F)
        if nl > 1:
            scores[1] = scores[0]
    if pattern == "special" and C > 2:                     # bit patterns a float comparison would lose
        scores[:, C // 2] = F(-0.0)
        scores[:, -1] = F(-1e-42)
        scores[nl // 2] = (np.round(scores[nl // 2] * 1.5) / 1.5).astype(F)
    if pattern == "tails":
        for l in range(nl):
            cut = [C // 2, 0, 1, C - 1, C][l % 5]          # list 1 of a group is entirely empty
            live = rows[l].copy()
            rows[l, cut:], scores[l, cut:] = -1, -np.inf
            rows[l, cut + 1:] = live[cut + 1:]             # what follows the first -1 is live rows again: not to be read
    if pattern == "dup" and C > 2:
        for l in range(nl):
            rows[l, C - 1] = rows[l, 0]
            rows[l, C // 2] = rows[l, 1] if l % 2 else rows[l, 0]
    if pattern == "bigrows":                               # above 2**32 and near 2**62; the map keeps rows distinct
        rows = np.where(rows % 5 == 0, (1 << 62) - 1 - rows, rows + ((rows % 4) << 32))
    return np.ascontiguousarray(scores), np.ascontiguousarray(rows)


def make_case(counts, C, pattern, seed):
    """a call: lists of all groups stacked, list_off, and weights holding 0 and a negative value"""
    g = np.random.default_rng(seed)
    parts = [make_group(g, nl, C, pattern) for nl in counts]
    scores = np.concatenate([p[0] for p in parts])
    rows = np.concatenate([p[1] for p in parts])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    weights = g.choice(np.array([0, -1, .5, 1, 2, 1.25], F), len(rows)).astype(F)
    if len(rows) > 1:
        weights[0], weights[-1] = 0, -1
    return scores, rows, off, weights


def run_kernel(dev, scores, rows, off, n, weights=None, method="rrf", rrf_k=60, device_off=False):
    from multimodal_rag_amd import _native

    w = None if weights is None else torch.from_numpy(weights).to(dev)
    o = torch.from_numpy(off).to(dev) if device_off else off
    out = _native.fuse_select(torch.from_numpy(scores).to(dev), torch.from_numpy(rows).to(dev), o, n, weights=w,
                              method=method, rrf_k=rrf_k)
    return [t.cpu().numpy() for t in out]


def check_against_reference(dev, case, what, ns=NS, rrf_k=60):
    scores, rows, off, weights = case
    for method in ("rrf", "max"):
        for w in (None, weights):
            full = R.fuse_select(scores, rows, off, 4096, w, method, rrf_k)    # the answer for n is its first n slots
            for n in ns:
                got = run_kernel(dev, scores, rows, off, n, w, method, rrf_k)
                for name, g_, w_ in zip(NAMES, got, full):
                    want = w_ if name == "info" else np.ascontiguousarray(w_[:, :n])
                    assert bits_equal(g_, want), (what, method, w is not None, n, name,
                                                  np.argwhere(g_ != want)[:4].tolist())


# ---------------------------------------------------------------- 1. the kernel against the reference
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("C", CS)
def test_kernel_equals_reference(dev, C, pattern):
    # every list count of the issue in one ragged launch, a group without lists among them
    check_against_reference(dev, make_case([1, 2, 0, 3, 16], C, pattern, seed=100 * C + len(pattern)), (C, pattern))


@pytest.mark.parametrize("counts", [[2, 0, 16], [0, 3, 1], [16, 16, 0]])
def test_three_ragged_groups_in_one_launch(dev, counts):
    """G = 3, a group that owns no lists among them, at a list length on each side of a wave"""
    for C, pattern in ((63, "overlap"), (65, "tails"), (256, "tiekeys")):
        check_against_reference(dev, make_case(counts, C, pattern, seed=sum(counts) + C), (counts, C, pattern))


@pytest.mark.parametrize("nl", [1, 2, 3, 16])
def test_single_group_launch(dev, nl):
    for C in (1, 65):
        check_against_reference(dev, make_case([nl], C, "overlap", seed=nl + C), (nl, C), rrf_k=0)


def test_seventy_ragged_groups_and_a_group_is_independent_of_its_launch(dev):
    g = np.random.default_rng(70)
    counts = g.choice([0, 1, 2, 3, 16], 70).tolist()
    counts[0], counts[37], counts[69] = 0, 3, 0
    case = make_case(counts, 65, "overlap", seed=71)
    check_against_reference(dev, case, "G=70", ns=[5, 4096])
    scores, rows, off, weights = case
    lo, hi = int(off[37]), int(off[38])
    alone_off = np.array([0, hi - lo], np.int32)
    for method in ("rrf", "max"):
        for n in (5, 4096):
            whole = run_kernel(dev, scores, rows, off, n, weights, method)
            alone = run_kernel(dev, scores[lo:hi].copy(), rows[lo:hi].copy(), alone_off, n, weights[lo:hi].copy(), method)
            again = run_kernel(dev, scores, rows, off, n, weights, method, device_off=True)
            for name, a, b, c in zip(NAMES, whole, alone, again):
                assert bits_equal(a[37:38], b), (method, n, name)
                assert bits_equal(a, c), (method, n, name)


@pytest.mark.parametrize("pattern", ["disjoint", "overlap", "tiekeys"])
def test_full_size_group(dev, pattern):
    """16 lists x 256 entries: 4096 entries in one workgroup, with 4096 distinct rows when the lists are disjoint"""
    case = make_case([16], 256, pattern, seed=4096)
    check_against_reference(dev, case, ("full", pattern), ns=[64, 4096])
    if pattern == "disjoint":
        info = run_kernel(dev, *case[:3], 4096)[5]
        assert info.tolist() == [[4096, 4096]]


def test_native_argument_checks(dev):
    from multimodal_rag_amd import _native

    def call(L=4, C=10, off=(0, 2, 4), n=3, **kw):
        s = torch.zeros((L, C), dtype=torch.float32, device=dev)
        r = torch.arange(L * C, dtype=torch.int64, device=dev).reshape(L, C)
        return _native.fuse_select(s, r, list(off), n, **kw)

    for bad in (dict(C=257), dict(n=0), dict(n=4097), dict(rrf_k=-1), dict(method="sum"), dict(off=(0, 4)[:1]),
                dict(off=(0, 3)), dict(off=(1, 4)), dict(off=(0, 3, 2, 4)), dict(L=17, off=(0, 17)),
                dict(weights=torch.ones(3, device=dev)), dict(weights=torch.ones(4, device=dev).double())):
        with pytest.raises(_native.MMRagNativeError):
            call(**bad)
    for good in (dict(C=256), dict(C=1), dict(n=4096), dict(n=1), dict(rrf_k=0), dict(L=16, off=(0, 16)),
                 dict(L=0, off=(0, 0)), dict(weights=torch.ones(4, device=dev))):
        out = call(**good)
        assert out[0].shape == (len(good.get("off", (0, 2, 4))) - 1, good.get("n", 3))
    assert call(L=0, off=(0, 0, 0))[5].tolist() == [[0, 0], [0, 0]]
    s = torch.zeros((4, 10), dtype=torch.float32, device=dev)
    r = torch.zeros((4, 10), dtype=torch.int64, device=dev)
    for args in ((s.cpu(), r), (s, r.int()), (s.t().contiguous().t(), r), (s, r[:, :5]), (s.double(), r)):
        with pytest.raises(_native.MMRagNativeError):
            _native.fuse_select(*args, [0, 4], 3)
    with pytest.raises(_native.MMRagNativeError):
        _native.fuse_select(s, r, torch.tensor([0, 4], device=dev), 3)             # a device list_off is int32


def test_graph_capture_replays_the_same_bits(dev):
    from multimodal_rag_amd import _native

    scores, rows, off, weights = make_case([3, 0, 4, 1], 50, "overlap", seed=9)
    s, r, o, w = (torch.from_numpy(x).to(dev) for x in (scores, rows, off, weights))
    eager = [t.clone() for t in _native.fuse_select(s, r, o, 10, weights=w)]
    side = torch.cuda.Stream()                                             # one stream, no parallel branches
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _native.fuse_select(s, r, o, 10, weights=w)                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _native.fuse_select(s, r, o, 10, weights=w)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---------------------------------------------------------------- 2. through VectorIndex
N_ROWS, DIM = 3000, 128
KINDS = {"fp16": dict(dtype=torch.float16), "fp32": dict(dtype=torch.float32),
         "fp8-rescored": dict(dtype=torch.float8_e4m3fn, rescore_dtype=torch.float16),
         "fp8-capacity": dict(dtype=torch.float8_e4m3fn, rescore_dtype=None)}


@pytest.fixture(scope="module")
def corpus():
    g = np.random.default_rng(3000)
    centres = g.standard_normal((40, DIM))
    x = centres[g.integers(0, 40, N_ROWS)] + 0.8 * g.standard_normal((N_ROWS, DIM))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F)
    # 5 questions of 4, 1, 3, 16 and 2 phrasings: a stored row plus noise, the phrasings of a question near each other
    counts = [4, 1, 3, 16, 2]
    q = []
    for nl in counts:
        base = x[g.integers(0, N_ROWS)] + 0.5 * g.standard_normal(DIM) / np.sqrt(DIM)
        q.append(base + 0.35 * g.standard_normal((nl, DIM)) / np.sqrt(DIM))
    q = np.concatenate(q)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    return x, q, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def build_index(dev, x, **kw):
    from multimodal_rag_amd.index import VectorIndex

    idx = VectorIndex(dim=x.shape[1], device=dev, capacity=len(x), **kw)
    idx.add(x, documents=[f"text {i}" for i in range(len(x))], ids=[f"id{i}" for i in range(len(x))],
            metadatas=[{"doc_id": f"doc{i // 10}", "parity": i % 2} for i in range(len(x))])
    return idx


def check_fused_search(idx, q, off, n, want_depth, weights=None, method=None, where=None, fetch_k=None):
    got = [t.cpu().numpy() for t in idx.fused_search(q, off, n, fetch_k=fetch_k, weights=weights, method=method,
                                                     where=where)]
    s, r = (t.cpu().numpy() for t in idx.search(q, want_depth, where=where))   # the same rows of the batch, same depth
    want = R.fuse_select(s, r, off, n, None if weights is None else np.asarray(weights, F), method or "rrf", 60)
    for name, g_, w_ in zip(NAMES, got, want):
        assert bits_equal(g_, w_), (name, n, method, np.argwhere(g_ != w_)[:4].tolist())
    return got, (s, r)


@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_search_equals_reference_over_search(dev, corpus, kind):
    x, q, off = corpus
    idx = build_index(dev, x, **KINDS[kind])
    weights = np.where(np.arange(len(q)) % 3 == 0, 1.0, 0.5).astype(F)
    got, (s, r) = check_fused_search(idx, q, off, 10, 50)                          # MMRAG_FUSE_CANDIDATES = 50, rrf
    assert (got[1] >= 0).all() and (got[4][1] == 1).all() and got[4][3].max() > 1  # one phrasing: every count is 1
    check_fused_search(idx, q, off, 10, 50, weights=weights, method="max")
    check_fused_search(idx, q, off, 80, 80, weights=weights)                       # n_results above the default depth
    check_fused_search(idx, q, off, 5, 20, fetch_k=20, method="max")               # the register-list search
    check_fused_search(idx, q, off, 300, 256, fetch_k=1000)                        # capped at 256
    # a filter, and rows deleted before the call
    got, _ = check_fused_search(idx, q, off, 10, 50, where={"parity": 1})
    assert (got[1] % 2 == 1).all()
    gone = sorted({int(v) for v in r[:, :3].ravel()})
    idx.delete(ids=[f"id{i}" for i in gone])
    got, _ = check_fused_search(idx, q, off, 10, 50, weights=weights)
    assert not set(got[1].ravel().tolist()) & set(gone)
    res = idx.fused_query(q, off, n_results=10, weights=weights)
    assert set(res) == {"ids", "distances", "metadatas", "documents", "embeddings", "fused_scores", "matched_queries",
                        "best_query"}
    for g_ in range(len(off) - 1):
        assert res["ids"][g_] == [f"id{i}" for i in got[1][g_]] and res["fused_scores"][g_] == got[0][g_].tolist()
        assert res["matched_queries"][g_] == got[4][g_].tolist() and res["best_query"][g_] == got[3][g_].tolist()
        assert res["distances"][g_] == (F(1) - got[2][g_]).tolist()
        assert res["documents"][g_] == [f"text {i}" for i in got[1][g_]]
    for bad in (dict(n_results=0), dict(n_results=4097), dict(method="sum"), dict(weights=[1.0]), dict(fetch_k=0)):
        with pytest.raises(ValueError):
            idx.fused_query(q, off, **{"n_results": 5, **bad})
    with pytest.raises(ValueError):
        idx.fused_query(q, [0, 17, len(q)], n_results=5)                           # 17 phrasings of one question
    with pytest.raises(ValueError):
        idx.fused_query(q, off[:-1], n_results=5)                                  # list_off does not cover the rows


def test_planted_row_wins_under_rrf_not_under_max(dev):
    """exact in every dtype: phrasing v scores its own A_v = 1, its own B_v = 3/4 and the planted row 1/2, so each
    ranks the planted row third and nothing else is returned twice"""
    d = 64
    x = np.zeros((4 + 4 + 1 + 20, d), F)
    for v in range(4):
        x[v, v] = 1.0                                                              # A_v
        x[4 + v, v] = 0.75                                                         # B_v: 9/16 + 7 * 1/16
        x[4 + v, 8 + 7 * v: 15 + 7 * v] = 0.25
    x[8, :4] = 0.5                                                                 # the planted row
    for i in range(20):
        x[9 + i, 40 + i] = 1.0                                                     # bystanders, orthogonal to all
    q = np.eye(d, dtype=F)[:4]
    idx = build_index(dev, x, dtype=torch.float16)
    lists = idx.query(q, n_results=3)
    assert [ids for ids in lists["ids"]] == [[f"id{v}", f"id{4 + v}", "id8"] for v in range(4)]
    assert lists["distances"] == [[0.0, 0.25, 0.5]] * 4
    rrf = idx.fused_query(q, [0, 4], n_results=9, fetch_k=3, method="rrf")
    assert rrf["ids"][0][0] == "id8" and rrf["matched_queries"][0] == [4] + [1] * 8
    assert rrf["fused_scores"][0][0] == float(((F(1) / F(63) + F(1) / F(63)) + F(1) / F(63)) + F(1) / F(63))
    assert rrf["ids"][0][1:5] == ["id0", "id1", "id2", "id3"] and rrf["best_query"][0][:5] == [0, 0, 1, 2, 3]
    top = idx.fused_query(q, [0, 4], n_results=9, fetch_k=3, method="max")
    assert top["ids"][0] == [f"id{i}" for i in range(9)] and top["matched_queries"][0][8] == 4
    assert top["fused_scores"][0] == [1.0] * 4 + [0.75] * 4 + [0.5]


# ---------------------------------------------------------------- 3. end to end
def reference_over_hits(collection, per_variant, n, method="rrf", weights=None):
    """the reference over per-variant result dicts: ranks from their order, scores from their distances"""
    row_of = {i: r for r, i in enumerate(collection._ids)}
    C = max(len(h["ids"]) for h in per_variant)
    rows = np.full((len(per_variant), C), -1, np.int64)
    scores = np.full((len(per_variant), C), -np.inf, F)
    for l, h in enumerate(per_variant):
        rows[l, : len(h["ids"])] = [row_of[i] for i in h["ids"]]
        scores[l, : len(h["ids"])] = F(1) - np.asarray(h["distances"], F)
    f, r, *_ = R.fuse_group(scores, rows, weights, R.METHODS[method], 60, n)
    keep = r >= 0
    return [collection._ids[i] for i in r[keep]], f[keep].tolist()


def test_through_embedding_manager(dev):
    from multimodal_rag_amd.embedder import EmbeddingManager

    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_multi_query()
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình"]
    g = np.random.default_rng(62)
    for doc, count in (("long", 120), ("mid", 30), ("short", 4)):
        texts = [" ".join(g.choice(words, int(g.integers(3, 9)))) + f" {doc} {i}" for i in range(count)]
        items = [{"id": f"{doc}_{i}", "type": "text", "summary": t} for i, t in enumerate(texts)]
        asyncio.run(m.embed_and_store(items, doc))
    variants = ["học máy dữ liệu", "mô hình học máy", "dữ liệu cho mô hình", "gpu kernel"]
    before = m.stats["total_queries"]
    out = asyncio.run(m.multi_query(variants, n_results=7))
    assert m.stats["total_queries"] == before + 1
    assert set(out) == {"ids", "distances", "metadatas", "documents", "fused_scores", "matched_queries", "best_query"}
    per = asyncio.run(m.batch_query(variants, n_results=50))                        # MMRAG_FUSE_CANDIDATES = 50
    ids, fused = reference_over_hits(m.collection, per, 7)
    assert out["ids"] == ids and out["fused_scores"] == fused
    weighted = asyncio.run(m.multi_query(variants, n_results=7, weights=[1.0, 0.5, 0.5, 0.25], method="max"))
    ids, fused = reference_over_hits(m.collection, per, 7, "max", np.array([1.0, 0.5, 0.5, 0.25], F))
    # under "max" the fused value is made of the score itself, and a hit dict carries 1 - score: the round trip
    # 1 - (1 - s) is exact for s >= 1/2 and within one unit of 2^-24 below
    assert weighted["ids"] == ids and np.abs(np.asarray(weighted["fused_scores"]) - np.asarray(fused)).max() <= 2.0 ** -24
    many = asyncio.run(m.batch_multi_query([variants, [], variants[:1]], n_results=7))
    assert all(many[0][key] == out[key] for key in ("ids", "fused_scores", "matched_queries", "best_query"))
    assert many[1]["error"] == "Query text cannot be empty" and many[1]["ids"] == []
    assert many[2]["ids"] == per[0]["ids"][:7] and many[2]["matched_queries"] == [1] * 7
    with pytest.raises(ValueError):
        asyncio.run(m.multi_query([]))
    asyncio.run(m.cleanup())


def test_query_endpoint_with_variants(dev):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    app = create_app()
    with TestClient(app) as c:
        bodies = [" ".join(f"Học máy là gì, phần {i}." for i in range(60)), "GPU kernel và dữ liệu. " * 3,
                  "Machine learning cơ bản, học máy. " * 3, "Bảng và ảnh. " * 3]
        for i, body in enumerate(bodies):
            assert c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")}).status_code == 200
        plain = c.post("/query", json={"query": "học máy", "top_k": 4})
        assert plain.status_code == 200 and all("fused_score" not in s for s in plain.json()["sources"])
        texts = ["học máy", "machine learning", "gpu kernel"]
        r = c.post("/query", json={"query": texts[0], "top_k": 4, "variants": texts[1:]})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        m = app.state.components["embedder"]
        per = asyncio.run(m.batch_query(texts, n_results=50))
        ids, fused = reference_over_hits(m.collection, per, 4)
        assert [s["doc_id"] for s in src] == ids and [s["fused_score"] for s in src] == fused
        assert all(1 <= s["matched_queries"] <= 3 for s in src)
        for other in ("mmr", "hybrid", "group_by_document"):
            assert c.post("/query", json={"query": "học máy", "variants": ["x"], other: True}).status_code == 400
        assert c.post("/query", json={"query": "học máy", "expand": 2}).status_code == 400
