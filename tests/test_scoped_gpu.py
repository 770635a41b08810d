"""GPU: document-scoped retrieval (csrc/scoped.hip through _native.scoped_topk, VectorIndex.scoped_search /
scoped_query, EmbeddingManager and the dispatcher) against tests/scoped_ref.py.

The bar is tests/test_search_gpu.py's: scores within 1e-4 of the reference, identical id sets with candidates within
2e-4 of the k-th score interchangeable; bit-equal wherever the data is exactly representable or where two runs of the
kernel are compared (a score's bits depend on the query row, the stored row and d alone)."""
import asyncio

import numpy as np
import pytest
import torch

from oracle import search_oracle as O
from tests import scoped_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def unit_rows(n, d, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def to_dev(N, x, dtype):
    n, d = x.shape
    ld = N.padded_dim(d, dtype)
    t = torch.zeros((max(n, 1), ld), dtype=dtype, device="cuda")
    if n:
        t[:n, :d] = torch.from_numpy(x).to("cuda").to(dtype)
    return t, t[:n, :d].to(torch.float32).cpu().numpy()


def bits_of(alive):
    words = np.zeros((alive.size + 31) // 32 + 8, dtype=np.uint32)
    idx = np.nonzero(alive)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32)).to("cuda")


def check(s, r, es, er):
    assert r.shape == er.shape and s.shape == es.shape
    fin = np.isfinite(es)
    assert np.array_equal(np.isfinite(s), fin)
    assert np.array_equal(r[~fin], er[~fin])  # -1 padding
    assert np.all(np.abs(s[fin] - es[fin]) <= TOL)
    assert np.all(np.diff(s, axis=1)[fin[:, 1:]] <= 0)  # descending
    assert O.same_topk_sets(r, s, er, es)


def documents(n, seed):
    """group_of_row [n] int32 and the number of ordinals: contiguous documents of 1 .. max(1, min(200, n // 40)) rows
    (one of 200 rows over rows 100 .. 299 when n >= 1000), one document across the rows 126 .. 129, ordinals a random
    permutation of 0 .. n_groups-1 with n_groups >= 100 (more than two bitmap words), about 5 % of the rows -1"""
    g = np.random.default_rng(seed)
    longest = max(1, min(200, n // 40))
    doc_of, at, docs = np.zeros(n, np.int64), 0, 0
    while at < n:
        m = int(g.integers(1, longest + 1))
        doc_of[at:at + m] = docs
        at, docs = at + m, docs + 1
    if n >= 1000:
        doc_of[100:300] = doc_of[100]
    if n >= 130:
        doc_of[126:130] = doc_of[126]
    n_groups = max(docs + 30, 100)
    col = g.permutation(n_groups)[doc_of].astype(np.int32)
    if n > 20:
        col[g.choice(n, n // 20, replace=False)] = -1
    return col, n_groups


def make_scopes(col, n_groups, B, seed):
    """S = B // 2 + 1 scopes shared by the B queries: one document, several documents, an empty scope, a document whose
    rows the caller kills (returned), ordinals no row has"""
    g = np.random.default_rng(seed)
    used = np.unique(col[col >= 0])
    S = B // 2 + 1
    scopes = []
    for s in range(S):
        kind = s % 4
        if kind == 0 or used.size == 0:
            scopes.append(sorted(g.choice(n_groups, 1).tolist()) if used.size == 0 else [int(g.choice(used))])
        elif kind == 1:
            scopes.append(sorted(set(g.choice(used, int(g.integers(2, 12))).tolist())))
        elif kind == 2:
            scopes.append(sorted(set(g.choice(n_groups, int(g.integers(1, 64))).tolist())))
        else:
            scopes.append([])
    dead_doc = int(used[0]) if used.size else 0
    if S > 1:
        scopes[1] = [dead_doc]
    soq = g.integers(0, S, B)
    soq[: min(B, S)] = np.arange(min(B, S))       # every scope is some query's
    return scopes, soq.astype(np.int32), dead_doc


def tables(soq, scopes):
    off = np.cumsum([0] + [len(s) for s in scopes]).astype(np.int32)
    flat = np.array([o for s in scopes for o in s], dtype=np.int32)
    return torch.from_numpy(np.asarray(soq, np.int32)), torch.from_numpy(off), torch.from_numpy(flat)


def run(N, qd, cd, n, d, k, col, n_groups, soq, scopes, max_candidates=None, **kw):
    s, r = N.scoped_topk(qd, cd, n, d, k, torch.from_numpy(col).to("cuda"), n_groups, *tables(soq, scopes),
                         n if max_candidates is None else max_candidates, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


# ---------------------------------------------------------------- 1. the C-ABI against the reference
# (n, B, d, dtype, k): every value of each grid at least once
PARITY = [
    (1, 1, 8, "f32", 1),
    (129, 3, 384, "f16", 5),
    (300, 128, 768, "bf16", 20),
    (1000, 129, 384, "f32", 21),
    (1000, 200, 768, "f16", 100),
    (300, 200, 8, "bf16", 5),
    (1000, 3, 768, "f32", 20),
    (129, 129, 8, "f16", 100),
]


@pytest.mark.parametrize("n,B,d,dt,k", PARITY)
def test_parity(N, n, B, d, dt, k):
    """one / several documents, scopes shared by queries (S < B), an empty scope, a scope whose rows are all dead,
    k larger than a scope, rows with ordinal -1, a document across a tile boundary, dead rows"""
    col, n_groups = documents(n, 7 * n + B)
    scopes, soq, dead_doc = make_scopes(col, n_groups, B, n + k)
    g = np.random.default_rng(n + B + k)
    alive = g.random(n) > 0.03
    if B > 1:
        alive[col == dead_doc] = False
    cd, cs = to_dev(N, unit_rows(n, d, 3 * n + d), DT[dt])
    qd, qs = to_dev(N, unit_rows(B, d, B + 11), DT[dt])
    s, r = run(N, qd, cd, n, d, k, col, n_groups, soq, scopes, alive_bits=bits_of(alive))
    es, er = R.scoped_topk(qs, cs, k, col, soq, scopes, alive)
    check(s, r, es, er)
    if B > 1:
        assert np.all(r[soq == 1] == -1)                  # the dead document's queries


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_integer_data_bit_exact_with_heavy_ties(N, dt):
    """values in {-2..2}/8 on 4 columns: every product and sum is exact in float32, so scores and rows (ties -> the
    lower row) equal the reference bit for bit"""
    n, B, d, k = 1000, 200, 384, 100
    g = np.random.default_rng(5)
    c = np.zeros((n, d), np.float32)
    c[:, :4] = g.integers(-2, 3, (n, 4)) / 8
    q = np.zeros((B, d), np.float32)
    q[:, :4] = g.integers(-2, 3, (B, 4)) / 8
    col, n_groups = documents(n, 17)
    scopes, soq, _ = make_scopes(col, n_groups, B, 19)
    cd, cs = to_dev(N, c, DT[dt])
    qd, qs = to_dev(N, q, DT[dt])
    s, r = run(N, qd, cd, n, d, k, col, n_groups, soq, scopes)
    es, er = R.scoped_topk(qs, cs, k, col, soq, scopes)
    assert np.array_equal(s, es) and np.array_equal(r, er)


def test_skipped_tiles_do_not_touch_the_kept_ones(N):
    """two documents 20 row tiles apart, every row between them in other documents: the answer equals the reference, and
    is bit-equal to the same queries' answer when a further query's scope makes the kernel read the tiles in between"""
    d, k, T = 384, 20, 22
    n = T * 128
    col = (2 + np.arange(n) // 50).astype(np.int32)       # 50-row documents 2, 3, ...
    col[:100] = 0
    col[21 * 128 + 10: 21 * 128 + 110] = 1
    between = sorted(set(col[128: 21 * 128].tolist()) - {0, 1})
    assert len(between) <= 64
    n_groups = int(col.max()) + 1
    cd, cs = to_dev(N, unit_rows(n, d, 31), torch.float16)
    qd, qs = to_dev(N, unit_rows(4, d, 32), torch.float16)
    scopes = [[0, 1], [1], between]
    s, r = run(N, qd[:3].contiguous(), cd, n, d, k, col, n_groups, [0, 1, 0], scopes[:2], max_candidates=200)
    es, er = R.scoped_topk(qs[:3], cs, k, col, [0, 1, 0], scopes)
    check(s, r, es, er)
    assert set(np.unique(r[0] // 128).tolist()) == {0, 21}     # both ends of the gap are in the answer
    s4, r4 = run(N, qd, cd, n, d, k, col, n_groups, [0, 1, 0, 2], scopes)
    assert np.array_equal(s4[:3], s) and np.array_equal(r4[:3], r)
    es4, er4 = R.scoped_topk(qs, cs, k, col, [0, 1, 0, 2], scopes)
    check(s4, r4, es4, er4)


def test_a_query_does_not_depend_on_its_batch(N):
    n, B, d, k = 1000, 200, 384, 20
    col, n_groups = documents(n, 41)
    scopes, soq, _ = make_scopes(col, n_groups, B, 43)
    cd, _ = to_dev(N, unit_rows(n, d, 44), torch.float16)
    qd, _ = to_dev(N, unit_rows(B, d, 45), torch.float16)
    s, r = run(N, qd, cd, n, d, k, col, n_groups, soq, scopes)
    for b in range(B):
        s1, r1 = run(N, qd[b: b + 1].contiguous(), cd, n, d, k, col, n_groups, [0], [scopes[soq[b]]])
        assert np.array_equal(s1[0], s[b]) and np.array_equal(r1[0], r[b]), b


def test_overflow_of_one_scope_in_a_batch(N):
    """256 candidate slots, a scope of 700 rows and max_candidates = n: its queries are produced again alone; the
    other queries of the batch are what they are without the small capacity"""
    n, d, k = 1000, 384, 21
    col = (1 + np.arange(n) // 20).astype(np.int32)
    col[150:850] = 0
    n_groups = int(col.max()) + 1
    scopes = [[0], [3], [2, 45, 46], []]
    soq = [1, 0, 2, 0, 3, 1]
    cd, cs = to_dev(N, unit_rows(n, d, 51), torch.bfloat16)
    qd, qs = to_dev(N, unit_rows(len(soq), d, 52), torch.bfloat16)
    s, r = run(N, qd, cd, n, d, k, col, n_groups, soq, scopes, cap=256)
    es, er = R.scoped_topk(qs, cs, k, col, soq, scopes)
    check(s, r, es, er)
    assert np.all((r[1] >= 150) & (r[1] < 850))
    s0, r0 = run(N, qd, cd, n, d, k, col, n_groups, soq, scopes)
    assert np.array_equal(s, s0) and np.array_equal(r, r0)


def test_alive_bits_and_row_offset(N):
    n, B, d, k = 300, 3, 8, 5
    col = (np.arange(n) // 30).astype(np.int32)
    scopes, soq = [[0, 9], [4]], [0, 1, 0]
    cd, cs = to_dev(N, unit_rows(n, d, 61), torch.float32)
    qd, qs = to_dev(N, unit_rows(B, d, 62), torch.float32)
    alive = np.ones(n, bool)
    alive[:29] = False
    alive[125:135] = False
    for a in (None, alive):
        s, r = run(N, qd, cd, n, d, k, col, 100, soq, scopes, row_offset=10 ** 10,
                   alive_bits=None if a is None else bits_of(a))
        es, er = R.scoped_topk(qs, cs, k, col, soq, scopes, a, row_offset=10 ** 10)
        check(s, r, es, er)
    assert r[0].min() >= 10 ** 10 + 29 and not np.any((r[1] >= 10 ** 10 + 125) & (r[1] < 10 ** 10 + 135))


def test_wrapper_checks_host_scope_tables(N):
    cd, _ = to_dev(N, unit_rows(10, 8, 1), torch.float16)
    qd, _ = to_dev(N, unit_rows(2, 8, 2), torch.float16)
    col = torch.zeros(10, dtype=torch.int32, device="cuda")
    for soq, scopes in (([0, 1], [[0]]), ([0, 0], [list(range(65))]), ([0, 0], [[3, 2]]), ([0, 0], [[100]])):
        with pytest.raises(N.MMRagNativeError):
            N.scoped_topk(qd, cd, 10, 8, 3, col, 100, *tables(soq, scopes), 10)


# ---------------------------------------------------------------- 2. VectorIndex
def doc_names(n, seed, longest=40):
    g = np.random.default_rng(seed)
    names, at, docs = [], 0, 0
    while at < n:
        m = int(g.integers(1, longest + 1))
        names += [f"doc{docs}"] * min(m, n - at)
        at, docs = at + m, docs + 1
    return names


def build_index(rows, names, dtype=torch.float16, first=0, idx=None, **kw):
    from multimodal_rag_amd.index import VectorIndex

    n, d = rows.shape
    if idx is None:
        idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=256, **kw)
    metas = [{"doc_id": names[i], "parity": i % 2} for i in range(n)]
    idx.add(rows, documents=[f"text {first + i}" for i in range(n)], metadatas=metas,
            ids=[f"id{first + i}" for i in range(n)])
    return idx


def assert_equals_where(idx, q, k, scopes, where=None):
    """scoped_query against query(where={"doc_id": ...}) per query, under the bar"""
    res = idx.scoped_query(q, n_results=k, scopes=scopes, where=where)
    assert len(res["ids"]) == len(q)
    for b, entry in enumerate(scopes):
        only = {"doc_id": {"$in": list(entry)}} if isinstance(entry, (list, tuple)) else {"doc_id": entry}
        want = idx.query(q[b: b + 1], n_results=k, where={"$and": [where, only]} if where else only)
        m = len(want["ids"][0])
        assert len(res["ids"][b]) == m
        row = lambda ids: np.array([[int(i[2:]) for i in ids] + [-1] * (k - m)])          # noqa: E731
        score = lambda ds: np.array([[1.0 - x for x in ds] + [-np.inf] * (k - m)], np.float32)   # noqa: E731
        check(score(res["distances"][b]), row(res["ids"][b]), score(want["distances"][0]), row(want["ids"][0]))
        assert all(meta["doc_id"] in (entry if isinstance(entry, (list, tuple)) else [entry])
                   for meta in res["metadatas"][b])
    return res


def test_index_scoped_query_through_add_delete_compact(N):
    d, n, k = 384, 1500, 8
    rows, names = unit_rows(n, d, 71), doc_names(n, 72)
    idx = build_index(rows, names)
    docs = sorted(set(names))
    g = np.random.default_rng(73)
    q = unit_rows(12, d, 74)
    scopes = [docs[int(i)] for i in g.integers(0, len(docs), 8)] + [[docs[0], docs[5], "nowhere"], "nowhere", [],
                                                                    (docs[3], docs[4])]
    assert_equals_where(idx, q, k, scopes)
    assert_equals_where(idx, q, k, scopes, where={"parity": 1})
    more, more_names = unit_rows(400, d, 75), [f"new{i // 25}" for i in range(400)]
    build_index(more, more_names, first=n, idx=idx)               # grows the matrix and the column
    scopes[0], scopes[1] = "new3", ["new0", docs[1]]
    assert_equals_where(idx, q, k, scopes)
    gone = scopes[5]
    idx.delete(where={"doc_id": gone})
    res = assert_equals_where(idx, q, k, scopes)
    assert res["ids"][5] == []
    st = idx.enable_grouping("doc_id")
    assert st["counts"][st["ordinal"][gone]] > 0                  # dead rows still counted: an upper bound
    idx.compact()
    assert st["counts"][st["ordinal"][gone]] == 0
    assert sum(st["counts"]) == idx.count()
    assert_equals_where(idx, q, k, scopes)


def test_index_f8_collection_runs_on_its_plane(N):
    d, n, k = 384, 800, 6
    rows, names = unit_rows(n, d, 81), doc_names(n, 82)
    q = unit_rows(5, d, 83)
    scopes = ["doc1", ["doc2", "doc3"], "doc7", "none", "doc0"]
    half = build_index(rows, names, torch.float16)
    f8 = build_index(rows, names, torch.float8_e4m3fn, rescore_dtype=torch.float16)
    a, b = half.scoped_query(q, k, scopes), f8.scoped_query(q, k, scopes)
    assert a["ids"] == b["ids"] and a["distances"] == b["distances"]
    lean = build_index(rows, names, torch.float8_e4m3fn, rescore_dtype=None)
    with pytest.raises(ValueError, match="MMRAG_F8_RESCORE=none"):
        lean.scoped_query(q, k, scopes)


def test_index_wide_and_large_scopes_take_the_where_path(N, monkeypatch):
    from multimodal_rag_amd import index as index_mod

    d, n, k = 64, 18000, 5
    names = ["big"] * 17000 + [f"doc{i // 10}" for i in range(1000)]     # "big": more rows than 16384 candidate slots
    idx = build_index(unit_rows(n, d, 91), names)
    q = unit_rows(4, d, 92)
    wide = [f"doc{i}" for i in range(70)]                                # more than MAX_SCOPE_GROUPS values
    scopes = ["doc3", wide, "big", ["doc4", "doc5"]]
    calls = {"scoped": 0, "plain": 0}
    real_scoped, real_plain = N.scoped_topk, N.cosine_topk

    def scoped(qd, *a, **kw):
        calls["scoped"] += 1
        assert qd.shape[0] == 2                                          # queries 0 and 3 only
        return real_scoped(qd, *a, **kw)

    def plain(*a, **kw):
        calls["plain"] += 1
        return real_plain(*a, **kw)

    monkeypatch.setattr(index_mod._native, "scoped_topk", scoped)
    monkeypatch.setattr(index_mod._native, "cosine_topk", plain)
    res = idx.scoped_query(q, k, scopes)
    assert calls == {"scoped": 1, "plain": 2}
    monkeypatch.undo()
    again = assert_equals_where(idx, q, k, scopes)
    assert again["ids"] == res["ids"] and again["distances"] == res["distances"]
    for b in (1, 2):                                                      # the same path: the same bits
        only = {"doc_id": {"$in": scopes[b]}} if isinstance(scopes[b], list) else {"doc_id": scopes[b]}
        want = idx.query(q[b: b + 1], n_results=k, where=only)
        assert res["ids"][b] == want["ids"][0] and res["distances"][b] == want["distances"][0]


def test_index_one_kernel_call_for_fifty_scopes(N, monkeypatch):
    from multimodal_rag_amd import index as index_mod

    d, n, k = 128, 2000, 4
    names = doc_names(n, 95, longest=30)
    idx = build_index(unit_rows(n, d, 96), names)
    docs = sorted(set(names))
    assert len(docs) >= 50
    scopes = docs[:50]
    q = unit_rows(50, d, 97)
    idx.scoped_search(q[:1], k, scopes[:1])          # builds the group column
    calls = {"scoped": 0, "plain": 0}
    real = N.scoped_topk
    monkeypatch.setattr(index_mod._native, "scoped_topk",
                        lambda *a, **kw: (calls.__setitem__("scoped", calls["scoped"] + 1), real(*a, **kw))[1])
    monkeypatch.setattr(index_mod._native, "cosine_topk",
                        lambda *a, **kw: calls.__setitem__("plain", calls["plain"] + 1))
    s, r = idx.scoped_search(q, k, scopes)
    assert calls == {"scoped": 1, "plain": 0}
    monkeypatch.undo()
    r = r.cpu().numpy()
    for b in range(50):
        assert all(names[i] == scopes[b] for i in r[b] if i >= 0) and (r[b] >= 0).sum() == min(k, names.count(scopes[b]))


# ---------------------------------------------------------------- 3. manager and dispatcher on the HIP engine
def test_manager_and_dispatcher_keep_each_caller_in_its_document(N):
    from multimodal_rag_amd.embedder import EmbeddingManager

    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_scoped()
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình"]
    g = np.random.default_rng(99)
    docs = [f"doc{i}" for i in range(16)]
    for doc in docs:
        items = [{"id": f"{doc}_{i}", "type": "text", "summary": " ".join(g.choice(words, int(g.integers(3, 9))))}
                 for i in range(int(g.integers(3, 12)))]
        asyncio.run(m.embed_and_store(items, doc))
    texts = [f"{words[i % 12]} {words[(i * 5 + 1) % 12]}" for i in range(16)]
    solo = asyncio.run(m.scoped_query(texts[3], [docs[3], docs[4]], n_results=4))
    assert solo["ids"] and {meta["doc_id"] for meta in solo["metadatas"]} <= {docs[3], docs[4]}
    many = asyncio.run(m.batch_scoped_query(texts, [[doc] for doc in docs], n_results=4))
    assert asyncio.run(m.scoped_query(texts[0], ["nowhere"]))["ids"] == []

    async def go():
        disp = m.enable_dynamic_batching(max_batch=64, max_wait_ms=50.0)
        try:
            out = await asyncio.gather(*[m.scoped_query(t, [doc], n_results=4) for t, doc in zip(texts, docs)])
            stats = dict(disp.stats)
        finally:
            await disp.stop()
            m._dispatcher = None
        return out, stats

    out, stats = asyncio.run(go())
    assert stats["max_batch_seen"] > 1, stats
    for res, alone, doc in zip(out, many, docs):
        assert "error" not in res and res["ids"]
        assert all(meta["doc_id"] == doc for meta in res["metadatas"])
        assert res["ids"] == alone["ids"] and res["distances"] == alone["distances"]
    asyncio.run(m.cleanup())


def test_query_endpoint_doc_ids(N):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    with TestClient(create_app()) as c:
        bodies = [" ".join(f"Học máy là gì, phần {i}." for i in range(60)), "GPU kernel và dữ liệu. " * 3,
                  "Machine learning cơ bản, học máy. " * 3, "Bảng và ảnh. " * 3]
        uploaded = []
        for i, body in enumerate(bodies):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
            uploaded.append(r.json()["doc_id"])
        plain = c.post("/query", json={"query": "học máy", "top_k": 3})
        assert plain.status_code == 200, plain.text
        for asked in ([uploaded[1]], [uploaded[3], uploaded[2]]):
            for extra in ({}, {"hybrid": True}, {"mmr": True}, {"group_by_document": True}, {"variants": ["máy học"]}):
                r = c.post("/query", json={"query": "học máy", "top_k": 3, "doc_ids": asked, **extra})
                assert r.status_code == 200, r.text
                src = r.json()["sources"]
                assert src and all(s["doc_id"].startswith(tuple(asked)) for s in src), (asked, extra)
        scoped = c.post("/query", json={"query": "học máy", "top_k": 3, "doc_ids": uploaded}).json()["sources"]
        assert [s["doc_id"] for s in scoped] == [s["doc_id"] for s in plain.json()["sources"]]
        assert set(scoped[0]) == set(plain.json()["sources"][0])
        r = c.post("/query", json={"query": "học máy", "doc_ids": ["doc_unknown"]})
        assert r.status_code == 200 and r.json()["sources"] == []
        assert c.post("/query", json={"query": "học máy", "doc_ids": []}).status_code == 422
