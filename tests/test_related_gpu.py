"""GPU: related-document retrieval (csrc/related.hip through _native.related_groups, VectorIndex.related_search /
related_query, EmbeddingManager and the routes) against tests/related_ref.py.

Bit-equal wherever the data is exactly representable (small integers: every dot is exact in float32, the similarity is
one float64 division rounded once) and wherever two runs of the kernel are compared; on real unit rows the project's
bar: scores within 1e-4 of the reference, candidates within 2e-4 of the k-th similarity interchangeable."""
import numpy as np
import pytest
import torch

from tests import related_ref as R

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


def int_rows(n, d, seed):
    return np.random.default_rng(seed).integers(-2, 3, (n, d)).astype(np.float32)


def to_dev(N, x, dtype, spare=0):
    """(device [max(n, 1) + spare, ld] with zero pad columns, the stored values as float32 on the host)"""
    n, d = x.shape
    ld = N.padded_dim(d, dtype)
    t = torch.zeros((max(n, 1) + spare, ld), dtype=dtype, device="cuda")
    if n:
        t[:n, :d] = torch.from_numpy(x).to("cuda").to(dtype)
    return t, t[:n, :d].to(torch.float32).cpu().numpy()


def bits_of(alive):
    words = np.zeros((alive.size + 31) // 32 + 8, dtype=np.uint32)
    idx = np.nonzero(alive)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32)).to("cuda")


def documents(n, seed):
    """group_of_row [n] int32 and the number of ordinals: contiguous documents of 1 .. max(1, min(60, n // 10)) rows,
    one of 200 rows over rows 400 .. 599 (longer than a tile) when n >= 1000, one across the rows 126 .. 129 (a tile
    edge), two interleaved over rows 10 .. 39 (runs of length 1), ordinals a random permutation of 0 .. n_groups-1 with
    n_groups >= 100 (ordinals above 63), about 5 % of the rows -1"""
    g = np.random.default_rng(seed)
    longest = max(1, min(60, n // 10))
    doc_of, at, docs = np.zeros(n, np.int64), 0, 0
    while at < n:
        m = int(g.integers(1, longest + 1))
        doc_of[at:at + m] = docs
        at, docs = at + m, docs + 1
    if n >= 1000:
        doc_of[400:600] = doc_of[400]
    if n >= 130:
        doc_of[126:130] = doc_of[126]
    if n >= 40:
        doc_of[10:40:2], doc_of[11:40:2] = docs, docs + 1
        docs += 2
    n_groups = max(docs + 30, 100)
    col = g.permutation(n_groups)[doc_of].astype(np.int32)
    if n > 20:
        col[g.choice(n, n // 20, replace=False)] = -1
    return col, n_groups


def liveness(n, col, seed):
    """about 3 % dead rows, one whole dead document, and a whole dead 128-row tile (rows 256 .. 383) when n >= 1000"""
    alive = np.random.default_rng(seed).random(n) > 0.03
    if n >= 130:
        alive[col == col[126]] = False
    if n >= 1000:
        alive[256:384] = False
    return alive


def offsets(M, S):
    """S sets over M columns; with S = 3 the middle one is empty"""
    return [0, M] if S == 1 else [0, (M + 1) // 2, (M + 1) // 2, M]


def run(N, sd, off, cd, n, d, k, col, n_groups, thr, excl=None, alive=None, **kw):
    out = N.related_groups(sd, off, cd, n, d, k, torch.from_numpy(col).to("cuda"), n_groups, thr, exclude=excl,
                           alive_bits=None if alive is None else bits_of(alive), **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def assert_bit_equal(got, want):
    for name, a, b in zip(("similarity", "group", "covered", "best", "best_row"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(a.view(np.int32 if a.itemsize == 4 else np.int64),
                              b.view(np.int32 if b.itemsize == 4 else np.int64)), name


# ---------------------------------------------------------------- 1. bit-equality on integer data
# (n, M, S, d, dtype, k): every value of each grid of the issue at least once; d = 100 is padded to whole slabs
EXACT = [
    (1, 1, 1, 128, "f32", 1),
    (127, 5, 3, 100, "f16", 5),
    (129, 128, 1, 128, "bf16", 150),
    (300, 129, 3, 100, "f32", 5),
    (1000, 300, 3, 128, "f16", 150),
    (1000, 5, 1, 100, "bf16", 5),
    (300, 1, 1, 128, "f16", 150),
]


@pytest.mark.parametrize("n,M,S,d,dt,k", EXACT)
def test_integer_data_bit_exact(N, n, M, S, d, dt, k):
    """documents across a tile edge, longer than a tile, interleaved, rows of no document, dead rows / document / tile,
    ordinals above 63, an empty set in the middle, k beyond the candidate groups, an excluded group and -1"""
    col, n_groups = documents(n, 7 * n + M)
    alive = liveness(n, col, n + k) if n > 1 else None
    cd, cs = to_dev(N, int_rows(n, d, 3 * n + d), DT[dt])
    sd, ss = to_dev(N, int_rows(M, d, M + 11), DT[dt])
    off = offsets(M, S)
    used = np.unique(col[col >= 0])
    excl = [int(used[0]) if s == 0 and used.size > 1 else -1 for s in range(S)]
    got = run(N, sd, off, cd, n, d, k, col, n_groups, 3.0, excl, alive)
    want, _ = R.related_groups(ss, off, cs, col, n_groups, k, 3.0, excl, alive)
    assert_bit_equal(got, want)
    assert got[1][0, 0] >= 0 and (k < 100 or got[1][0, -1] == -1)                  # something found; padded
    if used.size > 1:
        assert excl[0] not in got[1][0]
    if S == 3:
        assert np.all(got[1][1] == -1) and np.all(np.isneginf(got[0][1])) and np.all(got[2][1] == 0)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_constructed_ties(N, dt):
    """two rows of one document with the same dot -> the lower row; two documents with the same similarity -> the
    lower ordinal: document 7 is a copy of document 3's rows in another order, and row 131 repeats row 127"""
    n, d, M, k = 300, 128, 6, 30
    rows = int_rows(n, d, 5)
    col = (np.arange(n) // 10).astype(np.int32)
    rows[70:80] = rows[30:40][::-1]
    rows[131] = rows[127]
    col[120:135] = 12                                   # rows 127 and 131 in one document, across the tile edge
    sets = int_rows(M, d, 6)
    sets[0] = rows[127]
    cd, cs = to_dev(N, rows, DT[dt])
    sd, ss = to_dev(N, sets, DT[dt])
    got = run(N, sd, [0, 3, 6], cd, n, d, k, col, 30, 1.0)
    want, (all_sim, _) = R.related_groups(ss, [0, 3, 6], cs, col, 30, k, 1.0)
    assert_bit_equal(got, want)
    assert np.array_equal(all_sim[:, 3], all_sim[:, 7])
    for s in range(2):
        at = got[1][s].tolist()
        assert at.index(3) < at.index(7) and got[0][s, at.index(3)] == got[0][s, at.index(7)]
    j = got[1][0].tolist().index(12)
    assert got[4][0, j] == 127 and got[3][0, j] == float(rows[127] @ rows[127])


# ---------------------------------------------------------------- 2. real-valued unit rows under the project's bar
@pytest.mark.parametrize("d,dt", [(384, "f16"), (768, "bf16"), (384, "f32")])
def test_unit_rows_within_tolerance(N, d, dt):
    n, M, k = 3000, 140, 10
    col, n_groups = documents(n, 31)
    alive = liveness(n, col, 32)
    rows, sets = unit_rows(n, d, 33 + d), unit_rows(M, d, 34)
    # a planted document of 40 rows: five of set 0's vectors are five of its rows, so some columns ARE covered
    planted, n_groups = n_groups, n_groups + 1
    col[1500:1540], alive[1500:1540], sets[:5] = planted, True, rows[1500:1505]
    cd, cs = to_dev(N, rows, DT[dt])
    sd, ss = to_dev(N, sets, DT[dt])
    off = [0, 60, 60, 140]
    _, (_, best_all) = R.related_groups(ss, off, cs, col, n_groups, k, 0.5, alive=alive)
    # a threshold no reference best is within 1e-4 of: the middle of the widest gap in the upper tail of the bests
    # (around the median they lie closer together than the bar)
    v = np.sort(best_all[np.isfinite(best_all)].astype(np.float64))
    mid = v[-120:-10]
    at = int(np.argmax(np.diff(mid)))
    thr = float(np.float32((mid[at] + mid[at + 1]) / 2))
    assert np.min(np.abs(best_all[np.isfinite(best_all)] - np.float32(thr))) > TOL
    (esim, egrp, ecov, _, _), (all_sim, best_all) = R.related_groups(ss, off, cs, col, n_groups, k, thr, alive=alive)
    sim, grp, cov, best, row = run(N, sd, off, cd, n, d, k, col, n_groups, thr, alive=alive)
    dots = ss.astype(np.float64) @ cs.astype(np.float64).T
    for s in range(3):
        lo, hi = off[s], off[s + 1]
        if hi == lo:
            assert np.all(grp[s] == -1)
            continue
        assert np.all(grp[s] >= 0) and len(set(grp[s].tolist())) == k and np.all(np.diff(sim[s]) <= 0)
        assert np.all(np.abs(sim[s] - all_sim[s, grp[s]]) <= TOL)
        kth = esim[s, k - 1]
        assert set(np.nonzero(all_sim[s] > kth + 2 * TOL)[0].tolist()) <= set(grp[s].tolist())
        assert np.all(all_sim[s, grp[s]] >= kth - 2 * TOL)
        for j, g in enumerate(grp[s].tolist()):
            assert np.all(np.abs(best[lo:hi, j] - best_all[lo:hi, g]) <= TOL)
            r = row[lo:hi, j]
            assert np.all(col[r] == g) and np.all(alive[r])
            assert np.all(np.abs(dots[np.arange(lo, hi), r] - best[lo:hi, j]) <= TOL)
            assert cov[s, j] == int(np.sum(best_all[lo:hi, g] >= np.float32(thr)))
    assert grp[0, 0] == planted and 5 <= cov[0, 0] < 60          # the threshold separates: covered and not


# ---------------------------------------------------------------- 3. reproducibility
def test_reproducible_across_calls_batches_and_grids(N):
    n, d, k = 1000, 384, 20
    col, n_groups = documents(n, 41)
    alive = liveness(n, col, 42)
    cd, _ = to_dev(N, unit_rows(n, d, 43), torch.float16, spare=700)
    sd, _ = to_dev(N, unit_rows(300, d, 44), torch.float16)
    off = [0, 100, 229, 300]
    a = run(N, sd, off, cd, n, d, k, col, n_groups, 0.1, [-1, 5, -1], alive)
    assert_bit_equal(run(N, sd, off, cd, n, d, k, col, n_groups, 0.1, [-1, 5, -1], alive), a)
    for grid in (1, 3, 1000):
        assert_bit_equal(run(N, sd, off, cd, n, d, k, col, n_groups, 0.1, [-1, 5, -1], alive, grid=grid), a)
    # set 1 alone
    alone = run(N, sd[100:229].contiguous(), [0, 129], cd, n, d, k, col, n_groups, 0.1, [5], alive)
    assert_bit_equal(alone, (a[0][1:2], a[1][1:2], a[2][1:2], a[3][100:229], a[4][100:229]))
    # the same rows inside a larger buffer: 700 further rows of another document behind them, all dead
    g = np.random.default_rng(45)
    cd[n:, :d] = torch.from_numpy(unit_rows(700, d, 46)).to("cuda").to(torch.float16)
    col2 = np.concatenate([col, g.integers(0, n_groups, 700).astype(np.int32)])
    alive2 = np.concatenate([alive, np.zeros(700, bool)])
    assert_bit_equal(run(N, sd, off, cd, n + 700, d, k, col2, n_groups, 0.1, [-1, 5, -1], alive2), a)


# ---------------------------------------------------------------- 4. cross-checks against existing code
def test_best_equals_scoped_topk_bit_for_bit(N):
    n, d, k, M = 1000, 384, 3, 130
    col, n_groups = documents(n, 51)
    alive = liveness(n, col, 52)
    cd, _ = to_dev(N, unit_rows(n, d, 53), torch.bfloat16)
    sd, _ = to_dev(N, unit_rows(M, d, 54), torch.bfloat16)
    sim, grp, cov, best, row = run(N, sd, [0, 70, 130], cd, n, d, k, col, n_groups, 0.1, alive=alive)
    for j in range(k):
        scopes = [[int(grp[0, j])], [int(grp[1, j])]]
        s, r = N.scoped_topk(sd, cd, n, d, 1, torch.from_numpy(col).to("cuda"), n_groups, [0] * 70 + [1] * 60,
                             [0, 1, 2], [scopes[0][0], scopes[1][0]], n, alive_bits=bits_of(alive))
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy()[:, 0].view(np.int32), best[:, j].view(np.int32))
        assert np.array_equal(r.cpu().numpy()[:, 0], row[:, j])


def build_index(rows, names, dtype=torch.float16, **kw):
    from multimodal_rag_amd.index import VectorIndex

    n, d = rows.shape
    idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=256, **kw)
    idx.add(rows, documents=[f"text {i}" for i in range(n)],
            metadatas=[{"doc_id": names[i], "parity": i % 2} for i in range(n)], ids=[f"id{i}" for i in range(n)])
    return idx


def test_one_vector_equals_grouped_search(N):
    """M = 1: a document's similarity is its best row's score, so the winners are grouped_search's groups.  The search
    kernel accumulates in another K order than the pair-tile body, so the scores agree within 1e-4, not bit for bit,
    and documents within 2e-4 of each other may swap"""
    n, d, k = 2000, 384, 10
    names = [f"doc{i // 50}" for i in range(n)]
    idx = build_index(unit_rows(n, d, 61), names)
    q = unit_rows(1, d, 62)
    sim, grp, _, best, row = (t.cpu().numpy() for t in idx.related_search([q], k))
    gs, gr, _, gg, _, _ = idx.grouped_search(q, n_groups=k, group_size=1, fetch_k=4096)
    gs, gr, gg = gs.cpu().numpy()[0, :, 0], gr.cpu().numpy()[0, :, 0], gg.cpu().numpy()[0]
    assert np.all(np.abs(sim[0] - gs) <= TOL) and np.array_equal(sim[0], best[0])
    for j in range(k):
        if grp[0, j] != gg[j]:
            assert abs(gs[j] - sim[0, j]) <= 2 * TOL and grp[0, j] in gg
        else:
            assert row[0, j] == gr[j]


# ---------------------------------------------------------------- 5. the table split
def test_table_split_is_exact(N, monkeypatch):
    from multimodal_rag_amd import config

    n, d, k = 1000, 128, 7
    col, n_groups = documents(n, 71)
    cd, _ = to_dev(N, unit_rows(n, d, 72), torch.float16)
    sd, _ = to_dev(N, unit_rows(90, d, 73), torch.float16)
    off = [0, 30, 30, 70, 90]
    excl = [-1, -1, int(col[500]), -1]
    whole = run(N, sd, off, cd, n, d, k, col, n_groups, 0.1, excl)
    calls = []
    real = N.lib().mmrag_internal_related_groups_ex
    monkeypatch.setattr(N.lib(), "mmrag_internal_related_groups_ex", lambda *a: (calls.append(a[3]), real(*a))[1])
    monkeypatch.setattr(config.settings, "MMRAG_RELATED_TABLE_BYTES", 8 * n_groups * 45)
    split = run(N, sd, off, cd, n, d, k, col, n_groups, 0.1, excl)
    assert calls == [2, 1, 1]                       # whole sets: {0, the empty one}, {2}, {3}
    assert_bit_equal(split, whole)
    calls.clear()
    assert_bit_equal(run(N, sd, off, cd, n, d, k, col, n_groups, 0.1, excl, table_bytes=8 * n_groups * 70), whole)
    assert calls == [3, 1]
    with pytest.raises(ValueError, match="MMRAG_RELATED_TABLE_BYTES"):
        run(N, sd, off, cd, n, d, k, col, n_groups, 0.1, excl, table_bytes=8 * n_groups * 39)
    for bad_off in ([0, 30, 20, 90], [0, 89], [1, 90]):
        with pytest.raises(ValueError, match="set_off"):
            run(N, sd, bad_off, cd, n, d, k, col, n_groups, 0.1)


# ---------------------------------------------------------------- 6. VectorIndex
def half_rows(n, d, seed):
    """unit rows whose dots are exact: four entries of +-0.5"""
    g = np.random.default_rng(seed)
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        x[i, g.choice(d, 4, replace=False)] = g.choice([-0.5, 0.5], 4)
    return x


@pytest.mark.parametrize("exact", [True, False])
def test_index_finds_a_planted_copy_through_where_delete_compact(N, exact):
    d, n = 384, 1400
    rows = half_rows(n, d, 81) if exact else unit_rows(n, d, 81)
    names = [f"doc{i // 35}" for i in range(n)]
    perm = np.random.default_rng(82).permutation(35)
    rows[700:735] = rows[70:105][perm]                      # doc20 = doc2's rows in another order
    idx = build_index(rows, names)
    (found,) = idx.related_query([{"value": "doc2"}], n_results=5, threshold=0.98)
    assert [f["key"] for f in found][0] == "doc20" and "doc2" not in [f["key"] for f in found]
    top = found[0]
    assert top["coverage"] == 1.0 and top["matched"] == 35 and top["rows_in_group"] == 35
    assert top["similarity"] == 1.0 if exact else abs(top["similarity"] - 1.0) <= TOL
    assert [p["item"] for p in top["pairs"]] == [f"id{i}" for i in range(70, 105)]
    assert [p["match_id"] for p in top["pairs"]] == [f"id{700 + int(np.nonzero(perm == i)[0][0])}" for i in range(35)]
    assert found[1]["similarity"] < 0.9 and found[1]["coverage"] < 1.0
    # exclude=[None]: the document is a candidate of its own rows, and wins
    (own,) = idx.related_query([{"value": "doc2"}], n_results=2, threshold=0.98, exclude=[None])
    assert [f["key"] for f in own] == ["doc2", "doc20"]
    # the same rows given as vectors: no exclusion, items are indices
    (vec,) = idx.related_query([rows[70:105]], n_results=2, threshold=0.98)
    assert [f["key"] for f in vec] == ["doc2", "doc20"] and [p["item"] for p in vec[0]["pairs"]] == list(range(35))
    # `where` removes a document from the answer
    (odd,) = idx.related_query([{"value": "doc2"}], n_results=5, threshold=0.98, where={"doc_id": {"$ne": "doc20"}})
    assert "doc20" not in [f["key"] for f in odd] and [f["key"] for f in odd][:4] == [f["key"] for f in found[1:]]
    with pytest.raises(ValueError, match="no stored row"):
        idx.related_search([{"value": "nowhere"}], 3)
    with pytest.raises(ValueError, match="threshold"):
        idx.related_search([{"value": "doc2"}], 3, threshold=1.5)
    idx.delete(where={"doc_id": "doc20"})
    (after,) = idx.related_query([{"value": "doc2"}], n_results=4, threshold=0.98)
    assert [f["key"] for f in after] == [f["key"] for f in found[1:]]
    idx.compact()
    (packed,) = idx.related_query([{"value": "doc2"}], n_results=4, threshold=0.98)
    assert [(f["key"], f["similarity"], f["matched"]) for f in packed] == \
           [(f["key"], f["similarity"], f["matched"]) for f in after]
    assert [[p["match_id"] for p in f["pairs"]] for f in packed] == [[p["match_id"] for p in f["pairs"]] for f in after]


def test_index_f8_collection_runs_on_its_plane(N):
    d, n = 384, 800
    rows, names = unit_rows(n, d, 91), [f"doc{i // 40}" for i in range(n)]
    sets = [{"value": "doc3"}, unit_rows(7, d, 92)]
    half = build_index(rows, names, torch.float16)
    f8 = build_index(rows, names, torch.float8_e4m3fn, rescore_dtype=torch.float16)
    a, b = half.related_search(sets, 6, threshold=0.2), f8.related_search(sets, 6, threshold=0.2)
    assert_bit_equal(tuple(t.cpu().numpy() for t in b), tuple(t.cpu().numpy() for t in a))
    lean = build_index(rows, names, torch.float8_e4m3fn, rescore_dtype=None)
    with pytest.raises(ValueError, match="MMRAG_F8_RESCORE=none"):
        lean.related_search(sets, 6)


# ---------------------------------------------------------------- 7. end to end
def test_related_route_end_to_end(N):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    topics = ["kernel", "bảng", "ảnh", "văn bản", "mô hình", "dữ liệu", "bộ nhớ", "mạng", "đồ thị", "chỉ mục"]
    common = " ".join(f"Câu số {i} nói về {topics[i % 10]} và {topics[(i * 3 + 1) % 10]} trong phần {i // 7}."
                      for i in range(110))
    tail_a = " ".join(f"Phần kết A, ý {i}: học máy trên GPU." for i in range(20))
    tail_b = " ".join(f"Ghi chú B thứ {i}: một bản sửa đổi khác của tài liệu." for i in range(40))
    other = " ".join(f"Công thức nấu ăn {i}: {topics[(i * 7) % 10]} không liên quan, thêm muối và đường." for i in range(120))
    with TestClient(create_app()) as c:
        ids = []
        for name, body in (("a.txt", common + " " + tail_a), ("b.txt", common + " " + tail_b), ("c.txt", other)):
            r = c.post("/upload", files={"file": (name, body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
            ids.append(r.json()["doc_id"])
        before = c.post("/query", json={"query": "học máy trên GPU", "top_k": 3})
        assert before.status_code == 200, before.text
        r = c.get(f"/documents/{ids[0]}/related", params={"top_k": 5})
        assert r.status_code == 200, r.text
        body = r.json()
        assert body["doc_id"] == ids[0] and body["chunks"] >= 4
        assert [d["key"] for d in body["related"]] == [ids[1], ids[2]]
        sharer, third = body["related"]
        assert sharer["coverage"] > third["coverage"] and sharer["coverage"] >= 0.5
        assert sharer["similarity"] > third["similarity"] and sharer["matched"] == round(sharer["coverage"] * body["chunks"])
        assert 1 <= len(sharer["pairs"]) <= 5 and all(p["match_id"].startswith(ids[1]) for p in sharer["pairs"])
        r = c.post("/related", json={"texts": [common[:600]], "top_k": 2, "threshold": 0.5})
        assert r.status_code == 200, r.text
        assert {d["key"] for d in r.json()["related"]} == {ids[0], ids[1]}
        assert c.get("/documents/doc_unknown/related").status_code == 404
        after = c.post("/query", json={"query": "học máy trên GPU", "top_k": 3})
        assert after.json()["sources"] == before.json()["sources"]
