"""GPU: filtered retrieval (csrc/filtered.hip through _native.filter_eval / filtered_topk, VectorIndex.filtered_search /
filtered_query, MMRAG_DEVICE_FILTERS, EmbeddingManager and the dispatcher) against tests/filter_ref.py.

The bar is tests/test_scoped_gpu.py's: scores within 1e-4 of the reference, identical id sets with candidates within
2e-4 of the k-th score interchangeable; bit-equal where two runs of the kernels are compared (a bitmap is a pure function
of its inputs; a score's bits depend on the query row, the stored row and d alone)."""
import asyncio

import numpy as np
import pytest
import torch

from multimodal_rag_amd import filters as F
from oracle import search_oracle as O
from tests import filter_ref as R

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


def alive_words(alive):
    words = np.zeros((alive.size + 31) // 32 + 8, dtype=np.uint32)
    idx = np.nonzero(alive)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32)).to("cuda")


def bitmaps(N, vis, n):
    """bool [F, n] -> device int32 [F, filter_words(n)]"""
    W = N.filter_words(n)
    words = np.stack([F.pack_bits(v, W) for v in vis]) if len(vis) else np.zeros((0, W), np.uint32)
    return torch.from_numpy(words.view(np.int32)).to("cuda").contiguous()


def check(s, r, es, er):
    assert r.shape == er.shape and s.shape == es.shape
    fin = np.isfinite(es)
    assert np.array_equal(np.isfinite(s), fin)
    assert np.array_equal(r[~fin], er[~fin])  # -1 padding
    assert np.all(np.abs(s[fin] - es[fin]) <= TOL)
    assert np.all(np.diff(s, axis=1)[fin[:, 1:]] <= 0)  # descending
    assert O.same_topk_sets(r, s, er, es)


def run(N, qd, cd, n, d, k, foq, vis_dev, **kw):
    out = N.filtered_topk(qd, cd, n, d, k, foq, vis_dev, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


# ---------------------------------------------------------------- 1. filter_eval is bit-exact
def eval_table(n, seed):
    """16 keys c0 .. c15 over n rows (even: numbers, odd: strings; about a fifth of the values missing) and 40 seeded
    filters over them, the first 5 on c0 alone"""
    g = np.random.default_rng(seed)
    metas = []
    for i in range(n):
        m = {}
        for c in range(16):
            if i > 0 and g.random() < 0.2:       # row 0 holds every key: each column has its kind at any n
                continue
            m[f"c{c}"] = f"s{int(g.integers(0, 5))}" if c % 2 else [int(g.integers(-3, 4)), float(g.integers(-6, 7)) / 2,
                                                                     bool(g.integers(0, 2))][c % 3]
        metas.append(m)
    number_ops = ["$eq", "$ne", "$gt", "$gte", "$lt", "$lte"]

    def leaf(c):
        key = f"c{c}"
        if c % 2:
            op = ["$eq", "$ne", "$in", "$nin"][int(g.integers(0, 4))]
            vals = [f"s{int(v)}" for v in g.integers(0, 7, int(g.integers(1, 5)))]
        else:
            op = (number_ops + ["$in", "$nin"])[int(g.integers(0, 8))]
            vals = [float(v) / 2 for v in g.integers(-7, 8, int(g.integers(1, 5)))]
        return {key: {op: vals if op in ("$in", "$nin") else vals[0]}}

    wheres = [leaf(0) for _ in range(4)] + [{"$or": [leaf(0), {"$and": [leaf(0), leaf(0)]}]}]
    while len(wheres) < 40:
        cols = g.integers(0, 16, int(g.integers(1, 7)))
        parts = [leaf(int(c)) for c in cols]
        wheres.append(parts[0] if len(parts) == 1 else
                      {["$and", "$or"][int(g.integers(0, 2))]: parts[:2] + ([{"$or": parts[2:]}] if parts[2:] else [])})
    wheres[7] = None
    wheres[9] = {"c1": "nowhere"}
    wheres[11] = {"c2": {"$in": [float(v) / 2 for v in range(-32, 32)]}}
    # all 16 columns between these two, at any n: a string constant some row has keeps its column in the program
    keep = lambda c: {f"c{c}": metas[0][f"c{c}"]} if c % 2 else leaf(c)          # noqa: E731
    wheres[12] = {"$and": [keep(c) for c in range(8)]}
    wheres[13] = {"$or": [keep(c) for c in range(8, 16)]}
    return metas, wheres


@pytest.mark.parametrize("n", [1, 31, 33, 127, 128, 129, 1000])
def test_filter_eval_is_bit_exact(N, n):
    metas, wheres = eval_table(n, 100 + n)
    reg = F.ColumnRegistry.from_metadatas(metas)
    progs = [F.compile_where(w, reg) for w in wheres]
    assert all(p is not None for p in progs)
    W = N.filter_words(n)
    assert W == 4 * ((n + 127) // 128)
    g = np.random.default_rng(n)
    alive = g.random(n) > 0.3
    for n_f, one_column in ((1, True), (5, True), (1, False), (5, False), (40, False)):
        mine = progs[:n_f] if one_column else progs[-n_f:] if n_f < 40 else progs
        ops, off, sets, keys = F.pack_programs(mine)
        if not one_column and n_f == 40:
            assert len(keys) == 16
        if one_column:
            assert keys == ["c0"]
        cols = [torch.from_numpy(np.ascontiguousarray(reg.host(k)[:n])).to("cuda") for k in keys]
        assert {c.dtype for c in cols} <= {torch.float64, torch.int32}
        for a in (None, alive):
            out = N.filter_eval(ops, off, sets, cols, n, alive_bits=None if a is None else alive_words(a), device="cuda")
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert got.shape == (n_f, W)
            for f, prog in enumerate(mine):
                flags = F.run_program_host(prog, reg.host_columns(prog.keys), n)
                want = F.pack_bits(flags if a is None else flags & a, W)       # zero from n to 128 ceil(n / 128)
                assert np.array_equal(got[f], want), (n_f, one_column, f)


def test_filter_eval_wrapper_checks_its_host_tables(N):
    reg = F.ColumnRegistry.from_metadatas([{"a": 1, "s": "x"}] * 10)
    ops, off, sets, keys = F.pack_programs([F.compile_where({"a": {"$in": [1, 2]}, "s": "x"}, reg)])
    cols = [torch.from_numpy(np.ascontiguousarray(reg.host(k)[:10])).to("cuda") for k in keys]
    bad = ops.copy()
    bad["column"][0] = 2
    with pytest.raises(N.MMRagNativeError, match="column"):
        N.filter_eval(bad, off, sets, cols, 10)
    with pytest.raises(N.MMRagNativeError, match="at least n"):
        N.filter_eval(ops, off, sets, cols, 11)
    with pytest.raises(N.MMRagNativeError, match="ascending"):
        N.filter_eval(ops, off[::-1].copy(), sets, cols, 10)
    cd, _ = to_dev(N, unit_rows(10, 8, 1), torch.float16)
    qd, _ = to_dev(N, unit_rows(2, 8, 2), torch.float16)
    vis = bitmaps(N, [np.ones(10, bool)], 10)
    for foq in ([0, 1], [0, -1], [0]):
        with pytest.raises(N.MMRagNativeError, match="filter_of_query"):
            N.filtered_topk(qd, cd, 10, 8, 3, foq, vis)
    with pytest.raises(N.MMRagNativeError, match="vis_bits"):
        N.filtered_topk(qd, cd, 10, 8, 3, [0, 0], vis[:, :2].contiguous())


# ---------------------------------------------------------------- 2. scan parity on arbitrary bitmaps
def patterns(n, n_f, seed):
    """n_f visibility patterns cycling through: all rows, none, one row, rows 126 .. 129 only (a tile edge), about 50 %
    random, about 2 % random"""
    g = np.random.default_rng(seed)
    out = []
    for f in range(n_f):
        v = np.zeros(n, bool)
        kind = f % 6
        if kind == 0:
            v[:] = True
        elif kind == 2:
            v[int(g.integers(0, n))] = True
        elif kind == 3:
            v[126:130] = True
        elif kind == 4:
            v = g.random(n) < 0.5
        elif kind == 5:
            v = g.random(n) < 0.02
        out.append(v)
    return out


PARITY = [
    (1, 1, 8, "f32", 1),
    (129, 3, 384, "f16", 5),
    (300, 128, 768, "bf16", 20),
    (1000, 129, 384, "f32", 21),
    (1000, 200, 768, "f16", 100),
    (129, 129, 8, "f16", 100),
]


@pytest.mark.parametrize("n,B,d,dt,k", PARITY)
def test_scan_parity_on_arbitrary_bitmaps(N, n, B, d, dt, k):
    n_f = B // 2 + 1
    vis = patterns(n, n_f, 5 * n + B)
    g = np.random.default_rng(n + B + k)
    foq = g.integers(0, n_f, B)
    foq[: min(B, n_f)] = np.arange(min(B, n_f))          # every bitmap is some query's
    counts = np.array([vis[f].sum() for f in foq])
    assert (counts >= k).any() and (B == 1 or (counts < k).any())      # a full answer and a padded one
    cd, cs = to_dev(N, unit_rows(n, d, 3 * n + d), DT[dt])
    qd, qs = to_dev(N, unit_rows(B, d, B + 11), DT[dt])
    s, r = run(N, qd, cd, n, d, k, foq, bitmaps(N, vis, n))
    es, er = R.topk_of_visible(qs, cs, k, [vis[f] for f in foq])
    check(s, r, es, er)
    assert np.array_equal((r >= 0).sum(1), np.minimum(counts, k))
    s2, r2 = run(N, qd, cd, n, d, k, foq, bitmaps(N, vis, n), row_offset=10 ** 10)
    assert np.array_equal(s2, s) and np.array_equal(r2[r >= 0], r[r >= 0] + 10 ** 10) and np.all(r2[r < 0] == -1)


def test_bits_past_n_are_ignored(N):
    """a bitmap from elsewhere may hold bits at and past n: rows that do not exist are never candidates"""
    n, B, d, k = 130, 2, 8, 5
    cd, cs = to_dev(N, unit_rows(n, d, 1), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 2), torch.float16)
    W = N.filter_words(n)
    words = torch.full((1, W), -1, dtype=torch.int32, device="cuda")
    s, r = run(N, qd, cd, n, d, k, [0, 0], words)
    es, er = R.topk_of_visible(qs, cs, k, [np.ones(n, bool)] * 2)
    check(s, r, es, er)


# ---------------------------------------------------------------- 3. equal to the scoped kernel, bit for bit
def test_equals_the_scoped_kernel_bit_for_bit(N):
    n, B, d, k = 1000, 200, 768, 100
    g = np.random.default_rng(31)
    col = (np.arange(n) // 20).astype(np.int32)
    col[g.choice(n, 50, replace=False)] = -1
    n_groups = 60                                            # ordinals 50 .. 59: no row has them
    S = B // 2 + 1
    scopes = [sorted(set(g.integers(0, n_groups, int(g.integers(1, 9))).tolist())) for _ in range(S)]
    scopes[3] = []
    soq = g.integers(0, S, B).astype(np.int32)
    soq[:S] = np.arange(S)
    cd, _ = to_dev(N, unit_rows(n, d, 32), torch.float16)
    qd, _ = to_dev(N, unit_rows(B, d, 33), torch.float16)
    off = np.cumsum([0] + [len(s) for s in scopes]).astype(np.int32)
    flat = np.array([o for s in scopes for o in s], dtype=np.int32)
    ss, sr = N.scoped_topk(qd, cd, n, d, k, torch.from_numpy(col).to("cuda"), n_groups, torch.from_numpy(soq),
                           torch.from_numpy(off), torch.from_numpy(flat), n)
    vis = [np.isin(col, np.array(s, dtype=np.int64)) & (col >= 0) for s in scopes]
    fs, fr = N.filtered_topk(qd, cd, n, d, k, soq, bitmaps(N, vis, n))
    torch.cuda.synchronize()
    assert torch.equal(fs, ss) and torch.equal(fr, sr)
    assert int((fr >= 0).sum()) > 0


# ---------------------------------------------------------------- 4. a query alone, and the items the scan issues
def items_of(vis, foq, n, B):
    """(row tile, query tile) pairs in which some query of the tile sees some row of the tile"""
    count = 0
    for qt in range((B + 127) // 128):
        seen = np.zeros(n, bool)
        for f in set(foq[qt * 128: (qt + 1) * 128].tolist()):
            seen |= vis[f]
        count += sum(bool(seen[t: t + 128].any()) for t in range(0, n, 128))
    return count


@pytest.mark.parametrize("mostly_skipped", [True, False])
def test_a_query_alone_equals_it_in_a_batch_and_items_issued(N, mostly_skipped):
    n, B, d, k = 1000, 200, 384, 20
    g = np.random.default_rng(41 + mostly_skipped)
    if mostly_skipped:
        # queries 0 .. 127 see rows of tiles 0 and 1 only, the others rows of tile 6 only: 3 of 16 items
        vis = []
        for f in range(64):
            v = np.zeros(n, bool)
            lo = int(g.integers(0, 230)) if f < 40 else int(g.integers(768, 870))
            v[lo: lo + int(g.integers(1, 25))] = True
            vis.append(v)
        foq = np.concatenate([g.integers(0, 40, 128), g.integers(40, 64, B - 128)])
        vis[0][0], vis[1][255] = True, True
        foq[0], foq[1] = 0, 1
    else:
        vis = patterns(n, 64, 43)                    # some query of each tile sees every row: nothing is skipped
        foq = g.integers(0, 64, B)
        foq[0], foq[150] = 0, 0
    want_items = items_of(vis, foq, n, B)
    assert want_items == (3 if mostly_skipped else 16)
    cd, _ = to_dev(N, unit_rows(n, d, 44), torch.float16)
    qd, _ = to_dev(N, unit_rows(B, d, 45), torch.float16)
    vd = bitmaps(N, vis, n)
    s, r, items = run(N, qd, cd, n, d, k, foq, vd, count_items=True)
    assert int(items[0]) == want_items
    for b in list(range(0, B, 9)) + [127, 128, B - 1]:
        s1, r1 = run(N, qd[b: b + 1].contiguous(), cd, n, d, k, [0], vd[foq[b]: foq[b] + 1].contiguous())
        assert np.array_equal(s1[0], s[b]) and np.array_equal(r1[0], r[b]), b


# ---------------------------------------------------------------- 5. bound stages and overflow
def test_bound_stages_are_exact_for_every_filter(N):
    """n = 20000 is above the 16384 candidate slots of k = 5, so one bound pass over 96 of the 157 row tiles runs first.
    The third filter shows fewer than k rows to that sample: its tau stays -inf"""
    n, B, d, k = 20000, 3, 8, 5
    T, walk = (n + 127) // 128, 96
    sampled = {i * T // walk for i in range(walk)}
    g = np.random.default_rng(51)
    rare = np.zeros(n, bool)
    outside = np.array([t for t in range(T) if t not in sampled])
    rare[(g.choice(outside, 97) * 128 + g.integers(0, 32, 97))] = True
    rare[[min(sampled) * 128 + 5, max(sampled) * 128 + 1, sorted(sampled)[40] * 128 + 127]] = True
    in_sample = sum(int(rare[t * 128: (t + 1) * 128].sum()) for t in sampled)
    assert 0 < in_sample < k <= rare.sum() <= 100
    vis = [np.ones(n, bool), g.random(n) < 0.5, rare]
    cd, cs = to_dev(N, unit_rows(n, d, 52), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 53), torch.float16)
    vd = bitmaps(N, vis, n)
    s, r = run(N, qd, cd, n, d, k, [0, 1, 2], vd)
    es, er = R.topk_of_visible(qs, cs, k, vis)
    check(s, r, es, er)
    s0, r0 = run(N, qd, cd, n, d, k, [0, 1, 2], vd, dbg=1)           # no bound pass: every visible row is a candidate
    assert np.array_equal(s, s0) and np.array_equal(r, r0)


def test_overflow_of_one_query_in_a_batch(N):
    """64 candidate slots at n = 1000: the queries whose filters pass more rows are produced again alone"""
    n, d, k = 1000, 384, 21
    g = np.random.default_rng(55)
    few = np.zeros(n, bool)
    few[g.choice(n, 50, replace=False)] = True
    vis = [np.ones(n, bool), few, g.random(n) < 0.5, np.zeros(n, bool)]
    foq = [1, 0, 2, 0, 3, 1]
    cd, cs = to_dev(N, unit_rows(n, d, 56), torch.bfloat16)
    qd, qs = to_dev(N, unit_rows(len(foq), d, 57), torch.bfloat16)
    vd = bitmaps(N, vis, n)
    s, r = run(N, qd, cd, n, d, k, foq, vd, cap=64)
    es, er = R.topk_of_visible(qs, cs, k, [vis[f] for f in foq])
    check(s, r, es, er)
    s0, r0 = run(N, qd, cd, n, d, k, foq, vd)
    assert np.array_equal(s, s0) and np.array_equal(r, r0)


# ---------------------------------------------------------------- 6. VectorIndex end to end
class Mirror:
    """the rows a VectorIndex holds, kept beside it: vectors as stored, metadata, add times, ids, alive flags"""

    def __init__(self, dim, dtype, **kw):
        from multimodal_rag_amd.index import VectorIndex

        self.idx = VectorIndex(dim=dim, dtype=dtype, device="cuda:0", capacity=256, **kw)
        self.dim, self.metas, self.ids, self.added = dim, [], [], 0
        self.times, self.alive = np.zeros(0), np.zeros(0, bool)

    def add(self, x, metas, times):
        ids = [f"id{self.added + i}" for i in range(len(metas))]
        self.added += len(metas)
        self.idx.add(x, documents=[f"text {i}" for i in ids], metadatas=metas, ids=ids, timestamps=times)
        self.metas += [dict(m) for m in metas]
        self.ids += ids
        self.times = np.concatenate([self.times, times])
        self.alive = np.concatenate([self.alive, np.ones(len(metas), bool)])

    def delete(self, ids):
        self.idx.delete(ids=ids)
        self.alive[[self.ids.index(i) for i in ids]] = False

    def compact(self):
        self.idx.compact()
        keep = np.nonzero(self.alive)[0]
        self.metas, self.ids = [self.metas[i] for i in keep], [self.ids[i] for i in keep]
        self.times, self.alive = self.times[keep], self.alive[keep]

    def stored(self):
        n = self.idx.rows_in_use
        assert n == len(self.ids)
        return self.idx._full[:n, : self.dim].to(torch.float32).cpu().numpy()

    def check(self, q, k, wheres, against_query=True):
        idx = self.idx
        res = idx.filtered_query(q, n_results=k, wheres=wheres)
        assert len(res["ids"]) == len(q)
        qs = torch.from_numpy(q).to(idx._full.dtype).to(torch.float32).numpy()
        cs = self.stored()
        vis = [R.visible(self.metas, w, self.alive, self.times) for w in wheres]
        es, er = R.topk_of_visible(qs, cs, k, vis)
        row_of = {s: i for i, s in enumerate(self.ids)}

        def as_arrays(ids, dist):
            m = len(ids)
            return (np.array([[1.0 - x for x in dist] + [-np.inf] * (k - m)], np.float32),
                    np.array([[row_of[i] for i in ids] + [-1] * (k - m)]))

        for b, w in enumerate(wheres):
            s, r = as_arrays(res["ids"][b], res["distances"][b])
            check(s, r, es[b: b + 1], er[b: b + 1])
            assert all(vis[b][row_of[i]] for i in res["ids"][b])
            assert res["metadatas"][b] == [self.metas[row_of[i]] for i in res["ids"][b]]
            if against_query and not F.names_added_at(w):
                want = idx.query(q[b: b + 1], n_results=k, where=w)
                check(s, r, *as_arrays(want["ids"][0], want["distances"][0]))
        return res


def index_filters():
    """40 distinct covered filters, None and "$added_at" ranges among them, and three the compiler refuses"""
    family = R.covered_filters(400, 2)
    picked, seen = [None, {"$added_at": {"$gte": R.T0 + 60.0 * 100, "$lt": R.T0 + 60.0 * 300}},
                    {"$and": [{"$added_at": {"$gt": R.T0 + 6000.0}}, {"type": "table"}]}, {"$added_at": {"$lt": R.T0}},
                    {"type": "table"}, {"page": {"$gte": 10, "$lte": 40}}, {"doc_id": "doc3"}], set()
    for w in family[4::8] + family[5::8]:
        if len(picked) == 40:
            break
        if repr(w) not in seen and w not in picked:
            seen.add(repr(w))
            picked.append(w)
    uncovered = [{"mixed": "m1"}, {"type": {"$gt": "t"}}, {"page": {"$in": list(range(5, 70))}}]
    return picked, uncovered


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_index_filtered_query_end_to_end(N, dt):
    d, k = 64, 7
    metas, times = R.metadata(400, 1)
    m = Mirror(d, DT[dt])
    m.add(unit_rows(400, d, 61), metas, times)
    covered, uncovered = index_filters()
    assert len(covered) == 40
    wheres = covered[:20] + uncovered[:2] + covered[20:] + uncovered[2:]        # the host-path filters in between
    for w in covered:
        assert m.idx.filter_plan(w)["device"], w
    for w in uncovered:
        plan = m.idx.filter_plan(w)
        assert not plan["device"] and plan["reason"]
    q = unit_rows(64, d, 62)
    m.check(q[: len(wheres)], k, wheres)
    one = m.idx.filtered_query(q[:3], n_results=k, wheres={"type": "table"})    # one dict for all
    assert all(meta["type"] == "table" for hits in one["metadatas"] for meta in hits)
    s, r = m.idx.filtered_search(q[: len(wheres)], k, wheres)
    assert s.shape == (len(wheres), k) and r.dtype == torch.int64 and s.is_cuda
    with pytest.raises(ValueError, match="added_at"):
        m.idx.filtered_query(q[:1], n_results=k, wheres=[{"$added_at": "yesterday"}])
    with pytest.raises(ValueError, match="unsupported where operator"):
        m.idx.filtered_query(q[:1], n_results=k, wheres=[{"page": {"$between": 1}}])
    with pytest.raises(ValueError, match="entries for"):
        m.idx.filtered_query(q[:2], n_results=k, wheres=[None])
    # add rows: the columns follow (new dictionary values, a later time range)
    more, more_times = R.metadata(100, 9)
    for i, meta in enumerate(more):
        meta["doc_id"] = f"new{i // 10}"
    m.add(unit_rows(100, d, 63), more, more_times + 60.0 * 400)
    wheres[4] = {"doc_id": {"$in": ["new3", "doc1"]}}
    wheres[5] = {"$added_at": {"$gte": R.T0 + 60.0 * 420}}
    m.check(q[: len(wheres)], k, wheres)
    # delete some
    m.delete([f"id{i}" for i in range(0, 500, 3)])
    m.check(q[: len(wheres)], k, wheres)
    # a row whose page is a string: filters on page take the host path from now on, results stay right
    m.add(unit_rows(1, d, 64), [{"page": "seven", "type": "table", "doc_id": "odd"}], np.array([R.T0]))
    plan = m.idx.filter_plan({"page": {"$gte": 10, "$lte": 40}})
    assert not plan["device"] and "page" in plan["reason"] and m.idx.filter_plan({"type": "table"})["device"]
    # (the host path cannot order a str against a number: TypeError, today's exception; equality and lists it can)
    page_free = [w for w in wheres if "page" not in repr(w)] + [{"type": "table"}, {"page": 7}, {"page": {"$ne": 7}},
                                                                {"page": {"$in": [3, 4, 5]}}]
    assert len(page_free) <= 64
    m.check(q[: len(page_free)], k, page_free)
    # compact
    m.compact()
    assert m.idx.rows_in_use == int(m.alive.sum()) == len(m.ids)
    m.check(q[: len(page_free)], k, page_free)
    # growth past the capacity
    cap = m.idx.matrix.shape[0]
    grow, grow_times = R.metadata(cap, 11)
    for meta in grow:
        meta.pop("page", None)
    m.add(unit_rows(cap, d, 65), grow, grow_times + 60.0 * 1000)
    assert m.idx.matrix.shape[0] > cap
    m.check(q[: len(page_free)], k, page_free, against_query=False)
    # reset: every column is dropped, page is a number again
    m.idx.reset()
    empty = m.idx.filtered_query(q[:2], n_results=k, wheres=[{"type": "table"}, None])
    assert empty["ids"] == [[], []]
    m2 = Mirror(d, DT[dt])
    m2.idx = m.idx
    m2.add(unit_rows(50, d, 66), metas[:50], times[:50])
    assert m2.idx.filter_plan({"page": {"$gte": 10}})["device"]
    m2.check(q[:4], k, [{"page": {"$gte": 10}}, None, {"type": "table"}, {"$added_at": {"$lt": R.T0 + 600.0}}])


def test_index_f8_collection_runs_on_its_plane(N):
    d, n, k = 64, 400, 6
    metas, times = R.metadata(n, 1)
    x, q = unit_rows(n, d, 71), unit_rows(4, d, 72)
    wheres = [{"type": "table"}, {"page": {"$lt": 20}}, None, {"doc_id": "nowhere"}]
    half, f8 = Mirror(d, torch.float16), Mirror(d, torch.float8_e4m3fn, rescore_dtype=torch.float16)
    half.add(x, metas, times)
    f8.add(x, metas, times)
    a, b = half.idx.filtered_query(q, k, wheres), f8.idx.filtered_query(q, k, wheres)
    assert a["ids"] == b["ids"] and a["distances"] == b["distances"] and a["ids"][3] == []
    lean = Mirror(d, torch.float8_e4m3fn, rescore_dtype=None)
    lean.add(x, metas, times)
    with pytest.raises(ValueError, match="MMRAG_F8_RESCORE=none"):
        lean.idx.filtered_query(q, k, wheres)


def test_index_serves_more_filters_than_one_launch_holds_in_slices(N, monkeypatch):
    from multimodal_rag_amd import config

    d, k = 64, 5
    metas, times = R.metadata(400, 1)
    m = Mirror(d, torch.float16)
    m.add(unit_rows(400, d, 75), metas, times)
    wheres = [{"doc_id": f"doc{i}"} for i in range(12)] + [{"type": "table"}] * 3
    q = unit_rows(len(wheres), d, 76)
    whole = m.idx.filtered_query(q, k, wheres)
    monkeypatch.setattr(config.settings, "MMRAG_FILTER_BITMAP_BYTES", 5 * 4 * N.filter_words(400))     # 5 per launch
    calls = []
    real = N.filtered_topk
    monkeypatch.setattr(N, "filtered_topk", lambda qd, *a, **kw: (calls.append(qd.shape[0]), real(qd, *a, **kw))[1])
    sliced = m.idx.filtered_query(q, k, wheres)
    assert calls == [5, 5, 5]
    assert sliced["ids"] == whole["ids"] and sliced["distances"] == whole["distances"]


# ---------------------------------------------------------------- 7. MMRAG_DEVICE_FILTERS
def test_device_filters_build_the_same_words_and_answers(N):
    d, k = 64, 7
    metas, times = R.metadata(400, 1)
    m = Mirror(d, torch.float16)
    m.add(unit_rows(400, d, 81), metas, times)
    covered, uncovered = index_filters()
    wheres = [w for w in covered if w and not F.names_added_at(w)][:24] + uncovered
    q = unit_rows(3, d, 82)
    assert m.idx.device_filters is False
    for dead in (False, True):
        if dead:
            m.delete([f"id{i}" for i in range(5, 400, 4)])
        for w in wheres:
            m.idx.device_filters = False
            host = m.idx._where_bits(w)
            off = m.idx.query(q, n_results=k, where=w)
            m.idx.device_filters = True
            dev = m.idx._where_bits(w)
            on = m.idx.query(q, n_results=k, where=w)
            assert host.dtype == dev.dtype and host.shape == dev.shape and torch.equal(host, dev), w
            assert on["ids"] == off["ids"] and on["distances"] == off["distances"], w
    # the reserved key exists with device filters only
    times_only = {"$added_at": {"$gte": R.T0 + 6000.0}}
    got = m.idx.query(q, n_results=k, where=times_only)
    want = m.idx.filtered_query(q, n_results=k, wheres=times_only)
    assert got["ids"] == want["ids"] and all(len(ids) == k for ids in got["ids"])
    with pytest.raises(ValueError, match="added_at"):
        m.idx.query(q, n_results=k, where={"$added_at": None})
    m.idx.device_filters = False
    assert m.idx.query(q, n_results=k, where=times_only)["ids"] == [[], [], []]       # today's path: no such metadata


# ---------------------------------------------------------------- 8. manager and dispatcher on the HIP engine
def test_manager_and_dispatcher_serve_different_filters_in_one_call(N, monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd.embedder import EmbeddingManager

    monkeypatch.setattr(config.settings, "MMRAG_DEVICE_FILTERS", True)
    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_device_filters()
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình"]
    g = np.random.default_rng(99)
    docs = [f"doc{i}" for i in range(8)]
    for doc in docs:
        items = [{"id": f"{doc}_{i}", "type": ["text", "table"][i % 2],
                  "summary": f"{doc} {i} " + " ".join(g.choice(words, int(g.integers(3, 9))))} for i in range(10)]
        asyncio.run(m.embed_and_store(items, doc))
    filters = [{"doc_id": doc} for doc in docs] + [{"type": "table"}, {"$and": [{"type": "text"}, {"doc_id": docs[2]}]},
                                                  {"doc_id": {"$nin": docs[:6]}}, {"doc_id": "nowhere"}]
    texts = [f"{words[i % 12]} {words[(i * 5 + 1) % 12]}" for i in range(len(filters))]
    alone = [asyncio.run(m.query(t, n_results=4, filter_dict=f)) for t, f in zip(texts, filters)]
    assert alone[-1]["ids"] == [] and all(meta["type"] == "table" for meta in alone[8]["metadatas"])

    async def go():
        disp = m.enable_dynamic_batching(max_batch=64, max_wait_ms=500.0)
        disp.idle = 0.05
        calls = []
        real = disp.filtered_fn
        assert real is not None

        async def counted(texts, k, flts):
            calls.append(len(texts))
            return await real(texts, k, flts)

        disp.filtered_fn = counted
        try:
            out = await asyncio.gather(*[m.query(t, n_results=4, filter_dict=f) for t, f in zip(texts, filters)])
        finally:
            await disp.stop()
            m._dispatcher = None
        return out, calls

    out, calls = asyncio.run(go())
    assert calls == [len(filters)]                       # ONE filtered call for twelve different filters
    for res, one in zip(out, alone):
        assert "error" not in res and res["ids"] == one["ids"]
        assert np.allclose(res["distances"], one["distances"], atol=TOL, rtol=0)
    asyncio.run(m.cleanup())
