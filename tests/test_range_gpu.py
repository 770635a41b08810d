"""GPU: range retrieval (csrc/range.hip through _native.range_scan, VectorIndex.range_search / range_query) against
tests/range_ref.py.

Counts and facet slots are compared for EQUALITY: on integer rows every product and sum is exact, and on unit rows every
threshold sits in the middle of a gap of at least 4e-4 between consecutive reference scores (range_ref.gap_threshold),
2e-4 on each side, above the 1e-4 score tolerance.  Hit scores are within 1e-4 of the reference, identical sets with
candidates within 2e-4 of the last score interchangeable; bit-equal where two runs of the kernels are compared."""
import numpy as np
import pytest
import torch

from multimodal_rag_amd import filters as F
from oracle import search_oracle as O
from tests import filter_ref
from tests import range_ref as R

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


def to_dev(N, x, dtype):
    """(device rows in the padded width, the values as stored up-cast to float32 on the host)"""
    n, d = x.shape
    ld = N.padded_dim(d, dtype)
    t = torch.zeros((max(n, 1), ld), dtype=dtype, device="cuda")
    if n:
        t[:n, :d] = torch.from_numpy(x).to("cuda").to(dtype)
    return t, t[:n, :d].to(torch.float32).cpu().numpy()


def bitmaps(N, vis, n):
    """bool [F, n] -> device int32 [F, filter_words(n)]"""
    W = N.filter_words(n)
    words = np.stack([F.pack_bits(v, W) for v in vis])
    return torch.from_numpy(words.view(np.int32)).to("cuda").contiguous()


def codes_dev(codes):
    return [torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to("cuda") for c in codes]


def run(N, qd, cd, n, d, thr, limit, cols=(), sizes=(), **kw):
    out = N.range_scan(qd, cd, n, d, thr, limit, cols, sizes, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def split(facets, sizes):
    out, lo = [], 0
    for G in sizes:
        out.append(facets[:, lo:lo + G + 1])
        lo += G + 1
    assert facets.shape[1] == lo
    return out


def check_tables(got, ref, sizes):
    counts, facets = got[0], got[1]
    assert np.array_equal(counts, ref[0]), (counts, ref[0])
    if sizes:
        for t, e in zip(split(facets, sizes), ref[1]):
            assert np.array_equal(t, e)
            assert np.array_equal(t.sum(axis=1), counts)
    else:
        assert facets is None


def check_hits(s, r, es, er):
    assert r.shape == er.shape and s.shape == es.shape
    fin = np.isfinite(es)
    assert np.array_equal(np.isfinite(s), fin)
    assert np.array_equal(r[~fin], er[~fin])  # -1 padding
    assert np.all(np.abs(s[fin] - es[fin]) <= TOL)
    assert np.all(np.diff(s, axis=1)[fin[:, 1:]] <= 0)  # descending
    assert O.same_topk_sets(r, s, er, es)


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def facet_codes(n, sizes, seed):
    """codes in -1 .. G + 1 per column: -1 and values at and past G among them"""
    g = np.random.default_rng(seed)
    return [g.integers(-1, G + 2, n).astype(np.int32) for G in sizes]


def gap_thresholds(qs, cs, vis, targets):
    """one threshold per query in a gap of ITS visible reference scores, near targets[b % len(targets)] passing rows"""
    s = R.scores64(qs, cs)
    thr = []
    for b in range(len(qs)):
        mine = s[b] if vis is None else s[b][vis[b]]
        thr.append(R.gap_threshold(mine, targets[b % len(targets)]) if mine.size >= 2 else 0.0)
    return np.array(thr, np.float32)


# ---------------------------------------------------------------- 1. integer rows: everything is exact
INT_THR = [0.0, -3.0, 4.0, 1000.0, 1.0]      # a negative one and one above every score among them


def int_thresholds(s64):
    """INT_THR in turn, but query 0 mod 5 gets its median score and query 2 mod 5 the score most of its rows have:
    integers that rows hit exactly, which tells >= from >"""
    thr = np.array([INT_THR[b % len(INT_THR)] for b in range(len(s64))], np.float32)
    for b in range(len(s64)):
        if b % 5 == 0:
            thr[b] = np.sort(s64[b])[s64.shape[1] // 2]
        elif b % 5 == 2:
            vals, cnt = np.unique(s64[b], return_counts=True)
            thr[b] = vals[np.argmax(cnt)]
    return thr


@pytest.mark.parametrize("d", [64, 100])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_integer_rows_are_exact(N, dt, d):
    for n in (1, 127, 128, 129, 1000):
        cd, cs = to_dev(N, int_rows(n, d, 10 * n + d), DT[dt])
        for B in (1, 5, 130):
            qd, qs = to_dev(N, int_rows(B, d, 7 * n + B), DT[dt])
            s64 = R.scores64(qs, cs)
            thr = int_thresholds(s64)
            assert (s64[0] == thr[0]).sum() >= 1
            if n >= 127 and B >= 5:
                assert (s64[2] == thr[2]).sum() > 1                                # ">=" is told from ">"
            for sizes in ([3], [1, 200]) if B != 5 else ([200], [3, 1]):
                codes = facet_codes(n, sizes, n + B + len(sizes))
                ref = R.range_ref(qs, cs, thr, 7, None, codes, sizes)
                got = run(N, qd, cd, n, d, thr, 7, codes_dev(codes), sizes)
                check_tables(got, ref, sizes)
                assert np.array_equal(got[3], ref[3])                              # ties to the lower row, exactly
                assert np.array_equal(got[2], ref[2])
                if B >= 4:
                    assert got[0][3] == 0 and np.all(got[3][3] == -1)              # the threshold above every score


# ---------------------------------------------------------------- 2. unit rows, thresholds in gaps, per-query bitmaps
@pytest.mark.parametrize("n,d,B,dt", [(129, 64, 5, "f16"), (129, 64, 5, "bf16"), (129, 64, 5, "f32"),
                                      (1000, 100, 130, "f16"), (3000, 64, 3, "f16"), (20000, 64, 3, "f16"),
                                      (1000, 384, 5, "f32")])
def test_unit_rows_with_gap_thresholds_and_bitmaps(N, n, d, B, dt):
    cd, cs = to_dev(N, unit_rows(n, d, n + d), DT[dt])
    qd, qs = to_dev(N, unit_rows(B, d, n + d + 1), DT[dt])
    g = np.random.default_rng(n)
    filters = np.stack([g.random(n) > 0.4, np.zeros(n, bool), g.random(n) > 0.4, np.ones(n, bool)])   # 40 % dead; empty
    foq = np.array([(0, 2, 1, 7, 3)[b % 5] for b in range(B)])     # 7: outside 0..F-1, sees nothing
    vis = np.stack([filters[f] if f < 4 else np.zeros(n, bool) for f in foq])
    sizes = [3, 200]
    codes = facet_codes(n, sizes, n + 2)
    cols = codes_dev(codes)
    targets = [1, 10, max(n // 20, 2)]
    limit = 10
    for v, kw in ((vis, {"filter_of_query": foq, "vis_bits": bitmaps(N, filters, n)}), (None, {})):
        thr = gap_thresholds(qs, cs, v, targets)
        ref = R.range_ref(qs, cs, thr, limit, v, codes, sizes)
        got = run(N, qd, cd, n, d, thr, limit, cols, sizes, **kw)
        check_tables(got, ref, sizes)
        check_hits(got[2], got[3], ref[2], ref[3])
        if v is not None:
            assert all(c == 0 for b, c in enumerate(got[0]) if foq[b] in (1, 7))
            assert all(v[b][r] for b in range(B) for r in got[3][b] if r >= 0)
        assert got[0].max() >= min(n // 20, 2)


def test_bits_past_n_and_row_offset(N):
    n, d, B = 200, 64, 3
    cd, cs = to_dev(N, unit_rows(n, d, 1), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 2), torch.float16)
    W = N.filter_words(n)
    ones = torch.full((1, W), -1, dtype=torch.int32, device="cuda")          # bits at and past n are set
    thr = gap_thresholds(qs, cs, None, [20])
    ref = R.range_ref(qs, cs, thr, 5, None, row_offset=1000)
    got = run(N, qd, cd, n, d, thr, 5, filter_of_query=[0] * B, vis_bits=ones, row_offset=1000)
    check_tables(got, ref, [])
    check_hits(got[2], got[3], ref[2], ref[3])
    same_bits(got, run(N, qd, cd, n, d, thr, 5, row_offset=1000))


def test_empty_collection_and_refusals(N):
    d = 64
    cd, _ = to_dev(N, np.zeros((0, d), np.float32), torch.float16)
    qd, _ = to_dev(N, unit_rows(2, d, 3), torch.float16)
    col = torch.zeros(4, dtype=torch.int32, device="cuda")
    counts, facets, s, r = run(N, qd, cd, 0, d, 0.5, 3, [col], [2])
    assert counts.tolist() == [0, 0] and not facets.any() and facets.shape == (2, 3)
    assert np.all(np.isneginf(s)) and np.all(r == -1)
    with pytest.raises(ValueError, match="finite"):
        N.range_scan(qd, cd, 0, d, float("nan"), 3)
    with pytest.raises(N.MMRagNativeError, match="threshold holds"):
        N.range_scan(qd, cd, 0, d, [0.1, 0.2, 0.3], 3)
    c8 = torch.zeros((4, 128), dtype=torch.float8_e4m3fn, device="cuda")
    with pytest.raises(N.MMRagNativeError, match="range-scanned"):
        N.range_scan(c8[:2].contiguous(), c8, 4, 64, 0.5, 3)


# ---------------------------------------------------------------- 3. overflow: the re-run counts nothing twice
def test_overflow_rerun_leaves_the_tables_alone(N):
    n, d, B, limit = 3000, 64, 5, 20
    cd, cs = to_dev(N, unit_rows(n, d, 31), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 32), torch.float16)
    thr = gap_thresholds(qs, cs, None, [1000, 10, 1000, 300, 1])
    sizes = [3, 200]
    codes = facet_codes(n, sizes, 33)
    cols = codes_dev(codes)
    ref = R.range_ref(qs, cs, thr, limit, None, codes, sizes)
    assert ref[0][0] > 256 and ref[0][2] > 256 and ref[0][1] < 256      # some queries overflow 256 slots, some do not
    full = run(N, qd, cd, n, d, thr, limit, cols, sizes)
    small = run(N, qd, cd, n, d, thr, limit, cols, sizes, cap=256)
    check_tables(full, ref, sizes)
    check_tables(small, ref, sizes)
    check_hits(full[2], full[3], ref[2], ref[3])
    same_bits(full, small)


# ---------------------------------------------------------------- 4. bound passes: tau > threshold, counts unchanged
@pytest.mark.parametrize("limit", [5, 100])
def test_bound_passes_do_not_change_counts(N, limit):
    n, d, B = 20000, 64, 3
    assert n > N.lib().mmrag_internal_candidate_capacity(limit)          # the plan stages bound passes
    sizes = [3]
    codes = facet_codes(n, sizes, 41)
    cols = codes_dev(codes)
    # dense: integer rows, a threshold about half the rows pass, hit exactly by many
    cd, cs = to_dev(N, int_rows(n, d, 42), torch.float16)
    qd, qs = to_dev(N, int_rows(B, d, 43), torch.float16)
    thr = np.zeros(B, np.float32)
    ref = R.range_ref(qs, cs, thr, limit, None, codes, sizes)
    assert np.all(ref[0] > n // 3) and np.all(ref[0] < 16384)
    bounded = run(N, qd, cd, n, d, thr, limit, cols, sizes)
    plain = run(N, qd, cd, n, d, thr, limit, cols, sizes, dbg=1)
    same_bits(bounded, plain)
    check_tables(bounded, ref, sizes)
    assert np.array_equal(bounded[3], ref[3]) and np.array_equal(bounded[2], ref[2])
    # sparse: unit rows, a gap threshold
    cd, cs = to_dev(N, unit_rows(n, d, 44), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 45), torch.float16)
    thr = gap_thresholds(qs, cs, None, [n // 20, 10, 1])
    ref = R.range_ref(qs, cs, thr, limit, None, codes, sizes)
    bounded = run(N, qd, cd, n, d, thr, limit, cols, sizes)
    plain = run(N, qd, cd, n, d, thr, limit, cols, sizes, dbg=1)
    same_bits(bounded, plain)
    check_tables(bounded, ref, sizes)
    check_hits(bounded[2], bounded[3], ref[2], ref[3])


# ---------------------------------------------------------------- 5. limit == 0: the numbers alone
def test_limit_zero_counts_without_hit_outputs(N):
    for n, seed in ((1000, 51), (20000, 52)):
        d, B = 64, 5
        cd, cs = to_dev(N, int_rows(n, d, seed), torch.bfloat16)
        qd, qs = to_dev(N, int_rows(B, d, seed + 1), torch.bfloat16)
        thr = np.array(INT_THR, np.float32)
        sizes = [1, 3]
        codes = facet_codes(n, sizes, seed + 2)
        cols = codes_dev(codes)
        g = np.random.default_rng(seed)
        filters = np.stack([g.random(n) > 0.4, g.random(n) > 0.9])
        foq = [0, 1, 0, 1, 0]
        vb = bitmaps(N, filters, n)
        ref = R.range_ref(qs, cs, thr, 0, filters[foq], codes, sizes)
        zero = run(N, qd, cd, n, d, thr, 0, cols, sizes, filter_of_query=foq, vis_bits=vb)
        five = run(N, qd, cd, n, d, thr, 5, cols, sizes, filter_of_query=foq, vis_bits=vb)
        assert zero[2] is None and zero[3] is None
        check_tables(zero, ref, sizes)
        same_bits(zero[:2], five[:2])
        same_bits(zero[:2], run(N, qd, cd, n, d, thr, 0, cols, sizes, filter_of_query=foq, vis_bits=vb)[:2])


# ---------------------------------------------------------------- 6. a query's outputs do not depend on the batch
def test_a_query_alone_equals_it_in_a_batch(N):
    n, d, B, limit = 1000, 100, 130, 9
    cd, cs = to_dev(N, unit_rows(n, d, 61), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 62), torch.float16)
    thr = gap_thresholds(qs, cs, None, [50, 5, 200])
    sizes = [200]
    cols = codes_dev(facet_codes(n, sizes, 63))
    g = np.random.default_rng(64)
    filters = np.stack([g.random(n) > 0.4, g.random(n) > 0.7, np.zeros(n, bool)])
    foq = g.integers(0, 3, B)
    vb = bitmaps(N, filters, n)
    whole = run(N, qd, cd, n, d, thr, limit, cols, sizes, filter_of_query=foq, vis_bits=vb)
    for b in (0, 77, 129):
        alone = run(N, qd[b:b + 1].contiguous(), cd, n, d, thr[b:b + 1], limit, cols, sizes,
                    filter_of_query=foq[b:b + 1], vis_bits=vb)
        same_bits(alone, tuple(t[b:b + 1] for t in whole))
    # one launch against the batch split in two (another grid of query tiles)
    lo = run(N, qd[:60].contiguous(), cd, n, d, thr[:60], limit, cols, sizes, filter_of_query=foq[:60], vis_bits=vb)
    hi = run(N, qd[60:].contiguous(), cd, n, d, thr[60:], limit, cols, sizes, filter_of_query=foq[60:], vis_bits=vb)
    same_bits(tuple(np.concatenate([a, b]) for a, b in zip(lo, hi)), whole)


# ---------------------------------------------------------------- 7. VectorIndex
class Held:
    """a VectorIndex and, beside it, what it holds: metadata, ids, alive flags"""

    def __init__(self, dim, dtype, x, metas, **kw):
        from multimodal_rag_amd.index import VectorIndex

        self.idx = VectorIndex(dim=dim, dtype=dtype, device="cuda:0", capacity=256, **kw)
        self.dim = dim
        self.ids = [f"id{i}" for i in range(len(metas))]
        self.metas = [dict(m) for m in metas]
        self.alive = np.ones(len(metas), bool)
        self.idx.add(x, documents=[f"text {i}" for i in self.ids], metadatas=metas, ids=self.ids)

    def delete(self, ids):
        self.idx.delete(ids=ids)
        self.alive[[self.ids.index(i) for i in ids]] = False

    def compact(self):
        self.idx.compact()
        keep = np.nonzero(self.alive)[0]
        self.metas, self.ids = [self.metas[i] for i in keep], [self.ids[i] for i in keep]
        self.alive = self.alive[keep]

    def stored(self):
        n = self.idx.rows_in_use
        assert n == len(self.ids)
        return self.idx._full[:n, : self.dim].to(torch.float32).cpu().numpy()

    def expect(self, q, wheres, target):
        """(thresholds in gaps of each query's visible scores, bool [B, n] visibility)"""
        qs = torch.from_numpy(q).to(self.idx._full.dtype).to(torch.float32).numpy()
        vis = np.stack([filter_ref.visible(self.metas, w, self.alive) for w in wheres])
        return qs, vis, gap_thresholds(qs, self.stored(), vis, [target])

    def check(self, q, wheres, keys, limit, target=10):
        qs, vis, thr = self.expect(q, wheres, target)
        s64 = R.scores64(qs, self.stored())
        res = self.idx.range_query(q, thr.tolist(), limit=limit, wheres=wheres, facets=keys)
        row_of = {s: i for i, s in enumerate(self.ids)}
        for b in range(len(q)):
            passing = np.nonzero(vis[b] & (s64[b] >= thr[b]))[0]
            assert res["total"][b] == passing.size and res["truncated"][b] == (passing.size > limit)
            for key in keys:
                want = {}
                for r in passing:
                    v = self.metas[r].get(key)
                    want[v] = want.get(v, 0) + 1
                got = res["facets"][b][key]
                assert {e["value"]: e["count"] for e in got} == want and len(got) == len(want)
                assert [e["count"] for e in got] == sorted((e["count"] for e in got), reverse=True)
            hits = [row_of[i] for i in res["ids"][b]]
            assert len(hits) == min(limit, passing.size) and set(hits) <= set(passing.tolist())
            assert np.all(np.abs((1.0 - np.array(res["distances"][b])) - s64[b][hits]) <= TOL)
            assert res["metadatas"][b] == [self.metas[r] for r in hits]
        return res, thr


INDEX_WHERES = [None, {"type": "table"}, {"page": {"$lt": 20}}, {"mixed": "m1"}, {"doc_id": "nowhere"},
                {"type": {"$in": ["text", "image"]}}]


def test_index_range_query_end_to_end(N, monkeypatch):
    from multimodal_rag_amd import config

    d, n, limit = 64, 400, 6
    metas, _ = filter_ref.metadata(n, 1)
    for m in metas[5::9]:
        del m["type"]                                      # rows without the key: the missing slot
    h = Held(d, torch.float16, unit_rows(n, d, 71), metas)
    q = unit_rows(len(INDEX_WHERES), d, 72)
    assert not h.idx.filter_plan({"mixed": "m1"})["device"]          # one filter the compiler does not cover
    keys = ["type", "doc_id"]
    res, thr = h.check(q, INDEX_WHERES, keys, limit)
    assert res["total"][4] == 0 and res["ids"][4] == [] and res["facets"][4] == {"type": [], "doc_id": []}
    # everything passes at -1: the totals are the matching rows, rows without the key are the None entry
    every = h.idx.range_query(q[:2], -1.0, limit=3, wheres=[None, {"type": "table"}], facets=["type"])
    assert every["total"] == [n, sum(m.get("type") == "table" for m in metas)] and every["truncated"] == [True, True]
    assert {e["value"]: e["count"] for e in every["facets"][0]["type"]}[None] == len(metas[5::9])
    assert every["facets"][1]["type"] == [{"value": "table", "count": every["total"][1]}]
    # the raw call; hit scores are filtered_search's bits for the same rows
    counts, tables, s, r, values = h.idx.range_search(q, thr, limit=limit, wheres=INDEX_WHERES, facets=keys)
    assert counts.dtype == torch.int64 and counts.is_cuda and counts.tolist() == res["total"]
    assert [t.shape for t in tables] == [(len(q), len(v) + 1) for v in values] and values[0][:1] == [metas[0]["type"]]
    assert all(t.dtype == torch.int64 and t.sum(dim=1).tolist() == res["total"] for t in tables)
    fs, fr = h.idx.filtered_search(q, limit, INDEX_WHERES)
    for b, c in enumerate(counts.tolist()):
        m = min(c, limit)
        assert torch.equal(r[b, :m], fr[b, :m]) and torch.equal(s[b, :m].view(torch.int32), fs[b, :m].view(torch.int32))
        assert bool((r[b, m:] == -1).all()) and bool(torch.isneginf(s[b, m:]).all())
    # limit 0 and one threshold for all
    zero = h.idx.range_query(q, float(thr[0]), limit=0, wheres=None, facets="type")
    assert zero["ids"] == [[]] * len(q) and zero["total"][0] == res["total"][0]
    assert zero["facets"][0]["type"] == res["facets"][0]["type"]
    # a table budget that splits the batch by queries: the same answer; smaller than one query: refused
    slots = sum(len(v) + 1 for v in values)
    monkeypatch.setattr(config.settings, "MMRAG_RANGE_TABLE_BYTES", 4 * slots * 2)
    again = h.idx.range_query(q, thr.tolist(), limit=limit, wheres=INDEX_WHERES, facets=keys)
    assert again == res
    monkeypatch.setattr(config.settings, "MMRAG_RANGE_TABLE_BYTES", 4 * slots - 1)
    with pytest.raises(ValueError, match="MMRAG_RANGE_TABLE_BYTES"):
        h.idx.range_query(q, thr.tolist(), limit=limit, wheres=INDEX_WHERES, facets=keys)
    h.idx.range_query(q, thr.tolist(), limit=limit, wheres=INDEX_WHERES)             # no tables, no budget
    monkeypatch.setattr(config.settings, "MMRAG_RANGE_TABLE_BYTES", 256 << 20)
    for bad, what in (({"threshold": 1.5}, "cosine"), ({"threshold": [0.1, 0.2]}, "entries for"),
                      ({"limit": -1}, "limit"), ({"facets": list("abcde")}, "facets"), ({"wheres": [None]}, "entries for")):
        kw = {"threshold": 0.5, "limit": 3, **bad}
        with pytest.raises(ValueError, match=what):
            h.idx.range_query(q, **kw)
    # tombstones, then compaction: the group columns follow
    h.delete([f"id{i}" for i in range(0, n, 3)])
    h.check(q, INDEX_WHERES, keys, limit)
    h.compact()
    h.check(q, INDEX_WHERES, keys, limit)
    more, _ = filter_ref.metadata(50, 9)
    for i, meta in enumerate(more):
        meta["doc_id"] = f"new{i // 10}"
    h.idx.add(unit_rows(50, d, 73), documents=["t"] * 50, metadatas=more, ids=[f"more{i}" for i in range(50)])
    h.ids += [f"more{i}" for i in range(50)]
    h.metas += more
    h.alive = np.concatenate([h.alive, np.ones(50, bool)])
    h.check(q, INDEX_WHERES, keys, limit)


def test_index_f8_collection_scans_its_plane(N):
    d, n = 64, 400
    metas, _ = filter_ref.metadata(n, 1)
    x, q = unit_rows(n, d, 81), unit_rows(4, d, 82)
    wheres = [{"type": "table"}, {"page": {"$lt": 20}}, None, {"doc_id": "nowhere"}]
    half = Held(d, torch.float16, x, metas)
    f8 = Held(d, torch.float8_e4m3fn, x, metas, rescore_dtype=torch.float16)
    _, _, thr = half.expect(q, wheres, 10)
    a = half.idx.range_query(q, thr.tolist(), limit=5, wheres=wheres, facets=["type"])
    b = f8.idx.range_query(q, thr.tolist(), limit=5, wheres=wheres, facets=["type"])
    assert a == b and a["total"][3] == 0 and max(a["total"]) >= 5
    lean = Held(d, torch.float8_e4m3fn, x, metas, rescore_dtype=None)
    with pytest.raises(ValueError, match="MMRAG_F8_RESCORE=none"):
        lean.idx.range_query(q, 0.5, limit=5)
