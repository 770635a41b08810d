"""GPU: boosted retrieval (csrc/boosted.hip through _native.boosted_topk, VectorIndex.set_prior / boosted_search /
boosted_query, EmbeddingManager, the dispatcher and POST /query) against tests/boost_ref.py.

The bar is tests/test_search_gpu.py's, on the FINAL scores (|w * prior| <= 1 throughout, so it carries over): within
1e-4 of the reference, identical id sets with candidates within 2e-4 of the k-th score interchangeable; bit-equal
wherever the data is exactly representable or where two runs of the kernel are compared (a final score's bits depend on
the query row, the stored row, d, the query's weight and the row's prior alone)."""
import asyncio
import time
import types

import numpy as np
import pytest
import torch

from oracle import search_oracle as O
from tests import boost_ref as R

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


def check_boosts(bo, r, prior, w, row_offset=0):
    """every hit's boost is the exact float32 product of ITS row's prior and its query's weight; 0 in padding"""
    want = np.zeros_like(bo)
    for b in range(r.shape[0]):
        hit = r[b] >= 0
        want[b, hit] = np.float32(w[b]) * prior[r[b, hit] - row_offset]
    assert np.array_equal(bo, want)


def run(N, qd, cd, n, d, k, prior, w, alive=None, **kw):
    s, r, bo = N.boosted_topk(qd, cd, n, d, k, prior, w, alive_bits=None if alive is None else bits_of(alive), **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy(), bo.cpu().numpy()


def weights(B, seed):
    """per query in [-1, 1], every third one exactly 0"""
    w = np.random.default_rng(seed).uniform(-1.0, 1.0, B).astype(np.float32)
    w[::3] = 0.0
    return w


# ---------------------------------------------------------------- 1. the C-ABI against the reference, no bound pass
PARITY = [
    (1, 1, 8, "f32", 1),
    (129, 3, 384, "f16", 5),
    (300, 128, 768, "bf16", 20),
    (1000, 129, 200, "f32", 21),
    (1000, 200, 768, "f16", 100),
    (129, 129, 8, "f16", 100),
]


@pytest.mark.parametrize("n,B,d,dt,k", PARITY)
def test_parity(N, n, B, d, dt, k):
    g = np.random.default_rng(n + B + k)
    alive = g.random(n) > 0.03
    if n == 1:
        alive[:] = True
    prior = g.random(n).astype(np.float32)
    w = weights(B, n + d)
    if B == 1:
        w[:] = 0.75
    cd, cs = to_dev(N, unit_rows(n, d, 3 * n + d), DT[dt])
    qd, qs = to_dev(N, unit_rows(B, d, B + 11), DT[dt])
    s, r, bo = run(N, qd, cd, n, d, k, prior, w, alive)
    es, er, eb = R.boosted_topk(qs, cs, k, prior, w, alive)
    check(s, r, es, er)
    check_boosts(bo, r, prior, w)
    same = r == er
    assert np.array_equal(bo[same], eb[same])
    if k > n:
        assert np.all(r[:, int(alive.sum()):] == -1) and np.all(bo[:, int(alive.sum()):] == 0.0)


# ---------------------------------------------------------------- 2. the bound passes
@pytest.fixture(scope="module")
def big(N):
    """17 000 x 64 float16 rows (132 full tiles and one of 104 rows: more than the 16 384 candidate slots of k <= 512, so
    the bound passes run), 130 queries and their float64 cosines, computed once"""
    n, d, B = 17000, 64, 130
    cd, cs = to_dev(N, unit_rows(n, d, 201), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 202), torch.float16)
    return {"n": n, "d": d, "B": B, "cd": cd, "cs": cs, "qd": qd, "qs": qs,
            "cos": qs.astype(np.float64) @ cs.astype(np.float64).T}


def big_priors(big, name):
    n, B = big["n"], big["B"]
    if name == "rising":                 # a recency prior: rises with the row number
        return (np.arange(n) / (n - 1)).astype(np.float32), weights(B, 203)
    if name.startswith("tile"):          # 30 rows of ONE tile carry everything
        prior = np.zeros(n, np.float32)
        at = int(name[4:]) * 128 + 40
        prior[at: at + 30] = 1.0
        return prior, np.ones(B, np.float32)
    # anti-correlated with query 0's cosine: what that query likes best is pushed down hardest
    cos0 = big["cos"][0]
    return np.clip(-cos0 / np.abs(cos0).max(), -1.0, 1.0).astype(np.float32), np.ones(B, np.float32)


@pytest.mark.parametrize("k", [5, 100])
@pytest.mark.parametrize("name", ["rising", "tile0", "tile77", "tile3", "anti"])
def test_bound_passes_lose_nothing(N, big, name, k):
    """a threshold that is ever too high loses hits: equal to the reference, and bit-equal to the scan without bound
    passes (tau = -inf: every live row a candidate, every query through the overflow re-run).  The one bound stage
    samples tiles i * 133 // 96 of the 133: tiles 0 and 77 are in the sample, tile 3 is not"""
    n, d = big["n"], big["d"]
    assert n > N.candidate_capacity(k)
    sampled = {i * 133 // 96 for i in range(96)}
    assert {0, 77} <= sampled and 3 not in sampled
    prior, w = big_priors(big, name)
    alive = np.random.default_rng(204).random(n) > 0.03
    if name.startswith("tile"):
        alive[prior > 0] = True
    s, r, bo = run(N, big["qd"], big["cd"], n, d, k, prior, w, alive)
    es, er, _ = R.boosted_topk(big["qs"], big["cs"], k, prior, w, alive)
    check(s, r, es, er)
    check_boosts(bo, r, prior, w)
    if name.startswith("tile"):          # cosines of a 64-d random corpus stay far below 1: the 30 rows lead every list
        lead = min(k, 30)
        assert np.all(prior[r[:, :lead]] == 1.0) and (k <= 30 or np.all(prior[r[:, 30:]] == 0.0))
    s1, r1, b1 = run(N, big["qd"], big["cd"], n, d, k, prior, w, alive, dbg=1)
    assert np.array_equal(s, s1) and np.array_equal(r, r1) and np.array_equal(bo, b1)


# ---------------------------------------------------------------- 3. exactly representable data
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_integer_data_bit_exact_with_heavy_ties(N, dt):
    """rows and queries in {-2..2}/8 on 4 columns, priors in {0..8}/16, weights in {-1, -0.5, 0, 0.5, 1}: every product
    and sum is exact in float32, so scores, rows (ties -> the lower row) and boosts equal the reference bit for bit"""
    n, B, d, k = 1000, 200, 384, 100
    g = np.random.default_rng(5)
    c = np.zeros((n, d), np.float32)
    c[:, :4] = g.integers(-2, 3, (n, 4)) / 8
    q = np.zeros((B, d), np.float32)
    q[:, :4] = g.integers(-2, 3, (B, 4)) / 8
    prior = (g.integers(0, 9, n) / 16).astype(np.float32)
    w = g.choice(np.array([-1, -0.5, 0, 0.5, 1], np.float32), B)
    cd, cs = to_dev(N, c, DT[dt])
    qd, qs = to_dev(N, q, DT[dt])
    s, r, bo = run(N, qd, cd, n, d, k, prior, w)
    es, er, eb = R.boosted_topk(qs, cs, k, prior, w)
    assert np.array_equal(s, es) and np.array_equal(r, er) and np.array_equal(bo, eb)


# ---------------------------------------------------------------- 4. overflow, batches, weight 0
def test_overflow_rerun_of_every_query(N):
    """256 candidate slots for 1000 rows and no threshold (n is below the real capacity): every query overflows and is
    produced again alone"""
    n, d, k, B = 1000, 384, 21, 6
    g = np.random.default_rng(53)
    prior, w = g.random(n).astype(np.float32), weights(B, 54)
    alive = g.random(n) > 0.03
    cd, cs = to_dev(N, unit_rows(n, d, 51), torch.bfloat16)
    qd, qs = to_dev(N, unit_rows(B, d, 52), torch.bfloat16)
    s, r, bo = run(N, qd, cd, n, d, k, prior, w, alive, cap=256)
    es, er, _ = R.boosted_topk(qs, cs, k, prior, w, alive)
    check(s, r, es, er)
    check_boosts(bo, r, prior, w)
    s0, r0, b0 = run(N, qd, cd, n, d, k, prior, w, alive)
    assert np.array_equal(s, s0) and np.array_equal(r, r0) and np.array_equal(bo, b0)


def test_a_query_does_not_depend_on_its_batch(N):
    n, B, d, k = 1000, 200, 384, 20
    g = np.random.default_rng(41)
    prior, w = g.random(n).astype(np.float32), weights(B, 42)
    cd, _ = to_dev(N, unit_rows(n, d, 44), torch.float16)
    qd, _ = to_dev(N, unit_rows(B, d, 45), torch.float16)
    prior_dev = torch.from_numpy(prior).to("cuda")
    s, r, bo = run(N, qd, cd, n, d, k, prior_dev, w)
    for b in range(B):
        s1, r1, b1 = run(N, qd[b: b + 1].contiguous(), cd, n, d, k, prior_dev, w[b: b + 1])
        assert np.array_equal(s1[0], s[b]) and np.array_equal(r1[0], r[b]) and np.array_equal(b1[0], bo[b]), b


def test_weight_zero_is_the_scoped_kernels_plain_topk(N):
    """one tile body, one K order: with weight 0 the scores are mmrag_scoped_topk's bits for a scope of every row"""
    n, B, d, k = 1000, 130, 384, 20
    g = np.random.default_rng(61)
    prior = g.random(n).astype(np.float32)
    alive = g.random(n) > 0.03
    cd, cs = to_dev(N, unit_rows(n, d, 62), torch.float16)
    qd, qs = to_dev(N, unit_rows(B, d, 63), torch.float16)
    s, r, bo = run(N, qd, cd, n, d, k, prior, 0.0, alive)
    col = torch.zeros(n, dtype=torch.int32, device="cuda")
    ss, sr = N.scoped_topk(qd, cd, n, d, k, col, 1, [0] * B, [0, 1], [0], n, alive_bits=bits_of(alive))
    assert np.array_equal(s, ss.cpu().numpy()) and np.array_equal(r, sr.cpu().numpy())
    es, er, _ = R.boosted_topk(qs, cs, k, prior, 0.0, alive)
    check(s, r, es, er)
    assert np.all(bo == 0.0)


def test_alive_bits_row_offset_and_an_all_dead_collection(N):
    n, B, d, k = 300, 3, 8, 5
    g = np.random.default_rng(71)
    prior, w = g.random(n).astype(np.float32), np.array([1.0, -0.5, 0.0], np.float32)
    cd, cs = to_dev(N, unit_rows(n, d, 72), torch.float32)
    qd, qs = to_dev(N, unit_rows(B, d, 73), torch.float32)
    alive = np.ones(n, bool)
    alive[:29] = False
    alive[125:135] = False
    for a in (None, alive):
        s, r, bo = run(N, qd, cd, n, d, k, prior, w, a, row_offset=10 ** 10)
        es, er, _ = R.boosted_topk(qs, cs, k, prior, w, a, row_offset=10 ** 10)
        check(s, r, es, er)
        check_boosts(bo, r, prior, w, row_offset=10 ** 10)
    assert r.min() >= 10 ** 10 + 29 and not np.any((r >= 10 ** 10 + 125) & (r < 10 ** 10 + 135))
    s, r, bo = run(N, qd, cd, n, d, k, prior, w, np.zeros(n, bool))
    assert np.all(np.isneginf(s)) and np.all(r == -1) and np.all(bo == 0.0)
    s, r, bo = run(N, qd, cd, 0, d, k, np.zeros(0, np.float32), w)                # an empty collection
    assert np.all(np.isneginf(s)) and np.all(r == -1) and np.all(bo == 0.0)


def test_wrapper_checks_launch_nothing(N, monkeypatch):
    cd, _ = to_dev(N, unit_rows(10, 8, 1), torch.float16)
    qd, _ = to_dev(N, unit_rows(2, 8, 2), torch.float16)
    calls = []
    monkeypatch.setattr(N.lib(), "mmrag_internal_boosted_topk_ex", lambda *a: calls.append(a) or 0)
    ok = np.zeros(10, np.float32)
    bad_prior = ok.copy()
    bad_prior[3] = np.nan
    for prior, w, k in ((bad_prior, 1.0, 3), (np.full(10, np.inf), 1.0, 3), (ok, float("nan"), 3), (ok, [1.0, np.inf], 3),
                        (ok[:9], 1.0, 3), (np.zeros(11, np.float32), 1.0, 3), (ok, [1.0, 1.0, 1.0], 3), (ok, 1.0, 0),
                        (ok, 1.0, 4097), (torch.zeros(9, device="cuda"), 1.0, 3)):
        with pytest.raises(ValueError):
            N.boosted_topk(qd, cd, 10, 8, k, prior, w)
    assert calls == []
    N.boosted_topk(qd, cd, 10, 8, 3, ok, 1.0)
    assert len(calls) == 1


# ---------------------------------------------------------------- 5. VectorIndex
NOW = 1_760_000_000.0
DAY = 86400.0
KINDS = ("text", "table", "image")


def index_fixture(n, d, seed, dtype=torch.float16, **kw):
    from multimodal_rag_amd.index import VectorIndex

    g = np.random.default_rng(seed)
    rows = unit_rows(n, d, seed + 1)
    times = NOW - g.uniform(-5.0, 120.0, n) * DAY              # a few in the future
    times[g.choice(n, n // 25, replace=False)] = np.nan        # and a few unknown
    metas = [{"type": KINDS[int(i)], "parity": j % 2} for j, i in enumerate(g.integers(0, 3, n))]
    idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=256, **kw)
    idx.add(rows, documents=[f"text {i}" for i in range(n)], metadatas=[dict(m) for m in metas],
            ids=[f"id{i}" for i in range(n)], timestamps=times)
    return idx, rows, times, metas


def spec_prior(times, metas, recency, half_life_s, table):
    age = np.maximum(0.0, NOW - times)
    term = np.where(np.isnan(times), 0.0, recency * 2.0 ** (-age / half_life_s))
    return (term + np.array([table.get(m["type"], 0.0) for m in metas])).astype(np.float32)


def assert_index_equals_reference(idx, q, k, prior_name, w, ids, rows16, prior, where_mask=None, where=None):
    """boosted_query against the reference over the surviving rows `ids` (original numbers, in row order)"""
    res = idx.boosted_query(q, n_results=k, prior=prior_name, weight=w, where=where)
    q16 = q.astype(np.float16).astype(np.float32)
    wq = np.broadcast_to(np.asarray(w, np.float32), (len(q),))
    es, er, _ = R.boosted_topk(q16, rows16[ids], k, prior[ids], wq, where_mask[ids] if where_mask is not None else None)
    B = len(q)
    s = np.full((B, k), -np.inf, np.float32)
    r = np.full((B, k), -1, np.int64)
    local = {int(o): i for i, o in enumerate(ids)}
    for b in range(B):
        m = len(res["ids"][b])
        assert m == len(res["scores"][b]) == len(res["boosts"][b]) == len(res["distances"][b])
        got = [int(s_[2:]) for s_ in res["ids"][b]]
        s[b, :m] = res["scores"][b]
        r[b, :m] = [local[o] for o in got]
        cos = q16[b].astype(np.float64) @ rows16[got].astype(np.float64).T
        assert np.all(np.abs((1.0 - np.array(res["distances"][b])) - cos) <= TOL)
        assert np.array_equal(np.array(res["boosts"][b], np.float32), np.float32(wq[b]) * prior[got])
        assert res["metadatas"][b] == [{"type": idx._metadatas[idx._row_of[f"id{o}"]]["type"], "parity": o % 2}
                                       for o in got]
    check(s, r, es, er)
    return res


def test_index_boosted_query_through_add_delete_compact(N):
    from multimodal_rag_amd.boost import BoostSpec

    d, n, k = 384, 1500, 8
    idx, rows, times, metas = index_fixture(n, d, 301)
    q = unit_rows(12, d, 303)
    table = {"table": 0.3, "image": -0.2}
    spec = BoostSpec(recency=0.5, half_life_s=30 * DAY, values={"type": table}, now=NOW)
    idx.set_prior("default", spec=spec)
    pins = np.random.default_rng(304).random(n).astype(np.float32)
    idx.set_prior("pins", values=pins)
    rows16 = rows.astype(np.float16).astype(np.float32)
    sp = spec_prior(times, metas, 0.5, 30 * DAY, table)
    ids = np.arange(n)
    w = weights(12, 305)
    assert_index_equals_reference(idx, q, k, "default", 1.0, ids, rows16, sp)
    assert_index_equals_reference(idx, q, k, "pins", w, ids, rows16, pins)
    assert_index_equals_reference(idx, q, k, spec, 0.5, ids, rows16, sp)               # a spec as it is: the same column
    assert len(idx._spec_cols) == 1
    is_table = np.array([m["type"] == "table" for m in metas])
    res = assert_index_equals_reference(idx, q, k, "default", 1.0, ids, rows16, sp, is_table, where={"type": "table"})
    assert all(m["type"] == "table" for hits in res["metadatas"] for m in hits)
    # grow: rows added later follow the spec at ITS now and get 0.0 in the caller's own column
    g = np.random.default_rng(306)
    more = unit_rows(400, d, 307)
    more_t = NOW - g.uniform(0.0, 60.0, 400) * DAY
    more_m = [{"type": KINDS[i % 3], "parity": (n + i) % 2} for i in range(400)]
    idx.add(more, documents=[f"text {n + i}" for i in range(400)], metadatas=[dict(m) for m in more_m],
            ids=[f"id{n + i}" for i in range(400)], timestamps=more_t)
    rows16 = np.concatenate([rows16, more.astype(np.float16).astype(np.float32)])
    times, metas = np.concatenate([times, more_t]), metas + more_m
    sp = spec_prior(times, metas, 0.5, 30 * DAY, table)
    pins = np.concatenate([pins, np.zeros(400, np.float32)])
    ids = np.arange(n + 400)
    assert_index_equals_reference(idx, q, k, "default", 1.0, ids, rows16, sp)
    assert_index_equals_reference(idx, q, k, "pins", w, ids, rows16, pins)
    # delete, then compact: the columns and the times follow the rows
    gone = g.choice(n + 400, 300, replace=False)
    idx.delete(ids=[f"id{i}" for i in gone])
    alive = np.ones(n + 400, bool)
    alive[gone] = False
    assert_index_equals_reference(idx, q, k, "default", 1.0, ids, rows16, sp, alive)
    idx.compact()
    ids = np.nonzero(alive)[0]
    assert np.array_equal(idx.row_times(), times[ids], equal_nan=True)
    assert_index_equals_reference(idx, q, k, "default", 1.0, ids, rows16, sp)
    assert_index_equals_reference(idx, q, k, "pins", w, ids, rows16, pins)

    def add_after_compact(m, seed):
        """m further rows on top of compacted columns: the spec column at ITS now, 0.0 in the caller's own column"""
        nonlocal rows16, times, metas, sp, pins, alive, ids
        first = len(times)
        new = unit_rows(m, d, seed)
        new_t = NOW - np.random.default_rng(seed + 1).uniform(-2.0, 90.0, m) * DAY
        new_t[::17] = np.nan
        new_m = [{"type": KINDS[(i + 1) % 3], "parity": (first + i) % 2} for i in range(m)]
        idx.add(new, documents=[f"text {first + i}" for i in range(m)], metadatas=[dict(x) for x in new_m],
                ids=[f"id{first + i}" for i in range(m)], timestamps=new_t)
        rows16 = np.concatenate([rows16, new.astype(np.float16).astype(np.float32)])
        times, metas = np.concatenate([times, new_t]), metas + new_m
        sp = spec_prior(times, metas, 0.5, 30 * DAY, table)
        pins = np.concatenate([pins, np.zeros(m, np.float32)])
        alive = np.concatenate([alive, np.ones(m, bool)])
        ids = np.nonzero(alive)[0]
        assert np.array_equal(idx.row_times(), times[ids], equal_nan=True)
        assert_index_equals_reference(idx, q, k, "default", 1.0, ids, rows16, sp)
        assert_index_equals_reference(idx, q, k, "pins", w, ids, rows16, pins)

    # add after compact: enough rows to outgrow the capacity, so the compacted columns are regrown as well
    cap = idx.matrix.shape[0]
    add_after_compact(cap - idx.count() + 100, 308)
    assert idx.matrix.shape[0] > cap
    # a compaction that SHRINKS the capacity (fewer than a quarter of it survive), then an add into the shrunk columns
    cap = idx.matrix.shape[0]
    gone = np.random.default_rng(309).choice(ids, ids.size - cap // 4 + 200, replace=False)
    idx.delete(ids=[f"id{i}" for i in gone])
    alive[gone] = False
    idx.compact()
    assert idx.matrix.shape[0] < cap
    ids = np.nonzero(alive)[0]
    assert_index_equals_reference(idx, q, k, "pins", w, ids, rows16, pins)
    add_after_compact(150, 310)
    new_rows = np.arange(len(times) - 150, len(times))
    res = idx.boosted_query(rows16[new_rows[:3]], n_results=1, prior="pins", weight=-1.0)
    assert [hit[0] for hit in res["ids"]] == [f"id{i}" for i in new_rows[:3]] and all(b == [0.0] for b in res["boosts"])
    with pytest.raises(ValueError):
        idx.set_prior("pins", values=np.zeros(3))
    with pytest.raises(ValueError):
        idx.boosted_query(q, n_results=k, prior="nobody")
    with pytest.raises(ValueError):
        idx.boosted_query(q, n_results=5000)
    assert idx._metadatas[0] == {"type": metas[ids[0]]["type"], "parity": int(ids[0]) % 2}   # nothing was added to it
    idx.reset()
    assert idx._priors == {} and not idx._spec_cols


def test_index_spec_columns_are_cached_by_floored_now(N, monkeypatch):
    from multimodal_rag_amd import boost as boost_mod
    from multimodal_rag_amd.boost import BoostSpec

    idx, *_ = index_fixture(300, 64, 311)
    clock = {"t": NOW + 100.0}
    monkeypatch.setattr(boost_mod, "time", types.SimpleNamespace(time=lambda: clock["t"]))
    spec = BoostSpec(recency=0.5)
    q = unit_rows(2, 64, 312)
    idx.boosted_search(q, 3, prior=spec)
    col = idx._spec_cols[spec.cache_key()]["col"]
    clock["t"] += 50.0                                       # the same hour: the same column object
    idx.boosted_search(q, 3, prior=BoostSpec(recency=0.5))
    assert len(idx._spec_cols) == 1 and idx._spec_cols[spec.cache_key()]["col"] is col
    clock["t"] += 3600.0                                     # the floored time moved on: a new column
    idx.boosted_search(q, 3, prior=spec)
    assert len(idx._spec_cols) == 2
    # an add keeps the column in use current and drops the one of the hour that has passed
    more = unit_rows(5, 64, 313)
    more_t = np.array([clock["t"], clock["t"] - 30 * DAY, np.nan, clock["t"] + DAY, clock["t"] - 60 * DAY])
    idx.add(more, ids=[f"late{i}" for i in range(5)], timestamps=more_t)
    assert list(idx._spec_cols) == [spec.cache_key()]
    got = idx._spec_cols[spec.cache_key()]["col"][300:305].cpu().numpy()
    assert np.array_equal(got, spec.column(more_t, [{}] * 5, spec.cache_key()[1]))
    assert got[2] == 0.0 and got[3] == np.float32(0.5) and abs(got[4] - 0.125) < 1e-3
    for i in range(4):                                       # at most MAX_SPEC_COLUMNS, the oldest evicted
        idx.boosted_search(q, 3, prior=BoostSpec(recency=0.1 * (i + 1), now=NOW))
    assert len(idx._spec_cols) == idx.MAX_SPEC_COLUMNS
    assert all(key[1] == NOW for key in idx._spec_cols)


def test_index_f8_collection_runs_on_its_plane(N):
    d, n, k = 384, 800, 6
    g = np.random.default_rng(321)
    rows, q = unit_rows(n, d, 322), unit_rows(5, d, 323)
    pins = g.random(n).astype(np.float32)
    out = []
    for dtype, kw in ((torch.float16, {}), (torch.float8_e4m3fn, {"rescore_dtype": torch.float16})):
        from multimodal_rag_amd.index import VectorIndex

        idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=256, **kw)
        idx.add(rows, ids=[f"id{i}" for i in range(n)], timestamps=NOW)
        idx.set_prior("pins", values=pins)
        out.append(idx.boosted_query(q, k, prior="pins", weight=0.5))
    assert out[0]["ids"] == out[1]["ids"] and out[0]["scores"] == out[1]["scores"]
    assert out[0]["distances"] == out[1]["distances"]
    lean = VectorIndex(dim=d, dtype=torch.float8_e4m3fn, device="cuda:0", capacity=256, rescore_dtype=None)
    lean.add(rows, ids=[f"id{i}" for i in range(n)])
    lean.set_prior("pins", values=pins)
    with pytest.raises(ValueError, match="MMRAG_F8_RESCORE=none"):
        lean.boosted_query(q, k, prior="pins")


def test_added_at_survives_save_and_load(N, tmp_path):
    from multimodal_rag_amd.persistence import load_index, save_index

    idx, rows, times, metas = index_fixture(200, 64, 331)
    before = idx.query(rows[:4], n_results=3)
    save_index(idx, str(tmp_path / "ix"))
    back = load_index(str(tmp_path / "ix"))
    assert np.array_equal(back.row_times(), times, equal_nan=True)
    assert back.query(rows[:4], n_results=3) == before and back._metadatas == metas
    import json

    with open(tmp_path / "ix" / "tables.json", encoding="utf-8") as f:
        t = json.load(f)
    del t["added_at"]                                         # a directory written before the times existed
    with open(tmp_path / "ix" / "tables.json", "w", encoding="utf-8") as f:
        json.dump(t, f)
    old = load_index(str(tmp_path / "ix"))
    assert np.all(np.isnan(old.row_times())) and old.query(rows[:4], n_results=3) == before


# ---------------------------------------------------------------- 6. manager, dispatcher and endpoint on the HIP engine
def test_manager_and_dispatcher_boost_the_newer_upload(N, monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd import index as index_mod
    from multimodal_rag_amd.embedder import EmbeddingManager

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    monkeypatch.setattr(config.settings, "MMRAG_BOOST_TIME_KEY", "published")
    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_boost()
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình"]
    texts = [f"{words[i % 12]} {words[(i * 5 + 1) % 12]} {words[(i * 7 + 2) % 12]}" for i in range(16)]
    now = time.time()
    for doc, when in (("old", now - 365 * DAY), ("new", now)):           # the same texts, a year apart
        items = [{"id": f"{doc}_{i}", "type": "text", "summary": t, "published": when} for i, t in enumerate(texts)]
        asyncio.run(m.embed_and_store(items, doc))
    assert "published" not in m.collection._metadatas[0]
    plain = asyncio.run(m.query(texts[3], n_results=4))
    assert plain["metadatas"][0]["doc_id"] == "old"                       # tied cosines: the earlier row
    boost = {"recency": 0.2, "half_life_days": 30}
    solo = [asyncio.run(m.boosted_query(t, n_results=4, boost=boost)) for t in texts]
    for res in solo:
        assert res["metadatas"][0]["doc_id"] == "new" and abs(res["boosts"][0] - 0.2) < 1e-6
        assert res["scores"] == sorted(res["scores"], reverse=True)
        assert all(abs(sc - (1.0 - dist) - bo) < 1e-4 for sc, dist, bo in zip(res["scores"], res["distances"], res["boosts"]))
    assert abs(solo[3]["distances"][0] - plain["distances"][0]) < 1e-4

    calls = {"boosted": 0}
    real = index_mod._native.boosted_topk
    monkeypatch.setattr(index_mod._native, "boosted_topk",
                        lambda *a, **kw: (calls.__setitem__("boosted", calls["boosted"] + 1), real(*a, **kw))[1])

    async def go():
        disp = m.enable_dynamic_batching(max_batch=64, max_wait_ms=200.0)
        try:
            assert disp.boosted_fn is not None
            out = await asyncio.gather(*[m.boosted_query(t, n_results=4, boost=boost) for t in texts])
            stats = dict(disp.stats)
        finally:
            await disp.stop()
            m._dispatcher = None
        return out, stats

    out, stats = asyncio.run(go())
    assert calls["boosted"] == 1 and stats["batches"] == 1 and stats["max_batch_seen"] == 16, (calls, stats)
    for res, alone in zip(out, solo):
        assert res["ids"] == alone["ids"] and res["scores"] == alone["scores"] and res["distances"] == alone["distances"]
    asyncio.run(m.cleanup())


def test_query_endpoint_boost(N):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    with TestClient(create_app()) as c:
        bodies = [" ".join(f"Học máy là gì, phần {i}." for i in range(60)), "GPU kernel và dữ liệu. " * 3,
                  "Machine learning cơ bản, học máy. " * 3, "Bảng và ảnh. " * 3]
        for i, body in enumerate(bodies):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
        before = c.post("/query", json={"query": "học máy", "top_k": 3})
        assert before.status_code == 200, before.text
        r = c.post("/query", json={"query": "học máy", "top_k": 3,
                                   "boost": {"recency": 0.3, "half_life_days": 1, "values": {"type": {"text": 0.25}}}})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert len(src) == 3 and set(src[0]) == set(before.json()["sources"][0]) | {"boost", "score"}
        assert all(abs(s["boost"] - 0.55) < 1e-3 for s in src)            # uploaded just now, every item a text
        assert [s["score"] for s in src] == sorted((s["score"] for s in src), reverse=True)
        assert [s["doc_id"] for s in src] == [s["doc_id"] for s in before.json()["sources"]]   # a constant prior
        after = c.post("/query", json={"query": "học máy", "top_k": 3})
        assert after.json()["sources"] == before.json()["sources"] and after.json()["answer"] == before.json()["answer"]
        r = c.post("/query", json={"query": "học máy", "boost": {"recency": 0.3}, "mmr": True})
        assert r.status_code == 400 and "not combined" in r.json()["detail"]
