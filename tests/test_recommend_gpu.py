"""GPU: recommend retrieval (csrc/recommend.hip through _native.recommend_topk, VectorIndex.recommend_search /
recommend_query, EmbeddingManager, the dispatcher, POST /query and POST /recommend) against tests/recommend_ref.py.

The project's bar is 1e-4 per dot and a final combines two dots, pos - w * max(neg, 0): finals within (1 + w) * 1e-4 of
the reference, identical id sets with candidates within twice that of the k-th score interchangeable (w <= 1 in the
random tests: at most 2e-4 and 4e-4).  The explain outputs are single dots: 1e-4.  Bit-equal wherever the data is
exactly representable or where two runs of the kernel are compared (a final's bits depend on the request's examples,
signs and weight and the stored row alone)."""
import asyncio

import numpy as np
import pytest
import torch

from oracle import search_oracle as O
from tests import recommend_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
E = 16
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


COUNTS = [(1, 0), (16, 0), (1, 15), (3, 2), (5, 11), (2, 0), (4, 7), (1, 1)]    # (positives, negatives) of a request


def requests(R_, d, seed, rows=None, counts=COUNTS):
    """R_ requests: (examples [16 R, d] float32, sign int8 [16 R], weights float32 [R] in [0, 1]), the example counts
    cycling through `counts`; every second example is a stored row (when there are any), so that negatives bite"""
    g = np.random.default_rng(seed)
    pos, neg = [], []
    for i in range(R_):
        p, m = counts[i % len(counts)]
        v = unit_rows(p + m, d, seed * 1000 + i)
        if rows is not None and len(rows):
            for j in range(0, p + m, 2):
                v[j] = rows[g.integers(len(rows))]
        pos.append(v[:p])
        neg.append(v[p:])
    ex, sign = R.pack(pos, neg, d)
    w = g.uniform(0.0, 1.0, R_).astype(np.float32)
    w[::3] = 1.0
    w[1::5] = 0.0
    return ex, sign, w


def run(N, ed, sign, w, cd, n, d, k, alive=None, **kw):
    out = N.recommend_topk(ed, sign, w, cd, n, d, k, alive_bits=None if alive is None else bits_of(alive), **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check(s, r, es, er, w):
    """finals within (1 + w) * 1e-4 of the reference, request by request; sets with twice that as the margin"""
    assert r.shape == er.shape and s.shape == es.shape
    fin = np.isfinite(es)
    assert np.array_equal(np.isfinite(s), fin)
    assert np.array_equal(r[~fin], er[~fin])  # -1 padding
    w = np.broadcast_to(np.asarray(w, np.float32), (s.shape[0],))
    for g in range(s.shape[0]):
        tol = (1.0 + float(w[g])) * TOL
        assert np.all(np.abs(s[g][fin[g]] - es[g][fin[g]]) <= tol), g
        assert O.same_topk_sets(r[g: g + 1], s[g: g + 1], er[g: g + 1], es[g: g + 1], margin=2 * tol), g
    with np.errstate(invalid="ignore"):           # (-inf) - (-inf) in the padding, masked out below
        assert np.all(np.diff(s, axis=1)[fin[:, 1:]] <= 0)  # descending


def check_explain(out, ex, sign, cs, row_offset=0):
    """every hit's pos / neg is the largest float64 dot of ITS row with the request's positives / negatives to 1e-4, the
    slot named is one that reaches it (to 2e-4: two dots are compared), neg = 0 / -1 without a negative; 0 / -1 padding"""
    s, r, pos, neg, pa, na = out
    sign = np.asarray(sign).reshape(-1, E)
    pad = r < 0
    assert np.all(pos[pad] == 0) and np.all(neg[pad] == 0) and np.all(pa[pad] == -1) and np.all(na[pad] == -1)
    for g in range(r.shape[0]):
        hit = np.nonzero(r[g] >= 0)[0]
        if not hit.size:
            continue
        dots = ex[E * g: E * (g + 1)].astype(np.float64) @ cs[r[g, hit] - row_offset].astype(np.float64).T   # [16, hits]
        at = np.arange(hit.size)
        for val, arg, sel in ((pos, pa, sign[g] > 0), (neg, na, sign[g] < 0)):
            if not sel.any():
                assert np.all(val[g, hit] == 0) and np.all(arg[g, hit] == -1)
                continue
            best = dots[sel].max(axis=0)
            assert np.all(np.abs(val[g, hit] - best) <= TOL), g
            assert np.all(sel[arg[g, hit]]), g
            assert np.all(dots[arg[g, hit], at] >= best - 2 * TOL), g


# ---------------------------------------------------------------- 1. the C-ABI against the reference, no bound pass
PARITY = [
    (1, 1, 8, "f32", 1),
    (129, 8, 384, "f16", 5),
    (300, 9, 768, "bf16", 21),
    (1000, 130, 200, "f32", 21),
    (1000, 9, 768, "f16", 100),
    (129, 130, 8, "bf16", 100),
    (300, 8, 200, "f16", 5),
    (1, 1, 8, "f32", 5),                 # k > n: one hit, then padding
    (129, 9, 8, "bf16", 4096),           # the deep end of k, every live row a hit, then padding
    (300, 130, 384, "f16", 1000),
]


@pytest.mark.parametrize("n,R_,d,dt,k", PARITY)
def test_parity(N, n, R_, d, dt, k):
    g = np.random.default_rng(n + R_ + k)
    alive = g.random(n) > 0.03
    if n == 1:
        alive[:] = True
    cd, cs = to_dev(N, unit_rows(n, d, 3 * n + d), DT[dt])
    ex, sign, w = requests(R_, d, n + d + R_, rows=cs)
    ed, exs = to_dev(N, ex, DT[dt])
    out = run(N, ed, sign, w, cd, n, d, k, alive)
    es, er, *_ = R.recommend_topk(exs, sign, w, cs, k, alive)
    check(out[0], out[1], es, er, w)
    check_explain(out, exs, sign, cs)
    if k > n:                            # hits first, then (-inf, -1) and 0 / -1 explain padding
        live = int(alive.sum())
        assert np.all(out[1][:, :live] >= 0) and np.all(out[1][:, live:] == -1) and np.all(np.isneginf(out[0][:, live:]))
        assert np.all(out[2][:, live:] == 0) and np.all(out[3][:, live:] == 0)
        assert np.all(out[4][:, live:] == -1) and np.all(out[5][:, live:] == -1)
    s, r, *rest = N.recommend_topk(ed, sign, w, cd, n, d, k, alive_bits=bits_of(alive), want_explain=False)
    assert rest == [None] * 4           # every explain output null: the same ranking
    assert np.array_equal(s.cpu().numpy(), out[0]) and np.array_equal(r.cpu().numpy(), out[1])


# ---------------------------------------------------------------- 2. more than one launch
def test_more_requests_than_one_launch_takes(N):
    """520 requests: a launch of 64 example tiles (512 requests) and one of a single tile"""
    n, R_, d, k = 300, 520, 8, 5
    cd, cs = to_dev(N, unit_rows(n, d, 21), torch.float16)
    ex, sign, w = requests(R_, d, 22, rows=cs)
    ed, exs = to_dev(N, ex, torch.float16)
    out = run(N, ed, sign, w, cd, n, d, k)
    es, er, *_ = R.recommend_topk(exs, sign, w, cs, k)
    check(out[0], out[1], es, er, w)
    check_explain(out, exs, sign, cs)


# ---------------------------------------------------------------- 3. the bound passes
@pytest.fixture(scope="module")
def big(N):
    """17 000 x 64 float16 rows (132 full tiles and one of 104 rows: more than the 16 384 candidate slots of k <= 512, so
    the bound passes run), built once"""
    n, d = 17000, 64
    cd, cs = to_dev(N, unit_rows(n, d, 201), torch.float16)
    return {"n": n, "d": d, "cd": cd, "cs": cs, "alive": np.random.default_rng(204).random(n) > 0.03}


def big_requests(big, name):
    """20 requests of the case `name`: (positives, negatives, weights, rows that must stay alive)"""
    n, d, cs, R_ = big["n"], big["d"], big["cs"], 20
    g = np.random.default_rng(205)
    w = g.uniform(0.0, 1.0, R_).astype(np.float32)
    w[::2] = 1.0
    keep = np.zeros(0, np.int64)
    if name == "near":                   # negatives = the 13 stored rows nearest the 3 positives
        pos = [unit_rows(3, d, 300 + i).astype(np.float16).astype(np.float32) for i in range(R_)]
        neg = []
        for p in pos:
            best = (p.astype(np.float64) @ cs.astype(np.float64).T).max(axis=0)
            neg.append(cs[np.argsort(-best)[:13]])
    elif name.startswith("tile"):        # 4 positives copied from rows of ONE tile, 2 random negatives
        t = int(name[4:])
        pos, neg = [], [unit_rows(2, d, 400 + i) for i in range(R_)]
        for i in range(R_):
            at = t * 128 + g.choice(128, 4, replace=False)
            keep = np.concatenate([keep, at])
            pos.append(cs[at])
    else:                                # "same": the negatives equal the positives
        pos = [unit_rows(3, d, 500 + i) for i in range(R_)]
        neg = [p.copy() for p in pos]
    return pos, neg, w, keep


@pytest.mark.parametrize("k", [5, 100])
@pytest.mark.parametrize("name", ["near", "tile77", "tile3", "same"])
def test_bound_passes_lose_nothing(N, big, name, k):
    """a threshold that is ever too high loses hits: equal to the reference, and bit-equal to the scan without bound
    passes (tau = -inf: every live row a candidate, every request through the overflow re-run).  The one bound stage
    samples tiles i * 133 // 96 of the 133: tile 77 is in the sample, tile 3 is not"""
    n, d = big["n"], big["d"]
    assert n > N.candidate_capacity(k)
    sampled = {i * 133 // 96 for i in range(96)}
    assert 77 in sampled and 3 not in sampled
    pos, neg, w, keep = big_requests(big, name)
    alive = big["alive"].copy()
    alive[keep] = True
    ex, sign = R.pack(pos, neg, d)
    ed, exs = to_dev(N, ex, torch.float16)
    out = run(N, ed, sign, w, big["cd"], n, d, k, alive)
    es, er, *_ = R.recommend_topk(exs, sign, w, big["cs"], k, alive)
    check(out[0], out[1], es, er, w)
    check_explain(out, exs, sign, big["cs"])
    if name.startswith("tile"):          # cosines of a 64-d random corpus stay far below 1: the 4 copies lead
        t = int(name[4:])
        assert np.all(out[1][:, :4] // 128 == t)
    if name == "near" and k == 100:
        # the winners are far down the positive ranking: with w = 1 the reference's top 100 reach down to places
        # 3 593 .. 6 805 of it over these requests (5 396 for request 0), so no re-sort of a finished list of a
        # thousand finds them
        for g in np.nonzero(w == 1.0)[0]:
            best = (exs[E * g: E * g + 3].astype(np.float64) @ big["cs"].astype(np.float64).T).max(axis=0)
            rank = np.empty(n, np.int64)
            rank[np.argsort(-best)] = np.arange(n)
            assert rank[out[1][g]].max() > 3000, g
    out1 = run(N, ed, sign, w, big["cd"], n, d, k, alive, dbg=1)
    for a, b in zip(out, out1):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 4. exactly representable data
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_integer_data_bit_exact_with_heavy_ties(N, dt):
    """rows and examples in {-2..2}/8 on 4 columns, weights in {0, 0.5, 1}: every product and sum is exact in float32, so
    scores, rows (ties -> the lower row) and every explain output (ties -> the lower slot) equal the reference bit for
    bit"""
    n, R_, d, k = 1000, 100, 384, 100
    g = np.random.default_rng(5)
    c = np.zeros((n, d), np.float32)
    c[:, :4] = g.integers(-2, 3, (n, 4)) / 8
    pos, neg = [], []
    for i in range(R_):
        p, m = COUNTS[i % len(COUNTS)]
        v = np.zeros((p + m, d), np.float32)
        v[:, :4] = g.integers(-2, 3, (p + m, 4)) / 8
        pos.append(v[:p])
        neg.append(v[p:])
    ex, sign = R.pack(pos, neg, d)
    w = g.choice(np.array([0, 0.5, 1], np.float32), R_)
    cd, cs = to_dev(N, c, DT[dt])
    ed, exs = to_dev(N, ex, DT[dt])
    out = run(N, ed, sign, w, cd, n, d, k)
    want = R.recommend_topk(exs, sign, w, cs, k)
    for a, b in zip(out, want):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 5. overflow
def test_overflow_rerun_of_every_request(N):
    """256 candidate slots for 1000 rows and no threshold (n is below the real capacity): every request overflows and is
    produced again alone"""
    n, d, k, R_ = 1000, 384, 21, 11
    alive = np.random.default_rng(53).random(n) > 0.03
    cd, cs = to_dev(N, unit_rows(n, d, 51), torch.bfloat16)
    ex, sign, w = requests(R_, d, 52, rows=cs)
    ed, exs = to_dev(N, ex, torch.bfloat16)
    out = run(N, ed, sign, w, cd, n, d, k, alive, cap=256)
    es, er, *_ = R.recommend_topk(exs, sign, w, cs, k, alive)
    check(out[0], out[1], es, er, w)
    check_explain(out, exs, sign, cs)
    out0 = run(N, ed, sign, w, cd, n, d, k, alive)
    for a, b in zip(out, out0):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 6. position independence
def test_a_request_does_not_depend_on_where_it_sits(N):
    n, R_, d, k = 1000, 100, 384, 20
    cd, cs = to_dev(N, unit_rows(n, d, 44), torch.float16)
    ex, sign, w = requests(R_, d, 45, rows=cs)
    ed, _ = to_dev(N, ex, torch.float16)
    sign_d, w_d = torch.from_numpy(sign).to("cuda"), torch.from_numpy(w).to("cuda")
    out = run(N, ed, sign_d, w_d, cd, n, d, k)
    for g in range(R_):                  # alone: its 16 example rows as a batch of one
        one = run(N, ed[E * g: E * (g + 1)].contiguous(), sign_d[E * g: E * (g + 1)].contiguous(),
                  w_d[g: g + 1].contiguous(), cd, n, d, k)
        for a, b in zip(one, out):
            assert np.array_equal(a[0], b[g]), g
    # request 4 (5 positives, 11 negatives) at slot 0, slot 7 and in the second example tile
    src = 4
    assert COUNTS[src % len(COUNTS)] == (5, 11)
    for at in (0, 7, 8, 13):
        order = [g for g in range(14) if g != src]
        order.insert(at, src)
        idx = np.concatenate([np.arange(E * g, E * (g + 1)) for g in order])
        moved = run(N, ed[torch.from_numpy(idx).to("cuda")].contiguous(), sign[idx], w[order], cd, n, d, k)
        for a, b in zip(moved, out):
            assert np.array_equal(a[at], b[src]), at
    # the examples of a request permuted among its 16 slots: the same bits, and the slots follow
    perm = np.random.default_rng(46).permutation(E)         # new slot j holds old slot perm[j]
    idx = E * src + perm
    one = run(N, ed[torch.from_numpy(idx).to("cuda")].contiguous(), sign[idx], w[src: src + 1], cd, n, d, k)
    for j in range(4):
        assert np.array_equal(one[j][0], out[j][src])
    assert np.array_equal(perm[one[4][0]], out[4][src]) and np.array_equal(perm[one[5][0]], out[5][src])


# ---------------------------------------------------------------- 7. unused slots
@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_unused_slots_are_ignored_whatever_they_hold(N, dt):
    n, R_, d, k = 300, 17, 200, 21
    cd, cs = to_dev(N, unit_rows(n, d, 61), DT[dt])
    ex, sign, w = requests(R_, d, 62, rows=cs)
    ed, _ = to_dev(N, ex, DT[dt])
    clean = run(N, ed, sign, w, cd, n, d, k)
    unused = torch.from_numpy(np.nonzero(sign == 0)[0]).to("cuda")
    assert unused.numel() > 100
    for fill in ("huge", "rows"):
        dirty = ed.clone()
        if fill == "huge":               # large and finite: 6e4 in every logical column, alternating in sign
            dirty[unused, :d] = 6.0e4 * (1.0 - 2.0 * (torch.arange(d, device="cuda") % 2)).to(DT[dt])
        else:                            # copies of stored rows: a positive there would win every list
            dirty[unused] = cd[torch.arange(unused.numel(), device="cuda") % n]
        got = run(N, dirty, sign, w, cd, n, d, k)
        for a, b in zip(got, clean):
            assert np.array_equal(a, b), fill


# ---------------------------------------------------------------- 8. one positive, no negative
def test_one_positive_and_no_negative_is_the_plain_search(N):
    """against mmrag_boosted_topk with weight 0 on the same inputs: w = 0, so finals within 1e-4 and sets with 2e-4 (the
    operands are swapped in the tile body: bit-equality is not demanded)"""
    n, B, d, k = 1000, 130, 384, 20
    alive = np.random.default_rng(71).random(n) > 0.03
    cd, _ = to_dev(N, unit_rows(n, d, 72), torch.float16)
    q = unit_rows(B, d, 73)
    qd, qs = to_dev(N, q, torch.float16)
    ex, sign = R.pack([q[b: b + 1] for b in range(B)], None, d)
    ed, _ = to_dev(N, ex, torch.float16)
    out = run(N, ed, sign, 0.0, cd, n, d, k, alive)
    bs, br, _ = N.boosted_topk(qd, cd, n, d, k, np.zeros(n, np.float32), 0.0, alive_bits=bits_of(alive))
    check(out[0], out[1], bs.cpu().numpy(), br.cpu().numpy(), 0.0)
    assert np.all(out[3] == 0) and np.all(out[5] == -1) and np.all(out[4][out[1] >= 0] == 0)
    assert np.all(np.abs(out[2] - out[0]) <= TOL)       # pos, recomputed, against the final


# ---------------------------------------------------------------- 9. alive bits, row offset, nothing to return, refusals
def test_alive_bits_row_offset_and_an_all_dead_collection(N):
    n, R_, d, k = 300, 3, 8, 5
    cd, cs = to_dev(N, unit_rows(n, d, 81), torch.float32)
    ex, sign, w = requests(R_, d, 82, rows=cs, counts=[(2, 3), (1, 0), (16, 0)])
    ed, exs = to_dev(N, ex, torch.float32)
    alive = np.ones(n, bool)
    alive[:29] = False
    alive[125:135] = False
    for a in (None, alive):
        out = run(N, ed, sign, w, cd, n, d, k, a, row_offset=10 ** 10)
        es, er, *_ = R.recommend_topk(exs, sign, w, cs, k, a, row_offset=10 ** 10)
        check(out[0], out[1], es, er, w)
        check_explain(out, exs, sign, cs, row_offset=10 ** 10)
    r = out[1]
    assert r.min() >= 10 ** 10 + 29 and not np.any((r >= 10 ** 10 + 125) & (r < 10 ** 10 + 135))
    for out in (run(N, ed, sign, w, cd, n, d, k, np.zeros(n, bool)), run(N, ed, sign, w, cd, 0, d, k)):
        s, r, pos, neg, pa, na = out
        assert np.all(np.isneginf(s)) and np.all(r == -1) and np.all(pos == 0) and np.all(neg == 0)
        assert np.all(pa == -1) and np.all(na == -1)


def test_wrapper_checks_launch_nothing(N, monkeypatch):
    cd, _ = to_dev(N, unit_rows(10, 8, 1), torch.float16)
    ex, sign, w = requests(2, 8, 2, counts=[(2, 3), (1, 0)])
    ed, _ = to_dev(N, ex, torch.float16)
    calls = []
    monkeypatch.setattr(N.lib(), "mmrag_internal_recommend_topk_ex", lambda *a: calls.append(a) or 0)
    no_pos, two = sign.copy(), sign.copy()
    no_pos[E:] = 0
    no_pos[E + 3] = -1
    two[1] = 2
    for s_, w_, k in ((no_pos, w, 3), (two, w, 3), (sign[:-1], w, 3), (sign, [1.0, float("nan")], 3),
                      (sign, [1.0, np.inf], 3), (sign, [0.5, -0.1], 3), (sign, [1.0, 1.0, 1.0], 3), (sign, w, 0),
                      (sign, w, 4097), (torch.zeros(31, dtype=torch.int8, device="cuda"), w, 3),
                      (sign, torch.zeros(3, device="cuda"), 3),
                      # device tensors are checked as well
                      (torch.from_numpy(no_pos).to("cuda"), w, 3), (torch.from_numpy(two).to("cuda"), w, 3),
                      (sign, torch.tensor([0.5, -0.1], device="cuda"), 3),
                      (sign, torch.tensor([0.5, float("nan")], device="cuda"), 3)):
        with pytest.raises(ValueError):
            N.recommend_topk(ed, s_, w_, cd, 10, 8, k)
    with pytest.raises(ValueError):
        N.recommend_topk(ed[:31].contiguous(), sign, w, cd, 10, 8, 3)
    assert calls == []
    N.recommend_topk(ed, sign, w, cd, 10, 8, 3)
    N.recommend_topk(ed, torch.from_numpy(sign).to("cuda"), np.float32(0.5), cd, 10, 8, 3)     # a 0-d weight: every request's
    N.recommend_topk(ed, torch.from_numpy(sign).to("cuda"), torch.tensor(0.5), cd, 10, 8, 3)
    assert len(calls) == 3


# ---------------------------------------------------------------- 10. VectorIndex
def make_index(rows, dtype=torch.float16, **kw):
    from multimodal_rag_amd.index import VectorIndex

    n, d = rows.shape
    idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=256, **kw)
    idx.add(rows, documents=[f"text {i}" for i in range(n)], metadatas=[{"parity": i % 2} for i in range(n)],
            ids=[f"id{i}" for i in range(n)])
    return idx


def index_requests(rows, d, seed, named):
    """6 requests over the stored rows `named` (original numbers) and fresh vectors: ids and vectors mixed"""
    g = np.random.default_rng(seed)
    v = unit_rows(12, d, seed + 1)
    near = rows[named[6]] + 0.3 * v[11]
    near /= np.linalg.norm(near)
    pos = [[f"id{named[0]}"], [v[0], f"id{named[1]}", v[1]], [v[2]], [f"id{named[2]}", f"id{named[3]}"], [near],
           [f"id{named[6]}"] + [v[3 + j] for j in range(5)]]
    neg = [None, [f"id{named[4]}", v[8]], [v[9], f"id{named[5]}"], [], [f"id{named[6]}"],
           [f"id{named[7 + j]}" for j in range(10)]]
    w = [1.0, 0.5, 1.0, 0.25, 1.0, float(g.uniform(0.0, 1.0))]
    return pos, neg, w


def assert_index_equals_reference(idx, pos, neg, w, k, ids, rows16, where_mask=None, where=None, exclude=True):
    """recommend_query against the reference over the surviving rows `ids` (original numbers, in row order)"""
    res = idx.recommend_query(pos, neg, n_results=k, negative_weight=w, where=where, exclude_examples=exclude)
    d = rows16.shape[1]

    def vec(e):
        return rows16[int(e[2:])] if isinstance(e, str) else np.asarray(e, np.float32).astype(np.float16).astype(np.float32)

    R_ = len(pos)
    s = np.full((R_, k), -np.inf, np.float32)
    r = np.full((R_, k), -1, np.int64)
    es, er = s.copy(), r.copy()
    local = {int(o): i for i, o in enumerate(ids)}
    for g in range(R_):
        p_ent, n_ent = list(pos[g]), list(neg[g] or [])
        ex, sign = R.pack([[vec(e) for e in p_ent]], [[vec(e) for e in n_ent]], d)
        live = np.ones(len(ids), bool) if where_mask is None else where_mask[ids].copy()
        if exclude:
            for e in p_ent + n_ent:
                if isinstance(e, str):
                    live[local[int(e[2:])]] = False
        es[g], er[g], *_ = R.recommend_topk(ex, sign, w[g], rows16[ids], k, live)
        m = len(res["ids"][g])
        assert m == len(res["scores"][g]) == len(res["penalties"][g]) == len(res["distances"][g]) \
            == len(res["matched"][g]) == len(res["repelled_by"][g]) == len(res["metadatas"][g])
        got = [int(x[2:]) for x in res["ids"][g]]
        s[g, :m] = res["scores"][g]
        r[g, :m] = [local[o] for o in got]
        pd = np.stack([vec(e) for e in p_ent]).astype(np.float64) @ rows16[got].astype(np.float64).T
        assert np.all(np.abs((1.0 - np.array(res["distances"][g])) - pd.max(axis=0)) <= TOL)
        names = [e if isinstance(e, str) else f"vector:{j}" for j, e in enumerate(p_ent)]
        for j, name in enumerate(res["matched"][g]):
            assert pd[names.index(name), j] >= pd[:, j].max() - 2 * TOL
        if n_ent:
            nd = np.stack([vec(e) for e in n_ent]).astype(np.float64) @ rows16[got].astype(np.float64).T
            best = nd.max(axis=0)
            assert np.all(np.abs(np.array(res["penalties"][g]) - w[g] * np.maximum(best, 0.0)) <= w[g] * TOL + 1e-7)
            names = [e if isinstance(e, str) else f"vector:{j}" for j, e in enumerate(n_ent)]
            for j, name in enumerate(res["repelled_by"][g]):
                if abs(best[j]) > TOL:
                    assert (name is None) == (best[j] < 0)
                if name is not None:
                    assert nd[names.index(name), j] >= best[j] - 2 * TOL
        else:
            assert res["penalties"][g] == [0.0] * m and res["repelled_by"][g] == [None] * m
        assert res["metadatas"][g] == [{"parity": o % 2} for o in got]
    check(s, r, es, er, np.asarray(w, np.float32))
    return res


def test_index_recommend_query_through_add_delete_compact(N):
    d, n, k = 384, 1500, 8
    rows = unit_rows(n, d, 301)
    rows16 = rows.astype(np.float16).astype(np.float32)
    idx = make_index(rows)
    named = list(range(100, 1500, 80))                     # 18 stored rows used as examples
    pos, neg, w = index_requests(rows16, d, 302, named)
    ids = np.arange(n)
    res = assert_index_equals_reference(idx, pos, neg, w, k, ids, rows16)
    for g in range(len(pos)):                               # the stored rows a request names are not returned
        assert not {e for e in pos[g] + list(neg[g] or []) if isinstance(e, str)} & set(res["ids"][g])
    assert res["matched"][0] == [f"id{named[0]}"] * k
    # the examples themselves are returned first when they are not excluded
    res = assert_index_equals_reference(idx, pos, neg, w, k, ids, rows16, exclude=False)
    assert res["ids"][0][0] == f"id{named[0]}" and abs(res["scores"][0][0] - 1.0) <= TOL
    assert set(res["ids"][3][:2]) == {f"id{named[2]}", f"id{named[3]}"}
    # the device tensors of recommend_search
    out = idx.recommend_search(pos, neg, n_results=k, negative_weight=w)
    assert [tuple(t.shape) for t in out] == [(6, k)] * 6 and out[1].dtype == torch.int64 and out[4].dtype == torch.int32
    assert int(out[1][0, 0]) == named[0]                   # not excluded here
    # where
    even = np.arange(n) % 2 == 0
    res = assert_index_equals_reference(idx, pos, neg, w, k, ids, rows16, even, where={"parity": 0})
    assert all(m["parity"] == 0 for hits in res["metadatas"] for m in hits)
    # grow, delete, compact: the examples are looked up where the rows are now
    more = unit_rows(400, d, 303)
    idx.add(more, documents=[f"text {n + i}" for i in range(400)], metadatas=[{"parity": (n + i) % 2} for i in range(400)],
            ids=[f"id{n + i}" for i in range(400)])
    rows16 = np.concatenate([rows16, more.astype(np.float16).astype(np.float32)])
    ids = np.arange(n + 400)
    assert_index_equals_reference(idx, pos, neg, w, k, ids, rows16)
    g = np.random.default_rng(304)
    gone = g.choice(np.setdiff1d(ids, named), 300, replace=False)
    idx.delete(ids=[f"id{i}" for i in gone])
    alive = np.ones(n + 400, bool)
    alive[gone] = False
    assert_index_equals_reference(idx, pos, neg, w, k, ids, rows16, alive)
    idx.compact()
    ids = np.nonzero(alive)[0]
    assert_index_equals_reference(idx, pos, neg, w, k, ids, rows16)
    # refusals: an unknown id, a deleted id, too deep, too many examples, no positive, a bad weight
    idx.delete(ids=[f"id{named[5]}"])
    for bad_pos, bad_neg, kw in (([["nobody"]], None, {}), ([[f"id{gone[0]}"]], None, {}),
                                 ([[f"id{named[0]}"]], [[f"id{named[5]}"]], {}),
                                 ([[f"id{named[0]}"]], None, {"n_results": 5000}),
                                 ([[f"id{named[0]}"] * 17], None, {}), ([[]], [[f"id{named[0]}"]], {}),
                                 ([[f"id{named[0]}"]], None, {"negative_weight": -1.0}),
                                 ([[2.0 * rows[0]]], None, {}),
                                 ([f"id{named[0]}"], None, {}),          # an id where a request's list belongs
                                 (f"id{named[0]}", None, {}), ([[f"id{named[0]}"]], [f"id{named[1]}"], {}),
                                 ([[7]], None, {}), ([[f"id{named[0]}"]], [[np.int64(7)]], {}),   # a row number
                                 ([[rows[:2]]], None, {})):
        with pytest.raises(ValueError):
            idx.recommend_query(bad_pos, bad_neg, **kw)


def test_index_f8_collection_runs_on_its_plane(N):
    from multimodal_rag_amd.index import VectorIndex

    d, n, k = 384, 800, 6
    rows = unit_rows(n, d, 322)
    pos, neg, w = index_requests(rows, d, 323, list(range(10, 800, 40)))
    out = []
    for dtype, kw in ((torch.float16, {}), (torch.float8_e4m3fn, {"rescore_dtype": torch.float16})):
        idx = VectorIndex(dim=d, dtype=dtype, device="cuda:0", capacity=256, **kw)
        idx.add(rows, ids=[f"id{i}" for i in range(n)])
        out.append(idx.recommend_query(pos, neg, n_results=k, negative_weight=w))
    for key in ("ids", "scores", "distances", "penalties", "matched", "repelled_by"):
        assert out[0][key] == out[1][key], key
    lean = VectorIndex(dim=d, dtype=torch.float8_e4m3fn, device="cuda:0", capacity=256, rescore_dtype=None)
    lean.add(rows, ids=[f"id{i}" for i in range(n)])
    with pytest.raises(ValueError, match="MMRAG_F8_RESCORE=none"):
        lean.recommend_query(pos, neg, n_results=k)


# ---------------------------------------------------------------- 11. manager and dispatcher on the HIP engine
def test_manager_and_dispatcher_share_one_launch(N, monkeypatch):
    from multimodal_rag_amd import config
    from multimodal_rag_amd import index as index_mod
    from multimodal_rag_amd.embedder import EmbeddingManager

    monkeypatch.setattr(config.settings, "MMRAG_DEDUP_THRESHOLD", 0.0)
    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_recommend()
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình"]
    texts = [f"{words[i % 12]} {words[(i * 5 + 1) % 12]} {words[(i * 7 + 2) % 12]} {i}" for i in range(40)]
    asyncio.run(m.embed_and_store([{"id": str(i), "type": "text", "summary": t} for i, t in enumerate(texts)], "a"))
    calls = [dict(query_text=texts[i], like=[f"a_{(i + 1) % 40}"][: i % 2], unlike=[f"a_{(3 * i + 2) % 40}"][: (i // 2) % 2],
                  unlike_texts=[texts[(i + 7) % 40]][: (i // 4) % 2], negative_weight=[None, 0.5][i % 2]) for i in range(15)]
    calls.append(dict(like=["a_3", "a_4"], unlike=["a_5"]))                    # no question
    solo = [asyncio.run(m.recommend(n_results=4, **c)) for c in calls]
    for c, res in zip(calls, solo):
        named = set(c.get("like", [])) | set(c.get("unlike", []))
        assert len(res["ids"]) == 4 and not named & set(res["ids"])
        assert res["scores"] == sorted(res["scores"], reverse=True)
        assert all(abs(sc - (1.0 - dist) + pen) <= 2e-4 for sc, dist, pen in
                   zip(res["scores"], res["distances"], res["penalties"]))
        assert all(x == "query" or x in c.get("like", []) for x in res["matched"])
        assert all(x is None or x in c.get("unlike", []) + c.get("unlike_texts", []) for x in res["repelled_by"])
        assert all((pen > 0) == (x is not None) for pen, x in zip(res["penalties"], res["repelled_by"]))
    # the question alone is the plain query
    plain = asyncio.run(m.query(texts[0], n_results=4))
    assert set(solo[0]["ids"]) == set(plain["ids"]) and calls[0]["like"] == [] and calls[0]["unlike"] == []
    with pytest.raises(ValueError, match="Item not found"):
        asyncio.run(m.recommend("học máy", like=["a_999"]))

    count = {"search": 0, "encode": 0}
    real, real_embed = index_mod._native.recommend_topk, m._embed
    monkeypatch.setattr(index_mod._native, "recommend_topk",
                        lambda *a, **kw: (count.__setitem__("search", count["search"] + 1), real(*a, **kw))[1])
    monkeypatch.setattr(m, "_embed", lambda *a, **kw: (count.__setitem__("encode", count["encode"] + 1),
                                                        real_embed(*a, **kw))[1])

    async def go():
        disp = m.enable_dynamic_batching(max_batch=64, max_wait_ms=200.0)
        try:
            assert disp.recommend_fn is not None
            out = await asyncio.gather(*[m.recommend(n_results=4, **c) for c in calls])
            stats = dict(disp.stats)
            with pytest.raises(ValueError, match="Item not found"):
                await m.recommend("học máy", like=["a_999"])
        finally:
            await disp.stop()
            m._dispatcher = None
        return out, stats

    out, stats = asyncio.run(go())
    assert count == {"search": 1, "encode": 1} and stats["batches"] == 1 and stats["max_batch_seen"] == 16, (count, stats)
    for res, alone in zip(out, solo):
        for key in ("ids", "scores", "distances", "penalties", "matched", "repelled_by"):
            assert res[key] == alone[key], key
    asyncio.run(m.cleanup())


# ---------------------------------------------------------------- 12. the endpoints on the HIP engine
def test_query_endpoint_not_and_recommend_endpoint(N):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd.server import create_app

    senses = {"animal": "The jaguar is a large cat of the rainforest. The jaguar hunts deer and swims in jungle rivers.",
              "car": "The Jaguar is a British luxury car. The Jaguar has a powerful engine and leather seats."}
    with TestClient(create_app()) as c:
        doc_of = {}
        for sense, body in senses.items():
            r = c.post("/upload", files={"file": (f"{sense}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
            doc_of[r.json()["doc_id"]] = sense
        r = c.post("/upload", files={"file": ("other.txt", "Bảng và ảnh. GPU kernel và dữ liệu. ".encode() * 3,
                                              "text/plain")})
        assert r.status_code == 200, r.text

        def sense_of(source):
            return next((s for doc, s in doc_of.items() if source["doc_id"].startswith(doc)), None)

        before = c.post("/query", json={"query": "jaguar", "top_k": 3})
        assert before.status_code == 200, before.text
        top = sense_of(before.json()["sources"][0])
        assert top in senses
        r = c.post("/query", json={"query": "jaguar", "top_k": 3, "not": [senses[top]]})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert set(src[0]) == set(before.json()["sources"][0]) | {"score", "penalty", "matched", "repelled_by"}
        assert sense_of(src[0]) != top                      # the unwanted sense's document leaves the top source
        unwanted = [s for s in src if sense_of(s) == top]
        assert all(s["repelled_by"] == senses[top] and s["penalty"] > 0 for s in unwanted)
        assert [s["score"] for s in src] == sorted((s["score"] for s in src), reverse=True)
        assert all(s["matched"] == "query" for s in src) and r.json()["answer"]
        after = c.post("/query", json={"query": "jaguar", "top_k": 3})
        assert after.json()["sources"] == before.json()["sources"] and after.json()["answer"] == before.json()["answer"]
        # the "more like this" button: sources, no answer; the item itself is not returned
        me = before.json()["sources"][0]["doc_id"]
        r = c.post("/recommend", json={"like": [me], "top_k": 2})
        assert r.status_code == 200, r.text
        assert set(r.json()) == {"sources", "processing_time"} and 1 <= len(r.json()["sources"]) <= 2
        assert all(s["doc_id"] != me and s["matched"] == me and s["repelled_by"] is None for s in r.json()["sources"])
        r = c.post("/recommend", json={"like": ["nobody"]})
        assert r.status_code == 400 and "Item not found" in r.json()["detail"]
        for extra in ({"mmr": True}, {"hybrid": True}, {"group_by_document": True}, {"boost": {"recency": 0.3}},
                      {"variants": ["leopard"]}, {"doc_ids": ["x"]}):
            r = c.post("/query", json={"query": "jaguar", "not": ["car"], **extra})
            assert r.status_code == 400 and "not combined" in r.json()["detail"], extra
