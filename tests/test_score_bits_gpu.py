"""GPU: "a score's bits depend on the query row, the stored row and d alone" across the kernels that run pair_tile.h's
body, on data where the summation order matters: seeded random unit rows, not the lattice of tests/regime_ref.py.

One shape: n = 300 stored rows (two full 128-row tiles and one of 44), 130 columns (a full column tile and one of 2), and
three (dtype, d): float16 d = 96 in ld = 128 (two K-slabs, half of the second used), bfloat16 d = 64 (one slab), float32
d = 40 in ld = 64 (two slabs).  A few rows are dead through `alive` wherever an entry point takes one.  The full
[130, 300] score matrix is collected from scoped_topk (one scope of every group, k = 300), filtered_topk (an all-ones
bitmap), boosted_topk (weight 0, prior 0), range_scan (threshold -2, limit 300), related_groups (every row its own group,
130 one-vector sets) and recommend_topk (130 requests of one positive): np.array_equal between all of them.
kmeans_assign with the columns as centroids must return the matrix's row-wise maximum and its lowest arg-max, and, for
float16, maxsim_scores with one-token queries over the 300 rows as one passage its column-wise maxima.  Against the
float64 dot of the stored values the matrix is held to the 1e-4 of the per-kernel GPU files (tests/test_scoped_gpu.py
TOL)."""
import numpy as np
import pytest
import torch

from test_related_gpu import bits_of, to_dev, unit_rows
from test_scoped_gpu import TOL

pytestmark = pytest.mark.gpu

N_ROWS, N_COLS = 300, 130
DEAD = (0, 5, 127, 128, 200, 299)      # both sides of a tile edge, the first and the last row
CASES = [(torch.float16, 96), (torch.bfloat16, 64), (torch.float32, 40)]
MAX_SETS = 64


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def matrix_of(s, r, rows_expected, what):
    """[columns, n] float32 of a (scores [B, k], rows [B, k]) answer with k = n: every expected row exactly once per
    column, (-inf, -1) in the other places; NaN where a row was not expected"""
    B, k = s.shape
    assert k == N_ROWS and r.shape == s.shape, what
    m = np.full((B, N_ROWS), np.nan, np.float32)
    want = np.sort(np.asarray(rows_expected))
    for b in range(B):
        hit = r[b] >= 0
        assert np.array_equal(np.sort(r[b][hit]), want), (what, b)
        assert np.isneginf(s[b][~hit]).all(), (what, b)
        m[b, r[b][hit]] = s[b][hit]
    return m


@pytest.mark.parametrize("dtype,d", CASES)
def test_one_score_matrix(N, dtype, d):
    n, B = N_ROWS, N_COLS
    alive = np.ones(n, dtype=bool)
    alive[list(DEAD)] = False
    live = np.nonzero(alive)[0]
    every = np.arange(n)
    bits = bits_of(alive)
    cd, c_stored = to_dev(N, unit_rows(n, d, 11), dtype)
    qd, q_stored = to_dev(N, unit_rows(B, d, 12), dtype)
    ld = cd.shape[1]
    assert ld == {96: 128, 64: 64, 40: 64}[d]
    ref = q_stored.astype(np.float64) @ c_stored.astype(np.float64).T

    got = {}
    # filtered: an all-ones bitmap (bits past n too); no alive bits: every row
    W = N.filter_words(n)
    vis = torch.full((1, W), -1, dtype=torch.int32, device="cuda")
    s, r = host(*N.filtered_topk(qd, cd, n, d, n, np.zeros(B, np.int64), vis))
    got["filtered"] = matrix_of(s, r, every, "filtered")
    # range: threshold -2, every row passes; no alive bits
    counts, _, s, r = host(*N.range_scan(qd, cd, n, d, -2.0, n))
    assert np.array_equal(counts, np.full(B, n))
    got["range"] = matrix_of(s, r, every, "range")
    # scoped: 60 contiguous groups of 5 rows, one scope of them all
    col = torch.from_numpy((every // 5).astype(np.int32)).to("cuda")
    s, r = host(*N.scoped_topk(qd, cd, n, d, n, col, 60, np.zeros(B, np.int64), [0, 60], list(range(60)), n,
                               alive_bits=bits))
    got["scoped"] = matrix_of(s, r, live, "scoped")
    # boosted: weight 0, prior 0
    s, r, bo = host(*N.boosted_topk(qd, cd, n, d, n, np.zeros(n, np.float32), 0.0, alive_bits=bits))
    assert not bo.any()
    got["boosted"] = matrix_of(s, r, live, "boosted")
    # recommend: request g = column g as its one positive, in slot g % 16
    E = N.MAX_RECOMMEND_EXAMPLES
    ex = torch.zeros((E * B, ld), dtype=dtype, device="cuda")
    sign = np.zeros(E * B, np.int8)
    slot = E * np.arange(B) + np.arange(B) % E
    ex[torch.from_numpy(slot).to("cuda")] = qd
    sign[slot] = 1
    s, r, pos, neg, pa, na = host(*N.recommend_topk(ex, sign, 0.5, cd, n, d, n, alive_bits=bits))
    got["recommend"] = matrix_of(s, r, live, "recommend")
    assert not neg.any() and (na == -1).all()
    # related: every row its own group, one-vector sets, at most 64 sets per call
    own = torch.from_numpy(every.astype(np.int32)).to("cuda")
    parts = [host(*N.related_groups(qd[lo: lo + MAX_SETS], list(range(min(MAX_SETS, B - lo) + 1)), cd, n, d, n, own, n,
                                    0.0, alive_bits=bits)) for lo in range(0, B, MAX_SETS)]
    sim, grp, _, best, best_row = (np.concatenate(p) for p in zip(*parts))
    got["related"] = matrix_of(sim, grp.astype(np.int64), live, "related")
    assert np.array_equal(best, sim) and np.array_equal(best_row, grp.astype(np.int64))

    full = got["filtered"]
    assert np.isfinite(full).all()
    assert np.array_equal(got["range"], full)
    for name in ("scoped", "boosted", "recommend", "related"):
        m = got[name]
        assert np.isnan(m[:, list(DEAD)]).all(), name
        assert np.array_equal(m[:, live], full[:, live]), name
    err = float(np.abs(full.astype(np.float64) - ref).max())
    print("score matrix %s d=%d: max |score - float64| = %.3e" % (dtype, d, err))
    assert err <= TOL, err

    # kmeans_assign: the columns as centroids
    assign, score = host(*N.kmeans_assign(cd, n, d, qd, alive=bits))
    assert np.array_equal(score[live], full[:, live].max(axis=0))
    assert np.array_equal(assign[live], full[:, live].argmax(axis=0))      # numpy's argmax: the lowest index
    assert (assign[list(DEAD)] == -1).all() and np.isneginf(score[list(DEAD)]).all()

    # maxsim_scores (float16 rows, whole slabs of columns: the pad columns are zero): one-token queries, one passage
    if dtype == torch.float16:
        sums, bs, bi = host(*N.maxsim_scores(qd, cd, ld, np.arange(B), np.ones(B, np.int64), [0], [n], np.arange(B),
                                             np.zeros(B, np.int64)))
        assert np.array_equal(bs[:, 0], full.max(axis=1))
        assert np.array_equal(bi[:, 0], full.argmax(axis=1))
        assert np.array_equal(sums, full.max(axis=1))
