"""CPU: the generators of tests/regime_ref.py and their expected answers, before any kernel is involved.

For every generator, at a few thousand rows and full d: the oracle on the support columns equals the oracle on the full
matrix bit for bit, and the regime's precondition holds (what makes it the regime it claims to be)."""
import numpy as np
import pytest

import regime_ref as R
from oracle import search_oracle as O

C = 4                      # a small planning CU count: the sample pre-pass ends at row 1024, a walker's tiles are 256 rows apart
N = 12 * 64 * C + 5        # 3077 rows, ragged
B = 70
SHAPES = [(100, 2), (384, 2), (64, 4), (130, 1)]   # (d, element bytes)


def scores_of(q, c):
    return q.astype(np.float64) @ c.astype(np.float64).T


@pytest.mark.parametrize("d,esize", SHAPES + [(64, 2), (512, 2), (768, 4)])
def test_support_columns(d, esize):
    cols = R.support(d, esize)
    per = 128 // esize
    assert cols.size == 16 == np.unique(cols).size and cols[0] == 0 and cols[-1] == d - 1
    assert np.sum(cols >= d - R.PARKED) >= 4
    if per < d:
        assert per - 1 in cols and per in cols                      # both sides of a 128-byte slab boundary
    assert set(cols) <= set(R.band_columns(d, esize)) and set(range(d - 32, d)) <= set(R.band_columns(d, esize))


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("k", [5, 20])
def test_support_only_oracle_equals_full_oracle(regime, k):
    for d, esize in SHAPES[:2] if regime == "band" else SHAPES:
        f8 = esize == 1
        n = 187 if f8 and regime in ("rising", "falling") else N
        cols = R.band_columns(d, esize) if regime == "band" else R.support(d, esize)
        q, c, alive = R.make(regime, n, B, k, C, f8=f8, ncols=cols.size)
        es, er = R.expected(q, c, k, alive)
        fs, fr = O.cosine_topk(R.expand(q, cols, d), R.expand(c, cols, d), k, alive=alive)
        if regime == "band":    # not a lattice: the full matrix sums the same products among zeros, in sgemm's order
            assert np.abs(es - fs).max() <= 1e-6 and O.same_topk_sets(er, es, fr, fs, margin=2e-6)
        else:
            assert np.array_equal(es, fs) and np.array_equal(er, fr)
            assert np.array_equal(q, np.round(q)) and np.array_equal(c, np.round(c))
            assert np.abs(q).max() <= (2 if f8 else 256) and np.abs(c).max() <= (2 if f8 else 127)
            assert np.abs(scores_of(q, c)).max() < 2 ** 24


@pytest.mark.parametrize("k", [5, 20])
def test_negative(k):
    q, c = R.negative(N, B)
    assert scores_of(q, c).max() < 0 and c.any(axis=1).all()
    q, c = R.negative_with_zero_rows(N, B, k)
    live, dead = R.zero_rows_layout(N, k)
    alive = R.zero_rows_alive(N, k)
    assert live.size == k + 2 and 3 in live and N - 1 in live and dead.size == 5 and dead[0] < live[0]
    assert not alive[dead].any() and alive[live].all() and not c[live].any() and not c[dead].any()
    s = scores_of(q, c)
    assert (np.delete(s, np.concatenate([live, dead]), axis=1) < 0).all()
    es, er = R.expected(q, c, k, alive)
    assert np.array_equal(er, np.tile(live[:k], (B, 1))) and not es.any()          # the live zero rows, in row order
    _, masked_out = R.expected(q, c, k)                                           # without the mask a dead row wins
    assert dead[0] in masked_out[0]


@pytest.mark.parametrize("k", [5, 20])
def test_plateau(k):
    q, c = R.plateau(N, B)
    s = scores_of(q, c)
    es, er = R.expected(q, c, k)
    assert np.all((s == es[:, k - 1:k]).sum(axis=1) > 100 * k)                     # > 100 k rows tie with the k-th score
    assert np.array_equal(er, np.tile(np.arange(k), (B, 1)))
    assert len({float(x) for x in es[:, 0]}) >= 5 and (es[:, 0] < 0).any() and (es[:, 0] > 0).any()
    q, c = R.plateau(N, B, k, C, two_level=True)
    high = R.plateau_high_rows(N, k, C)
    assert high.size == k - 2 and N - 2 in high and 256 * C in high and high.min() > 1
    s = scores_of(q, c)
    es, er = R.expected(q, c, k)
    assert np.all((s == es[:, k - 1:k]).sum(axis=1) > 100 * k)
    assert np.array_equal(er, np.tile(np.concatenate([high, [0, 1]]), (B, 1)))
    assert np.array_equal(es[:, 0], es[:, k - 1] + 1)                             # one step


@pytest.mark.parametrize("falling", [False, True])
def test_rising_and_falling(falling):
    for f8, n in ((False, N), (True, 187)):
        q, c = R.rising(n, B, falling=falling, f8=f8)
        s = scores_of(q, c)
        mult = q[:, 0].astype(np.float64)
        blk = np.arange(n) // 32
        assert np.array_equal(s, mult[:, None] * (blk.max() - blk if falling else blk)[None, :])
        assert np.all(np.diff(s, axis=1) * (-1 if falling else 1) >= 0)                # monotone in the row number
        es, er = R.expected(q, c, 5)
        first = 0 if falling else (n - 1) // 32 * 32
        assert np.array_equal(er, np.tile(first + np.arange(5), (B, 1)))              # lower row first inside the block


@pytest.mark.parametrize("where", R.PLANTED)
@pytest.mark.parametrize("k", [5, 20])
def test_planted(where, k):
    rows, levels = R.planted_layout(where, N, k, C)
    q, c = R.planted(where, N, B, k, C)
    s = scores_of(q, c)
    assert (np.delete(s, rows, axis=1) < 0).all() and (s[:, rows] > 0).all()       # a negative background
    es, er = R.expected(q, c, k)
    take = min(k, rows.size)
    order = np.lexsort((rows, -levels))                                            # by level, the lower row on a tie
    assert np.array_equal(er[:, :take], np.tile(rows[order][:take], (B, 1)))       # the winners are the planted rows
    if where == "one_walker":
        assert rows.size == min(k + 3, 12) and np.all(np.diff(rows) == 64 * C)
    else:
        assert rows.size == k + 3 and np.all(np.diff(es[:, :k], axis=1) <= 0)
    if where == "one_tile":
        assert np.unique(rows // 64).size == 1
    if where == "one_slab_ring_tile":
        assert np.unique(rows // 256).size == 1 and np.unique(rows // 64).size > 1
    if where == "tail":
        assert N - 1 in rows and rows.min() >= ((N + 63) // 64 - 3 * C) * 64 and np.unique(rows // (64 * C)).size >= 3
    if where == "sample_edge":
        e = 256 * C
        assert set(range(e - 2, e + 2)) <= set(rows.tolist())
        assert np.array_equal(er[:, 1:3], np.tile([e - 5, e + 2], (B, 1))) and np.array_equal(es[:, 1], es[:, 2])
    assert R.planted_layout(where, 4099, k, C, f8=True)[0].size <= 32 or where in ("one_walker", "tail", "sample_edge")


@pytest.mark.parametrize("d,esize", SHAPES[:2])
def test_band(d, esize):
    k = 20
    q, c = R.band(N, B, R.band_columns(d, esize).size)
    assert np.allclose(np.linalg.norm(c, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(q, axis=1), 1, atol=1e-6)
    s = scores_of(q, c)
    assert R.BAND[0] < s.min() and s.max() < R.BAND[1]                             # a narrow high band, nothing near 0
    top = -np.sort(-s, axis=1)
    med = np.median(s, axis=1)
    assert np.all(top[:, 0] - top[:, k - 1] < 0.06)                                # best to k-th
    assert np.all(top[:, k - 1] - med < 0.15) and np.all(top[:, k - 1] - med > 0.02)   # k-th to median
    ns, nr = R.expected(-q, c, k)                                                  # negation: every score negative
    assert (ns < 0).all() and np.array_equal(nr[0], np.lexsort((np.arange(N), s[0]))[:k])
