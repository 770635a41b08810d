"""CPU: the data of tests/test_scan_regimes_gpu.py proved before a GPU sees it -- each kernel's own reference
(tests/*_ref.py) in its neutral configuration gives the plain search's answer on every lattice regime, the planted tile
layouts lie where their names say relative to the bound stages' samples, the restated plan gives the stages the rows of
the GPU file are named after, and the sparse-sample filter never shows a sample k visible rows."""
import numpy as np
import pytest

import regime_ref as R
import scan_regimes as S

N_SHORT = 4099
K = 5
B = 7



@pytest.mark.parametrize("regime", R.SCAN_LATTICE)
@pytest.mark.parametrize("kernel", S.KERNELS)
def test_neutral_reference_is_the_plain_search(kernel, regime):
    d = S.data(regime, N_SHORT, K)
    q, c, alive, es, er = d.q[:B], d.c, d.alive, d.es[:B], d.er[:B]
    assert np.isfinite(es).all() and (er >= 0).all()
    if kernel == "scoped":
        s, r = S.scoped_reference(q, c, K, alive, biting=False)
    elif kernel == "filtered":
        s, r = S.filtered_reference(q, c, K, d.stages, alive, biting=False)
    elif kernel == "range":
        thr = S.range_thresholds(q, c, es, "floor")
        counts, facets, s, r = S.range_reference(q, c, K, thr, alive)
        live = S.live_of(alive, N_SHORT)
        assert np.array_equal(counts, np.full(B, live.sum()))
        assert np.array_equal(facets, np.tile(np.bincount(S.facet_codes(N_SHORT)[live], minlength=S.FACET_G + 1), (B, 1)))
    elif kernel == "boosted":
        s, r, boosts = S.boosted_reference(q, c, K, S.neutral_prior(N_SHORT), 0.0, alive)
        assert not boosts.any()
    elif kernel == "recommend":
        s, r, pos, neg, pa, na = S.recommend_reference(q, c, K, alive, biting=False)
        assert np.array_equal(pos, es) and not neg.any() and (na == -1).all()
        assert np.array_equal(pa, np.tile(S.recommend_slots(B)[0][:, None], (1, K)))
    else:
        sim, grp, cov, best, best_row = S.related_reference(q, c, K, alive, 0.0, biting=False)
        s, r = sim, grp.astype(np.int64)
        assert np.array_equal(best, es) and np.array_equal(best_row, er) and np.array_equal(cov, (es >= 0).astype(np.int32))
    assert np.array_equal(r, er), (kernel, regime)
    assert np.array_equal(s, es), (kernel, regime)


def test_recommend_biting_reference_is_the_clamped_difference():
    """negative = the positive, weight 1: final = pos - max(pos, 0)"""
    for regime in ("negative", "plateau", "rising"):
        d = S.data(regime, N_SHORT, K)
        q = d.q[:B]
        s, r, pos, neg, pa, na = S.recommend_reference(q, d.c, K, d.alive, biting=True)
        assert np.array_equal(pos, neg) and np.array_equal(s, pos - np.maximum(pos, 0))
        assert np.array_equal(pa, np.tile(S.recommend_slots(B)[0][:, None], (1, K)))
        assert np.array_equal(na, np.tile(S.recommend_slots(B)[1][:, None], (1, K)))
        if regime == "negative":
            assert np.array_equal(s, d.es[:B]) and np.array_equal(r, d.er[:B])


PLAN_CASES = [(4099, 5, (16384, [])), (20000, 5, (16384, [96])), (20000, 100, (16384, [96])),
              (140000, 512, (16384, [96, 137]))]


@pytest.mark.parametrize("n,k,want", PLAN_CASES)
def test_bound_plan(n, k, want):
    assert R.bound_plan(n, k) == want
    assert R.bound_plan(n, k, cap=256) == (256, want[1])           # fewer slots, the same stages
    assert R.bound_plan(n, k, no_bound=True) == (16384, [])


def test_library_plan_is_the_restated_plan():
    """mmrag_internal_bound_plan (host code: no GPU) against regime_ref.bound_plan, over the thresholds of the rule"""
    from multimodal_rag_amd import _native as N

    for k in (1, 5, 100, 512, 513, 4096):
        C = R.candidate_capacity(k)
        assert N.candidate_capacity(k) == C
        for n in (0, 1, 100, 4099, C, C + 1, 20000, 140000, 400000, 786000, 3000000, 2 ** 31 - 1):
            for cap in (0, 256, C, C + 1):
                assert N.bound_plan(n, k, cap, 0) == R.bound_plan(n, k, cap), (n, k, cap)
                assert N.bound_plan(n, k, cap, 1) == R.bound_plan(n, k, cap, no_bound=True) == (min(cap, C) or C, [])


def test_bound_plan_needs_many_rows_for_a_second_stage():
    """what the regime rows are sized by: k <= 100 has one stage below 400 000 rows, k = 512 three from 786 000 on"""
    assert all(len(R.bound_plan(n, k)[1]) == 1 for k in (5, 100) for n in (16385, 100000, 399999))
    assert len(R.bound_plan(786000, 512)[1]) == 2 and len(R.bound_plan(900000, 512)[1]) == 3


def test_sample_tiles():
    for n, stages in ((20000, [96]), (140000, [96, 137])):
        T = -(-n // 128)
        tiles = R.sample_tiles(n, stages)
        assert 0 in tiles and T - 1 not in tiles and max(tiles) < T
        assert len(R.sample_tiles(n, stages[:1])) == stages[0]
        assert R.sample_tiles(n, [T]) == set(range(T))


@pytest.mark.parametrize("n,k", [(20000, 5), (140000, 512)])
def test_planted_tile_layouts(n, k):
    stages = R.bound_plan(n, k)[1]
    T = -(-n // 128)
    every, first = R.sample_tiles(n, stages), R.sample_tiles(n, stages[:1])
    rows, levels = R.planted_tile_layout("unsampled", n, k, stages)
    assert rows.size == k + 3 and np.unique(levels).size == k + 3
    assert not set((rows // 128).tolist()) & every
    assert n - 1 in rows and (T - 1) * 128 in rows
    assert any(r % 128 == 0 and r // 128 - 1 in every for r in rows.tolist())
    rows, levels = R.planted_tile_layout("sampled", n, k, stages)
    assert rows.size == k + 3
    order = np.lexsort((rows, -levels))                 # the answer's order: level descending, then the lower row
    kth, next_ = order[k - 1], order[k]
    assert levels[kth] == levels[next_] and np.sum(levels == levels[kth]) == 2 and np.sum(levels > levels[kth]) == k - 1
    assert rows[next_] // 128 == T - 1 and rows[next_] == rows.max()
    assert set((np.delete(rows, next_) // 128).tolist()) <= first
    if k <= R.ONE_LANE_MAX_K:
        rows, levels = R.planted_tile_layout("one_lane", n, k, stages)
        assert rows.size == k + 3
        in_tile = rows % 128
        assert np.unique(rows // 128).size == 1 and np.unique(in_tile // 64).size == 1 and np.unique(in_tile % 16 // 4).size == 1
        assert set(rows.tolist()) <= set(R.lane_rows(int(rows[0] // 128), int(in_tile[0] // 64), int(in_tile[0] % 16 // 4)).tolist())
    rows, levels = R.planted_tile_layout("one_pair_tile", n, k, stages)
    assert rows.size == min(k + 3, 128) and np.unique(rows // 128).size == 1 and np.unique(rows % 128 // 64).size == 2


@pytest.mark.parametrize("where", R.PLANTED_TILES)
def test_planted_rows_are_the_answer(where):
    """every planted row outscores the background for every query, in the order of the levels, the lower row first"""
    n, k = 20000, 5
    d = S.data("planted:" + where, n, k)
    rows, levels = R.planted_tile_layout(where, n, k, list(d.stages))
    want = rows[np.lexsort((rows, -levels))][:k]
    assert np.array_equal(d.er, np.tile(want, (S.B_MAX, 1))) and (d.es > 0).all()


def test_boosted_only_generators():
    n = N_SHORT
    q, c, prior, w = R.cancelled(n, B)
    assert not ((q @ c.T) + w[:, None] * prior[None, :]).any() and set(w.tolist()) <= {1.0, 2.0}
    q, c, prior, w = R.prior_only(n, B)
    dots = q @ c.T
    assert (dots == dots[:, :1]).all() and set(w.tolist()) == {-1.0, 0.0, 1.0, 2.0}
    assert np.array_equal(prior, (np.arange(n) // 32).astype(np.float32))
    s, r, _ = S.boosted_reference(q, c, K, prior, w, None)
    assert np.array_equal(r[0], np.arange(K)) and np.array_equal(r[1], np.arange(K))        # falling, plateau
    assert np.array_equal(r[2], np.lexsort((np.arange(n), -prior))[:K]) and r[2][0] == (n - 1) // 32 * 32     # rising


@pytest.mark.parametrize("n,k", [(20000, 5), (20000, 100), (140000, 512)])
def test_sparse_filter_never_shows_a_sample_k_rows(n, k):
    stages = R.bound_plan(n, k)[1]
    vis = S.sparse_filter(n, k, stages)
    sampled = np.isin(np.arange(n) // 128, sorted(R.sample_tiles(n, stages)))
    assert 0 < (vis & sampled).sum() < k and vis.sum() >= k + 3
    for regime in ("negative_with_zero_rows",):         # the filters the GPU sees carry the alive bits too
        d = S.data(regime, n, k)
        both = S.filters_of(n, k, stages, d.alive, biting=True)
        assert (both[1] & sampled).sum() < k and both[1].sum() >= k + 3 and not (both & ~d.alive[None, :]).any()


def test_bitmap_words():
    vis = np.zeros((2, 100), bool)
    vis[0, [0, 31, 32, 99]] = True
    w = S.bitmap_words(vis, 4)
    assert w.shape == (2, 4) and w[0, 0] == 0x80000001 and w[0, 1] == 1 and w[0, 3] == 0xfffffff8 and w[1, 3] == 0xfffffff0
    assert np.array_equal(S.bitmap_words(vis, 4, ones_past_n=False)[1], np.zeros(4, np.uint32))


def test_cases_cover_every_kernel_and_row():
    assert {c[0] for c in S.CASES} == set(S.KERNELS)
    assert {c[1] for c in S.CASES if c[0] == "boosted"} == set(S.ROWS)
    assert {c[1] for c in S.CASES if c[0] == "related"} == {"short", "tiny"}
    assert not [c for c in S.CASES if c[2].split(":")[-1] in ("one_walker", "tail", "sample_edge", "one_slab_ring_tile")]
