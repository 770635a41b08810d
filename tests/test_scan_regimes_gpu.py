"""GPU: the six kernels that run pair_tile.h's 128 x 128 body and hand candidates to candidate_select.h / deep_select.h
(csrc/scoped.hip, filtered.hip + masked_scan.h, range.hip, boosted.hip, recommend.hip, related.hip) on the score layouts
of tests/regime_ref.py: all scores negative (the zero fill of rows past n, queries past B and K padding then outscores
every real row), full plateaus and ties exactly at the bound, scores monotone in the row number, winners that no bound
sample sees / that the first sample sees all of / in the 16 rows of one lane / in one tile, samples that never hold k
visible rows.

Lattice regimes: np.array_equal, scores and rows.  In a kernel's NEUTRAL configuration the answer is the plain search's
(regime_ref.expected), in a BITING one the kernel's own reference on the support columns (tests/scan_regimes.py;
tests/test_scan_regimes_cpu.py proves both on a CPU).  `band`: each file's own check(), nothing else.

Rows (tests/scan_regimes.py ROWS) are the smallest shapes at which each path exists: no bound stage (4099 rows), one
tile with k > n (100 rows: at k = 128 the places past the live rows are (-inf, -1), boost 0), one stage (20000), two
stages -- a second scan under the first's tau, the fmaxf(tau, k-th) update of deep_select_kernel's bound mode and a main
pass under a tau raised twice -- (140000 rows at k = 512), and the same with 256 slots, where every tie overflows.
Before a shape's first call the restated plan (regime_ref.bound_plan) is asserted against the library's
(mmrag_internal_bound_plan).  A bounded row also runs without bound passes (dbg = 1) and must give the same bits; its
main pass's counters (the first 4 B bytes of the workspace, as tools/boost_bench.py reads them) show that the bound did
bite (rising, falling, planted) or that every row tied with it (plateau).

What these layouts found: on row two_stage_small_cap (256 candidate slots at k = 512) `rising` left 140000 survivors of
140000 rows for every query in all four bounded kernels, though every answer was exact.  The bound stages appended into
the 256 slots of the tests' cap, deep_select_kernel's bound mode so never held k candidates (S = min(count, slots) <
k), its `want == k` guard kept tau at -inf through both stages, and the overflow re-run the cap is there to exercise
never ran under a raised tau.  A bound stage now appends into the slots its plan was made for, candidate_capacity(k)
(csrc/candidate_select.h bound_stage_layout); the cap shrinks the main pass's slots only.  Host code; without a cap
nothing changes."""
import numpy as np
import pytest
import torch

import regime_ref as R
import scan_regimes as S
import test_boost_gpu
import test_filtered_gpu
import test_range_gpu
import test_recommend_gpu
import test_related_gpu
import test_scoped_gpu
from test_search_gpu import check as check_search
from test_search_regimes_gpu import ESIZE, N, alive_bits, upload   # noqa: F401  (N: the module's fixture)

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
BITE = ("rising", "falling")       # and every planted layout: the bound leaves fewer candidates than rows


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")      # a copy: the cached data sets are read-only


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


class Shape:
    """one (row, regime, variant): the uploaded data set and what every kernel's runner needs"""

    def __init__(self, Nn, row, regime, variant):
        self.N, self.row, self.regime = Nn, row, regime
        self.d, dt, self.k, self.B = variant
        self.dtype = DT[dt]
        self.n, self.cap = S.ROWS[row].n, S.ROWS[row].cap
        self.bounded = row in S.BOUNDED
        self.exact = regime != "band"
        n, k, B = self.n, self.k, self.B
        # the plan: restated, then the library's own
        self.slots, self.stages = R.bound_plan(n, k, self.cap)
        assert (len(self.stages) > 0) == self.bounded
        assert Nn.bound_plan(n, k, self.cap, 0) == (self.slots, self.stages), (row, variant)
        assert Nn.bound_plan(n, k, self.cap, 1) == (self.slots, []) == R.bound_plan(n, k, self.cap, no_bound=True)
        self.dbgs = (0, 1) if self.bounded else (0,)
        if self.exact:
            D = S.data(regime, n, k)
            self.cols = R.support(self.d, ESIZE[self.dtype])
            self.q, self.c, self.alive = D.q[:B], D.c, D.alive
            self.prior, self.weight = D.prior, None if D.weight is None else D.weight[:B]
            self.qd, _ = upload(Nn, self.q, self.cols, self.d, self.dtype)
            self.cd, _ = upload(Nn, self.c, self.cols, self.d, self.dtype)
            self.es, self.er = (None, None) if D.es is None else (D.es[:B], D.er[:B])
        else:       # band: unit rows, compared on the values as stored
            self.cols = R.band_columns(self.d, ESIZE[self.dtype])
            q, c, self.alive = R.make("band", n, S.B_MAX, k, 0, ncols=self.cols.size)
            self.qd, self.q = upload(Nn, q[:B], self.cols, self.d, self.dtype, exact=False)
            self.cd, self.c = upload(Nn, c, self.cols, self.d, self.dtype, exact=False)
            self.es, self.er = R.expected(self.q, self.c, k)
        self.bits = alive_bits(self.alive)
        self.live = S.live_of(self.alive, n)
        self.counter_misses = []      # asserted after every answer of the shape was compared (test_regime)
        if self.exact and self.es is not None and k > n:      # more places than rows: the plain answer is padded
            m = int(self.live.sum())
            assert np.isneginf(self.es[:, m:]).all() and (self.er[:, m:] == -1).all() and (self.er[:, :m] >= 0).all()

    def ref(self, kernel, kind=None):
        return S.reference(kernel, self.regime, self.n, self.k, self.B, kind)

    def workspace(self, nbytes):
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")

    def counters(self, ws, B=None):
        torch.cuda.synchronize()
        return ws[: 4 * (B or self.B)].view(torch.int32).cpu().numpy().astype(np.int64)

    def check_counters(self, cnt, visible, neutral, what):
        """the main pass's survivors per query of a bounded call against the rows the query may see"""
        visible = np.broadcast_to(np.asarray(visible, np.int64), cnt.shape)
        assert (cnt <= visible).all(), (self.regime, cnt, visible)
        if self.regime in ("plateau", "cancelled"):
            assert np.array_equal(cnt, visible), (self.regime, cnt, visible)       # every row ties with tau
        elif neutral and (self.regime in BITE or self.regime.startswith("planted:")) and not (cnt < visible).all():
            self.counter_misses.append((what, self.row, self.regime, "survivors", cnt.tolist(), "of", visible.tolist()))

    def same(self, got, want, what):
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape, (what, i, a.shape, b.shape)
            assert np.array_equal(a, b), (what, i, self.regime, self.row, (self.d, self.dtype, self.k, self.B))

    def zero_rows_hold(self, r, s):
        """negative_with_zero_rows: the live zero rows in row order; no dead row, no row >= n and no -1 before the
        min(k, live)-th place"""
        if self.regime != "negative_with_zero_rows":
            return
        live, dead = R.zero_rows_layout(self.n, S.layout_k(self.n, self.k))
        m = min(self.k, int(self.live.sum()))
        head = r[:, :m]
        assert np.array_equal(head[:, : min(m, live.size)], np.tile(live[:m], (r.shape[0], 1)))
        assert not s[:, : min(m, live.size)].any()
        assert not np.isin(head, dead).any() and (head >= 0).all() and (head < self.n).all()

    def padding_holds(self, s, r, visible):
        """places past the rows a query may see are (-inf, -1)"""
        for b, m in enumerate(np.broadcast_to(visible, (r.shape[0],))):
            assert (r[b, m:] == -1).all() and np.isneginf(s[b, m:]).all() and (r[b, : min(m, self.k)] >= 0).all()


# ---- the kernels ---------------------------------------------------------------------------------------------------------
def run_scoped(x):
    Nn, n, k, B = x.N, x.n, x.k, x.B
    col = dev(S.documents64(n))
    for biting in (False, True):
        if biting and not x.exact:
            continue
        soq, scopes = S.scoped_config(B, biting)
        off = np.concatenate([[0], np.cumsum([len(s) for s in scopes])])
        groups = [g for s in scopes for g in s]
        # max_candidates = n: past the slots (20000 rows) the driver reads the counters and re-runs what overflowed
        s, r = host(*Nn.scoped_topk(x.qd, x.cd, n, x.d, k, col, S.N_DOCS, soq, off, groups, n, alive_bits=x.bits,
                                    cap=x.cap))
        if not x.exact:
            test_scoped_gpu.check(s, r, x.es, x.er)
            continue
        want = (x.es, x.er) if not biting else x.ref("scoped")
        x.same((s, r), want, "scoped biting=%s" % biting)
        if not biting:
            x.zero_rows_hold(r, s)
        vis = [int((np.isin(S.documents64(n), scopes[i]) & x.live).sum()) for i in soq]
        x.padding_holds(s, r, vis)


def run_filtered(x):
    Nn, n, k, B = x.N, x.n, x.k, x.B
    W = Nn.filter_words(n)
    foq = np.arange(B) % 2
    for biting in (False, True):
        if biting and not x.exact:
            continue
        vis = S.filters_of(n, k, x.stages, x.alive, biting)
        vis_dev = dev(S.bitmap_words(vis, W).view(np.int32))
        want = (x.es, x.er) if not biting else x.ref("filtered")
        first = None
        for dbg in x.dbgs:
            ws = x.workspace(Nn.filtered_topk_workspace_bytes(B, n, k))
            s, r = host(*Nn.filtered_topk(x.qd, x.cd, n, x.d, k, foq, vis_dev, workspace=ws, cap=x.cap, dbg=dbg))
            if not x.exact:
                test_filtered_gpu.check(s, r, x.es, x.er)
                continue
            x.same((s, r), want, "filtered biting=%s dbg=%d" % (biting, dbg))
            first = first or (s, r)
            x.same((s, r), first, "filtered bounded against unbounded")
            seen = vis.sum(axis=1)[foq]
            x.padding_holds(s, r, seen)
            if dbg == 0 and x.bounded:
                x.check_counters(x.counters(ws), seen, not biting, "filtered")
        if x.exact and not biting:
            x.zero_rows_hold(r, s)


def run_range(x):
    Nn, n, k, B = x.N, x.n, x.k, x.B
    codes = dev(S.facet_codes(n))
    vis_dev, foq = None, None
    if x.alive is not None:         # range_scan takes no alive bits: dead rows are a filter's business
        vis_dev = dev(S.bitmap_words(x.alive[None, :], Nn.filter_words(n)).view(np.int32))
        foq = np.zeros(B, np.int64)
    n_live = int(x.live.sum())
    for kind in ("floor",) + (S.RANGE_BITING if x.exact else ()):
        thr = S.range_thresholds(x.q, x.c, x.es, kind) if x.exact else np.full(B, -1.0, np.float32)
        want = x.ref("range", kind) if x.exact and kind != "floor" else None
        first = None
        for dbg in x.dbgs:
            ws = x.workspace(Nn.range_scan_workspace_bytes(B, n, k, S.FACET_G + 1))
            counts, facets, s, r = host(*Nn.range_scan(x.qd, x.cd, n, x.d, thr, k, [codes], [S.FACET_G], filter_of_query=foq,
                                                       vis_bits=vis_dev, workspace=ws, cap=x.cap, dbg=dbg))
            if kind == "floor":     # neutral: limit as k, every live row passes
                assert np.array_equal(counts, np.full(B, n_live)), (x.regime, counts)
                table = np.bincount(S.facet_codes(n)[x.live], minlength=S.FACET_G + 1)
                assert np.array_equal(facets, np.tile(table, (B, 1)))
                if not x.exact:
                    test_range_gpu.check_hits(s, r, x.es, x.er)
                    continue
                x.same((s, r), (x.es, x.er), "range floor dbg=%d" % dbg)
                x.zero_rows_hold(r, s)
            else:
                x.same((counts.astype(np.int64), facets.astype(np.int64), s, r), want, "range %s dbg=%d" % (kind, dbg))
                assert np.array_equal(facets.sum(axis=1), counts)
                if kind == "above":
                    assert not counts.any() and (r == -1).all()
                if kind == "kth" and x.regime == "plateau":
                    assert np.array_equal(counts, np.full(B, n))         # `>` would count none
                if kind == "best" and x.regime == "plateau_two_level":
                    assert np.array_equal(counts, np.full(B, S.layout_k(n, k) - 2))
            first = first or (counts, facets, s, r)
            x.same((counts, facets, s, r), first, "range bounded against unbounded")
            x.padding_holds(s, r, np.minimum(counts, n_live))
            if dbg == 0 and x.bounded:
                x.check_counters(x.counters(ws), counts, kind == "floor", "range")


def run_boosted(x):
    Nn, n, k, B = x.N, x.n, x.k, x.B
    if x.regime in S.BOOST_ONLY:
        prior, weight = x.prior, np.array(x.weight)      # copies: the cached data sets are read-only
        want = x.ref("boosted")
    else:       # neutral: weight 0 cancels whatever the prior holds
        prior, weight = S.neutral_prior(n), np.zeros(B, np.float32)
        want = (x.es, x.er, np.zeros((B, k), np.float32))
    prior_dev = dev(prior)
    first = None
    for dbg in x.dbgs:
        ws = x.workspace(Nn.boosted_topk_workspace_bytes(B, n, k))
        s, r, bo = host(*Nn.boosted_topk(x.qd, x.cd, n, x.d, k, prior_dev, weight, alive_bits=x.bits, workspace=ws,
                                         cap=x.cap, dbg=dbg))
        if not x.exact:
            test_boost_gpu.check(s, r, x.es, x.er)
            assert not bo.any()
            continue
        x.same((s, r, bo), want, "boosted dbg=%d" % dbg)
        first = first or (s, r, bo)
        x.same((s, r, bo), first, "boosted bounded against unbounded")
        x.zero_rows_hold(r, s)
        x.padding_holds(s, r, int(x.live.sum()))
        assert not bo[r < 0].any()
        if x.regime == "cancelled":
            assert not s[r >= 0].any() and np.array_equal(r[:, : min(k, n)], np.tile(np.arange(min(k, n)), (B, 1)))
        if dbg == 0 and x.bounded:
            x.check_counters(x.counters(ws), int(x.live.sum()), x.regime not in S.BOOST_ONLY, "boosted")


def run_recommend(x):
    Nn, n, k, B = x.N, x.n, x.k, x.B
    cols = x.cols
    for biting in (False, True):
        if biting and not x.exact:
            continue
        ex, sign, w = S.recommend_examples(x.q, biting)
        exd, _ = upload(Nn, ex, cols, x.d, x.dtype, exact=x.exact)
        first = None
        for dbg in x.dbgs:
            ws = x.workspace(Nn.recommend_topk_workspace_bytes(B, n, k))
            out = host(*Nn.recommend_topk(exd, sign, w, x.cd, n, x.d, k, alive_bits=x.bits, workspace=ws, cap=x.cap,
                                          dbg=dbg))
            s, r, pos, neg, pa, na = out
            if not x.exact:
                test_recommend_gpu.check(s, r, x.es, x.er, 0.0)
                continue
            if biting:
                want = x.ref("recommend")
                x.same(out, want, "recommend biting dbg=%d" % dbg)
                hit = r >= 0
                assert np.array_equal(s[hit], (pos - np.maximum(pos, 0))[hit])
            else:
                x.same((s, r), (x.es, x.er), "recommend neutral dbg=%d" % dbg)
                hit = r >= 0
                assert np.array_equal(pos[hit], x.es[hit]) and not neg.any() and (na == -1).all()
                assert np.array_equal(pa, np.where(hit, S.recommend_slots(B)[0][:, None], -1))
                x.zero_rows_hold(r, s)
            first = first or out
            x.same(out, first, "recommend bounded against unbounded")
            x.padding_holds(s, r, int(x.live.sum()))
            if dbg == 0 and x.bounded:
                x.check_counters(x.counters(ws), int(x.live.sum()), not biting, "recommend")


def run_related(x):
    Nn, n, k, B = x.N, x.n, x.k, x.B
    thr = 0.0
    for biting in (False, True):
        if biting and not x.exact:
            continue
        off, col, n_groups, excl = S.related_config(n, B, biting)
        if biting:
            out = test_related_gpu.run(Nn, x.qd, off, x.cd, n, x.d, k, col, n_groups, thr, excl, x.alive)
            test_related_gpu.assert_bit_equal(out, x.ref("related"))
            continue
        # at most MAX_SETS sets per call: the batch in calls of 64 one-vector sets
        parts = [test_related_gpu.run(Nn, x.qd[lo: lo + S.MAX_SETS], off[: min(S.MAX_SETS, B - lo) + 1], x.cd, n, x.d, k,
                                      col, n_groups, thr, excl, x.alive) for lo in range(0, B, S.MAX_SETS)]
        sim, grp, cov, best, best_row = (np.concatenate(p) for p in zip(*parts))
        if not x.exact:
            check_search(sim, grp.astype(np.int64), x.es, x.er)
            continue
        # neutral: sets of one vector, one row per group -- the plain search over ordinals
        x.same((sim, grp.astype(np.int64), best, best_row), (x.es, x.er, x.es, x.er), "related neutral")
        assert np.array_equal(cov, (x.es >= thr).astype(np.int32))
        x.zero_rows_hold(best_row, best)
        x.padding_holds(sim, grp, int(x.live.sum()))
        if x.regime == "negative":      # the table's zero word means "no candidate": no key of a real row may be it
            m = min(k, n)
            assert (grp[:, :m] >= 0).all() and (sim[:, :m] < 0).all() and np.isfinite(sim[:, :m]).all()


RUN = {"scoped": run_scoped, "filtered": run_filtered, "range": run_range, "boosted": run_boosted,
       "recommend": run_recommend, "related": run_related}


@pytest.mark.parametrize("kernel,row,regime", S.CASES)
def test_regime(N, kernel, row, regime):   # noqa: F811
    variants = S.variants_of(row, regime)
    assert variants
    misses = []
    for v in variants:
        x = Shape(N, row, regime, v)
        RUN[kernel](x)
        misses += x.counter_misses
    # the bound did bite: fewer survivors than rows for every query
    assert not misses, misses


# ---- one workspace across regimes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["boosted", "filtered", "recommend"])
def test_workspace_reuse_across_regimes(N, kernel):   # noqa: F811
    """falling leaves the highest tau and full counters a call can leave behind; negative is the regime in which a stale
    positive tau hides every real row"""
    row, v = "one_stage", (64, "f16", 5, 130)
    n, (d, _, k, B) = S.ROWS[row].n, v
    size = {"boosted": N.boosted_topk_workspace_bytes, "filtered": N.filtered_topk_workspace_bytes,
            "recommend": N.recommend_topk_workspace_bytes}[kernel](B, n, k)
    ws = torch.empty(size, dtype=torch.uint8, device="cuda")
    got = []
    for regime in ("falling", "negative", "falling"):
        x = Shape(N, row, regime, v)
        if kernel == "boosted":
            out = N.boosted_topk(x.qd, x.cd, n, d, k, dev(S.neutral_prior(n)), 0.0, workspace=ws)[:2]
        elif kernel == "filtered":
            vis = dev(S.bitmap_words(S.filters_of(n, k, x.stages, None, False), N.filter_words(n)).view(np.int32))
            out = N.filtered_topk(x.qd, x.cd, n, d, k, np.arange(B) % 2, vis, workspace=ws)
        else:
            ex, sign, w = S.recommend_examples(x.q, False)
            out = N.recommend_topk(upload(N, ex, x.cols, d, x.dtype)[0], sign, w, x.cd, n, d, k, workspace=ws)[:2]
        s, r = host(*out)
        x.same((s, r), (x.es, x.er), "%s on a used workspace, %s" % (kernel, regime))
        cnt = x.counters(ws)
        assert (cnt < n).all() and (cnt >= k).all()
        got.append((s, r))
    assert np.array_equal(got[2][0], got[0][0]) and np.array_equal(got[2][1], got[0][1])
    assert (got[1][0] < 0).all() and (got[0][0] > 0).all()
