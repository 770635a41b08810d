"""GPU: the list-search kernels (csrc/search.hip + slab_ring_body.inc, search_qs.hip, search_qsw.hip, search_f8.hip) and
the filter mode search_deep.hip drives, on the score layouts of tests/regime_ref.py: all scores negative, full plateaus,
scores monotone in the row number, winners concentrated in one tile / one workgroup's walk / the ticketed tail / the
edge of the sample pre-pass, a narrow high band, rows that are not unit length.

Lattice regimes: np.array_equal with the oracle on the support columns, scores and rows (tests/test_search_regimes_cpu.py
shows that oracle right on a CPU).  `band` and its negation: check() of tests/test_search_gpu.py, nothing else.

What these layouts found: `plateau_two_level` on the slab-ring and the three-launch kernels returned plateau rows 1, 2 (or
2, 3 ...) for 0, 1 -- TopList::insert_strict (csrc/search_shared.h) compared the entry it carried down the list, not the
new score, and dropped the carried entry at the first slot it tied with.

Every path row derives its n from the CU count the library plans with and asserts, before a variant's first call, which
kernel that variant runs on: `plan_path` restates make_plan and the dispatch of mmrag_internal_cosine_topk_lists_ex
(csrc/search.hip), `deep_path` make_deep_plan (csrc/search_deep.hip); at dbg = 0 `plan_path` is itself checked against
the library's mmrag_internal_search_uses_qs."""
import functools
from typing import NamedTuple

import numpy as np
import pytest
import torch

import f8_ref
import regime_ref as R
from test_search_gpu import check

pytestmark = pytest.mark.gpu

F16, BF16, F32, F8 = torch.float16, torch.bfloat16, torch.float32, torch.float8_e4m3fn
ESIZE = {F16: 2, BF16: 2, F32: 4, F8: 1}
B_MAX = 300


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


@pytest.fixture(scope="module")
def C(N):
    return N.device_info()["compute_units"]


# ---- which kernel a variant runs on -----------------------------------------------------------------------------------
def plan_path(N, C, B, n, d, dtype, k, dbg):
    """csrc/search.hip: make_plan, then the order in which mmrag_internal_cosine_topk_lists_ex tries the kernels"""
    K = 5 if k <= 5 else (10 if k <= 10 else 20)
    WN = 2 if B <= 64 else (4 if B <= 128 else 8)                         # plan_wn
    grid_y = -(-B // (32 * WN))
    n_tiles = -(-n // 256)
    grid_x = min(n_tiles, C)                                              # plan_walkers
    if grid_y > 1 and n_tiles >= C:
        w = C // grid_y // 8 * 8
        grid_x = w if w >= 8 else max(C // grid_y, 1)
    NW = 16 if (K == 5 and WN == 8 and not dbg & N.DBG_8_WAVES) else 8
    want_pre = (WN == 8 or K > 5) and n_tiles >= 3 * C
    pre = want_pre and not dbg & N.DBG_NO_PREPASS
    qs_room = WN == 8 and n_tiles >= C
    long_enough = n_tiles * 4 >= 15 * C if K <= 5 else n_tiles >= 6 * C
    qs_ok = qs_room and not dbg & N.DBG_NO_QS and (long_enough or bool(dbg & N.DBG_FORCE_QS))
    slabs = N.padded_dim(d, dtype) * ESIZE[dtype] // 128
    qs_rows = dtype in (F16, BF16) and slabs in (6, 8, 12)                # qs_supported / qsw_supported
    if dtype == F8:     # search_f8.hip dispatch_f8: no WN = 8 shape, more than 128 queries run as groups of the WN = 4 plan
        return "f8 slab-ring WN=%d" % min(WN, 4) + (" groups=%d" % -(-B // 128) if WN == 8 else "")
    if qs_ok and not dbg & N.DBG_OLD_QS and qs_rows and K == 5:
        per = -(-n // 64) // grid_x
        seed = per >= 12 and not dbg & N.DBG_NO_SEED
        dyn = grid_y == 1 and per >= 24 and not dbg & N.DBG_NO_DYN
        return "walk" + (" exchange" if seed else "") + (" tickets" if dyn else "") + (" groups=%d" % grid_y if grid_y > 1 else "")
    if qs_ok and qs_rows and K in (5, 10):
        return "qs3" + (" seeded" if pre else "")
    return "slab-ring WN=%d NW=%d" % (WN, NW) + (" pre-pass" if pre else "")


def deep_path(N, B, n, k, dbg, cap, dtype):
    """csrc/search_deep.hip make_deep_plan: bound passes only when the rows outnumber the candidate slots"""
    slots = N.candidate_capacity(k)
    if 0 < cap < slots:
        slots = cap
    WN = 2 if B <= 64 else (4 if B <= 128 else 8)
    if dtype == F8:
        WN = min(WN, 4)     # dispatch_f8
    bounded = n > slots and not dbg & N.DEEP_DBG_NO_BOUND
    return "filter WN=%d" % WN + (" bounded" if bounded else "") + (" overflow" if n > slots and not bounded else "")


class V(NamedTuple):
    """one call: a shape, the debug switches, and the path the plan rule must give it"""
    d: int
    dtype: torch.dtype
    k: int
    B: int
    dbg: int
    path: str
    deep: bool = False
    cap: int = 0
    only: tuple = ()       # regimes this variant is limited to (empty: all)


def rows_table(N, C):
    """the path rows: name -> (n, variants)"""
    FQ, OLD, NQ = N.DBG_FORCE_QS, N.DBG_OLD_QS, N.DBG_NO_QS
    t = {}
    wn = {33: 2, 100: 4, 200: 8}
    t["slab_ring_small"] = (4099, [
        V(d, dt, k, B, 0, "slab-ring WN=%d NW=%d" % (wn[B], 16 if (B == 200 and k == 5) else 8))
        for dt in (F16, BF16, F32) for d in (64, 100) for k in (5, 10, 20) for B in (33, 100, 200)])
    n3 = 3 * 256 * C + 5
    t["slab_ring_prepass"] = (n3, [
        V(64, F16, 5, 200, NQ, "slab-ring WN=8 NW=16 pre-pass"),
        V(64, F16, 5, 200, NQ | N.DBG_8_WAVES, "slab-ring WN=8 NW=8 pre-pass"),
        V(64, F16, 5, 200, NQ | N.DBG_NO_PREPASS, "slab-ring WN=8 NW=16"),
        V(64, F16, 20, 200, NQ, "slab-ring WN=8 NW=8 pre-pass"),
        V(64, F16, 20, 200, NQ | N.DBG_8_WAVES, "slab-ring WN=8 NW=8 pre-pass"),
        V(64, F16, 20, 200, NQ | N.DBG_NO_PREPASS, "slab-ring WN=8 NW=8")])
    for name, n, seeded in (("qs3", 256 * C + 3, ""), ("qs3_seeded", n3, " seeded")):
        t[name] = (n, [V(384, dt, k, 200, dbg, "qs3" + seeded)
                       for dt in (F16, BF16) for k, dbg in ((5, FQ | OLD), (10, FQ))])
    t["walk_exchange"] = (12 * 64 * C + 5, [
        V(384, F16, 5, 200, FQ, "walk exchange"), V(384, F16, 5, 200, FQ | N.DBG_NO_SEED, "walk"),
        V(384, F16, 5, 300, FQ, "walk exchange groups=2"), V(384, F16, 5, 300, FQ | N.DBG_NO_SEED, "walk groups=2")])
    t["walk_tickets"] = (24 * 64 * C + 200, [
        V(384, F16, 5, 256, FQ, "walk exchange tickets"), V(384, F16, 5, 256, 0, "walk exchange tickets"),
        V(384, F16, 5, 256, FQ | N.DBG_NO_DYN, "walk exchange"), V(384, F16, 5, 256, FQ | N.DBG_NO_SEED, "walk tickets"),
        V(384, F16, 5, 130, FQ, "walk exchange tickets"), V(384, F16, 5, 130, FQ | N.DBG_NO_DYN, "walk exchange"),
        V(384, F16, 5, 130, FQ | N.DBG_NO_SEED, "walk tickets"),
        V(512, F16, 5, 256, FQ, "walk exchange tickets")])
    # FP8 (search_f8.hip): no WN = 8 shape, 200 queries run as two groups of the 128-query plan
    f8_plans = ((7, "WN=2"), (65, "WN=4"), (200, "WN=4 groups=2"))
    t["f8"] = (4099, [V(130, F8, k, B, 0, "f8 slab-ring " + plan) for k in (5, 20) for B, plan in f8_plans]
               + [V(130, F8, 64, B, 0, "filter " + plan[:4], deep=True) for B, plan in f8_plans])
    NB = N.DEEP_DBG_NO_BOUND
    ties = ("plateau", "plateau_two_level", "rising")
    t["deep_small"] = (4099, [
        V(100, dt, k, B, dbg, "filter WN=%d" % wn[B], deep=True)
        for dt in (F16, F32) for k in (64, 1000) for B in (33, 200) for dbg in (0, NB)]
        + [V(100, dt, 64, 200, 0, "filter WN=8 bounded", deep=True, cap=256, only=ties) for dt in (F16, F32)])
    t["deep_long"] = (n3, [
        V(100, F16, 64, 33, 0, "filter WN=2 bounded", deep=True), V(100, F16, 1000, 200, 0, "filter WN=8 bounded", deep=True),
        V(100, F32, 64, 200, 0, "filter WN=8 bounded", deep=True), V(100, F32, 1000, 33, 0, "filter WN=2 bounded", deep=True),
        V(100, F16, 64, 33, NB, "filter WN=2 overflow", deep=True), V(100, F32, 64, 33, NB, "filter WN=2 overflow", deep=True),
        V(100, F16, 64, 33, 0, "filter WN=2 bounded", deep=True, cap=256, only=ties),
        V(100, F32, 64, 33, 0, "filter WN=2 bounded", deep=True, cap=256, only=ties)])
    return t


ROWS = ("slab_ring_small", "slab_ring_prepass", "qs3", "qs3_seeded", "walk_exchange", "walk_tickets", "f8", "deep_small",
        "deep_long")


def assert_path(N, C, v, n):
    got = deep_path(N, v.B, n, v.k, v.dbg, v.cap, v.dtype) if v.deep else plan_path(N, C, v.B, n, v.d, v.dtype, v.k, v.dbg)
    assert got == v.path, (v, n, got)
    if not v.deep and v.dbg == 0:      # the restated rule against the library's own
        name = N.search_kernel_name(v.B, n, v.d, v.k, v.dtype)
        assert name == ("cosine_topk_walk_kernel" if got.startswith("walk") else
                        "cosine_topk_qs_kernel" if got.startswith("qs3") else "cosine_topk_kernel (slab-ring)"), (v, name)
        assert N.search_uses_query_stationary(v.B, n, v.d, v.k, v.dtype) == ("slab-ring" not in got)


# ---- data: one (regime, n, k) data set and its expected answer, built once ----------------------------------------------
def regime_n(regime, n, f8):
    return 187 if f8 and regime in ("rising", "falling") else n   # FP8: (block % 2, block // 2) stays inside -2 .. 2


@functools.lru_cache(maxsize=4)
def lattice(regime, n, k, C, f8):
    q, c, alive = R.make(regime, n, B_MAX, k, C, f8=f8)
    es, er = R.expected(q, c, k, alive)
    for a in (q, c, es, er):
        a.setflags(write=False)
    return q, c, alive, es, er


def alive_bits(alive):
    if alive is None:
        return None
    words = np.zeros((alive.shape[0] + 31) // 32 + 8, dtype=np.uint32)
    idx = np.nonzero(alive)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32)).to("cuda")


def upload(N, vals, cols, d, dtype, scale=1.0, exact=True):
    """`vals * scale` on the columns `cols` of a zero matrix of the kernel's leading dimension, in the storage type;
    also the stored values as float32 (`exact`: they are the values, and normal numbers of the storage type)"""
    ld = N.padded_dim(d, dtype)
    want = (vals * np.float32(scale)).astype(np.float32)
    at = torch.from_numpy(np.asarray(cols)).to("cuda")
    if dtype == F8:     # an FP8 row stores 256 x its value (tests/f8_ref.py)
        codes = f8_ref.encode(want)
        t = torch.zeros((vals.shape[0], ld), dtype=torch.uint8, device="cuda")
        t[:, at] = torch.from_numpy(codes).to("cuda")
        t = t.view(F8)
        stored = (f8_ref.decode(codes) / 256.0).astype(np.float32)
        tiny = 2.0 ** -6 / 256.0
    else:
        t = torch.zeros((vals.shape[0], ld), dtype=dtype, device="cuda")
        t[:, at] = torch.from_numpy(want).to("cuda").to(dtype)
        stored = t[:, at].to(torch.float32).cpu().numpy()
        tiny = float(torch.finfo(dtype).tiny)
    if exact:
        assert np.array_equal(stored, want) and np.all((want == 0) | (np.abs(want) >= tiny))
    return t, stored


def call(N, v, qd, cd, n, bits=None, workspace=None):
    q = qd[:v.B]
    if v.deep:
        s, r = N.cosine_topk_deep(q, cd, n, v.d, v.k, alive_bits=bits, dbg=v.dbg, cap=v.cap)
    else:
        s, r = N.cosine_topk(q, cd, n, v.d, v.k, alive_bits=bits, dbg=v.dbg, workspace=workspace)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def variants_of(N, C, row, regime):
    n, variants = rows_table(N, C)[row]
    return n, [v for v in variants if not v.only or regime in v.only]


def groups_of(variants):
    """variants that share one uploaded data set: (d, dtype, k)"""
    out = {}
    for v in variants:
        out.setdefault((v.d, v.dtype, v.k), []).append(v)
    return out


# ---- 1 + 2: every regime on every path row ----------------------------------------------------------------------------
# The three shards of 4099 rows hold every regime but the planted layouts that need a long shard (R.NEEDS_LONG_SHARD):
# make_plan gives a collection of fewer than 256 * C rows one tile per workgroup at most (grid_x = n_tiles < cus) and
# neither a sample pre-pass (n_tiles >= 3 * cus) nor a query-stationary kernel (qs_room: n_tiles >= cus), so it has no
# second tile of a walker, no ticketed tail and no sample edge to plant rows at.
SHORT_ROWS = ("slab_ring_small", "f8", "deep_small")
PAIRS = [(row, regime) for row in ROWS for regime in R.REGIMES
         if not (row in SHORT_ROWS and regime in R.NEEDS_LONG_SHARD)]


@pytest.mark.parametrize("row,regime", PAIRS)
def test_regime_on_path(N, C, row, regime):
    n0, variants = variants_of(N, C, row, regime)
    assert (n0 == 4099) == (row in SHORT_ROWS)
    for (d, dtype, k), vs in groups_of(variants).items():
        f8 = dtype == F8
        n = regime_n(regime, n0, f8)
        for v in vs:
            assert_path(N, C, v, n)
        if regime == "band":
            cols = R.band_columns(d, ESIZE[dtype])
            q, c, _ = R.make("band", n, B_MAX, k, C, ncols=cols.size)
            qd, qs = upload(N, q, cols, d, dtype, exact=False)
            cd, cs = upload(N, c, cols, d, dtype, exact=False)
            es, er = R.expected(qs, cs, k)
            same = {}
            for v in vs:
                s, r = call(N, v, qd, cd, n)
                check(s, r, es[:v.B], er[:v.B])
                first = same.setdefault(v.B, (s, r))                 # variants of one shape: bit for bit
                assert np.array_equal(s, first[0]) and np.array_equal(r, first[1]), v
            continue
        q, c, alive, es, er = lattice(regime, n, k, C, f8)
        cols = R.support(d, ESIZE[dtype])
        scale = 1.0 / 256.0 if f8 else 1.0                           # the FP8 set: stored codes are the integers
        qd, _ = upload(N, q, cols, d, dtype, scale)
        cd, _ = upload(N, c, cols, d, dtype, scale)
        bits = alive_bits(alive)
        for v in vs:
            s, r = call(N, v, qd, cd, n, bits)
            want = es[:v.B] * np.float32(scale * scale)
            assert np.array_equal(r, er[:v.B]), (v, regime)
            assert np.array_equal(s, want), (v, regime)
            if regime == "negative_with_zero_rows":   # what the answer must be: the live zero rows, never a dead one
                live, dead = R.zero_rows_layout(n, k)
                assert np.array_equal(r[0], live[:k]) and not s.any() and not np.isin(r, dead).any()


# ---- 3: metamorphic checks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["negative", "plateau", "rising"])
@pytest.mark.parametrize("row", [r for r in ROWS if r != "f8"])      # FP8 saturates at 448 / 256
def test_power_of_two_scaling(N, C, row, regime):
    """corpus and queries times 2^s: the same rows, scores times 4^s bit for bit"""
    n, variants = variants_of(N, C, row, regime)
    for (d, dtype, k), vs in list(groups_of(variants).items())[:3]:
        v = vs[-1]
        assert_path(N, C, v, n)
        q, c, alive, es, er = lattice(regime, n, k, C, False)
        cols = R.support(d, ESIZE[dtype])
        cd, _ = upload(N, c, cols, d, dtype)
        qd, _ = upload(N, q, cols, d, dtype)
        s0, r0 = call(N, v, qd, cd, n)
        assert np.array_equal(r0, er[:v.B]) and np.array_equal(s0, es[:v.B])
        for e in (-6, 1 if dtype == BF16 else 3):
            cd, _ = upload(N, c, cols, d, dtype, 2.0 ** e)       # asserts: exact and normal in the storage type
            qd, _ = upload(N, q, cols, d, dtype, 2.0 ** e)
            s, r = call(N, v, qd, cd, n)
            assert np.array_equal(r, r0), (v, e)
            assert np.array_equal(s, s0 * np.float32(4.0 ** e)), (v, e)


@pytest.mark.parametrize("row", ROWS)
def test_negated_queries_on_the_band(N, C, row):
    """-q on the band: the k most dissimilar rows, every score negative"""
    n, variants = variants_of(N, C, row, "band")
    for (d, dtype, k), vs in list(groups_of(variants).items())[:3]:
        cols = R.band_columns(d, ESIZE[dtype])
        q, c, _ = R.make("band", n, B_MAX, k, C, ncols=cols.size)
        qd, qs = upload(N, -q, cols, d, dtype, exact=False)
        cd, cs = upload(N, c, cols, d, dtype, exact=False)
        es, er = R.expected(qs, cs, k)
        assert (es < 0).all()
        for v in vs:
            assert_path(N, C, v, n)
            s, r = call(N, v, qd, cd, n)
            check(s, r, es[:v.B], er[:v.B])
            assert (s < 0).all()


# ---- 4: one workspace across regimes -----------------------------------------------------------------------------------
def test_workspace_reuse_across_regimes(N, C):
    """falling leaves the highest thresholds and bests a launch can publish in the exchange block; negative is the
    regime in which a stale positive value hides every real row"""
    n, variants = rows_table(N, C)["walk_tickets"]
    v = variants[0]
    assert_path(N, C, v, n)
    cols = R.support(v.d, ESIZE[v.dtype])
    ws = torch.empty(N.cosine_topk_workspace_bytes(v.B, n, v.k), dtype=torch.uint8, device="cuda")
    got = []
    for regime in ("falling", "negative", "falling"):
        q, c, _, es, er = lattice(regime, n, v.k, C, False)
        qd, _ = upload(N, q, cols, v.d, v.dtype)
        cd, _ = upload(N, c, cols, v.d, v.dtype)
        s, r = call(N, v, qd, cd, n, workspace=ws)
        assert np.array_equal(r, er[:v.B]) and np.array_equal(s, es[:v.B]), regime
        got.append((s, r))
    assert np.array_equal(got[2][0], got[0][0]) and np.array_equal(got[2][1], got[0][1])
    assert (got[1][0] < 0).all() and (got[0][0] > 0).all()
