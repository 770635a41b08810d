"""Score layouts the list kernels have to survive, and their exact answers (tests/test_search_regimes_*.py).

Every generator returns (q, c): float32 values ON THE SUPPORT ONLY, q [B, 16] and c [n, 16]; the matrix a kernel sees is
`expand(x, support(d, esize), d)`, zero in every other column.  The lattice generators use small integers that fp16,
bf16, fp32 (and, with `f8=True`, the FP8 set -2 .. 2 of tests/test_f8_gpu.py's exact-data cases) hold exactly, so every
score is an integer below 2^24 in magnitude: every float32 summation order gives the same bits, and the three-term
bf16 split of the fp32 path is exact too (hi holds the integer, lo = 0).  The expected answer is
oracle.search_oracle.cosine_topk on the support columns (`expected`), compared with np.array_equal.

C is the CU count the library plans with (the sample pre-pass covers the first 256 * C rows, a walk workgroup's static
tiles are 64 * C rows apart); k the requested depth.  Row layouts (`zero_rows_layout`, `plateau_high_rows`,
`planted_layout`) are functions of (n, k, C) alone, so a test can name the rows it expects without the data.

The scan family (tests/test_scan_regimes_*.py: the kernels that run pair_tile.h's body over 128-row tiles) has a part of
its own below: the bound plan restated (`bound_plan`, `sample_tiles`), planted layouts that are functions of
(n, k, the plan's stages) alone (`planted_tile_layout`), and two generators with integer priors for the boosted scan."""
import numpy as np

from oracle import search_oracle as O

NSUP = 16        # support columns
PARKED = 32      # dimensions of the walk's parked k-step (the last one of a row)
DISTINCT = 64    # distinct query rows of a generator; a batch repeats them (tile_queries)
Q_TILE = 64      # rows per tile of the query-stationary kernels
S_TILE = 256     # rows per tile of the slab-ring kernel; the sample pre-pass covers the first S_TILE * C rows


def support(d, esize):
    """16 columns of a d-wide row of esize-byte elements: column 0, both sides of the first and the last 128-byte slab
    boundary inside the row (a 64-d fp16 row is one slab: it has none), four columns of the last PARKED dimensions
    (d - 1, d - 2, d - 17, d - 32), the rest spread evenly"""
    assert d >= 64
    per = 128 // esize
    cols = [0, d - 1, d - 2, d - 17, d - PARKED]
    if per < d:
        last = (d - 1) // per * per
        cols += [per - 1, per, last - 1, last]
    cols = list(dict.fromkeys(cols))
    for c in [(j * d) // 17 for j in range(1, 17)] + list(range(d)):
        if len(cols) == NSUP:
            break
        if c not in cols:
            cols.append(c)
    cols = np.array(sorted(cols))
    assert cols.size == NSUP and cols[0] == 0 and np.sum(cols >= d - PARKED) >= 4
    return cols


def band_columns(d, esize):
    """the columns `band` rows are non-zero on: the support plus the last PARKED dimensions"""
    return np.union1d(support(d, esize), np.arange(d - PARKED, d))


def expand(x, cols, d):
    full = np.zeros((x.shape[0], d), dtype=np.float32)
    full[:, cols] = x
    return full


def tile_queries(base, B):
    """B query rows out of the distinct rows of `base`; neighbouring 64-query groups start at different rows"""
    b = np.arange(B)
    return np.ascontiguousarray(base[(b * 37 + b // 64) % base.shape[0]], dtype=np.float32)


def expected(q, c, k, alive=None):
    """oracle.search_oracle.cosine_topk(q, c, k): run once per distinct query row (equal queries have equal answers)"""
    uq, inv = np.unique(q, axis=0, return_inverse=True)
    es, er = O.cosine_topk(uq, c, k, alive=alive)
    inv = np.asarray(inv).reshape(-1)
    return es[inv], er[inv]


def spread_rows(n, m, must=(), lo=2):
    """m distinct rows of [lo, n): those of `must`, the others evenly spread"""
    rows = {int(r) for r in must}
    assert all(lo <= r < n for r in rows) and len(rows) <= m <= n - lo
    cand = lo + (np.arange(2 * m) * 2 + 1) * (n - lo) // (4 * m)
    for r in list(cand[::2]) + list(cand[1::2]) + list(range(lo, n)):
        if len(rows) == m:
            break
        rows.add(int(r))
    return np.array(sorted(rows), dtype=np.int64)


# ---- negative: every real score below zero -------------------------------------------------------------------------
def negative(n, B, seed=1):
    g = np.random.default_rng(seed)
    c = g.choice(np.array([0, 1, 2]), p=[0.5, 0.3, 0.2], size=(n, NSUP))
    empty = np.nonzero(~c.any(axis=1))[0]
    c[empty, g.integers(0, NSUP, empty.size)] = 1            # every row has a non-zero on the support
    base = g.integers(-2, 0, size=(DISTINCT, NSUP))           # {-2, -1} on the whole support
    c = c.astype(np.float32)
    assert (base.astype(np.float32) @ c.T).max() < 0
    return tile_queries(base, B), c


def zero_rows_layout(n, k):
    """(live, dead) all-zero rows of negative_with_zero_rows: k + 2 live ones (row 3 of tile 0 and row n - 1 among them)
    and five dead ones, one of them below every live one"""
    live = spread_rows(n, k + 2, must=(3, n - 1))
    dead = [r for r in (1, 70, n // 2 + 7, n - 2, n - 3, 2 * n // 3 + 1, n // 5, 5, 6, 7, 8) if r not in set(live.tolist())][:5]
    return live, np.array(sorted(dead), dtype=np.int64)


def zero_rows_alive(n, k):
    alive = np.ones(n, dtype=bool)
    alive[zero_rows_layout(n, k)[1]] = False
    return alive


def negative_with_zero_rows(n, B, k):
    q, c = negative(n, B)
    live, dead = zero_rows_layout(n, k)
    c[live] = 0.0
    c[dead] = 0.0
    return q, c


# ---- plateau: every row identical ----------------------------------------------------------------------------------
STEP_COL = NSUP - 1   # support column (the row's last dimension) that carries the higher level of the two-level variant


def plateau_high_rows(n, k, C):
    """the k - 2 rows of the two-level plateau that score one step higher: row n - 2 (last tile), the first row after
    the pre-pass sample (n // 3 where the collection is shorter than that), the rest spread; never row 0 or 1"""
    edge = S_TILE * C if S_TILE * C < n - 2 else n // 3
    return spread_rows(n, k - 2, must=(edge, n - 2))


def plateau(n, B, k=0, C=0, two_level=False, seed=2):
    g = np.random.default_rng(seed)
    p = 1 + (np.arange(NSUP) % 2 == 0)                        # {2, 1, 2, 1, ...}: p[STEP_COL] = 1
    base = g.integers(-2, 3, size=(8, NSUP))                  # scores of either sign, and zero
    c = np.tile(p.astype(np.float32), (n, 1))
    if two_level:
        base[:, STEP_COL] = 1
        c[plateau_high_rows(n, k, C), STEP_COL] += 1.0
    return tile_queries(base, B), c


# ---- rising / falling: the score is the row's 32-row block ------------------------------------------------------------
def rising(n, B, falling=False, f8=False, seed=3):
    """score = m * (r // 32) (falling: m * (max_block - r // 32)), m = 1 or 2 by query.  The block is held in two
    support columns as (block % radix, block // radix), radix 128 (FP8: 2, no multiplier, n <= 192)"""
    radix, vmax = (2, 2) if f8 else (128, 127)
    g = np.random.default_rng(seed)
    blk = np.arange(n) // 32
    if falling:
        blk = blk.max() - blk
    assert (blk // radix).max() <= vmax
    c = g.integers(0, 3, size=(n, NSUP)).astype(np.float32)   # the other columns meet zeros in the query
    c[:, 0] = blk % radix
    c[:, NSUP - 1] = blk // radix
    base = np.zeros((1 if f8 else 2, NSUP))
    base[:, 0] = np.arange(base.shape[0]) + 1
    base[:, NSUP - 1] = base[:, 0] * radix
    return tile_queries(base, B), c


# ---- planted: k + 3 distinct positive scores on a negative background ----------------------------------------------
PLANTED = ("one_tile", "one_walker", "tail", "sample_edge", "one_slab_ring_tile")


def planted_layout(where, n, k, C, f8=False):
    """(rows ascending, level of each row): level L > 0 is a row that outscores every row of a lower level for every
    query.  k + 3 rows (FP8: at most 32, what its value set can tell apart; one_walker: at most one per tile position)"""
    m = min(k + 3, 32) if f8 else k + 3
    g = np.random.default_rng(k + len(where))
    if where == "one_tile":            # one 64-row tile in the middle (more than 64 rows: the rows that follow it too)
        base = (n // Q_TILE) // 2 * Q_TILE
        rows = base + (np.sort(g.permutation(Q_TILE)[:m]) if m <= Q_TILE else np.arange(m))
    elif where == "one_slab_ring_tile":
        base = (n // S_TILE) // 2 * S_TILE
        rows = base + (np.sort(g.permutation(S_TILE)[:m]) if m <= S_TILE else np.arange(m))
    elif where == "one_walker":        # the same place in consecutive tiles of one workgroup's static walk
        r0 = Q_TILE * (C // 2) + 17
        m = min(m, (n - 1 - r0) // (Q_TILE * C) + 1)
        rows = r0 + Q_TILE * C * np.arange(m)
    elif where == "tail":              # the last three tile positions of the walk, row n - 1 and its tile's first row
        lo = max(((n + Q_TILE - 1) // Q_TILE - 3 * C) * Q_TILE, 2)
        rows = spread_rows(n, m, must=(n - 1, (n - 1) // Q_TILE * Q_TILE), lo=lo)
    elif where == "sample_edge":       # both sides of the row where the sample pre-pass ends
        e = S_TILE * C
        assert e + 2 < n and m >= 8
        rows = np.array(sorted({e - 5, e - 2, e - 1, e, e + 1, e + 2} | set(spread_rows(e - Q_TILE, m - 6).tolist())))
    else:
        raise ValueError(where)
    rows = np.asarray(rows, dtype=np.int64)
    m = rows.size
    assert m >= 1 and rows.max() < n and np.unique(rows).size == m
    levels = g.permutation(m) + 1
    if where == "sample_edge":
        # rows e - 5 and e + 2 tie on the second-highest level: the lower row must come first
        others = np.array([m] + list(range(1, m - 2)))
        levels = np.empty(m, dtype=np.int64)
        pair = np.isin(rows, (S_TILE * C - 5, S_TILE * C + 2))
        levels[pair] = m - 1
        levels[~pair] = g.permutation(others)
    return rows, levels


def staircase(levels):
    """support values of planted rows: no column above zero and, from one level to the next, one column a step lower:
    a query that is negative on the whole support scores a higher level strictly higher"""
    lv = np.asarray(levels, dtype=np.int64)[:, None]
    return -((lv + NSUP - 1 - np.arange(NSUP)[None, :]) // NSUP).astype(np.float32)


def planted(where, n, B, k, C, f8=False):
    q, c = negative(n, B)
    rows, levels = planted_layout(where, n, k, C, f8)
    c[rows] = staircase(levels)
    assert not f8 or np.abs(c).max() <= 2
    return q, c


# ---- the scan family (tests/test_scan_regimes_*.py): 128-row tiles, strided bound samples -----------------------------
P_TILE = 128             # rows per tile of pair_tile.h's body
SAMPLE0_TILES = 96       # tiles of the first bound stage (csrc/candidate_select.h)
MAX_STAGES = 8


def candidate_capacity(k):
    """csrc/candidate_select.h: candidate slots per query for a top-k of k"""
    return -(-max(32 * k, 16384) // 256) * 256


def bound_plan(n, k, cap=0, no_bound=False):
    """csrc/candidate_select.h make_bound_plan restated: (candidate slots per query, tiles of each bound stage)"""
    C = candidate_capacity(k)
    slots = cap if 0 < cap < C else C
    stages = []
    if n <= C or no_bound:
        return slots, stages
    n_tiles = -(-n // P_TILE)
    target = -(-(-(-4 * k * n // C)) // P_TILE)
    t = min(SAMPLE0_TILES, n_tiles)
    while True:
        stages.append(t)
        if t >= target or len(stages) == MAX_STAGES:
            break
        nt = min(t * C // (4 * k), target, n_tiles)
        if nt <= t:
            break
        t = nt
    return slots, stages


def sample_tiles(n, stages):
    """the 128-row tiles the bound stages visit: a stage of w tiles visits tile i * T // w for i in 0 .. w - 1
    (boosted_scan_kernel, masked_scan_body)"""
    T = -(-n // P_TILE)
    return {i * T // w for w in stages for i in range(w)}


def layout_stages(n, stages):
    """the stages a tile layout is planted against: the plan's, or, for a collection short enough to have none, one
    nominal stage over every other tile, so that the same rows are placed at every n"""
    return list(stages) or [(-(-n // P_TILE) + 1) // 2]


PLANTED_TILES = ("unsampled", "sampled", "one_lane", "one_pair_tile")
ONE_LANE_MAX_K = 13      # k + 3 winners in the 16 rows of one lane


def lane_rows(tile, wm, g4):
    """the 16 rows of a tile that one lane of pair_tile.h's body holds for each of its query columns"""
    return np.array([tile * P_TILE + 64 * wm + 16 * a + 4 * g4 + r for a in range(4) for r in range(4)], dtype=np.int64)


def planted_tile_layout(where, n, k, stages):
    """(rows ascending, level of each row) on 128-row tiles, a function of (n, k, stages) alone; k + 3 rows (one_pair_tile:
    at most the rows of its tile).  Levels as in planted_layout; `sampled` has two rows on the k-th level."""
    T = -(-n // P_TILE)
    st = layout_stages(n, stages)
    every, first = sample_tiles(n, st), sample_tiles(n, st[:1])
    g = np.random.default_rng(k + len(where))
    m = k + 3
    levels = None
    if where == "unsampled":           # no stage sees a winner: tau stays at what the background gives
        free = sorted(set(range(T)) - every)
        assert T - 1 in free and m <= n - (T - len(free)) * P_TILE
        after = next(t for t in free if t - 1 in every)
        must = {n - 1, (T - 1) * P_TILE, after * P_TILE}
        pool = np.concatenate([np.arange(t * P_TILE, min((t + 1) * P_TILE, n)) for t in free])
        pick = pool[(np.arange(2 * m) * 2 + 1) * pool.size // (4 * m)]
        rows = set(must)
        for r in list(pick[::2]) + list(pick[1::2]) + list(pool):
            if len(rows) == m:
                break
            rows.add(int(r))
        rows = np.array(sorted(rows), dtype=np.int64)
    elif where == "sampled":           # stage 1 sees the whole top-k; the k-th level ties with a row of the last tile
        assert T - 1 not in every and k >= 2
        pool = np.concatenate([np.arange(t * P_TILE, min((t + 1) * P_TILE, n)) for t in sorted(first)])
        assert m - 1 <= pool.size
        inner = np.unique(pool[(np.arange(m - 1) * 2 + 1) * pool.size // (2 * (m - 1))])
        inner = np.array(sorted(set(inner.tolist()) | set(pool[: m - 1 - inner.size + 8].tolist()))[: m - 1], dtype=np.int64)
        assert inner.size == m - 1
        high = (T - 1) * P_TILE + (n - 1 - (T - 1) * P_TILE) // 2
        rows = np.concatenate([inner, [high]])
        # ranks: k - 1 distinct levels above, two rows on level 3 (the k-th), levels 2 and 1 below
        lv = g.permutation(np.array([1, 2] + list(range(4, k + 3))))
        tied = int(g.integers(0, m - 1))
        levels = np.concatenate([lv[:tied], [3], lv[tied:], [3]])
    elif where == "one_lane":
        assert k <= ONE_LANE_MAX_K
        tile = T // 2
        wm = 1 if n - tile * P_TILE >= P_TILE else 0
        lane = lane_rows(tile, wm, 2)
        assert lane.max() < n
        rows = np.sort(lane[g.permutation(16)[:m]])
    elif where == "one_pair_tile":
        tile = T // 2
        width = min(P_TILE, n - tile * P_TILE)
        m = min(m, width)
        off = {min(63, width - 2), min(64, width - 1)} if width > 64 else {0, width - 1}   # both wm halves
        for o in g.permutation(width):
            if len(off) == m:
                break
            off.add(int(o))
        rows = tile * P_TILE + np.array(sorted(off), dtype=np.int64)
    else:
        raise ValueError(where)
    rows = np.asarray(rows, dtype=np.int64)
    if levels is None:
        levels = g.permutation(rows.size) + 1
    assert rows.size == m and np.unique(rows).size == m and rows.min() >= 0 and rows.max() < n
    assert np.all(np.diff(rows) > 0) and levels.size == m
    return rows, np.asarray(levels, dtype=np.int64)


def planted_tiles(where, n, B, k, stages):
    q, c = negative(n, B)
    rows, levels = planted_tile_layout(where, n, k, stages)
    c[rows] = staircase(levels)
    return q, c


# ---- boosted only: integer priors, weights from {-1, 0, 1, 2}: the fmaf is exact ---------------------------------------
def cancelled(n, B):
    """(q, c, prior, weight): the `rising` corpus with prior = -block and weight = the query's multiplier: every final is
    0, a plateau that only the epilogue makes"""
    q, c = rising(n, B)
    prior = -(np.arange(n) // 32).astype(np.float32)
    return q, c, prior, np.ascontiguousarray(q[:, 0])


def prior_only(n, B):
    """(q, c, prior, weight): the `plateau` corpus (every dot of a query equal) with a prior that rises in steps of 32
    rows; weight -1 makes the final fall with the row number, 0 leaves the plateau, 1 and 2 make it rise"""
    q, c = plateau(n, B)
    prior = (np.arange(n) // 32).astype(np.float32)
    return q, c, prior, ((np.arange(B) % 4) - 1).astype(np.float32)


# ---- band: unit rows around one direction, the only generator that is not a lattice -------------------------------------
BAND = (0.55, 0.98)     # all cosines, about
SIGMA2 = 0.2


def band(n, B, ncols, seed=5):
    """rows and queries normalize(m + noise) on `ncols` columns (band_columns): cos = (1 + ...) / (1 + SIGMA2 + ...)"""
    g = np.random.default_rng(seed)
    m = g.standard_normal(ncols)
    m /= np.linalg.norm(m)

    def rows_of(count):
        x = m[None, :] + np.sqrt(SIGMA2 / ncols) * g.standard_normal((count, ncols))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)

    c = rows_of(n)
    return tile_queries(rows_of(DISTINCT), B), c


# ---- one entry point ---------------------------------------------------------------------------------------------------
BASE = ("negative", "negative_with_zero_rows", "plateau", "plateau_two_level", "rising", "falling")
LATTICE = BASE + tuple("planted:" + w for w in PLANTED)
SCAN_LATTICE = BASE + tuple("planted:" + w for w in PLANTED_TILES)     # the scan family's exact regimes
REGIMES = LATTICE + ("band",)
NEEDS_LONG_SHARD = ("planted:one_walker", "planted:tail", "planted:sample_edge")   # no meaning below 256 * C rows


def make(regime, n, B, k, C, f8=False, ncols=NSUP, stages=None):
    """(q, c, alive or None) of a regime; `stages` (a bound_plan's) selects the scan family's planted layouts, which
    take the place of C"""
    if regime == "negative":
        return negative(n, B) + (None,)
    if regime == "negative_with_zero_rows":
        return negative_with_zero_rows(n, B, k) + (zero_rows_alive(n, k),)
    if regime == "plateau":
        return plateau(n, B) + (None,)
    if regime == "plateau_two_level":
        return plateau(n, B, k, C, two_level=True) + (None,)
    if regime in ("rising", "falling"):
        return rising(n, B, falling=regime == "falling", f8=f8) + (None,)
    if regime.startswith("planted:") and regime.split(":")[1] in PLANTED_TILES:
        return planted_tiles(regime.split(":")[1], n, B, k, stages or []) + (None,)
    if regime.startswith("planted:"):
        return planted(regime.split(":")[1], n, B, k, C, f8) + (None,)
    if regime == "band":
        return band(n, B, ncols) + (None,)
    raise ValueError(regime)
