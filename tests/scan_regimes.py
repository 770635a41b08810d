"""The rows, regimes and per-kernel configurations of tests/test_scan_regimes_*.py, numpy only: what the six kernels
that run pair_tile.h's body (scoped, filtered, range, boosted, recommend, related) are called with, and what each kernel's
own reference (tests/*_ref.py) answers on the support columns.  TEST INFRASTRUCTURE ONLY.

A NEUTRAL configuration is one in which the kernel must give the plain search's answer, regime_ref.expected; a BITING
one makes what is the kernel's own decide the answer, and the kernel's reference says what it is.  Equal queries (and
equal scopes, filters, thresholds, weights) have equal answers, so a reference runs once per distinct row of its keys
(`by_unique`)."""
import functools
from typing import NamedTuple

import numpy as np

import boost_ref
import filter_ref
import range_ref
import recommend_ref
import regime_ref as R
import related_ref
import scoped_ref

B_MAX = 130
PLATEAU_C = 1            # regime_ref.plateau_high_rows' CU count: the first high row is row 256, the first of tile 2
TIES = ("plateau", "plateau_two_level", "rising")
BOOST_ONLY = ("cancelled", "prior_only")
KERNELS = ("scoped", "filtered", "range", "boosted", "recommend", "related")
E = recommend_ref.E


class Row(NamedTuple):
    n: int
    variants: tuple        # (d, dtype name, k, B)
    cap: int = 0           # candidate slots (0: the plan's)
    only: tuple = ()       # regimes the row is limited to (empty: all)


ROWS = {
    "short": Row(4099, tuple((d, dt, k, B) for dt in ("f16", "bf16", "f32") for d in (64, 100) for k in (5, 100)
                             for B in (3, 130))),
    "tiny": Row(100, tuple((64, dt, k, 3) for dt in ("f16", "f32") for k in (5, 128))),
    "one_stage": Row(20000, ((64, "f16", 5, 130), (64, "f16", 100, 130), (100, "f32", 5, 130))),
    "two_stage": Row(140000, ((64, "f16", 512, 130),)),
    "two_stage_small_cap": Row(140000, ((64, "f16", 512, 3),), cap=256, only=TIES + ("cancelled",)),
}
BOUNDED = ("one_stage", "two_stage", "two_stage_small_cap")
ROWS_OF = {"scoped": ("short", "tiny", "one_stage"), "related": ("short", "tiny")}      # the others: every row


def rows_of(kernel):
    return ROWS_OF.get(kernel, tuple(ROWS))


def regimes_of(kernel, row):
    """the regimes of a (kernel, row): the six lattice regimes, the planted tile layouts that exist at the row's shape
    (a single tile has no sample to be in or out of; k = 512 winners fit no lane), `band` on the short row, and the
    two boosted-only generators"""
    out = list(R.BASE)
    planted = {"tiny": ("one_lane", "one_pair_tile"), "two_stage": ("unsampled", "sampled", "one_pair_tile"),
               "two_stage_small_cap": ()}.get(row, R.PLANTED_TILES)
    out += ["planted:" + w for w in planted]
    if row == "short":
        out.append("band")
    if kernel == "boosted":
        out += list(BOOST_ONLY)
    only = ROWS[row].only
    return [g for g in out if not only or g in only]


def variants_of(row, regime):
    """the row's (d, dtype, k, B) at which the regime exists: one_lane holds k + 3 <= 16 winners"""
    return [v for v in ROWS[row].variants if not (regime == "planted:one_lane" and v[2] > R.ONE_LANE_MAX_K)]


CASES = [(kernel, row, regime) for kernel in KERNELS for row in rows_of(kernel) for regime in regimes_of(kernel, row)]


class Data(NamedTuple):
    q: np.ndarray          # [B_MAX, 16] on the support
    c: np.ndarray          # [n, 16]
    alive: object          # bool [n] or None
    es: object             # regime_ref.expected (None for the boosted-only generators)
    er: object
    stages: tuple
    prior: object = None   # boosted-only generators
    weight: object = None


def layout_k(n, k):
    """the k a regime's rows are laid out for: k itself unless the collection is too short to hold k + 3 planted rows"""
    return min(k, n // 4)


@functools.lru_cache(maxsize=4)
def data(regime, n, k):
    """one (regime, n, k) data set and the plain search's answer, built once and read-only"""
    stages = tuple(R.bound_plan(n, k)[1])
    if regime in BOOST_ONLY:
        q, c, prior, weight = (R.cancelled if regime == "cancelled" else R.prior_only)(n, B_MAX)
        out = Data(q, c, None, None, None, stages, prior, weight)
    else:
        q, c, alive = R.make(regime, n, B_MAX, layout_k(n, k), PLATEAU_C, stages=list(stages))
        es, er = R.expected(q, c, k, alive)
        out = Data(q, c, alive, es, er, stages)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def by_unique(keys, fn):
    """fn(indices of one representative per distinct row of `keys`) -> arrays with one leading row per representative;
    returns them expanded to every row of `keys`"""
    keys = np.ascontiguousarray(keys)
    _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    return tuple(np.asarray(o)[inv] for o in fn(first))


def live_of(alive, n):
    return np.ones(n, dtype=bool) if alive is None else np.asarray(alive, dtype=bool)


# ---- scoped ------------------------------------------------------------------------------------------------------------
N_DOCS = 64


def documents64(n):
    """64 contiguous documents (fewer when n < 64) that cover every row"""
    return (np.arange(n, dtype=np.int64) * N_DOCS // n).astype(np.int32)


def scoped_config(B, biting):
    """(scope_of_query [B], scopes): neutral = one scope of all 64 documents; biting = the even documents, the odd ones
    and an empty scope, taken in turn by the queries"""
    if not biting:
        return np.zeros(B, np.int64), [list(range(N_DOCS))]
    return np.arange(B) % 3, [list(range(0, N_DOCS, 2)), list(range(1, N_DOCS, 2)), []]


def scoped_reference(q, c, k, alive, biting):
    soq, scopes = scoped_config(q.shape[0], biting)
    col = documents64(c.shape[0])
    return by_unique(np.column_stack([q, soq]),
                     lambda at: scoped_ref.scoped_topk(q[at], c, k, col, soq[at], scopes, alive))


# ---- filtered ----------------------------------------------------------------------------------------------------------
SPARSE_SAMPLED_ROWS = 9


def sparse_filter(n, k, stages):
    """bool [n]: every row of the tiles no bound stage visits and fewer than k rows (odd rows of tile 0, which every
    stage visits) of the others: a sample that never holds k visible rows, so tau must stay where it started"""
    tile_of = np.arange(n) // R.P_TILE
    vis = ~np.isin(tile_of, sorted(R.sample_tiles(n, R.layout_stages(n, stages))))
    m = min(k - 1, SPARSE_SAMPLED_ROWS)
    vis[2 * np.arange(m) + 1] = True
    return vis


def filters_of(n, k, stages, alive, biting):
    """bool [2, n], two filters the batch shares: neutral = every live row, twice; biting = every other 32-row word, and
    the sparse-sample filter"""
    live = live_of(alive, n)
    if not biting:
        return np.stack([live, live])
    return np.stack([(np.arange(n) // 32 % 2 == 0) & live, sparse_filter(n, k, stages) & live])


def bitmap_words(vis, W, ones_past_n=True):
    """uint32 [F, W] of bool [F, n]; bits at and past n are ones: a bitmap from elsewhere may hold them"""
    F, n = vis.shape
    bits = np.full((F, W * 32), ones_past_n, dtype=bool)
    bits[:, :n] = vis
    return np.packbits(bits.reshape(F, W, 32), axis=2, bitorder="little").view(np.uint32).reshape(F, W)


def filtered_reference(q, c, k, stages, alive, biting):
    B, n = q.shape[0], c.shape[0]
    foq = np.arange(B) % 2
    vis = filters_of(n, k, stages, alive, biting)
    return by_unique(np.column_stack([q, foq]), lambda at: filter_ref.topk_of_visible(q[at], c, k, vis[foq[at]]))


# ---- range -------------------------------------------------------------------------------------------------------------
FACET_G = 7
RANGE_BITING = ("kth", "best", "above")


def facet_codes(n):
    return (np.arange(n) % FACET_G).astype(np.int32)


def score_floor(q, c):
    """a finite threshold below every score of the data set"""
    uq = np.unique(q, axis=0)
    return float(np.floor((uq.astype(np.float64) @ c.astype(np.float64).T).min()) - 1.0)


def range_thresholds(q, c, es, kind):
    """float32 [B]: `floor` = below every score; `kth` = exactly the last finite score of the plain top-k (on a plateau
    every row ties with it: `>` would count none; on the two-level plateau the low level); `best` = exactly the best score
    (the two-level plateau: its k - 2 high rows); `above` = one integer above the best (nothing passes)"""
    B = q.shape[0]
    if kind == "floor":
        return np.full(B, score_floor(q, c), np.float32)
    fin = np.isfinite(es)
    assert fin[:, 0].all()
    last = es[np.arange(B), fin.sum(axis=1) - 1]
    return {"kth": last, "best": es[:, 0], "above": es[:, 0] + np.float32(1.0)}[kind].astype(np.float32)


def range_reference(q, c, limit, thr, alive):
    """(counts [B], facets [B, FACET_G + 1], scores, rows) of range_ref.range_ref"""
    n = c.shape[0]
    vis = None if alive is None else np.asarray(alive, bool)
    codes = facet_codes(n)

    def run(at):
        counts, tables, s, r = range_ref.range_ref(q[at], c, thr[at], limit,
                                                   None if vis is None else np.tile(vis, (at.size, 1)), [codes], [FACET_G])
        return counts, tables[0], s, r

    return by_unique(np.column_stack([q, thr]), run)


# ---- boosted -----------------------------------------------------------------------------------------------------------
def neutral_prior(n):
    """a prior that weight 0 must cancel"""
    return (np.arange(n) % 7).astype(np.float32)


def boosted_reference(q, c, k, prior, weight, alive):
    weight = np.broadcast_to(np.asarray(weight, np.float32), (q.shape[0],))
    return by_unique(np.column_stack([q, weight]),
                     lambda at: boost_ref.boosted_topk(q[at], c, k, prior, weight[at], alive))


# ---- recommend ---------------------------------------------------------------------------------------------------------
def recommend_slots(R_):
    """(slot of the positive, slot of the negative) of each request: the kernel must not care where they sit"""
    g = np.arange(R_)
    pos = g % 5
    return pos, pos + 1 + g % 3


def recommend_examples(q, biting):
    """(examples [16 R, 16] on the support, sign int8 [16 R], weight [R]): request g = query g as its one positive;
    biting: the same vector as its one negative with weight 1, so final = pos - max(pos, 0): 0 where pos > 0, pos where
    pos <= 0, and on all-negative data the clamp is all that keeps the scores"""
    R_ = q.shape[0]
    ex = np.zeros((E * R_, q.shape[1]), np.float32)
    sign = np.zeros(E * R_, np.int8)
    pos, neg = recommend_slots(R_)
    g = np.arange(R_)
    ex[E * g + pos] = q
    sign[E * g + pos] = 1
    if biting:
        ex[E * g + neg] = q
        sign[E * g + neg] = -1
    return ex, sign, np.full(R_, 1.0 if biting else 0.5, np.float32)


def recommend_reference(q, c, k, alive, biting):
    """the six outputs of recommend_ref.recommend_topk for recommend_examples(q, biting): a request's scores depend on its
    vector alone, so the reference runs once per distinct vector with the examples in slots 0 and 1, and the slots it
    names are then those of recommend_slots"""
    def run(at):
        ex, sign, w = recommend_examples(q[at], biting)
        ex, sign = ex.reshape(at.size, E, -1), sign.reshape(at.size, E)
        canon_ex, canon_sign = np.zeros_like(ex), np.zeros_like(sign)
        p, m = recommend_slots(at.size)
        i = np.arange(at.size)
        canon_ex[:, 0], canon_sign[:, 0] = ex[i, p], sign[i, p]
        canon_ex[:, 1], canon_sign[:, 1] = ex[i, m], sign[i, m]
        return recommend_ref.recommend_topk(canon_ex.reshape(at.size * E, -1), canon_sign.reshape(-1), w, c, k, alive)

    s, r, pos, neg, pa, na = by_unique(q, run)
    p, m = recommend_slots(q.shape[0])
    pa = np.where(pa >= 0, p[:, None], -1).astype(np.int32)
    na = np.where(na >= 0, m[:, None], -1).astype(np.int32)
    return s, r, pos, neg, pa, na


# ---- related -----------------------------------------------------------------------------------------------------------
MAX_SETS = 64            # mmrag_related_groups takes at most 64 sets per call


def related_config(n, M, biting):
    """(set_off, group_of_row int32 [n], n_groups, exclude): neutral = sets of one vector, one row per group; biting =
    sets of 1, 2, 3 and 4 vectors in turn (at most MAX_SETS sets) over test_scoped_gpu.documents (groups of 1 to 200 rows, one across the rows 126
    to 129, some rows in no group), every third set excluding a group"""
    if not biting:
        return list(range(M + 1)), np.arange(n, dtype=np.int32), n, None
    from test_scoped_gpu import documents

    col, n_groups = documents(n, 11)
    off = [0]
    while off[-1] < M:
        off.append(min(M, off[-1] + 1 + (len(off) - 1) % 4))
    used = np.unique(col[col >= 0])
    excl = [int(used[s % used.size]) if s % 3 == 0 else -1 for s in range(len(off) - 1)]
    return off, col, n_groups, excl


def related_reference(q, c, k, alive, threshold, biting):
    off, col, n_groups, excl = related_config(c.shape[0], q.shape[0], biting)
    return related_ref.related_groups(q, off, c, col, n_groups, k, threshold, excl, alive)[0]


# ---- one entry point, cached: a reference does not depend on d or on the storage type --------------------------------------
@functools.lru_cache(maxsize=16)
def reference(kernel, regime, n, k, B, kind=None):
    """the BITING reference of a kernel on data(regime, n, k)[:B] (`kind`: range's threshold kind), read-only"""
    D = data(regime, n, k)
    q = D.q[:B]
    if kernel == "scoped":
        out = scoped_reference(q, D.c, k, D.alive, True)
    elif kernel == "filtered":
        out = filtered_reference(q, D.c, k, D.stages, D.alive, True)
    elif kernel == "range":
        out = range_reference(q, D.c, k, range_thresholds(q, D.c, D.es[:B], kind), D.alive)
    elif kernel == "boosted":
        out = boosted_reference(q, D.c, k, D.prior, D.weight[:B], None)
    elif kernel == "recommend":
        out = recommend_reference(q, D.c, k, D.alive, True)
    else:
        out = related_reference(q, D.c, k, D.alive, 0.0, True)
    for a in out:
        a.setflags(write=False)
    return out
