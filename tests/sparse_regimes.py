"""Structured inputs for the learned sparse leg (csrc/sparse_score.hip, csrc/sparse_expand.hip) with fully determined
answers.  Pure NumPy, no package import.

Impact corpora.  As in tests/lexical_regimes.py a corpus is a list of signature classes, each a fixed sorted tuple of
(term, impact) pairs, and a layout that gives every row a class through a LEVEL (-2 a row that cannot match, -1 a row
without terms, >= 0 a matching class).  Scores are exact integers, so there is no gap condition: the answer is score
descending, then row ascending, and the levels of a case give strictly increasing scores for the case's query
(`level_scores`).  A test names the rows it expects without the data: lexical_regimes.named_topk.

Two layouts are defined by the kernel's own sampling.  mmrag_impact_topk runs under candidate_select.h's
bounded_scan_select, whose plan (`bound_plan`, make_bound_plan restated) counts 128-row tiles; impact_topk_impl maps a
stage of `tiles` tiles onto walk = ceil(tiles / 16) of its 2048-row blocks, block i * n_blocks / walk for i < walk
(`stage_blocks`).  `planted:sampled_blocks` puts k + 3 winners into blocks EVERY stage visits (the stages raise tau to
the true k-th score, few rows survive the main pass); `planted:unsampled_blocks` puts them into blocks NO stage visits,
above a full plateau (tau stops at the plateau, every row survives, the query overflows and is produced again alone).

Pool cases are integer-valued fp16 planes (every dot product exact: the comparison is by bits), select cases lie on a
grid 0.25 away from every half-integer.  tests/test_sparse_regimes_cpu.py proves every claim made here."""
import functools
from typing import NamedTuple, Tuple

import numpy as np

import lexical_regimes as LR
import sparse_ref as R

# csrc/sparse_score.hip, csrc/sparse_expand.hip and csrc/pair_tile.h, restated: the tests compare them with
# mmrag_internal_sparse_limits
IMP_R = 2048          # rows one workgroup of impact_score_kernel scores
SP_BATCH = 8          # chunk pieces sparse_pool_kernel folds per pair of barriers
SP_VRUN = 16          # vocabulary tiles a pool workgroup takes at most
SEL_T = 256           # terms sparse_select_kernel takes per step
PT = 128              # rows of a pair tile: token rows and vocabulary rows of one pool tile, the bound plan's tile
LIMITS = {"impact_rows": IMP_R, "pool_batch": SP_BATCH, "pool_vrun": SP_VRUN, "select_terms": SEL_T, "tile_rows": PT}
assert LR.SCORE_R == IMP_R       # lexical_regimes' layouts place their rows by this block
IMP_TILES = IMP_R // PT
MAX_SCORE = 255 * 255 * R.MAX_QUERY_TERMS      # 4 161 600 < 2^24

candidate_capacity = LR.candidate_capacity
BOUND_SAMPLE0_TILES, BOUND_MAX_STAGES = 96, 8


def bound_plan(n, k, cap_override=0, no_bound=False):
    """(candidate slots per query, 128-row tiles of each bound stage): candidate_select.h make_bound_plan"""
    C = candidate_capacity(k)
    cap = cap_override if 0 < cap_override < C else C
    if n <= C or no_bound:
        return cap, []
    n_tiles = (n + PT - 1) // PT
    target = ((4 * k * n + C - 1) // C + PT - 1) // PT
    stages, t = [], min(BOUND_SAMPLE0_TILES, n_tiles)
    while True:
        stages.append(t)
        if t >= target or len(stages) == BOUND_MAX_STAGES:
            break
        nt = min(t * C // (4 * k), target, n_tiles)
        if nt <= t:
            break
        t = nt
    return cap, stages


def blocks(n):
    return (n + IMP_R - 1) // IMP_R


def stage_blocks(n, tiles):
    """the 2048-row blocks a pass over `tiles` of the driver's tiles visits (impact_topk_impl's `produce`)"""
    nb = blocks(n)
    walk = min(max((tiles + IMP_TILES - 1) // IMP_TILES, 1), nb)
    return [i * nb // walk for i in range(walk)]


def sampled_blocks(n, k):
    """(blocks every stage visits, blocks no stage visits) of the plan of (n, k)"""
    _, stages = bound_plan(n, k)
    assert stages, (n, k)
    seen = [set(stage_blocks(n, t)) for t in stages]
    every, some = set.intersection(*seen), set.union(*seen)
    return sorted(every), sorted(set(range(blocks(n))) - some)


def rows_in_blocks(n, blks, W):
    """W distinct rows spread over the blocks `blks`, first and last row of every block first"""
    rows = []
    for j, b in enumerate(blks):
        lo, hi = b * IMP_R, min((b + 1) * IMP_R, n)
        take = W // len(blks) + (1 if j < W % len(blks) else 0)
        if take == 0:
            continue
        assert take <= hi - lo, (n, b, W)
        rows.append(lo + np.unique(np.linspace(0, hi - lo - 1, take).astype(np.int64)))
        assert rows[-1].size == take
    return np.concatenate(rows)


def layout(name, n, W, k=0):
    """level per row: lexical_regimes.layout, and the two layouts placed by the plan of (n, k)"""
    if name in ("planted:sampled_blocks", "planted:unsampled_blocks"):
        every, never = sampled_blocks(n, k)
        rows = rows_in_blocks(n, every if name.endswith(":sampled_blocks") else never, k + 3)
        level = np.zeros(n, np.int64)
        level[rows] = 1 + np.arange(rows.size) % 3
        return level
    return LR.layout(name, n, W)


# ---------------------------------------------------------------------------------------------------- corpora, queries
V = 604               # terms: query terms are 0 .. 598 in a scrambled order (lexical_regimes.query_terms)
NQ = 599              # in no query, in most rows
LONE = 600            # held by ONE row, a row of the layout's highest level; the 64-term query asks for it
NONE = 601            # in no row
EMPTY, NOMATCH = LR.EMPTY, LR.NOMATCH
ANCHORS_64 = (63, 0, 31, 32, 17, 40)      # positions of the 64-term query whose terms the classes hold, the last first
LONE_AT = 7                               # position of LONE in the 64-term query; every other position has no posting


def query(T, mode):
    """(terms ascending, as a sparse vector is; their impacts; the anchor terms) of a case's query: one term, or
    MMRAG_MAX_SPARSE_QUERY_TERMS of them.  ANCHORS_64 and LONE_AT are positions of the scrambled list"""
    assert T in (1, R.MAX_QUERY_TERMS)
    t = LR.query_terms(T)
    if T == 1:
        assert mode != "top"
        return t, [200], t
    anchors = [t[p] for p in ANCHORS_64]
    w = [1 + (i * 53) % 255 for i in range(T)]      # 1 .. 255; position 0 has impact 1
    w[63], w[31] = 255, 254
    if mode == "top":
        w = [255] * T
    else:
        t[LONE_AT] = LONE
    order = np.argsort(t)
    return [t[i] for i in order], [w[i] for i in order], anchors


def level_classes(q, A, n_levels, mode):
    """classes 0 .. n_levels - 1 of rising score, then the EMPTY and the NOMATCH class.
    terms:  level l holds the first l + 1 anchor terms (impact 3)
    impact: one anchor, impact 1 + l
    top:    the highest level holds all 64 query terms at impact 255 (score 4 161 600 under impacts 255), each level
            below it has one more of them at 254; level 0 holds the first term alone, impact 1"""
    out = []
    for lv in range(n_levels):
        if mode == "terms":
            assert n_levels <= len(A), (n_levels, len(A))
            pairs = [(t, 3) for t in A[: lv + 1]] + [(NQ, 1)]
        elif mode == "impact":
            assert n_levels <= 255
            pairs = [(A[0], 1 + lv), (NQ, 1)]
        else:
            assert mode == "top" and len(q) == R.MAX_QUERY_TERMS and n_levels <= 4
            lower = n_levels - 1 - lv
            pairs = [(q[0], 1)] if lv == 0 else [(t, 254 if i < lower else 255) for i, t in enumerate(q)]
        out.append(tuple(sorted(pairs)))
    return out + [(), ((NQ, 1),)]


class Corpus:
    """classes (tuples of (term, impact) pairs) and a class per row"""

    def __init__(self, classes, row_class):
        self.classes, self.row_class = list(classes), np.asarray(row_class, np.int64)
        self.n = self.row_class.size

    @functools.cached_property
    def log(self):
        """(off int64 [n + 1], terms int32, impacts int32): what ImpactIndex.append takes"""
        off, ids, imps, _ = LR.Corpus([(p, 0) for p in self.classes], self.row_class).log
        return off, ids, imps

    def class_scores(self, qt, qw):
        have = dict(zip(qt, qw))
        return np.array([sum(have.get(t, 0) * i for t, i in p) for p in self.classes], np.int64)

    def scores(self, qt, qw):
        """score per row by class: an independent restatement of sparse_ref.scores for these corpora"""
        return self.class_scores(qt, qw)[self.row_class]


class Case(NamedTuple):
    id: str
    layout: str
    n: int
    T: int
    ks: Tuple[int, ...]
    W: int = 9
    mode: str = "auto"           # auto: terms when the levels fit the anchors, else impact | top
    mask: str = "none"           # none | masked (alive bits of the case)
    plan_k: int = 0              # the k the sampled / unsampled layouts are placed for
    regime: str = ""             # "" | few (survivors far below n) | all (every live match survives, above the slots)


KS = (1, 5, 100, 512)
BIG = 140_000
CASES = [
    Case("plateau-1", "plateau", 1, 1, (1, 5)),
    Case("plateau-100", "plateau", 100, 64, KS),
    Case("plateau-2048", "plateau", 2048, 1, KS),
    Case("plateau-2049", "plateau", 2049, 64, KS),
    Case("plateau-4099", "plateau", 4099, 1, KS + (4096,)),
    Case("plateau-16640", "plateau", 16640, 64, KS + (4096,)),
    Case("plateau-140000", "plateau", BIG, 1, (512,), regime="all"),
    Case("two-level-4099", "two_level", 4099, 64, KS, W=50),
    Case("two-level-16640", "two_level", 16640, 1, KS, W=256),
    Case("rising-4099", "rising", 4099, 1, KS),
    Case("falling-4099", "falling", 4099, 64, KS, mode="impact"),
    Case("block-edges-4099", "planted:block_edges", 4099, 64, KS + (4096,)),
    Case("block-edges-100", "planted:block_edges", 100, 1, KS),
    Case("block-edges-top-4099", "planted:block_edges", 4099, 64, KS, mode="top"),
    Case("one-block-4099", "planted:one_block", 4099, 64, KS),
    Case("one-block-2049", "planted:one_block", 2049, 1, KS),
    Case("one-per-block-16640", "planted:one_per_block", 16640, 64, KS),
    Case("word-edges-4099", "planted:word_edges", 4099, 64, KS, mask="masked"),
    Case("dead-term-4099", "dead_term", 4099, 64, KS, mask="masked"),
    Case("sparse-1", "sparse", 1, 1, (1, 5)),
    Case("sparse-2048", "sparse", 2048, 64, (1, 5)),
    Case("sparse-2049", "sparse", 2049, 1, (1, 5)),
    Case("sampled-16640", "planted:sampled_blocks", 16640, 64, (5,), plan_k=5, regime="few"),
    Case("unsampled-16640", "planted:unsampled_blocks", 16640, 1, (5,), plan_k=5, regime="all"),
    Case("sampled-140000", "planted:sampled_blocks", BIG, 1, (512,), plan_k=512, regime="few"),
    Case("unsampled-140000", "planted:unsampled_blocks", BIG, 64, (512,), plan_k=512, regime="all"),
]
CASE_IDS = [c.id for c in CASES]


def case(case_id):
    return CASES[CASE_IDS.index(case_id)]


class Built(NamedTuple):
    corpus: Corpus
    qt: list                     # query terms
    qw: list                     # query impacts
    level: np.ndarray            # per row, AFTER the lone row was raised by one where the query asks for LONE
    allowed: np.ndarray
    lone_row: int


@functools.lru_cache(maxsize=None)
def build(c):
    n = c.n
    base = layout(c.layout, n, c.W, c.plan_k)
    n_levels = int(base.max()) + 1
    mode = c.mode if c.mode != "auto" else ("terms" if n_levels <= (len(ANCHORS_64) if c.T > 1 else 1) else "impact")
    qt, qw, anchors = query(c.T, mode)
    classes = level_classes(qt, anchors, n_levels, mode)
    row_class = np.where(base >= 0, base, np.where(base == EMPTY, n_levels, n_levels + 1))
    # LONE: on the first row of the highest level; with it in the query that row is a level of its own above all
    lone_row = int(np.nonzero(base == base.max())[0][0])
    classes.append(tuple(sorted(classes[row_class[lone_row]] + ((LONE, 2),))))
    row_class[lone_row] = len(classes) - 1
    level = base.copy()
    if LONE in qt:
        level[lone_row] += 1
    allowed = np.ones(n, bool)
    if c.layout == "planted:word_edges":
        allowed = LR.word_edges_allowed(n)
    if c.layout == "dead_term":
        allowed = base != 2
    return Built(Corpus(classes, row_class), qt, qw, level, allowed, lone_row)


def level_scores(b):
    """score of every level >= 0 of a built case, ascending by level; asserts one score per level"""
    s = b.corpus.scores(b.qt, b.qw)
    out = []
    for lv in np.unique(b.level[b.level >= 0]):
        of = np.unique(s[b.level == lv])
        assert of.size == 1, lv
        out.append(int(of[0]))
    return out


def fillers(b):
    """the queries a case's query sits between in a batch, all over the case's own corpus: the plateau's term alone
    (every matching row: it overflows wherever anything does), the term of one row, the 64 terms at impact 255, a term
    without postings"""
    low = b.corpus.classes[0][0][0] if b.corpus.classes[0] else NQ
    return [([low], [1]), ([LONE], [255]), (sorted(LR.query_terms(R.MAX_QUERY_TERMS)), [255] * R.MAX_QUERY_TERMS), ([NONE], [9])]


BATCH = 130
BATCH_AT = (0, 64, 65, 129)       # where the case's query sits in the batch of 130; fillers[i % 4] elsewhere


def pack(qs):
    """(off int64, terms int32, impacts int32) of [(terms, impacts), ...]: what ImpactIndex.topk takes"""
    off = np.zeros(len(qs) + 1, np.int64)
    np.cumsum([len(t) for t, _ in qs], out=off[1:])
    return (off, np.asarray([x for t, _ in qs for x in t], np.int32), np.asarray([x for _, w in qs for x in w], np.int32))


# ---------------------------------------------------------------------------------------------------- pool cases
class PoolCase(NamedTuple):
    tok: np.ndarray              # [T, ld] float16
    cu: np.ndarray               # int32
    E: np.ndarray                # [V, ld_e] float16
    dim: int
    signed: bool


MIXED = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 8, 8, 8, 300, 3, 200]     # 1152 tokens
BATCH_EDGE_LENS = [16] * 7 + [20] + [16] * 7 + [20] + [8] * 14 + [12] + [8] * 15 + [10] + [5]
POOL_V = 300
REAL_V = 30522        # a BERT vocabulary: 239 tiles, the last of 58 rows
RUN_V = 17 * PT + 5   # SP_VRUN + 1 full tiles and one of 5 rows


def pool_planes(lens, Vt, dim, signed, seed, ld=None, ld_e=None):
    """integer-valued fp16 planes (every dot product exact).  `signed`: tests/test_sparse_gpu.py's construction --
    decoder rows >= 1 everywhere, chunks alternately all-negative and all-positive, so one leaked neighbour token, or
    one zero row past T or V, shows as a wrong sign.  Columns past `dim` (ld > dim) hold 7s and -7s that must not leak.
    A length of 0 or 513 in `lens` is a chunk the kernel refuses: it takes its rows like any other"""
    g = np.random.default_rng(seed)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(cu[-1])
    if signed:
        E = g.integers(1, 5, (Vt, dim))
        tok = g.integers(0, 5, (T, dim))
        tok[:, 0] = np.maximum(tok[:, 0], 1)
        tok *= np.repeat(np.where(np.arange(len(lens)) % 2 == 0, -1, 1), lens)[:, None]
    else:
        E = g.integers(-4, 5, (Vt, dim))
        tok = g.integers(-4, 5, (T, dim))

    def widen(x, w):
        if w is None or w == dim:
            return x.astype(np.float16)
        out = np.where(g.random((x.shape[0], w)) < 0.5, 7, -7).astype(np.float16)
        out[:, :dim] = x
        return out
    return PoolCase(widen(tok, ld), cu, widen(E, ld_e), dim, signed)


@functools.lru_cache(maxsize=None)
def pool_case(name):
    if name == "eights":                  # 256 queries of 8 tokens: 16 pieces in every tile, two batches
        return pool_planes([8] * 256, POOL_V, 64, True, 1)
    if name == "ones":                    # 128 pieces in tile 0, sixteen batches; one row in tile 1
        return pool_planes([1] * 129, POOL_V, 64, True, 2)
    if name == "batch_edges":             # tiles of 8, 9, 16 and 17 pieces, one of them across each tile edge
        return pool_planes(BATCH_EDGE_LENS, POOL_V, 64, False, 3)
    if name == "invalid_between":         # an empty and an over-long chunk among short ones
        return pool_planes([8] * 5 + [0] + [8] * 5 + [513] + [8] * 6, POOL_V, 64, False, 4)
    if name == "pitch_128_192":
        return pool_planes(MIXED[:8], POOL_V, 64, False, 5, ld=128, ld_e=192)
    if name == "pitch_192_128":
        return pool_planes(MIXED[:8], POOL_V, 64, True, 6, ld=192, ld_e=128)
    if name == "dim_128":
        return pool_planes(MIXED[:10], POOL_V, 128, False, 7)
    if name == "dim_1024":
        return pool_planes(MIXED[:8], POOL_V, 1024, True, 8)
    if name == "real_vocab":              # T = 1200: 10 token tiles x 239 vocabulary tiles
        return pool_planes(MIXED + [8] * 6, REAL_V, 64, False, 9)
    assert name == "run_tail"             # vrun = 16: a second workgroup with one tile of 5 rows
    return pool_planes(MIXED[:9], RUN_V, 64, False, 10)


POOL_CASES = ["eights", "ones", "batch_edges", "invalid_between", "pitch_128_192", "pitch_192_128", "dim_128",
              "dim_1024", "real_vocab", "run_tail"]


def pool_ref(pc):
    """float32 [n_chunks, V]: sparse_ref.pool over the dim columns"""
    return R.pool(pc.tok[:, : pc.dim], pc.cu, pc.E[:, : pc.dim]).astype(np.float32)


def pool_by_plane(pc):
    """the same maxima by another route: every logit of the whole plane (float32 is exact for these integers), then
    one segmented maximum over the rows of the good chunks, a block of vocabulary columns at a time"""
    tok, E = pc.tok[:, : pc.dim].astype(np.float32), pc.E[:, : pc.dim].astype(np.float32)
    cu = pc.cu.astype(np.int64)
    T = tok.shape[0]
    good = np.array([R.chunk_ok(int(cu[c]), int(cu[c + 1]), T) for c in range(cu.size - 1)])
    out = np.full((cu.size - 1, E.shape[0]), -np.inf, np.float32)
    rows = np.concatenate([np.arange(cu[c], cu[c + 1]) for c in np.nonzero(good)[0]])
    starts = np.concatenate([[0], np.cumsum((cu[1:] - cu[:-1])[good])[:-1]])
    for v0 in range(0, E.shape[0], 4096):
        out[good, v0: v0 + 4096] = np.maximum.reduceat(tok[rows] @ E[v0: v0 + 4096].T, starts, axis=0)
    return out


def pieces_per_tile(cu, T):
    """good chunk pieces (the rows of one chunk inside one 128-row tile) per token tile"""
    out = np.zeros((T + PT - 1) // PT, np.int64)
    for c in range(len(cu) - 1):
        s, e = int(cu[c]), int(cu[c + 1])
        if R.chunk_ok(s, e, T):
            out[s // PT: (e - 1) // PT + 1] += 1
    return out


def default_vrun(T, Vt, cus):
    """mmrag_internal_sparse_pool_ex's run of vocabulary tiles per workgroup on a device of `cus` compute units"""
    tt, vt = (T + PT - 1) // PT, (Vt + PT - 1) // PT
    return min(max(tt * vt // (4 * cus), 1), SP_VRUN)


EIGHTS_SAMPLE = (0, 1, 7, 8, 15, 16, 17, 23, 24, 31, 127, 128, 135, 136, 248, 255)   # chunks taken one per call


# ---------------------------------------------------------------------------------------------------- select cases
SELECT_MS = (1, 63, 64, 65, 255, 256)
SELECT_SCALE = 1024.0
TIE_RUN, TIE_IMPACT, TIE_FIRST = 3000, 7, 250
# (ordinal of a tie in ascending term id, its term): m = 63 | 64 | 65 ends on lanes 63 | 64 | 65 of step 5 (the last
# lane of wave 0, the first of wave 1, the one after), m = 255 | 256 on lanes 127 | 128 of step 20
TIE_PINS = ((1, TIE_FIRST), (63, 5 * SEL_T + 63), (64, 5 * SEL_T + 64), (65, 5 * SEL_T + 65),
            (255, 20 * SEL_T + 127), (256, 20 * SEL_T + 128), (257, 20 * SEL_T + 129), (TIE_RUN, REAL_V - 1))
# bits 0 and 31 of the words around both cuts; none is a pin
SKIP_AT = tuple(32 * w + b for w0 in ((5 * SEL_T + 64) // 32, (20 * SEL_T + 128) // 32) for w, b in
                ((w0 - 2, 31), (w0 - 1, 0), (w0, 31), (w0 + 1, 0)))
ABOVE = 10            # terms above the cut in chunk 1


def tie_terms(skip):
    """TIE_RUN ascending term ids outside `skip` through the pins"""
    free = np.nonzero(~skip)[0]
    out = []
    for (o0, t0), (o1, t1) in zip(TIE_PINS, TIE_PINS[1:]):
        between = free[(free > t0) & (free < t1)]
        pick = between[np.unique(np.linspace(0, between.size - 1, o1 - o0 - 1).astype(np.int64))] if o1 - o0 > 1 else []
        assert len(pick) == o1 - o0 - 1
        out += [t0] + list(pick)
    out.append(TIE_PINS[-1][1])
    assert not skip[out].any()
    return np.asarray(out, np.int64)


@functools.lru_cache(maxsize=None)
def select_case():
    """(pooled [4, V] float32, bias [V] float32, skip [V] bool, scale, the terms of chunk 2's special values: +inf, NaN,
    -inf, 3e38, then targets 255, 255.25, 256, 300, 254, 100, 1, 0.25).  Every finite w * scale lies within 0.25 of an
    integer.  Chunk 0: the tie run of TIE_RUN terms at impact 7 over every step, nothing above, impact 3 elsewhere in
    places, would-be 200s under the skip bits; chunk 1: the same with ABOVE terms of impact 9; chunk 2: +inf, NaN,
    saturated values and -inf; chunk 3: random targets up to 300"""
    g = np.random.default_rng(51)
    Vt, scale = REAL_V, SELECT_SCALE
    skip = g.random(Vt) < 0.03
    for _, t in TIE_PINS:
        skip[t] = False
    skip[list(SKIP_AT)] = True
    ties = tie_terms(skip)
    target = np.zeros((4, Vt), np.float64)
    low = np.setdiff1d(np.nonzero(g.random(Vt) < 0.2)[0], ties)
    for c in (0, 1):
        target[c, low] = 3
        target[c, ties] = TIE_IMPACT
        target[c, skip] = 200
    above = np.setdiff1d(np.nonzero(~skip)[0], ties)[np.linspace(100, Vt - 4000, ABOVE).astype(np.int64)]
    target[1, above] = 9
    target[3] = g.integers(0, 301, Vt)
    delta = g.uniform(-0.25, 0.25, (4, Vt))
    delta[target == 0] = np.abs(delta[target == 0])
    bias = (g.standard_normal(Vt) * 0.1).astype(np.float32)
    pooled = np.expm1((target + delta) / scale) - bias.astype(np.float64)
    neg = (target == 0) & (g.random((4, Vt)) < 0.5)
    pooled[neg] = -g.uniform(0.5, 4.0, int(neg.sum()))
    sp = pooled[2]
    sp[:] = -g.uniform(0.5, 4.0, Vt)
    at = np.nonzero(~skip)[0][np.linspace(3, Vt - 3000, 12).astype(np.int64)]
    sp[at[0]], sp[at[1]], sp[at[2]], sp[at[3]] = np.inf, np.nan, -np.inf, 3.0e38
    sp[at[4:8]] = np.expm1(np.array([255.0, 255.25, 256.0, 300.0]) / scale) - bias[at[4:8]]
    sp[at[8:]] = np.expm1(np.array([254.0, 100.0, 1.0, 0.25]) / scale) - bias[at[8:]]
    sp[Vt - 1] = np.inf
    return pooled.astype(np.float32), bias, skip, scale, at
