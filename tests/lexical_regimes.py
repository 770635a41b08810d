"""Structured corpora for the BM25 leg (csrc/lexical.hip) with fully determined answers.  Pure NumPy, no package import.

Signature classes.  A corpus is a list of classes, each a fixed sorted tuple of (term id, tf) pairs and a fixed dl, and
a layout that gives every row a class.  Two rows of one class present bm25_score_kernel with the same float32
operations in query order, so their device scores are bit-identical by construction.  More precisely the kernel sees a
row only through the pairs whose term the query holds, and through dl; with k1 = 0 the contribution of a term is
exactly its idf whatever tf and dl are.  `groups` therefore keys a row by (its pairs on query terms in query order,
dl), or with k1 = 0 by its query terms alone: rows of one group tie bit for bit on the device and exactly in the
float64 reference (tests/bm25_ref.py RefIndex.scores).

The gap condition (`expect` asserts it for every corpus, query and parameter set it is given): any two groups that
match the query have reference scores at least GAP = 1e-3 relative apart, 100 times the rtol of 1e-5 that
bm25_ref.assert_topk grants the float32 kernel against float64.  It concerns the inputs, not the kernel.  Under it the
answer is determined: groups by reference score descending, rows ascending inside a group (bm25_ref.topk).

Layouts are functions of (n, the number of planted rows, the constants below): they return a LEVEL per row (-2 a row
that cannot match, -1 an empty row with dl = 0, >= 0 a matching class whose score grows with the level), so a test
names the rows it expects without the data: `named_topk`.  tests/test_lexical_regimes_cpu.py proves that the names
are the reference's answer for every case of CASES.
"""
import functools
from typing import NamedTuple, Tuple

import numpy as np

import bm25_ref as R

# csrc/lexical.hip and csrc/candidate_select.h, restated: the tests compare them with mmrag_internal_lexical_limits
SCORE_R = 2048        # rows one workgroup of bm25_score_kernel scores
SCORE_TERMS = 128     # query terms looked up per chunk
SORT_LDS = 8192       # the longest postings list csr_sort_kernel sorts in LDS
SORT_GRID = 256       # workgroups of csr_sort_kernel
SCAN_TERMS = 1024     # terms csr_scan_kernel takes per step
LIMITS = {"score_rows": SCORE_R, "score_terms": SCORE_TERMS, "sort_lds": SORT_LDS, "sort_grid": SORT_GRID,
          "scan_terms": SCAN_TERMS}


def candidate_capacity(k):
    """candidate slots per query: 32 k, at least 16384, in whole 256s"""
    return (max(32 * k, 16384) + 255) // 256 * 256


GAP = 1e-3
V = 600               # vocabulary: query terms are 0 .. 598 in a scrambled order, NQ is in no query
NQ = V - 1
EMPTY, NOMATCH = -1, -2
RISE_LEVELS = 12


def query_terms(T):
    """T distinct term ids, not in id order (599 is prime)"""
    assert 0 <= T < V
    return [(37 * i + 11) % (V - 1) for i in range(T)]


def anchor_positions(T):
    """query positions whose terms the classes hold: both ends of the query and both sides of every chunk edge, the
    last term first (the lowest class then has postings in the last chunk only); every other query term has no posting"""
    out = []
    for p in (T - 1, 0, SCORE_TERMS, SCORE_TERMS - 1, 2 * SCORE_TERMS - 1, SCORE_TERMS + 1, 1, 2 * SCORE_TERMS, 64, 200):
        if 0 <= p < T and p not in out:
            out.append(p)
    return out[:6]


def level_classes(q, n_levels, mode):
    """classes 0 .. n_levels - 1 of rising score, then the EMPTY and the NOMATCH class.
    terms: level l holds the first l + 1 anchors (tf 2): another term, a higher score for any k1, b
    tf:    every anchor with tf = 1 + l (needs k1 > 0)
    dl:    every anchor with tf 2, dl falling with the level (needs k1 > 0 and b > 0)"""
    A = [q[p] for p in anchor_positions(len(q))]
    out = []
    for lv in range(n_levels):
        if mode == "terms":
            assert n_levels <= len(A), (n_levels, len(A))
            pairs, dl = [(t, 2) for t in A[: lv + 1]], 16
        elif mode == "tf":
            pairs, dl = [(t, 1 + lv) for t in A], 64
        else:
            assert mode == "dl"
            pairs, dl = [(t, 2) for t in A], 16 + 8 * (n_levels - 1 - lv)
        out.append((tuple(sorted(pairs + [(NQ, 1)])), dl))
    return out + [((), 0), (((NQ, 1),), 5)]


class Corpus:
    def __init__(self, classes, row_class):
        self.classes, self.row_class = list(classes), np.asarray(row_class, np.int64)
        self.n = self.row_class.size

    @functools.cached_property
    def log(self):
        """(off int64 [n + 1], ids int32, tfs int32, dl int32 [n]): what LexicalIndex.append_postings takes"""
        lens = np.array([len(p) for p, _ in self.classes], np.int64)[self.row_class]
        off = np.zeros(self.n + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        ids_c = [np.array([t for t, _ in p], np.int32) for p, _ in self.classes]
        tfs_c = [np.array([f for _, f in p], np.int32) for p, _ in self.classes]
        ids = np.concatenate([ids_c[c] for c in self.row_class] + [np.zeros(0, np.int32)])
        tfs = np.concatenate([tfs_c[c] for c in self.row_class] + [np.zeros(0, np.int32)])
        dl = np.array([d for _, d in self.classes], np.int32)[self.row_class]
        return off, ids, tfs, dl

    @functools.cached_property
    def ref(self):
        return R.RefIndex(*self.log)

    def groups(self, q, k1):
        """group id per row (-1: the row holds no query term)"""
        keys, of_class = {}, []
        for pairs, dl in self.classes:
            have = dict(pairs)
            on_q = tuple((t, have[t]) for t in q if t in have)
            if not on_q:
                of_class.append(-1)
                continue
            key = tuple(t for t, _ in on_q) if k1 == 0 else (on_q, dl)
            of_class.append(keys.setdefault(key, len(keys)))
        return np.array(of_class, np.int64)[self.row_class]

    def df(self, live):
        """live rows per term [V]"""
        off, ids, _, _ = self.log
        return np.bincount(ids[np.repeat(np.asarray(live, bool), np.diff(off))], minlength=V)


def expect(corpus, q, live=None, k1=1.2, b=0.75):
    """(acc float64 [n], matched bool [n], group [n]) of query q with the statistics of the `live` rows; asserts the
    gap condition"""
    live = np.ones(corpus.n, bool) if live is None else np.asarray(live, bool)
    acc, matched = corpus.ref.scores(q, live, k1, b)
    group = corpus.groups(q, k1)
    assert np.array_equal(matched, group >= 0)
    level = []
    for g in np.unique(group[matched]):
        s = acc[group == g]
        assert np.all(s == s[0]) and s[0] > 0, g          # one group, one float64 score
        level.append(s[0])
    level = np.sort(np.array(level))
    assert np.all(np.diff(level) >= GAP * level[1:]), level
    return acc, matched, group


def named_topk(level, allowed, k):
    """the answer by the layout alone: matching allowed rows by level descending, then row ascending"""
    rows = np.nonzero((level >= 0) & np.asarray(allowed, bool))[0]
    return rows[np.lexsort((rows, -level[rows]))][:k]


def alive_words(allowed):
    """the alive bitmap as the kernels read it: bit r & 31 of int32 word r >> 5"""
    bits = np.zeros((allowed.size + 31) // 32 * 32, np.uint8)
    bits[: allowed.size] = allowed
    return np.packbits(bits, bitorder="little").view(np.int32)


# ---------------------------------------------------------------------------------------------------- row layouts
def blocks(n):
    return (n + SCORE_R - 1) // SCORE_R


def planted_rows(where, n, W):
    """the rows of the planted winners (ascending)"""
    if where == "block_edges":       # both sides of every block edge and the last row, then evenly spread ones
        rows = [r for r in (0, SCORE_R - 1, SCORE_R, 2 * SCORE_R - 1, 2 * SCORE_R, n - 1) if 0 <= r < n]
        rows += [(j + 1) * n // (W + 1) for j in range(W)]
        return np.sort(np.array(list(dict.fromkeys(rows))[: max(W, 6)], np.int64))
    if where == "one_block":         # all in the last, partial block
        s = (n - 1) // SCORE_R * SCORE_R
        return s + np.unique(np.linspace(0, n - 1 - s, min(W, n - s)).astype(np.int64))
    if where == "one_per_block":
        return np.array([b * SCORE_R + (b * 997 + 1) % min(SCORE_R, n - b * SCORE_R) for b in range(blocks(n))], np.int64)
    assert where == "word_edges"     # a run across the first block edge
    return np.arange(SCORE_R - 70, SCORE_R + 70, dtype=np.int64)


def word_edges_allowed(n):
    """of the run of `word_edges`, only bits 31, 0, 10 and 21 of every word are alive: rows 31 | 32 and 63 | 64 of the
    words on both sides of the block edge win, with dead rows of the same classes between them; the pattern does not
    repeat after 16 bits"""
    allowed = np.ones(n, bool)
    run = planted_rows("word_edges", n, 0)
    allowed[run] = np.isin(run % 32, (31, 0, 10, 21))
    return allowed


def layout(name, n, W):
    """level per row"""
    r = np.arange(n)
    if name == "plateau":
        return np.zeros(n, np.int64)
    if name == "two_level":              # W high rows over all blocks above a full plateau
        level = np.zeros(n, np.int64)
        level[(2 * np.arange(W) + 1) * n // (2 * W)] = 1
        level[n - 1] = 1                 # W + 1 with the last row: the partial block has one too
        return level
    if name == "rising":
        return r * RISE_LEVELS // n
    if name == "falling":
        return RISE_LEVELS - 1 - r * RISE_LEVELS // n
    if name.startswith("planted:"):      # winners of levels 1, 2, 3 in turn above a low plateau
        level = np.zeros(n, np.int64)
        rows = planted_rows(name[8:], n, W)
        level[rows] = 1 + np.arange(rows.size) % 3
        if name[8:] == "one_per_block":   # and rows without text, or without a query term, in the plateau
            level[(r % 7 == 3) & (level == 0)] = EMPTY
            level[(r % 11 == 5) & (level == 0)] = NOMATCH
        return level
    if name == "dead_term":              # level 2, the best class and the only holder of its term, is dead throughout
        level = np.zeros(n, np.int64)
        level[planted_rows("block_edges", n, W)] = 1
        dead = np.unique(np.concatenate([(np.arange(40) * 97 + 13) % n, [SCORE_R - 2, SCORE_R + 1, n - 2]]))
        level[dead[(dead < n) & (level[np.minimum(dead, n - 1)] == 0)]] = 2
        return level
    assert name == "sparse"              # one row with text, the last
    level = np.full(n, EMPTY, np.int64)
    level[n - 1] = 0
    return level


def delete_set(level):
    """rows to delete on a planted layout: every third winner, the whole of level 3, every fifth plateau row"""
    win = np.nonzero(level >= 1)[0]
    low = np.nonzero(level == 0)[0]
    dead = np.zeros(level.size, bool)
    dead[win[::3]] = True
    dead[level == 3] = True
    dead[low[::5]] = True
    return dead


# ---------------------------------------------------------------------------------------------------- the cases
class Case(NamedTuple):
    id: str
    layout: str
    n: int
    T: int                       # query terms
    ks: Tuple[int, ...]
    W: int = 9                   # planted rows
    k1: float = 1.2
    b: float = 0.75
    mask: str = "none"           # none | masked (alive bits only) | deleted (delete_rows and alive bits)
    overflow: bool = False       # more matches than candidate_capacity(k) for every k <= 512 of ks
    mirror: bool = False         # the query reversed


KS = (1, 5, 100, 512)     # every case but `sparse` (one match) runs them all; past the matches the answer is padding
CASES = [
    Case("plateau-100", "plateau", 100, 1, KS),                       # k = 512: 100 hits, then padding
    Case("plateau-2048", "plateau", 2048, 1, KS),
    Case("plateau-2049", "plateau", 2049, 128, KS),
    Case("plateau-4099", "plateau", 4099, 1, KS),
    Case("plateau-16640", "plateau", 16640, 1, KS + (4096,), overflow=True),
    Case("two-level-4099", "two_level", 4099, 129, KS, W=50),
    Case("two-level-16640", "two_level", 16640, 257, KS, W=256, overflow=True),
    Case("rising-4099", "rising", 4099, 1, KS),
    Case("falling-4099", "falling", 4099, 128, KS),
    Case("block-edges-4099", "planted:block_edges", 4099, 257, KS + (4096,)),
    Case("block-edges-100", "planted:block_edges", 100, 256, KS),
    Case("one-block-4099", "planted:one_block", 4099, 257, KS),
    Case("one-block-2049", "planted:one_block", 2049, 1, KS),
    Case("one-per-block-16640", "planted:one_per_block", 16640, 128, KS),
    Case("word-edges-4099", "planted:word_edges", 4099, 129, KS, mask="masked"),
    Case("dead-term-4099", "dead_term", 4099, 257, KS, mask="deleted"),
    Case("sparse-1", "sparse", 1, 1, (1, 5)),
    Case("sparse-2048", "sparse", 2048, 257, (1, 5)),
    Case("sparse-2049", "sparse", 2049, 1, (1, 5)),
    Case("split-4099", "split", 4099, 257, KS),
    Case("split-mirror-4099", "split", 4099, 257, KS, mirror=True),
    Case("k1zero-ties-4099", "k1zero", 4099, 129, KS, k1=0.0),
]
for _k1, _b in ((0.0, 0.75), (1.2, 0.0), (1.2, 1.0)):
    CASES.append(Case(f"block-edges-4099-k1={_k1}-b={_b}", "planted:block_edges", 4099, 257, KS, k1=_k1, b=_b))
    CASES.append(Case(f"plateau-4099-k1={_k1}-b={_b}", "plateau", 4099, 1, KS, k1=_k1, b=_b))
CASE_IDS = [c.id for c in CASES]


class Built(NamedTuple):
    corpus: Corpus
    q: list
    level: np.ndarray            # per row; a level names the rank of a row's class for this query
    live: np.ndarray             # the rows the statistics count
    allowed: np.ndarray          # the rows that may be returned


def split_corpus(n, q):
    """block 1 (rows 2048 .. 4095) holds query terms of positions >= 129 only: chunk 0 of the 257-term query has no
    posting there while chunks 1 and 2 have; of the reversed query it is chunks 1 and 2 that have none.  The other
    blocks hold terms of every chunk.  Levels are the classes' ranks, which `build` takes from the reference."""
    assert len(q) == 2 * SCORE_TERMS + 1 and blocks(n) >= 3
    t = lambda *ps: tuple(sorted([(q[p], 2) for p in ps] + [(NQ, 1)]))   # noqa: E731
    classes = [(t(256), 16),                                  # 0 late, the plateau of block 1
               (t(129, 200, 256), 16),                        # 1 late, few
               (t(0, 127), 16),                               # 2 early, the plateau elsewhere
               (t(0, 5, 127, 128, 255, 256), 16)]             # 3 every chunk, few
    r = np.arange(n)
    in1 = (r >= SCORE_R) & (r < 2 * SCORE_R)
    row_class = np.where(in1, 0, 2)
    row_class[in1 & np.isin(r % SCORE_R, (0, 1, 77, 1000, SCORE_R - 1))] = 1
    row_class[~in1 & np.isin(r % SCORE_R, (0, 2, 500, SCORE_R - 1))] = 3
    return Corpus(classes, row_class)


def k1zero_corpus(n, q):
    """with k1 = 0 every row holding both q[0] and q[128] ties, whatever its tf and dl: three such classes interleaved
    over every block are one group; a few rows hold a third term (above), every tenth row q[0] alone (below)"""
    a, c, e = q[0], q[SCORE_TERMS], q[64]
    classes = [(tuple(sorted([(a, 1), (c, 1)])), 10), (tuple(sorted([(a, 5), (c, 3), (NQ, 2)])), 90),
               (tuple(sorted([(a, 2), (c, 9)])), 33), (((a, 2),), 7), (tuple(sorted([(a, 1), (c, 1), (e, 4)])), 20)]
    r = np.arange(n)
    row_class = r % 3
    row_class[r % 10 == 9] = 3
    row_class[[17, SCORE_R - 1, SCORE_R, n - 1]] = 4
    level = np.array([1, 1, 1, 0, 2])[row_class]
    return Corpus(classes, row_class), level


@functools.lru_cache(maxsize=None)
def build(case):
    n = case.n
    q = query_terms(case.T)
    if case.mirror:
        q = q[::-1]
    live = allowed = np.ones(n, bool)
    if case.layout == "split":
        corpus = split_corpus(n, query_terms(case.T))
        acc, _, _ = expect(corpus, q, live, case.k1, case.b)
        by_class = np.array([acc[np.nonzero(corpus.row_class == c)[0][0]] for c in range(4)])
        level = np.argsort(np.argsort(by_class))[corpus.row_class]
    elif case.layout == "k1zero":
        corpus, level = k1zero_corpus(n, q)
    else:
        level = layout(case.layout, n, case.W)
        n_levels = int(level.max()) + 1
        mode = "dl" if case.layout == "falling" else "terms" if n_levels <= min(case.T, 6) else "tf"
        assert mode == "terms" or case.k1 > 0
        classes = level_classes(q, n_levels, mode)
        corpus = Corpus(classes, np.where(level >= 0, level, np.where(level == EMPTY, n_levels, n_levels + 1)))
    if case.layout == "planted:word_edges":
        allowed = word_edges_allowed(n)
    if case.layout == "dead_term":
        allowed = level != 2
    if case.mask == "deleted":
        live = allowed
    return Built(corpus, q, level, live, allowed)


def chunk_has_postings(corpus, q, chunk, block):
    """does any term of q[chunk * SCORE_TERMS ..) have a posting in rows [block * SCORE_R, (block + 1) * SCORE_R)?"""
    terms = set(q[chunk * SCORE_TERMS: (chunk + 1) * SCORE_TERMS])
    classes = np.unique(corpus.row_class[block * SCORE_R: (block + 1) * SCORE_R])
    return any(t in terms for c in classes for t, _ in corpus.classes[c][0])


# ---------------------------------------------------------------------------------------------------- CSR build logs
CSR_N = 8199                     # not a multiple of 32; the last bitmap word holds rows 8192 .. 8198
CSR_V = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
CSR_EMPTY_ROWS = (5, 4096, 8000)  # rows without postings (the longest list leaves room for no more than 6)
CSR_COUNTS = (0, 1, 2, 4095, 4096, 4097, 0, 8191, 8192, 8193)   # a term's postings, around every path edge of the sort


def csr_counts(Vt):
    """postings per term: CSR_COUNTS spread over the term ids (an empty term first, one in the middle, the longest list
    last), t % 5 elsewhere: more empty terms, and 1023 | 1024 are not empty"""
    if Vt == 1:
        return np.array([SORT_LDS + 1], np.int64)
    counts = np.arange(Vt, dtype=np.int64) % 5
    counts[np.linspace(0, Vt - 1, len(CSR_COUNTS)).astype(np.int64)] = CSR_COUNTS
    return counts


def csr_log(Vt, n=CSR_N):
    """(off, ids, tfs, dl) of n rows whose terms have csr_counts(Vt) postings; the term with 8193 holds the rows of the
    last bitmap word; rows are in no order a term's postings could inherit"""
    counts = csr_counts(Vt)
    g = np.random.default_rng(Vt)
    pool = np.setdiff1d(np.arange(n), CSR_EMPTY_ROWS)         # rows that may hold postings
    rows, terms = [], []
    for t in np.nonzero(counts)[0]:
        c = int(counts[t])
        if c <= 4:
            rr = pool[(t * 131 + np.arange(c) * 1009) % pool.size]
        elif c == SORT_LDS + 1:
            tail = np.arange(n - 7, n)
            rr = np.concatenate([tail, g.choice(pool[pool < n - 7], c - 7, replace=False)])
        else:
            rr = g.choice(pool, c, replace=False)
        rows.append(rr)
        terms.append(np.full(c, t))
    rows = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
    terms = np.concatenate(terms + [np.zeros(0, np.int64)]).astype(np.int64)
    order = np.lexsort((terms, rows))
    rows, terms = rows[order], terms[order]
    tfs = 1 + (rows * 7 + terms * 13) % 5
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=off[1:])
    dl = np.bincount(rows, weights=tfs, minlength=n).astype(np.int32)
    return off, terms.astype(np.int32), tfs.astype(np.int32), dl
