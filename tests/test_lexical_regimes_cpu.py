"""CPU: the generators of tests/lexical_regimes.py and their expected answers, before any kernel is involved.

For every case the GPU file runs: the gap condition holds (lexical_regimes.expect asserts it), the rows the layout names
are the float64 reference's top-k, the overflow cases overflow, the split queries leave the intended chunks without
postings in the intended block, and the restated constants are the library's."""
import numpy as np
import pytest

import bm25_ref as R
import lexical_regimes as LR


@pytest.fixture(scope="module")
def native():
    from multimodal_rag_amd import _native, build

    build.build(verbose=False)
    _native.lib()
    return _native


def test_restated_constants(native):
    from multimodal_rag_amd.lexical import lexical_limits

    assert lexical_limits() == LR.LIMITS
    for k in (1, 5, 100, 512, 513, 4096):
        assert native.candidate_capacity(k) == LR.candidate_capacity(k)


def test_limits_export_is_internal():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "mmrag_internal_lexical_limits" not in open(os.path.join(root, "include", "mmrag.h")).read()


@pytest.mark.parametrize("case", LR.CASES, ids=LR.CASE_IDS)
def test_names_are_the_reference_answer(case):
    c = LR.build(case)
    acc, matched, group = LR.expect(c.corpus, c.q, c.live, case.k1, case.b)      # asserts the gap condition
    assert np.array_equal(matched, c.level >= 0)
    hits = int((matched & c.allowed).sum())
    for k in case.ks:
        want = R.topk(acc, matched, c.allowed, k)
        assert np.array_equal(want, LR.named_topk(c.level, c.allowed, k))
        assert want.size == min(k, hits)
        if case.overflow and k <= 512:
            assert hits > LR.candidate_capacity(k)
    # a group is a set of rows of one level; the reference scores rise with the level
    for g in np.unique(group[matched]):
        assert np.unique(c.level[group == g]).size == 1
    lv = c.level[matched]
    assert np.all(np.diff(acc[matched][np.argsort(lv, kind="stable")]) >= 0)


@pytest.mark.parametrize("case", LR.CASES, ids=LR.CASE_IDS)
def test_first_term_alone_is_a_regime_too(case):
    """the GPU file also sends every case's first query term alone, in a batch with the whole query"""
    c = LR.build(case)
    LR.expect(c.corpus, c.q[:1], c.live, case.k1, case.b)


def test_batch_queries_are_regimes():
    c = LR.build(LR.CASES[LR.CASE_IDS.index("block-edges-4099")])
    for q in (c.q[-1:], c.q, c.q[: LR.SCORE_TERMS + 1]):
        acc, matched, _ = LR.expect(c.corpus, q)
        assert matched.sum() > 0
    acc, matched, group = LR.expect(c.corpus, c.q[-1:])
    assert matched.all() and np.unique(group).size == 1                    # the last term: every row, one plateau


@pytest.mark.parametrize("case_id", ["block-edges-4099", "one-block-4099", "one-per-block-16640", "word-edges-4099"])
def test_delete_sets(case_id):
    """the planted layouts after deletes: winners, a whole class (its term dies out) and plateau rows go"""
    case = LR.CASES[LR.CASE_IDS.index(case_id)]
    c = LR.build(case)
    dead = LR.delete_set(c.level) | ~c.allowed
    live = ~dead
    win = c.level >= 1
    assert dead[win].any() and live[win].any() and dead[c.level == 3].all() and (c.level == 3).any()
    assert dead[c.level == 0].any() and live[c.level == 0].sum() > 100
    df0, df1 = c.corpus.df(np.ones(c.corpus.n, bool)), c.corpus.df(live)
    assert ((df0 > 0) & (df1 == 0)).sum() == 1 and (df1 <= df0).all() and (df1 < df0).sum() >= 3
    acc, matched, _ = LR.expect(c.corpus, c.q, live, case.k1, case.b)
    for k in case.ks:
        assert np.array_equal(R.topk(acc, matched, live, k), LR.named_topk(c.level, live, k))


def test_layouts_are_where_they_claim():
    S = LR.SCORE_R
    n = 4099
    rows = LR.planted_rows("block_edges", n, 9)
    assert {0, S - 1, S, 2 * S - 1, 2 * S, n - 1} <= set(rows.tolist()) and rows.size == 9
    assert np.array_equal(LR.named_topk(LR.layout("plateau", 16640, 0), np.ones(16640, bool), 512), np.arange(512))
    assert LR.planted_rows("one_block", n, 9).min() >= 2 * S and n - 1 in LR.planted_rows("one_block", n, 9)
    per = LR.planted_rows("one_per_block", 16640, 0)
    assert np.array_equal(per // S, np.arange(LR.blocks(16640))) and LR.blocks(16640) == 9
    high = np.nonzero(LR.layout("two_level", n, 50))[0]
    assert high.size == 51 and n - 1 in high and np.unique(high // S).size == LR.blocks(n)
    allowed = LR.word_edges_allowed(n)
    for r in (S - 33, S - 32, S - 1, S, S + 31, S + 32, S + 63, S + 64):   # bits 31 | 0 on both sides of the block edge
        assert allowed[r]
    run = LR.planted_rows("word_edges", n, 0)
    alive_run = run[allowed[run]]
    assert np.all(np.diff(alive_run)[np.diff(alive_run) > 1] >= 10)          # dead rows between the pairs
    assert not np.array_equal(allowed[run], allowed[run - 16])               # the pattern has no period of 16 bits
    words = LR.alive_words(allowed)
    assert words.size == (n + 31) // 32 and all(((int(words[r >> 5]) >> (r & 31)) & 1) == allowed[r] for r in run)
    c = LR.build(LR.CASES[LR.CASE_IDS.index("dead-term-4099")])
    top = c.level == 2
    assert top.sum() >= 40 and np.unique(np.nonzero(top)[0] // S).size == 3 and not c.live[top].any()
    held = [t for t, _ in c.corpus.classes[2][0] if t != LR.NQ and t not in dict(c.corpus.classes[1][0])]
    assert len(held) == 1 and c.corpus.df(c.live)[held[0]] == 0 and c.corpus.df(np.ones(n, bool))[held[0]] == top.sum()
    for m in (1, 2048, 2049):
        lv = LR.layout("sparse", m, 0)
        assert (lv >= 0).sum() == 1 and lv[m - 1] == 0 and (lv[: m - 1] == LR.EMPTY).all()
    c = LR.build(LR.CASES[LR.CASE_IDS.index("k1zero-ties-4099")])
    tie = c.corpus.groups(c.q, 0.0)
    big = np.nonzero(tie == tie[0])[0]
    assert np.unique(c.corpus.row_class[big]).size == 3 and big.size > 3000 and np.unique(big // S).size == 3
    assert np.unique(c.corpus.groups(c.q, 1.2)[big]).size == 3            # apart again once tf and dl count


def test_split_queries_leave_chunks_empty():
    T = LR.SCORE_TERMS
    c = LR.build(LR.CASES[LR.CASE_IDS.index("split-4099")])
    m = LR.build(LR.CASES[LR.CASE_IDS.index("split-mirror-4099")])
    assert len(c.q) == 2 * T + 1 and m.q == c.q[::-1]
    has = lambda b, blk: [LR.chunk_has_postings(b.corpus, b.q, ch, blk) for ch in range(3)]   # noqa: E731
    assert has(c, 1) == [False, True, True]       # a chunk skipped, the accumulator zeroed in a later one
    assert has(m, 1) == [True, False, False]      # zeroed at once, then two chunks skipped
    assert has(c, 0) == [True, True, True] and has(m, 0) == [True, True, True]
    assert has(c, 2) == [True, True, True]
    # the low classes of the anchor layouts hold the query's last term alone: chunks 0 and 1 are both skipped in a
    # block of plateau rows only, and the accumulator is zeroed in the last chunk
    p = LR.build(LR.CASES[LR.CASE_IDS.index("one-block-4099")])
    blk = next(b for b in range(LR.blocks(p.corpus.n)) if not p.level[b * LR.SCORE_R: (b + 1) * LR.SCORE_R].any())
    assert [LR.chunk_has_postings(p.corpus, p.q, ch, blk) for ch in range(3)] == [False, False, True]


@pytest.mark.parametrize("Vt", LR.CSR_V)
def test_csr_logs(Vt):
    off, ids, tfs, dl = LR.csr_log(Vt)
    counts = np.bincount(ids, minlength=Vt)
    assert np.array_equal(counts, LR.csr_counts(Vt)) and off[-1] == ids.size and dl.size == LR.CSR_N
    assert LR.CSR_N % 32 != 0 and LR.SORT_LDS + 1 in counts
    if Vt > 1:
        assert set(LR.CSR_COUNTS) <= set(counts.tolist()) and counts[0] == 0 and 0 in counts[1:-1].tolist()
        assert (np.diff(off) == 0).any()                                   # rows without postings
    if Vt > LR.SCAN_TERMS:
        assert counts[LR.SCAN_TERMS - 1] > 0 and counts[LR.SCAN_TERMS] > 0
    longest = int(np.argmax(counts))
    rows = np.repeat(np.arange(LR.CSR_N), np.diff(off))
    assert set(range(LR.SORT_LDS, LR.CSR_N)) <= set(rows[ids == longest].tolist())   # the last, partial bitmap word
    for r in (0, 1, LR.CSR_N - 1):                                         # terms ascending and distinct inside a row
        assert np.all(np.diff(ids[off[r]: off[r + 1]]) > 0)
    assert np.all(np.diff(rows * 4096 + ids) > 0)
