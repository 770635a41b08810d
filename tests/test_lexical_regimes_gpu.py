"""GPU: csrc/lexical.hip at its edges, on the structured corpora of tests/lexical_regimes.py whose answers are fully
determined (tests/test_lexical_regimes_cpu.py proves the generators): the strict order "descending, ties to the lower
row", the term-chunk loop of bm25_score_kernel, its row blocks, df under deletes per term, both sort paths and the scan
of the CSR build at their thresholds, and mmrag_rows_dot against float64.

Every LexicalIndex here is built through append_postings alone."""
import math

import numpy as np
import pytest
import torch

import bm25_ref as R
import lexical_regimes as LR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


def new_index(dev, corpus):
    """the corpus appended in two pieces (one when it has a single row)"""
    from multimodal_rag_amd.lexical import LexicalIndex

    off, ids, tfs, dl = corpus.log
    lex = LexicalIndex(dev)
    m = corpus.n * 2 // 5
    for lo, hi in ((0, m), (m, corpus.n)):
        if hi > lo:
            lex.append_postings(off[lo: hi + 1] - off[lo], ids[off[lo]: off[hi]], tfs[off[lo]: off[hi]], dl[lo:hi])
    assert lex.n == corpus.n and lex.n_terms == LR.V
    return lex


def pack(qs):
    off = np.zeros(len(qs) + 1, np.int32)
    np.cumsum([len(q) for q in qs], out=off[1:])
    return off, np.asarray([t for q in qs for t in q], np.int32)


def search(lex, qs, k, allowed=None, k1=1.2, b=0.75):
    alive = None if allowed is None or allowed.all() else torch.from_numpy(LR.alive_words(allowed)).to(lex.device)
    s, r = lex.topk_ids(*pack(qs), k, alive, k1, b)
    return s.cpu(), r.cpu()


class Regimes:
    """what the search tests of this module share: one LexicalIndex (and its workspaces) per corpus, used by every
    regime over that corpus whatever its query, B, k and parameters, and the first answer of every (case, k)"""

    def __init__(self, dev):
        self.dev, self.index, self.first = dev, {}, {}

    def index_of(self, case):
        key = (case.layout, case.n, case.T, case.W, case.mask == "deleted")
        if key not in self.index:
            c = LR.build(case)
            lex = new_index(self.dev, c.corpus)
            if case.mask == "deleted":
                lex.delete_rows(np.nonzero(~c.live)[0])
            self.index[key] = lex
        return self.index[key]

    def run(self, case, k):
        c = LR.build(case)
        return search(self.index_of(case), [c.q], k, c.allowed, case.k1, case.b)

    def first_run(self, case, k):
        if (case.id, k) not in self.first:
            self.first[(case.id, k)] = self.run(case, k)
        return self.first[(case.id, k)]


@pytest.fixture(scope="module")
def regimes(dev):
    shared = Regimes(dev)
    yield shared
    shared.index.clear()      # the indexes leave the device with the module


def test_restated_constants(dev):
    from multimodal_rag_amd import _native
    from multimodal_rag_amd.lexical import lexical_limits

    assert lexical_limits() == LR.LIMITS
    for k in (1, 5, 100, 512, 4096):
        assert _native.candidate_capacity(k) == LR.candidate_capacity(k)


@pytest.mark.parametrize("case", LR.CASES, ids=LR.CASE_IDS)
def test_search_regimes(regimes, case):
    c = LR.build(case)
    acc, matched, group = LR.expect(c.corpus, c.q, c.live, case.k1, case.b)
    lex = regimes.index_of(case)
    for k in case.ks:
        s, r = regimes.first_run(case, k)
        R.assert_topk_strict(s[0].numpy(), r[0].numpy(), acc, matched, c.allowed, k, group)
        want = LR.named_topk(c.level, c.allowed, k)
        assert np.array_equal(r[0].numpy()[: want.size], want)
    # the same index and workspace with another B: the query between an empty one and its own first term
    k = case.ks[-1]
    s1, r1 = search(lex, [c.q[:1]], k, c.allowed, case.k1, case.b)
    s3, r3 = search(lex, [[], c.q, c.q[:1]], k, c.allowed, case.k1, case.b)
    s, r = regimes.first_run(case, k)
    assert torch.equal(s3[1], s[0]) and torch.equal(r3[1], r[0])
    assert torch.equal(s3[2], s1[0]) and torch.equal(r3[2], r1[0])
    assert bool((r3[0] == -1).all()) and bool(torch.isneginf(s3[0]).all())
    a1, m1, g1 = LR.expect(c.corpus, c.q[:1], c.live, case.k1, case.b)
    R.assert_topk_strict(s1[0].numpy(), r1[0].numpy(), a1, m1, c.allowed, k, g1)


def test_reverse_sweep_gives_the_same_bits(regimes):
    first = {(case.id, k): regimes.first_run(case, k) for case in LR.CASES for k in case.ks}
    for case in reversed(LR.CASES):
        for k in reversed(case.ks):
            s, r = regimes.run(case, k)
            assert torch.equal(s, first[(case.id, k)][0]) and torch.equal(r, first[(case.id, k)][1]), (case.id, k)


@pytest.mark.parametrize("k", LR.KS)
def test_batch_of_1_257_and_no_terms(regimes, k):
    case = LR.CASES[LR.CASE_IDS.index("block-edges-4099")]
    c = LR.build(case)
    lex = regimes.index_of(case)
    qs = [c.q[-1:], c.q, [], c.q[: LR.SCORE_TERMS + 1]]
    sb, rb = search(lex, qs, k)
    for i, q in enumerate(qs):
        s1, r1 = search(lex, [q], k)
        assert torch.equal(s1[0], sb[i]) and torch.equal(r1[0], rb[i]), i      # no answer depends on the batch
        if q:
            acc, matched, group = LR.expect(c.corpus, q)
            R.assert_topk_strict(sb[i].numpy(), rb[i].numpy(), acc, matched, c.allowed, k, group)
        else:
            assert bool((rb[i] == -1).all()) and bool(torch.isneginf(sb[i]).all())
    assert np.array_equal(rb[0].numpy(), np.arange(k))                           # every row holds the last term: a plateau


DELETE_CASES = ["block-edges-4099", "one-block-4099", "one-per-block-16640", "word-edges-4099"]


@pytest.mark.parametrize("case_id", DELETE_CASES)
def test_deletes_df_per_term_and_compaction(dev, case_id):
    case = LR.CASES[LR.CASE_IDS.index(case_id)]
    c = LR.build(case)
    lex = new_index(dev, c.corpus)
    assert np.array_equal(lex.df_host(), c.corpus.df(np.ones(c.corpus.n, bool)))
    dead = LR.delete_set(c.level) | ~c.allowed
    live = ~dead
    lex.delete_rows(np.nonzero(dead)[0])
    want_df = c.corpus.df(live)
    assert (want_df[: LR.V - 1][c.corpus.df(np.ones(c.corpus.n, bool))[: LR.V - 1] > 0] == 0).any()   # a term died out
    assert np.array_equal(lex.df_host(), want_df)                              # per term, not sorted
    acc, matched, group = LR.expect(c.corpus, c.q, live, case.k1, case.b)
    before = {}
    for k in case.ks:
        s, r = search(lex, [c.q], k, live)
        R.assert_topk_strict(s[0].numpy(), r[0].numpy(), acc, matched, live, k, group)
        assert np.array_equal(r[0].numpy()[: min(k, int((matched & live).sum()))], LR.named_topk(c.level, live, k))
        before[k] = (s, r)
    keep = np.nonzero(live)[0]
    lex.compact(keep)
    assert lex.n == keep.size and np.array_equal(lex.df_host(), want_df)
    new_row = np.cumsum(live) - 1
    for k in case.ks:
        s, r = search(lex, [c.q], k)
        old = before[k][1][0].numpy()
        assert torch.equal(s, before[k][0])                                      # the same bits for the same live rows
        assert np.array_equal(r[0].numpy(), np.where(old >= 0, new_row[np.maximum(old, 0)], -1))


# ------------------------------------------------------------------------------------------------ CSR build
def csr_build_twice(dev, off, ids, tfs, n, Vt):
    """mmrag_lexical_csr_build on a workspace full of ones, twice on the same workspace: (term_off, post_row, post_tf)
    of both runs"""
    from multimodal_rag_amd import _native

    L = _native.lib()
    P = int(ids.size)
    d_off = torch.from_numpy(off).to(dev)
    d_ids = torch.from_numpy(np.concatenate([ids, np.zeros(1, np.int32)])).to(dev)
    d_tfs = torch.from_numpy(np.concatenate([tfs, np.zeros(1, np.int32)])).to(dev)
    need = int(L.mmrag_lexical_csr_build_workspace_bytes(n, Vt))
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    out = []
    for _ in range(2):
        term_off = torch.full((Vt + 1,), -7, dtype=torch.int64, device=dev)
        post_row = torch.full((max(P, 1),), -7, dtype=torch.int32, device=dev)
        post_tf = torch.full((max(P, 1),), -7, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _native._check(L.mmrag_lexical_csr_build(d_off.data_ptr(), d_ids.data_ptr(), d_tfs.data_ptr(), n, P, Vt,
                                                     term_off.data_ptr(), post_row.data_ptr(), post_tf.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), _native._stream_ptr(torch.device(dev))),
                           "mmrag_lexical_csr_build")
        out.append((term_off.cpu().numpy(), post_row.cpu().numpy()[:P], post_tf.cpu().numpy()[:P]))
    return out


@pytest.mark.parametrize("Vt", LR.CSR_V)
def test_csr_build_at_the_path_edges(dev, Vt):
    off, ids, tfs, dl = LR.csr_log(Vt)
    ref = R.RefIndex(off, ids, tfs, dl)                  # NumPy's stable sort by term: rows ascending inside a term
    want_off = np.searchsorted(ref.t_sorted, np.arange(Vt + 1))
    for term_off, post_row, post_tf in csr_build_twice(dev, off, ids, tfs, LR.CSR_N, Vt):
        assert np.array_equal(term_off, want_off)
        assert np.array_equal(post_row, ref.p_rows)
        assert np.array_equal(post_tf, ref.p_tf)


@pytest.mark.parametrize("n,Vt", [(5, 3), (1, 1), (100, 257)])
def test_csr_build_of_an_empty_log(dev, n, Vt):
    empty = np.zeros(0, np.int32)
    for term_off, post_row, post_tf in csr_build_twice(dev, np.zeros(n + 1, np.int64), empty, empty, n, Vt):
        assert np.array_equal(term_off, np.zeros(Vt + 1, np.int64)) and post_row.size == 0 and post_tf.size == 0


def test_index_builds_the_same_csr(dev):
    """the path the product takes (LexicalIndex._ensure_csr through a search), on the log with every edge"""
    from multimodal_rag_amd.lexical import LexicalIndex

    Vt = 1025
    off, ids, tfs, dl = LR.csr_log(Vt)
    ref = R.RefIndex(off, ids, tfs, dl)
    lex = LexicalIndex(dev)
    lex.append_postings(off, ids, tfs, dl)
    assert lex.n_terms == Vt and np.array_equal(lex.df_host(), np.bincount(ids, minlength=Vt))
    live = np.ones(LR.CSR_N, bool)
    long_term, short_term = Vt - 1, int(np.nonzero(LR.csr_counts(Vt) == 2)[0][0])
    for q in ([long_term], [short_term], [short_term, long_term, 0]):
        s, r = search(lex, [q], 100)
        R.assert_topk(s[0].numpy(), r[0].numpy(), *ref.scores(q, live), live, 100)
    assert lex.csr_builds == 1


# ------------------------------------------------------------------------------------------------ rows_dot
DOT_D = (1, 63, 64, 65, 200, 384, 1000)
DOT_M = (1, 4, 5, 1000)
DOT_ROWS = 5000
POISON = 3.0e4        # in the padding columns of both operands: one product read from there is 9e8


def dot_pairs(m):
    """qi / rows from both ends of the matrix and in between, with repeated pairs"""
    g = np.random.default_rng(m)
    ends = np.array([0, DOT_ROWS - 1, 1, DOT_ROWS - 2, 0], np.int64)
    qi = np.concatenate([ends, g.integers(0, DOT_ROWS, max(m - 5, 0))])[:m]
    rows = np.concatenate([ends[::-1], g.integers(0, DOT_ROWS, max(m - 5, 0))])[:m]
    if m >= 5:
        qi[-1], rows[-1] = qi[0], rows[0]                # a repeated pair
    return qi, rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
def test_rows_dot_against_float64(dev, dtype):
    """wave_row_dot (csrc/row_dot.h): lane j sums columns j, j + 64, ... by fmaf, then six butterfly additions.

    Integer data in -2 .. 2: every product and partial sum is an integer below 2^24, so the result is exact.

    Unit rows, against the float64 dot of the values as stored: a product of two stored values is exact inside fmaf
    (at most 24 + 24 significant bits), so a lane's chain of c = ceil(d / 64) fmaf makes c roundings and the butterfly
    6 more on every path from a column to the result.  With u = 2^-24 every term a_j c_j therefore carries a factor
    (1 + e)^(c + 6), |e| <= u, and |got - exact| <= ((1 + u)^(c + 6) - 1) sum |a_j c_j|, which is below
    1.01 (c + 6) u sum |a_j c_j|.  The float64 reference's own error, about d 2^-53 of that sum, is below the 1 %."""
    from multimodal_rag_amd import _native
    from multimodal_rag_amd.lexical import rows_dot

    u = 2.0 ** -24
    worst = 0.0
    for d in DOT_D:
        ld = _native.padded_dim(d, dtype)
        g = np.random.default_rng(d)
        for kind in ("int", "unit"):
            if kind == "int":
                a, c = (g.integers(-2, 3, (DOT_ROWS, d)).astype(np.float32) for _ in range(2))
            else:
                a, c = (g.standard_normal((DOT_ROWS, d)).astype(np.float32) for _ in range(2))
                a /= np.linalg.norm(a, axis=1, keepdims=True)
                c /= np.linalg.norm(c, axis=1, keepdims=True)
            dq = torch.full((DOT_ROWS, ld), POISON, dtype=dtype, device=dev)
            dc = torch.full((DOT_ROWS, ld), POISON, dtype=dtype, device=dev)
            dq[:, :d] = torch.from_numpy(a).to(dev).to(dtype)
            dc[:, :d] = torch.from_numpy(c).to(dev).to(dtype)
            a64 = dq[:, :d].double().cpu().numpy()           # as stored
            c64 = dc[:, :d].double().cpu().numpy()
            for m in DOT_M:
                qi, rows = dot_pairs(m)
                got = rows_dot(dq, dc, d, torch.from_numpy(qi).to(dev), torch.from_numpy(rows).to(dev)).cpu().numpy()
                exact = np.einsum("ij,ij->i", a64[qi], c64[rows])
                assert got.shape == (m,) and got.dtype == np.float32
                if kind == "int":
                    assert np.array_equal(got.astype(np.float64), exact), (d, m)
                else:
                    mag = np.einsum("ij,ij->i", np.abs(a64[qi]), np.abs(c64[rows]))
                    bound = 1.01 * (math.ceil(d / 64) + 6) * u * mag
                    err = np.abs(got.astype(np.float64) - exact)
                    worst = max(worst, float((err / (u * mag)).max()))
                    assert np.all(err <= bound), (d, m, float((err / bound).max()))
                if m >= 5:
                    assert got[-1] == got[0]
    print(f"rows_dot {dtype}: worst error {worst:.3f} u sum|a c| (bound: ceil(d / 64) + 6 = 7 .. 22)")
