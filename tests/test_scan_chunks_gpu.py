"""GPU: a batch wider than one scan launch.  A launch of the pair-tile scans holds at most 64 column tiles -- 8192
queries, 512 recommend requests of 16 example rows -- and the host cuts a longer batch into launches, moving every
per-query pointer (queries, scopes, filters, thresholds, weights, tau, counters, candidate slots, union bitmaps) by the
queries of the launches before.  B = 8193 queries (R = 513 requests) is the smallest batch with a second launch: its
one query sits alone in a column tile of its own.

n = 130 (a full row tile and one of 2), d = 64 float16 (one K-slab), k = 4, the `negative` lattice of
tests/regime_ref.py (64 distinct query rows, so neighbouring queries have different answers): np.array_equal against its
exact oracle, the whole batch, and queries 8191 and 8192 -- the last of one launch and the first of the next (requests
511 and 512) -- once more by name."""
import numpy as np
import pytest
import torch

import regime_ref as R
import scan_regimes as S
from test_search_regimes_gpu import upload

pytestmark = pytest.mark.gpu

N_ROWS, D, K = 130, 64, 4
B_ALL, R_ALL = 64 * 128 + 1, 64 * 8 + 1
DTYPE = torch.float16


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


@pytest.fixture(scope="module")
def data(N):
    """the lattice, uploaded once, and the oracle's answer; read-only"""
    q, c, alive = R.make("negative", N_ROWS, B_ALL, K, 0)
    assert alive is None
    es, er = R.expected(q, c, K)
    assert not np.array_equal(er[B_ALL - 2], er[B_ALL - 1]) or not np.array_equal(es[B_ALL - 2], es[B_ALL - 1])
    cols = R.support(D, 2)
    qd, _ = upload(N, q, cols, D, DTYPE)
    cd, _ = upload(N, c, cols, D, DTYPE)
    for a in (q, c, es, er):
        a.setflags(write=False)
    return q, c, es, er, cols, qd, cd


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def same(got, want, last):
    """the whole batch, then the two sides of the launch boundary by name"""
    for g, w in zip(got, want):
        assert g.shape == w.shape
        for b in (last - 1, last):
            assert np.array_equal(g[b], w[b]), (b, g[b], w[b])
        assert np.array_equal(g, w)


def test_scoped(N, data):
    q, c, es, er, cols, qd, cd = data
    col = torch.from_numpy(S.documents64(N_ROWS)).to("cuda")
    soq, scopes = S.scoped_config(B_ALL, False)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scopes])])
    out = host(*N.scoped_topk(qd, cd, N_ROWS, D, K, col, S.N_DOCS, soq, off, [g for s in scopes for g in s], N_ROWS))
    same(out, (es, er), B_ALL - 1)


def test_filtered(N, data):
    q, c, es, er, cols, qd, cd = data
    vis = S.bitmap_words(S.filters_of(N_ROWS, K, (), None, False), N.filter_words(N_ROWS)).view(np.int32)
    out = host(*N.filtered_topk(qd, cd, N_ROWS, D, K, np.arange(B_ALL) % 2, torch.from_numpy(vis.copy()).to("cuda")))
    same(out, (es, er), B_ALL - 1)


def test_boosted(N, data):
    q, c, es, er, cols, qd, cd = data
    s, r, bo = host(*N.boosted_topk(qd, cd, N_ROWS, D, K, S.neutral_prior(N_ROWS), np.zeros(B_ALL, np.float32)))
    same((s, r), (es, er), B_ALL - 1)
    assert not bo.any()


def test_range(N, data):
    q, c, es, er, cols, qd, cd = data
    codes = torch.from_numpy(S.facet_codes(N_ROWS)).to("cuda")
    thr = S.range_thresholds(q, c, es, "kth")        # per query: the counts differ from query to query
    want = S.range_reference(q, c, K, thr, None)
    counts, facets, s, r = host(*N.range_scan(qd, cd, N_ROWS, D, thr, K, [codes], [S.FACET_G]))
    same((counts.astype(np.int64), facets.astype(np.int64), s, r), want, B_ALL - 1)
    same((s, r), (es, er), B_ALL - 1)


def test_recommend(N, data):
    q, c, es, er, cols, qd, cd = data
    ex, sign, w = S.recommend_examples(q[:R_ALL], False)
    exd, _ = upload(N, ex, cols, D, DTYPE)
    s, r, pos, neg, pa, na = host(*N.recommend_topk(exd, sign, w, cd, N_ROWS, D, K))
    same((s, r, pos), (es[:R_ALL], er[:R_ALL], es[:R_ALL]), R_ALL - 1)
    assert np.array_equal(pa, np.tile(S.recommend_slots(R_ALL)[0][:, None], (1, K))) and not neg.any()
