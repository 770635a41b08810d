"""GPU: MaxSim over FP8 token rows -- mmrag_f8_encode_rows, the FP8 scan (_native.maxsim_topk_f8) and the FP8 pair
scorer (_native.maxsim_scores_f8) against tests/late_f8_ref.py, VectorIndex's token store at dtype float8_e4m3fn, and
the EmbeddingManager's store-backed re-rank and late_query over an FP8 store (synthetic weights).

Tolerances
  unit rows .......... test_unit_rows_within_the_float32_bound's docstring
  integer grid ....... x * 256 is an integer in -4..4 (an exact E4M3 value), so every partial sum of the accumulator is
                       an integer below 2^24 in any order and float32 is exact: scores and items EQUAL the float64
                       reference
"""
import numpy as np
import pytest
import torch

from tests import f8_ref
from tests import late_f8_ref as R
from tests.test_late_store_gpu import ITEM_LENS, Q_LENS, bitmap, plane, questions

pytestmark = pytest.mark.gpu

GUARD = 1.5     # x * 256 = 384: rows outside every sequence; a read outside a sequence shows as a huge similarity


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def int_rows(g, n, dim):
    """rows whose scaled values x * 256 are integers in -4..4"""
    return (g.integers(-4, 5, (n, dim)) / 256.0).astype(np.float32)


class Case:
    """a plane of code rows and a batch of questions (code rows) on the device, the float64 score matrix computed once"""

    def __init__(self, q_seqs, items, dim, alive=None, tail_guard=0):
        self.dim, self.alive = dim, alive
        q_np, self.qs, self.ql = questions(q_seqs, dim)
        t_np, self.off = plane(items, dim, tail_guard)
        q_np[q_np == 100.0] = GUARD        # the helpers' guard value, brought into the format's range
        t_np[t_np == 100.0] = GUARD
        self.q_codes, self.t_codes = R.encode_rows(q_np), R.encode_rows(t_np)
        self.q_dev = torch.from_numpy(self.q_codes).cuda()
        self.t_dev = torch.from_numpy(self.t_codes).cuda() if len(t_np) else torch.zeros(
            (1, self.q_codes.shape[1]), dtype=torch.uint8, device="cuda")
        self.off_dev = torch.from_numpy(self.off).cuda()
        self.bits = bitmap(alive) if alive is not None else None
        self.n_items, self.n_rows = len(items), len(t_np)
        self.scores = R.score_matrix(self.q_codes, self.qs, self.ql, self.t_codes, self.off, alive)

    def run(self, N, k, **kw):
        s, r = N.maxsim_topk_f8(self.q_dev, self.qs, self.ql, self.t_dev, self.n_rows, self.off_dev, self.n_items,
                                self.dim, k, alive_bits=self.bits, **kw)
        torch.cuda.synchronize()
        return s.cpu().numpy(), r.cpu().numpy()

    def assert_exact(self, N, k, **kw):
        from tests import late_store_ref

        got_s, got_r = self.run(N, k, **kw)
        ref_s, ref_r = late_store_ref.topk_of_scores(self.scores, k)
        assert np.array_equal(got_r, ref_r), (k, kw, got_r, ref_r)
        assert np.array_equal(got_s, ref_s.astype(np.float32)), (k, kw, got_s, ref_s)
        return got_s, got_r


@pytest.fixture(scope="module", params=[64, 128, 384, 768])
def grid_case(request):
    dim = request.param
    g = np.random.default_rng(900 + dim)
    return Case([int_rows(g, n, dim) for n in Q_LENS], [int_rows(g, n, dim) for n in ITEM_LENS], dim, tail_guard=3)


# ---------------------------------------------------------------- the encoder
@pytest.mark.parametrize("src_dtype", [torch.float16, torch.float32])
def test_encode_rows_equals_the_reference(N, src_dtype):
    x = np.concatenate([f8_ref.sweep(), f8_ref.saturating()])
    if src_dtype == torch.float16:
        with np.errstate(over="ignore"):
            x = x.astype(np.float16).astype(np.float32)      # what a half source holds
    for d in (64, 100, 384):
        rows = np.resize(x, (x.size // d + 1, d)).astype(np.float32)
        src = torch.from_numpy(rows).to(src_dtype).cuda()
        got = N.f8_encode_rows(src).cpu().numpy()
        ld = (d + 127) // 128 * 128
        assert got.shape == (rows.shape[0], ld) and got.dtype == np.uint8
        assert np.array_equal(got[:, :d], f8_ref.encode(rows)), d
        assert (got[:, d:] == 0).all(), d
    # a strided source (rows of a wider tensor) and an output given by the caller, filled with something else first
    wide = torch.from_numpy(np.resize(x, (7, 200)).astype(np.float32)).to(src_dtype).cuda()
    out = torch.full((7, 128), 0x55, dtype=torch.uint8, device="cuda")
    got = N.f8_encode_rows(wide[:, :128], 70, out=out).cpu().numpy()
    assert np.array_equal(got[:, :70], f8_ref.encode(wide[:, :70].float().cpu().numpy())) and (got[:, 70:] == 0).all()
    with pytest.raises(N.MMRagNativeError):
        N.f8_encode_rows(wide.to(torch.bfloat16))


# ---------------------------------------------------------------- the scan and the pair scorer
@pytest.mark.parametrize("k", [1, 5, 50])
@pytest.mark.parametrize("chunk_rows", [0, 256, 100])
def test_integer_exact_grid(N, grid_case, k, chunk_rows):
    """tests/test_late_store_gpu.py's grid on code rows: items of every length class back to back, straddling the
    128-row B tiles and the chunks; four questions share an A tile and one fills a tile; dim 64 is half a slab of pad"""
    s, r = grid_case.assert_exact(N, k, chunk_rows=chunk_rows)
    if k == 50:
        assert (r[:, 20:] == -1).all() and np.isneginf(s[:, 20:]).all() and (r[:, :20] >= 0).all()


def test_outputs_do_not_depend_on_chunks_batch_or_bound(N, grid_case):
    c = grid_case
    base_s, base_r = c.run(N, 5)
    for kw in (dict(chunk_rows=128), dict(chunk_rows=4096), dict(dbg=1), dict(cap=8), dict(cap=8, chunk_rows=300)):
        s, r = c.run(N, 5, **kw)
        assert np.array_equal(s.view(np.int32), base_s.view(np.int32)) and np.array_equal(r, base_r), kw
    for q in (0, 3, 7, 10):           # a question alone
        s, r = N.maxsim_topk_f8(c.q_dev, c.qs[q: q + 1], c.ql[q: q + 1], c.t_dev, c.n_rows, c.off_dev, c.n_items, c.dim, 5)
        assert np.array_equal(s.cpu().numpy().view(np.int32), base_s[q: q + 1].view(np.int32)), q
        assert np.array_equal(r.cpu().numpy(), base_r[q: q + 1]), q


def test_pair_scorer_is_exact_and_scan_bits_equal_it(N, grid_case):
    """best_sim / best_idx / out_sum of every (question, item) pair equal the float64 reference (lowest j on ties: small
    integers tie often); the scan's scores have the pair scorer's bits"""
    c = grid_case
    Q, n = len(c.ql), c.n_items
    pq, pd = np.repeat(np.arange(Q), n).astype(np.int32), np.tile(np.arange(n), Q).astype(np.int32)
    d_start, d_len = c.off[:-1], c.off[1:] - c.off[:-1]
    sums, best_sim, best_idx = N.maxsim_scores_f8(c.q_dev, c.t_dev, c.dim, c.qs, c.ql, d_start, d_len, pq, pd)
    sums, best_sim, best_idx = sums.cpu().numpy(), best_sim.cpu().numpy(), best_idx.cpu().numpy()
    ref = R.score_tables(c.q_codes, c.t_codes, c.qs, c.ql, d_start, d_len, pq, pd)
    for p, (b_sim, b_idx, total, _) in enumerate(ref):
        m = len(b_sim)
        assert np.array_equal(best_sim[p, :m], b_sim.astype(np.float32)), p
        assert np.array_equal(best_idx[p, :m], b_idx), p
        assert sums[p] == np.float32(total), p
    s, r = c.run(N, n)
    assert (np.sort(r, axis=1) == np.arange(n)).all()
    by_item = sums.reshape(Q, n)
    assert np.array_equal(np.take_along_axis(by_item, r, axis=1).view(np.int32), s.view(np.int32))


@pytest.mark.parametrize("neg_len", [1, 5, 129, 300])
def test_all_negative_similarities(N, neg_len):
    """every similarity of the negative items is negative: neither the positive rows of the neighbours, nor the GUARD
    rows after the last item, nor zero padding (code 0) may be a maximum"""
    dim = 64
    g = np.random.default_rng(neg_len)
    q = [(g.integers(1, 5, (n, dim)) / 256.0).astype(np.float32) for n in (20, 32, 128)]
    pos = lambda n: (g.integers(1, 5, (n, dim)) / 256.0).astype(np.float32)     # noqa: E731
    neg = lambda n: -(g.integers(1, 5, (n, dim)) / 256.0).astype(np.float32)    # noqa: E731
    c = Case(q, [pos(70), neg(neg_len), pos(200), pos(3), neg(neg_len)], dim, tail_guard=140)
    s, r = c.assert_exact(N, 5, chunk_rows=128)
    for row_s, row_r in zip(s, r):
        assert (row_s[np.isin(row_r, (1, 4))] < 0).all() and (row_s[np.isin(row_r, (0, 2, 3))] > 0).all()


def test_duplicates_dead_and_empty_items(N):
    dim = 128
    g = np.random.default_rng(5)
    v = (g.choice([-4.0, 4.0], (9, dim)) / 256.0).astype(np.float32)
    dup = np.concatenate([v, int_rows(g, 60, dim)])
    lens = (100, 0, 130, 0, 257, 5, 300, 0, 64, 1)
    items = [int_rows(g, n, dim) for n in lens]
    at = (1, 3, 4, 8, 11, 13)
    for i in at:
        items.insert(i, dup.copy())
    alive = np.ones(len(items), bool)
    alive[[at[1], 0]] = False
    c = Case([v, v[:4]], items, dim, alive=alive)
    s, r = c.assert_exact(N, 8, chunk_rows=200)
    live_dups = [i for i in at if alive[i]]
    assert r[0, :5].tolist() == live_dups and (s[0, :5] == np.float32(9 * 16 * dim * 2.0 ** -16)).all()
    empty = [i for i, x in enumerate(items) if len(x) == 0]
    assert not np.isin(r, empty + [at[1], 0]).any()


@pytest.fixture(scope="module")
def many_case():
    """20 000 items of 1..8 tokens (above the 16 384 candidate slots), two questions, planted winners"""
    dim = 64
    g = np.random.default_rng(77)
    q = [(g.choice([-4.0, 4.0], (n, dim)) / 256.0).astype(np.float32) for n in (5, 8)]
    lens = g.integers(1, 9, 20000)
    items = [int_rows(g, n, dim) for n in lens]
    for j, i in enumerate((19999, 17, 12345, 16384, 8000, 3)):
        items[i][: min(len(items[i]), 1 + j)] = q[j % 2][: min(len(items[i]), 1 + j)]
    return Case(q, items, dim, tail_guard=1)


@pytest.mark.parametrize("k", [5, 100])
def test_bound_pass_is_exact(N, many_case, k):
    s, r = many_case.assert_exact(N, k)
    s2, r2 = many_case.run(N, k, dbg=1)          # no bound pass: every question overflows and is produced again alone
    assert np.array_equal(s.view(np.int32), s2.view(np.int32)) and np.array_equal(r, r2)


# ---------------------------------------------------------------- VectorIndex's token store
def test_index_store_add_delete_compact_add(N):
    """item = row through add / set_tokens / delete / compact / add again at dtype float8_e4m3fn: late_search equals
    the reference over the live rows at each step, from fp16 question rows (quantised by the index)"""
    from multimodal_rag_amd.index import VectorIndex

    dim = 128
    g = np.random.default_rng(11)
    idx = VectorIndex(dim=dim, dtype=torch.float16)
    st = idx.enable_token_store(dim, 40, dtype="float8_e4m3fn")
    assert st.plane.dtype == torch.uint8 and st.plane.shape[1] == 128
    with pytest.raises(ValueError, match="holds float8_e4m3fn rows"):
        idx.enable_token_store(dim, 40, dtype="float16")
    tokens = {}

    def unit(n):
        x = g.standard_normal((n, dim))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)

    def add(lo, hi, with_tokens=True):
        ids = [f"i{j}" for j in range(lo, hi)]
        idx.add(unit(hi - lo), documents=ids, metadatas=[{"par": j % 2} for j in range(lo, hi)], ids=ids)
        if with_tokens:
            lens = g.integers(0, 41, hi - lo)
            seqs = [int_rows(g, n, dim) for n in lens]
            idx.set_tokens(idx.rows_of_ids(ids), np.concatenate(seqs).astype(np.float16), lens)
            tokens.update({s: x for s, x in zip(ids, seqs) if len(x)})

    q_np, qs, ql = questions([int_rows(g, n, dim) for n in (6, 33, 1)], dim)
    q_np[q_np == 100.0] = GUARD
    q_dev = torch.from_numpy(q_np.astype(np.float16)).cuda()

    def check(k, where=None, live=None):
        s, r = idx.late_search(q_dev, qs, ql, k, where=where)
        s, r = s.cpu().numpy(), r.cpu().numpy()
        n = idx.rows_in_use
        ids = idx.ids_of_rows(range(n))
        row_live = np.array([i in idx._row_of for i in ids], bool) if live is None else live(ids)
        rows, off = plane([tokens.get(i, np.zeros((0, dim), np.float32)) for i in ids], dim)
        ref_s, ref_r = R.topk(R.encode_rows(q_np), qs, ql, R.encode_rows(rows), off, k, row_live)
        assert np.array_equal(r, ref_r) and np.array_equal(s, ref_s.astype(np.float32)), (k, where)
        return r

    add(0, 30)
    check(5)
    add(30, 34, with_tokens=False)
    check(40)
    idx.delete(ids=[f"i{j}" for j in (0, 3, 4, 17, 29, 31)])
    assert not np.isin(check(40), [0, 3, 4, 17, 29, 31]).any()
    check(7, where={"par": 1}, live=lambda ids: np.array([i in idx._row_of and int(i[1:]) % 2 == 1 for i in ids]))
    idx.compact()
    check(40)
    add(34, 50)
    check(60)
    stats = idx.token_stats()
    assert stats["dtype"] == "float8_e4m3fn" and stats["bytes"] == stats["tokens"] * dim
    (span,), pl, _ = idx.token_spans([["i5"]])
    assert pl.dtype == torch.uint8 and span[1] == len(tokens["i5"])
    # an fp16 store in the same process answers as the plain fp16 calls do, bit for bit
    idx16 = VectorIndex(dim=dim, dtype=torch.float16)
    idx16.enable_token_store(dim, 40)
    ids = [f"h{j}" for j in range(12)]
    idx16.add(unit(12), documents=ids, ids=ids)
    lens = g.integers(1, 41, 12)
    rows16 = torch.from_numpy(np.concatenate([int_rows(g, n, dim) for n in lens]).astype(np.float16)).cuda()
    idx16.set_tokens(idx16.rows_of_ids(ids), rows16, lens)
    s, r = idx16.late_search(q_dev, qs, ql, 5)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).cuda()
    s2, r2 = N.maxsim_topk(q_dev, qs, ql, rows16, len(rows16), off, 12, dim, 5)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(r, r2)
    assert idx16.token_stats()["dtype"] == "float16"


# ---------------------------------------------------------------- slots, ties and overflow
def test_best_slots_past_q_len_are_not_written(N):
    """the C entry with caller-filled outputs: slots i >= q_len of best_sim / best_idx keep the sentinel, the slots
    below hold the reference (lowest j on ties: the passage repeats its rows)"""
    dim = 128
    g = np.random.default_rng(3)
    q_lens, d_lens = (1, 7, 127, 128), (1, 130, 300)
    q_np, qs, ql = questions([int_rows(g, n, dim) for n in q_lens], dim)
    q_np[q_np == 100.0] = GUARD
    items = [int_rows(g, n, dim) for n in d_lens]
    items[1][65:130] = items[1][:65]               # every row of the first half again: ties 65 apart, across a tile edge
    t_np, off = plane(items, dim, 2)
    t_np[t_np == 100.0] = GUARD
    q_codes, t_codes = R.encode_rows(q_np), R.encode_rows(t_np)
    pq = np.repeat(np.arange(len(q_lens)), len(d_lens)).astype(np.int32)
    pd = np.tile(np.arange(len(d_lens)), len(q_lens)).astype(np.int32)
    d_start, d_len = off[:-1].astype(np.int32), (off[1:] - off[:-1]).astype(np.int32)
    P, W = len(pq), N.MAX_LATE_QUERY_TOKENS
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    q_dev, t_dev = dev(q_codes), dev(t_codes)
    tabs = [dev(x) for x in (qs, ql, d_start, d_len, pq, pd)]
    sums = torch.full((P,), -7.0, dtype=torch.float32, device="cuda")
    best_sim = torch.full((P, W), -7.0, dtype=torch.float32, device="cuda")
    best_idx = torch.full((P, W), -7, dtype=torch.int32, device="cuda")
    st = N.lib().mmrag_maxsim_scores_f8(
        q_dev.data_ptr(), q_dev.shape[0], q_dev.shape[1], t_dev.data_ptr(), t_dev.shape[0], t_dev.shape[1], dim,
        tabs[0].data_ptr(), tabs[1].data_ptr(), len(q_lens), tabs[2].data_ptr(), tabs[3].data_ptr(), len(d_lens),
        tabs[4].data_ptr(), tabs[5].data_ptr(), P, sums.data_ptr(), best_sim.data_ptr(), best_idx.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert st == 0, N.lib().mmrag_last_error()
    torch.cuda.synchronize()
    sums, best_sim, best_idx = sums.cpu().numpy(), best_sim.cpu().numpy(), best_idx.cpu().numpy()
    ref = R.score_tables(q_codes, t_codes, qs, ql, d_start, d_len, pq, pd)
    tie_seen = False
    for p, (b_sim, b_idx, total, _) in enumerate(ref):
        m = len(b_sim)
        assert np.array_equal(best_sim[p, :m], b_sim.astype(np.float32)) and np.array_equal(best_idx[p, :m], b_idx), p
        assert sums[p] == np.float32(total), p
        assert (best_sim[p, m:] == -7.0).all() and (best_idx[p, m:] == -7).all(), p
        if pd[p] == 1:
            assert not ((b_idx >= 65) & (b_idx < 130)).any(), p       # a repeated row never wins: the lowest j does
            tie_seen = True
    assert tie_seen


def test_all_items_tie_overflow_rerun(N):
    """20 000 identical items: every score ties, so every item is at or above the staged bound, the question overflows
    its slots and is produced again alone; the winners are items 0 .. k-1"""
    dim = 64
    g = np.random.default_rng(8)
    item = int_rows(g, 3, dim)
    q_np, qs, ql = questions([int_rows(g, 6, dim), int_rows(g, 2, dim)], dim)
    q_np[q_np == 100.0] = GUARD
    q_codes = R.encode_rows(q_np)
    t_codes = np.tile(R.encode_rows(item), (20000, 1))
    off = (3 * np.arange(20001)).astype(np.int32)
    q_dev, t_dev, off_dev = (torch.from_numpy(x).cuda() for x in (q_codes, t_codes, off))
    one = R.score_matrix(q_codes, qs, ql, t_codes[:3], off[:2])[:, 0]
    for k in (5, 100):
        s, r = N.maxsim_topk_f8(q_dev, qs, ql, t_dev, len(t_codes), off_dev, 20000, dim, k)
        s, r = s.cpu().numpy(), r.cpu().numpy()
        assert (r == np.arange(k)).all(), r
        assert np.array_equal(s, np.repeat(one.astype(np.float32)[:, None], k, axis=1))


# ---------------------------------------------------------------- unit rows
@pytest.mark.parametrize("dim", [384, 768])
def test_unit_rows_within_the_float32_bound(N, dim):
    """f8_ref.clustered token rows, 300 items of 1..60 tokens, questions of 7, 32 and 128 tokens.  Bound of a score
    against tests/late_f8_ref.py: sum over i of max over j of the per-dot bound of tests/test_f8_gpu.py::_check_unit
    (2 d_pad 2^-24 sum|q_i||d_j| 2^-16: a maximum of values each within e_ij of its reference is within max_j e_ij of
    the reference maximum) plus the float32 sum's q_len 2^-24 sum_i |best_i|.  An item that differs from the reference
    list must lie within that bound (its own plus the k-th item's) of the k-th score."""
    from tests import late_store_ref

    g = np.random.default_rng(dim)
    lens = g.integers(1, 61, 300)
    q_lens = (7, 32, 128)
    rows, q_rows = f8_ref.clustered(n=int(lens.sum()), d=dim, n_q=sum(q_lens), seed=dim)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    qs = np.concatenate([[0], np.cumsum(q_lens)[:-1]]).astype(np.int32)
    ql = np.array(q_lens, np.int32)
    q_codes, t_codes = R.encode_rows(q_rows), R.encode_rows(rows)
    d_pad = t_codes.shape[1]
    vq, vt = R.values(q_codes), R.values(t_codes)
    sims, absum = vq @ vt.T, np.abs(vq) @ np.abs(vt).T
    e = 2 * d_pad * 2.0 ** -24 * absum
    best = np.maximum.reduceat(sims, off[:-1], axis=1)             # [q rows, items]: every item has rows
    e_max = np.maximum.reduceat(e, off[:-1], axis=1)
    ref = np.stack([best[s: s + n].sum(axis=0) for s, n in zip(qs, ql)])
    bound = np.stack([e_max[s: s + n].sum(axis=0) + n * 2.0 ** -24 * np.abs(best[s: s + n]).sum(axis=0)
                      for s, n in zip(qs, ql)])
    assert np.allclose(ref, R.score_matrix(q_codes, qs, ql, t_codes, off), rtol=0, atol=1e-9)
    q_dev, t_dev, off_dev = (torch.from_numpy(x).cuda() for x in (q_codes, t_codes, off))
    for k in (5, 40):
        s, r = N.maxsim_topk_f8(q_dev, qs, ql, t_dev, len(t_codes), off_dev, len(lens), dim, k, chunk_rows=1024)
        s, r = s.cpu().numpy().astype(np.float64), r.cpu().numpy()
        _, ref_r = late_store_ref.topk_of_scores(ref, k)
        for q in range(len(ql)):
            err = np.abs(s[q] - ref[q, r[q]])
            print(f"dim {dim} k {k} q_len {ql[q]}: max err {err.max():.3e}, smallest bound {bound[q, r[q]].min():.3e}")
            assert (err <= bound[q, r[q]]).all(), (q, float(err.max()))
            kth = ref_r[q, -1]
            for item in set(r[q].tolist()) ^ set(ref_r[q].tolist()):
                assert abs(ref[q, item] - ref[q, kth]) <= bound[q, item] + bound[q, kth], (q, item)
    # the scan's bits are the pair scorer's on these rows too
    pq = np.repeat(np.arange(len(ql)), 40).astype(np.int32)
    sums, _, _ = N.maxsim_scores_f8(q_dev, t_dev, dim, qs, ql, off[:-1], off[1:] - off[:-1], pq, r.reshape(-1),
                                    want_best=False)
    s32, _ = N.maxsim_topk_f8(q_dev, qs, ql, t_dev, len(t_codes), off_dev, len(lens), dim, 40)
    assert np.array_equal(sums.cpu().numpy().view(np.int32), s32.cpu().numpy().reshape(-1).view(np.int32))


# ---------------------------------------------------------------- manager level
@pytest.fixture()
def manager(N):
    from multimodal_rag_amd import embedder as EM

    names = ("MMRAG_MODEL_DIR", "MMRAG_ENCODER_PRECISION", "MMRAG_RERANKER_DIR", "MMRAG_LATE_STORE",
             "MMRAG_LATE_STORE_MAX_BYTES", "MMRAG_LATE_STORE_DTYPE")
    saved = [getattr(EM.settings, n) for n in names]
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION, EM.settings.MMRAG_RERANKER_DIR = "", "fp16", ""
    EM.settings.MMRAG_LATE_STORE, EM.settings.MMRAG_LATE_STORE_MAX_BYTES = True, 0
    EM.settings.MMRAG_LATE_STORE_DTYPE = "float8_e4m3fn"
    try:
        yield EM.EmbeddingManager(engine=EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2"), enable_cache=False)
    finally:
        for n, v in zip(names, saved):
            setattr(EM.settings, n, v)


def test_manager_f8_store_rerank_late_query_and_fp16_unchanged(N, manager, monkeypatch):
    """synthetic weights, tests/test_late_store_gpu.py's documents (its docstring says why their forwards are
    bit-stable): with an FP8 store a stored passage scores the same from the plane as forced through re-encoding,
    with and without `explain`; late_query returns the reference's ids over the plane's own codes; an fp16 store in the
    same process still equals the plain fp16 calls bit for bit"""
    import asyncio

    from starlette.testclient import TestClient

    from multimodal_rag_amd import embedder as EM
    from multimodal_rag_amd import server
    from tests.test_late_store_gpu import DOCS, QUERY, stored_hits, summaries

    run = asyncio.run
    with TestClient(server.create_app(embedder=manager)) as c:
        run(manager.initialize())
        run(manager.delete_all_documents())
        run(manager.embed_and_store(summaries(DOCS), "docA"))
        ids = [f"docA_c{i}" for i in range(len(DOCS))]
        store = manager.collection.token_store
        stats = run(manager.get_collection_stats())["late_store"]
        assert store.f8 and stats["dtype"] == "float8_e4m3fn" and stats["items"] == len(DOCS)
        assert stats["bytes"] == stats["tokens"] * 384 and stats["bytes_per_token"] == 384     # dim bytes per token
        # ---- re-rank: from the plane == forced through re-encoding (ids the store does not know), list against list
        hits = stored_hits(manager, ids)
        forced = {**hits, "ids": ["unknown" + i for i in hits["ids"]]}
        mixed = {**hits, "ids": [i if at % 2 else "unknown" + i for at, i in enumerate(hits["ids"])]}
        for explain in (False, True):
            backed = run(manager.late_rerank(QUERY, hits, explain=explain))
            for other in (forced, mixed):
                again = run(manager.late_rerank(QUERY, other, explain=explain))
                assert [i.replace("unknown", "") for i in again["ids"]] == backed["ids"], explain
                assert again["rerank_scores"] == backed["rerank_scores"], explain
                if explain:
                    assert again["late_matches"] == backed["late_matches"]
        assert backed["ids"][0] == ids[1] and len(backed["late_matches"][0]) > 0
        # the scores are the quantised rows' own: not the fp16 scorer's
        monkeypatch.setattr(manager.collection, "_tokens", None)
        plain16 = run(manager.late_rerank(QUERY, hits))
        monkeypatch.undo()
        assert plain16["rerank_scores"] != run(manager.late_rerank(QUERY, hits))["rerank_scores"]
        # ---- late_query end to end: the reference over the plane's codes and the quantised question rows
        scorer = manager._get_late()
        q_tok, q_start, q_len, _ = scorer.encode_questions([QUERY])
        n = manager.collection.rows_in_use
        ref_s, ref_r = R.topk(R.encode_rows(q_tok.float().cpu().numpy()), q_start, q_len,
                              store.plane[: store.n_rows].cpu().numpy(), store.offsets(n), len(DOCS))
        found = run(manager.late_query(QUERY, n_results=len(DOCS)))
        assert found["ids"] == manager.collection.ids_of_rows([int(i) for i in ref_r[0] if i >= 0])
        assert found["ids"][0] == ids[1] and found["ids"] == backed["ids"]
        # unit rows: sum|q_i||d_j| <= 1 (Cauchy-Schwarz; quantising moves a norm by well under 2^-4), so the per-dot bound
        # 2 d 2^-24 sum|q_i||d_j| of test_unit_rows_within_the_float32_bound is at most 2 * 384 * 2^-24 * 1.13 per
        # similarity, hence per maximum and per mean of maxima; the float32 sum adds q_len * 2^-24 * |mean| <= 128 * 2^-24
        tol = 2 * 384 * 2.0 ** -24 * 1.13 + 128 * 2.0 ** -24
        assert np.allclose(found["late_scores"], ref_s[0][: len(found["ids"])] / q_len[0], rtol=0, atol=tol)
        assert found["late_scores"] == backed["rerank_scores"]
        r = c.post("/query", json={"query": QUERY, "top_k": 3, "late": True})
        assert r.status_code == 200 and [s["doc_id"] for s in r.json()["sources"]] == found["ids"][:3], r.text
        # ---- an fp16 store in the same process: what the plain fp16 calls give, bit for bit
        monkeypatch.setattr(EM.settings, "MMRAG_LATE_STORE_DTYPE", "float16")
        manager.collection._tokens = None
        stats = run(manager.enable_late_store())
        assert stats["dtype"] == "float16" and stats["bytes"] == stats["tokens"] * 768
        backed16 = run(manager.late_rerank(QUERY, hits, explain=True))
        assert backed16["rerank_scores"] == plain16["rerank_scores"] and backed16["ids"] == plain16["ids"]
        assert backed16 == run(manager.late_rerank(QUERY, forced, explain=True)) | {"ids": backed16["ids"]}
        found16 = run(manager.late_query(QUERY, n_results=len(DOCS)))
        assert found16["ids"] == plain16["ids"] and found16["late_scores"] == plain16["rerank_scores"]
        st16 = manager.collection.token_store
        s, r = manager.collection.late_search(q_tok, q_start, q_len, len(DOCS))
        s2, r2 = N.maxsim_topk(q_tok, q_start, q_len, st16.plane, st16.n_rows, st16.device_offsets(n), n, 384, len(DOCS))
        assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(r, r2)
