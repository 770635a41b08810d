"""GPU: the token store -- the exact MaxSim scan (csrc/maxsim_scan.hip through _native.maxsim_topk) against
tests/late_store_ref.py and against mmrag_maxsim_scores' own sums, VectorIndex's token store, re-ranking from stored
tokens and first-stage late retrieval.

Tolerances
  integer rows ....... entries in {-2..2}: every dot product and every sum is an integer below 2^24, exact in float32;
                       scores and items are compared bit for bit with the float64 reference
  random unit rows ... every winner's score equals mmrag_maxsim_scores' out_sum of the same pair bit for bit; its mean
                       is within 1e-4 + q_len * 2^-23 of float64 (tests/test_late_gpu.py's bound) and an item that did
                       not win is not better than the last winner by more than twice that
"""
import numpy as np
import pytest
import torch

from tests import late_store_ref as R

pytestmark = pytest.mark.gpu

GUARD = 100.0   # rows outside every sequence: a read outside a sequence shows as a huge similarity


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def int_rows(g, n, dim):
    return g.integers(-2, 3, (n, dim)).astype(np.float32)


def unit_rows(g, n, dim):
    x = g.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def questions(q_seqs, dim, guard_rows=2):
    """question sequences -> (rows [n, dim] float32 with GUARD rows before, between and after them, starts, lens)"""
    parts, starts, at = [], [], 0
    for s in q_seqs:
        parts.append(np.full((guard_rows, dim), GUARD, np.float32))
        at += guard_rows
        parts.append(np.asarray(s, np.float32))
        starts.append(at)
        at += len(s)
    parts.append(np.full((guard_rows, dim), GUARD, np.float32))
    return np.concatenate(parts), np.array(starts, np.int32), np.array([len(s) for s in q_seqs], np.int32)


def plane(items, dim, tail_guard=0):
    """items (arrays [len, dim], len 0 allowed) -> (rows [T, dim] float32, the items back to back and `tail_guard` GUARD
    rows after the last, item_off [n + 1])"""
    off = np.zeros(len(items) + 1, np.int64)
    np.cumsum([len(x) for x in items], out=off[1:])
    parts = [np.asarray(x, np.float32).reshape(-1, dim) for x in items] + [np.full((tail_guard, dim), GUARD, np.float32)]
    return np.concatenate(parts), off.astype(np.int32)


def bitmap(alive):
    flags = np.zeros((len(alive) + 31) // 32 * 32, bool)
    flags[: len(alive)] = alive
    return torch.from_numpy(np.packbits(flags, bitorder="little").view(np.int32).copy()).cuda()


class Case:
    """a token plane and a batch of questions on the device, with the float64 score matrix computed once"""

    def __init__(self, q_seqs, items, dim, alive=None, tail_guard=0):
        self.dim, self.alive = dim, alive
        self.q_np, self.qs, self.ql = questions(q_seqs, dim)
        self.t_np, self.off = plane(items, dim, tail_guard)
        self.q_np = self.q_np.astype(np.float16)
        self.t_np = self.t_np.astype(np.float16)
        self.q_dev = torch.from_numpy(self.q_np).cuda().contiguous()
        self.t_dev = torch.from_numpy(self.t_np).cuda().contiguous() if len(self.t_np) else torch.zeros(
            (1, dim), dtype=torch.float16, device="cuda")
        self.off_dev = torch.from_numpy(self.off).cuda()
        self.bits = bitmap(alive) if alive is not None else None
        self.n_items = len(items)
        self.scores = R.score_matrix(self.q_np, self.qs, self.ql, self.t_np, self.off, alive)

    def run(self, N, k, **kw):
        s, r = N.maxsim_topk(self.q_dev, self.qs, self.ql, self.t_dev, len(self.t_np), self.off_dev, self.n_items,
                             self.dim, k, alive_bits=self.bits, **kw)
        torch.cuda.synchronize()
        return s.cpu().numpy(), r.cpu().numpy()

    def assert_exact(self, N, k, **kw):
        got_s, got_r = self.run(N, k, **kw)
        ref_s, ref_r = R.topk_of_scores(self.scores, k)
        assert np.array_equal(got_r, ref_r), (k, kw, got_r, ref_r)
        assert np.array_equal(got_s, ref_s.astype(np.float32)), (k, kw, got_s, ref_s)
        return got_s, got_r


ITEM_LENS = (63, 300, 1, 129, 512, 5, 64, 127, 65, 128, 300, 1, 128, 129, 512, 127, 5, 63, 65, 64)
Q_LENS = (32, 32, 32, 32, 1, 31, 33, 128, 33, 31, 1)      # tiles: 4 x 32 | 1 + 31 + 33 | 128 | 33 + 31 + 1


@pytest.fixture(scope="module", params=[64, 384])
def grid_case(request):
    dim = request.param
    g = np.random.default_rng(300 + dim)
    return Case([int_rows(g, n, dim) for n in Q_LENS], [int_rows(g, n, dim) for n in ITEM_LENS], dim, tail_guard=3)


@pytest.mark.parametrize("k", [1, 5, 50])
@pytest.mark.parametrize("chunk_rows", [0, 256, 100])
def test_integer_exact_grid(N, grid_case, k, chunk_rows):
    """items of every length class back to back (2743 rows): they straddle the 128-row B tiles and, with R = 256 or
    100, the chunks -- chunks that own one item, chunks that own none (the 300- and 512-token items run over them) and
    chunks that own several; four questions share an A tile and one question fills a tile; k = 50 exceeds the 20 items"""
    s, r = grid_case.assert_exact(N, k, chunk_rows=chunk_rows)
    if k == 50:
        assert (r[:, 20:] == -1).all() and np.isneginf(s[:, 20:]).all() and (r[:, :20] >= 0).all()


def test_outputs_do_not_depend_on_chunks_batch_or_bound(N, grid_case):
    c = grid_case
    base_s, base_r = c.run(N, 5)
    for kw in (dict(chunk_rows=128), dict(chunk_rows=4096), dict(dbg=1), dict(cap=8), dict(cap=8, chunk_rows=300)):
        s, r = c.run(N, 5, **kw)      # cap = 8 < 20 items: every question overflows and is produced again alone
        assert np.array_equal(s.view(np.int32), base_s.view(np.int32)) and np.array_equal(r, base_r), kw
    for q in (0, 3, 7, 10):           # a question alone
        s, r = N.maxsim_topk(c.q_dev, c.qs[q: q + 1], c.ql[q: q + 1], c.t_dev, len(c.t_np), c.off_dev, c.n_items, c.dim, 5)
        assert np.array_equal(s.cpu().numpy().view(np.int32), base_s[q: q + 1].view(np.int32)), q
        assert np.array_equal(r.cpu().numpy(), base_r[q: q + 1]), q


@pytest.mark.parametrize("dim", [64, 128, 384, 768])
def test_score_bits_equal_maxsim_scores(N, dim):
    g = np.random.default_rng(400 + dim)
    q_lens, lens = (7, 32, 128, 33, 1), (40, 200, 1, 129, 512, 128, 77, 300, 256, 12)
    c = Case([unit_rows(g, n, dim) for n in q_lens], [unit_rows(g, n, dim) for n in lens], dim, tail_guard=2)
    k = len(lens)
    s, r = c.run(N, k, chunk_rows=512)
    assert (np.sort(r, axis=1) == np.arange(k)).all()
    pq = np.repeat(np.arange(len(q_lens)), k)
    sums, _, _ = N.maxsim_scores(c.q_dev, c.t_dev, dim, c.qs, c.ql, c.off[:-1], c.off[1:] - c.off[:-1], pq,
                                 r.reshape(-1), want_best=False)
    assert np.array_equal(sums.cpu().numpy().view(np.int32), s.reshape(-1).view(np.int32))
    worst = 0.0
    for q, n in enumerate(q_lens):
        tol = 1e-4 + n * 2.0 ** -23
        ref = c.scores[q] / n
        err = np.abs(s[q] / n - ref[r[q]])
        worst = max(worst, float(err.max()))
        assert err.max() <= tol, (q, float(err.max()))
        assert (np.diff(ref[r[q]]) <= 2 * tol).all(), q       # descending against float64, within the tolerance
    print(f"dim {dim}: max |mean - float64| = {worst:.2e}")
    # a shorter list holds the best of the full one
    s3, r3 = c.run(N, 3)
    assert np.array_equal(r3, r[:, :3]) and np.array_equal(s3.view(np.int32), s[:, :3].view(np.int32))


@pytest.mark.parametrize("neg_len", [1, 5, 129, 300])
def test_all_negative_similarities(N, neg_len):
    """every similarity of the negative items is negative: neither the large positive rows of the neighbours on both
    sides, nor the GUARD rows after the last item, nor zero padding may be a maximum"""
    dim = 64
    g = np.random.default_rng(neg_len)
    q = [g.integers(1, 3, (n, dim)).astype(np.float32) for n in (20, 32, 128)]
    pos = lambda n: g.integers(1, 3, (n, dim)).astype(np.float32)     # noqa: E731
    neg = lambda n: -g.integers(1, 3, (n, dim)).astype(np.float32)    # noqa: E731
    items = [pos(70), neg(neg_len), pos(200), pos(3), neg(neg_len)]
    c = Case(q, items, dim, tail_guard=140)
    s, r = c.assert_exact(N, 5, chunk_rows=128)
    for row_s, row_r in zip(s, r):
        assert (row_s[np.isin(row_r, (1, 4))] < 0).all() and (row_s[np.isin(row_r, (0, 2, 3))] > 0).all()


@pytest.mark.parametrize("k", [3, 6, 8])
def test_duplicated_items_go_to_the_lower_item(N, k):
    """six copies of one item among others that score less, spread over tiles and chunks: equal scores rank by item"""
    dim = 64
    g = np.random.default_rng(k)
    v = g.choice([-2.0, 2.0], (9, dim)).astype(np.float32)
    dup = np.concatenate([v, int_rows(g, 60, dim)])
    items = [int_rows(g, n, dim) for n in (100, 30, 128, 257, 5, 40, 300, 90, 64, 129)]
    at = (1, 3, 4, 8, 11, 15)
    for i in at:
        items.insert(i, dup.copy())
    c = Case([v, v[:4]], items, dim)
    s, r = c.assert_exact(N, k, chunk_rows=200)
    assert r[0, : min(k, 6)].tolist() == list(at)[:k] and (s[0, : min(k, 6)] == 9 * 4.0 * dim).all()


def test_dead_and_empty_items(N):
    dim = 64
    g = np.random.default_rng(5)
    lens = (10, 0, 130, 0, 0, 7, 300, 0, 64, 1, 0)
    items = [int_rows(g, n, dim) for n in lens]
    alive = np.array([1, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1], bool)
    q = [int_rows(g, n, dim) for n in (5, 128)]
    c = Case(q, items, dim, alive=alive, tail_guard=4)
    s, r = c.assert_exact(N, 8, chunk_rows=64)
    assert sorted(r[0, :4].tolist()) == [0, 5, 6, 9] and (r[:, 4:] == -1).all() and np.isneginf(s[:, 4:]).all()
    c.assert_exact(N, 2)
    # without the bitmap the dead items are back, the empty ones are not
    s, r = Case(q, items, dim, tail_guard=4).assert_exact(N, 8)
    assert sorted(r[1, :6].tolist()) == [0, 2, 5, 6, 8, 9] and (r[:, 6:] == -1).all()
    # nothing alive: padding only
    s, r = Case(q, items, dim, alive=np.zeros(len(lens), bool)).run(N, 3)
    assert (r == -1).all() and np.isneginf(s).all()
    # an item longer than MAX_LATE_DOC_TOKENS is no candidate; its neighbours are
    s, r = Case(q, [int_rows(g, n, dim) for n in (20, 513, 20)], dim).assert_exact(N, 3, chunk_rows=128)
    assert sorted(r[0, :2].tolist()) == [0, 2] and r[0, 2] == -1
    # no items, or no rows
    for kw in (dict(n_items=0), dict(n_rows=0)):
        args = dict(n_items=3, n_rows=c.t_dev.shape[0])
        args.update(kw)
        s, r = N.maxsim_topk(c.q_dev, c.qs, c.ql, c.t_dev, args["n_rows"], c.off_dev, args["n_items"], dim, 2)
        assert (r.cpu().numpy() == -1).all() and np.isneginf(s.cpu().numpy()).all()


@pytest.fixture(scope="module")
def many_case():
    """20 000 items of 1..8 tokens (above the 16 384 candidate slots of k <= 512), two questions, planted winners: items
    that hold the question's own tokens"""
    dim = 64
    g = np.random.default_rng(77)
    q = [g.choice([-2.0, 2.0], (n, dim)).astype(np.float32) for n in (5, 8)]
    lens = g.integers(1, 9, 20000)
    items = [int_rows(g, n, dim) for n in lens]
    for j, i in enumerate((19999, 17, 12345, 16384, 8000, 3)):
        items[i][: min(len(items[i]), 1 + j)] = q[j % 2][: min(len(items[i]), 1 + j)]
    return Case(q, items, dim, tail_guard=1)


@pytest.mark.parametrize("k", [5, 100])
def test_bound_pass_is_exact(N, many_case, k):
    many_case.assert_exact(N, k)
    s, r = many_case.run(N, k)
    s2, r2 = many_case.run(N, k, dbg=1)          # no bound pass: every question overflows and is produced again alone
    assert np.array_equal(s.view(np.int32), s2.view(np.int32)) and np.array_equal(r, r2)


def test_all_items_tie_overflow_rerun(N):
    """20 000 identical items: every score ties, so every item is at or above the staged bound, the question overflows
    its slots and is produced again alone; the winners are items 0 .. k-1"""
    dim = 64
    g = np.random.default_rng(8)
    item = int_rows(g, 3, dim)
    q = [int_rows(g, 6, dim), int_rows(g, 2, dim)]
    c = Case.__new__(Case)
    c.dim, c.alive, c.bits, c.n_items = dim, None, None, 20000
    c.q_np, c.qs, c.ql = questions(q, dim)
    c.q_np = c.q_np.astype(np.float16)
    c.t_np = np.tile(item, (20000, 1)).astype(np.float16)
    c.off = (3 * np.arange(20001)).astype(np.int32)
    c.q_dev, c.t_dev, c.off_dev = (torch.from_numpy(x).cuda() for x in (c.q_np, c.t_np, c.off))
    one = R.score_matrix(c.q_np, c.qs, c.ql, c.t_np[:3], c.off[:2])[:, 0]
    for k in (5, 100):
        s, r = c.run(N, k)
        assert (r == np.arange(k)).all(), r
        assert np.array_equal(s, np.repeat(one.astype(np.float32)[:, None], k, axis=1))


def test_bad_question_gets_padding(N, grid_case):
    """the tables are device data: the wrapper checks its host copies; the kernel itself answers a question whose
    length is out of range or whose rows lie outside q_rows with padding, and the other questions as if it were absent"""
    c = grid_case
    qs, ql = c.qs.copy(), c.ql.copy()
    for bad in (dict(at=1, ql=0), dict(at=5, ql=129), dict(at=0, qs=-1), dict(at=10, qs=len(c.q_np) - 0)):
        qs2, ql2 = qs.copy(), ql.copy()
        if "ql" in bad:
            ql2[bad["at"]] = bad["ql"]
        if "qs" in bad:
            qs2[bad["at"]] = bad["qs"]
        with pytest.raises(N.MMRagNativeError, match="maxsim_topk: question"):
            N.maxsim_topk(c.q_dev, qs2, ql2, c.t_dev, len(c.t_np), c.off_dev, c.n_items, c.dim, 5)
        s, r = N.maxsim_topk(c.q_dev, qs2, ql2, c.t_dev, len(c.t_np), c.off_dev, c.n_items, c.dim, 5,
                             check_tables=False)
        s, r = s.cpu().numpy(), r.cpu().numpy()
        ref_s, ref_r = R.topk(c.q_np, qs2, ql2, c.t_np, c.off, 5)
        assert (r[bad["at"]] == -1).all() and np.isneginf(s[bad["at"]]).all(), bad
        assert np.array_equal(r, ref_r) and np.array_equal(s, ref_s.astype(np.float32)), bad


def test_wrapper_refusals(N, grid_case):
    c = grid_case
    ok = dict(q_tok=c.q_dev, q_start=c.qs, q_len=c.ql, tok=c.t_dev, n_rows=len(c.t_np), item_off=c.off_dev,
              n_items=c.n_items, dim=c.dim, k=5)
    for change, err in ((dict(k=0), ValueError), (dict(k=4097), ValueError), (dict(n_rows=len(c.t_np) + 1), N.MMRagNativeError),
                        (dict(n_items=c.n_items + 1), N.MMRagNativeError), (dict(q_len=c.ql[:3]), N.MMRagNativeError),
                        (dict(tok=c.t_dev.float()), N.MMRagNativeError), (dict(q_tok=c.q_dev.cpu()), N.MMRagNativeError),
                        (dict(alive_bits=torch.zeros(0, dtype=torch.int32, device="cuda")), N.MMRagNativeError),
                        (dict(dim=96), N.MMRagNativeError)):
        with pytest.raises(err):
            N.maxsim_topk(**{**ok, **change})


# ---------------------------------------------------------------- VectorIndex's token store
def test_index_store_add_delete_compact_add(N):
    """item = row through add / delete / compact / add again: late_search equals the reference over the live rows"""
    from multimodal_rag_amd.index import VectorIndex

    dim = 64
    g = np.random.default_rng(11)
    idx = VectorIndex(dim=dim, dtype=torch.float16)
    with pytest.raises(ValueError, match="token store"):
        idx.late_search(torch.zeros((4, dim), dtype=torch.float16, device="cuda"), [0], [4], 3)
    idx.enable_token_store(dim, 40)
    tokens = {}                     # id -> its token rows (none: the id keeps no tokens)

    def add(lo, hi, with_tokens=True):
        ids = [f"i{j}" for j in range(lo, hi)]
        idx.add(unit_rows(g, hi - lo, dim), documents=ids, metadatas=[{"par": j % 2} for j in range(lo, hi)], ids=ids)
        if with_tokens:
            lens = g.integers(0, 41, hi - lo)
            seqs = [int_rows(g, n, dim) for n in lens]
            idx.set_tokens(idx.rows_of_ids(ids), np.concatenate(seqs).astype(np.float16), lens,
                           [list(range(n)) for n in lens])
            tokens.update({s: x for s, x in zip(ids, seqs) if len(x)})

    q_seqs = [int_rows(g, n, dim) for n in (6, 33, 1)]
    q_np, qs, ql = questions(q_seqs, dim)
    q_dev = torch.from_numpy(q_np.astype(np.float16)).cuda()

    def check(k, where=None, live=None):
        s, r = idx.late_search(q_dev, qs, ql, k, where=where)
        s, r = s.cpu().numpy(), r.cpu().numpy()
        n = idx.rows_in_use
        ids = idx.ids_of_rows(range(n))
        row_live = np.array([i in idx._row_of for i in ids], bool) if live is None else live(ids)
        items = [tokens.get(i, np.zeros((0, dim), np.float32)) for i in ids]
        rows, off = plane(items, dim)
        ref_s, ref_r = R.topk(q_np.astype(np.float16), qs, ql, rows.astype(np.float16), off, k, row_live)
        assert np.array_equal(r, ref_r) and np.array_equal(s, ref_s.astype(np.float32)), (k, where)
        assert idx.token_store.offsets(n).tolist() == off.tolist()
        return r

    add(0, 30)
    check(5)
    add(30, 34, with_tokens=False)          # rows the store has not heard of: no candidates
    check(40)
    idx.delete(ids=[f"i{j}" for j in (0, 3, 4, 17, 29, 31)])
    r = check(40)
    assert not np.isin(r, [0, 3, 4, 17, 29, 31]).any()
    check(7, where={"par": 1}, live=lambda ids: np.array([i in idx._row_of and int(i[1:]) % 2 == 1 for i in ids]))
    idx.compact()
    assert idx.rows_in_use == 28
    check(40)
    add(34, 50)
    check(60)
    # a fill of the earlier rows that kept none
    late = [f"i{j}" for j in (30, 32, 33)]
    seqs = [int_rows(g, n, dim) for n in (3, 40, 1)]
    idx.set_tokens(idx.rows_of_ids(late), np.concatenate(seqs).astype(np.float16), [3, 40, 1])
    tokens.update(dict(zip(late, seqs)))
    check(60)
    res = idx.late_query(q_dev, qs, ql, n_results=3)
    assert set(res) >= {"ids", "distances", "documents", "metadatas", "late_scores"} and len(res["ids"]) == 3
    s, r = idx.late_search(q_dev, qs, ql, 3)
    assert res["ids"] == [idx.ids_of_rows(row) for row in r.cpu().tolist()]
    assert np.array_equal(np.asarray(res["late_scores"], np.float32),
                          (s / torch.tensor(ql, device="cuda").float()[:, None]).cpu().numpy())
    st = idx.token_stats()
    assert st["tokens"] == sum(len(x) for i, x in tokens.items() if i in idx._row_of) and st["bytes"] == st["tokens"] * 128
    idx.reset()
    assert idx.token_stats()["tokens"] == 0


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def manager(N):
    from multimodal_rag_amd import embedder as EM

    names = ("MMRAG_MODEL_DIR", "MMRAG_ENCODER_PRECISION", "MMRAG_RERANKER_DIR", "MMRAG_LATE_STORE",
             "MMRAG_LATE_STORE_MAX_BYTES")
    saved = [getattr(EM.settings, n) for n in names]
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION, EM.settings.MMRAG_RERANKER_DIR = "", "fp16", ""
    EM.settings.MMRAG_LATE_STORE, EM.settings.MMRAG_LATE_STORE_MAX_BYTES = False, 0
    try:
        yield EM.EmbeddingManager(engine=EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2"), enable_cache=False)
    finally:
        for n, v in zip(names, saved):
            setattr(EM.settings, n, v)


DOCS = ["the quick brown fox jumps over the lazy dog " * 3, "how do solar panels turn light into power",
        "a recipe for sourdough bread with a long cold proof " * 12, "solar power",
        "wind turbines and solar panels feed the grid " * 40, "alpha beta gamma delta " * 5, "bread"]
QUERY = "how do solar panels turn light into power"


def summaries(docs, lo=0):
    return [{"id": f"c{lo + i}", "type": "text", "summary": d} for i, d in enumerate(docs)]


def stored_hits(manager, ids):
    got = manager.collection.get(ids=ids)
    return {"ids": got["ids"], "distances": [0.5] * len(got["ids"]), "metadatas": got["metadatas"],
            "documents": got["documents"]}


def test_store_backed_rerank_and_late_query_end_to_end(N, manager, monkeypatch):
    """The re-encoding calls this test compares against hold more than 64 tokens per forward.  Below that the encoder's
    single-query GEMM kernels split K over waves and the SAME sequence gets other low bits than in any larger batch
    (measured: 2944 of 3840 halfs of a 10-token sequence differ, similarities by ~1e-5), so a re-encoding call that
    small is not bit-stable against itself in a larger batch either; the store keeps, and scores against, the rows
    of the batch-independent tile kernels."""
    import asyncio

    from starlette.testclient import TestClient

    from multimodal_rag_amd import embedder as EM
    from multimodal_rag_amd import server

    run = asyncio.run
    # one client for the whole test: closing it cleans the manager up (the collection goes with it)
    with TestClient(server.create_app(embedder=manager)) as c:
        _end_to_end(manager, monkeypatch, run, c, EM)


def _end_to_end(manager, monkeypatch, run, c, EM):
    run(manager.initialize())
    run(manager.delete_all_documents())
    assert manager.supports_late_store() and not manager.late_store_enabled() and not manager.supports_late_query()
    # ---- store off: uploads keep no tokens, late retrieval is refused the way the other opt-in modes are
    run(manager.embed_and_store(summaries(DOCS[:3]), "docA"))
    with pytest.raises(ValueError, match="token store"):
        run(manager.late_query(QUERY, 3))
    r = c.post("/query", json={"query": QUERY, "late": True})
    assert r.status_code == 400 and "token store" in r.json()["detail"], r.text
    ids_a = [f"docA_c{i}" for i in range(3)]
    plain = run(manager.late_rerank(QUERY, stored_hits(manager, ids_a), explain=True))     # the re-encoding path
    # ---- store on: the three stored documents are filled lazily, later uploads as they come
    stats = run(manager.enable_late_store())
    assert stats["items"] == 3 and stats["tokens"] > 0 and manager.supports_late_query()
    monkeypatch.setattr(EM.settings, "MMRAG_LATE_STORE", True)
    run(manager.embed_and_store(summaries(DOCS[3:], 3), "docB"))
    ids_b = [f"docB_c{i}" for i in range(3, len(DOCS))]
    stats = run(manager.get_collection_stats())["late_store"]
    assert stats["items"] == len(DOCS) and stats["bytes"] == stats["tokens"] * 768, stats
    scorer = manager._get_late()
    store = manager.collection.token_store
    want = scorer.plan(["x"], DOCS, [(0, j) for j in range(len(DOCS))])
    assert [store.length(r) for r in manager.collection.rows_of_ids(ids_a + ids_b)] == want["d_len"].tolist()
    assert store.token_ids(manager.collection.rows_of_ids([ids_a[1]])[0]) == want["d_ids"][1]

    # ---- re-rank: the store-backed call equals the re-encoding call, list against list, and encodes the question only
    seen = []
    real = scorer.encoder.encode_tokens
    monkeypatch.setattr(scorer.encoder, "encode_tokens",
                        lambda ids, lens, *a, **kw: (seen.append(np.asarray(lens).tolist()), real(ids, lens, *a, **kw))[1])
    backed = run(manager.late_rerank(QUERY, stored_hits(manager, ids_a), explain=True))
    assert backed == plain
    # ONE forward, and no passage in it: [CLS] question [SEP], and the filler that lifts a forward of <= 64 tokens out
    # of the single-query GEMM kernels (LateInteractionScorer._encode_stable) -- 65 tokens in all
    q_ids = len(scorer.plan([QUERY], ["x"], [(0, 0)])["q_ids"][0]) + 2
    assert seen == [[q_ids, 65 - q_ids]], seen
    # a hit with no stored tokens (an id the collection does not have) is re-encoded and still agrees; so is a batch
    mixed = stored_hits(manager, ids_a + ids_b)
    mixed["ids"] = [i if at % 2 else "unknown" + i for at, i in enumerate(mixed["ids"])]
    del seen[:]
    got = run(manager.batch_late_rerank([QUERY, "bread"], [mixed, stored_hits(manager, ids_b)], top_k=4))
    assert len(seen) == 1 and len(seen[0]) == 2 + (len(DOCS) + 1) // 2        # two questions + the unknown ids' texts
    monkeypatch.setattr(manager.collection, "_tokens", None)                   # the same calls without the store
    alone = run(manager.batch_late_rerank([QUERY, "bread"], [mixed, stored_hits(manager, ids_b)], top_k=4))
    monkeypatch.undo()
    assert got == alone and got[0]["ids"][0] == ids_a[1]
    monkeypatch.setattr(EM.settings, "MMRAG_LATE_STORE", True)

    # ---- first-stage retrieval: the document equal to the query first; the full ranking is late_rerank of ALL documents
    found = run(manager.late_query(QUERY, n_results=len(DOCS)))
    assert found["ids"][0] == ids_a[1] and found["late_scores"][0] >= 0.9996, found["late_scores"]
    everything = run(manager.late_rerank(QUERY, stored_hits(manager, ids_a + ids_b)))
    assert found["ids"] == everything["ids"] and found["late_scores"] == everything["rerank_scores"]
    assert found["distances"] == [float(np.float32(1.0) - np.float32(s)) for s in found["late_scores"]]
    both = run(manager.batch_late_query([QUERY, "", "bread"], n_results=2))
    assert both[0]["ids"] == found["ids"][:2] and "error" in both[1] and both[2]["ids"][0] == ids_b[-1]
    only_b = run(manager.late_query(QUERY, n_results=10, filter_dict={"doc_id": "docB"}))
    assert only_b["ids"] == [i for i in found["ids"] if i.startswith("docB")]
    r = c.post("/query", json={"query": QUERY, "top_k": 4, "late": True})
    assert r.status_code == 200, r.text
    src = r.json()["sources"]
    assert [s["doc_id"] for s in src] == found["ids"][:4]
    assert [s["late_score"] for s in src] == found["late_scores"][:4]
    # no pooled search ran: relevance_score is the late score (rounded as every relevance_score is)
    assert all(abs(s["relevance_score"] - s["late_score"]) <= 1e-3 for s in src)
    r = c.post("/query", json={"query": QUERY, "late": True, "hybrid": True})
    assert r.status_code == 400 and "Late retrieval is not combined" in r.json()["detail"]
    # ---- the cap: a row past it keeps no tokens, is re-encoded by a re-rank and is no candidate of late_query
    manager.collection.token_store.max_bytes = manager.collection.token_store.stats()["bytes"] + 768
    run(manager.embed_and_store(summaries(["solar panels on the roof turn light into power"], 20), "docC"))
    row = manager.collection.rows_of_ids(["docC_c20"])[0]
    assert row >= 0 and manager.collection.token_store.length(row) == 0
    capped = run(manager.late_rerank(QUERY, stored_hits(manager, ids_a + ["docC_c20"])))
    monkeypatch.setattr(manager.collection, "_tokens", None)
    uncapped = run(manager.late_rerank(QUERY, stored_hits(manager, ids_a + ["docC_c20"])))
    monkeypatch.undo()
    assert capped == uncapped and "docC_c20" in capped["ids"]
    assert "docC_c20" not in run(manager.late_query(QUERY, n_results=20))["ids"]


# ---------------------------------------------------------------- ids, locks and batch shapes
def test_tokens_are_written_and_read_by_id_under_the_index_lock(N):
    """what an upload does around its encoder forward, with a delete that compacts in between: the token rows land
    under the rows their ids have NOW; an id that is gone is dropped, an id whose row keeps tokens is left alone; and
    a snapshot of spans names the plane it was taken from"""
    from multimodal_rag_amd.index import VectorIndex

    dim = 64
    g = np.random.default_rng(21)
    idx = VectorIndex(dim=dim, dtype=torch.float16)
    idx.enable_token_store(dim, 8)
    ids = [f"a{j}" for j in range(6)]
    idx.add(unit_rows(g, 6, dim), documents=ids, ids=ids)

    def rows_for(tag, lens):
        x = np.zeros((int(sum(lens)), dim), np.float16)
        x[:, 0] = tag + np.arange(len(x))
        return x

    def stored(i):
        (span,), plane, _ = idx.token_spans([[i]])
        return None if span is None else plane[span[0]: span[0] + span[1], 0].cpu().numpy().astype(int).tolist()

    assert idx.set_tokens_for_ids(ids[:3], rows_for(100, [2, 3, 1]), [2, 3, 1]) == 3
    assert idx.ids_without_tokens(ids + ["nobody"]) == ids[3:]
    # an upload resolved a3 .. a5, its forward runs ... and a delete compacts the rows away under it
    idx.delete(ids=["a0", "a4"])
    idx.compact()
    assert idx.rows_of_ids(ids) == [-1, 0, 1, 2, -1, 3]
    assert idx.set_tokens_for_ids(ids[3:], rows_for(200, [2, 2, 2]), [2, 2, 2], [[1, 2], [3, 4], [5, 6]]) == 2
    assert [stored(i) for i in ids] == [None, [102, 103, 104], [105], [200, 201], None, [204, 205]]
    assert idx.token_store.token_ids(3) == [5, 6] and idx.token_store.offsets(4).tolist() == [0, 3, 4, 6, 8]
    # an id that exists keeps the tokens of the document stored under it; only_empty=False replaces them
    assert idx.set_tokens_for_ids(["a1", "a3"], rows_for(300, [1, 1]), [1, 1]) == 0 and stored("a1") == [102, 103, 104]
    assert idx.set_tokens_for_ids(["a1"], rows_for(300, [1]), [1], only_empty=False) == 1 and stored("a1") == [300]
    # a snapshot outlives a fill and a compaction: its plane is the one its spans index
    spans, plane, most = idx.token_spans([["a2", "zz"], ["a5"]], with_ids=True)
    assert most == 8 and spans[1] is None and spans[2][2] == [5, 6]
    idx.delete(ids=["a1"])
    idx.compact()
    assert plane[spans[0][0], 0].item() == 105 and plane[spans[2][0], 0].item() == 204 and stored("a2") == [105]
    idx.reset()
    assert idx.set_tokens_for_ids(["a2"], rows_for(1, [1]), [1]) == 0        # nothing to misplace after a reset


def test_a_question_past_the_tile_bound_gets_padding(N, grid_case):
    """max_tiles below the tiles the questions need (a caller whose host tables disagree with the device's): the
    questions that fit are answered, the others get padding, nothing is written outside the packed tiles"""
    c = grid_case
    Q = len(c.ql)
    tabs = torch.from_numpy(np.concatenate([c.qs, c.ql])).cuda()
    s, r = N._topk_out(Q, 3, c.q_dev.device)
    ws = torch.empty(N.maxsim_topk_workspace_bytes(Q, c.n_items, 3, c.dim, 2), dtype=torch.uint8, device="cuda")
    st = N.lib().mmrag_internal_maxsim_topk_ex(
        c.q_dev.data_ptr(), c.q_dev.shape[0], c.dim, tabs.data_ptr(), tabs[Q:].data_ptr(), Q, c.t_dev.data_ptr(),
        len(c.t_np), c.dim, c.off_dev.data_ptr(), c.n_items, None, c.dim, 3, s.data_ptr(), r.data_ptr(), ws.data_ptr(),
        ws.numel(), torch.cuda.current_stream().cuda_stream, 0, 0, 0, 2)
    assert st == 0
    ref_s, ref_r = R.topk_of_scores(c.scores, 3)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert np.array_equal(r[:7], ref_r[:7]) and np.array_equal(s[:7], ref_s[:7].astype(np.float32))   # tiles 0 and 1
    assert (r[7:] == -1).all() and np.isneginf(s[7:]).all()


def test_token_row_bits_do_not_depend_on_the_batch_above_64_tokens(N, manager):
    """What the store relies on: in every forward of more than 64 tokens a sequence's token rows have the same bits,
    whichever GEMM tile kernel the batch size selects -- 65 tokens, a few hundred, an ingest batch of 64 x 256 -- and
    LateInteractionScorer._encode_stable gives those bits to a forward that would be smaller."""
    import asyncio

    asyncio.run(manager.initialize())
    scorer = manager._get_late()
    enc = scorer.encoder
    g = np.random.default_rng(31)
    seq = g.integers(1000, 20000, 12).astype(np.int32)
    long = g.integers(1000, 20000, 200).astype(np.int32)

    def rows(others, which, at=0):
        batch = list(others)
        batch.insert(at, which)
        ids = np.zeros((len(batch), max(len(b) for b in batch)), np.int32)
        for i, b in enumerate(batch):
            ids[i, : len(b)] = b
        tokens, cu = enc.encode_tokens(ids, np.array([len(b) for b in batch], np.int32))
        return tokens[cu[at]: cu[at + 1]].view(torch.int16).cpu().numpy()

    fill = lambda n, m: [g.integers(1000, 20000, m).astype(np.int32) for _ in range(n)]      # noqa: E731
    for which in (seq, long):
        base = rows(fill(1, 65 - min(len(which), 12)), which)             # 65 tokens (the short one), 253 (the long)
        for others, at in ((fill(5, 60), 0), (fill(5, 60), 5), (fill(63, 256), 0), (fill(63, 256), 40), (fill(20, 120), 3)):
            assert np.array_equal(rows(others, which, at), base), (len(which), len(others), at)
    stable, _ = scorer._encode_stable(seq[None, :], np.array([12], np.int32))
    assert stable.shape[0] == 12 and np.array_equal(stable.view(torch.int16).cpu().numpy(), rows(fill(1, 53), seq))
    alone = enc.encode_tokens(seq[None, :], np.array([12], np.int32))[0].view(torch.int16).cpu().numpy()
    print("halfs of a 12-token sequence that differ between a forward of its own and a larger one:",
          int((alone != rows(fill(1, 53), seq)).sum()), "of", alone.size)
