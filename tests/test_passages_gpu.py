"""GPU: answer passages -- the windowed MaxSim kernel (csrc/maxsim_windows.hip) against tests/passage_ref.py, bit for
bit, and the layers above it.

Tolerances: none.
  integer rows ....... entries in {-2..2} (FP8: x * 256 in {-2..2}): every dot product and every sum is an integer (times
                       2^-16) below 2^24, exact in float32; out_sum, all 32 slots of out_win and out_best are compared
                       bit for bit with the float64 reference
  random unit rows ... the similarity matrix S is taken from mmrag_maxsim_scores itself (each passage token scored as a
                       one-token passage: best_sim IS S, bit for bit) and the reference's block and window steps run on
                       it in float32, so every output is again compared bit for bit
"""
import numpy as np
import pytest
import torch

from tests import late_f8_ref, passage_ref

pytestmark = pytest.mark.gpu

SLOTS = 32
GUARD = 100.0   # rows between sequences: a read outside a sequence shows as a huge similarity
D_LENS = (1, 15, 16, 17, 128, 129, 300, 512)
Q_LENS = (1, 5, 128)
WIDTHS = (1, 2, 4, 32)


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def layout(seqs, dim, guard_rows=3):
    """sequences (float arrays [len, dim]) -> (rows [n, dim] float32 with GUARD-filled rows before, between and after
    them; starts; lens)"""
    parts, starts, at = [], [], 0
    for s in seqs:
        parts.append(np.full((guard_rows, dim), GUARD, np.float32))
        at += guard_rows
        parts.append(np.asarray(s, np.float32))
        starts.append(at)
        at += len(s)
    parts.append(np.full((guard_rows, dim), GUARD, np.float32))
    return np.concatenate(parts), np.array(starts, np.int32), np.array([len(s) for s in seqs], np.int32)


class Rows:
    """the two row buffers of a launch on the device, fp16 unit rows or E4M3 code rows, and what the reference reads"""

    def __init__(self, N, f8, q_rows, d_rows, dim):
        self.N, self.f8, self.dim = N, f8, dim
        dev = [torch.from_numpy(np.ascontiguousarray(r)).cuda().half().contiguous() for r in (q_rows, d_rows)]
        if f8:
            dev = [N.f8_encode_rows(r, dim) for r in dev]
            self.values = [late_f8_ref.values(r.cpu().numpy())[:, :dim] for r in dev]
        else:
            self.values = [r.cpu().numpy().astype(np.float64) for r in dev]
        self.q, self.d = dev

    def windows(self, tables, w):
        fn = self.N.maxsim_windows_f8 if self.f8 else self.N.maxsim_windows
        out = fn(self.q, self.d, self.dim, *tables, w)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]

    def scores(self, tables, want_best=True):
        fn = self.N.maxsim_scores_f8 if self.f8 else self.N.maxsim_scores
        out = fn(self.q, self.d, self.dim, *tables, want_best=want_best)
        torch.cuda.synchronize()
        return [o.cpu().numpy() if o is not None else None for o in out]


def assert_equals_reference(got, ref, note=""):
    sums, win, best = got
    assert win.shape == (len(ref), SLOTS) and best.shape == (len(ref), 3)
    for p, (r_sum, r_win, r_best) in enumerate(ref):
        assert bits(sums[p]) == bits(r_sum), (note, p, sums[p], r_sum)
        assert np.array_equal(bits(win[p]), bits(r_win)), (note, p, win[p], r_win)
        assert tuple(best[p]) == r_best, (note, p, best[p], r_best)


def int_rows(g, n, dim, f8):
    x = g.integers(-2, 3, (n, dim)).astype(np.float32)
    return x / 256.0 if f8 else x


# ---------------------------------------------------------------- 1 / 4: integer rows, the float64 reference
@pytest.mark.parametrize("f8", [False, True], ids=["fp16", "f8"])
@pytest.mark.parametrize("dim", [64, 384])
def test_integer_exact_grid(N, dim, f8):
    """every (q_len, d_len) of the grid in one launch per width (dim 384: every other pair, two widths), sequences at
    non-zero starts between GUARD rows and shared between pairs"""
    g = np.random.default_rng(300 + dim)
    q_seqs = [int_rows(g, n, dim, f8) for n in Q_LENS]
    d_seqs = [int_rows(g, n, dim, f8) for n in D_LENS]
    pairs = [(a, b) for a in range(len(Q_LENS)) for b in range(len(D_LENS)) if dim == 64 or (a + b) % 2 == 0]
    qr, qs, ql = layout(q_seqs, dim)
    dr, ds, dl = layout(d_seqs, dim, guard_rows=5)
    rows = Rows(N, f8, qr, dr, dim)
    tables = (qs, ql, ds, dl, [a for a, _ in pairs], [b for _, b in pairs])
    ties = 0
    for w in WIDTHS if dim == 64 else (2, 32):
        ref = passage_ref.windows_of_tables(rows.values[0], rows.values[1], *tables, w)
        got = rows.windows(tables, w)
        assert_equals_reference(got, ref, note=f"w={w}")
        ties += sum(int((r_win == r_win.max()).sum() > 1) for _, r_win, _ in ref)
        for p, (_, b) in enumerate(pairs):
            if w * 16 >= D_LENS[b]:        # one window: the whole passage
                assert bits(got[1][p, 0]) == bits(got[0][p]) and np.isneginf(got[1][p, 1:]).all()
        again = rows.windows(tables, w)     # identical calls give identical bits
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(got, again))
    print(f"dim {dim} f8={f8}: {ties} cases with tied best windows")


# ---------------------------------------------------------------- 2 / 4: random unit rows, S from the pair kernel
def unit_rows(g, n, dim):
    x = g.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("f8", [False, True], ids=["fp16", "f8"])
def test_same_bits_as_the_pair_kernel(N, f8):
    dim, q_lens, d_lens = 384, (5, 128), (17, 129, 300)
    g = np.random.default_rng(17)
    q_seqs = [unit_rows(g, n, dim) for n in q_lens]
    d_seqs = [unit_rows(g, n, dim) for n in d_lens]
    qr, qs, ql = layout(q_seqs, dim)
    dr, ds, dl = layout(d_seqs, dim)
    rows = Rows(N, f8, qr, dr, dim)
    # S of (question a, passage b): every passage token as a one-token passage; best_sim[.][i] is then S[i][j]
    tok_start = np.concatenate([s + np.arange(n) for s, n in zip(ds, dl)]).astype(np.int32)
    first_tok = np.concatenate([[0], np.cumsum(dl)])
    S = {}
    for a, n_q in enumerate(q_lens):
        _, best_sim, _ = rows.scores((qs, ql, tok_start, np.ones_like(tok_start), [a] * len(tok_start),
                                      list(range(len(tok_start)))))
        for b in range(len(d_lens)):
            S[a, b] = best_sim[first_tok[b]: first_tok[b + 1], :n_q].T.copy()
            assert S[a, b].dtype == np.float32 and S[a, b].shape == (n_q, d_lens[b])
    pairs = [(a, b) for a in range(len(q_lens)) for b in range(len(d_lens))]
    tables = (qs, ql, ds, dl, [a for a, _ in pairs], [b for _, b in pairs])
    pair_sums = rows.scores(tables, want_best=False)[0]
    for w in (1, 3, 4, 32):
        got = rows.windows(tables, w)
        assert_equals_reference(got, [passage_ref.windows(S[a, b], w) for a, b in pairs], note=f"w={w}")
        assert np.array_equal(bits(got[0]), bits(pair_sums))
        if w == 32:
            assert np.array_equal(bits(got[1][:, 0]), bits(pair_sums))


# ---------------------------------------------------------------- 3: padding and neighbours
@pytest.mark.parametrize("f8", [False, True], ids=["fp16", "f8"])
@pytest.mark.parametrize("w", [1, 2])
def test_padding_and_the_next_passage_stay_out(N, f8, w):
    """17 passage tokens whose similarities are all negative: the 15 pad columns of block 1 would score 0, and the rows
    right behind the passage are another passage whose tokens ARE the question's"""
    dim, scale = 64, (1.0 / 256.0 if f8 else 1.0)
    g = np.random.default_rng(5)
    q = g.integers(1, 3, (20, dim)).astype(np.float32) * scale
    d = -g.integers(1, 3, (17, dim)).astype(np.float32) * scale
    rows = Rows(N, f8, q, np.concatenate([d, q]), dim)
    tables = ([0], [20], [0, 17], [17, 20], [0, 0], [0, 1])
    sums, win, best = got = rows.windows(tables, w)
    assert_equals_reference(got, passage_ref.windows_of_tables(rows.values[0], rows.values[1], *tables, w))
    n_win = 3 - w
    assert sums[0] < 0 and (win[0, :n_win] < 0).all() and np.isneginf(win[0, n_win:]).all()
    assert 0 <= best[0, 1] <= best[0, 2] <= 1
    assert sums[1] > 0      # the neighbour, as its own pair, is the match it looks like


# ---------------------------------------------------------------- 5: bad pairs
@pytest.mark.parametrize("f8", [False, True], ids=["fp16", "f8"])
def test_bad_pairs_get_nan_and_leave_the_others_alone(N, f8):
    """the C entry with tables the wrapper would refuse: a pair index out of range, a d_len of 0 and a d_len of 513"""
    dim, w = 64, 2
    g = np.random.default_rng(11)
    q_seqs = [int_rows(g, n, dim, f8) for n in (5, 128)]
    d_seqs = [int_rows(g, n, dim, f8) for n in (40, 129)]
    qr, qs, ql = layout(q_seqs, dim)
    dr, ds, dl = layout(d_seqs + [int_rows(g, 520, dim, f8)], dim)
    rows = Rows(N, f8, qr, dr, dim)
    good = [(0, 0), (1, 1), (0, 1), (1, 0)]
    want = rows.windows((qs, ql, ds[:2], dl[:2], [a for a, _ in good], [b for _, b in good]), w)
    # passage 2: 513 tokens that do lie inside the buffer; passage 3: no tokens
    d_start, d_len = list(ds) + [0], list(dl[:2]) + [513, 0]
    pairs = [good[0], (0, 4), good[1], (1, 3), good[2], (2, 0), (0, 2), good[3], (0, -1)]
    t = torch.tensor(list(qs) + list(ql) + d_start + d_len + [a for a, _ in pairs] + [b for _, b in pairs],
                     dtype=torch.int32, device="cuda")
    P = len(pairs)
    sums = torch.full((P,), 7.0, dtype=torch.float32, device="cuda")
    win = torch.full((P, SLOTS), 7.0, dtype=torch.float32, device="cuda")
    best = torch.full((P, 3), 7, dtype=torch.int32, device="cuda")
    at = t.data_ptr()
    fn = N.lib().mmrag_maxsim_windows_f8 if f8 else N.lib().mmrag_maxsim_windows
    st = fn(rows.q.data_ptr(), rows.q.shape[0], rows.q.shape[1], rows.d.data_ptr(), rows.d.shape[0], rows.d.shape[1],
            dim, at, at + 8, 2, at + 16, at + 32, 4, at + 48, at + 48 + 4 * P, P, w, sums.data_ptr(), win.data_ptr(),
            best.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    sums, win, best = sums.cpu().numpy(), win.cpu().numpy(), best.cpu().numpy()
    at_good = [pairs.index(p) for p in good]
    for p in range(P):
        if p in at_good:
            continue
        assert np.isnan(sums[p]) and best[p].tolist() == [-1, -1, -1], (p, sums[p], best[p])
        assert (win[p] == 7.0).all()        # the row of a refused pair is not written
    assert np.array_equal(bits(sums[at_good]), bits(want[0]))
    assert np.array_equal(bits(win[at_good]), bits(want[1]))
    assert np.array_equal(best[at_good], want[2])


# ---------------------------------------------------------------- 6: the scorer, the token store, the re-rank
@pytest.fixture(scope="module")
def manager(N):
    from multimodal_rag_amd import embedder as EM

    names = ("MMRAG_MODEL_DIR", "MMRAG_ENCODER_PRECISION", "MMRAG_RERANKER_DIR", "MMRAG_LATE_STORE",
             "MMRAG_LATE_STORE_MAX_BYTES", "MMRAG_LATE_STORE_DTYPE")
    saved = [getattr(EM.settings, n) for n in names]
    EM.settings.MMRAG_MODEL_DIR, EM.settings.MMRAG_ENCODER_PRECISION, EM.settings.MMRAG_RERANKER_DIR = "", "fp16", ""
    EM.settings.MMRAG_LATE_STORE, EM.settings.MMRAG_LATE_STORE_MAX_BYTES = False, 0
    EM.settings.MMRAG_LATE_STORE_DTYPE = "float16"
    try:
        yield EM.EmbeddingManager(engine=EM.HipEngine("sentence-transformers/all-MiniLM-L6-v2"), enable_cache=False)
    finally:
        for n, v in zip(names, saved):
            setattr(EM.settings, n, v)


DOCS = ["the quick brown fox jumps over the lazy dog " * 3, "how do solar panels turn light into power",
        "a recipe for sourdough bread with a long cold proof " * 12, "solar power",
        "wind turbines and solar panels feed the grid " * 40, "alpha beta gamma delta " * 5]
QUERY = "how do solar panels turn light into power"


def test_scorer_best_passages_equal_the_reference(N, manager):
    """a small random-weight encoder: the scorer's records are the reference's block and window steps over the
    similarities of the scorer's own token rows (read back through the pair kernel, one passage token at a time)"""
    scorer = manager._get_late()
    assert manager.supports_passages()
    queries, window = [QUERY, "bread and a fox"], 32
    pairs = [(a, b) for a in range(2) for b in range(len(DOCS))]
    got = scorer.best_passages(queries, DOCS, pairs, window)
    plan = scorer.plan(queries, DOCS, pairs)
    tokens, _ = scorer.encoder.encode_tokens(plan["ids"], plan["lens"])
    dim = tokens.shape[1]
    torch.cuda.synchronize()
    tok_start = np.concatenate([s + np.arange(n) for s, n in zip(plan["d_start"], plan["d_len"])]).astype(np.int32)
    first_tok = np.concatenate([[0], np.cumsum(plan["d_len"])])
    plain = scorer.score_pairs(queries, DOCS, pairs)
    assert len(got) == len(pairs) and scorer.window_blocks(window) == 2
    for p, rec in enumerate(got):
        a, b = int(plan["pair_q"][p]), int(plan["pair_d"][p])
        q_len, d_len = int(plan["q_len"][a]), int(plan["d_len"][b])
        _, best_sim, _ = N.maxsim_scores(tokens, tokens, dim, plan["q_start"], plan["q_len"], tok_start,
                                         np.ones_like(tok_start), [a] * d_len,
                                         list(range(first_tok[b], first_tok[b + 1])))
        S = best_sim.cpu().numpy()[:, :q_len].T
        r_sum, r_win, (start, first, last) = passage_ref.windows(S, 2)
        assert bits(rec["sum"]) == bits(r_sum) and bits(rec["window_sum"]) == bits(r_win[start]), (p, rec, r_sum)
        assert bits(rec["score"]) == bits(r_sum / np.float32(q_len)) == bits(plain[p])
        assert bits(rec["window_score"]) == bits(r_win[start] / np.float32(q_len))
        assert (rec["window_start"], rec["window_end"]) == (16 * start, min(16 * (start + 2), d_len))
        assert (rec["token_start"], rec["token_end"]) == (16 * first, min(16 * (last + 1), d_len))
        n_win = max(-(-d_len // 16) - 2, 0) + 1
        assert np.array_equal(bits(rec["window_scores"]), bits(r_win[:n_win] / np.float32(q_len)))
        assert rec["doc_ids"] == plan["d_ids"][b]
    # the passage equal to the question: every token finds itself, in the one block there is
    assert got[1]["token_start"] == 0 and got[1]["token_end"] == len(plan["d_ids"][1]) and got[1]["score"] >= 0.9996


def test_store_backed_passages_and_rerank_order(N, manager):
    """hits scored from an fp16 token store give the bits of the same hits re-encoded (forwards of more than 64 tokens,
    as tests/test_late_store_gpu.py explains), and asking for passages changes neither order nor scores of a re-rank"""
    import asyncio

    run = asyncio.run
    run(manager.initialize())
    run(manager.delete_all_documents())
    run(manager.embed_and_store([{"id": f"c{i}", "type": "text", "summary": d} for i, d in enumerate(DOCS)], "docP"))
    ids = [f"docP_c{i}" for i in range(len(DOCS))]
    got = manager.collection.get(ids=ids)
    hits = {"ids": got["ids"], "distances": [0.5] * len(ids), "metadatas": got["metadatas"], "documents": got["documents"]}
    assert hits["documents"] == DOCS
    without = run(manager.late_rerank(QUERY, hits))
    plain = run(manager.late_rerank(QUERY, hits, passages=64))
    assert {k: plain[k] for k in without} == without and set(plain) == set(without) | {"passages"}
    assert plain["ids"][0] == ids[1] and plain["passages"][0]["text"] == QUERY and plain["passages"][0]["share"] == 1.0
    for found, doc in zip(plain["passages"], plain["documents"]):
        assert found["text"] == doc[found["char_start"]: found["char_end"]] and 0.0 < found["share"] <= 1.0
        assert doc[found["char_start"]: found["char_end"]].strip() == found["text"] and found["text"]
    alone = run(manager.extract_passages(QUERY, hits, window_tokens=64))
    assert alone["ids"] == hits["ids"] and sorted(map(str, alone["passages"])) == sorted(map(str, plain["passages"]))
    stats = run(manager.enable_late_store())
    assert stats["items"] == len(DOCS) and manager.late_store_enabled()
    try:
        backed = run(manager.late_rerank(QUERY, hits, passages=64))
        assert backed == plain
        assert run(manager.extract_passages(QUERY, hits, window_tokens=64)) == alone
    finally:
        run(manager.delete_all_documents())
        manager.collection._tokens = None       # the next test of this module attaches its own store


def test_f8_store_passages_from_the_plane_equal_forced_re_encoding(N, manager, monkeypatch):
    """an FP8 token store: a hit's passage is the same from the plane's codes as forced through re-encoding (ids the store
    does not know: the scorer quantises what it encodes), and asking for passages leaves order and scores alone"""
    import asyncio

    from multimodal_rag_amd import embedder as EM

    run = asyncio.run
    monkeypatch.setattr(EM.settings, "MMRAG_LATE_STORE", True)
    monkeypatch.setattr(EM.settings, "MMRAG_LATE_STORE_DTYPE", "float8_e4m3fn")
    run(manager.initialize())
    run(manager.delete_all_documents())
    try:
        run(manager.embed_and_store([{"id": f"c{i}", "type": "text", "summary": d} for i, d in enumerate(DOCS)], "docF"))
        ids = [f"docF_c{i}" for i in range(len(DOCS))]
        store = manager.collection.token_store
        assert store is not None and store.f8 and store.stats()["items"] == len(DOCS)
        got = manager.collection.get(ids=ids)
        hits = {"ids": got["ids"], "distances": [0.5] * len(ids), "metadatas": got["metadatas"],
                "documents": got["documents"]}
        without = run(manager.late_rerank(QUERY, hits))
        backed = run(manager.late_rerank(QUERY, hits, passages=64))
        assert {k: backed[k] for k in without} == without
        assert backed["ids"][0] == ids[1] and backed["passages"][0]["text"] == QUERY
        for other in ({**hits, "ids": ["unknown" + i for i in ids]},
                      {**hits, "ids": [i if at % 2 else "unknown" + i for at, i in enumerate(ids)]}):
            again = run(manager.late_rerank(QUERY, other, passages=64))
            assert [i.replace("unknown", "") for i in again["ids"]] == backed["ids"]
            assert again["rerank_scores"] == backed["rerank_scores"] and again["passages"] == backed["passages"]
    finally:
        run(manager.delete_all_documents())
        manager.collection._tokens = None
