"""GPU: learned sparse retrieval -- the fused vocabulary projection + per-chunk max (mmrag_sparse_pool), activation /
quantisation / top-m (mmrag_sparse_select), exact integer impact scoring (mmrag_impact_topk) and the path above them
(DeviceSparseEncoder, VectorIndex, EmbeddingManager, POST /query) against tests/sparse_ref.py."""
import asyncio

import numpy as np
import pytest
import torch

from tests import sparse_ref as R
from tests.test_sparse_cpu import (E2E_SHAPE, e2e_sequences, e2e_weights, random_select_case, select_grid_case,
                                   synthetic_log)

pytestmark = pytest.mark.gpu

CHUNK_LENS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 512]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


def _pool(dev, tok, cu, E, dim):
    from multimodal_rag_amd import _native

    t = torch.from_numpy(tok).to(dev)
    e = torch.from_numpy(E).to(dev)
    c = torch.from_numpy(np.asarray(cu, np.int32)).to(dev)
    return _native.sparse_pool(t, c, e, dim).cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ---- pool -------------------------------------------------------------------------------------------------------------
def pool_case(dim, signed, seed):
    """integer-valued fp16 rows in -4..4 (every dot product exact).  `signed`: chunks alternate between all-negative
    and large positive logits (decoder rows >= 1 everywhere, token rows of one sign), so one leaked neighbour row, or
    one zero row past T or past V, shows as a wrong maximum"""
    g = np.random.default_rng(seed)
    lens = CHUNK_LENS + CHUNK_LENS[::-1]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, V = int(cu[-1]), 300
    assert T % 128 != 0
    if signed:
        E = g.integers(1, 5, (V, dim))
        tok = g.integers(0, 5, (T, dim))
        tok[:, 0] = np.maximum(tok[:, 0], 1)           # no zero row
        sign = np.repeat(np.where(np.arange(len(lens)) % 2 == 0, -1, 1), lens)
        tok = tok * sign[:, None]
    else:
        E = g.integers(-4, 5, (V, dim))
        tok = g.integers(-4, 5, (T, dim))
    return tok.astype(np.float16), cu, E.astype(np.float16)


@pytest.mark.parametrize("dim", [64, 384])
@pytest.mark.parametrize("signed", [True, False])
def test_pool_bit_exact_and_packing_independent(dev, dim, signed):
    tok, cu, E = pool_case(dim, signed, seed=dim + int(signed))
    ref = R.pool(tok, cu, E).astype(np.float32)
    got = _pool(dev, tok, cu, E, dim)
    assert got.shape == ref.shape
    assert np.array_equal(_bits(got), _bits(ref))
    if signed:
        neg = np.arange(len(cu) - 1) % 2 == 0
        assert (got[neg] < 0).all() and (got[~neg] > 0).all()
    # the bits do not depend on the grid: one vocabulary tile per workgroup, and all three in one run
    from multimodal_rag_amd import _native

    dev_args = (torch.from_numpy(tok).to(dev), torch.from_numpy(cu).to(dev), torch.from_numpy(E).to(dev), dim)
    for vrun in (1, 3):
        assert np.array_equal(_bits(_native.sparse_pool(*dev_args, vrun=vrun).cpu().numpy()), _bits(got)), vrun
    # the same chunks one per call: the bits do not depend on the packing
    for c in range(len(cu) - 1):
        rows = np.ascontiguousarray(tok[cu[c]: cu[c + 1]])
        one = _pool(dev, rows, [0, rows.shape[0]], E, dim)
        assert np.array_equal(_bits(one[0]), _bits(got[c])), c


def test_pool_bad_chunks_get_minus_inf(dev):
    tok, cu, E = pool_case(64, False, seed=3)
    T = tok.shape[0]
    bad = np.asarray([0, 5, 5, 5 + 513, 5 + 513 + 3, T + 1], np.int32)      # empty, over-long, fine, past T
    got = _pool(dev, tok, bad, E, 64)
    ref = R.pool(tok, bad, E).astype(np.float32)
    assert np.isneginf(got[1]).all() and np.isneginf(got[2]).all() and np.isneginf(got[4]).all()
    assert np.array_equal(_bits(got), _bits(ref))


def test_pool_random_rows_within_the_float32_bound(dev):
    g = np.random.default_rng(11)
    dim, V = 768, 1000
    lens = [7, 130, 64, 300, 33, 1]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    tok = g.standard_normal((int(cu[-1]), dim)).astype(np.float16)
    E = g.standard_normal((V, dim)).astype(np.float16)
    ref, mag = R.pool_with_bound(tok, cu, E)
    got = _pool(dev, tok, cu, E, dim).astype(np.float64)
    bound = 2.0 * dim * 2.0 ** -24 * mag
    worst = float((np.abs(got - ref) / bound).max())
    print(f"pool random rows: worst |delta| / bound = {worst:.4f}")
    assert (np.abs(got - ref) <= bound).all()


def test_pool_rejects_bad_arguments_before_any_launch(dev):
    from multimodal_rag_amd import _native

    tok = torch.zeros((4, 64), dtype=torch.float16, device=dev)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    with pytest.raises(_native.MMRagNativeError):
        _native.sparse_pool(tok, cu, tok, 32)                      # dim not a multiple of 64
    with pytest.raises(_native.MMRagNativeError):
        _native.sparse_pool(tok, cu, tok, 128)                     # dim > ld
    wide = torch.zeros((4, 96), dtype=torch.float16, device=dev)
    with pytest.raises(_native.MMRagNativeError):
        _native.sparse_pool(wide, cu, wide, 64)                    # pitch not whole slabs
    L = _native.lib()
    assert L.mmrag_sparse_pool(None, 4, 64, cu.data_ptr(), 1, tok.data_ptr(), 4, 64, 64, tok.data_ptr(), None, 0,
                               None) == 1
    assert L.mmrag_sparse_pool(tok.data_ptr(), 4, 64, cu.data_ptr(), 1, tok.data_ptr(), 70000, 64, 64,
                               tok.data_ptr(), None, 0, None) == 1
    assert L.mmrag_sparse_pool(tok.data_ptr(), 4, 64, cu.data_ptr(), 0, tok.data_ptr(), 4, 64, 64, tok.data_ptr(),
                               None, 0, None) == 1


# ---- select -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 32, 256])
def test_select_exact_on_the_grid(dev, m):
    from multimodal_rag_amd import _native

    pooled, bias, skip, scale = select_grid_case()
    ref_cnt, ref_terms, ref_imp = R.select_batch(R.impacts(pooled, bias, scale), m, skip)
    cnt, terms, imps = _native.sparse_select(torch.from_numpy(pooled).to(dev), torch.from_numpy(bias).to(dev), scale, m,
                                             torch.from_numpy(R.bool_to_bits(skip)).to(dev))
    assert np.array_equal(cnt.cpu().numpy(), ref_cnt)
    assert np.array_equal(terms.cpu().numpy(), ref_terms)
    assert np.array_equal(imps.cpu().numpy(), ref_imp)
    # the cases the grid is built to hold: a chunk without terms, and one with some but fewer than m
    assert ref_cnt.min() == 0 and (m == 1 or ((ref_cnt > 0) & (ref_cnt < m)).any())


def test_select_random_values_differ_only_at_half_integers(dev):
    from multimodal_rag_amd import _native

    pooled, bias, scale = random_select_case()
    n, V = pooled.shape
    assert V <= 256                       # every positive term is emitted at m = 256: the impacts themselves are compared
    cnt, terms, imps = (x.cpu().numpy() for x in _native.sparse_select(
        torch.from_numpy(pooled).to(dev), torch.from_numpy(bias).to(dev), scale, 256))
    got = np.zeros((n, V), np.int64)
    for c in range(n):
        got[c, terms[c, : cnt[c]]] = imps[c, : cnt[c]]
    ws = R.weights(pooled, bias, scale)
    ref = R.impacts(pooled, bias, scale)
    near = np.abs(ws - np.floor(ws) - 0.5) <= 2.0 ** -10
    diff = got != ref
    print(f"select random: {int(diff.sum())} of {diff.size} impacts differ, {int(near.sum())} lie near a half-integer")
    assert (np.abs(got - ref)[diff] == 1).all()
    assert not (diff & ~near).any()
    assert near.mean() <= 0.01


def test_select_rejects_bad_arguments(dev):
    from multimodal_rag_amd import _native

    pooled = torch.zeros((2, 40), dtype=torch.float32, device=dev)
    bias = torch.zeros(40, dtype=torch.float32, device=dev)
    for scale, m in ((64.0, 0), (64.0, 257), (0.0, 4), (-1.0, 4)):
        with pytest.raises(_native.MMRagNativeError):
            _native.sparse_select(pooled, bias, scale, m)


# ---- scoring ------------------------------------------------------------------------------------------------------------
V_SYN = 200


def unit_rows(n, d, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def make_index(dev, n, log, how="add"):
    """a VectorIndex of n rows carrying the forward log: `add` = vectors given with the rows in one add, `set` =
    rows first, then set_sparse, `two` = grown by two adds"""
    from multimodal_rag_amd.index import VectorIndex

    off, terms, imps = log
    idx = VectorIndex(64, dtype=torch.float32, device=dev)
    idx.enable_sparse(V_SYN)
    emb = unit_rows(n, 64, 5)
    metas = [{"g": i % 3} for i in range(n)]
    ids = [f"id{i}" for i in range(n)]
    if how == "set":
        idx.add(emb, metadatas=metas, ids=ids)
        idx.set_sparse(np.arange(n), off, terms, imps)
    elif how == "two":
        h = n // 3
        idx.add(emb[:h], metadatas=metas[:h], ids=ids[:h], sparse=(off[: h + 1], terms[: off[h]], imps[: off[h]]))
        idx.add(emb[h:], metadatas=metas[h:], ids=ids[h:], sparse=(off[h:] - off[h], terms[off[h]:], imps[off[h]:]))
    else:
        idx.add(emb, metadatas=metas, ids=ids, sparse=log)
    return idx


def syn_queries():
    """q0: the every-row term and two common ones; q1: the single-row term and the term without postings; q2: the 64
    terms of impact 255 (the largest sum); q3: the every-row term alone (one score for every row: ties everywhere)"""
    qs = [([0, 10, 11], [3, 200, 17]), ([1, 2], [255, 255]), (list(range(100, 164)), [255] * 64), ([0], [9])]
    off = np.concatenate([[0], np.cumsum([len(t) for t, _ in qs])]).astype(np.int64)
    return qs, (off, np.concatenate([t for t, _ in qs]).astype(np.int32),
                np.concatenate([w for _, w in qs]).astype(np.int32))


def check_topk(idx, log, packed, qs, k, allowed=None, where=None, **hook):
    s, r = idx.sparse_search(packed, k, where, **hook)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    for b, (t, w) in enumerate(qs):
        es, er = R.topk(R.scores(*log, V_SYN, t, w), k, allowed)
        assert np.array_equal(r[b], er), (b, k)
        assert np.array_equal(s[b], es), (b, k)
    return s, r


@pytest.fixture(scope="module")
def syn(dev):
    cache = {}

    def get(n, how="add"):
        if (n, how) not in cache:
            log = synthetic_log(n, V_SYN)
            cache[(n, how)] = (make_index(dev, n, log, how), log)
        return cache[(n, how)]
    return get


@pytest.mark.parametrize("n", [300, 2049, 4097])
def test_scoring_exact_at_block_seams(syn, n):
    idx, log = syn(n, "set")
    qs, packed = syn_queries()
    for k in (1, 5, 4096):
        s, r = check_topk(idx, log, packed, qs, k)
    assert (r[1] >= 0).sum() == 1 and r[1, 1] == -1 and np.isneginf(s[1, 1:]).all()      # one match, then padding
    assert (r[0] >= 0).sum() == min(n, 4096)                                              # term 0 is in every row
    assert s[2].max() == 255 * 255 * 64
    # alone against in the batch
    for b in range(len(qs)):
        off = np.asarray([0, len(qs[b][0])], np.int64)
        s1, r1 = idx.sparse_search((off, np.asarray(qs[b][0], np.int32), np.asarray(qs[b][1], np.int32)), 5)
        s5, r5 = idx.sparse_search(packed, 5)
        assert torch.equal(s1[0], s5[b]) and torch.equal(r1[0], r5[b])
    # the overflow re-run at small n: fewer slots than matches, through the kernel's test hook
    check_topk(idx, log, packed, qs, 5, cap=256)
    check_topk(idx, log, packed, qs, 300, cap=256)


def test_scoring_where_alive_compact_and_growth(syn, dev):
    n = 2049
    idx, log = syn(n, "two")
    same, _ = syn(n, "set")
    qs, packed = syn_queries()
    for k in (5, 4096):
        a = idx.sparse_search(packed, k)
        b = same.sparse_search(packed, k)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    g1 = np.arange(n) % 3 == 1
    check_topk(idx, log, packed, qs, 5, allowed=g1, where={"g": 1})
    gone = [0, 7, 2047, 2048] + list(range(40, 60))
    idx.delete(ids=[f"id{i}" for i in gone])
    live = np.ones(n, bool)
    live[gone] = False
    s, r = check_topk(idx, log, packed, qs, 50, allowed=live)
    check_topk(idx, log, packed, qs, 5, allowed=live & g1, where={"g": 1})
    idx.compact()
    new_of_old = np.cumsum(live) - 1
    s2, r2 = idx.sparse_search(packed, 50)
    r2 = r2.cpu().numpy()
    assert np.array_equal(s2.cpu().numpy(), s)
    assert np.array_equal(r2, np.where(r >= 0, new_of_old[np.maximum(r, 0)], -1))


def test_scoring_above_the_candidate_slots(syn):
    """n = 20 000 with every row matching q0 and q3: bound stages, and for q3 (one score for all rows) more survivors
    than slots -- the overflow re-run -- without any hook; then the hook's regimes"""
    from multimodal_rag_amd import _native

    n = 20_000
    assert n > _native.candidate_capacity(5)
    idx, log = syn(n)
    qs, packed = syn_queries()
    for k in (1, 5, 4096):
        check_topk(idx, log, packed, qs, k)
    check_topk(idx, log, packed, qs, 5, dbg=1)               # no bound stages
    check_topk(idx, log, packed, qs, 5, cap=256)             # stages, then overflow and re-run
    check_topk(idx, log, packed, qs, 5, cap=256, dbg=1)


def test_scoring_rejects_bad_queries(syn):
    idx, _ = syn(300, "set")
    one = np.asarray([0, 1], np.int64)
    with pytest.raises(ValueError):
        idx.sparse_search((one, np.asarray([V_SYN], np.int32), np.asarray([1], np.int32)), 5)
    with pytest.raises(ValueError):
        idx.sparse_search((one, np.asarray([3], np.int32), np.asarray([256], np.int32)), 5)
    with pytest.raises(ValueError):
        idx.sparse_search((np.asarray([0, 65], np.int64), np.arange(65, dtype=np.int32), np.ones(65, np.int32)), 5)
    with pytest.raises(ValueError):
        idx.sparse_search((np.asarray([0, 2], np.int64), np.asarray([4, 4], np.int32), np.ones(2, np.int32)), 5)
    with pytest.raises(ValueError):
        idx.sparse_search((one, np.asarray([3], np.int32), np.asarray([1], np.int32)), 4097)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dev):
    from multimodal_rag_amd.encoder import EncoderConfig
    from multimodal_rag_amd.sparse import DeviceSparseEncoder

    L, H, heads, inter, V, max_pos = E2E_SHAPE
    cfg = EncoderConfig("tiny-mlm", L, H, heads, inter, V, max_pos, max_pos, "cls", 1e-12)
    w = e2e_weights()
    enc = DeviceSparseEncoder(cfg, w, dev, scale=64.0, skip_ids=list(range(5)))
    return enc, w


def test_expand_ids_matches_the_float64_forward(tiny):
    enc, w = tiny
    L, H, heads, inter, V, max_pos = E2E_SHAPE
    seqs = e2e_sequences()
    W = max(len(s) for s in seqs)
    ids = np.zeros((len(seqs), W), np.int32)
    for i, s in enumerate(seqs):
        ids[i, : len(s)] = s
    lens = np.asarray([len(s) for s in seqs], np.int32)
    pooled = R.expand(R.round_matrices_fp16(w), seqs, L, heads, 1e-12)
    ws = R.weights(pooled, w["cls.predictions.bias"], 64.0)
    ws[:, :5] = 0.0                                             # the skipped ids
    ref_imp = np.minimum(np.rint(ws), 255).astype(np.int64)
    checked = 0
    for m in (1, 2, 4, 8, 32, 256):
        off, terms, imps = enc.expand_ids(ids, lens, m)
        assert off[0] == 0 and off[-1] == terms.size == imps.size
        for i in range(len(seqs)):
            t, q = terms[off[i]: off[i + 1]], imps[off[i]: off[i + 1]]
            assert (np.diff(t) > 0).all() and t.size <= m and (q >= 1).all() and (t >= 5).all()
            assert (np.abs(q - ref_imp[i, t]) <= 1).all(), (m, i)
            order = np.sort(ws[i])[::-1]
            n_pos = int((ref_imp[i] >= 1).sum())
            if n_pos > m and order[m - 1] - order[m] > 1.0 and order[m - 1] >= 1.5:
                assert set(t.tolist()) == set(np.argsort(-ws[i], kind="stable")[:m].tolist()), (m, i)
                checked += 1
            elif n_pos <= m and (np.abs(ws[i] - 0.5) > 0.5)[ref_imp[i] <= 1].all():
                assert set(t.tolist()) == set(np.nonzero(ref_imp[i] >= 1)[0].tolist()), (m, i)
                checked += 1
            # never a term whose reference weight lies more than one unit under the cut
            if t.size and n_pos > m:
                assert ws[i, t].min() >= order[m - 1] - 1.0, (m, i)
    assert checked > 0


def test_index_path_hybrid_and_delete(tiny, dev):
    from multimodal_rag_amd.index import VectorIndex
    from multimodal_rag_amd.lexical import rrf_fuse
    from multimodal_rag_amd.config import settings

    enc, _ = tiny
    seqs = e2e_sequences()
    W = max(len(s) for s in seqs)
    ids = np.zeros((len(seqs), W), np.int32)
    for i, s in enumerate(seqs):
        ids[i, : len(s)] = s
    lens = np.asarray([len(s) for s in seqs], np.int32)
    d_log = enc.expand_ids(ids, lens, 128)
    q_log = enc.expand_ids(ids[:3], lens[:3], 32)
    n = len(seqs)
    emb = unit_rows(n, 64, 9)
    idx = VectorIndex(64, dtype=torch.float32, device=dev)
    idx.enable_sparse(enc.cfg.vocab)
    idx.add(emb, documents=[f"doc {i}" for i in range(n)], metadatas=[{"g": i % 2} for i in range(n)],
            ids=[f"id{i}" for i in range(n)], sparse=d_log)
    out = idx.sparse_query(q_log, 5)
    for b in range(3):
        sc = R.scores(*d_log, enc.cfg.vocab, q_log[1][q_log[0][b]: q_log[0][b + 1]], q_log[2][q_log[0][b]: q_log[0][b + 1]])
        es, er = R.topk(sc, 5)
        assert out["rows"][b] == [int(r) for r in er if r >= 0]
        assert out["ids"][b][0] == f"id{b}"                      # a text matches itself best
        assert np.allclose(out["sparse_scores"][b], es[: len(out['rows'][b])] / (64.0 * 64.0), rtol=0, atol=0)
        ex = idx.sparse_explain(q_log[1][q_log[0][b]: q_log[0][b + 1]], q_log[2][q_log[0][b]: q_log[0][b + 1]],
                                out["rows"][b][0])
        assert abs(sum(c for _, c in ex) - out["sparse_scores"][b][0]) < 1e-9
        assert [c for _, c in ex] == sorted((c for _, c in ex), reverse=True)
    # dense + sparse fused by rrf_fuse over the two legs' own lists
    C = min(max(4, settings.MMRAG_HYBRID_CANDIDATES), 4096)
    hy = idx.sparse_hybrid_query(emb[:3], q_log, 4)
    dense = idx.query(emb[:3], n_results=min(C, n))
    sp = idx.sparse_query(q_log, C)
    row_of = {f"id{i}": i for i in range(n)}
    for b in range(3):
        want = rrf_fuse([row_of[i] for i in dense["ids"][b]], sp["rows"][b], settings.MMRAG_HYBRID_RRF_K)[:4]
        assert hy["rows"][b] == [r for r, _ in want]
        assert hy["hybrid_scores"][b] == [s for _, s in want]
    # where, delete, then query
    odd = idx.sparse_query(q_log, 5, where={"g": 1})
    assert all(int(i[2:]) % 2 == 1 for row in odd["ids"] for i in row)
    idx.delete(ids=["id0"])
    after = idx.sparse_query(q_log, 5)
    assert all("id0" not in row for row in after["ids"])
    assert after["ids"][1][0] == "id1"


def _bodies():
    g = np.random.default_rng(41)
    return [" ".join(f"w{int(t)}" for t in g.integers(0, 590, 30)) + "." for _ in range(6)]


def test_embedding_manager_stores_and_queries(dev, tmp_path, monkeypatch):
    from multimodal_rag_amd import embedder as emb_mod
    from multimodal_rag_amd.lexical import rrf_fuse
    from tests.test_sparse_cpu import write_checkpoint

    write_checkpoint(str(tmp_path), tied=True)
    monkeypatch.setattr(emb_mod.settings, "MMRAG_SPARSE_ENCODER_DIR", str(tmp_path))
    m = emb_mod.EmbeddingManager(enable_cache=False)
    asyncio.run(m.initialize())
    assert m.has_sparse_encoder() and m.supports_sparse()
    bodies = _bodies()
    items = [{"id": f"t{i}", "type": "text", "summary": b} for i, b in enumerate(bodies)]
    asyncio.run(m.embed_and_store(items, "doc"))
    coll, enc = m.collection, m._get_sparse()
    assert coll.sparse_enabled and coll._sparse.n == 6 and coll._sparse.n_postings > 0
    # what was stored is the expansion of the summaries, at most MMRAG_SPARSE_DOC_TERMS terms each
    off, terms, imps = enc.expand_texts(bodies, 128)
    for r in range(6):
        t, q = coll._sparse.row_vector(r)
        assert np.array_equal(t, terms[off[r]: off[r + 1]]) and np.array_equal(q, imps[off[r]: off[r + 1]])
    before = m.stats["total_queries"]
    out = asyncio.run(m.sparse_query(bodies[2], n_results=3, explain=True))
    assert m.stats["total_queries"] == before + 1
    assert out["ids"][0] == "doc_t2" and out["sparse_scores"] == sorted(out["sparse_scores"], reverse=True)
    q = enc.expand_texts([bodies[2]], 32)
    sc = R.scores(off, terms, imps, enc.cfg.vocab, q[1], q[2])
    es, er = R.topk(sc, 3)
    assert out["ids"] == [f"doc_t{int(r)}" for r in er if r >= 0]
    assert out["sparse_scores"] == [float(s) / (enc.scale * enc.scale) for s in es[: len(out["ids"])]]
    top = out["matched_terms"][0]
    assert top and all(set(e) == {"term", "score"} for e in top)
    assert abs(sum(e["score"] for e in top) - out["sparse_scores"][0]) < 1e-9
    assert [e["score"] for e in top] == sorted((e["score"] for e in top), reverse=True)
    batch = asyncio.run(m.batch_sparse_query([bodies[2], " ", bodies[0]], n_results=3))
    assert batch[0]["ids"] == out["ids"] and "error" in batch[1] and batch[2]["ids"][0] == "doc_t0"
    # the word pieces of the question alone: no forward pass on the query path
    monkeypatch.setattr(emb_mod.settings, "MMRAG_SPARSE_QUERY_MODE", "tokens")
    tok = asyncio.run(m.sparse_query(bodies[2], n_results=3))
    qt = enc.token_terms([bodies[2]], 32)
    es, er = R.topk(R.scores(off, terms, imps, enc.cfg.vocab, qt[1], qt[2]), 3)
    assert tok["ids"] == [f"doc_t{int(r)}" for r in er if r >= 0]
    monkeypatch.setattr(emb_mod.settings, "MMRAG_SPARSE_QUERY_MODE", "expand")
    # dense + sparse: rrf_fuse over the two legs' own lists
    hy = asyncio.run(m.hybrid_query(bodies[1], n_results=4, leg="sparse"))
    dense = asyncio.run(m.query(bodies[1], n_results=6))
    sp = asyncio.run(m.sparse_query(bodies[1], n_results=6))
    num = lambda found: [int(i[len("doc_t"):]) for i in found]  # noqa: E731 (the row of "doc_t<row>")
    want = rrf_fuse(num(dense["ids"]), num(sp["ids"]), emb_mod.settings.MMRAG_HYBRID_RRF_K)[:4]
    assert num(hy["ids"]) == [r for r, _ in want] and hy["hybrid_scores"] == [s for _, s in want]
    assert set(hy) >= {"sparse_scores", "distances"}
    with pytest.raises(ValueError):
        asyncio.run(m.sparse_query("  "))
    # delete, then query; then a second document; then the state after enable_sparse() from scratch
    asyncio.run(m.embed_and_store([{"id": "x", "type": "text", "summary": bodies[2]}], "other"))
    asyncio.run(m.delete_document("doc"))
    after = asyncio.run(m.sparse_query(bodies[2], n_results=3))
    assert after["ids"] == ["other_x"]
    coll._sparse = None
    assert asyncio.run(m.enable_sparse())["items"] == 1
    assert asyncio.run(m.sparse_query(bodies[2], n_results=3))["ids"] == ["other_x"]
    asyncio.run(m.cleanup())


def test_query_endpoint_sparse_and_explain(dev, tmp_path, monkeypatch):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd import embedder as emb_mod
    from multimodal_rag_amd.server import create_app
    from tests.test_sparse_cpu import write_checkpoint

    write_checkpoint(str(tmp_path), tied=False)
    monkeypatch.setattr(emb_mod.settings, "MMRAG_SPARSE_ENCODER_DIR", str(tmp_path))
    bodies = _bodies()
    with TestClient(create_app()) as c:
        for i, body in enumerate(bodies[:3]):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
        plain = c.post("/query", json={"query": bodies[1], "top_k": 3})
        assert plain.status_code == 200 and all("sparse_score" not in s for s in plain.json()["sources"])
        r = c.post("/query", json={"query": bodies[1], "top_k": 3, "sparse": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert src and all("sparse_score" in s and "matched_terms" not in s for s in src)
        assert [s["sparse_score"] for s in src] == sorted((s["sparse_score"] for s in src), reverse=True)
        r = c.post("/query", json={"query": bodies[1], "top_k": 3, "sparse": True, "explain": True})
        assert r.status_code == 200, r.text
        ex = r.json()["sources"]
        assert [s["doc_id"] for s in ex] == [s["doc_id"] for s in src]
        for s in ex:
            assert s["matched_terms"] and all(isinstance(e["term"], str) and e["score"] > 0 for e in s["matched_terms"])
            assert abs(sum(e["score"] for e in s["matched_terms"]) - s["sparse_score"]) < 1e-9
        r = c.post("/query", json={"query": bodies[1], "top_k": 2, "hybrid": True, "hybrid_leg": "sparse"})
        assert r.status_code == 200, r.text
        assert all("hybrid_score" in s and "sparse_score" in s for s in r.json()["sources"])
