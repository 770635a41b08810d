"""GPU: maximal-marginal-relevance selection (csrc/mmr.hip through _native.mmr_select, VectorIndex, EmbeddingManager and
POST /query) against tests/mmr_ref.py: bit-exact on exactly representable data, within a derived bound on real-valued
data at every step, reproducible, and with the collection's semantics."""
import asyncio

import numpy as np
import pytest
import torch

from tests import mmr_ref as R

pytestmark = pytest.mark.gpu

TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


# ---------------------------------------------------------------- 1. exact data, strict equality
def int_corpus(n, d, dtype, dev, seed, distinct=None, pad_fill=0):
    """rows with entries -2..2 (exact in every storage dtype) in storage layout [n, ld]; `distinct`: that many
    different rows only (heavy ties); pad_fill: what the pad columns hold (the kernel must not read them)"""
    from multimodal_rag_amd import _native

    g = np.random.default_rng(seed)
    base = g.integers(-2, 3, (distinct or n, d))
    M = base[g.integers(0, len(base), n)] if distinct else base
    ld = _native.padded_dim(d, dtype)
    full = np.full((n, ld), pad_fill, np.float32)
    full[:, :d] = M
    return M, torch.from_numpy(full).to(device=dev, dtype=dtype).contiguous()


def int_candidates(M, B, C, seed, ragged=False):
    """the C best rows per query by (score descending, row ascending) for integer queries, as float32 / int64 [B, C]"""
    g = np.random.default_rng(seed)
    q = g.integers(-2, 3, (B, M.shape[1]))
    scores = q @ M.T
    rel = np.full((B, C), -np.inf, np.float32)
    rows = np.full((B, C), -1, np.int64)
    for b in range(B):
        order = np.lexsort((np.arange(M.shape[0]), -scores[b]))[:C]
        m = len(order)
        if ragged:
            m = int(g.integers(0, m + 1)) if b else m
        rel[b, :m] = scores[b, order[:m]]
        rows[b, :m] = order[:m]
    return rel, rows


def check_exact(dev, dtype, d, n, C, k, B, seed, ragged=False, distinct=None, pad_fill=0, lam=0.5):
    from multimodal_rag_amd import _native

    M, corpus = int_corpus(n, d, dtype, dev, seed, distinct, pad_fill)
    rel, rows = int_candidates(M, B, C, seed + 1, ragged)
    rel_t, rows_t = torch.from_numpy(rel).to(dev), torch.from_numpy(rows).to(dev)
    got = [t.cpu().numpy() for t in _native.mmr_select(corpus, d, rel_t, rows_t, k, lam)]
    streamed = [t.cpu().numpy() for t in _native.mmr_select(corpus, d, rel_t, rows_t, k, lam,
                                                            dbg=_native.MMR_DBG_STREAM)]
    for a, b in zip(got, streamed):                       # the two kernel forms: the same bits
        assert np.array_equal(a, b)
    for b in range(B):
        want = R.select_padded(rel[b], rows[b], M, k, lam)
        for name, g_, w_ in zip(("scores", "rows", "positions", "values"), got, want):
            assert g_[b].dtype == w_.dtype and np.array_equal(g_[b], w_), (name, b, g_[b][:8], w_[:8])


SHAPES = [(1, 1, 1), (2, 1, 3), (2, 2, 1), (21, 5, 64), (21, 21, 3), (50, 1, 3), (50, 5, 257), (50, 20, 64),
          (50, 50, 3), (64, 20, 257), (64, 64, 1), (333, 20, 3), (333, 333, 1), (1024, 5, 64), (1024, 20, 3),
          (1024, 1024, 1)]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("d", [64, 200])
def test_exact_integer_data_equals_reference(dev, dt, d):
    for at, (C, k, B) in enumerate(SHAPES):
        check_exact(dev, TORCH_DT[dt], d, max(C + 40, 300), C, k, B, seed=100 * d + at)


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
def test_exact_heavy_ties_ragged_and_tails(dev, dt):
    dtype = TORCH_DT[dt]
    # 12 different rows among 1500: most candidates are copies of one another with equal relevance
    for C, k, B in [(50, 20, 64), (333, 333, 3), (1024, 20, 3), (64, 64, 257)]:
        check_exact(dev, dtype, 64, 1500, C, k, B, seed=7 + C, distinct=12)
    # -1 tails of different lengths per query (query 0 full, the others 0 .. C candidates)
    check_exact(dev, dtype, 64, 400, 50, 20, 64, seed=11, ragged=True)
    check_exact(dev, dtype, 200, 1200, 1024, 20, 5, seed=12, ragged=True, distinct=40)
    # d that is no whole number of 16-byte chunks, pad columns full of 7s: they must not enter a dot product
    check_exact(dev, dtype, 70, 300, 50, 20, 3, seed=13, pad_fill=7)
    check_exact(dev, dtype, 3, 300, 21, 21, 3, seed=14, pad_fill=7)
    # rows longer than the streamed form's LDS copy of the picked row (read in place)
    check_exact(dev, dtype, 8200, 64, 21, 5, 3, seed=15)
    # lambda 1 and 0 are exact too
    check_exact(dev, dtype, 64, 300, 50, 20, 3, seed=16, lam=1.0)
    check_exact(dev, dtype, 64, 300, 50, 20, 3, seed=17, lam=0.0, distinct=30)


def test_native_argument_checks(dev):
    from multimodal_rag_amd import _native

    M, corpus = int_corpus(100, 64, torch.float16, dev, 0)
    rel, rows = int_candidates(M, 2, 10, 1)
    rel_t, rows_t = torch.from_numpy(rel).to(dev), torch.from_numpy(rows).to(dev)
    with pytest.raises(_native.MMRagNativeError):
        _native.mmr_select(corpus, 64, rel_t.cpu(), rows_t, 5, 0.5)            # host tensor
    with pytest.raises(_native.MMRagNativeError):
        _native.mmr_select(corpus, 64, rel_t, rows_t.int(), 5, 0.5)            # wrong dtype
    with pytest.raises(_native.MMRagNativeError):
        _native.mmr_select(corpus, 64, rel_t.t().contiguous().t(), rows_t, 5, 0.5)   # not contiguous
    with pytest.raises(_native.MMRagNativeError):
        _native.mmr_select(corpus, 64, rel_t, rows_t, 11, 0.5)                 # k > C
    with pytest.raises(_native.MMRagNativeError):
        _native.mmr_select(corpus, 64, rel_t, rows_t, 5, 1.01)


def test_select_is_graph_capturable(dev):
    from multimodal_rag_amd import _native

    M, corpus = int_corpus(400, 64, torch.float16, dev, 3)
    rel, rows = int_candidates(M, 8, 50, 4)
    rel_t, rows_t = torch.from_numpy(rel).to(dev), torch.from_numpy(rows).to(dev)
    eager = [t.clone() for t in _native.mmr_select(corpus, 64, rel_t, rows_t, 10, 0.5)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _native.mmr_select(corpus, 64, rel_t, rows_t, 10, 0.5)                 # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _native.mmr_select(corpus, 64, rel_t, rows_t, 10, 0.5)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 2. real-valued data, every step validated
def clustered_unit_rows(n, d, seed, centres=300, noise=0.25):
    g = np.random.default_rng(seed)
    c = g.standard_normal((centres, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[g.integers(0, centres, n)] + noise * g.standard_normal((n, d)) / np.sqrt(d)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def build_index(dev, rows, dtype=torch.float16, docs=None, metas=None):
    from multimodal_rag_amd.index import VectorIndex

    n, d = rows.shape
    idx = VectorIndex(dim=d, dtype=dtype, device=dev, capacity=n)
    idx.add(rows, documents=docs or [f"doc {i}" for i in range(n)], metadatas=metas,
            ids=[f"id{i}" for i in range(n)])
    return idx


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
@pytest.mark.parametrize("d", [384, 768])
def test_real_data_every_step_within_the_derived_bound(dev, dt, d):
    """At every step t of every query the GPU's pick must be, in float64 arithmetic on the stored (quantised) rows and
    queries and given the GPU's own prefix, within tol of the best free candidate.

    tol is derived, not measured: a float32 dot product of d products of two unit vectors is within d * 2^-24 of the
    exact one (gamma_d * sum |a_i b_i| with sum |a_i b_i| <= 1); v is a convex mix of two such values plus two
    multiplications and a subtraction (the + 4); two v are compared, so tol = 2 (d + 4) 2^-24: 4.6e-5 at d = 384,
    9.2e-5 at d = 768.  B = 24 <= 64 keeps float32 storage on the exact float32 matrix instruction.  No step is
    left out and there is no near-tie exclusion."""
    dtype = TORCH_DT[dt]
    n, B, k, fetch_k = 20_000, 24, 10, 64
    rows = clustered_unit_rows(n, d, seed=d)
    idx = build_index(dev, rows, dtype)
    g = np.random.default_rng(d + 1)
    rnd = g.standard_normal((B // 2, d))
    q = np.concatenate([rows[g.integers(0, n, B // 2)], rnd / np.linalg.norm(rnd, axis=1, keepdims=True)])
    q = q.astype(np.float32)
    tol = 2.0 * (d + 4) * 2.0 ** -24
    stored = idx.matrix[:n, :d].double().cpu().numpy()
    q_stored = torch.from_numpy(q).to(dtype).double().numpy()                  # the queries as the kernels read them
    s_all, r_all = (t.cpu().numpy() for t in idx.search(q, fetch_k))
    worst, steps = 0.0, 0
    for lam in (0.3, 0.5, 0.7):
        out_s, out_r, out_p, out_v = (t.cpu().numpy() for t in idx.mmr_search(q, k, fetch_k=fetch_k, lambda_mult=lam))
        for b in range(B):
            cand = r_all[b]
            assert (cand >= 0).all() and (out_p[b] >= 0).all()
            # rel is the search's own score of that row, bit for bit, and the row is the candidate at that position
            assert np.array_equal(out_s[b], s_all[b][out_p[b]]) and np.array_equal(out_r[b], cand[out_p[b]])
            assert len(set(out_p[b].tolist())) == k and out_p[b][0] == 0 and out_v[b][0] == s_all[b][0]
            X = stored[cand]
            rel64 = X @ q_stored[b]
            for t in range(1, k):
                v, free = R.step_values(rel64, X, out_p[b][:t], lam)
                pick = int(out_p[b][t])
                assert free[pick]
                gap = float(v[free].max() - v[pick])
                worst = max(worst, gap)
                steps += 1
                assert gap <= tol, (lam, b, t, gap, tol)
                assert abs(float(out_v[b][t]) - v[pick]) <= tol, (lam, b, t, float(out_v[b][t]), v[pick])
    print(f"mmr path validation d={d} {dt}: {steps} steps, worst float64 gap {worst:.3e}, tol {tol:.3e}")
    assert steps == 3 * B * (k - 1)


# ---------------------------------------------------------------- 3. reproducibility
def ids_of(idx, rows):
    return [[idx._ids[r] if r >= 0 else None for r in row] for row in rows.tolist()]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
def test_reproducible_alone_in_a_batch_run_to_run_and_after_compact(dev, dt):
    d, n = 384, 6000
    rows = clustered_unit_rows(n, d, seed=5, centres=60)
    idx = build_index(dev, rows, TORCH_DT[dt])
    # float32 collections score batches above 64 queries on the bf16-split path unless MMRAG_F32_EXACT_SEARCH routes
    # them 64 at a time; the candidates' scores are batch-independent only with that routing
    idx.f32_exact = True
    q = clustered_unit_rows(256, d, seed=6, centres=60)
    batch = [t.cpu() for t in idx.mmr_search(q, 10, fetch_k=50, lambda_mult=0.5)]
    again = [t.cpu() for t in idx.mmr_search(q, 10, fetch_k=50, lambda_mult=0.5)]
    for a, b in zip(batch, again):
        assert torch.equal(a, b)
    for at in (0, 17, 255):
        alone = [t.cpu() for t in idx.mmr_search(q[at:at + 1], 10, fetch_k=50, lambda_mult=0.5)]
        for a, b in zip(alone, batch):
            assert torch.equal(a[0], b[at]), at
    # tombstones, then the same collection compacted: the same ids, scores and values
    idx.delete(ids=[f"id{i}" for i in range(0, n, 3)])
    before = [t.cpu() for t in idx.mmr_search(q[:32], 10, fetch_k=50, lambda_mult=0.5)]
    ids_before = ids_of(idx, before[1])
    idx.compact()
    assert idx.rows_in_use == idx.count()
    after = [t.cpu() for t in idx.mmr_search(q[:32], 10, fetch_k=50, lambda_mult=0.5)]
    assert ids_of(idx, after[1]) == ids_before
    for j in (0, 2, 3):
        assert torch.equal(before[j], after[j])


# ---------------------------------------------------------------- 4. semantics through VectorIndex
def test_deleted_and_filtered_rows_never_appear(dev):
    d, n = 64, 3000
    rows = clustered_unit_rows(n, d, seed=21, centres=40)
    metas = [{"kind": "a" if i % 3 else "b", "i": i} for i in range(n)]
    idx = build_index(dev, rows, metas=metas)
    q = clustered_unit_rows(9, d, seed=22, centres=40)
    gone = {f"id{i}" for i in range(0, n, 2)}
    idx.delete(ids=sorted(gone))
    res = idx.mmr_query(q, n_results=15, fetch_k=100, lambda_mult=0.4)
    assert all(len(x) == 15 for x in res["ids"]) and not gone & {i for x in res["ids"] for i in x}
    res = idx.mmr_query(q, n_results=15, fetch_k=100, lambda_mult=0.4, where={"kind": "b"})
    assert all(m["kind"] == "b" for x in res["metadatas"] for m in x)
    assert not gone & {i for x in res["ids"] for i in x} and all(len(x) == 15 for x in res["ids"])
    assert set(res) >= {"ids", "distances", "metadatas", "documents", "mmr_scores"}
    assert all(len(v) == 15 for v in res["mmr_scores"])


def test_fetch_k_beyond_the_live_count_n_results_one_and_limits(dev):
    from multimodal_rag_amd import _native

    d = 64
    rows = clustered_unit_rows(30, d, seed=31, centres=5)
    idx = build_index(dev, rows)
    q = clustered_unit_rows(4, d, seed=32, centres=5)
    res = idx.mmr_query(q, n_results=40, fetch_k=500, lambda_mult=0.5)           # 30 live rows
    assert all(len(x) == 30 and len(set(x)) == 30 for x in res["ids"])
    assert all(len(v) == 30 for v in res["mmr_scores"]) and all(len(v) == 30 for v in res["distances"])
    s, r, p, v = idx.mmr_search(q, 40, fetch_k=500)
    assert (r[:, 30:] == -1).all() and (p[:, 30:] == -1).all() and torch.isneginf(s[:, 30:]).all() \
        and torch.isneginf(v[:, 30:]).all()
    one = idx.mmr_query(q, n_results=1)
    assert [x[0] for x in one["ids"]] == [x[0] for x in idx.query(q, n_results=1)["ids"]]
    assert np.allclose([m[0] for m in one["mmr_scores"]], [1.0 - dist[0] for dist in one["distances"]], atol=1e-6)
    with pytest.raises(ValueError):
        idx.mmr_query(q, n_results=_native.MAX_MMR_CANDIDATES + 1)
    with pytest.raises(ValueError):
        idx.mmr_query(q, n_results=0)
    with pytest.raises(ValueError):
        idx.mmr_query(q, n_results=3, lambda_mult=1.2)
    idx.reset()
    assert idx.mmr_query(q, n_results=3)["ids"] == [[] for _ in range(4)]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32"])
def test_lambda_one_equals_query(dev, dt):
    d, n = 100, 5000
    rows = clustered_unit_rows(n, d, seed=41, centres=50)
    idx = build_index(dev, rows, TORCH_DT[dt])
    q = clustered_unit_rows(33, d, seed=42, centres=50)
    for n_results in (5, 20, 37):
        plain = idx.query(q, n_results=n_results)
        mmr = idx.mmr_query(q, n_results=n_results, fetch_k=n_results, lambda_mult=1.0)
        assert mmr["ids"] == plain["ids"] and mmr["distances"] == plain["distances"]
        assert mmr["documents"] == plain["documents"] and mmr["metadatas"] == plain["metadatas"]


def test_triplicated_corpus_returns_distinct_originals(dev):
    # originals: random unit vectors (mutual |cos| well under 0.4 at d = 128), each stored three times; a query is the
    # mean of 16 originals, so each of them has cos about 1/4 and their 48 copies are the dense top.  At lambda 0.5 a
    # copy of a picked row has v = (rel - 1) / 2 < -0.3 while an unpicked original has v > (rel - 0.4) / 2 > -0.2
    d, n = 128, 2000
    g = np.random.default_rng(51)
    base = g.standard_normal((n, d))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    rows = np.repeat(base, 3, axis=0).astype(np.float32)
    idx = build_index(dev, rows, docs=[f"orig {i // 3}" for i in range(3 * n)])
    q = np.stack([base[g.choice(n, 16, replace=False)].sum(axis=0) for _ in range(5)])
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    n_results = 10
    plain = idx.query(q, n_results=n_results)
    assert all(len(set(docs)) <= 4 for docs in plain["documents"])               # triplicates fill the list
    res = idx.mmr_query(q, n_results=n_results, fetch_k=50, lambda_mult=0.5)
    for docs, plain_docs in zip(res["documents"], plain["documents"]):
        assert len(docs) == n_results and len(set(docs)) == n_results
        assert docs[0] == plain_docs[0]


# ---------------------------------------------------------------- 5. end to end
def test_through_embedding_manager(dev):
    from multimodal_rag_amd.embedder import EmbeddingManager

    m = EmbeddingManager()
    asyncio.run(m.initialize())
    assert m.supports_mmr()
    words = ["học", "máy", "dữ", "liệu", "gpu", "kernel", "bảng", "ảnh", "văn", "bản", "mô", "hình"]
    g = np.random.default_rng(61)
    docs = [" ".join(g.choice(words, int(g.integers(3, 9)))) for _ in range(300)]
    docs += docs[:100]                                                           # the same texts uploaded twice
    items = [{"id": f"t{i}", "type": "text", "summary": t} for i, t in enumerate(docs)]
    asyncio.run(m.embed_and_store(items, "doc"))
    queries = ["học máy dữ liệu", "gpu kernel", "bảng và ảnh"]
    before = m.stats["total_queries"]
    out = asyncio.run(m.mmr_query(queries[0], n_results=7, fetch_k=40, lambda_mult=0.6))
    assert m.stats["total_queries"] == before + 1
    assert set(out) == {"ids", "distances", "metadatas", "documents", "mmr_scores"} and len(out["ids"]) == 7
    vec = np.asarray(asyncio.run(m.embed_texts_batch(queries)), np.float32)
    res = m.collection.mmr_query(vec, n_results=7, fetch_k=40, lambda_mult=0.6)
    assert out["ids"] == res["ids"][0] and out["mmr_scores"] == res["mmr_scores"][0]
    assert out["distances"] == res["distances"][0]
    many = asyncio.run(m.batch_mmr_query(queries + [" "], n_results=7, fetch_k=40, lambda_mult=0.6))
    assert m.stats["total_queries"] == before + 1 + 3
    for b in range(3):
        assert many[b]["ids"] == res["ids"][b] and many[b]["mmr_scores"] == res["mmr_scores"][b]
    assert many[3]["error"] == "Query text cannot be empty" and many[3]["ids"] == []
    with pytest.raises(ValueError):
        asyncio.run(m.mmr_query("  "))
    asyncio.run(m.cleanup())


def test_query_endpoint_mmr_and_rerank(dev, tmp_path, monkeypatch):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd import embedder as emb_mod
    from multimodal_rag_amd.server import create_app
    from tests.test_cross_encoder_gpu import _write_checkpoint

    words = ["học", "máy", "dữ", "liệu", "machine", "learning", "gpu"]
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + [f"w{i}" for i in range(1000 - 5 - len(words))]
    _write_checkpoint(str(tmp_path), "tiny", vocab)
    with TestClient(create_app()) as c:
        bodies = ["Học máy là gì? " * 3, "GPU kernel và dữ liệu. " * 3, "Machine learning cơ bản. " * 3,
                  "Học máy là gì? " * 3]
        for i, body in enumerate(bodies):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
        plain = c.post("/query", json={"query": "học máy", "top_k": 3})
        assert plain.status_code == 200 and all("mmr_score" not in s for s in plain.json()["sources"])
        r = c.post("/query", json={"query": "học máy", "top_k": 3, "mmr": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert len(src) == 3 and all("mmr_score" in s for s in src)
        assert src[0]["doc_id"] == plain.json()["sources"][0]["doc_id"]
        r = c.post("/query", json={"query": "học máy", "top_k": 3, "mmr": True, "mmr_lambda": 1.0})
        assert [s["doc_id"] for s in r.json()["sources"]] == [s["doc_id"] for s in plain.json()["sources"]]
        assert c.post("/query", json={"query": "học máy", "top_k": 3, "mmr": True, "hybrid": True}).status_code == 400
        monkeypatch.setattr(emb_mod.settings, "MMRAG_RERANKER_DIR", str(tmp_path))
        r = c.post("/query", json={"query": "học máy", "top_k": 2, "mmr": True, "rerank": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert src and all("mmr_score" in s and "rerank_score" in s for s in src)
