"""GPU: the BM25 lexical leg (csrc/lexical.hip through lexical.LexicalIndex and VectorIndex) against tests/bm25_ref.py,
its bit-reproducibility, its upkeep under adds / deletes / compaction / reset / save-load, and hybrid retrieval."""
import asyncio
import os

import numpy as np
import pytest
import torch

from tests import bm25_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return "cuda:0"


def zipf_corpus(n, vocab=200_000, tokens=150, seed=0):
    """synthetic Zipf corpus as term-id arrays (s = 1.1); term 0 is in every row, term vocab-1 in none"""
    g = np.random.default_rng(seed)
    lens = g.integers(tokens // 2, tokens * 3 // 2, n)
    tok = (g.zipf(1.1, int(lens.sum())) - 1) % (vocab - 2) + 1
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    key = np.concatenate([row * vocab + tok, np.arange(n, dtype=np.int64) * vocab])   # + term 0 once per row
    uk, cnt = np.unique(key, return_counts=True)
    rows, ids = uk // vocab, (uk % vocab).astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=off[1:])
    return off, ids, cnt.astype(np.int32), (lens + 1).astype(np.int32)


@pytest.fixture(scope="module")
def zipf(dev):
    from multimodal_rag_amd.lexical import LexicalIndex

    off, ids, tfs, dl = zipf_corpus(200_000)
    lex = LexicalIndex(dev)
    lex.append_postings(off, ids, tfs, dl)
    lex._max_term = 199_999   # the vocabulary (term 199999 is in no row)
    return lex, R.RefIndex(off, ids, tfs, dl)


def zipf_queries(B, seed):
    g = np.random.default_rng(seed)
    qs = []
    for i in range(B):
        qs.append(list(dict.fromkeys(((g.zipf(1.1, int(g.integers(1, 6))) - 1) % 199_998 + 1).tolist())))
    qs[0] = [0] + qs[0]                     # the every-row term
    if B > 2:
        qs[1] = [199_999]                   # no row holds it
        qs[2] = []                          # only unknown terms
    return qs


def pack(qs):
    off = np.zeros(len(qs) + 1, np.int32)
    np.cumsum([len(q) for q in qs], out=off[1:])
    return off, np.asarray([t for q in qs for t in q], np.int32)


@pytest.mark.parametrize("B", [1, 7, 64, 256])
def test_zipf_matches_reference(zipf, B):
    lex, ref = zipf
    qs = zipf_queries(B, seed=B)
    off, terms = pack(qs)
    live = np.ones(ref.n, bool)
    refs = [ref.scores(q, live) for q in qs]
    for k in (1, 5, 20, 21, 4096):
        s, r = lex.topk_ids(off, terms, k)
        s, r = s.cpu().numpy(), r.cpu().numpy()
        for b in range(B):
            R.assert_topk(s[b], r[b], *refs[b], live, k)
    if B >= 7:   # the every-row term's top-4096 went through the overflow re-run; the no-match queries are empty
        assert (r[1] == -1).all() and (r[2] == -1).all()


def test_zipf_bit_identical_alone_vs_batch_and_repeated(zipf):
    lex, _ = zipf
    qs = zipf_queries(64, seed=99)
    off, terms = pack(qs)
    s_all, r_all = lex.topk_ids(off, terms, 21)
    s2, r2 = lex.topk_ids(off, terms, 21)
    assert torch.equal(s_all, s2) and torch.equal(r_all, r2)
    for b in (0, 5, 63):
        o, t = pack([qs[b]])
        s1, r1 = lex.topk_ids(o, t, 21)
        assert torch.equal(s1[0], s_all[b]) and torch.equal(r1[0], r_all[b])


def test_csr_matches_forward_log(zipf):
    lex, ref = zipf
    term_off, post_row, post_tf = lex._ensure_csr()
    to = term_off.cpu().numpy()
    pr, pt = post_row.cpu().numpy(), post_tf.cpu().numpy()
    np.testing.assert_array_equal(np.diff(to)[: 199_999], np.bincount(ref.ids, minlength=200_000)[: 199_999])
    assert to[-1] == ref.ids.size
    np.testing.assert_array_equal(pr, ref.p_rows)    # stable by term: rows ascending within each term
    np.testing.assert_array_equal(pt, ref.p_tf)


# ---------------------------------------------------------------- text collections through VectorIndex
WORDS = None


def vi_words():
    global WORDS
    if WORDS is None:
        text = open(os.path.join(GOLDEN, "sample_document.txt"), encoding="utf-8").read()
        WORDS = sorted(set(R.analyze(text)))
    return WORDS


def text_docs(n, seed):
    import unicodedata

    g = np.random.default_rng(seed)
    w = vi_words()
    docs = []
    for i in range(n):
        ws = [w[j] for j in np.minimum(g.zipf(1.3, int(g.integers(3, 40))) - 1, len(w) - 1)]
        t = " ".join(ws)
        docs.append(unicodedata.normalize("NFC", t).capitalize() + ("." if i % 3 else ", C++ và Python!"))
    if n > 3:
        docs[3] = None
    return docs


QUERIES = ["học máy", "Machine Learning", "HỌC", "dữ liệu không có nhãn", "C++", "python học máy dữ liệu",
           "không", "zzzz qqqq", "trí tuệ nhân tạo", "Y tế: chẩn đoán bệnh"]


def unit_rows(n, d, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def make_index(dev, n, seed=0, dtype=torch.float32):
    from multimodal_rag_amd.index import VectorIndex

    docs = text_docs(n, seed)
    idx = VectorIndex(64, dtype=dtype, device=dev)
    idx.add(unit_rows(n, 64, seed), documents=docs, metadatas=[{"g": i % 3} for i in range(n)],
            ids=[f"id{i}" for i in range(n)])
    return idx, docs


def ref_for(docs, live):
    ref = R.RefIndex.from_texts(docs)
    return ref, np.asarray(live, bool)


def check_lexical(idx, docs, live, where_mask=None, k=20):
    ref, live = ref_for(docs, live)
    allowed = live if where_mask is None else live & where_mask
    where = None if where_mask is None else {"g": 1}
    res = idx.lexical_query(QUERIES, n_results=k, where=where)
    for b, q in enumerate(QUERIES):
        acc, matched = ref.scores(ref.query_ids(q), live)
        want = R.topk(acc, matched, allowed, k)
        rows = [int(i[2:]) for i in res["ids"][b]]
        got_s = np.full(k, -np.inf, np.float32)
        got_r = np.full(k, -1, np.int64)
        got_s[: len(rows)] = res["lexical_scores"][b]
        got_r[: len(rows)] = rows
        R.assert_topk(got_s, got_r, acc, matched, allowed, k)
        assert res["documents"][b] == [docs[r] for r in rows]
        assert len(rows) == want.size
    return res


def test_text_collection_and_lazy_build(dev):
    idx, docs = make_index(dev, 3000)
    assert idx._lex is None            # nothing lexical happened on add
    res = check_lexical(idx, docs, np.ones(3000, bool))
    assert res["ids"][QUERIES.index("zzzz qqqq")] == []
    check_lexical(idx, docs, np.ones(3000, bool), where_mask=np.arange(3000) % 3 == 1)
    for k in (1, 5, 4096):
        check_lexical(idx, docs, np.ones(3000, bool), k=k)


def test_bit_identical_across_build_paths(dev, tmp_path):
    from multimodal_rag_amd.persistence import load_index, save_index

    n = 4000
    docs = text_docs(n, 7)
    vecs = unit_rows(n, 64, 7)
    ids = [f"id{i}" for i in range(n)]
    once, _ = make_index(dev, 1, 7)
    once.reset()
    once.add(vecs, documents=docs, ids=ids)
    base = once.lexical_query(QUERIES, n_results=50)
    grown = make_index(dev, 1, 7)[0]
    grown.reset()
    grown.add(vecs[:1000], documents=docs[:1000], ids=ids[:1000])
    grown.lexical_query(QUERIES[:2], n_results=5)                    # enabled, then grown by adds
    for lo in range(1000, n, 700):
        grown.add(vecs[lo:lo + 700], documents=docs[lo:lo + 700], ids=ids[lo:lo + 700])
    assert grown.lexical_query(QUERIES, n_results=50) == base
    # alone vs in the batch
    for b in (0, 4, 9):
        one = once.lexical_query([QUERIES[b]], n_results=50)
        assert one["ids"][0] == base["ids"][b] and one["lexical_scores"][0] == base["lexical_scores"][b]
    # deletes, then compaction: the same statistics over the same live rows give the same bits
    gone = [f"id{i}" for i in range(0, n, 5)]
    once.delete(ids=gone)
    after_delete = once.lexical_query(QUERIES, n_results=50)
    once.compact()
    assert once._lex.n == n - len(gone)
    assert once.lexical_query(QUERIES, n_results=50) == after_delete
    save_index(once, str(tmp_path / "ix"))
    loaded = load_index(str(tmp_path / "ix"), device=dev)
    assert loaded._lex is None
    assert loaded.lexical_query(QUERIES, n_results=50) == after_delete


def test_deletes_where_and_reset_follow_reference(dev):
    idx, docs = make_index(dev, 2500, seed=3)
    idx.enable_lexical()
    dead = np.zeros(2500, bool)
    g = np.random.default_rng(1)
    victims = g.choice(2500, 600, replace=False)
    idx.delete(ids=[f"id{i}" for i in victims])
    dead[victims] = True
    df = idx._lex.df_host()
    ref, live = ref_for(docs, ~dead)
    want_df = np.zeros(len(ref.vocab), np.int64)
    np.add.at(want_df, ref.ids[np.repeat(live, np.diff(ref.off))], 1)
    np.testing.assert_array_equal(np.sort(df), np.sort(want_df))
    check_lexical(idx, docs, ~dead)
    check_lexical(idx, docs, ~dead, where_mask=np.arange(2500) % 3 == 1)
    idx.reset()
    assert idx.lexical_query(QUERIES, n_results=5)["ids"] == [[] for _ in QUERIES]
    idx.add(unit_rows(3, 64, 9), documents=["học máy", "máy", None], ids=["a", "b", "c"])
    assert idx.lexical_query(["học máy"], n_results=5)["ids"] == [["a", "b"]]


# ---------------------------------------------------------------- hybrid
def check_hybrid(idx, qvec, texts, docs, live, n_results, res):
    from multimodal_rag_amd.config import settings

    C = max(n_results, settings.MMRAG_HYBRID_CANDIDATES)
    dense = idx.query(qvec, n_results=C)
    ref, live = ref_for(docs, live)
    M = idx.matrix[: idx.rows_in_use, : idx.dim].double().cpu().numpy()
    for b, t in enumerate(texts):
        acc, matched = ref.scores(ref.query_ids(t), live)
        lex_rows = R.topk(acc, matched, live, C).tolist()
        d_rows = [idx._row_of[i] for i in dense["ids"][b]]
        want = R.rrf(d_rows, lex_rows, settings.MMRAG_HYBRID_RRF_K)[:n_results]
        got = [idx._row_of[i] for i in res["ids"][b]]
        assert got == [r for r, _ in want]
        assert res["hybrid_scores"][b] == [s for _, s in want]
        q = torch.as_tensor(np.asarray(qvec[b], np.float32)).to(idx.dtype).double().numpy()   # as the kernels read it
        cos = M[got] @ q
        np.testing.assert_allclose(res["distances"][b], 1.0 - cos, rtol=0, atol=1e-6)
        for r, d in zip(got, res["distances"][b]):
            if r in d_rows:
                assert d == dense["distances"][b][d_rows.index(r)]
        for r, s in zip(got, res["lexical_scores"][b]):
            assert (s > 0) == (r in lex_rows)


def test_hybrid_query_vector_index(dev):
    idx, docs = make_index(dev, 3000, seed=11)
    qv = unit_rows(len(QUERIES), 64, 12)
    for n_results in (5, 60):
        res = idx.hybrid_query(qv, QUERIES, n_results=n_results)
        check_hybrid(idx, qv, QUERIES, docs, np.ones(3000, bool), n_results, res)
        assert any(r not in set(idx.query(qv, n_results=50)["ids"][b]) for b in range(len(QUERIES))
                   for r in res["ids"][b])        # some rows come from the lexical leg alone


def test_hybrid_through_embedding_manager(dev):
    from multimodal_rag_amd.embedder import EmbeddingManager

    m = EmbeddingManager()
    asyncio.run(m.initialize())
    docs = text_docs(400, 21)
    docs[3] = "placeholder"
    items = [{"id": f"t{i}", "type": "text", "summary": d} for i, d in enumerate(docs)]
    asyncio.run(m.embed_and_store(items, "doc"))
    q = "học máy dữ liệu"
    before = m.stats["total_queries"]
    out = asyncio.run(m.hybrid_query(q, n_results=7))
    assert m.stats["total_queries"] == before + 1
    vec = np.asarray(asyncio.run(m.embed_texts_batch([q])), np.float32)
    coll = m.collection
    res = coll.hybrid_query(vec, [q], n_results=7)
    assert out["ids"] == res["ids"][0] and out["hybrid_scores"] == res["hybrid_scores"][0]
    check_hybrid(coll, vec, [q], docs, np.ones(400, bool), 7, res)
    with pytest.raises(ValueError):
        asyncio.run(m.hybrid_query("  "))
    asyncio.run(m.cleanup())


def test_query_endpoint_hybrid_and_rerank(dev, tmp_path, monkeypatch):
    from fastapi.testclient import TestClient

    from multimodal_rag_amd import embedder as emb_mod
    from multimodal_rag_amd.server import create_app
    from tests.test_cross_encoder_gpu import _write_checkpoint

    words = ["học", "máy", "dữ", "liệu", "machine", "learning", "gpu"]
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + [f"w{i}" for i in range(1000 - 5 - len(words))]
    _write_checkpoint(str(tmp_path), "tiny", vocab)
    with TestClient(create_app()) as c:
        for i, body in enumerate(["Học máy là gì? " * 3, "GPU kernel và dữ liệu. " * 3, "Machine learning cơ bản. " * 3]):
            r = c.post("/upload", files={"file": (f"d{i}.txt", body.encode(), "text/plain")})
            assert r.status_code == 200, r.text
        plain = c.post("/query", json={"query": "học máy", "top_k": 3})
        assert plain.status_code == 200 and all("hybrid_score" not in s for s in plain.json()["sources"])
        r = c.post("/query", json={"query": "học máy", "top_k": 3, "hybrid": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert src and all("hybrid_score" in s for s in src)
        monkeypatch.setattr(emb_mod.settings, "MMRAG_RERANKER_DIR", str(tmp_path))
        r = c.post("/query", json={"query": "học máy", "top_k": 2, "hybrid": True, "rerank": True})
        assert r.status_code == 200, r.text
        src = r.json()["sources"]
        assert src and all("hybrid_score" in s and "rerank_score" in s for s in src)
