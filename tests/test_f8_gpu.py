"""GPU: FP8 (E4M3) collections -- quantiser, the FP8 scan (lists and deep), exact re-scoring, the index on top.

References are tests/f8_ref.py (numpy float64).  Bounds: a float32 sum of d exact products in any order stays within
(d - 1) * 2^-24 * sum|q_i c_i| of the exact value; the factor 2 covers an adder tree that truncates."""
import os

import numpy as np
import pytest
import torch

import f8_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _native():
    from multimodal_rag_amd import _native

    return _native


def _quantise(x: np.ndarray, d: int, poison: bool = False) -> torch.Tensor:
    nat = _native()
    ld = nat.padded_dim(d, torch.float8_e4m3fn)
    out = torch.full((x.shape[0], ld), 0xAB if poison else 0, dtype=torch.uint8, device=DEV)
    out = out.view(torch.float8_e4m3fn)          # the storage dtype the library knows; uint8 is not one
    nat.append_rows(out, 0, torch.from_numpy(x).to(DEV), d)
    return out


def _codes_to_dev(codes: np.ndarray) -> torch.Tensor:
    n, d = codes.shape
    ld = (d + 127) // 128 * 128
    full = np.zeros((n, ld), np.uint8)
    full[:, :d] = codes
    return torch.from_numpy(full).to(DEV).view(torch.float8_e4m3fn)


@pytest.mark.parametrize("d", [3, 70, 768])
def test_quantiser_matches_reference(d):
    nat = _native()
    x = np.concatenate([f8_ref.sweep(), f8_ref.saturating()])
    m = (x.size + d - 1) // d
    x = np.resize(x, m * d).reshape(m, d)
    got = _quantise(x, d, poison=True)
    codes = got.view(torch.uint8).cpu().numpy()
    assert np.array_equal(codes[:, :d], f8_ref.encode(x))
    assert not codes[:, d:].any()                                  # poisoned pad columns come out 0x00
    rows = torch.arange(m - 1, -1, -1, device=DEV)
    back = nat.fetch_rows_f32(got, rows, d).cpu().numpy()
    want = (f8_ref.decode(codes[::-1, :d]) / 256.0).astype(np.float32)
    assert np.array_equal(back, want)
    dst = torch.zeros_like(got.view(torch.uint8)).view(torch.float8_e4m3fn)
    nat.gather_rows(dst, got, rows)
    assert torch.equal(dst.view(torch.uint8), got.view(torch.uint8).flip(0))
    with pytest.raises(KeyError):                   # a plain byte tensor is not taken for an FP8 matrix
        nat.fetch_rows_f32(got.view(torch.uint8), rows, d)


def _exact_case(B, n, d, seed, ties):
    rng = np.random.default_rng(seed)
    ints = np.array([-2, -1, 0, 1, 2])
    code_of = f8_ref.encode_scaled(ints.astype(np.float64))
    hi = 2 if ties else 5
    c = rng.integers(0, hi, (n, d))
    q = rng.integers(0, 5, (B, d))
    # asymmetric: the query is heavy where the corpus is light, per column position
    q[:, ::3] = 4
    c[:, 1::3] = rng.integers(3, 5, (n, (d - 2) // 3 + 1))[:, : c[:, 1::3].shape[1]]
    return code_of[q], code_of[c]


@pytest.mark.parametrize("B,n,d", [(1, 1000, 768), (7, 777, 100), (64, 5000, 384), (65, 300, 130), (128, 4099, 768),
                                   (129, 2000, 70), (256, 9000, 256), (257, 513, 768), (600, 1500, 128), (3, 3, 128)])
def test_exact_data_lists_bit_for_bit(B, n, d):
    nat = _native()
    qc, cc = _exact_case(B, n, d, B * 7 + n, ties=(B % 2 == 1))
    alive = None
    bits = None
    if n % 2 == 1:
        alive = np.random.default_rng(n).random(n) < 0.7
        words = np.packbits(np.concatenate([alive, np.zeros((-n) % 32 + 256, bool)]), bitorder="little").view(np.int32)
        bits = torch.from_numpy(words.copy()).to(DEV)
    ref = f8_ref.scores(qc, cc)
    q, c = _codes_to_dev(qc), _codes_to_dev(cc)
    for k in (1, 5, 10, 20):
        s, r = nat.cosine_topk(q, c, n, d, k, alive_bits=bits)
        rr, rs = f8_ref.topk(ref, k, alive)
        assert np.array_equal(r.cpu().numpy(), rr), (B, n, d, k)
        assert np.array_equal(s.cpu().numpy().astype(np.float64), rs), (B, n, d, k)


@pytest.mark.parametrize("B,n,d,k", [(1, 5000, 768, 21), (7, 3000, 100, 100), (64, 40000, 128, 1000),
                                      (129, 5000, 384, 4096), (256, 30000, 256, 100), (3, 50, 128, 100),
                                      (600, 20000, 128, 21)])
def test_exact_data_deep_bit_for_bit(B, n, d, k):
    nat = _native()
    qc, cc = _exact_case(B, n, d, B + n + k, ties=(k == 100))
    ref = f8_ref.scores(qc, cc)
    alive, bits = None, None
    if B != 64:                                    # every case but one runs with an alive bitmap
        alive = np.random.default_rng(n + k).random(n) < 0.8
        words = np.packbits(np.concatenate([alive, np.zeros((-n) % 32 + 256, bool)]), bitorder="little").view(np.int32)
        bits = torch.from_numpy(words.copy()).to(DEV)
    s, r = nat.cosine_topk_deep(_codes_to_dev(qc), _codes_to_dev(cc), n, d, k, alive_bits=bits)
    rr, rs = f8_ref.topk(ref, k, alive)
    assert np.array_equal(r.cpu().numpy(), rr)
    assert np.array_equal(s.cpu().numpy().astype(np.float64), rs)


@pytest.mark.parametrize("B,n,d,k", [(64, 40000, 256, 1000), (64, 40000, 128, 100), (33, 40000, 128, 1000),
                                      (1, 40000, 128, 1000), (64, 70000, 128, 1000), (64, 40000, 384, 1000)])
def test_exact_data_bounded_deep_two_block_waves(B, n, d, k):
    """the bounded path (n above the candidate capacity: few scores pass the filter) on the 64-query plan, whose waves
    own two row blocks: the filter epilogue reads the last block's last accumulator register right after the last
    MFMA, and lost that row before the kernel waited for the instruction to drain (csrc/slab_ring_body.inc)"""
    test_exact_data_deep_bit_for_bit(B, n, d, k)


def test_operand_map_asymmetric():
    """one-hot query columns against a corpus whose column j holds a value that names j: a swapped or permuted operand
    map pairs the wrong columns and cannot reproduce the scores"""
    nat = _native()
    d, n = 256, 512
    vals = np.array([0.5, 1, 1.5, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128])
    c = vals[(np.arange(n)[:, None] * 7 + np.arange(d)[None, :] * 3) % 16] * (1 + (np.arange(d) % 2))
    q = np.zeros((d, d))
    q[np.arange(d), np.arange(d)] = 1.0 + (np.arange(d) % 5)
    qc, cc = f8_ref.encode_scaled(q), f8_ref.encode_scaled(c)
    ref = f8_ref.scores(qc, cc)
    s, r = nat.cosine_topk(_codes_to_dev(qc), _codes_to_dev(cc), n, d, 20)
    rr, rs = f8_ref.topk(ref, 20)
    assert np.array_equal(r.cpu().numpy(), rr)
    assert np.array_equal(s.cpu().numpy().astype(np.float64), rs)


def _check_unit(q, c, k, s_gpu, r_gpu):
    d = q.shape[1]
    qc, cc = f8_ref.encode(q), f8_ref.encode(c)
    ref = f8_ref.scores(qc, cc)
    absum = np.abs(f8_ref.decode(qc)) @ np.abs(f8_ref.decode(cc)).T * 2.0 ** -16
    bound = 2 * d * 2.0 ** -24 * absum
    rr, rs = f8_ref.topk(ref, k)
    s_gpu, r_gpu = s_gpu.cpu().numpy().astype(np.float64), r_gpu.cpu().numpy()
    for b in range(q.shape[0]):
        err = np.abs(s_gpu[b] - ref[b, r_gpu[b]])
        assert (err <= bound[b, r_gpu[b]]).all(), (b, err.max())
        kth = rs[b, -1]
        for row in set(r_gpu[b]) ^ set(rr[b]):     # rows inside the bound of the k-th score are interchangeable
            assert abs(ref[b, row] - kth) <= bound[b, row] + bound[b, rr[b, -1]], (b, row)


def test_unit_vectors_within_float32_bound():
    nat = _native()
    rows, qs = f8_ref.clustered(n=6000, d=768, n_q=48)
    g = np.random.default_rng(5)
    gr = g.standard_normal((3000, 200)).astype(np.float32)
    gq = g.standard_normal((9, 200)).astype(np.float32)
    gr /= np.linalg.norm(gr, axis=1, keepdims=True)
    gq /= np.linalg.norm(gq, axis=1, keepdims=True)
    for q, c in ((qs, rows), (gq, gr)):
        d = q.shape[1]
        qd, cd = _quantise(q, d), _quantise(c, d)
        for k in (5, 20):
            s, r = nat.cosine_topk(qd, cd, c.shape[0], d, k)
            _check_unit(q, c, k, s, r)
        s, r = nat.cosine_topk_deep(qd, cd, c.shape[0], d, 80)
        _check_unit(q, c, 80, s, r)


def test_scores_do_not_depend_on_batch():
    nat = _native()
    rows, qs = f8_ref.clustered(n=5000, d=768, n_q=256)
    qd, cd = _quantise(qs, 768), _quantise(rows, 768)
    s256, r256 = nat.cosine_topk(qd, cd, 5000, 768, 10)
    again, _ = nat.cosine_topk(qd, cd, 5000, 768, 10)
    assert torch.equal(s256, again)
    for b in (0, 100, 255):
        s1, r1 = nat.cosine_topk(qd[b:b + 1].contiguous(), cd, 5000, 768, 10)
        assert torch.equal(s1[0], s256[b]) and torch.equal(r1[0], r256[b])


@pytest.mark.parametrize("C", [1, 20, 21, 80, 4096])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_rescore_topk(C, dtype):
    nat = _native()
    from multimodal_rag_amd.lexical import rows_dot

    n, d, B = 6000, 200, 5
    g = np.random.default_rng(C)
    c = g.standard_normal((n, d)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    c[1::2] = c[::2]                                   # pairs of equal rows: equal scores, the lower row first
    q = c[g.integers(0, n, B)] + 0.1 * g.standard_normal((B, d)).astype(np.float32)
    ld = nat.padded_dim(d, dtype)
    plane = torch.zeros((n, ld), dtype=dtype, device=DEV)
    nat.append_rows(plane, 0, torch.from_numpy(c).to(DEV), d)
    qp = torch.zeros((B, ld), dtype=dtype, device=DEV)
    nat.append_rows(qp, 0, torch.from_numpy(q).to(DEV), d)
    cand = np.stack([g.permutation(n)[:C] for _ in range(B)]).astype(np.int64)
    if C > 1:
        cand[1, C // 2:] = -1                          # a list that ends early
        cand[2, 1:] = -1
    cand_d = torch.from_numpy(cand).to(DEV)
    pf, qf = plane[:, :d].float().cpu().numpy(), qp[:, :d].float().cpu().numpy()
    for k in sorted({1, min(5, C), C}):
        s, r = nat.rescore_topk(qp, plane, d, cand_d, k)
        # scores: mmrag_rows_dot on the same pairs, bit for bit
        valid = r >= 0
        qi = torch.nonzero(valid)[:, 0].to(torch.int32)
        dots = rows_dot(qp, plane, d, qi.contiguous(), r[valid].contiguous())
        assert torch.equal(dots, s[valid])
        assert torch.isinf(s[~valid]).all()
        # rows and order: the float64 re-scoring of the same lists; near-ties inside rows_dot's bound may swap
        rr, rs = f8_ref.rescore(qf, pf, cand, k)
        r_h, s_h = r.cpu().numpy(), s.cpu().numpy().astype(np.float64)
        assert np.array_equal(r_h >= 0, rr >= 0)
        for b in range(B):
            m = int((rr[b] >= 0).sum())
            bound = 2 * d * 2.0 ** -24 * (np.abs(pf[rr[b, :m]]) @ np.abs(qf[b])).max(initial=0.0)
            assert np.all(np.abs(s_h[b, :m] - rs[b, :m]) <= bound)
            for i in np.nonzero(r_h[b, :m] != rr[b, :m])[0]:
                assert abs(rs[b, i] - pf[r_h[b, i]].astype(np.float64) @ qf[b]) <= 2 * bound
            assert np.all((np.diff(s_h[b, :m]) < 0) | ((np.diff(s_h[b, :m]) == 0) & (np.diff(r_h[b, :m]) > 0)))
        # the order in which candidates are listed does not matter (the early-ending lists keep their live prefix)
        sh = cand.copy()
        for b in range(B):
            m = int((sh[b] >= 0).sum()) if (sh[b] < 0).any() else C
            sh[b, :m] = sh[b, :m][g.permutation(m)]
        s2, r2 = nat.rescore_topk(qp, plane, d, torch.from_numpy(sh).to(DEV), k)
        assert torch.equal(s2, s) and torch.equal(r2, r)
        s3, r3 = nat.rescore_topk(qp[3:4].contiguous(), plane, d, cand_d[3:4].contiguous(), k)
        assert torch.equal(s3[0], s[3]) and torch.equal(r3[0], r[3])


def _recall(found, truth):
    return float(np.mean([len(set(f) & set(t)) / len(t) for f, t in zip(found, truth)]))


@pytest.mark.parametrize("oversample", [4, 8])
def test_recall_end_to_end(oversample, monkeypatch):
    from multimodal_rag_amd.config import settings
    from multimodal_rag_amd.index import VectorIndex

    monkeypatch.setattr(settings, "MMRAG_F8_OVERSAMPLE", oversample)
    rows, qs = f8_ref.clustered()
    n = rows.shape[0]
    idx = VectorIndex(768, dtype=torch.float8_e4m3fn, device=DEV, capacity=n)
    assert idx.rescore_dtype == torch.float16 and idx.matrix.element_size() == 1
    idx.add(rows, ids=[f"r{i}" for i in range(n)])
    exact = rows.astype(np.float64) @ qs.astype(np.float64).T            # [n, B], unquantised
    ref8 = f8_ref.scores(f8_ref.encode(qs), f8_ref.encode(rows))
    plane = rows.astype(np.float16).astype(np.float64)
    q16 = qs.astype(np.float16).astype(np.float64)
    for k in (5, 10, 20):
        truth = [np.lexsort((np.arange(n), -exact[:, b]))[:k] for b in range(qs.shape[0])]
        C = min(max(20, oversample * k), 4096)
        cand, _ = f8_ref.topk(ref8, C)
        ref_rows, _ = f8_ref.rescore(q16, plane, cand, k)
        ref_recall = _recall(ref_rows, truth)
        _, got = idx.search(qs, k)
        gpu_recall = _recall(got.cpu().numpy(), truth)
        print(f"oversample {oversample} k {k}: reference recall {ref_recall:.4f}, GPU recall {gpu_recall:.4f}")
        assert ref_recall >= 0.98
        assert gpu_recall >= ref_recall - 0.01


@pytest.mark.parametrize("rescore", [torch.float16, None])
def test_index_behaviour(rescore, tmp_path):
    from multimodal_rag_amd.index import VectorIndex
    from multimodal_rag_amd.persistence import load_index, save_index

    rows, qs = f8_ref.clustered(n=3000, d=384, n_q=6)
    n = rows.shape[0]
    ids = [f"id{i}" for i in range(n)]
    metas = [{"g": i % 3} for i in range(n)]
    docs = [f"document number {i} about topic {i % 17}" for i in range(n)]
    idx = VectorIndex(384, dtype=torch.float8_e4m3fn, device=DEV, capacity=256, rescore_dtype=rescore)
    idx.add(rows[:2000], docs[:2000], metas[:2000], ids[:2000])
    idx.add(rows[2000:], docs[2000:], metas[2000:], ids[2000:])
    assert idx.matrix.element_size() == 1 and idx.matrix.shape[1] == 384
    assert (idx.plane is None) == (rescore is None)
    assert idx.bytes_per_row() == (384 + (768 if rescore is not None else 0))
    res = idx.query(qs, n_results=5)
    if rescore is not None:
        f16 = VectorIndex(384, dtype=torch.float16, device=DEV, capacity=n)
        f16.add(rows, docs, metas, ids)
        want = f16.query(qs, n_results=6)
        for b in range(qs.shape[0]):
            dist = want["distances"][b]
            for i in range(5):
                # the two kernels' float32 bounds (2 d 2^-24 each, unit vectors): ids agree where neighbours differ more
                gap = 4 * 384 * 2.0 ** -24
                if (i == 0 or dist[i] - dist[i - 1] > gap) and dist[i + 1] - dist[i] > gap:
                    assert res["ids"][b][i] == want["ids"][b][i]
                    assert abs(res["distances"][b][i] - dist[i]) <= gap
    filt = idx.query(qs, n_results=5, where={"g": 1})
    assert all(int(i[2:]) % 3 == 1 for row in filt["ids"] for i in row)
    victims = [res["ids"][0][0], res["ids"][1][1]]
    idx.delete(ids=victims)
    after = idx.query(qs, n_results=5)
    assert not set(victims) & {i for row in after["ids"] for i in row}
    emb = idx.get(ids=[after["ids"][0][0]], include=["embeddings"])["embeddings"][0]
    src = rows[int(after["ids"][0][0][2:])]
    assert np.abs(np.asarray(emb) - src).max() <= (2.0 ** -11 if rescore is not None else 2.0 ** -4 * np.abs(src).max())
    idx.compact()
    assert idx.rows_in_use == n - 2
    compacted = idx.query(qs, n_results=5)
    assert compacted["ids"] == after["ids"] and compacted["distances"] == after["distances"]
    deep = idx.query(qs[:2], n_results=30)
    if rescore is None:
        assert deep["ids"][0][:5] == after["ids"][0]       # one scan plane, one order
    else:
        # candidates differ (C = 120 against 20), so compare with the float64 re-scoring of the reference's candidates
        live = np.array([i not in victims for i in ids])
        cand, _ = f8_ref.topk(f8_ref.scores(f8_ref.encode(qs[:2]), f8_ref.encode(rows)), 120, live)
        p64, q64 = rows.astype(np.float16).astype(np.float64), qs[:2].astype(np.float16).astype(np.float64)
        want_rows, want_s = f8_ref.rescore(q64, p64, cand, 30)
        gap = 4 * 384 * 2.0 ** -24
        for b in range(2):
            assert np.abs(1.0 - np.array(deep["distances"][b]) - want_s[b]).max() <= gap
            for i in range(30):
                lone = (i == 0 or want_s[b, i - 1] - want_s[b, i] > gap) and (i == 29 or want_s[b, i] - want_s[b, i + 1] > gap)
                if lone:
                    assert deep["ids"][b][i] == ids[want_rows[b, i]]
    save_index(idx, str(tmp_path / "save"))
    back = load_index(str(tmp_path / "save"), device=DEV)
    assert back.dtype == torch.float8_e4m3fn and back.rescore_dtype == rescore
    loaded = back.query(qs, n_results=5)
    assert loaded["ids"] == after["ids"] and loaded["distances"] == after["distances"]
    texts = [f"topic {b}" for b in range(qs.shape[0])]
    if rescore is None:
        with pytest.raises(ValueError, match="MMRAG_F8_RESCORE"):
            idx.mmr_query(qs, n_results=5)
        with pytest.raises(ValueError, match="MMRAG_F8_RESCORE"):
            idx.hybrid_query(qs, texts, n_results=5)
    else:
        m = idx.mmr_query(qs, n_results=5, lambda_mult=1.0)
        assert m["ids"] == after["ids"]
        h = idx.hybrid_query(qs, texts, n_results=5)
        assert all(len(row) == 5 for row in h["ids"]) and all(np.isfinite(x) for row in h["distances"] for x in row)


def test_embedding_manager_on_fp8_collection(monkeypatch):
    import asyncio

    from multimodal_rag_amd.config import settings
    from multimodal_rag_amd.embedder import EmbeddingManager

    monkeypatch.setattr(settings, "MMRAG_INDEX_DTYPE", "float8_e4m3fn")
    run = asyncio.run
    m = EmbeddingManager(batch_size=32, enable_cache=False)
    run(m.initialize())
    assert m.collection.dtype == torch.float8_e4m3fn and m.collection.plane is not None
    assert m.collection.matrix.element_size() == 1
    corpus = [f"Paragraph {i} about topic {i % 7}: " + "word " * (5 + i % 40) for i in range(150)]
    summ = [{"id": f"text_{i}", "summary": t, "raw": t, "type": "text"} for i, t in enumerate(corpus)]
    assert run(m.embed_and_store(summ, "doc_0123456789ab"))["text"] == 150
    r = run(m.query(corpus[17], n_results=5))
    assert r["ids"][0] == "doc_0123456789ab_text_17" and abs(r["distances"][0]) <= 2e-3   # the fp16 plane's score
    assert r["distances"] == sorted(r["distances"])
    sim = run(m.get_similar_documents("doc_0123456789ab", "text_5", n_results=20))
    assert len(sim["ids"]) == 20 and "doc_0123456789ab_text_5" not in sim["ids"]
    run(m.delete_document("doc_0123456789ab"))
    st = run(m.get_collection_stats())
    assert st["count"] == 0 and st["index_dtype"] == "float8_e4m3fn" and st["bytes_per_row"] == 384 + 2 * 384
    run(m.cleanup())


def test_query_endpoint_refuses_mmr_and_hybrid_in_capacity_mode(monkeypatch):
    from starlette.testclient import TestClient

    from multimodal_rag_amd.config import settings
    from multimodal_rag_amd.server import create_app

    monkeypatch.setattr(settings, "MMRAG_INDEX_DTYPE", "float8_e4m3fn")
    monkeypatch.setattr(settings, "MMRAG_F8_RESCORE", "none")
    with TestClient(create_app()) as client:
        up = client.post("/upload", files={"file": ("a.txt", b"Machine learning on matrix cores.", "text/plain")})
        assert up.status_code == 200
        ok = client.post("/query", json={"query": "Machine Learning", "top_k": 5})
        assert ok.status_code == 200 and len(ok.json()["sources"]) == 1
        for flag in ("mmr", "hybrid"):
            r = client.post("/query", json={"query": "Machine Learning", "top_k": 5, flag: True})
            assert r.status_code == 400 and "MMRAG_F8_RESCORE" in r.json()["detail"]


def test_rescored_search_deeper_than_one_candidate_list():
    """n_results above 4096 on a collection with a plane: the single-query masked-pass loop on the scan plane,
    over-fetch 1, each pass of 20 re-scored -- the rows are the scan plane's, pass by pass, each pass in the order of
    its exact scores, and the scores are the plane's (mmrag_rows_dot's, bit for bit)"""
    from multimodal_rag_amd.index import VectorIndex
    from multimodal_rag_amd.lexical import rows_dot

    rows, qs = f8_ref.clustered(n=4400, d=128, n_q=1)
    n, k = rows.shape[0], 4200
    idx = VectorIndex(128, dtype=torch.float8_e4m3fn, device=DEV, capacity=n)
    idx.add(rows, ids=[str(i) for i in range(n)])
    s, r = idx.search(qs, k)
    assert s.shape == (1, k) and r.shape == (1, k)
    r_h, s_h = r[0].cpu().numpy(), s[0].cpu().numpy()
    assert len(set(r_h.tolist())) == k and r_h.min() >= 0
    ref8 = f8_ref.scores(f8_ref.encode(qs), f8_ref.encode(rows))[0]
    order = np.lexsort((np.arange(n), -ref8))
    bound = 2 * 128 * 2.0 ** -24 * (np.abs(f8_ref.decode(f8_ref.encode(rows))) @ np.abs(f8_ref.decode(f8_ref.encode(qs[0])))) * 2.0 ** -16
    for lo in range(0, k, 20):
        got, want = set(r_h[lo:lo + 20].tolist()), set(order[lo:lo + 20].tolist())
        for row in got ^ want:                      # rows inside the float32 bound of a pass boundary may swap passes
            edge = ref8[order[[max(lo - 1, 0), lo, min(lo + 19, n - 1), min(lo + 20, n - 1)]]]
            assert np.abs(ref8[row] - edge).min() <= 2 * bound.max(), (lo, row)
        d = np.diff(s_h[lo:lo + 20])
        assert np.all((d < 0) | ((d == 0) & (np.diff(r_h[lo:lo + 20]) > 0)))
    qp = idx._pack_plane_queries(torch.from_numpy(qs).to(DEV))
    dots = rows_dot(qp, idx.plane, 128, torch.zeros(k, dtype=torch.int32, device=DEV), r[0].contiguous())
    assert torch.equal(dots, s[0])
