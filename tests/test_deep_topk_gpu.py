"""GPU: deep exact top-k (k = 21 .. 4096, csrc/search_deep.hip) through the C-ABI, the collection, the manager, the
dispatcher and the serving path, against the CPU oracle and against the k <= 20 kernels.

Bar: as tests/test_search_gpu.py (identical top-k id sets with candidates within 2e-4 of the k-th score
interchangeable, cosine within 1e-4); bit-exact on exactly representable integer data; the first 20 results
bit-equal (scores and rows) to mmrag_cosine_topk(k = 20) on the same inputs."""
import asyncio
import os
import socket

import numpy as np
import pytest
import torch

from oracle import search_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_rag_amd import _native

    _native.lib()
    return _native


def unit_rows(n, d, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def to_dev(N, x, dtype):
    n, d = x.shape
    ld = N.padded_dim(d, dtype)
    t = torch.zeros((max(n, 1), ld), dtype=dtype, device="cuda")
    if n:
        t[:n, :d] = torch.from_numpy(x).to("cuda").to(dtype)
    return t, t[:n, :d].to(torch.float32).cpu().numpy()


def bits_of(alive):
    words = np.zeros((alive.size + 31) // 32 + 8, dtype=np.uint32)
    idx = np.nonzero(alive)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32)).to("cuda")


def deep(N, qd, cd, n, d, k, **kw):
    s, r = N.cosine_topk_deep(qd, cd, n, d, k, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def check(s, r, es, er):
    assert r.shape == er.shape and s.shape == es.shape
    fin = np.isfinite(es)
    assert np.array_equal(np.isfinite(s), fin)
    assert np.array_equal(r[~fin], er[~fin])  # -1 padding
    assert np.all(np.abs(s[fin] - es[fin]) <= TOL)
    assert np.all(np.diff(s, axis=1)[fin[:, 1:]] <= 0)  # descending
    assert O.same_topk_sets(r, s, er, es)


# (k, B, n, d, dtype): every k, B, n and d of the grid at least once, every dtype at every B regime
PARITY = [
    (21, 1, 5000, 384, "f16"),
    (21, 300, 210000, 768, "f32"),
    (64, 7, 210000, 512, "bf16"),
    (64, 129, 5000, 768, "f16"),
    (100, 64, 210000, 384, "f32"),
    (100, 256, 1000000, 768, "f16"),
    (257, 256, 256, 384, "bf16"),
    (257, 129, 210000, 512, "f32"),
    (1000, 300, 210000, 384, "bf16"),
    (1000, 1, 1000000, 384, "f32"),
    (4096, 64, 210000, 384, "f16"),
    (4096, 1, 4095, 768, "bf16"),
]


@pytest.mark.parametrize("k,B,n,d,dt", PARITY)
def test_random_parity(N, k, B, n, d, dt):
    c = unit_rows(n, d, k + n)
    q = unit_rows(B, d, B + 7)
    cd, cs = to_dev(N, c, DT[dt])
    qd, qs = to_dev(N, q, DT[dt])
    s, r = deep(N, qd, cd, n, d, k)
    del cd
    es, er = O.cosine_topk(qs, cs, k)
    check(s, r, es, er)


@pytest.mark.parametrize("k,B", [(100, 3), (1000, 200), (257, 300)])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_integer_data_bit_exact_with_heavy_ties(N, k, B, dt):
    """values in {-2..2}/8: every product and sum is exact in float32, so scores and rows (ties -> lower row, across
    the sample boundary of the bound passes included) must equal the oracle's bit for bit"""
    g = np.random.default_rng(k + B)
    n, d = 60000, 384
    c = (g.integers(-2, 3, (n, d)) / 8).astype(np.float32)
    c[:, 4:] = 0
    q = (g.integers(-2, 3, (B, d)) / 8).astype(np.float32)
    q[:, 4:] = 0
    cd, cs = to_dev(N, c, DT[dt])
    qd, qs = to_dev(N, q, DT[dt])
    s, r = deep(N, qd, cd, n, d, k)
    es, er = O.cosine_topk(qs, cs, k)
    assert np.array_equal(s, es) and np.array_equal(r, er)


# every B regime (WN = 2, 4, 8; one and two query groups) in every dtype, and the 1M-row shape of the walk kernel
FIRST20 = [(B, 210000, dt) for B in (1, 40, 100, 200, 300) for dt in ("f16", "bf16", "f32")] + [(256, 1000000, "f16")]


@pytest.mark.parametrize("B,n,dt", FIRST20)
def test_first_20_bit_equal_to_the_list_kernels(N, B, n, dt):
    d = 768 if n == 1000000 else 384
    c = unit_rows(n, d, B)
    q = unit_rows(B, d, B + 1)
    cd, _ = to_dev(N, c, DT[dt])
    qd, _ = to_dev(N, q, DT[dt])
    s20, r20 = N.cosine_topk(qd, cd, n, d, 20)
    s, r = deep(N, qd, cd, n, d, 50)
    s20, r20 = s20.cpu().numpy(), r20.cpu().numpy()
    assert np.array_equal(s[:, :20].view(np.uint32), s20.view(np.uint32))
    assert np.array_equal(r[:, :20], r20)


def test_masks_offset_ragged_and_padding(N):
    d, n, k, B = 384, 70001, 300, 70
    c = unit_rows(n, d, 11)
    q = unit_rows(B, d, 12)
    cd, cs = to_dev(N, c, torch.float16)
    qd, qs = to_dev(N, q, torch.float16)
    alive = np.random.default_rng(13).random(n) < 0.7
    s, r = deep(N, qd, cd, n, d, k, row_offset=1000, alive_bits=bits_of(alive))
    es, er = O.cosine_topk(qs, cs, k, row_offset=1000, alive=alive)
    check(s, r, es, er)
    # a selective filter: fewer live rows than k -> (-inf, -1) padding
    few = np.zeros(n, bool)
    few[np.random.default_rng(14).choice(n, 50, replace=False)] = True
    s, r = deep(N, qd, cd, n, d, k, alive_bits=bits_of(few))
    es, er = O.cosine_topk(qs, cs, k, alive=few)
    check(s, r, es, er)
    assert np.all(r[:, 50:] == -1) and np.all(np.isneginf(s[:, 50:]))
    # n = 0
    s, r = deep(N, qd, cd, 0, d, k)
    assert np.all(r == -1) and np.all(np.isneginf(s))


def test_overflow_all_scores_tie(N):
    """50 000 identical rows and a query equal to them: every row survives every bound, the buffer overflows and the
    query is re-run alone -- still exact (the lowest k rows, in order)"""
    d, n, k = 384, 50000, 100
    g = np.random.default_rng(21)
    v = np.zeros((1, d), np.float32)
    v[0, :16] = g.integers(-2, 3, 16) / 8   # exact in every dtype and every sum: bit-exact against the oracle
    c = np.repeat(v, n, 0)
    w = np.zeros((2, d), np.float32)
    w[:, :16] = g.integers(-2, 3, (2, 16)) / 8
    q = np.concatenate([v, w])
    cd, cs = to_dev(N, c, torch.float16)
    qd, qs = to_dev(N, q, torch.float16)
    s, r = deep(N, qd, cd, n, d, k)
    es, er = O.cosine_topk(qs, cs, k)
    assert np.array_equal(r, er) and np.array_equal(s, es)
    assert np.array_equal(r[0], np.arange(k))


@pytest.mark.parametrize("dbg,cap", [(0, 512), (1, 0), (1, 700)])
def test_overflow_small_capacity_and_no_bound(N, dbg, cap):
    d, n, k, B = 512, 100000, 100, 70
    c = unit_rows(n, d, 31)
    q = unit_rows(B, d, 32)
    cd, cs = to_dev(N, c, torch.bfloat16)
    qd, qs = to_dev(N, q, torch.bfloat16)
    s, r = deep(N, qd, cd, n, d, k, dbg=dbg, cap=cap)
    es, er = O.cosine_topk(qs, cs, k)
    check(s, r, es, er)
    s0, r0 = deep(N, qd, cd, n, d, k)
    assert np.array_equal(s, s0) and np.array_equal(r, r0)


def test_overflow_of_one_query_in_a_batch(N):
    """two tiles and 256 candidate slots: query 0 ties on every row, so its 512 survivors overflow and it is re-run
    alone.  Queries 1 and 2 have 512 distinct scores each, rising and falling with the row: whichever 256 rows the
    bound pass kept, at least 30 of them come from one tile, so at least one of the two gets a bound with at most
    256 survivors and is selected from the batch's slots.  Every value is exact in float16 and every sum in float32:
    bit for bit against the oracle"""
    d, n, k = 384, 512, 30
    c = np.zeros((n, d), np.float32)
    c[:, 0] = np.arange(n) / 512
    c[:, 1] = 0.25
    q = np.zeros((3, d), np.float32)
    q[0, 1] = 1.0
    q[1, 0] = 1.0
    q[2, :2] = (-1.0, 0.5)
    cd, cs = to_dev(N, c, torch.float16)
    qd, qs = to_dev(N, q, torch.float16)
    s, r = deep(N, qd, cd, n, d, k, cap=256)
    es, er = O.cosine_topk(qs, cs, k)
    assert np.array_equal(r, er) and np.array_equal(s, es)
    assert np.array_equal(r[0], np.arange(k)) and np.array_equal(r[1], n - 1 - np.arange(k))
    assert np.array_equal(r[2], np.arange(k))


def unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_collection_query_batch_deep(N):
    """fails before the deep search: 'n_results > 20 is supported for single queries only'"""
    from multimodal_rag_amd.index import VectorIndex

    d, n = 384, 30000
    idx = VectorIndex(d, dtype=torch.float16, capacity=1024)
    V = unit(n, d, 41)
    ids = [f"id{i}" for i in range(n)]
    idx.add(V.tolist(), [f"d{i}" for i in range(n)], [{"t": i % 3} for i in range(n)], ids)
    q = unit(9, d, 42)
    res = idx.query(q.tolist(), n_results=45)
    stored = np.asarray(idx.get(ids=ids, include=["embeddings"])["embeddings"], np.float32)
    es, er = O.cosine_topk(q.astype(np.float16).astype(np.float32), stored, 45)
    got = np.array([[int(x[2:]) for x in row] for row in res["ids"]])
    check(1.0 - np.array(res["distances"], np.float32), got, es, er)
    # where filter
    res_f = idx.query(q.tolist(), n_results=45, where={"t": 1})
    es, er = O.cosine_topk(q.astype(np.float16).astype(np.float32), stored, 45, alive=np.arange(n) % 3 == 1)
    got = np.array([[int(x[2:]) for x in row] for row in res_f["ids"]])
    check(1.0 - np.array(res_f["distances"], np.float32), got, es, er)


@pytest.fixture(scope="module")
def manager(N):
    from multimodal_rag_amd.embedder import EmbeddingManager, HipEngine

    eng = HipEngine("sentence-transformers/all-MiniLM-L6-v2")
    m = EmbeddingManager(engine=eng)

    async def go():
        await m.initialize()
        items = [{"id": f"text_{i}", "summary": f"passage number {i} about topic {i % 17}", "raw": "", "type":
                  "text" if i % 4 else "table"} for i in range(3000)]
        for lo in range(0, 3000, 1000):
            await m.embed_and_store(items[lo:lo + 1000], f"doc_{lo:012x}")
    asyncio.run(go())
    return m


def test_manager_batch_query_and_similar_documents(manager):
    m = manager
    texts = [f"what is said about topic {i}" for i in range(6)]
    out = asyncio.run(m.batch_query(texts, n_results=30))
    assert len(out) == 6
    for res, t in zip(out, texts):
        assert "error" not in res, res.get("error")
        assert len(res["ids"]) == 30
        solo = asyncio.run(m.query(t, n_results=30))
        assert solo["ids"] == res["ids"]
    sim = asyncio.run(m.get_similar_documents("doc_000000000000", "text_5", n_results=20))
    assert "error" not in sim and len(sim["ids"]) == 20 and "text_5" not in sim["ids"]


def test_dispatcher_concurrent_deep_queries(manager):
    m = manager
    texts = [f"passage {i * 13} on topic {i}" for i in range(8)]
    solo = [asyncio.run(m.query(t, n_results=30)) for t in texts]

    async def go():
        disp = m.enable_dynamic_batching(max_batch=64, max_wait_ms=50.0)
        try:
            out = await asyncio.gather(*[m.query(t, n_results=30) for t in texts])
            stats = dict(disp.stats)
        finally:
            await disp.stop()
            m._dispatcher = None
        return out, stats

    out, stats = asyncio.run(go())
    assert stats["max_batch_seen"] > 1, stats
    for a, b in zip(out, solo):
        assert "error" not in a
        assert a["ids"] == b["ids"]
        assert np.array_equal(np.array(a["distances"]), np.array(b["distances"]))


@pytest.fixture(scope="module")
def pg(N):
    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield True
    dist.destroy_process_group()


def test_serving_deep_batch_equals_plain_collection(pg):
    from multimodal_rag_amd.index import VectorIndex
    from multimodal_rag_amd.serving import ShardedCollection

    d, n = 384, 20000
    v = unit(n, d, 51)
    ids = [f"doc_{i // 1000:012x}_text_{i}" for i in range(n)]
    metas = [{"doc_id": s[:16], "type": "image" if i % 5 == 0 else "text"} for i, s in enumerate(ids)]
    q = unit(4, d, 52)
    plain = VectorIndex(d, device="cuda:0")
    col = ShardedCollection(VectorIndex(d, device="cuda:0"), device=torch.device("cuda", 0))
    try:
        for c in (plain, col):
            for lo in range(0, n, 5000):
                c.add(v[lo:lo + 5000].tolist(), documents=[f"d{i}" for i in range(lo, lo + 5000)],
                      metadatas=metas[lo:lo + 5000], ids=ids[lo:lo + 5000])
        for kw in ({"n_results": 50}, {"n_results": 50, "where": {"type": "image"}}):
            a, b = col.query(q.tolist(), **kw), plain.query(q.tolist(), **kw)
            assert a["ids"] == b["ids"] and a["documents"] == b["documents"]
            assert np.array_equal(np.array(a["distances"]), np.array(b["distances"]))
            assert len(a["ids"]) == 4 and all(len(row) == 50 for row in a["ids"])
    finally:
        col.stop()
