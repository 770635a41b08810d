"""CPU: the host half of the token store -- tests/late_store_ref.py against a loop over late_ref.score_tables, the
C-ABI's argument checks of mmrag_maxsim_topk (nothing is launched) and TokenStore's bookkeeping on its numpy stand-in
(device=None): append, length-0 items, fills, the byte cap and compaction in `keep` order."""
import ctypes
import logging
import os

import numpy as np
import pytest

from multimodal_rag_amd import _native
from multimodal_rag_amd.late_store import TokenStore, _ranges
from tests import late_store_ref as R

EINVAL, EWORKSPACE = 1, 2


# ---------------------------------------------------------------- the reference
def int_rows(g, n, dim):
    return g.integers(-2, 3, (n, dim)).astype(np.float32)


def test_reference_topk_equals_pair_loop():
    dim = 16
    g = np.random.default_rng(0)
    lens = [3, 0, 7, 1, 3, 0, 12, 3]
    tok = np.concatenate([int_rows(g, n, dim) for n in lens] + [np.full((2, dim), 50.0, np.float32)])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    tok[off[4]: off[5]] = tok[off[0]: off[1]]      # items 0 and 4 tie for every question
    tok[off[7]: off[8]] = tok[off[0]: off[1]]      # and item 7
    q_tok = int_rows(g, 20, dim)
    q_start, q_len = np.array([0, 5, 6, 19], np.int32), np.array([5, 1, 10, 2], np.int32)   # the last: outside q_tok
    alive = np.array([1, 1, 1, 0, 1, 1, 1, 1], bool)
    for k in (1, 3, 9):
        for a in (None, alive):
            s, r = R.topk(q_tok, q_start, q_len, tok, off, k, a)
            s2, r2 = R.topk_by_pairs(q_tok, q_start, q_len, tok, off, k, a)
            assert np.array_equal(r, r2) and np.array_equal(s, s2), (k, a)
            assert (r[3] == -1).all() and np.isneginf(s[3]).all()                # the bad question: padding only
            n_cand = 6 if a is None else 5
            assert ((r[:3] >= 0).sum(axis=1) == min(k, n_cand)).all()
            assert not np.isin(r, [1, 5]).any() and (a is None or not (r == 3).any())
            for q in range(3):
                got = [int(i) for i in r[q] if i >= 0]
                # ties to the lower item: 0 before 4 before 7 wherever they appear
                tied = [i for i in got if i in (0, 4, 7)]
                assert tied == sorted(tied)
                assert all(s[q, j] >= s[q, j + 1] for j in range(len(got) - 1))
    # the guard rows after the last item never take part: a huge row there changes nothing
    tok2 = tok.copy()
    tok2[off[-1]:] = -50.0
    assert np.array_equal(R.score_matrix(q_tok, q_start, q_len, tok, off), R.score_matrix(q_tok, q_start, q_len, tok2, off))


def test_reference_integer_rows_are_exact_in_float32():
    g = np.random.default_rng(1)
    q, d = int_rows(g, 128, 384), int_rows(g, 512, 384)
    s = R.score_matrix(q, [0], [128], d, [0, 512])
    assert s[0, 0] == float(np.float32(s[0, 0])) and abs(s[0, 0]) < 2 ** 24


# ---------------------------------------------------------------- the C ABI
def test_symbols_and_header():
    L = _native.lib()
    for name in ("mmrag_maxsim_topk", "mmrag_maxsim_topk_workspace_bytes", "mmrag_internal_maxsim_topk_ex"):
        assert hasattr(L, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mmrag.h")) as f:
        header = f.read()
    assert "#define MMRAG_MAX_LATE_QUESTIONS 4096" in header and _native.MAX_LATE_QUESTIONS == 4096
    assert "mmrag_internal_maxsim_topk_ex" not in header


def test_workspace_bytes():
    wsb = _native.maxsim_topk_workspace_bytes
    assert wsb(1, 1000, 5) >= 16384 * 8 + 128 * 2048
    assert wsb(16, 1000, 5) > wsb(1, 1000, 5) and wsb(1, 1 << 20, 5) > wsb(1, 1000, 5)
    assert wsb(1, 1000, 4096) > wsb(1, 1000, 5)
    for bad in ((0, 10, 5), (4097, 10, 5), (1, -1, 5), (1, 1 << 31, 5), (1, 10, 0), (1, 10, 4097)):
        assert wsb(*bad) == 0, bad
    # with dim and a bound on the question tiles: what the call itself checks; smaller at 384-d and with shared tiles
    assert wsb(16, 1000, 5, 1024, 0) == wsb(16, 1000, 5) > wsb(16, 1000, 5, 384) > wsb(16, 1000, 5, 384, 4)
    assert wsb(16, 1000, 5, 384) - wsb(16, 1000, 5, 384, 4) == 12 * 128 * 768
    assert wsb(16, 1000, 5, 96) == 0 and wsb(16, 1000, 5, 384, 99) == wsb(16, 1000, 5, 384)
    assert _native.late_question_tiles([0, 32, 64, 96, 128], [32, 32, 32, 32, 1], 200) == 2
    assert _native.late_question_tiles([0, 0, 0], [100, 100, 0], 200) == 2 and _native.late_question_tiles([], [], 5) == 1
    assert _native.late_question_tiles([0, 150], [128, 60], 200) == 1        # the second lies outside the rows


def test_entry_refusals():
    L = _native.lib()
    x = ctypes.c_void_p(256)
    # what this call needs (dim 64, a tile per question); the public size is an upper bound of it for every dim
    need = _native.maxsim_topk_workspace_bytes(2, 10, 5, 64)
    assert 0 < need <= _native.maxsim_topk_workspace_bytes(2, 10, 5)

    def call(q=x, q_rows=10, q_ld=64, qs=x, ql=x, Q=2, tok=x, T=100, ld=64, off=x, n_items=10, alive=None, dim=64, k=5,
             out_s=x, out_r=x, ws=x, ws_bytes=need):
        return L.mmrag_maxsim_topk(q, q_rows, q_ld, qs, ql, Q, tok, T, ld, off, n_items, alive, dim, k, out_s, out_r, ws,
                                   ws_bytes, None)

    cases = [(dict(**{k: None}), EINVAL, "null") for k in ("q", "qs", "ql", "tok", "off", "out_s", "out_r")]
    cases += [(dict(dim=0), EINVAL, "dim must be a multiple of 64"), (dict(dim=96, q_ld=128, ld=128), EINVAL, "dim must be"),
              (dict(dim=1088, q_ld=1088, ld=1088), EINVAL, "at most 1024"), (dict(dim=128), EINVAL, "0 < d <= ld"),
              (dict(q_ld=96), EINVAL, "whole 128-byte slabs"), (dict(ld=100), EINVAL, "whole 128-byte slabs"),
              (dict(Q=0), EINVAL, "outside 1..4096"), (dict(Q=4097), EINVAL, "outside 1..4096"),
              (dict(n_items=-1), EINVAL, "n_items"), (dict(n_items=1 << 31), EINVAL, "n_items"),
              (dict(T=-1), EINVAL, "T < 2^31"), (dict(T=1 << 31), EINVAL, "T < 2^31"), (dict(q_rows=0), EINVAL, "q_rows"),
              (dict(k=0), EINVAL, "outside 1..4096"), (dict(k=4097), EINVAL, "outside 1..4096"),
              (dict(q=ctypes.c_void_p(264)), EINVAL, "16-byte aligned"),
              (dict(tok=ctypes.c_void_p(260)), EINVAL, "16-byte aligned"),
              (dict(ws=None), EWORKSPACE, "workspace"), (dict(ws_bytes=need - 1), EWORKSPACE, "workspace"),
              (dict(ws=ctypes.c_void_p(264)), EWORKSPACE, "16-byte aligned")]
    for kw, status, text in cases:
        assert call(**kw) == status, kw
        err = L.mmrag_last_error().decode()
        assert err.startswith("maxsim_topk:") and text in err, (kw, err)


# ---------------------------------------------------------------- the store's bookkeeping
def rows_of(n, dim, tag):
    """n rows whose first column names them: tag + 0, tag + 1, ..."""
    x = np.zeros((n, dim), np.float16)
    x[:, 0] = tag + np.arange(n)
    return x


def item_rows(st, i):
    s, n = st.span(i)
    return st.plane[s: s + n, 0].astype(int).tolist()


def test_ranges():
    assert _ranges(np.array([5, 0, 9]), np.array([2, 0, 3])).tolist() == [5, 6, 9, 10, 11]
    assert _ranges(np.array([3]), np.array([0])).tolist() == []
    assert _ranges(np.array([7, 2]), np.array([1, 2])).tolist() == [7, 2, 3]


def test_store_append_fill_and_lengths():
    st = TokenStore(64, 8, capacity=1)
    assert st.n_rows == 0 and st.offsets(3).tolist() == [0, 0, 0, 0]
    st.set_tokens([0, 1, 2], rows_of(7, 64, 100), [3, 0, 4], token_ids=[[1, 2, 3], None, [4, 5, 6, 7]])
    assert st.offsets().tolist() == [0, 3, 3, 7] and st.n_rows == 7
    assert item_rows(st, 0) == [100, 101, 102] and item_rows(st, 1) == [] and item_rows(st, 2) == [103, 104, 105, 106]
    assert st.token_ids(0) == [1, 2, 3] and st.token_ids(1) is None and st.token_ids(2) == [4, 5, 6, 7]
    # an append that leaves a gap: items 3, 4 are unknown to the store, i.e. empty
    st.set_tokens([5], rows_of(2, 64, 200), [2])
    assert st.offsets().tolist() == [0, 3, 3, 7, 7, 7, 9] and st.length(4) == 0 and item_rows(st, 5) == [200, 201]
    # offsets for more rows than the store has heard of: they are empty too
    assert st.offsets(8).tolist() == [0, 3, 3, 7, 7, 7, 9, 9, 9]
    # the plane grew past its first capacity
    big = TokenStore(64, 8, capacity=256)
    for i in range(60):
        big.set_tokens([i], rows_of(8, 64, 8 * i), [8])
    assert big.n_rows == 480 and big.plane.shape[0] >= 480 and item_rows(big, 59) == list(range(472, 480))
    # a fill of an earlier, empty item and a replacement: one gather, every other item keeps its rows
    st.set_tokens([1, 2], rows_of(3, 64, 300), [1, 2], token_ids=[[9], [8, 7]])
    assert st.offsets().tolist() == [0, 3, 4, 6, 6, 6, 8]
    assert [item_rows(st, i) for i in range(6)] == [[100, 101, 102], [300], [301, 302], [], [], [200, 201]]
    assert st.token_ids(1) == [9] and st.token_ids(2) == [8, 7] and st.token_ids(5) is None
    s = st.stats()
    assert (s["items"], s["tokens"], s["bytes"], s["dim"], s["max_doc_tokens"]) == (4, 8, 8 * 128, 64, 8)
    st.reset()
    assert st.n_rows == 0 and st.n_items == 0 and st.offsets(2).tolist() == [0, 0, 0]
    for bad in (dict(rows=[0, 0], lens=[1, 1], n=2), dict(rows=[-1], lens=[1], n=1), dict(rows=[0], lens=[9], n=9),
                dict(rows=[0], lens=[2], n=3), dict(rows=[0, 1], lens=[2], n=2)):
        with pytest.raises(ValueError, match="token store"):
            st.set_tokens(bad["rows"], rows_of(bad["n"], 64, 0), bad["lens"])
    for bad in (dict(dim=96), dict(dim=0), dict(dim=1088), dict(max_doc_tokens=0), dict(max_doc_tokens=513)):
        with pytest.raises(ValueError, match="token store"):
            TokenStore(**{**dict(dim=64, max_doc_tokens=8), **bad})


def test_store_cap_gives_length_zero_and_one_warning(caplog):
    st = TokenStore(64, 8, max_bytes=10 * 128)          # ten token rows
    with caplog.at_level(logging.WARNING, logger="multimodal_rag_amd.late_store"):
        st.set_tokens([0, 1], rows_of(8, 64, 0), [4, 4])
        st.set_tokens([2, 3, 4], rows_of(6, 64, 50), [2, 3, 1])     # item 3 would make 13 rows: it and item 4 get none
        st.set_tokens([5], rows_of(1, 64, 90), [1])
    assert st.offsets().tolist() == [0, 4, 8, 10, 10, 10, 10] and st.n_rows == 10
    assert item_rows(st, 2) == [50, 51] and st.length(3) == 0 and st.length(4) == 0 and st.length(5) == 0
    assert len([r for r in caplog.records if "cap" in r.getMessage()]) == 1
    assert st.stats()["dropped_items"] == 3 and st.stats()["bytes"] == 10 * 128


def test_store_compaction_keeps_the_keep_order():
    st = TokenStore(64, 8)
    st.set_tokens([0, 1, 2, 3, 4], rows_of(12, 64, 0), [3, 0, 4, 2, 3], token_ids=[[0] * 3, None, [2] * 4, [3] * 2, [4] * 3])
    keep = np.array([0, 2, 4, 6])                        # item 6 is unknown to the store: empty
    st.compact(keep)
    assert st.offsets().tolist() == [0, 3, 7, 10, 10] and st.n_rows == 10 and st.n_items == 4
    assert [item_rows(st, i) for i in range(4)] == [[0, 1, 2], [3, 4, 5, 6], [9, 10, 11], []]
    assert [st.token_ids(i) for i in range(4)] == [[0] * 3, [2] * 4, [4] * 3, None]
    # and the store goes on: an append after the compaction
    st.set_tokens([4], rows_of(2, 64, 70), [2])
    assert st.offsets().tolist() == [0, 3, 7, 10, 10, 12] and item_rows(st, 4) == [70, 71]
    st.compact(np.array([], np.int64))
    assert st.n_rows == 0 and st.n_items == 0


# ---------------------------------------------------------------- EmbeddingManager and POST /query, without a GPU
def test_supports_late_store_rule_and_route_refusals(monkeypatch):
    import asyncio
    import types

    from starlette.testclient import TestClient

    from multimodal_rag_amd import embedder as emb_mod
    from multimodal_rag_amd import server
    from multimodal_rag_amd.embedder import EmbeddingManager
    from multimodal_rag_amd.tokenizer import HashTokenizer
    from tests.fakes import FakeEngine

    def engine(**kw):
        e = FakeEngine()
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    enc16 = types.SimpleNamespace(encode_tokens=lambda *a: None, precision="fp16")
    enc32 = types.SimpleNamespace(encode_tokens=lambda *a: None, precision="fp32")
    tk = HashTokenizer(3000)
    can = EmbeddingManager(engine=engine(encoder=enc16, tokenizer=tk))
    assert can.supports_late_store() and not can.late_store_enabled() and not can.supports_late_query()
    assert not EmbeddingManager(engine=engine(encoder=enc32, tokenizer=tk)).supports_late_store()     # fp32 mode
    assert not EmbeddingManager(engine=engine(clip=object(), tokenizer=tk)).supports_late_store()    # the CLIP towers
    can.collection = types.SimpleNamespace()         # a collection without a token store: the sharded path
    assert not can.supports_late_store()
    with pytest.raises(ValueError, match="token store needs a single BERT-family fp16 HIP engine"):
        can._enable_late_store_sync()
    # MMRAG_LATE_STORE with an embedder that cannot: one warning, the upload goes through
    monkeypatch.setattr(emb_mod.settings, "MMRAG_LATE_STORE", True)
    monkeypatch.setattr(emb_mod, "_late_store_warned", False)
    m = EmbeddingManager(engine=FakeEngine())
    with TestClient(server.create_app(embedder=m)) as c:
        for i in range(2):
            r = c.post("/upload", files={"file": (f"d{i}.txt", b"alpha beta gamma. " * 3, "text/plain")})
            assert r.status_code == 200, r.text
        assert emb_mod._late_store_warned
        q = {"query": "alpha", "top_k": 2}
        plain = c.post("/query", json=q).json()["sources"]
        r = c.post("/query", json={**q, "late": True})
        assert r.status_code == 400 and r.json()["detail"] == server.LATE_QUERY_NEEDS[2]
        assert "is not available with this embedder: it needs" in server.LATE_QUERY_NEEDS[2]
        for other in ({"hybrid": True}, {"mmr": True}, {"group_by_document": True}, {"variants": ["beta"]},
                      {"boost": True}, {"like": ["d0"]}):
            r = c.post("/query", json={**q, "late": True, **other})
            assert r.status_code == 400, other
        r = c.post("/query", json={**q, "late": True, "hybrid": True})
        assert "Late retrieval is not combined with" in r.json()["detail"]
        assert c.post("/query", json={**q, "late": False}).json()["sources"] == plain       # the default changes nothing
        with pytest.raises(ValueError, match="late retrieval needs a single-GPU collection"):
            asyncio.run(m.late_query("alpha"))
        out = asyncio.run(m.batch_late_query(["alpha", ""]))
        assert all("error" in o and o["ids"] == [] and o["late_scores"] == [] for o in out)


def test_late_store_settings(monkeypatch):
    from multimodal_rag_amd.config import Settings

    assert Settings().MMRAG_LATE_STORE is False and Settings().MMRAG_LATE_STORE_MAX_BYTES == 0
    monkeypatch.setenv("MMRAG_LATE_STORE", "1")
    monkeypatch.setenv("MMRAG_LATE_STORE_MAX_BYTES", str(1 << 30))
    assert Settings().MMRAG_LATE_STORE is True and Settings().MMRAG_LATE_STORE_MAX_BYTES == 1 << 30
