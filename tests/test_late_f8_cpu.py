"""CPU: the host half of the FP8 token store -- the C ABI's new symbols and their argument checks (nothing is launched),
the numpy encoder against tests/f8_ref.py, TokenStore's bookkeeping at dtype="float8_e4m3fn" on its numpy stand-in, the
setting, the generated code of the FP8 and the fp16 instantiations of both MaxSim kernels, and what the quantisation
does to a ranking (references only)."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

from multimodal_rag_amd import _native
from multimodal_rag_amd.late_store import TokenStore, f8_encode_numpy
from tests import asm_util, f8_ref, late_f8_ref, late_store_ref

EINVAL, EWORKSPACE = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = "float8_e4m3fn"


# ---------------------------------------------------------------- the C ABI
PUBLIC = ("mmrag_f8_encode_rows", "mmrag_maxsim_scores_f8", "mmrag_maxsim_topk_f8_workspace_bytes", "mmrag_maxsim_topk_f8")
INTERNAL = ("mmrag_internal_maxsim_topk_f8_ex", "mmrag_internal_maxsim_topk_f8_workspace_bytes_ex")


def test_symbols_and_header():
    L = _native.lib()
    with open(os.path.join(ROOT, "include", "mmrag.h")) as f:
        header = f.read()
    for name in PUBLIC:
        assert hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    for name in INTERNAL:
        assert hasattr(L, name) and name not in header, name
    assert L.mmrag_abi_version() == 1
    for name in ("f8_encode_rows", "maxsim_scores_f8", "maxsim_topk_f8"):
        assert callable(getattr(_native, name)), name


def test_workspace_bytes():
    import torch

    wsb = _native.maxsim_topk_workspace_bytes
    f8 = torch.float8_e4m3fn
    # the dtype argument defaults to the fp16 scan's sizes
    assert wsb(16, 1000, 5) == wsb(16, 1000, 5, dtype=torch.float16)
    assert wsb(16, 1000, 5, 384, 4) == wsb(16, 1000, 5, 384, 4, torch.float16)
    # code rows: the packed question tiles are half as wide (the padded dim in bytes)
    assert wsb(16, 1000, 5) - wsb(16, 1000, 5, dtype=f8) == 16 * 128 * 1024
    assert wsb(16, 1000, 5, 1024, 0, f8) == wsb(16, 1000, 5, dtype=f8)
    assert wsb(16, 1000, 5, 384, 4, torch.float16) - wsb(16, 1000, 5, 384, 4, f8) == 4 * 128 * 384
    assert wsb(16, 1000, 5, 64, 4, torch.float16) == wsb(16, 1000, 5, 64, 4, f8)       # dim 64 pads to one slab of codes
    for bad in ((0, 10, 5), (4097, 10, 5), (1, -1, 5), (1, 1 << 31, 5), (1, 10, 0), (1, 10, 4097)):
        assert wsb(*bad, dtype=f8) == 0, bad
    assert wsb(16, 1000, 5, 96, 0, f8) == 0
    with pytest.raises(ValueError, match="dtype"):
        wsb(1, 10, 5, dtype=torch.bfloat16)


def test_entry_refusals():
    import torch

    L = _native.lib()
    x = ctypes.c_void_p(256)
    need = _native.maxsim_topk_workspace_bytes(2, 10, 5, 64, dtype=torch.float8_e4m3fn)
    assert 0 < need <= _native.maxsim_topk_workspace_bytes(2, 10, 5, dtype=torch.float8_e4m3fn)

    def topk(q=x, q_rows=10, q_ld=128, qs=x, ql=x, Q=2, tok=x, T=100, ld=128, off=x, n_items=10, alive=None, dim=64, k=5,
             out_s=x, out_r=x, ws=x, ws_bytes=need):
        return L.mmrag_maxsim_topk_f8(q, q_rows, q_ld, qs, ql, Q, tok, T, ld, off, n_items, alive, dim, k, out_s, out_r,
                                      ws, ws_bytes, None)

    cases = [(dict(**{k: None}), EINVAL, "null") for k in ("q", "qs", "ql", "tok", "off", "out_s", "out_r")]
    cases += [(dict(dim=0), EINVAL, "dim must be a multiple of 64"), (dict(dim=96), EINVAL, "dim must be"),
              (dict(dim=1088, q_ld=1152, ld=1152), EINVAL, "at most 1024"),
              (dict(dim=256), EINVAL, "0 < d <= ld"),
              # the fp16 pitch rule's widths: 64 halfs are a slab, 64 codes are half of one
              (dict(q_ld=64), EINVAL, "whole 128-byte slabs of codes"), (dict(ld=64), EINVAL, "whole 128-byte slabs of codes"),
              (dict(dim=192, q_ld=192, ld=256), EINVAL, "whole 128-byte slabs of codes"),
              (dict(Q=0), EINVAL, "outside 1..4096"), (dict(Q=4097), EINVAL, "outside 1..4096"),
              (dict(n_items=-1), EINVAL, "n_items"), (dict(n_items=1 << 31), EINVAL, "n_items"),
              (dict(T=-1), EINVAL, "T < 2^31"), (dict(T=1 << 31), EINVAL, "T < 2^31"), (dict(q_rows=0), EINVAL, "q_rows"),
              (dict(k=0), EINVAL, "outside 1..4096"), (dict(k=4097), EINVAL, "outside 1..4096"),
              (dict(q=ctypes.c_void_p(264)), EINVAL, "16-byte aligned"),
              (dict(tok=ctypes.c_void_p(260)), EINVAL, "16-byte aligned"),
              (dict(ws=None), EWORKSPACE, "workspace"), (dict(ws_bytes=need - 1), EWORKSPACE, "workspace"),
              (dict(ws=ctypes.c_void_p(264)), EWORKSPACE, "16-byte aligned")]
    for kw, status, text in cases:
        assert topk(**kw) == status, kw
        err = L.mmrag_last_error().decode()
        assert err.startswith("maxsim_topk_f8:") and text in err, (kw, err)

    def scores(q=x, q_rows=10, q_ld=128, d=x, d_rows=10, d_ld=128, dim=64, qs=x, ql=x, n_q=1, ds=x, dl=x, n_d=1, pq=x,
               pd=x, P=1, out=x):
        return L.mmrag_maxsim_scores_f8(q, q_rows, q_ld, d, d_rows, d_ld, dim, qs, ql, n_q, ds, dl, n_d, pq, pd, P, out,
                                        None, None, None)

    cases = [(dict(**{k: None}), "null") for k in ("q", "d", "qs", "ql", "ds", "dl", "pq", "pd", "out")]
    cases += [(dict(dim=96), "dim must be"), (dict(dim=2048, q_ld=2048, d_ld=2048), "at most 1024"),
              (dict(q_ld=64), "whole 128-byte slabs of codes"), (dict(d_ld=192), "whole 128-byte slabs of codes"),
              (dict(dim=256), "0 < d <= ld"), (dict(P=0), "outside 1..65535"), (dict(P=65536), "outside 1..65535"),
              (dict(n_q=0), "at least one sequence"), (dict(d_rows=0), "at least one sequence"),
              (dict(q=ctypes.c_void_p(264)), "16-byte aligned")]
    for kw, text in cases:
        assert scores(**kw) == EINVAL, kw
        err = L.mmrag_last_error().decode()
        assert err.startswith("maxsim_scores_f8:") and text in err, (kw, err)

    def encode(src=x, dt=_native.F16, m=4, d=64, src_ld=64, dst=x, dst_ld=128):
        return L.mmrag_f8_encode_rows(src, dt, m, d, src_ld, dst, dst_ld, None)

    for kw, text in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(dt=_native.BF16), "MMRAG_F16 or MMRAG_F32"),
                     (dict(dt=_native.F8E4M3), "MMRAG_F16 or MMRAG_F32"), (dict(m=-1), "m >= 0"), (dict(d=0), "0 < d"),
                     (dict(src_ld=32), "src_ld"), (dict(dst_ld=64), "whole 128-byte slabs of codes"),
                     (dict(d=192, src_ld=192, dst_ld=128), "dst_ld"), (dict(dst=ctypes.c_void_p(264)), "16-byte aligned")):
        assert encode(**kw) == EINVAL, kw
        err = L.mmrag_last_error().decode()
        assert err.startswith("f8_encode_rows:") and text in err, (kw, err)
    assert encode(m=0) == 0      # nothing to do, nothing launched
    # the fp16 entries refuse what they refused: their messages carry their own names
    assert L.mmrag_maxsim_topk(x, 10, 100, x, x, 2, x, 100, 64, x, 10, None, 64, 5, x, x, x, need, None) == EINVAL
    assert L.mmrag_last_error().decode().startswith("maxsim_topk: ld must cover whole 128-byte slabs (mmrag_padded_dim)")


# ---------------------------------------------------------------- the numpy encoder
def test_numpy_encoder_equals_the_reference():
    for x in (f8_ref.sweep(), f8_ref.saturating()):
        assert np.array_equal(f8_encode_numpy(x), f8_ref.encode(x))
    # fp16 sources: every finite half, widened exactly
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    assert np.array_equal(f8_encode_numpy(h), f8_ref.encode(h.astype(np.float32)))
    assert f8_encode_numpy(np.zeros((3, 5), np.float16)).shape == (3, 5)


# ---------------------------------------------------------------- the store's bookkeeping
def rows_of(n, dim, tag):
    """n rows whose first column names them: (tag + i) / 256 stores the code of tag + i, exact for integers up to 16"""
    x = np.zeros((n, dim), np.float32)
    x[:, 0] = (tag + np.arange(n)) / 256.0
    return x


def item_rows(st, i):
    s, n = st.span(i)
    return f8_ref.decode(st.plane[s: s + n, 0]).astype(int).tolist()


def test_f8_store_append_fill_compact_and_stats():
    st = TokenStore(64, 8, capacity=1, dtype=F8)
    assert st.plane.dtype == np.uint8 and st.plane.shape[1] == 128 and st.bytes_per_row == 128 and st.dtype == F8
    st.set_tokens([0, 1, 2], rows_of(7, 64, 1), [3, 0, 4], token_ids=[[1, 2, 3], None, [4, 5, 6, 7]])
    assert st.offsets().tolist() == [0, 3, 3, 7] and st.n_rows == 7
    assert item_rows(st, 0) == [1, 2, 3] and item_rows(st, 1) == [] and item_rows(st, 2) == [4, 5, 6, 7]
    assert (st.plane[:7, 64:] == 0).all() and (st.plane[:7, 1:64] == 0).all()           # pad columns: code 0
    st.set_tokens([5], rows_of(2, 64, 9).astype(np.float16), [2])                          # fp16 rows in
    assert st.offsets().tolist() == [0, 3, 3, 7, 7, 7, 9] and item_rows(st, 5) == [9, 10]
    # a fill of an earlier, empty item and a replacement: one gather, every other item keeps its rows
    st.set_tokens([1, 2], rows_of(3, 64, 12), [1, 2], token_ids=[[9], [8, 7]])
    assert st.offsets().tolist() == [0, 3, 4, 6, 6, 6, 8]
    assert [item_rows(st, i) for i in range(6)] == [[1, 2, 3], [12], [13, 14], [], [], [9, 10]]
    assert st.token_ids(1) == [9] and st.token_ids(2) == [8, 7]
    s = st.stats()
    assert (s["items"], s["tokens"], s["bytes"], s["dtype"], s["bytes_per_token"]) == (4, 8, 8 * 128, F8, 128)
    # rows that already are codes pass through on the internal path alone (what set_tokens_for_ids hands on)
    codes = st._as_rows(rows_of(2, 64, 15))
    assert codes.dtype == np.uint8 and codes.shape == (2, 128)
    with pytest.raises(ValueError, match="floating-point"):
        st.set_tokens([6], codes, [2])
    with pytest.raises(ValueError, match="floating-point"):
        st.set_tokens([6], np.zeros((2, 64), np.uint8), [2])
    st.set_tokens([6], codes, [2], _codes=True)
    assert item_rows(st, 6) == [15, 16]
    # compaction in `keep` order
    st.compact(np.array([0, 2, 6, 9]))
    assert st.offsets().tolist() == [0, 3, 5, 7, 7] and [item_rows(st, i) for i in range(4)] == [[1, 2, 3], [13, 14], [15, 16], []]
    with pytest.raises(ValueError, match="token store"):
        st.set_tokens([7], rows_of(1, 32, 0), [1])
    with pytest.raises(ValueError, match="dtype"):
        TokenStore(64, 8, dtype="bfloat16")
    # the stored codes are the reference's
    g = np.random.default_rng(0)
    x = g.standard_normal((5, 384)).astype(np.float32) / 8
    st = TokenStore(384, 8, dtype=F8)
    st.set_tokens([0], x, [5])
    assert np.array_equal(st.plane[:5], late_f8_ref.encode_rows(x)) and st.stats()["bytes"] == 5 * 384
    assert TokenStore(64, 8).stats()["dtype"] == "float16" and TokenStore(64, 8).stats()["bytes_per_token"] == 128


def test_f8_store_keeps_twice_the_rows_under_one_cap(caplog):
    dim, cap = 128, 20 * 256            # twenty fp16 token rows of 128-d
    kept = {}
    with caplog.at_level(logging.WARNING, logger="multimodal_rag_amd.late_store"):
        for dtype in ("float16", F8):
            st = TokenStore(dim, 8, max_bytes=cap, dtype=dtype)
            i = 0
            while st.dropped == 0:
                st.set_tokens([i], rows_of(4, dim, 1), [4])
                i += 1
            assert st.length(i - 1) == 0 and all(st.length(j) == 4 for j in range(i - 1))
            kept[dtype] = st.n_rows
            assert st.stats()["bytes"] == st.n_rows * st.bytes_per_row <= cap
    assert kept == {"float16": 20, F8: 40}


# ---------------------------------------------------------------- settings
def test_late_store_dtype_setting(monkeypatch):
    from multimodal_rag_amd.config import Settings

    monkeypatch.delenv("MMRAG_LATE_STORE_DTYPE", raising=False)
    assert Settings().MMRAG_LATE_STORE_DTYPE == "float16" and Settings().late_store_dtype() == "float16"
    monkeypatch.setenv("MMRAG_LATE_STORE_DTYPE", F8)
    assert Settings().late_store_dtype() == F8
    monkeypatch.setenv("MMRAG_LATE_STORE_DTYPE", "fp8")
    with pytest.raises(ValueError, match="MMRAG_LATE_STORE_DTYPE must be 'float16' or 'float8_e4m3fn'"):
        Settings()
    s = Settings.__new__(Settings)
    s.MMRAG_LATE_STORE_DTYPE = "int8"
    with pytest.raises(ValueError, match="MMRAG_LATE_STORE_DTYPE"):
        s.late_store_dtype()


def test_enable_token_store_twice_with_another_dtype_raises(monkeypatch):
    import threading
    import types

    from multimodal_rag_amd import config
    from multimodal_rag_amd.index import VectorIndex

    # enable_token_store touches the lock, the store slot and the device only: no GPU is needed for the numpy stand-in
    idx = types.SimpleNamespace(_lock=threading.RLock(), _tokens=None, device=None)
    enable = lambda *a, **kw: VectorIndex.enable_token_store(idx, *a, **kw)      # noqa: E731
    monkeypatch.setattr(config.settings, "MMRAG_LATE_STORE_DTYPE", "float16")
    st = enable(128, 8, dtype=F8)
    assert st.dtype == F8 and enable(128, 8) is st and enable(128, 8, dtype=F8) is st
    with pytest.raises(ValueError, match="holds float8_e4m3fn rows"):
        enable(128, 8, dtype="float16")
    with pytest.raises(ValueError, match="holds dim 128"):
        enable(64, 8, dtype=F8)
    idx._tokens = None
    assert enable(128, 8).dtype == "float16"                  # the setting's default
    idx._tokens = None
    monkeypatch.setattr(config.settings, "MMRAG_LATE_STORE_DTYPE", F8)
    assert enable(128, 8).dtype == F8
    with pytest.raises(ValueError, match="holds float8_e4m3fn rows"):
        enable(128, 8, dtype="float16")


# ---------------------------------------------------------------- generated code
@pytest.fixture(scope="module")
def late_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm")
    return {f: asm_util.bodies(asm_util.compile_asm(f + ".hip", out)) for f in ("maxsim", "maxsim_scan")}


# sha256[:16] of the normalised bodies (asm_util.bodies) of the fp16 instantiations of the two kernels.  Pinned when the
# FP8 instantiations were added beside them (then c67fa8cd43d26758 and 3295a16fb7437eea, the bodies of the plain functions
# before the templates) and pinned again when both kernels gave their ring loop to csrc/pair_tile.h's pair_tile_ring,
# which changed their instructions on purpose: same registers, scratch and LDS, 42 and 45 instructions fewer.
PAIR_KERNEL = "_ZN10mmrag_impl13maxsim_kernelILi%dEEEvNS_12MaxSimParamsE"
SCAN_KERNEL = "_ZN10mmrag_impl12_GLOBAL__N_118maxsim_scan_kernelILi%dEEEvNS0_12MsScanParamsE"
FP16_BASELINE = {("maxsim", PAIR_KERNEL % 1): "dec1c2280360e4a0", ("maxsim_scan", SCAN_KERNEL % 1): "7274b6d01aa4bc37"}
F8_KERNELS = (("maxsim", PAIR_KERNEL % 3), ("maxsim_scan", SCAN_KERNEL % 3))


def test_fp16_instantiations_unchanged(late_asm):
    for (src, name), want in FP16_BASELINE.items():
        assert name in late_asm[src], f"{name} no longer compiled"
        assert asm_util.body_hash(late_asm[src][name]) == want, f"{name}: instructions changed"


def test_f8_instantiations_tile_loop(late_asm):
    """16 block-scaled 16x16x128 MFMAs per slab and nothing else on the matrix pipe; no scratch anywhere in the kernel
    (so none in the tile loop: a spill reload there waits for every outstanding LDS-DMA piece)"""
    for src, name in F8_KERNELS:
        assert name in late_asm[src], name
        lines = late_asm[src][name]
        mfma = [i for i, l in enumerate(lines) if "v_mfma_scale_f32_16x16x128_f8f6f4" in l]
        assert len(mfma) == 16, (name, len(mfma))
        assert not any(re.match(r"v_mfma_(?!scale_f32_16x16x128_f8f6f4)", l) for l in lines), name
        assert not any("scratch_" in l for l in lines), f"{name}: scratch access"
        start, end = asm_util.tile_loop(name, lines, mfma)
        loop = lines[start: end + 1]
        # the wait after the tile's last block-scaled MFMA (csrc/pair_tile.h pair_tile_settle) is inside the loop
        assert any(re.match(r"s_sleep\s+1\b", l) for l in loop), name


# ---------------------------------------------------------------- what the quantisation does to a ranking
def test_quantised_ranking_keeps_the_top_of_the_fp16_ranking():
    """References only: a floor for the FORMAT on clustered unit rows, not a claim about trained models."""
    g = np.random.default_rng(7)
    dim, n_items, n_tok, n_centres, n_q, q_tok = 384, 600, 24, 300, 8, 12

    def unit_fp16(x):
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
        return x.astype(np.float16).astype(np.float32)

    centres = g.standard_normal((n_centres, dim))
    tok = unit_fp16(centres[g.integers(0, n_centres, n_items * n_tok)] + 0.6 * g.standard_normal((n_items * n_tok, dim)))
    off = (n_tok * np.arange(n_items + 1)).astype(np.int32)
    picks = g.integers(0, n_items, n_q)
    q = unit_fp16(np.concatenate([tok[off[i]: off[i] + q_tok] for i in picks]) + 0.05 * g.standard_normal((n_q * q_tok, dim)))
    qs, ql = (q_tok * np.arange(n_q)).astype(np.int32), np.full(n_q, q_tok, np.int32)
    full = late_store_ref.score_matrix(q, qs, ql, tok, off)
    quant = late_f8_ref.score_matrix(late_f8_ref.encode_rows(q), qs, ql, late_f8_ref.encode_rows(tok), off)
    _, top_full = late_store_ref.topk_of_scores(full, 10)
    _, top_quant = late_store_ref.topk_of_scores(quant, 10)
    shared = [len(set(a) & set(b)) for a, b in zip(top_full.tolist(), top_quant.tolist())]
    print("shared of 10:", shared, "largest score change:", float(np.abs(full - quant).max()))
    assert (top_full[:, 0] == top_quant[:, 0]).all()
    assert min(shared) >= 8, shared
