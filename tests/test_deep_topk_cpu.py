"""CPU only: the deep top-k's C-ABI surface (include/mmrag.h) and a codegen guard on csrc/search.hip.

The deep search (csrc/search_deep.hip) reuses the slab-ring cosine_topk_kernel in a new compile-time mode (K = 0, the
filter epilogue).  Adding it must leave every list instantiation that existed before instruction for instruction as
it was -- their scores are what the deep search is bit-identical to -- and the filter mode's tile loop must not spill
(a scratch reload waits vmcnt(0), which drains the LDS-DMA ring)."""
import ctypes
import os
import re

import pytest

import asm_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multimodal_rag_amd", "lib", "libmmrag.so")

# sha256[:16] of the normalised body (instructions and block labels, comments and directives dropped, block numbers
# made relative) of every function search.hip compiled to before the deep search existed.  The list kernels
# (cosine_topk_kernel) were pinned again after TopList::insert_strict stopped dropping the lowest row of a run of equal
# scores (search_shared.h; tests/test_search_regimes_gpu.py, plateau_two_level): that fix changes every one of them and
# nothing else.
BASELINE = {
    "_ZN10mmrag_impl17fill_empty_kernelEPfPxx": "f8a3b3df6c48d50f",
    "_ZN10mmrag_impl17merge_topk_kernelILi10EiEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "f45fa2fad5f17363",
    "_ZN10mmrag_impl17merge_topk_kernelILi10ExEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "9bc1a653ecb17eaa",
    "_ZN10mmrag_impl17merge_topk_kernelILi20EiEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "560e3aef8a41108d",
    "_ZN10mmrag_impl17merge_topk_kernelILi20ExEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "eb0c76b3f367ce8f",
    "_ZN10mmrag_impl17merge_topk_kernelILi5EiEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "79d346c634279511",
    "_ZN10mmrag_impl17merge_topk_kernelILi5ExEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "dc0bc87861225c25",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi2ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "00f106ddf86a4647",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi2ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "f62c8473f1fad9a5",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi2ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "e2b6a4fe89004f06",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi4ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "3d12cfb546523115",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi4ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "17ef77577ac1a047",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi4ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "db13dc8fafaebe52",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi10ELi2ELi8ELb0EEEvNS_7KParamsE": "d7559f9ebfec068d",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi10ELi2ELi8ELb1EEEvNS_7KParamsE": "d7559f9ebfec068d",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi20ELi2ELi8ELb0EEEvNS_7KParamsE": "af7d711efc36c0b8",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi20ELi2ELi8ELb1EEEvNS_7KParamsE": "af7d711efc36c0b8",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi16ELb0EEEvNS_7KParamsE": "f1b7a00f8d434008",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi16ELb1EEEvNS_7KParamsE": "1eaef91c4d474882",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi8ELb0EEEvNS_7KParamsE": "2dd4047893c8fddf",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi8ELb1EEEvNS_7KParamsE": "af23131c1b9a578d",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi2ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "40103555e9aa9687",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi2ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "5e6cc77019332627",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi2ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "2dca54e341e984b4",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi4ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "efa453b151b1e400",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi4ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "de1e7bf4a99cf5d1",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi4ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "1f0715c52ff342d9",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi10ELi2ELi8ELb0EEEvNS_7KParamsE": "40f13155b28acd37",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi10ELi2ELi8ELb1EEEvNS_7KParamsE": "40f13155b28acd37",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi20ELi2ELi8ELb0EEEvNS_7KParamsE": "2ad019c7e7051bee",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi20ELi2ELi8ELb1EEEvNS_7KParamsE": "2ad019c7e7051bee",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi16ELb0EEEvNS_7KParamsE": "bf5be2e38c33abe8",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi16ELb1EEEvNS_7KParamsE": "a5d16488c6b719dc",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi8ELb0EEEvNS_7KParamsE": "49413319c432600e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi8ELb1EEEvNS_7KParamsE": "68434f6b6f7c3935",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi2ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "e9032b2683508b07",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi2ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "66fcb32d1fa9cc21",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi2ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "3f158b1d52ccbb27",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi4ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "3b1a4b65e1a11d37",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi4ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "369030f4f1fd9237",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi4ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "2e1e153fdd7f8f0c",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi10ELi2ELi8ELb0EEEvNS_7KParamsE": "98cd20f378dbce6e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi10ELi2ELi8ELb1EEEvNS_7KParamsE": "98cd20f378dbce6e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi20ELi2ELi8ELb0EEEvNS_7KParamsE": "f70c55e30c388883",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi20ELi2ELi8ELb1EEEvNS_7KParamsE": "f70c55e30c388883",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi16ELb0EEEvNS_7KParamsE": "404a7495705b1abb",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi16ELb1EEEvNS_7KParamsE": "4db16f4601a0b6f1",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi8ELb0EEEvNS_7KParamsE": "1fe6d44a254e440c",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi8ELb1EEEvNS_7KParamsE": "76db663c036c58a6",
    "_ZN10mmrag_impl22fill_seed_empty_kernelEPfPixix": "cb045e16c5d7420a",
}


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("libmmrag.so not built")
    lib = ctypes.CDLL(LIB)
    lib.mmrag_cosine_topk_deep_workspace_bytes.restype = ctypes.c_size_t
    lib.mmrag_cosine_topk_deep_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    return lib


def test_deep_symbols_exported():
    lib = _lib()
    for name in ("mmrag_cosine_topk_deep", "mmrag_cosine_topk_deep_workspace_bytes", "mmrag_cosine_topk",
                 "mmrag_cosine_topk_workspace_bytes"):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "mmrag.h")).read()
    assert re.search(r"#define MMRAG_MAX_K_DEEP 4096\b", hdr)
    assert re.search(r"#define MMRAG_MAX_K 20\b", hdr)
    assert "int mmrag_cosine_topk_deep(" in hdr and "size_t mmrag_cosine_topk_deep_workspace_bytes(" in hdr


def test_deep_workspace_bytes():
    ws = _lib().mmrag_cosine_topk_deep_workspace_bytes
    for B, n, k in ((1, 1000, 0), (1, 1000, 4097), (0, 1000, 50), (4, -1, 50)):
        assert ws(B, n, k) == 0, (B, n, k)
    for B, n, k in ((1, 0, 1), (1, 1000, 21), (7, 5000, 100), (256, 1000000, 1000), (300, 210000, 4096)):
        assert ws(B, n, k) > 0, (B, n, k)
    # the single-query overflow re-run keeps n candidates: the workspace grows with n at least by 8 bytes a row
    assert ws(1, 2000000, 100) - ws(1, 1000000, 100) >= 8 * 1000000
    assert ws(256, 1000000, 100) > ws(1, 1000000, 100)


@pytest.fixture(scope="module")
def search_asm(tmp_path_factory):
    return asm_util.bodies(asm_util.compile_asm("search.hip", tmp_path_factory.mktemp("asm")))


def test_existing_instantiations_unchanged(search_asm):
    for name, want in BASELINE.items():
        assert name in search_asm, f"{name} no longer compiled"
        got = asm_util.body_hash(search_asm[name])
        assert got == want, f"{name}: instructions changed"


def test_filter_mode_tile_loop_has_no_spills(search_asm):
    filt = {k: v for k, v in search_asm.items() if re.match(r"_ZN10mmrag_impl18cosine_topk_kernelILi\dELi\dELi0E", k)}
    assert len(filt) == 9, sorted(filt)   # 3 dtypes x WN = 2, 4, 8
    for name, lines in filt.items():
        mfma = [i for i, l in enumerate(lines) if "v_mfma_f32" in l]
        assert mfma, name
        start, end = asm_util.tile_loop(name, lines, mfma)
        for l in lines[start:end + 1]:
            assert "scratch_" not in l, f"{name}: spill access inside the tile loop: {l}"
        assert sum("global_atomic_add" in l for l in lines) == 1, name   # one returning atomic per lane per tile
