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
# made relative) of every function search.hip compiled to before the deep search existed
BASELINE = {
    "_ZN10mmrag_impl17fill_empty_kernelEPfPxx": "f8a3b3df6c48d50f",
    "_ZN10mmrag_impl17merge_topk_kernelILi10EiEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "f45fa2fad5f17363",
    "_ZN10mmrag_impl17merge_topk_kernelILi10ExEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "9bc1a653ecb17eaa",
    "_ZN10mmrag_impl17merge_topk_kernelILi20EiEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "560e3aef8a41108d",
    "_ZN10mmrag_impl17merge_topk_kernelILi20ExEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "eb0c76b3f367ce8f",
    "_ZN10mmrag_impl17merge_topk_kernelILi5EiEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "79d346c634279511",
    "_ZN10mmrag_impl17merge_topk_kernelILi5ExEEvPKfPKT0_xxxxixPfPxS6_S6_Pix": "dc0bc87861225c25",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi2ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "b9736f7828061f5d",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi2ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "9c25911c3c73b548",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi2ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "c1d2c1be8bd999dc",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi4ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "c65359874b66bba6",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi4ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "8bd014d771a3c469",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi4ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "7da07a52ff178016",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi10ELi2ELi8ELb0EEEvNS_7KParamsE": "cb01a278856eb24e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi10ELi2ELi8ELb1EEEvNS_7KParamsE": "cb01a278856eb24e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi20ELi2ELi8ELb0EEEvNS_7KParamsE": "764e135edc7bd974",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi20ELi2ELi8ELb1EEEvNS_7KParamsE": "764e135edc7bd974",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi16ELb0EEEvNS_7KParamsE": "4d73e14248954dae",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi16ELb1EEEvNS_7KParamsE": "d435b1ff73958cba",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi8ELb0EEEvNS_7KParamsE": "b84f652a66867300",
    "_ZN10mmrag_impl18cosine_topk_kernelILi0ELi8ELi5ELi2ELi8ELb1EEEvNS_7KParamsE": "4d7fde0db46ea64c",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi2ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "e8a9980aae4b7204",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi2ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "f70f343428935c56",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi2ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "53a9c5815a936aef",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi4ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "23a6c39f4a8822e0",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi4ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "9fc6a1b39a0605ab",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi4ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "f93d3474d021b943",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi10ELi2ELi8ELb0EEEvNS_7KParamsE": "dc096b0107c94ae5",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi10ELi2ELi8ELb1EEEvNS_7KParamsE": "dc096b0107c94ae5",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi20ELi2ELi8ELb0EEEvNS_7KParamsE": "1b8c9d701f46505e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi20ELi2ELi8ELb1EEEvNS_7KParamsE": "1b8c9d701f46505e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi16ELb0EEEvNS_7KParamsE": "66752ac5c4e77312",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi16ELb1EEEvNS_7KParamsE": "c08e7e254630f2b7",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi8ELb0EEEvNS_7KParamsE": "936da2e4dab042be",
    "_ZN10mmrag_impl18cosine_topk_kernelILi1ELi8ELi5ELi2ELi8ELb1EEEvNS_7KParamsE": "629d8006d80ef74e",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi2ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "0460cfd343418dc6",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi2ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "3cfcd05d8b5b654f",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi2ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "bd018ed5ae54ae0c",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi4ELi10ELi3ELi8ELb0EEEvNS_7KParamsE": "d64fd3e7183615c3",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi4ELi20ELi3ELi8ELb0EEEvNS_7KParamsE": "0c7d542bb919b7ad",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi4ELi5ELi3ELi8ELb0EEEvNS_7KParamsE": "441435ac6e4309aa",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi10ELi2ELi8ELb0EEEvNS_7KParamsE": "b133117e6f517721",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi10ELi2ELi8ELb1EEEvNS_7KParamsE": "b133117e6f517721",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi20ELi2ELi8ELb0EEEvNS_7KParamsE": "360b8850cf92ea8f",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi20ELi2ELi8ELb1EEEvNS_7KParamsE": "360b8850cf92ea8f",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi16ELb0EEEvNS_7KParamsE": "a0e758cc2ae9ba7f",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi16ELb1EEEvNS_7KParamsE": "495d2cd5b49fdb29",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi8ELb0EEEvNS_7KParamsE": "081b7a0ec9962aca",
    "_ZN10mmrag_impl18cosine_topk_kernelILi2ELi8ELi5ELi2ELi8ELb1EEEvNS_7KParamsE": "4f4f11691a44880f",
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
