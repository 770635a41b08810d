"""CPU only: the FP8 (E4M3) collection's storage format, C-ABI surface and the code search_f8.hip compiles to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import asm_util
import f8_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multimodal_rag_amd", "lib", "libmmrag.so")
EINVAL = 1


def test_reference_encoder_equals_torch_cpu_cast():
    x = f8_ref.sweep()
    assert x.size > 3000
    want = (torch.from_numpy(x) * 256.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = f8_ref.encode(x)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    # every finite code is hit, both signs
    assert set(got.tolist()) >= set(range(0, 127)) | set(range(129, 255))
    # decode inverts encode on representable values; ties went to the even code
    rep = f8_ref.TABLE[np.isfinite(f8_ref.TABLE)]
    assert np.array_equal(f8_ref.decode(f8_ref.encode_scaled(rep)), rep)
    assert f8_ref.encode_scaled([0.0009765625, 0.0029296875, 17.0, 19.0]).tolist() == [0, 2, 0x58, 0x5A]


def test_reference_encoder_saturates():
    got = f8_ref.encode(f8_ref.saturating())
    assert got.tolist() == [0x7E] * 7 + [0xFE] * 7 + [0]


def _lib():
    assert os.path.exists(LIB), "libmmrag.so is not built: a missing library is a failed build, not missing hardware"
    lib = ctypes.CDLL(LIB)
    lib.mmrag_padded_dim.restype = ctypes.c_int64
    lib.mmrag_padded_dim.argtypes = [ctypes.c_int, ctypes.c_int]
    for f in (lib.mmrag_cosine_topk_workspace_bytes, lib.mmrag_cosine_topk_deep_workspace_bytes):
        f.restype = ctypes.c_size_t
        f.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    lib.mmrag_rescore_topk.restype = ctypes.c_int
    lib.mmrag_rescore_topk.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_abi_surface():
    lib = _lib()
    assert hasattr(lib, "mmrag_rescore_topk")
    hdr = open(os.path.join(ROOT, "include", "mmrag.h")).read()
    assert re.search(r"#define MMRAG_F8E4M3 3\b", hdr)
    assert re.search(r"#define MMRAG_MAX_RESCORE_CANDIDATES 4096\b", hdr)
    assert "int mmrag_rescore_topk(" in hdr
    assert lib.mmrag_abi_version() == 1
    for d, want in ((768, 768), (384, 384), (100, 128), (130, 256)):
        assert lib.mmrag_padded_dim(d, 3) == want
    assert lib.mmrag_padded_dim(768, 4) == -1
    for B, n, k in ((1, 1000, 5), (256, 1000000, 20), (600, 5000, 10)):
        assert lib.mmrag_cosine_topk_workspace_bytes(B, n, k) > 0
    for B, n, k in ((1, 1000, 21), (256, 1000000, 80), (7, 5000, 4096)):
        assert lib.mmrag_cosine_topk_deep_workspace_bytes(B, n, k) > 0


def test_rescore_bad_arguments_need_no_gpu():
    lib = _lib()
    p = ctypes.c_void_p(256)   # never dereferenced: the arguments are refused first
    call = lambda dtype, C, k, B=1, d=64, ld=64: lib.mmrag_rescore_topk(p, p, ld, dtype, d, p, B, C, k, p, p, None)  # noqa: E731
    assert call(1, 20, 0) == EINVAL          # k < 1
    assert call(1, 20, 21) == EINVAL         # k > C
    assert call(1, 4097, 5) == EINVAL        # C > 4096
    assert call(3, 20, 5) == EINVAL          # an FP8 plane
    assert call(1, 20, 5, B=0) == EINVAL
    assert call(1, 20, 5, d=65) == EINVAL    # d > ld


def test_index_rejects_bad_rescore_dtype_and_settings():
    from multimodal_rag_amd.config import Settings

    s = Settings()
    assert s.MMRAG_INDEX_DTYPE == os.getenv("MMRAG_INDEX_DTYPE", "float16")
    s.MMRAG_INDEX_DTYPE = "float8_e4m3fn"
    assert s.index_dtype() == torch.float8_e4m3fn
    s.MMRAG_F8_RESCORE = "none"
    assert s.f8_rescore_dtype() is None
    s.MMRAG_F8_RESCORE = "float16"
    assert s.f8_rescore_dtype() == torch.float16
    s.MMRAG_F8_RESCORE = "int8"
    with pytest.raises(ValueError):
        s.f8_rescore_dtype()
    assert int(Settings().MMRAG_F8_OVERSAMPLE) == int(os.getenv("MMRAG_F8_OVERSAMPLE", "4"))


@pytest.fixture(scope="module")
def f8_asm(tmp_path_factory):
    return asm_util.bodies(asm_util.compile_asm("search_f8.hip", tmp_path_factory.mktemp("asm")))


# sha256[:16] of the normalised body (asm_util.bodies, as test_deep_topk_cpu.py::BASELINE) of every function
# search_f8.hip compiled to while the kernel was still its own copy, before its body moved to slab_ring_body.inc; the
# list depths 5 / 10 / 20 pinned again after the fix of TopList::insert_strict (search_shared.h), the filter mode as it was
_F8_KERNEL = "_ZN10mmrag_impl12_GLOBAL__N_121cosine_topk_f8_kernelILi%dELi%dELi3EEEvNS_7KParamsE"
F8_BASELINE = {
    _F8_KERNEL % (2, 0): "d00faabe98f07dd7",
    _F8_KERNEL % (2, 5): "f6d4ccfc1b471fd7",
    _F8_KERNEL % (2, 10): "5ba77b7c339fa9f0",
    _F8_KERNEL % (2, 20): "aab99837d0a772f7",
    _F8_KERNEL % (4, 0): "5925728c63071711",
    _F8_KERNEL % (4, 5): "4c67c4ea4e7d5f3e",
    _F8_KERNEL % (4, 10): "bd4f1c14ea68a517",
    _F8_KERNEL % (4, 20): "88328577f8deb652",
    "_ZN10mmrag_impl12_GLOBAL__N_126fill_f8_lists_empty_kernelEPfPiiiiii": "06420a1d94009280",
}


def test_f8_instantiations_unchanged(f8_asm):
    """the body is shared with search.hip's kernel: a change there that disturbs an FP8 instruction stream fails here"""
    for name, want in F8_BASELINE.items():
        assert name in f8_asm, f"{name} no longer compiled"
        assert asm_util.body_hash(f8_asm[name]) == want, f"{name}: instructions changed"


def test_f8_tile_loops(f8_asm):
    """every instantiation's tile loop holds the block-scaled FP8 MFMA and no scratch access (a spill reload waits for
    every outstanding LDS-DMA piece); the filter instantiations have one returning atomic per lane per tile"""
    kern = {k: v for k, v in f8_asm.items() if "cosine_topk_f8_kernel" in k}
    depth = lambda name: int(re.search(r"cosine_topk_f8_kernelILi\d+ELi(\d+)E", name).group(1))  # noqa: E731
    assert sorted({depth(k) for k in kern}) == [0, 5, 10, 20], sorted(kern)
    assert len(kern) >= 8
    for name, lines in kern.items():
        mfma = [i for i, l in enumerate(lines) if "v_mfma_scale_f32_32x32x64_f8f6f4" in l]
        assert mfma, name
        assert not any(re.search(r"v_mfma_f32_\d+x\d+x\d+_(f16|bf16|fp8)", l) for l in lines), name
        start, end = asm_util.tile_loop(name, lines, mfma)
        for l in lines[start:end + 1]:
            assert "scratch_" not in l, f"{name}: spill access inside the tile loop: {l}"
        # the wait between the tile's last MFMA and the epilogue (csrc/slab_ring_body.inc: a stop-gap for a suspected
        # wait-state shortfall of the compiler): an s_sleep follows the last MFMA with nothing but scalar instructions
        # and labels in between, so no accumulator register is read before it
        sleeps = [i for i in range(start, end + 1) if re.match(r"s_sleep\s+1\b", lines[i])]
        assert sleeps, f"{name}: no s_sleep in the tile loop"
        last_mfma = max(i for i in mfma if start <= i <= end)
        after = [i for i in sleeps if i > last_mfma]
        assert after, f"{name}: s_sleep does not follow the tile loop's last MFMA"
        for l in lines[last_mfma + 1:after[0]]:
            assert re.match(r"^(s_|\.LBB_)", l), f"{name}: {l!r} between the last MFMA and the s_sleep"
        atomics = sum("global_atomic_add" in l for l in lines)
        assert atomics == (1 if depth(name) == 0 else 0), (name, atomics)
