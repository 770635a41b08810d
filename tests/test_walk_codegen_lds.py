"""CPU only: the walk kernel (csrc/search_qsw.hip) with the last Q k-step parked in LDS.

The parked k-step frees sixteen registers across the end of a tile, and the end of a tile spends them; that is only a gain
while hipcc keeps every product instantiation of the kernel free of spills -- a spill reload anywhere in the tile loop (the
tile end included, not only the k-steps tests/test_kernel_codegen.py looks at) waits vmcnt(0), i.e. drains the LDS-DMA
ring -- and while the parked region fits beside the ring, the lists and the exchange block in the 160 KiB of LDS."""
import re

import asm_util

WALK = r"_ZN10mmrag_impl23cosine_topk_walk_kernel\w+"


def _metadata(asm: str):
    """{kernel: {key: int}} from the amdhsa metadata at the end of the assembly"""
    out = {}
    for m in re.finditer(r"(?ms)^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:|\Z)", asm):
        block = m.group(0)
        name = re.search(r"\.name:\s+(%s)\s" % WALK, block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_walk_kernel_has_no_spills_and_fits_lds(tmp_path):
    asm = asm_util.compile_asm("search_qsw.hip", tmp_path)
    meta = _metadata(asm)
    kernels = re.findall(r"^(%s):[^\n]*\n(.*?)s_endpgm" % WALK, asm, re.S | re.M)
    assert len(kernels) >= 12          # 2 dtypes x 3 row lengths x 2 cache policies
    assert {n for n, _ in kernels} == set(meta), "metadata of every walk kernel"
    for name, body in kernels:
        md = meta[name]
        assert md["vgpr_spill_count"] == 0, f"{name}: {md['vgpr_spill_count']} VGPRs spilled"
        assert md["group_segment_fixed_size"] <= 160 * 1024, f"{name}: {md['group_segment_fixed_size']} bytes of LDS"
        lines = body.splitlines()
        mfma = [i for i, l in enumerate(lines) if "v_mfma_f32" in l]
        assert mfma, name
        start, end = asm_util.tile_loop(name, lines, mfma, label=r"\.LBB\d+_\d+")   # raw, not normalised, lines
        assert start < mfma[0] and end > mfma[-1], name
        for l in lines[start:end + 1]:
            assert "scratch_" not in l, f"{name}: spill access inside the tile loop: {l.strip()}"
