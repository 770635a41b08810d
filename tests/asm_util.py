"""Helpers of the CPU-only codegen tests: compile one csrc file to gfx950 assembly and take its functions apart."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal_rag_amd", "csrc")


def compile_asm(src_name: str, out_dir) -> str:
    """the gfx950 assembly text of csrc/<src_name>, compiled as the library build does"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = os.path.join(str(out_dir), os.path.splitext(src_name)[0] + ".s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I",
                        os.path.join(ROOT, "include"), os.path.join(CSRC, src_name), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def bodies(asm: str):
    """{function: normalised body}: instructions and block labels, comments and directives dropped, block numbers
    made relative to the function (.LBB12_3 -> .LBB_3)"""
    out, name, cur = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = cur
            name, cur = None, None
            continue
        t = line.split(";")[0].strip()
        if re.match(r"^\.LBB\d+_\d+:", t) or (t and not t.startswith(".")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def body_hash(lines) -> str:
    """sha256[:16] of a normalised body"""
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def tile_loop(name: str, lines, mfma, label: str = r"\.LBB_\d+"):
    """(start, end) line indices of the tile loop: the last backward branch after the last MFMA whose target sits
    before the first MFMA.  `mfma`: indices of the MFMA lines; `label`: the block-label form of `lines` (normalised
    by bodies() by default)"""
    labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(%s):" % label, l))}
    back = [(i, labels[m.group(1)]) for i, l in enumerate(lines)
            if i > mfma[-1] and (m := re.search(r"s_c?branch\w*\s+(%s)" % label, l)) and m.group(1) in labels
            and labels[m.group(1)] < mfma[0]]
    assert back, f"{name}: tile loop not found"
    end, start = back[-1]
    return start, end
