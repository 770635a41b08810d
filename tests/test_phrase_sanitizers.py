"""CPU only: mmrag_lexicon_analyze_positions (csrc/tokenizer.cpp) driven from several threads by a stand-alone program,
under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer.  Built host-only the way
tests/test_sanitizers.py builds its driver; never run on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal_rag_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "sanitize_positions.cpp")


@pytest.mark.parametrize("name,flags", [
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
    ("tsan", ["-fsanitize=thread"]),
])
def test_analyze_positions_under_sanitizers(tmp_path, name, flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / f"sanitize_positions_{name}")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", *flags,
           "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "tokenizer.cpp"), DRIVER, "-o", exe, "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0 and "sanitize_positions: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "WARNING: ThreadSanitizer" not in run.stderr
    assert "runtime error" not in run.stderr, run.stderr[-4000:]
