"""The job table of the deferred column-sum finish (csrc/kernels/colsum_table.h) is host arithmetic: a stand-alone
program (tests/csrc/colsum_table_check.cpp) packs an empty list, exactly the per-launch cap, cap + 1 and mixed
widths, replays both stages of every launch pair on the host the way the kernels walk them, on buffers of exactly
the sizes the host code allocates, and runs under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "distributedvolunteercomputing_amd", "csrc", "kernels")


def _compiler():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    return None


def test_colsum_table_packing_under_sanitizer(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "colsum_table_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=all", f"-I{KERNELS}", os.path.join(ROOT, "tests", "csrc", "colsum_table_check.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    # no leak detection: the program frees through std::vector alone, and LeakSanitizer needs ptrace, which a
    # container may withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0 exitcode=67", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-6000:]
    assert "OK" in p.stdout
