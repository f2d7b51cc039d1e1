"""The host copy pool (mrhash_amd/csrc/mrh_hostcopy.h) under AddressSanitizer + UBSan, without a GPU.

The header is plain host C++: tests/host/hostcopy_check.cpp includes it alone, is built here with g++ and runs as a process of
its own (its own main: nothing is loaded into Python, nothing is added to the environment).  It copies through copy_to_staging at the inline sizes, at the pool
threshold from both sides and with a ragged last chunk, and widens through widen_from_staging while a second thread publishes the
chunk flags in reverse order; see the program's header for the cases.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "hostcopy_check.cpp")


def test_hostcopy_header_stands_alone():
    """No HIP header, nothing of the library's namespace: a plain C++17 compiler accepts the header by itself."""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "mrh_hostcopy.h")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(CSRC, "mrh_hostcopy.h")).read()
    assert "#include <hip" not in src and "mrh::" not in src


def test_copy_pool_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "hostcopy_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                            "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if k != "MRH_COPY_THREADS"}  # the pool's default size; everything else as it is
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "hostcopy_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out
