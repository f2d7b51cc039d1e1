"""The exchange plan of the multi-GPU paths (mrhash_amd/csrc/mrh_xplan.h) at 1 .. 8 ranks, on the CPU, under AddressSanitizer + UBSan.

The header is plain host C++: tests/host/xplan_check.cpp includes it alone, is built here with g++ and runs as a process of its own
(its own main: nothing is loaded into Python, nothing is added to the environment).  It builds the plan of every rank of a group for the
halo exchange, the sub-map merge and the mesh gather (every root), with and without the self-loop, and plays the grouped sends and
receives through with memcpy: sizes pair by pair and in order, no zero-size call, ranges, the gather's alignment, payloads, byte
totals; see the program's header.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "xplan_check.cpp")


def test_xplan_header_stands_alone():
    """No HIP or RCCL header, nothing of the library's namespace: a plain C++17 compiler accepts the header by itself."""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "mrh_xplan.h")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(CSRC, "mrh_xplan.h")).read()
    assert "#include <hip" not in src and "#include <rccl" not in src and "mrh::" not in src


def test_exchange_plans_of_every_rank_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "xplan_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                            "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "xplan_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out
