"""The argument plans of the map readers and of the scan normals (mrhash_amd/csrc/mrh_readerplan.h) on the CPU, under AddressSanitizer +
UBSan.

The header is plain host C++: tests/host/readerplan_check.cpp includes it alone, is built here with g++ (-ffp-contract=off, as the
library) and runs as a process of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  It checks
the sample count against a literal linear count, the spherical angle bound, the limits of a distance field's box, the defaults of
w_min and of tracking, the order of the checks with each case's error code, and one message per feature against the C ABI's text;
see the program's header.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "readerplan_check.cpp")


def test_readerplan_header_stands_alone():
    """No HIP header, no context: a plain C++17 compiler accepts the header by itself."""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "mrh_readerplan.h")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(CSRC, "mrh_readerplan.h")).read()
    assert "#include <hip" not in src and "hip_runtime" not in src and "mrh_ctx*" not in src and "mrh_context.h" not in src


def test_reader_plans_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "readerplan_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "readerplan_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out
