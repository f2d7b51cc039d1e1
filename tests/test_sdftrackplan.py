"""The argument plan of render-free tracking (mrh_plan::sdftrack in mrhash_amd/csrc/mrh_readerplan.h) on the CPU, under
AddressSanitizer + UBSan.

tests/host/sdftrackplan_check.cpp includes the header alone, is built here with g++ (-ffp-contract=off, as the library) and runs as a
process of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  It checks every refusal with
its error code, their order, the defaults, what the points form does not read, and the 4096 and 2^24 caps; see the program's header.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "sdftrackplan_check.cpp")


def test_sdftrack_plan_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "sdftrackplan_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "sdftrackplan_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out
