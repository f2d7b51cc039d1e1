"""The argument and size plan of map-to-map fusion (mrh_plan::remap and its helpers in mrhash_amd/csrc/mrh_readerplan.h) on the CPU,
under AddressSanitizer + UBSan.

tests/host/remapplan_check.cpp includes the header alone, is built here with g++ (-ffp-contract=off, as the library) and runs as a
process of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  It checks every refusal with
its error code, their order, the ratio limits, the worst-case candidate counts at ratios 1/4, 1 and 4 and the overflow guards; see
the program's header.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "remapplan_check.cpp")


def test_remap_plan_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "remapplan_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "remapplan_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out


def test_remap_header_is_plain_c_and_bound():
    """include/mrhash_remap.h is a C header: a C compiler accepts it by itself, it adds no symbol to mrhash_hip.h, and capi binds
    every symbol it declares with structs of the C sizes."""
    import ctypes as C
    import re

    from mrhash_amd import capi

    path = os.path.join(ROOT, "include", "mrhash_remap.h")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "mrh_resample_map" not in open(os.path.join(ROOT, "include", "mrhash_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mrh_[a-z_]+)\s*\(", hdr))) == sorted(capi.REMAP_SYMBOLS)
    assert C.sizeof(capi.MrhRemapParams) == 16 and C.sizeof(capi.MrhRemapInfo) == 40
