"""The argument plans of the free-space layer (mrh_plan::freespace_create / _carve / _box / _segments in
mrhash_amd/csrc/mrh_readerplan.h) on the CPU, under AddressSanitizer + UBSan.

tests/host/freeplan_check.cpp includes the header alone, is built here with g++ (-ffp-contract=off, as the library) and runs as a
process of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  It checks the order of the
refusals with each case's error code, every limit at its edge, the defaults, the sample count and the bound; see the program's
header.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "freeplan_check.cpp")


def test_freespace_plans_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "freeplan_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "freeplan_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out


def test_freespace_header_is_plain_c(tmp_path):
    """include/mrhash_freespace.h is a C header: a C compiler accepts it by itself, it adds no symbol to mrhash_hip.h, and its three
    parameter blocks have the 32, 48 and 40 bytes the header states and the binding declares."""
    import ctypes as C

    from mrhash_amd import capi

    hdr = os.path.join(ROOT, "include", "mrhash_freespace.h")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    base = open(os.path.join(ROOT, "include", "mrhash_hip.h")).read()
    assert "freespace" not in base and "mrh_carve" not in base and "MRH_FREE" not in base
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(src, "w").write('#include <stdio.h>\n#include "mrhash_freespace.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                         'sizeof(mrh_freespace_params), sizeof(mrh_carve_params), sizeof(mrh_freespace_box_params), '
                         '__builtin_offsetof(mrh_freespace_params, cell_shift), __builtin_offsetof(mrh_carve_params, margin), '
                         '__builtin_offsetof(mrh_freespace_box_params, surface_band)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, timeout=120)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    want = [C.sizeof(capi.MrhFreespaceParams), C.sizeof(capi.MrhCarveParams), C.sizeof(capi.MrhFreespaceBoxParams), capi.MrhFreespaceParams.cell_shift.offset,
            capi.MrhCarveParams.margin.offset, capi.MrhFreespaceBoxParams.surface_band.offset]
    assert [int(x) for x in out] == [32, 48, 40, 24, 36, 28] == want


def test_every_declared_symbol_is_bound():
    """FREESPACE_SYMBOLS names exactly the functions the header declares."""
    import re

    from mrhash_amd import capi

    text = open(os.path.join(ROOT, "include", "mrhash_freespace.h")).read()
    declared = set(re.findall(r"^int (mrh_freespace_\w+)\(", text, re.M))
    assert declared == set(capi.FREESPACE_SYMBOLS) and len(capi.FREESPACE_SYMBOLS) == 11
