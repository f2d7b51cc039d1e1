"""The argument plan of the ray queries (mrh_plan::rays in mrhash_amd/csrc/mrh_readerplan.h) on the CPU, under AddressSanitizer +
UBSan.

tests/host/rayplan_check.cpp includes the header alone, is built here with g++ (-ffp-contract=off, as the library) and runs as a
process of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  It checks the order of the
refusals with each case's error code, the limits of n and of the sample count, min_range == 0, the messages against the C ABI's
text, and the refusal bound; see the program's header.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "rayplan_check.cpp")


def test_ray_plan_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "rayplan_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "rayplan_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out


def test_rays_header_is_plain_c(tmp_path):
    """include/mrhash_rays.h is a C header: a C compiler accepts it by itself, it adds no symbol to mrhash_hip.h, and its
    parameter block has the 32 bytes the header states and the binding declares."""
    import ctypes as C

    from mrhash_amd import capi

    hdr = os.path.join(ROOT, "include", "mrhash_rays.h")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    base = open(os.path.join(ROOT, "include", "mrhash_hip.h")).read()
    assert "mrh_cast_rays" not in base and "mrh_rays" not in base and "MRH_RAY" not in base
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(src, "w").write('#include <stdio.h>\n#include "mrhash_rays.h"\nint main(void) { printf("%zu %zu\\n", sizeof(mrh_rays_params), '
                         '__builtin_offsetof(mrh_rays_params, reserved)); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, timeout=120)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [32, 16] == [C.sizeof(capi.MrhRaysParams), capi.MrhRaysParams.reserved.offset]
