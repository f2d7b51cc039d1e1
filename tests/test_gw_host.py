"""The pure host parts of the GeoWrapper facade (mrhash_amd/csrc/gw_pose.h, gw_chunks.h, gw_files.h) on the CPU, under
AddressSanitizer + UBSan.

tests/host/gw_check.cpp includes the three headers, is built here with g++ (-ffp-contract=off, as the module) and runs as a process
of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  It checks the pose conversions, the
chunk arithmetic and the host chunk grid, the plan of extractMesh, the mesh PLY against an iostream restatement for 1, 2 and 7
workers, the MRHGRID1 file, the serializeData clouds and the seeds PLY; see the program's header.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
PROGRAM = os.path.join(ROOT, "tests", "host", "gw_check.cpp")


def test_gw_headers_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "gw_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-I", CSRC, "-I", INCLUDE, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "gw_check: 0 failures" in r.stdout
    assert "gw_check: compared 100017 doubles, 0 differ" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out


@pytest.mark.parametrize("header", ["gw_pose.h", "gw_chunks.h", "gw_files.h"])
def test_header_stands_alone(tmp_path, header):
    """Each header compiles by itself, includes nothing of the facade beyond include/*.h, and knows neither a context nor the C ABI's calls."""
    src = str(tmp_path / "alone.cpp")
    open(src, "w").write('#include "%s"\nint main() { return 0; }\n' % header)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", CSRC, "-I", INCLUDE, src],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(CSRC, header)).read()
    assert "mrh_ctx" not in text and "geowrapper.h" not in text
    for line in text.splitlines():
        if line.startswith("#include \""):
            assert line.split('"')[1].startswith("mrhash_"), line
