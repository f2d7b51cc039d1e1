"""The host half of depth-frame tracking (mrhash_amd/csrc/mrh_tracksolve.h) on the CPU, under AddressSanitizer +
UBSan: tests/host/track_solve_check.cpp includes the header alone, is built here with g++ (-ffp-contract=off, as the library) and
runs as a process of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  Its scale, solve,
update and rms equal the numpy restatement (tests/track_ref.py) bit for bit on the sums of the analytic room, of a degenerate
model and of an empty image."""
import os
import shutil
import subprocess

import numpy as np

import track_ref as tr
from mrhash_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mrhash_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "host", "track_solve_check.cpp")


def test_track_solve_header_stands_alone():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "mrh_tracksolve.h")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "#include <hip" not in open(os.path.join(CSRC, "mrh_tracksolve.h")).read()


def _cases():
    K = synth.REPLICA_640
    K80 = synth.Intrinsics(K.fx / 8, K.fy / 8, K.cx / 8, K.cy / 8, 60, 80)
    KT = (K80.fx, K80.fy, K80.cx, K80.cy, 60, 80)
    scene = synth.replica_room()
    poses = synth.orbit_poses(22)
    R19, t19 = synth.quat_to_rot(poses[19][1]), poses[19][0]
    Md, Mn = tr.analytic_model(scene, K80, R19, t19)
    out = []
    for target, far in ((20, 8.0), (21, 8.0), (20, 30.0)):
        f = synth.render(scene, K80, *poses[target], depth_scaling=6553.5)
        R, t = R19.astype(np.float64), t19.astype(np.float64)
        for _ in range(3):  # three steps of the loop: the state is no longer a widened float
            sums = tr.linearise(f.depth, KT, 0.1, far, 0.14, R.astype(np.float32), t.astype(np.float32), R19, t19, Md, Mn)
            out.append((far, 64, sums, R, t))
            R, t = tr.update(R, t, tr.solve(sums, far, 64))
    plane_d = np.full((60, 80), 2.0, np.float32)
    plane_n = np.zeros((60, 80, 3), np.float32)
    plane_n[..., 2] = -1.0
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    out.append((8.0, 64, tr.linearise((plane_d * np.float32(1.01)).astype(np.float32), KT, 0.1, 8.0, 0.14, I, z, I, z, plane_d, plane_n),
                np.eye(3), np.zeros(3)))  # the pivot gate
    out.append((8.0, 64, np.zeros(32, np.int64), np.eye(3), np.zeros(3)))  # no pixel
    out.append((8.0, 5000, out[0][2], out[0][3], out[0][4]))  # too few pixels
    return out


def test_host_solve_equals_the_restatement_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "track_solve_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-I", CSRC, PROGRAM, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    cases = _cases()
    text = ""
    for far, min_pixels, sums, R, t in cases:
        text += "%r %d %s %s %s\n" % (float(far), min_pixels, " ".join(str(int(v)) for v in sums),
                                      " ".join(float(v).hex() for v in np.asarray(R).ravel()), " ".join(float(v).hex() for v in t))
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out
    lines = r.stdout.splitlines()
    assert lines[-1] == "track_solve_check: %d cases" % len(cases)
    it = iter(lines)
    solved = 0
    for far, min_pixels, sums, R, t in cases:
        assert float.fromhex(next(it).split()[1]) == float(tr.angle_scale(far))
        xi = tr.solve(sums, far, min_pixels)
        if xi is None:
            assert next(it) == "lost"
        else:
            solved += 1
            got = [float.fromhex(x) for x in next(it).split()[1:]]
            assert np.array_equal(np.array(got), xi), (got, xi)
            Rn, tn = tr.update(R, t, xi)
            got = [float.fromhex(x) for x in next(it).split()[1:]]
            assert np.array_equal(np.array(got[:9]), Rn.ravel()) and np.array_equal(np.array(got[9:]), tn)
        n = int(sums[28])
        rms = float(np.sqrt(np.float64(sums[27]) / np.float64(n)) / np.float64(262144.0)) if n else 0.0
        assert float.fromhex(next(it).split()[1]) == rms
    assert solved == 9
