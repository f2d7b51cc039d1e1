"""The host half of depth-frame tracking (mrhash_amd/csrc/mrh_tracksolve.h) on the CPU, under AddressSanitizer +
UBSan: tests/host/track_solve_check.cpp includes the header alone, is built here with g++ (-ffp-contract=off, as the library) and
runs as a process of its own (its own main: nothing is loaded into Python, nothing is added to the environment).  Its scale, solve,
update and rms equal the numpy restatement (tests/track_ref.py) bit for bit on the sums of the analytic room, of a degenerate
model and of an empty image.  The loop around them (mrh_track::fit_run, D14 "Loop") runs in the same program with a callable that
replays recorded sums: the pose it hands out at every step, its status, its count, its pose and its sums equal the restatement
when every step is solved, when a step is lost, when the callable fails and when the loop is never entered."""
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


def _loop_cases(cases):
    """(far, min_pixels, iterations, run, recorded steps, fail_at, fail_code, R0, t0) for the loop, from the three-step sequences of
    _cases(): the sums of step k were taken at (float) of the restatement's state after k updates, so a callable that replays them
    stands for the linearisation."""
    seqs = [cases[i:i + 3] for i in (0, 3, 6)]
    R0, t0 = cases[0][3].astype(np.float32), cases[0][4].astype(np.float32)  # the start of every sequence: a widened float
    far, s = seqs[0][0][0], [c[2] for c in seqs[0]]
    zero, plane = np.zeros(32, np.int64), cases[9][2]
    assert tr.solve(plane, far, 64) is None and int(plane[28]) >= 64  # lost by the pivot gate, not by the count
    out = [(q[0][0], 64, 3, 1, [c[2] for c in q], -1, 0, R0, t0) for q in seqs]  # three solved steps
    out.append((far, 64, 3, 1, [s[0], zero], -1, 0, R0, t0))     # lost at the second step: no pixel
    out.append((far, 64, 3, 1, [s[0], plane], -1, 0, R0, t0))    # ... a degenerate plane
    out.append((far, 64, 3, 1, s, 1, -2, R0, t0))                # the callable fails at step 1
    out.append((far, 64, 1, 1, [s[0]], -1, 0, R0, t0))           # iterations = 1
    out.append((far, 64, 3, 0, [], -1, 0, R0, t0))               # an empty observation: the loop is not entered
    out.append((far, 5000, 3, 1, [s[0]], -1, 0, R0, t0))         # lost at the first step: too few pixels
    return out


def _loop_ref(far, min_pixels, iterations, run, steps, fail_at, fail_code, R0, t0):
    """D14 "Loop" in numpy (track_ref.track with the linearisation replaced by the recorded sums): the poses handed out, the
    return value, status, updates, the binary64 state and the sums."""
    R, t = R0.astype(np.float64), t0.astype(np.float64)
    handed, rc, status, done, sums = [], 0, tr.TRACK_LOST, 0, np.zeros(32, np.int64)
    if run:
        status = tr.TRACK_OK
        for k in range(iterations):
            handed.append((R.astype(np.float32), t.astype(np.float32)))
            if k == fail_at:
                rc, status = fail_code, None
                break
            sums = steps[k]
            xi = tr.solve(sums, far, min_pixels)
            if xi is None:
                rc = status = tr.TRACK_LOST
                break
            R, t = tr.update(R, t, xi)
            done += 1
    return handed, rc, status, done, R, t, sums


def _hex32(values):
    return " ".join(float(v).hex() for v in np.asarray(values, np.float32).ravel())


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
    loops = _loop_cases(cases)
    for far, min_pixels, iterations, run, steps, fail_at, fail_code, R0, t0 in loops:
        text += "loop %r %d %d %d %d %d %d %s %s %s\n" % (float(far), min_pixels, iterations, run, len(steps), fail_at, fail_code, _hex32(R0), _hex32(t0),
                                                         " ".join(str(int(v)) for s in steps for v in s))
    env =dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out
    lines = r.stdout.splitlines()
    assert lines[-1] == "track_solve_check: %d cases" % (len(cases) + len(loops))
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

    def floats(line, word):
        parts = line.split()
        assert parts[0] == word, line
        return np.array([float.fromhex(x) for x in parts[1:]])

    outcomes = []
    for case in loops:
        handed, rc, status, done, R, t, sums = _loop_ref(*case)
        for R32, t32 in handed:  # the pose the callable is handed at step k: (float) of the restatement's state, bit for bit
            got = floats(next(it), "at")
            assert np.array_equal(got[:9], R32.ravel().astype(np.float64)) and np.array_equal(got[9:], t32.astype(np.float64)), case
        got = [int(x) for x in next(it).split()[1:]]
        assert got[0] == rc and got[2] == done and got[3] == len(handed) and got[4] == int(sums[28]), (got, rc, done, len(handed))
        if status is not None:  # a failed callable leaves no status to report: the call returns its error
            assert got[1] == status, (got, status)
        pose = floats(next(it), "pose")
        assert np.array_equal(pose[:9], R.astype(np.float32).ravel().astype(np.float64)), case
        assert np.array_equal(pose[9:], t.astype(np.float32).astype(np.float64)), case
        n = int(sums[28])
        rms = float(np.sqrt(np.float64(sums[27]) / np.float64(n)) / np.float64(262144.0)) if n else 0.0
        assert floats(next(it), "rms")[0] == rms
        assert [int(x) for x in next(it).split()[1:]] == [int(v) for v in sums], case
        outcomes.append((rc, status, done, len(handed)))
    assert next(it) == lines[-1]
    OK, LOST = tr.TRACK_OK, tr.TRACK_LOST
    # three solved steps (x 3), lost at the second step (x 2: the pose is the one after the first step and the sums are the failed
    # step's, as compared above), the callable's -2 at step 1 (two calls, one update), one iteration, an empty observation, lost at once
    assert outcomes == [(0, OK, 3, 3)] * 3 + [(LOST, LOST, 1, 2)] * 2 + [(-2, None, 1, 2), (0, OK, 1, 1), (0, LOST, 0, 0), (LOST, LOST, 0, 1)]
    start = loops[0]
    assert np.array_equal(_loop_ref(*loops[8])[4], start[7].astype(np.float64)) and np.array_equal(_loop_ref(*loops[7])[5], start[8].astype(np.float64))
