"""CPU half of depth-frame tracking (include/mrhash_track.h): the header, the binding and the exported symbols
agree, both structs have the C layout, and the restatement (tests/track_ref.py) gives the hand-derived answers, sums that do not
depend on the pixel order, the poses of the analytic room and the three lost cases."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest

import track_ref as tr
from mrhash_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_track_header_and_binding_agree_and_the_library_exports_them(hip):
    hdr = open(os.path.join(ROOT, "include", "mrhash_track.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mrh_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == sorted(capi.TRACK_SYMBOLS)
    for name in declared:
        assert hasattr(hip, name), f"libmrhash_hip.so does not export {name}"


def test_track_structs_match_header():
    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "mrhash_track.h"
        #define P mrh_track_params
        #define I mrh_track_info
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(P), offsetof(P, cy), offsetof(P, rows), offsetof(P, min_depth), offsetof(P, step),
                 offsetof(P, dist_max), offsetof(P, iterations), offsetof(P, min_pixels));
          printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(I), offsetof(I, status), offsetof(I, iterations_done), offsetof(I, pixels),
                 offsetof(I, rms), offsetof(I, sums), MRH_TRACK_OK, MRH_TRACK_LOST);
          return 0;
        }"""
    )
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "probe.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    P, I = capi.MrhTrackParams, capi.MrhTrackInfo
    assert got == [C.sizeof(P), P.cy.offset, P.rows.offset, P.min_depth.offset, P.step.offset, P.dist_max.offset, P.iterations.offset,
                   P.min_pixels.offset, C.sizeof(I), I.status.offset, I.iterations_done.offset, I.pixels.offset, I.rms.offset, I.sums.offset,
                   capi.TRACK_OK, capi.TRACK_LOST]
    assert got[0] == 48 and got[8] == 280
    assert (tr.TRACK_OK, tr.TRACK_LOST) == (capi.TRACK_OK, capi.TRACK_LOST)


def test_track_without_a_context_is_an_invalid_argument(hip):
    p = capi.MrhTrackParams(100.0, 100.0, 3.5, 3.5, 8, 8, 0.1, 2.0, 0.0, 0.0, 0, 0)
    R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (C.c_float * 3)(0, 0, 0)
    oR, ot = (C.c_float * 9)(), (C.c_float * 3)()
    depth = (C.c_float * 64)()
    info = capi.MrhTrackInfo()
    assert hip.mrh_track_depth(None, C.byref(p), depth, R, t, oR, ot, C.byref(info)) == capi.MRH_ERR_INVALID_ARG
    assert hip.mrh_track_depth_device(None, C.byref(p), depth, R, t, oR, ot, C.byref(info)) == capi.MRH_ERR_INVALID_ARG


# ---- known answers ---------------------------------------------------------------------------------------------------------

def test_fixed_point_scale_of_the_rotation_part():
    assert tr.angle_scale(4.0) == 2048.0      # L = 8
    assert tr.angle_scale(8.0) == 1024.0      # L = 16
    assert tr.angle_scale(30.0) == 256.0      # L = 64
    assert tr.angle_scale(0.3) == 16384.0     # L = 1


def test_one_pixel_facing_a_plane_head_on():
    """A 1 x 1 camera with fx = fy = 128, cx = -64.5, cy = -0.5 at the identity pose: d_c = (2^-7 * 64, 0, 1) = (0.5, 0, 1).
    D = 2 gives p_c = a = p_w = q = (1, 0, 2); u = (128 * 0.5 - 64.5) + 1 = 0.5, v = 0.5: pixel (0, 0).  The model there is m = 2.5
    with normal (0, 0, -1): V = 2.5 * (0.5, 0, 1) = (1.25, 0, 2.5), delta = (0.25, 0, 0.5), |delta|^2 = 0.3125 <= 1, e = -0.5.
    a x N = (a.y N.z - a.z N.y, a.z N.x - a.x N.z, a.x N.y - a.y N.x) = (0, 1, 0), so J = (0, 1, 0, 0, 0, -1).  max_depth = 4: L = 8,
    S_a = 2048, J~ = (0, 2048, 0, 0, 0, -16384), e~ = -131072.  Every other word is 0."""
    K1 = (128.0, 128.0, -64.5, -0.5, 1, 1)
    I, z = np.eye(3, dtype=F), np.zeros(3, F)
    Md, Mn = np.full((1, 1), 2.5, F), np.array([[[0, 0, -1]]], F)
    ok, Jt, et = tr.pixel_terms(np.full((1, 1), 2.0, F), K1, 0.1, 4.0, 1.0, I, z, I, z, Md, Mn)
    assert ok.tolist() == [True] and Jt.tolist() == [[0, 2048, 0, 0, 0, -16384]] and et.tolist() == [-131072]
    want = np.zeros(32, np.int64)
    want[6], want[10], want[20] = 2048 * 2048, 2048 * -16384, 16384 * 16384       # H11, H15, H55
    want[22], want[26], want[27], want[28] = 2048 * -131072, 16384 * 131072, 131072 ** 2, 1  # b1, b5, sum e~^2, n
    assert np.array_equal(tr.sums_of(ok, Jt, et), want)
    # the gate, the depth range and a missing model pixel each reject it
    assert not tr.pixel_terms(np.full((1, 1), 2.0, F), K1, 0.1, 4.0, 0.5, I, z, I, z, Md, Mn)[0].any()   # 0.3125 > 0.25
    assert not tr.pixel_terms(np.full((1, 1), 4.5, F), K1, 0.1, 4.0, 1.0, I, z, I, z, Md, Mn)[0].any()
    assert not tr.pixel_terms(np.full((1, 1), np.nan, F), K1, 0.1, 4.0, 1.0, I, z, I, z, Md, Mn)[0].any()
    assert not tr.pixel_terms(np.full((1, 1), 2.0, F), K1, 0.1, 4.0, 1.0, I, z, I, z, Md * 0, Mn)[0].any()


def test_a_pure_translation_along_the_normal_is_solved_in_one_step():
    """The solve and the update alone, on sums built by hand: six rows, J the unit vector of each coordinate, e = 0.25 on the last.
    H is the identity and b = (0, .., 0, 0.25), so xi = (0, .., 0, 0.25) exactly and the pose moves 0.25 m along z."""
    rows = np.eye(6)
    sums = np.zeros(32, np.int64)
    s = np.array([2048] * 3 + [16384] * 3, np.int64)
    Jt = (rows * s).astype(np.int64)
    et = np.array([0, 0, 0, 0, 0, int(0.25 * 262144)], np.int64)
    sums[:] = tr.sums_of(np.ones(6, bool), Jt, et)
    xi = tr.solve(sums, 4.0, 6)
    assert np.array_equal(xi, np.array([0, 0, 0, 0, 0, 0.25]))
    assert tr.solve(sums, 4.0, 7) is None  # too few pixels
    R, t = tr.update(np.eye(3), np.zeros(3), xi)
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.array([0, 0, 0.25]))
    # a quarter turn's half-angle vector: omega = (0, 0, 2) is the unit quaternion (0, 0, 1, 1) / sqrt 2, a rotation by 90 degrees about z
    R, _ = tr.update(np.eye(3), np.zeros(3), np.array([0, 0, 2.0, 0, 0, 0]))
    assert np.allclose(R, np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), atol=1e-15)


# ---- the analytic room -----------------------------------------------------------------------------------------------------

K = synth.REPLICA_640
K80 = synth.Intrinsics(K.fx / 8, K.fy / 8, K.cx / 8, K.cy / 8, 60, 80)
KT = (K80.fx, K80.fy, K80.cx, K80.cy, 60, 80)
NEAR, FAR, GATE = 0.1, 8.0, 0.14


@pytest.fixture(scope="module")
def room():
    scene = synth.replica_room()
    poses = synth.orbit_poses(22)
    t19, q19 = poses[19]
    R19 = synth.quat_to_rot(q19)
    Md, Mn = tr.analytic_model(scene, K80, R19, t19)
    frames = {i: synth.render(scene, K80, *poses[i], depth_scaling=6553.5) for i in (20, 21)}
    return dict(R19=R19, t19=t19, Md=Md, Mn=Mn, frames=frames)


def test_sums_do_not_depend_on_the_pixel_order(room):
    f = room["frames"][20]
    ok, Jt, et = tr.pixel_terms(f.depth, KT, NEAR, FAR, GATE, room["R19"], room["t19"], room["R19"], room["t19"], room["Md"], room["Mn"])
    raster = tr.sums_of(ok, Jt, et)
    assert raster[28] > 2400
    order = np.random.default_rng(0).permutation(ok.size)
    assert np.array_equal(tr.sums_of(ok, Jt, et, order=order), raster)
    assert np.array_equal(tr.sums_of(ok, Jt, et, order=np.arange(ok.size)[::-1]), raster)
    assert np.array_equal(tr.linearise(f.depth, KT, NEAR, FAR, GATE, room["R19"], room["t19"], room["R19"], room["t19"], room["Md"], room["Mn"]), raster)


@pytest.mark.parametrize("target", [20, 21])
def test_analytic_room_pose_from_pose_19(room, target):
    """The restatement measured: pose 19 -> 20 (3.1 cm, 1.8 degrees away) translation error 1.0e-5 m, rotation error below 2e-5
    degrees, 86 % of the pixels associated; pose 19 -> 21 (6.3 cm, 3.6 degrees) 9.1e-6 m, 3.6e-4 degrees, 84 %.  The bounds are
    ten times the prototype's values."""
    f = room["frames"][target]
    out = tr.track(f.depth, KT, NEAR, FAR, GATE, 10, 64, room["R19"], room["t19"], room["Md"], room["Mn"])
    dt, dr = tr.pose_errors(out["R"], out["t"], f.R, f.t)
    print("pose 19 -> %d: translation error %.3g m, rotation error %.3g deg, %d of 4800 pixels, rms %.3g m" % (target, dt, dr, out["pixels"], out["rms"]))
    assert out["status"] == tr.TRACK_OK and out["iterations_done"] == 10
    assert dt <= 1e-4 and dr <= 4e-3, (dt, dr)
    assert out["pixels"] >= 2400


def test_lost_cases_return_the_initial_pose(room):
    f = room["frames"][20]
    R19, t19, Md, Mn = room["R19"], room["t19"], room["Md"], room["Mn"]
    plane_d = np.full((60, 80), 2.0, F)
    plane_n = np.zeros((60, 80, 3), F)
    plane_n[..., 2] = -1.0
    I, z = np.eye(3, dtype=F), np.zeros(3, F)
    cases = [("model of zeros", f.depth, R19, t19, np.zeros_like(Md), Mn, 0),
             ("depth of zeros", np.zeros_like(f.depth), R19, t19, Md, Mn, 0),
             ("one plane", (plane_d * F(1.01)).astype(F), I, z, plane_d, plane_n, 4800)]  # every pixel associates: the pivot gate
    for name, depth, R0, t0, md, mn, pixels in cases:
        out = tr.track(depth, KT, NEAR, FAR, GATE, 10, 64, R0, t0, md, mn)
        assert out["status"] == tr.TRACK_LOST and out["iterations_done"] == 0, name
        assert out["pixels"] == pixels, name
        assert np.array_equal(out["R"], R0) and np.array_equal(out["t"], t0), name
