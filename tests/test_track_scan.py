"""CPU half of scan tracking (include/mrhash_track.h): the restatement (tests/track_scan_ref.py) gives the
hand-derived answers and every rejection, sums that do not depend on the order of the points, the poses of the analytic street and
room, the lost cases, and — on the oracle's street map fused at a 4-voxel truncation and rendered by the restatement of the
spherical raycast — a pose within half a voxel of the true one."""
import ctypes as C

import numpy as np
import pytest

import parity_utils as pu
import raycast_ref as rr
import test_raycast_spherical as ts
import track_scan_ref as sr
from mrhash_amd import capi, synth

F = np.float32
I3, Z3 = np.eye(3, dtype=F), np.zeros(3, F)


def test_track_scan_without_a_context_is_an_invalid_argument(hip):
    p = capi.MrhTrackParams(1.0, 1.0, -0.5, -0.5, 1, 1, 0.1, 4.0, 0.0, 0.0, 0, 0)
    R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (C.c_float * 3)(0, 0, 0)
    oR, ot = (C.c_float * 9)(), (C.c_float * 3)()
    pts = (C.c_float * 3)(2, 1, 0)
    info = capi.MrhTrackInfo()
    assert hip.mrh_track_scan(None, C.byref(p), pts, 1, R, t, oR, ot, C.byref(info)) == capi.MRH_ERR_INVALID_ARG
    assert hip.mrh_track_scan_device(None, C.byref(p), pts, 1, R, t, oR, ot, C.byref(info)) == capi.MRH_ERR_INVALID_ARG


# ---- C1. known answers -------------------------------------------------------------------------------------------------

K1 = (1.0, 1.0, -0.5, -0.5, 1, 1)  # one pixel, one pixel per radian: az = el = 0 is u = v = 0.5


def _one(point, gate=1.0, Mr=2.5, N=(-1, 0, 0), Mp=(2.5, 1, 0)):
    return sr.point_terms(np.array([point], F), K1, 0.1, 4.0, gate, I3, Z3, I3, Z3, np.full((1, 1), Mr, F), np.array([[N]], F), np.array([Mp], F))


def test_one_point_beside_a_wall():
    """A 1 x 1 model with fx = fy = 1, cx = cy = -0.5 at the identity pose and the point p_s = (2, 1, 0): rho_p = sqrt 5, inside
    (0.1, 4]; a = p_w = q = (2, 1, 0); az = atan2(1, 2) = 0.4636, el = asin(0) = 0, so u = (0.4636 - 0.5) + 1 = 0.9636, v = 0.5:
    pixel (0, 0).  The model there is the point M_p = (2.5, 1, 0) with normal (-1, 0, 0): V = (2.5, 1, 0), delta = (0.5, 0, 0),
    |delta|^2 = 0.25 <= 1, e = -0.5.  a x N = (a.y N.z - a.z N.y, a.z N.x - a.x N.z, a.x N.y - a.y N.x) = (0, 0, 1), so
    J = (0, 0, 1, -1, 0, 0).  max_depth = 4: L = 8, S_a = 2048, J~ = (0, 0, 2048, -16384, 0, 0), e~ = -131072."""
    ok, Jt, et = _one((2, 1, 0))
    assert ok.tolist() == [True] and Jt.tolist() == [[0, 0, 2048, -16384, 0, 0]] and et.tolist() == [-131072]
    want = np.zeros(32, np.int64)
    want[11], want[12], want[15] = 2048 * 2048, 2048 * -16384, 16384 * 16384        # H22, H23, H33
    want[23], want[24], want[27], want[28] = 2048 * -131072, 16384 * 131072, 131072 ** 2, 1  # b2, b3, sum e~^2, n
    assert np.array_equal(sr.sums_of(ok, Jt, et), want)


@pytest.mark.parametrize("name, point, kw", [
    ("the distance gate: 0.25 > 0.4^2", (2, 1, 0), dict(gate=0.4)),
    ("beyond max_depth", (4.5, 1, 0), {}),
    ("at min_depth or nearer", (0.05, 0.025, 0), {}),
    ("the missing return", (0, 0, 0), {}),
    ("a NaN", (np.nan, 1, 0), {}),
    ("an infinity", (np.inf, 1, 0), {}),
    ("behind: azimuth pi leaves the one-pixel image", (-2, 0, 0), {}),
    ("a missing model pixel", (2, 1, 0), dict(Mr=0.0)),
    ("a zero normal", (2, 1, 0), dict(N=(0, 0, 0))),
])
def test_each_rejection_gives_a_row_of_zeros_and_no_count(name, point, kw):
    ok, Jt, et = _one(point, **kw)
    assert not ok.any() and not Jt.any() and not et.any(), name
    assert not sr.sums_of(ok, Jt, et).any(), name


def test_the_model_point_is_taken_through_the_render_pose():
    """V = t_r + R_r M_p: with the render pose a quarter turn about z and t_r = (1, 0, 0), the sensor-frame model point (2.5, 1, 0)
    is the world point (1 - 1, 0 + 2.5, 0) = (0, 2.5, 0); the scan point (2, 1, 0) under the same pose is p_w = (0, 2, 0), so
    delta = (0, 0.5, 0).  With N = (0, -1, 0): e = -0.5, a = (-1, 2, 0), a x N = (0, 0, 1)."""
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
    t = np.array([1, 0, 0], F)
    ok, Jt, et = sr.point_terms(np.array([[2, 1, 0]], F), K1, 0.1, 4.0, 1.0, Rz, t, Rz, t, np.full((1, 1), 2.5, F), np.array([[[0, -1, 0]]], F),
                                np.array([[2.5, 1, 0]], F))
    assert ok.tolist() == [True] and Jt.tolist() == [[0, 0, 2048, 0, -16384, 0]] and et.tolist() == [-131072]


# ---- the analytic scenes -----------------------------------------------------------------------------------------------

NEAR, FAR, GATE = 0.2, 60.0, 1.0


def scan_of(scene, t, q, rows, cols, el_deg=(-22.5, 22.5), max_range=FAR):
    """A spinning LiDAR's scan, float32 [rows * cols, 3] in the sensor frame, a missing return (0, 0, 0)."""
    d = synth.lidar_dirs(rows, cols, el_deg)
    rng, _ = scene.cast_dirs(d, synth.quat_to_rot(q), t)
    pts = d * rng[:, None]
    pts[~np.isfinite(rng) | (rng > max_range) | (rng <= 0)] = 0.0
    return pts.astype(F)


def _case(scene, pose_model, pose_scan, model_shape, scan_shape, el_deg=(-22.5, 22.5)):
    cam = synth.spherical_camera(*model_shape, el_deg=el_deg)
    (t0, q0), (t1, q1) = pose_model, pose_scan
    R0 = synth.quat_to_rot(q0)
    Mr, Mn, Mp = sr.analytic_model(scene, cam, R0, t0, max_range=FAR)
    return dict(K=ts.cam_args(cam), R0=R0, t0=np.asarray(t0, F), Mr=Mr, Mn=Mn, Mp=Mp, pts=scan_of(scene, t1, q1, *scan_shape, el_deg=el_deg),
                R1=synth.quat_to_rot(q1), t1=np.asarray(t1, F))


@pytest.fixture(scope="module")
def street_small():
    poses = synth.drive_poses(6)
    return _case(synth.street_canyon(), poses[4], poses[5], (32, 128), (16, 64))


def _track(c, pts=None, **over):
    a = dict(Mr=c["Mr"], Mn=c["Mn"], Mp=c["Mp"])
    a.update(over)
    return sr.track(c["pts"] if pts is None else pts, c["K"], NEAR, FAR, GATE, 10, 64, c["R0"], c["t0"], a["Mr"], a["Mn"], a["Mp"])


def test_sums_do_not_depend_on_the_order_of_the_points(street_small):
    """C2."""
    c = street_small
    args = (c["K"], NEAR, FAR, GATE, c["R0"], c["t0"], c["R0"], c["t0"], c["Mr"], c["Mn"], c["Mp"])
    given = sr.linearise(c["pts"], *args)
    assert given[28] > 256
    perm = np.random.default_rng(0).permutation(len(c["pts"]))
    assert np.array_equal(sr.linearise(c["pts"][perm], *args), given)
    assert np.array_equal(sr.linearise(c["pts"][::-1], *args), given)
    ok, Jt, et = sr.point_terms(c["pts"], *args)
    assert np.array_equal(sr.sums_of(ok, Jt, et, order=perm), given)


# C3: (scene, model pose, scan pose, model, scan, elevation) -> the bounds, ten times what the restatement measured (docstring below)
ANALYTIC = {
    "street 64x512 / 32x512": (lambda: _case(synth.street_canyon(), synth.drive_poses(6)[4], synth.drive_poses(6)[5], (64, 512), (32, 512)), "street_big"),
    "street 32x128 / 16x64": (lambda: _case(synth.street_canyon(), synth.drive_poses(6)[4], synth.drive_poses(6)[5], (32, 128), (16, 64)), "street_small"),
    "room 64x256 / 32x256": (lambda: _case(synth.scannet_room(), synth.walk_poses(36)[30], synth.walk_poses(36)[35], (64, 256), (32, 256), (-45.0, 45.0)), "room"),
}
MEASURED = {  # translation error (m), rotation error (degrees) of the restatement, see the docstring below
    "street_big": (9.11e-7, 1.31e-4),
    "street_small": (2.94e-7, 1.31e-4),
    "room": (1.14e-7, 0.0),
}
R_ULP_DEG = float(np.rad2deg(2.0 ** -24))  # what one rounding of a float32 rotation matrix entry turns the pose by: 3.4e-6 degrees


@pytest.mark.parametrize("name", list(ANALYTIC))
def test_analytic_scenes_converge(name):
    """C3.  The restatement measured (initial -> final, associated points of the last linearisation):
      street, model 64 x 512, scan 32 x 512 (drive_poses 4 -> 5): 0.503 m / 0.277 deg -> 9.11e-7 m / 1.31e-4 deg, 13 321 of 16 384 points
      street, model 32 x 128, scan 16 x 64:                        0.503 m / 0.277 deg -> 2.94e-7 m / 1.31e-4 deg, 627 of 1 024 points
      room (scannet_room, walk poses 30 -> 35, +-45 degrees), model 64 x 256, scan 32 x 256:
                                                                   0.0428 m / 4.90 deg -> 1.14e-7 m / 0 deg (below what
                                                                   pose_errors resolves), 6 669 of 8 192 points
    The bounds are ten times these values, the rotation's no less than ten roundings of a float32 matrix entry (3.4e-5 degrees)."""
    make, key = ANALYTIC[name]
    c = make()
    out = _track(c)
    dt0, dr0 = sr.pose_errors(c["R0"], c["t0"], c["R1"], c["t1"])
    dt, dr = sr.pose_errors(out["R"], out["t"], c["R1"], c["t1"])
    valid = int(np.count_nonzero(np.any(c["pts"] != 0, axis=1)))
    print("%s: translation error %.3g m (initial %.3g), rotation error %.3g deg (initial %.3g), %d of %d points (%d valid), rms %.3g m"
          % (name, dt, dt0, dr, dr0, out["pixels"], len(c["pts"]), valid, out["rms"]))
    assert out["status"] == sr.TRACK_OK and out["iterations_done"] == 10
    mt, mr = MEASURED[key]
    assert dt <= 10 * mt and dr <= 10 * max(mr, R_ULP_DEG), (dt, dr)
    assert out["pixels"] >= 0.5 * valid


def test_lost_cases_return_the_initial_pose(street_small):
    """C4."""
    c = street_small
    # one plane x = 2 seen by the model's pixels within 78 degrees of ahead, the scan 1 % behind it: every point associates
    cam =synth.spherical_camera(32, 128)
    az = (np.arange(128) - cam["cx"] - 0.5) / cam["fx"]
    el = (np.arange(32) - cam["cy"] - 0.5) / cam["fy"]
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (32, 128))], -1)
    ahead = d[..., 0] > 0.2
    plane_r = np.where(ahead, 2.0 / np.where(ahead, d[..., 0], 1.0), 0.0).astype(F)
    plane_p = (plane_r[..., None] * d.astype(F)).astype(F).reshape(-1, 3)
    plane_n = np.where(ahead[..., None], np.array([-1.0, 0.0, 0.0]), 0.0).astype(F)
    plane_scan = (plane_p[ahead.ravel()] * F(1.01)).astype(F)
    cases = [("model of zeros", c["pts"], c["R0"], c["t0"], np.zeros_like(c["Mr"]), c["Mn"], c["Mp"], 0),
             ("scan of (0, 0, 0)", np.zeros_like(c["pts"]), c["R0"], c["t0"], c["Mr"], c["Mn"], c["Mp"], 0),
             ("no points", np.zeros((0, 3), F), c["R0"], c["t0"], c["Mr"], c["Mn"], c["Mp"], 0),
             ("one plane", plane_scan, I3, Z3, plane_r, plane_n, plane_p, len(plane_scan)),  # the pivot gate
             ("normals all zero", c["pts"], c["R0"], c["t0"], c["Mr"], np.zeros_like(c["Mn"]), c["Mp"], 0)]
    for name, pts, R0, t0, Mr, Mn, Mp, pixels in cases:
        out = sr.track(pts, c["K"], NEAR, FAR, GATE, 10, 64, R0, t0, Mr, Mn, Mp)
        assert out["status"] == sr.TRACK_LOST and out["iterations_done"] == 0, name
        assert out["pixels"] == pixels, (name, out["pixels"], pixels)
        assert np.array_equal(out["R"], np.asarray(R0, F)) and np.array_equal(out["t"], np.asarray(t0, F)), name
        if name == "no points":
            assert not out["sums"].any() and out["rms"] == 0.0


# ---- C5. the fused map -------------------------------------------------------------------------------------------------

FUSED_PARAMS = dict(ts.STREET_PARAMS, sdf_truncation=0.8)  # 4 voxels: the ground renders
FUSED_CAM = synth.spherical_camera(32, 128)
FUSED_OFFSET = (np.array([0.4, 0.3, 0.1]), np.deg2rad([2.0, 1.0, -1.0]))  # metres in the world frame; yaw, pitch, roll


def fused_true_pose():
    """STREET_POSES[-1] moved by FUSED_OFFSET: (R, t, q) of the pose the scan is taken from."""
    t0, q0 = ts.STREET_POSES[-1]
    yaw, pitch, roll = FUSED_OFFSET[1]
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    R = synth.quat_to_rot(q0).astype(np.float64) @ Rz @ Ry @ Rx
    return R, np.asarray(t0, np.float64) + FUSED_OFFSET[0]


def fused_scan(rows=16, cols=64):
    """The rows x cols analytic scan from fused_true_pose()."""
    R, t = fused_true_pose()
    d = synth.lidar_dirs(rows, cols)
    rng, _ = synth.street_canyon().cast_dirs(d, R, t)
    pts = d * rng[:, None]
    pts[~np.isfinite(rng) | (rng > ts.STREET_MAX) | (rng <= 0)] = 0.0
    return pts.astype(F)


def check_fused(out, n_valid):
    """The conditions of C5 and G11; returns (translation error, rotation error)."""
    R0, t0 = synth.quat_to_rot(ts.STREET_POSES[-1][1]), ts.STREET_POSES[-1][0]
    R1, t1 = fused_true_pose()
    dt0, dr0 = sr.pose_errors(R0, t0, R1, t1)
    dt, dr = sr.pose_errors(out["R"], out["t"], R1, t1)
    print("fused street: translation error %.4g m (initial %.4g), rotation error %.4g deg (initial %.4g), %d of %d valid points, rms %.4g m"
          % (dt, dt0, dr, dr0, out["pixels"], n_valid, out["rms"]))
    assert out["status"] == sr.TRACK_OK and out["iterations_done"] == 10
    assert out["pixels"] >= 0.5 * n_valid, (out["pixels"], n_valid)
    assert dt < 0.5 * dt0 and dt < 0.1, (dt, dt0)  # half a 20 cm voxel
    assert dr < 0.5 * dr0, (dr, dr0)
    return dt, dr


def test_fused_street_map_on_the_cpu():
    """C5.  The oracle's map of the five street scans at sdf_truncation = 0.8, rendered 32 x 128 by tests/raycast_sph_ref.py at
    STREET_POSES[-1]; the 16 x 64 analytic scan from that pose moved by (0.4, 0.3, 0.1) m and turned by yaw 2, pitch 1 and roll -1
    degrees.  The restatement measured: 81.3 % of the model's pixels hit and 69.5 % carry a normal; 624 of the 996 valid points
    associated (0.627); 0.5099 m / 2.457 degrees -> 0.02984 m / 0.4083 degrees, rms 4.04 cm, all ten updates applied.  The
    rotation floor is the map's (20 cm voxels under 2.8 degree model pixels), not the solver's."""
    e = ts.fuse_street(pu.oracle_lib(), FUSED_PARAMS)
    d, v = e.dump_blocks()
    e.close()
    t0, q0 = ts.STREET_POSES[-1]
    R0 = synth.quat_to_rot(q0)
    r, c = np.mgrid[0:FUSED_CAM["rows"], 0:FUSED_CAM["cols"]]
    Mr, Mn, _, Mp = ts.street_raycaster(rr.make_map(FUSED_PARAMS, d, v), FUSED_PARAMS, FUSED_CAM, R0, t0).render(r, c)
    print("model: %.3f of the pixels hit, %.3f carry a normal" % (np.count_nonzero(Mr) / Mr.size, np.count_nonzero(np.any(Mn != 0, axis=-1)) / Mr.size))
    pts = fused_scan()
    gate, its, min_points = sr.defaults(0.0, 0, 0, FUSED_PARAMS["sdf_truncation"])
    out = sr.track(pts, ts.cam_args(FUSED_CAM), FUSED_PARAMS["min_depth"], ts.STREET_MAX, gate, its, min_points, R0, t0, Mr, Mn, Mp)
    check_fused(out, int(np.count_nonzero(np.any(pts != 0, axis=1))))
