"""The argument checks of the pybind11 binding (mrhash_amd/csrc/pygeowrapper.cpp), message by message, and the dtype and shape of
every array its newer methods return — on one pinhole wrapper (synth.CFG1, one plane frame, about 100 blocks) and one spherical
wrapper (16 x 64, one small scan).  The messages are the ones the binding raised before its pose parser and its array helpers
replaced the per-method copies."""
import numpy as np
import pytest

import test_raycast_spherical as ts
import test_track_scan as tc
from mrhash_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
T3, Q4 = np.zeros(3, F), np.array([0, 0, 0, 1], F)
T4, Q3 = np.zeros(4, F), np.zeros(3, F)
BOTH = "GeoWrapper::%s|give both t and q, or neither"
SIZES = "GeoWrapper::%s|expected a 3-vector and a 4-vector (qx,qy,qz,qw)"
PINHOLE_ONLY = "GeoWrapper::%s | pinhole cameras only (the camera is spherical)"
SPHERICAL_ONLY = "GeoWrapper::%s | spherical cameras only (the camera is pinhole)"
TRACK_KEYS = {"status", "iterations_done", "pixels", "rms", "sums"}
ALIGN_KEYS = {"status", "iterations_done", "source_blocks", "samples", "accepted", "rms", "pivot", "extent", "sums"}
FUSE_KEYS = {"source_blocks", "candidate_blocks", "records", "valid_voxels", "taken"}
SPH_PARAMS, SPH_CAM = tc.FUSED_PARAMS, synth.spherical_camera(16, 64)
NEAR, FAR = SPH_PARAMS["min_depth"], ts.STREET_MAX


def _pinhole(GeoWrapper):
    K, f = synth.CFG1, synth.cfg1_plane()
    g = GeoWrapper(sdf_truncation=0.06, sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=0.02, n_frames_invalidate_voxels=0,
                   voxel_extents_scale=1, viewer_active=False, marching_cubes_threshold=1.5, min_weight_threshold=5, min_depth=0.01, max_depth=30.0)
    g.setCamera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, 0.01, 30.0, 0)
    g.setCurrPose(f.t, f.q); g.setDepthImage(f.depth); g.setRGBImage(f.rgb); g.compute()
    return g


@pytest.fixture(scope="module")
def wrappers():
    """(pinhole, a second pinhole wrapper with the same map for fuseMap / alignMap, spherical, the plane frame, the scan)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MRHASH_NUM_SDF_BLOCKS", "32768")
        from mrhash.src.pygeowrapper import GeoWrapper

        g, other = _pinhole(GeoWrapper), _pinhole(GeoWrapper)
        p = SPH_PARAMS
        s = GeoWrapper(sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=p["virtual_voxel_size"],
                       n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=1, viewer_active=False,
                       marching_cubes_threshold=p["marching_cubes_threshold"], min_weight_threshold=p["min_weight_threshold"], min_depth=NEAR, max_depth=FAR)
        s.setCamera(*ts.cam_args(SPH_CAM), NEAR, FAR, 1)
        t, q = ts.STREET_POSES[0]
        scan = synth.lidar_scan(synth.street_canyon(), t, q, rows=16, cols=64)
        s.setCurrPose(t, q); s.setPointCloud(scan, False); s.compute()
        yield g, other, s, synth.cfg1_plane(), scan
        del g, other, s


def _raises(msg, call, *args, **kw):
    with pytest.raises(RuntimeError) as ei:
        call(*args, **kw)
    assert str(ei.value) == msg, (str(ei.value), msg)


def _pose_cases(name, call, *args):
    _raises(BOTH % name, call, *args, t=T3)
    _raises(BOTH % name, call, *args, q=Q4)
    _raises(SIZES % name, call, *args, t=T4, q=Q3)


def _is(a, dtype, shape):
    assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == tuple(shape), (a.dtype, a.shape, dtype, shape)


def _check_track(r):
    t, q, info = r
    _is(t, F, (3,)); _is(q, F, (4,))
    assert set(info) == TRACK_KEYS
    _is(info["sums"], np.int64, (32,))
    assert isinstance(info["status"], int) and isinstance(info["iterations_done"], int) and isinstance(info["pixels"], int) and isinstance(info["rms"], float)


def test_pose_arguments_of_the_pinhole_methods(wrappers):
    g, _, _, f, scan = wrappers
    _pose_cases("raycast", g.raycast)
    _pose_cases("trackDepthImage", g.trackDepthImage, f.depth)
    _pose_cases("trackDepthImageSDF", g.trackDepthImageSDF, f.depth)
    # the pose is parsed before the camera model is looked at
    _pose_cases("raycastScan", g.raycastScan)
    _pose_cases("trackPointCloud", g.trackPointCloud, scan)
    for name, call, args in (("raycastScan", g.raycastScan, ()), ("trackPointCloud", g.trackPointCloud, (scan,))):
        _raises(SPHERICAL_ONLY % name, call, *args)
        _raises(SPHERICAL_ONLY % name, call, *args, t=T3, q=Q4)


def test_pose_arguments_of_the_spherical_methods(wrappers):
    _, _, s, f, scan = wrappers
    _pose_cases("raycastScan", s.raycastScan)
    _pose_cases("trackPointCloud", s.trackPointCloud, scan)
    _pose_cases("trackPointCloudSDF", s.trackPointCloudSDF, scan)
    _pose_cases("raycast", s.raycast)
    _pose_cases("trackDepthImage", s.trackDepthImage, f.depth)
    for name, call, args in (("raycast", s.raycast, ()), ("trackDepthImage", s.trackDepthImage, (f.depth,)), ("trackDepthImageSDF", s.trackDepthImageSDF, (f.depth,))):
        _raises(PINHOLE_ONLY % name, call, *args)
        _raises(PINHOLE_ONLY % name, call, *args, t=T3, q=Q4)


def test_the_other_argument_checks(wrappers):
    g, other, _, f, scan = wrappers
    _raises(SIZES % "fuseMap", g.fuseMap, other, T4, Q3)
    _raises(SIZES % "fuseMap", g.fuseMap, other, T3, Q3)
    _raises(SIZES % "alignMap", g.alignMap, other, T4, Q3)
    _raises(SIZES % "alignMap", g.alignMap, other, T4, Q4)
    _raises("GeoWrapper::distanceField|expected two 3-vectors (lo, hi)", g.distanceField, np.zeros(2, F), np.ones(3, F), 0.1)
    _raises("GeoWrapper::distanceField|hi < lo on axis 0", g.distanceField, np.ones(3, F), np.zeros(3, F), 0.1)
    _raises("GeoWrapper::distanceField|hi < lo on axis 2", g.distanceField, np.array([0, 0, 1], F), np.zeros(3, F), 0.1)
    _raises("GeoWrapper::queryPoints|expected points of shape [n, 3]", g.queryPoints, np.zeros((5, 2), F))
    rays = "GeoWrapper::castRays|expected origins and directions of shape [n, 3]"
    _raises(rays, g.castRays, np.zeros((4, 3), F), np.ones((5, 3), F), 2.0)
    _raises(rays, g.castRays, np.zeros((4, 2), F), np.ones((4, 2), F), 2.0)
    _raises("GeoWrapper::castRays|expected tmax of shape [n]", g.castRays, np.zeros((4, 3), F), np.ones((4, 3), F), 2.0, tmax=np.ones(3, F))
    _raises(SIZES % "setCurrPose", g.setCurrPose, T4, Q3)
    _raises(SIZES % "setCurrPose", g.setCurrPose, T3, Q3)
    _raises("GeoWrapper::setCameraInLidar|expected a 4x4 matrix", g.setCameraInLidar, np.zeros(15, F))
    _raises("GeoWrapper::_commInit|the id has 128 bytes", g._commInit, b"\0" * 127, 0, 1)
    _raises("GeoWrapper::_stream|expected a 3-vector", g._stream, np.zeros(2, F), 1.0)
    _raises("GeoWrapper::trackDepthImage|input should be a 2D numpy array", g.trackDepthImage, f.depth.ravel())
    _raises("GeoWrapper::trackDepthImageSDF|input should be a 2D numpy array", g.trackDepthImageSDF, f.depth.ravel())
    _raises("GeoWrapper::trackPointCloudSDF|input should be a 2D numpy array with 3 columns", g.trackPointCloudSDF, scan.ravel())
    assert np.array_equal(g.getCurrPose()[:3, 3], np.asarray(f.t, F))  # no refused call moved the pose


def test_arrays_of_the_pinhole_wrapper(wrappers):
    g, other, _, f, scan = wrappers
    K = synth.CFG1
    H, W = K.rows, K.cols
    _is(g.getCurrPose(), F, (4, 4))
    for im in (g.raycast(), g.raycast(f.t, f.q), g.raycast(t=f.t, q=f.q)):
        assert len(im) == 3
        _is(im[0], F, (H, W)); _is(im[1], F, (H, W, 3)); _is(im[2], np.uint8, (H, W, 3))
    assert np.count_nonzero(g.raycast()[0]) > 0.5 * H * W  # the plane renders
    dist, state, origin, dims = g.distanceField(np.array([-0.1, -0.1, 0.9], F), np.array([0.1, 0.1, 1.1], F), 0.1)
    assert isinstance(origin, tuple) and isinstance(dims, tuple) and len(origin) == len(dims) == 3 and all(isinstance(v, int) for v in origin + dims)
    assert all(10 <= d <= 12 for d in dims)
    _is(dist, F, dims[::-1]); _is(state, np.uint8, dims[::-1])
    for pts in (np.zeros((0, 3), F), np.array([[0, 0, 1.0]] * 7, F), np.zeros(21, F)):
        n = pts.size // 3
        r = g.queryPoints(pts, smooth=True)
        assert len(r) == 4
        _is(r[0], F, (n,)); _is(r[1], F, (n, 3)); _is(r[2], np.uint8, (n, 4)); _is(r[3], np.uint8, (n,))
    for n in (0, 5):
        o, d = np.zeros((n, 3), F), np.tile(np.array([0, 0, 1], F), (n, 1))
        for kw in ({}, {"tmax": np.full(n, 1.5, F), "sensor_frame": True, "normalize": False}):
            r = g.castRays(o, d, 2.0, **kw)
            assert len(r) == 6
            _is(r[0], F, (n,)); _is(r[1], np.uint8, (n,)); _is(r[2], F, (n, 3)); _is(r[3], np.uint8, (n, 3)); _is(r[4], np.uint32, (n, 2)); _is(r[5], F, (n,))
    for r in (g.trackDepthImage(f.depth), g.trackDepthImage(f.depth, f.t, f.q), g.trackDepthImageSDF(f.depth), g.trackDepthImageSDF(f.depth, t=f.t, q=f.q),
              g.trackPointCloudSDF(scan), g.trackPointCloudSDF(scan, f.t, f.q)):
        _check_track(r)
    t, q, info = g.alignMap(other, T3, Q4, iterations=1)
    _is(t, F, (3,)); _is(q, F, (4,))
    assert set(info) == ALIGN_KEYS
    _is(info["pivot"], F, (3,)); _is(info["sums"], np.int64, (32,))
    d = g.fuseMap(other, T3, Q4)
    assert set(d) == FUSE_KEYS and all(isinstance(v, int) for v in d.values()) and d["source_blocks"] > 0


def test_arrays_of_the_spherical_wrapper(wrappers):
    _, _, s, _, scan = wrappers
    H, W = SPH_CAM["rows"], SPH_CAM["cols"]
    t, q = ts.STREET_POSES[0]
    for im in (s.raycastScan(), s.raycastScan(t, q)):
        assert len(im) == 4
        _is(im[0], F, (H, W)); _is(im[1], F, (H, W, 3)); _is(im[2], np.uint8, (H, W, 3)); _is(im[3], F, (H * W, 3))
    for r in (s.trackPointCloud(scan), s.trackPointCloud(scan, t, q), s.trackPointCloudSDF(scan), s.trackPointCloudSDF(scan, t=t, q=q)):
        _check_track(r)
    _is(s.getPointCloud(), F, scan.shape); _is(s.getNormals(), F, (0, 3))
