"""GPU half of scan tracking (k_track_scan_linearise in mrh_track.h, include/mrhash_track.h) on the street fused
through the C ABI at a 4-voxel truncation: bit-exact against the restatement of tests/track_scan_ref.py fed with the library's own
spherical render (whose parity the raycast tests pin) — sums, pose, status, count and rms; the known answer of a rendered scan
registered against its own pose; ragged, dirty and shuffled clouds; the device variant; no side effects on the frame and point
paths; the argument checks; the GeoWrapper facade; and the accuracy conditions of the CPU half on the GPU's map."""
import ctypes as C

import numpy as np
import pytest

import parity_utils as pu
import test_raycast_spherical as ts
import test_track_scan as tc
import track_scan_ref as sr
from mrhash_amd import capi, hipmem, synth

pytestmark = pytest.mark.gpu

PARAMS = tc.FUSED_PARAMS
CAM = tc.FUSED_CAM                       # the 32 x 128 model
CAM_BIG = ts.STREET_CAM                  # 64 x 512
NEAR, FAR = PARAMS["min_depth"], ts.STREET_MAX
T_LAST = np.asarray(ts.STREET_POSES[-1][0], np.float32)
R_LAST = synth.quat_to_rot(ts.STREET_POSES[-1][1]).astype(np.float32)
F = np.float32


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _model(e, cam, R0=R_LAST, t0=T_LAST):
    Mr, Mn, _, Mp = e.raycast_spherical(*ts.cam_args(cam), R0, t0, NEAR, FAR, colors=False, points=True)
    return Mr, Mn, Mp


def _reference(e, params, cam, pts, iterations, R0=R_LAST, t0=T_LAST):
    """tests/track_scan_ref.py on the GPU's own render from (R0, t0)."""
    gate, its, min_points = sr.defaults(0.0, iterations, 0, params["sdf_truncation"])
    return sr.track(pts, ts.cam_args(cam), NEAR, FAR, gate, its, min_points, R0, t0, *_model(e, cam, R0, t0))


def _track(e, cam, pts, iterations=0, R0=R_LAST, t0=T_LAST, **kw):
    return e.track_scan(pts, *ts.cam_args(cam), R0, t0, NEAR, FAR, iterations=iterations, **kw)


def _assert_bit_exact(got, want):
    R, t, info = got
    assert np.array_equal(info["sums"], want["sums"]), (info["sums"], want["sums"])
    assert info["pixels"] == want["pixels"] and info["iterations_done"] == want["iterations_done"] and info["status"] == want["status"]
    assert _same_bits(R, want["R"]) and _same_bits(t, want["t"]), (R, want["R"], t, want["t"])
    assert np.float64(info["rms"]).tobytes() == np.float64(want["rms"]).tobytes(), (info["rms"], want["rms"])


@pytest.fixture(scope="module")
def street():
    e = ts.fuse_street(capi.load_hip(), PARAMS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scan():
    return tc.fused_scan()  # 16 x 64: four workgroups


# ---- G1 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [1, 2, 10])
def test_bit_exact_32x128_model_16x64_scan(street, scan, iterations):
    got = _track(street, CAM, scan, iterations)
    _assert_bit_exact(got, _reference(street, PARAMS, CAM, scan, iterations))
    assert got[2]["status"] == capi.TRACK_OK and got[2]["iterations_done"] == iterations and got[2]["pixels"] >= 0.5 * 996


# ---- G2 ---------------------------------------------------------------------------------------------------------------

# synth.spherical_camera puts column 0 half a pixel beyond azimuth -pi (az = -(cx + 0.5) / fx = -pi - pi / cols).  mrh_atan2f
# returns (-pi, pi], so a point on that column's ray comes back at +pi - pi / cols, u = cols + 0.5, and leaves the image: D13 and
# D15 have no azimuth wrap.  With cx one pixel smaller every column looks inside (-pi, pi) and every model point finds its pixel.
CAM_INSIDE = dict(CAM, cx=CAM["cx"] - 1.0)


@pytest.mark.parametrize("cam, seam_columns", [(CAM_INSIDE, 0), (CAM, 1)], ids=["every column inside (-pi, pi)", "column 0 beyond -pi"])
def test_a_rendered_scan_registers_against_its_own_pose_with_zero_residual(street, cam, seam_columns):
    """V = t_r + R_r M_p and p_w = R32 p_s + t32 are the same IEEE expression when p_s is the model's own point and the pose is the
    render's: every residual is exactly 0, b = 0, the step is 0 and the pose comes back bit for bit.  n is the number of model
    pixels with a non-zero normal — less those of a column beyond the seam, whose points do not wrap back into the image."""
    n = cam["rows"] * cam["cols"]
    dr, dp = hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n)
    street.raycast_spherical_device(*ts.cam_args(cam), R_LAST, T_LAST, NEAR, FAR, d_range=dr.ptr, d_points=dp.ptr)
    street.sync()
    R, t, info = street.track_scan_device(dp.ptr, n, *ts.cam_args(cam), R_LAST, T_LAST, NEAR, FAR)
    _, Mn, _ = _model(street, cam)
    has_normal = np.any(Mn != 0, axis=-1)
    assert np.count_nonzero(has_normal) > 0.5 * n
    if seam_columns:
        assert has_normal[:, :seam_columns].any()
    assert info["pixels"] == np.count_nonzero(has_normal[:, seam_columns:])
    assert not info["sums"][21:28].any() and info["rms"] == 0.0
    assert info["status"] == capi.TRACK_OK and info["iterations_done"] == 10
    assert _same_bits(R, R_LAST) and _same_bits(t, T_LAST)


# ---- G3 ---------------------------------------------------------------------------------------------------------------

def test_a_dirty_cloud_of_1000_points(street, scan):
    pts = scan[:1000].copy()
    pts[5] = np.nan
    pts[300, 1] = np.nan
    pts[301, 0] = np.inf
    pts[640] = -np.inf
    pts[700:716] = 0.0
    got = _track(street, CAM, pts, 3)
    _assert_bit_exact(got, _reference(street, PARAMS, CAM, pts, 3))
    assert got[2]["status"] == capi.TRACK_OK and got[2]["pixels"] >= 400


def test_257_points_the_second_workgroup_has_one_live_lane(street, scan):
    valid = scan[np.any(scan != 0, axis=1)]
    pts = valid[::3][:257]
    got = _track(street, CAM, pts, 3)
    want = _reference(street, PARAMS, CAM, pts, 3)
    _assert_bit_exact(got, want)
    assert got[2]["pixels"] >= 64
    # the last point alone is what the second workgroup adds
    first = _track(street, CAM, pts[:256], 1)
    both = _track(street, CAM, pts, 1)
    last = sr.linearise(pts[256:], ts.cam_args(CAM), NEAR, FAR, sr.defaults(0.0, 0, 0, PARAMS["sdf_truncation"])[0], R_LAST, T_LAST, R_LAST, T_LAST,
                        *_model(street, CAM))
    assert np.array_equal(both[2]["sums"], first[2]["sums"] + last)


def test_one_point_is_lost_by_min_points(street, scan):
    pts = scan[np.any(scan != 0, axis=1)][500:501]
    R, t, info = _track(street, CAM, pts)
    _assert_bit_exact((R, t, info), _reference(street, PARAMS, CAM, pts, 0))
    assert info["status"] == capi.TRACK_LOST and info["iterations_done"] == 0 and info["pixels"] <= 1
    assert _same_bits(R, R_LAST) and _same_bits(t, T_LAST)


def test_no_points_is_lost_and_leaves_the_pose(street):
    R, t, info = _track(street, CAM, np.zeros((0, 3), F))
    assert info["status"] == capi.TRACK_LOST and info["iterations_done"] == 0 and info["pixels"] == 0 and info["rms"] == 0.0
    assert not info["sums"].any() and _same_bits(R, R_LAST) and _same_bits(t, T_LAST)


# ---- G4 ---------------------------------------------------------------------------------------------------------------

def test_a_shuffled_cloud_gives_the_same_sums_and_pose(street, scan):
    want = _track(street, CAM, scan, 4)
    got = _track(street, CAM, scan[np.random.default_rng(1).permutation(len(scan))], 4)
    assert np.array_equal(got[2]["sums"], want[2]["sums"]) and got[2]["pixels"] == want[2]["pixels"] and got[2]["rms"] == want[2]["rms"]
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


# ---- G5 ---------------------------------------------------------------------------------------------------------------

def test_bit_exact_64x512_model_32x512_scan(street):
    """64 rows of the partial slab."""
    pts = tc.fused_scan(32, 512)
    got = _track(street, CAM_BIG, pts, 2)
    _assert_bit_exact(got, _reference(street, PARAMS, CAM_BIG, pts, 2))
    assert got[2]["status"] == capi.TRACK_OK and got[2]["pixels"] >= 0.5 * np.count_nonzero(np.any(pts != 0, axis=1))


# ---- G6 ---------------------------------------------------------------------------------------------------------------

def test_bit_exact_on_a_variance_adaptive_map(scan):
    params = dict(PARAMS, sdf_var_threshold=0.05)
    e = ts.fuse_street(capi.load_hip(), params)
    try:
        assert e.stats().occupied_coarse > 0
        got = _track(e, CAM, scan, 2)
        _assert_bit_exact(got, _reference(e, params, CAM, scan, 2))
        assert got[2]["pixels"] >= 64
    finally:
        e.close()


# ---- G7 ---------------------------------------------------------------------------------------------------------------

def test_device_variant_equals_the_host_call(street, scan):
    want = _track(street, CAM, scan, 3)
    buf = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(scan, F))
    got = street.track_scan_device(buf.ptr, len(scan), *ts.cam_args(CAM), R_LAST, T_LAST, NEAR, FAR, iterations=3)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    assert np.array_equal(got[2]["sums"], want[2]["sums"]) and got[2]["rms"] == want[2]["rms"] and got[2]["status"] == want[2]["status"]


# ---- G8 ---------------------------------------------------------------------------------------------------------------

def test_tracking_leaves_the_map_the_current_scan_and_the_frame_path_alone(scan):
    hip = capi.load_hip()
    scene = synth.street_canyon()
    poses = synth.drive_poses(8, step=1.0)
    frames = [(synth.quat_to_rot(q), t, *synth.spherical_range_image(scene, t, q, CAM_BIG)) for t, q in poses]
    a, b = (capi.Engine(hip, capi.Params(num_sdf_blocks=131072, **PARAMS)) for _ in range(2))

    def feed(e, f):
        e.set_pose(f[0], f[1])
        e.upload_depth(f[2])
        e.upload_rgb(f[3])
        assert not e.integrate()

    try:
        for e in (a, b):
            e.set_camera(*ts.cam_args(CAM_BIG), NEAR, FAR, model=1)
        for i, f in enumerate(frames[:5]):
            if i:  # between every two pipelined frames, no sync in between
                _track(a, CAM, scan, 2, R0=frames[i - 1][0], t0=frames[i - 1][1])
            feed(a, f)
            feed(b, f)
        r = pu.compare_maps(a, b, tol=0.0)
        assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
        # the last extraction, the stats and the current scan of an engine that tracks against one that never did
        nxt = synth.lidar_scan(scene, *poses[5], rows=16, cols=64)
        for e in (a, b):
            e.extract_triangles()
            e.set_scan_layout(64)
            e.set_pose(frames[5][0], frames[5][1])
            e.upload_points(nxt)
        tris = a.extract_triangles()
        V, Fc, Cc = a.extract_mesh()
        a.stats()  # the per-call differences refer to the previous call
        d0, v0 = a.dump_blocks()
        s0 = a.stats()
        _track(a, CAM, scan)  # another cloud than the one uploaded
        s1 = a.stats()
        d1, v1 = a.dump_blocks()
        V2, F2, C2 = a.extract_mesh()
        assert np.array_equal(d0, d1) and _same_bits(v0, v1)
        assert _same_bits(V, V2) and np.array_equal(Fc, F2) and _same_bits(Cc, C2)
        for name, _ in capi.MrhStats._fields_:
            if "ms" not in name:
                assert getattr(s0, name) == getattr(s1, name), name
        b.extract_triangles()
        for e in (a, b):
            assert not e.integrate_points()
            e.sync()
        r = pu.compare_maps(a, b, tol=0.0)
        assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
        assert _same_bits(a.extract_triangles(), b.extract_triangles()) and len(tris) > 0
    finally:
        a.close()
        b.close()


# ---- G9 ---------------------------------------------------------------------------------------------------------------

def test_arguments_and_sharded_context(street, scan):
    hip = capi.load_hip()
    for over in (dict(dist_max=1.5), dict(dist_max=-0.1), dict(iterations=65), dict(iterations=-1), dict(step=-0.01)):
        with pytest.raises(capi.MrhError) as ei:
            _track(street, CAM, scan, **{"iterations": 0, **over})
        assert ei.value.code == capi.MRH_ERR_INVALID_ARG, over
    with pytest.raises(capi.MrhError) as ei:
        street.track_scan(scan, *ts.cam_args(CAM), R_LAST, T_LAST, FAR, NEAR)
    assert ei.value.code == capi.MRH_ERR_INVALID_ARG
    # beyond the domain of the sine and cosine (8192 rad): the first column's azimuth (256.5 / 0.03 = 8550 rad), the rows' elevations
    for over in (dict(fx=0.03), dict(fy=1e-4)):
        cam = dict(CAM_BIG, **over)
        with pytest.raises(capi.MrhError) as ei:
            _track(street, cam, scan)
        assert ei.value.code == capi.MRH_ERR_INVALID_ARG, over
    # null pointers and more than 2^24 points, through the raw entry points
    p = capi.MrhTrackParams(*ts.cam_args(CAM), NEAR, FAR, 0.0, 0.0, 0, 0)
    Fp = C.POINTER(C.c_float)
    R, t = R_LAST.ravel().copy(), T_LAST.copy()
    oR, ot, info = np.zeros(9, F), np.zeros(3, F), capi.MrhTrackInfo()
    pts = np.ascontiguousarray(scan, F)
    ok = [street._ctx, C.byref(p), pts.ctypes.data, len(pts), R.ctypes.data_as(Fp), t.ctypes.data_as(Fp), oR.ctypes.data_as(Fp), ot.ctypes.data_as(Fp), C.byref(info)]
    for fn in (hip.mrh_track_scan, hip.mrh_track_scan_device):
        for null in (1, 2, 4, 5, 6, 7):
            args = list(ok)
            args[null] = None
            assert fn(*args) == capi.MRH_ERR_INVALID_ARG, (fn.__name__, null)
        args = list(ok)
        args[3] = (1 << 24) + 1  # refused before the cloud is read: the pointer covers 1 024 points only
        assert fn(*args) == capi.MRH_ERR_INVALID_ARG, fn.__name__
    assert hip.mrh_track_scan(*ok[:8], None) == capi.MRH_OK  # out_info may be NULL
    s = capi.Engine(hip, capi.Params(num_sdf_blocks=4096, shard_rank=0, shard_count=2, **PARAMS))
    try:
        with pytest.raises(capi.MrhError) as ei:
            _track(s, CAM, scan)
        assert ei.value.code == capi.MRH_ERR_UNSUPPORTED
    finally:
        s.close()


# ---- G10 --------------------------------------------------------------------------------------------------------------

def test_geowrapper_track_point_cloud(street, scan, monkeypatch):
    monkeypatch.setenv("MRHASH_NUM_SDF_BLOCKS", "131072")
    from mrhash.src.pygeowrapper import GeoWrapper

    p = PARAMS
    g = GeoWrapper(sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=p["virtual_voxel_size"],
                   n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=1, viewer_active=False,
                   marching_cubes_threshold=p["marching_cubes_threshold"], min_weight_threshold=p["min_weight_threshold"], min_depth=NEAR, max_depth=FAR)
    try:
        with pytest.raises(RuntimeError):
            g.trackPointCloud(scan)  # no camera yet
        g.setCamera(*ts.cam_args(CAM_BIG), NEAR, FAR, 1)
        scene = synth.street_canyon()
        for t, q in ts.STREET_POSES:
            depth, rgb = synth.spherical_range_image(scene, t, q, CAM_BIG)
            g.setCurrPose(t, q)
            g.setDepthImage(depth)
            g.setRGBImage(rgb)
            g.compute()
        pose = g.getCurrPose().copy()
        R0, t0 = pose[:3, :3].astype(F), pose[:3, 3].astype(F)
        want = _track(street, CAM_BIG, scan, R0=R0, t0=t0)
        assert want[2]["status"] == capi.TRACK_OK and want[2]["pixels"] >= 0.5 * 996
        for t, q, info in (g.trackPointCloud(scan), g.trackPointCloud(scan, *ts.STREET_POSES[-1])):
            assert _same_bits(np.asarray(t, F), want[1])
            assert np.array_equal(np.asarray(info["sums"]), want[2]["sums"]) and info["status"] == capi.TRACK_OK and info["iterations_done"] == 10
            assert info["pixels"] == want[2]["pixels"] and info["rms"] == want[2]["rms"]
            q = np.asarray(q, np.float64)
            assert abs(np.linalg.norm(q) - 1.0) <= 1e-6 and q[3] >= 0
            assert np.abs(synth.quat_to_rot(q).astype(np.float64) - want[0]).max() <= 1e-6
        assert np.array_equal(g.getCurrPose(), pose)  # the current pose is the caller's to set
        g.setCamera(100.0, 100.0, 3.5, 3.5, 8, 8, NEAR, FAR, 0)
        with pytest.raises(RuntimeError):
            g.trackPointCloud(scan)
    finally:
        del g


# ---- G11 --------------------------------------------------------------------------------------------------------------

def test_accuracy_on_the_fused_map(street, scan):
    """The conditions of test_track_scan.test_fused_street_map_on_the_cpu on the GPU's map, and the bits of the restatement fed
    with the GPU's render.  The first run on the MI355X measured what the CPU half measures on the oracle's map, digit for digit:
    0.5099 m / 2.457 degrees -> 0.02984 m / 0.4083 degrees, 624 of 996 valid points associated, rms 4.043 cm."""
    R, t, info = _track(street, CAM, scan)
    want = _reference(street, PARAMS, CAM, scan, 0)
    _assert_bit_exact((R, t, info), want)
    tc.check_fused(dict(info, R=R, t=t), int(np.count_nonzero(np.any(scan != 0, axis=1))))


# ---- G12 --------------------------------------------------------------------------------------------------------------

def test_depth_images_and_scans_share_one_staging_pair(street, scan):
    """A host observation of either kind goes through one pinned and one device staging buffer, sized in floats (stage_obs).  On
    one context: track_depth on an 80 x 60 image (4 800 floats), track_scan with the 16 x 64 scan (3 072 floats: the pair is reused
    at a smaller size), track_scan with a 32 x 512 scan (49 152 floats: it grows), track_depth again (after a larger scan: reused at a
    smaller size, over what the cloud left behind), track_scan_device (no staging).  Every pose and its 32 sums equal, bit for
    bit, what a context that has made no other call returns.

    Two more users share that state (mrh_ctx::Stage and ::Fit).  Between the big cloud and the second depth image a host point
    query stages the scan's valid points (under 3 000 floats, over what the 49 152 of the cloud left) — its four outputs are
    compared; the depth image after it reuses the pair again.  Between the second depth image and the device scan a registration
    with this context as the destination reduces more than 8 192 accepted samples through the slab and the pinned sums that
    tracking uses: more than the 32 rows one stripe pass of k_track_finish covers and than the 20 rows of the 80 x 60 image, so
    the tracking call after it reuses the slab at a smaller row count.  Its source is a second context that imported this one's
    blocks; the fresh side is a fresh pair."""
    hip = capi.load_hip()
    scene = synth.street_canyon()
    frames = [(synth.quat_to_rot(q), t, *synth.spherical_range_image(scene, t, q, CAM_BIG)) for t, q in ts.STREET_POSES]

    def fresh():
        e = capi.Engine(hip, capi.Params(num_sdf_blocks=131072, **PARAMS))
        e.set_camera(*ts.cam_args(CAM_BIG), NEAR, FAR, model=1)
        for R, t, depth, rgb in frames:
            e.set_pose(R, t)
            e.upload_depth(depth)
            e.upload_rgb(rgb)
            assert not e.integrate()
        return e

    # the pinhole camera looks along the sensor's x axis (camera z forward, x right, y down), 80 x 60 pixels, 90 degrees wide
    pin = (40.0, 40.0, 39.5, 29.5, 60, 80)
    R_pin = (R_LAST @ np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], F)).astype(F)
    image, _, _ = street.raycast(*pin, R_pin, (T_LAST + np.array([0.2, 0.1, 0.05], F)).astype(F), NEAR, FAR, colors=False)
    big = tc.fused_scan(32, 512)
    dev = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(scan, F))
    walls = scan[np.any(scan != 0, axis=1)]  # sensor-frame points on the street's surfaces, about 1 000
    assert 900 <= len(walls) <= 1024
    blocks = street.dump_blocks()

    def source():
        s = capi.Engine(hip, capi.Params(num_sdf_blocks=131072, **PARAMS))
        s.import_blocks(*blocks)
        return s

    street_source = source()

    def register(e):  # a few centimetres off the identity, cropped to a cube around the sensor
        s = street_source if e is street else source()
        try:
            return e.align_map(s, np.eye(3, dtype=F), np.array([0.03, -0.02, 0.01], F), iterations=2, pivot=T_LAST, extent=8.0)
        finally:
            if s is not street_source:
                s.close()

    calls = [lambda e: e.track_depth(image, *pin, R_pin, T_LAST, NEAR, FAR, iterations=3),
             lambda e: _track(e, CAM, scan, 3),
             lambda e: _track(e, CAM, big, 1),
             lambda e: e.query(walls, R_LAST, T_LAST),
             lambda e: e.track_depth(image, *pin, R_pin, T_LAST, NEAR, FAR, iterations=3),
             register,
             lambda e: e.track_scan_device(dev.ptr, len(scan), *ts.cam_args(CAM), R_LAST, T_LAST, NEAR, FAR, iterations=3)]
    try:
        for i, call in enumerate(calls):
            got = call(street)
            e = fresh()
            try:
                want = call(e)
            finally:
                e.close()
            if call is calls[3]:  # the query: dist, grad, rgbw, state
                print("call %d: %d of %d points have a distance" % (i, np.count_nonzero(got[3] & capi.QUERY_DIST), len(walls)))
                assert all(_same_bits(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 4, i
                assert np.count_nonzero(got[3] & capi.QUERY_DIST) >= 64, i  # the points took part
                continue
            count = "accepted" if call is register else "pixels"
            print("call %d: status %d, %d iterations, %d %s" % (i, got[2]["status"], got[2]["iterations_done"], got[2][count], count))
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), i
            assert np.array_equal(got[2]["sums"], want[2]["sums"]) and got[2]["status"] == want[2]["status"], i
            assert got[2].keys() == want[2].keys()
            for key in got[2]:  # iterations_done, the counts, rms and, for the registration, pivot and extent
                assert _same_bits(np.asarray(got[2][key]), np.asarray(want[2][key])), (i, key)
            assert got[2][count] >= 64, i  # the observation took part
            if call is register:
                assert got[2]["accepted"] > 8192 and got[2]["iterations_done"] >= 1, got[2]
    finally:
        street_source.close()
