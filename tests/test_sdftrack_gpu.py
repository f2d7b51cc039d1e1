"""GPU half of render-free tracking (mrh_sdftrack.h, include/mrhash_sdftrack.h): every output of mrh_track_depth_sdf and
mrh_track_points_sdf bit for bit against the restatement of tests/sdftrack_ref.py — pose, status, iterations, count, rms and all 32
sums — on the hand-built maps whose coverage tests/test_sdftrack.py asserts; end to end on a fused map with the reader contract;
every refusal; the facade.  Maps are imported, not fused, unless said otherwise."""
import ctypes as C

import numpy as np
import pytest

import align_ref as ar
import esdf_ref as er
import parity_utils as pu
import remap_ref as rm
import sdftrack_ref as sr
import test_sdftrack as tsd
import track_ref as tr
from mrhash_amd import capi, hipmem, synth

pytestmark = pytest.mark.gpu

F = np.float32
NEAR, FAR = sr.VIEW_NEAR, sr.VIEW_FAR


def _engine(blocks, params, num_sdf_blocks=4096):
    e = pu.make_engine(capi.load_hip(), synth.CFG1, params, num_sdf_blocks)
    if blocks:
        e.import_blocks(*er.to_import(blocks))
    return e


def _result(R, t, info):
    return dict(info, R=R, t=t)


def _assert_same(got, want, what):
    bad = sr.same_result(got, want)
    assert not bad, f"{what}: {bad} differ: " + "; ".join(f"{k}: {got[k]} vs {want[k]}" for k in bad)


class Dest:
    """An engine on the imported map of a destination of sdftrack_ref, and the restatement's lookup structure of the same map."""

    def __init__(self, name):
        self.name, self.s = name, sr.destination(name)
        self.e = _engine(self.s["blocks"], self.s["params"])
        self.m = rm.Source(self.s["params"], self.s["blocks"])

    def depth(self, depth, K, R, t, what=None, **kw):
        want = sr.track_depth(self.s["params"], self.m, depth, K, NEAR, FAR, R, t, **kw)
        got = _result(*self.e.track_depth_sdf(depth, *K, R, t, NEAR, FAR, **kw))
        print(what or self.name, {k: got[k] for k in ("status", "iterations_done", "pixels", "rms")})
        _assert_same(got, want, what or self.name)
        return got

    def points(self, pts, R, t, what=None, **kw):
        want = sr.track_points(self.s["params"], self.m, pts, NEAR, FAR, R, t, **kw)
        got = _result(*self.e.track_points_sdf(pts, R, t, NEAR, FAR, **kw))
        print(what or self.name, {k: got[k] for k in ("status", "iterations_done", "pixels", "rms")})
        _assert_same(got, want, what or self.name)
        return got

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def corner():
    """The corner destination; the view and the start are given per call."""
    d = Dest("truth")
    yield d
    d.close()


def _cloud(s):
    """The corner view's valid pixels as a sensor-frame cloud."""
    valid, p = sr.depth_samples(s["depth"], s["K"], NEAR, FAR)
    return p[valid]


# ---- 1. the corner view ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [1, 10, 64])
@pytest.mark.parametrize("start", ["truth", "start"])
def test_corner_view(corner, start, iterations):
    s = corner.s
    R0, t0 = (s["R"], s["t"]) if start == "start" else (s["R_true"], s["t_true"])
    got = corner.depth(s["depth"], s["K"], R0, t0, f"{start}, {iterations} iterations", iterations=iterations)
    assert got["status"] == capi.TRACK_OK and got["iterations_done"] == iterations and got["pixels"] == 3072  # twelve rows of the slab
    cloud = corner.points(_cloud(s), R0, t0, f"{start}, {iterations} iterations, as a cloud", iterations=iterations)
    _assert_same(cloud, got, "the points form on the pixels' p_c")
    if iterations >= 10:
        t_err, deg = tr.pose_errors(got["R"], got["t"], s["R_true"], s["t_true"])
        print(f"{start}: {deg:.5f} deg, {1e3 * t_err:.3f} mm, rms {got['rms']:.7f}")
        assert deg <= 2 * tsd.VIEW_DEG and t_err <= 2 * tsd.VIEW_T_ERR and got["rms"] <= 2 * tsd.VIEW_RMS


# ---- 2. image shapes and point counts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows, cols", [(1, 1), (1, 257), (17, 19), (33, 65)])
def test_image_shapes(corner, rows, cols):
    """Partial tiles, one slab row and many (17 workgroups in a line, 3 x 5 of them): the corner seen through a camera of that shape."""
    s = corner.s
    f = 0.9 * max(rows, cols)
    K = (f, f, cols / 2.0, rows / 2.0, rows, cols)
    depth = sr.corner_depth(s["R_true"], s["t_true"], K)
    assert np.count_nonzero(depth) == rows * cols
    got = corner.depth(depth, K, s["R"], s["t"], f"{rows} x {cols}", iterations=2, min_pixels=1)
    if rows * cols == 1:
        assert got["status"] == capi.TRACK_LOST and got["pixels"] == 1  # one row cannot fix six unknowns: the pivot gate
    else:
        assert got["status"] == capi.TRACK_OK and got["pixels"] >= 0.5 * rows * cols


@pytest.mark.parametrize("k", [1, 255, 256, 257])
def test_point_counts_around_one_workgroup(corner, k):
    """One linearisation of k points spread over the view; lost where the solve says so (a single point)."""
    s = corner.s
    cloud = _cloud(s)
    pts = cloud[np.linspace(0, len(cloud) - 1, k).astype(int)] if k > 1 else cloud[1500:1501]
    got = corner.points(pts, s["R"], s["t"], f"{k} points", iterations=1, min_points=1)
    assert got["pixels"] == k
    assert got["status"] == (capi.TRACK_LOST if k == 1 else capi.TRACK_OK)


# ---- 3. the destinations -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["adaptive_dst", "holes_dst", "far", "beyond", "plane", "narrow_band", "steep"])
def test_destination(name):
    d = Dest(name)
    try:
        s = d.s
        if name == "adaptive_dst":
            desc, _ = d.e.dump_blocks()
            assert 0 < int((desc["resolution"] == 1).sum()) < len(desc)
        for iterations in (2, 10):
            got = d.depth(s["depth"], s["K"], s["R"], s["t"], f"{name}, {iterations} iterations", iterations=iterations, **s["kw"])
            _assert_same(d.points(_cloud(s), s["R"], s["t"], iterations=iterations, **s["kw"]), got, "as a cloud")
            if name in sr.LOST:
                assert got["status"] == capi.TRACK_LOST and got["iterations_done"] == 0
                assert rm.same_bits(got["R"], s["R"]) and rm.same_bits(got["t"], s["t"])
                assert got["pixels"] == (0 if name == "beyond" else 192)
            else:
                assert got["status"] == capi.TRACK_OK and got["pixels"] >= 64
        if name == "far":
            assert np.abs(s["t"]).min() > 26000.0
    finally:
        d.close()


def test_min_pixels_above_the_count_is_lost(corner):
    s = corner.s
    got = corner.depth(s["depth"], s["K"], s["R"], s["t"], min_pixels=1000000)
    assert got["status"] == capi.TRACK_LOST and got["iterations_done"] == 0 and got["pixels"] == 3072
    assert rm.same_bits(got["R"], s["R"]) and rm.same_bits(got["t"], s["t"])


# ---- 4. invalid inputs -------------------------------------------------------------------------------------------------------------

def test_invalid_pixels_and_points(corner):
    s = corner.s
    dirty = tsd.dirty_depth(s["depth"])
    got = corner.depth(dirty, s["K"], s["R"], s["t"], "a dirty image", iterations=3)
    assert got["status"] == capi.TRACK_OK and got["pixels"] == 3002
    cloud = _cloud(s)[:1000].copy()
    cloud[5] = np.nan
    cloud[300, 1] = np.nan
    cloud[301, 0] = np.inf
    cloud[640] = -np.inf
    cloud[700:716] = 0.0
    cloud[800] = (0.01, 0.01, 0.01)  # nearer than min_depth
    cloud[801] = (0.0, 0.0, 9.0)     # further than max_depth
    got = corner.points(cloud, s["R"], s["t"], "a dirty cloud", iterations=3)
    assert got["status"] == capi.TRACK_OK and got["pixels"] == 1000 - 22
    for what, got in (("an image of zeros", corner.depth(np.zeros((48, 64), F), s["K"], s["R"], s["t"])),
                      ("an image of NaNs", corner.depth(np.full((48, 64), np.nan, F), s["K"], s["R"], s["t"])),
                      ("no point", corner.points(np.zeros((0, 3), F), s["R"], s["t"])),
                      ("missing returns only", corner.points(np.zeros((300, 3), F), s["R"], s["t"]))):
        assert got["status"] == capi.TRACK_LOST and got["iterations_done"] == 0 and got["pixels"] == 0 and got["rms"] == 0.0, what
        assert not got["sums"].any() and rm.same_bits(got["R"], s["R"]) and rm.same_bits(got["t"], s["t"]), what


# ---- 5. host and device entry points, buffer growth --------------------------------------------------------------------------------

def test_device_variants_equal_the_host_calls_and_buffers_grow(corner):
    """The device entry points read the caller's buffers as they lie.  Then a small call, a large one and a small one again on one
    context — the staging pair and the slab grow and are reused at a smaller size — each against the restatement."""
    s = corner.s
    cloud = _cloud(s)
    want_d = corner.depth(s["depth"], s["K"], s["R"], s["t"], iterations=3)
    want_p = corner.points(cloud, s["R"], s["t"], iterations=3)
    d_depth = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(s["depth"], F))
    d_cloud = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(cloud, F))
    got_d = _result(*corner.e.track_depth_sdf_device(d_depth.ptr, *s["K"], s["R"], s["t"], NEAR, FAR, iterations=3))
    got_p = _result(*corner.e.track_points_sdf_device(d_cloud.ptr, len(cloud), s["R"], s["t"], NEAR, FAR, iterations=3))
    _assert_same(got_d, want_d, "depth, device")
    _assert_same(got_p, want_p, "points, device")
    fresh = Dest("truth")
    try:
        K_big = (240.0, 240.0, 128.0, 96.0, 192, 256)  # 49 152 pixels, 192 slab rows, after 16 and before 255
        big = sr.corner_depth(s["R_true"], s["t_true"], K_big)
        fresh.points(cloud[:16], s["R"], s["t"], "small", iterations=1, min_points=1)
        got = fresh.depth(big, K_big, s["R"], s["t"], "large", iterations=2)
        assert got["pixels"] > 40000
        fresh.points(cloud[:255], s["R"], s["t"], "small again", iterations=2)
        fresh.depth(s["depth"], s["K"], s["R"], s["t"], "and the view", iterations=2)
    finally:
        fresh.close()


# ---- 6. end to end on a fused map, and the reader contract ---------------------------------------------------------------------------

def _blocks_of(e):
    d, v = e.dump_blocks()
    return {(int(x["x"]), int(x["y"]), int(x["z"])): vox.copy() for x, vox in zip(d, v)}


def test_end_to_end_on_a_fused_map_and_the_reader_contract():
    """Frames 0 .. 7 of the synthetic room, 128 x 128 pixels 90 degrees wide (with the 53 degrees of synth.CFG1 the frame sees little
    more than the far wall, sliding along it costs nothing and the estimate drifts), go into a map of 20 mm voxels; frame 8 is
    tracked from a start 0.57 degrees and 52 mm off its pose, within the 60 mm band: bit-identical to the restatement on the
    dumped blocks, and nearer the truth in both the angle and the translation.  On the CPU oracle's map of the same frames the
    restatement ends at 0.147 degrees and 26.4 mm with 15 348 of 16 384 pixels and an rms of 4.10 mm — from that start, from a nearer
    one and from the truth alike, and a frame that is in the map ends 25 mm off too: what is left is the map's own bias at 55 mm
    pixels on 20 mm voxels, not the solver's.  The last frame was host-fed and kept back by mrh_integrate: it is in the map the
    call reads (a twin that was synchronised after every frame gives the same bits).  Map, counters, camera, pose and the last
    extraction are as before."""
    K, params = synth.Intrinsics(64.0, 64.0, 64.0, 64.0, 128, 128), dict(synth.CFG1_PARAMS)
    Kt = (K.fx, K.fy, K.cx, K.cy, K.rows, K.cols)
    frames = list(synth.replica_stream(10, K=K))
    lib = capi.load_hip()
    a, a2 = pu.make_engine(lib, K, params, 32768), pu.make_engine(lib, K, params, 32768)
    try:
        for f in frames[:8]:
            pu.feed(a, f)
            pu.feed(a2, f)
            a2.sync()
        f = frames[8]
        near, far = 0.1, 8.0
        R0, t0 = ar.perturbed(f.R, f.t, angle=0.01, dt=(0.03, -0.03, 0.03))
        got = _result(*a.track_depth_sdf(f.depth, *Kt, R0, t0, near, far))  # no sync, no dump before it: the kept-back frame runs first
        twin = _result(*a2.track_depth_sdf(f.depth, *Kt, R0, t0, near, far))
        _assert_same(got, twin, "a kept-back frame is in the map the call reads")
        A = _blocks_of(a)
        want = sr.track_depth(params, A, f.depth, Kt, near, far, R0, t0)
        _assert_same(got, want, "fused map")
        valid, p = sr.depth_samples(f.depth, Kt, near, far)
        pts = _result(*a.track_points_sdf(p[valid], R0, t0, near, far))
        _assert_same(pts, got, "the frame as a cloud")
        (t_0, a_0), (t_1, a_1) = tr.pose_errors(R0, t0, f.R, f.t), tr.pose_errors(got["R"], got["t"], f.R, f.t)
        print(f"end to end: {a_0:.4f} deg, {1e3 * t_0:.2f} mm -> {a_1:.4f} deg, {1e3 * t_1:.2f} mm; {got['pixels']} of {want['valid']} pixels, rms {1e3 * got['rms']:.3f} mm")
        assert got["status"] == capi.TRACK_OK and got["iterations_done"] == 10 and a_1 < a_0 and t_1 < t_0
        assert got["pixels"] >= 0.5 * want["valid"]
        # the reader contract: the map, the counters and the last extraction
        tris = a.extract_triangles()
        s1 = a.stats()
        again = _result(*a.track_depth_sdf(f.depth, *Kt, R0, t0, near, far))
        _assert_same(again, got, "a second call")
        a.track_points_sdf(p[valid], R0, t0, near, far)
        s2 = a.stats()  # it holds the triangle count of the last extraction
        for name, _ in capi.MrhStats._fields_:
            if "ms" not in name:
                assert getattr(s1, name) == getattr(s2, name), name
        assert len(tris) > 0 and rm.same_bits(a.extract_triangles(), tris)
        A2 = _blocks_of(a)
        assert sorted(A) == sorted(A2) and all(rm.same_bits(A[k], A2[k]) for k in A)
        r = pu.compare_maps(a, a2, tol=0.0)
        assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
        pu.feed(a, frames[8])  # the camera and the pose are still the stream's
        pu.feed(a2, frames[8])
        assert pu.compare_maps(a, a2, tol=0.0)["sdf_bit_exact"]
    finally:
        a.close()
        a2.close()


# ---- 7. arguments ------------------------------------------------------------------------------------------------------------------

def test_arguments_and_unsupported_contexts(corner):
    e, lib, s = corner.e, corner.e.lib, corner.s
    Fp = C.POINTER(C.c_float)
    R, t = np.ascontiguousarray(s["R"], F).reshape(9).copy(), np.ascontiguousarray(s["t"], F).copy()
    oR, ot, info = np.zeros(9, F), np.zeros(3, F), capi.MrhTrackInfo()
    depth, cloud = np.ascontiguousarray(s["depth"], F), np.ascontiguousarray(_cloud(s), F)
    before = e.dump_blocks()

    def block(**kw):
        p = capi.MrhSdftrackParams(*s["K"][:4], int(s["K"][4]), int(s["K"][5]), NEAR, FAR, 0.0, 0, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(fn, p, obs, pR=R, pt=t, oR=oR, ot=ot, info=info, ctx=e._ctx):
        ptr = lambda x: None if x is None else x.ctypes.data_as(Fp)  # noqa: E731
        return fn(ctx, C.byref(p) if p is not None else None, *obs, ptr(pR), ptr(pt), ptr(oR), ptr(ot), C.byref(info) if info is not None else None)

    forms = [(lib.mrh_track_depth_sdf, (depth.ctypes.data,), (None,)), (lib.mrh_track_points_sdf, (cloud.ctypes.data, len(cloud)), (None, len(cloud)))]
    d_depth, d_cloud = hipmem.DeviceBuffer.from_numpy(depth), hipmem.DeviceBuffer.from_numpy(cloud)
    forms += [(lib.mrh_track_depth_sdf_device, (d_depth.ptr,), (None,)), (lib.mrh_track_points_sdf_device, (d_cloud.ptr, len(cloud)), (None, len(cloud)))]
    for fn, obs, no_obs in forms:
        name = fn.__name__
        assert call(fn, block(), obs) == capi.MRH_OK and info.status == capi.TRACK_OK and info.iterations_done == 10, name
        assert call(fn, block(), obs, info=None) == capi.MRH_OK  # the info is optional
        for kw in (dict(p=None), dict(obs=no_obs), dict(pR=None), dict(pt=None), dict(oR=None), dict(ot=None)):
            args = dict(dict(p=block(), obs=obs), **kw)
            assert call(fn, **args) == capi.MRH_ERR_INVALID_ARG and b"null argument" in lib.mrh_last_error(e._ctx), (name, kw)
        assert call(fn, block(), obs, ctx=None) == capi.MRH_ERR_INVALID_ARG
        bad = [(block(reserved=1), b"reserved"), (block(min_depth=0.0), b"min_depth"), (block(min_depth=FAR, max_depth=NEAR), b"min_depth"),
               (block(max_depth=float("inf")), b"min_depth"), (block(band=-0.1), b"band"), (block(band=1.5), b"band"), (block(band=float("nan")), b"band"),
               (block(iterations=-1), b"iterations"), (block(iterations=65), b"iterations")]
        if "depth" in name:
            bad += [(block(rows=0), b"pixels"), (block(cols=4097), b"pixels"), (block(fx=0.0), b"intrinsics"), (block(cy=float("nan")), b"intrinsics")]
        else:  # the points calls do not read the camera; more than 2^24 points are refused before the cloud is read
            assert call(fn, block(rows=0, cols=-1, fx=0.0, cy=float("nan")), obs) == capi.MRH_OK
            assert call(fn, block(), (obs[0], (1 << 24) + 1)) == capi.MRH_ERR_INVALID_ARG and b"limit 2^24" in lib.mrh_last_error(e._ctx)
            assert call(fn, block(), (None, 0)) == capi.MRH_OK and info.status == capi.TRACK_LOST  # an empty cloud needs no pointer
        for p, word in bad:
            assert call(fn, p, obs) == capi.MRH_ERR_INVALID_ARG and word in lib.mrh_last_error(e._ctx), (name, word)
        for i in range(12):
            R2, t2 = R.copy(), t.copy()
            (R2 if i < 9 else t2)[i if i < 9 else i - 9] = [np.nan, np.inf, -np.inf][i % 3]
            assert call(fn, block(), obs, pR=R2, pt=t2) == capi.MRH_ERR_INVALID_ARG and b"not finite" in lib.mrh_last_error(e._ctx)
    with pytest.raises(ValueError):
        e.track_depth_sdf(depth[:10], *s["K"], R, t, NEAR, FAR)
    after = e.dump_blocks()
    assert rm.same_bits(before[0], after[0]) and rm.same_bits(before[1], after[1])  # none of the calls touched the map


def test_a_sharded_context_is_unsupported_and_a_pending_exchange_is_a_state_error(corner):
    s = corner.s
    params = dict(synth.CFG1_PARAMS, n_frames_invalidate_voxels=2)
    sharded = pu.make_engine(capi.load_hip(), synth.CFG1, params, 16384, shard_rank=0, shard_count=2, shard_chunk_log2=1)
    try:
        calls = (lambda: sharded.track_depth_sdf(s["depth"], *s["K"], s["R"], s["t"], NEAR, FAR), lambda: sharded.track_points_sdf(_cloud(s), s["R"], s["t"], NEAR, FAR))
        for c in calls:
            with pytest.raises(capi.MrhError) as ei:
                c()
            assert ei.value.code == capi.MRH_ERR_UNSUPPORTED and "sharded" in str(ei.value)
        # a starve frame of the host protocol leaves an exchange pending: mrh_integrate returns MRH_PENDING_EXCHANGE
        seen = 0
        for f in (synth.cfg1_sphere(), synth.cfg1_sphere(zc=1.51), synth.cfg1_sphere(zc=1.5), synth.cfg1_sphere(zc=1.49)):
            sharded.set_pose(f.R, f.t)
            sharded.upload_depth(f.depth)
            sharded.upload_rgb(f.rgb)
            pending = sharded.integrate()
            while pending:
                seen += 1
                for c in calls:
                    with pytest.raises(capi.MrhError) as ei:
                        c()
                    assert ei.value.code == capi.MRH_ERR_STATE and "pending" in str(ei.value)
                pending = sharded.integrate_resume()
        assert seen > 0
    finally:
        sharded.close()


# ---- 8. the facade -----------------------------------------------------------------------------------------------------------------

def test_geowrapper_track_sdf(monkeypatch):
    """GeoWrapper.trackDepthImageSDF / trackPointCloudSDF through the pybind module on a map fused from depth frames (the facade has no
    block import), against Engine.track_depth_sdf / track_points_sdf on a twin engine fed the same frames: intrinsics and depth limits
    are those of the last setCamera, the start the current pose or (t, q); the points form accepts either camera model."""
    monkeypatch.setenv("MRHASH_NUM_SDF_BLOCKS", "32768")
    from mrhash.src.pygeowrapper import GeoWrapper

    p, Kc = synth.CFG1_PARAMS, synth.CFG1
    Kt = (Kc.fx, Kc.fy, Kc.cx, Kc.cy, Kc.rows, Kc.cols)
    near, far = 0.1, 8.0
    g = GeoWrapper(sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=p["virtual_voxel_size"],
                   n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=1, viewer_active=False,
                   marching_cubes_threshold=p["marching_cubes_threshold"], min_weight_threshold=p["min_weight_threshold"], min_depth=near, max_depth=far)
    e = pu.make_engine(capi.load_hip(), Kc, dict(p, min_depth=near, max_depth=far), 32768)
    try:
        with pytest.raises(RuntimeError):
            g.trackPointCloudSDF(np.ones((4, 3), F))  # no camera yet: no depth limits
        g.setCamera(*Kt, near, far, 0)
        frames = list(synth.replica_stream(7, K=Kc))
        for f in frames[:6]:
            g.setCurrPose(f.t, f.q)
            g.setDepthImage(f.depth)
            g.setRGBImage(f.rgb)
            g.compute()
            pu.feed(e, f)
        f = frames[6]
        pose = g.getCurrPose().copy()  # frame 5's: 1.8 degrees and 31 mm from frame 6's
        R0, t0 = pose[:3, :3].astype(F), pose[:3, 3].astype(F)
        valid, pc = sr.depth_samples(f.depth, Kt, near, far)
        cloud = np.ascontiguousarray(pc[valid])
        want = e.track_depth_sdf(f.depth, *Kt, R0, t0, near, far)
        want_p = e.track_points_sdf(cloud, R0, t0, near, far)
        assert want[2]["status"] == capi.TRACK_OK and want[2]["pixels"] >= 64
        calls = ((g.trackDepthImageSDF(f.depth), want), (g.trackDepthImageSDF(f.depth, frames[5].t, frames[5].q), want),
                 (g.trackPointCloudSDF(cloud), want_p), (g.trackPointCloudSDF(cloud, frames[5].t, frames[5].q), want_p))
        for (t, q, info), w in calls:
            assert rm.same_bits(np.asarray(t, F), w[1])
            assert np.array_equal(np.asarray(info["sums"]), w[2]["sums"]) and info["status"] == w[2]["status"] and info["iterations_done"] == w[2]["iterations_done"]
            assert info["pixels"] == w[2]["pixels"] and info["rms"] == w[2]["rms"]
            q = np.asarray(q, np.float64)
            assert abs(np.linalg.norm(q) - 1.0) <= 1e-6 and q[3] >= 0
            assert np.abs(synth.quat_to_rot(q).astype(np.float64) - w[0]).max() <= 1e-6
        assert np.array_equal(g.getCurrPose(), pose)  # the current pose is the caller's to set
        with pytest.raises(RuntimeError):
            g.trackDepthImageSDF(f.depth[:100])
        with pytest.raises(RuntimeError, match=r"GeoWrapper::trackPointCloudSDF\|"):
            g.trackPointCloudSDF(np.ones((4, 2), F))
        g.setCamera(1.0, 1.0, 0.0, 0.0, 1, 1, near, far, 1)  # a spherical camera: the points form still runs, the depth form does not
        t, q, info = g.trackPointCloudSDF(cloud)
        assert rm.same_bits(np.asarray(t, F), want_p[1]) and np.array_equal(np.asarray(info["sums"]), want_p[2]["sums"])
        with pytest.raises(RuntimeError):
            g.trackDepthImageSDF(np.ones((1, 1), F))
    finally:
        e.close()
        del g
