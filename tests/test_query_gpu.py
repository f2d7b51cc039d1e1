"""GPU half of the point query (mrh_query.h, include/mrhash_query.h): byte for byte against the restatement of
tests/query_ref.py, in both fields and for all four outputs, on hand-built single- and multi-resolution maps (tests/mc_fields.py),
far from the origin, through a pose, with refused points, through the device variant and the GeoWrapper facade, and without side
effects on the frame path.  Maps are imported, not fused; the coverage conditions of tests/test_query.py are asserted again on
what the GPU returned."""
import ctypes as C

import numpy as np
import pytest

import esdf_ref as er
import mc_fields as mf
import parity_utils as pu
import query_ref as qr
import raycast_ref as rr
from mrhash_amd import capi, hipmem, synth

pytestmark = pytest.mark.gpu

F = np.float32
K = synth.REPLICA_640
VAR_PARAMS = dict(mf.PARAMS, sdf_var_threshold=0.005)
OUTPUTS = ("dist", "grad", "rgbw", "state")


def _engine(blocks, params, num_sdf_blocks=4096):
    e = pu.make_engine(capi.load_hip(), synth.CFG1, params, num_sdf_blocks)
    e.import_blocks(*er.to_import(blocks))
    return e


def _ref_map(e, params):
    d, v = e.dump_blocks()
    return rr.make_map(params, d, v)


def _assert_same(got, want, what):
    for a, b, name in zip(got, want, OUTPUTS):
        if b is None:
            assert a is None, f"{what}: {name} was not asked for"
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {name} {a.shape} {a.dtype}"
        if not qr.same_bits(a, b):
            rows = [np.ascontiguousarray(x).reshape(len(x), -1).view(np.uint8) for x in (a, b)]
            bad = np.flatnonzero(np.any(rows[0] != rows[1], axis=1))
            raise AssertionError(f"{what}: {name} differs at {len(bad)} of {len(a)} points, first {bad[:5]}: {a[bad[:3]]} vs {b[bad[:3]]}")


class Field:
    """An engine on an imported map, the restatement's map of its dump, a point set and the restatement's answer in both fields."""

    def __init__(self, blocks, params, pts):
        self.params, self.pts = params, pts
        self.e = _engine(blocks, params)
        self.m = _ref_map(self.e, params)
        self.want = {smooth: qr.query(self.m, pts, smooth=smooth) for smooth in (False, True)}

    def check(self, min_dist, min_grad, min_coarse=None):
        for smooth in (False, True):
            got = self.e.query(self.pts, smooth=smooth)
            _assert_same(got, self.want[smooth], "SMOOTH" if smooth else "MAP")
            cov = qr.coverage(got[3])
            print("SMOOTH" if smooth else "MAP", cov)
            assert cov["dist"] >= min_dist and cov["grad"] >= min_grad and cov["refused"] == 0
            if min_coarse is not None:
                assert cov["coarse"] >= min_coarse


@pytest.fixture(scope="module")
def dense():
    f = Field(mf.sign_field(7), mf.PARAMS, qr.cluster_points(mf.PARAMS["virtual_voxel_size"]))
    yield f
    f.e.close()


@pytest.fixture(scope="module")
def holes():
    f = Field(mf.sign_field(7, holes=0.03, starved=0.5, absent=0.1), mf.PARAMS, qr.cluster_points(mf.PARAMS["virtual_voxel_size"]))
    yield f
    f.e.close()


@pytest.fixture(scope="module")
def adaptive():
    f = Field(mf.sign_field(7, holes=0.02, absent=0.1, coarse=0.4, params=VAR_PARAMS), VAR_PARAMS, qr.cluster_points(VAR_PARAMS["virtual_voxel_size"]))
    yield f
    f.e.close()


# ---- 1 - 4. the fields ---------------------------------------------------------------------------------------------------------

def test_dense_field(dense):
    dense.check(0.40, 0.15)


def test_field_with_holes_starved_cells_and_absent_blocks(holes):
    holes.check(0.40, 0.15)


def test_variance_adaptive_field(adaptive):
    d, _ = adaptive.e.dump_blocks()
    assert 0 < int((d["resolution"] == 1).sum()) < len(d)
    adaptive.check(0.40, 0.15, min_coarse=0.15)


def test_ladder():
    """Blocks at +-2^k, k = 8 .. 16: where voxel -> block changes from the shift to the float detour."""
    blocks, p = mf.ladder(0.05)
    f = Field(blocks, p, qr.ladder_points(blocks, 0.05))
    try:
        f.check(0.30, 0.08)
    finally:
        f.e.close()


# ---- 5. a pose -----------------------------------------------------------------------------------------------------------------

def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_posed_call_equals_the_world_call_on_the_transformed_points(holes):
    R64, t64 = _rotation(2), np.array([0.31, -0.22, 0.47])
    R, t = R64.astype(F), t64.astype(F)
    world = holes.pts[:400].astype(np.float64)
    sensor = ((world - t64) @ R64).astype(F)  # R^T (p - t)
    sensor[::25] = 0.0                         # missing returns ...
    sensor[5::50] = [-0.0, 0.0, -0.0]          # ... with either sign of zero
    zero = np.all(sensor == 0, axis=-1)
    P = qr.transform(R, t, sensor)
    for smooth in (False, True):
        got = holes.e.query(sensor, R, t, smooth=smooth)
        _assert_same(got, qr.query(holes.m, sensor, R, t, smooth=smooth), "posed")
        assert np.all(got[3][zero] == qr.REFUSED) and not np.any(got[3][~zero] & qr.REFUSED)
        for out in got[:3]:
            assert not np.ascontiguousarray(out[zero]).view(np.uint8).any()
        world_call = holes.e.query(P, smooth=smooth)
        for a, b in zip(got, world_call):
            assert qr.same_bits(a[~zero], b[~zero])
        assert np.mean((got[3] & qr.DIST) != 0) >= 0.3


# ---- 6. refused points, sizes around a wave and a workgroup, canaries --------------------------------------------------------------

def _interleaved(field, n=257):
    pts = field.pts[:n].copy()
    bound = qr.bound(field.params["virtual_voxel_size"])
    bad = [[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], [bound, 0.1, 0.1], [0.1, -bound, 0.1], [3e38, 3e38, 3e38], [np.nan, np.nan, np.nan]]
    for k, i in enumerate(range(1, n, 3)):
        pts[i] = bad[k % len(bad)]
    pts[0] = [mf.prevfloat(bound), 0.1, 0.1]  # the last accepted magnitude: an absent block far out
    return pts


CANARY = 0xA5


def _canary_buffer(nbytes):
    b = hipmem.DeviceBuffer(nbytes + 64)
    hipmem.write(b.ptr, np.full(nbytes + 64, CANARY, np.uint8))
    return b


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_refused_points_sizes_and_canaries(dense, n):
    pts = _interleaved(dense)[:n]
    e = dense.e
    for smooth in (False, True):
        want = qr.query(dense.m, pts, smooth=smooth) if n else (np.zeros(0, F), np.zeros((0, 3), F), np.zeros((0, 4), np.uint8), np.zeros(0, np.uint8))
        got = e.query(pts, smooth=smooth)
        _assert_same(got, want, f"n = {n}")
        if n > 1:
            assert np.array_equal((got[3] & qr.REFUSED) != 0, np.arange(n) % 3 == 1) and not (got[3][0] & qr.REFUSED)
        d_pts = hipmem.DeviceBuffer.from_numpy(pts) if n else hipmem.DeviceBuffer(16)
        sizes = (4 * n, 12 * n, 4 * n, n)
        bufs = [_canary_buffer(s) for s in sizes]
        e.query_device(d_pts.ptr, n, smooth=smooth, d_dist=bufs[0].ptr, d_grad=bufs[1].ptr, d_rgbw=bufs[2].ptr, d_state=bufs[3].ptr)
        e.sync()
        for b, s, w, name in zip(bufs, sizes, want, OUTPUTS):
            raw = b.to_numpy(np.uint8)
            assert np.all(raw[s:] == CANARY), f"{name}: bytes behind the output were written (n = {n})"
            assert raw[:s].tobytes() == np.ascontiguousarray(w).tobytes(), f"{name}: device call differs (n = {n})"


# ---- 7. the device call and the optional outputs -----------------------------------------------------------------------------------

def test_device_variant_and_every_subset_of_the_optional_outputs(adaptive):
    e, pts = adaptive.e, adaptive.pts[:500]
    n = len(pts)
    d_pts = hipmem.DeviceBuffer.from_numpy(pts)
    for smooth in (False, True):
        full = tuple(x[:n] for x in adaptive.want[smooth])
        no_grad_state = qr.query(adaptive.m, pts, smooth=smooth, gradient=False)[3]
        assert np.array_equal(no_grad_state, full[3] & ~np.uint8(qr.GRAD)) and np.any(full[3] & qr.GRAD)
        for want_grad in (False, True):
            for want_rgbw in (False, True):
                state = full[3] if want_grad else no_grad_state
                got = e.query(pts, smooth=smooth, gradient=want_grad, colour=want_rgbw)
                _assert_same(got, (full[0], full[1] if want_grad else None, full[2] if want_rgbw else None, state), f"blocking, grad {want_grad}, rgbw {want_rgbw}")
                bufs = [_canary_buffer(s) for s in (4 * n, 12 * n, 4 * n, n)]
                e.query_device(d_pts.ptr, n, smooth=smooth, d_dist=bufs[0].ptr, d_grad=bufs[1].ptr if want_grad else 0,
                               d_rgbw=bufs[2].ptr if want_rgbw else 0, d_state=bufs[3].ptr)
                e.sync()
                assert qr.same_bits(bufs[0].to_numpy(F, n), full[0]) and np.array_equal(bufs[3].to_numpy(np.uint8, n), state)
                grad, rgbw = bufs[1].to_numpy(np.uint8), bufs[2].to_numpy(np.uint8)
                assert grad[: 12 * n].tobytes() == full[1].tobytes() if want_grad else np.all(grad == CANARY)
                assert rgbw[: 4 * n].tobytes() == full[2].tobytes() if want_rgbw else np.all(rgbw == CANARY)
    # an output bit without its pointer, and a pointer without its bit, both mean "not produced"
    p = capi.MrhQueryParams(capi.QUERY_FIELD_MAP, 0)
    bufs = [_canary_buffer(s) for s in (4 * n, 12 * n, 4 * n, n)]
    assert e.lib.mrh_query_points_device(e._ctx, C.byref(p), d_pts.ptr, n, None, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr) == capi.MRH_OK
    e.sync()
    assert np.all(bufs[1].to_numpy(np.uint8) == CANARY) and np.all(bufs[2].to_numpy(np.uint8) == CANARY)
    pg, ps = C.c_void_p(1), C.c_void_p()
    assert e.lib.mrh_query_points(e._ctx, C.byref(p), pts.ctypes.data, n, None, None, None, C.byref(pg), None, C.byref(ps)) == capi.MRH_OK
    assert pg.value is None and ps.value is not None


# ---- 8. the reader contract --------------------------------------------------------------------------------------------------------

def test_query_leaves_the_frame_path_alone():
    hip = capi.load_hip()
    params = dict(synth.REPLICA_PARAMS)
    frames = list(synth.replica_stream(8))
    a = pu.make_engine(hip, K, params, 65536)
    b = pu.make_engine(hip, K, params, 65536)
    try:
        for f in frames[:5]:
            pu.feed(a, f)
            pu.feed(b, f)
        d, v = b.dump_blocks()
        pts = qr.ladder_points(rr.blocks_from_dump(d, v, multi=False), params["virtual_voxel_size"], seed=6)[:300]
        got = [a.query(pts, smooth=s) for s in (False, True)]  # between two frames of the pipelined stream, no sync
        m = rr.make_map(params, *a.dump_blocks())
        for s in (False, True):
            _assert_same(got[s], qr.query(m, pts, smooth=s), "between pipelined frames")
            assert np.mean((got[s][3] & qr.DIST) != 0) >= 0.10
        for f in frames[5:]:
            pu.feed(a, f)
            a.query(pts)
            a.query(pts, f.R, f.t, smooth=True)
            pu.feed(b, f)
        r = pu.compare_maps(a, b, tol=0.0)
        assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
        pu.compare_meshes(a, b, tol=0.0)
        # counters, the camera and the last extraction survive the call
        tris = a.extract_triangles()
        V, Fc, Cc = a.extract_mesh()
        s0 = a.stats()
        a.query(pts)
        s1 = a.stats()
        V2, F2, C2 = a.extract_mesh()
        assert er.same_bits(V, V2) and np.array_equal(Fc, F2) and er.same_bits(Cc, C2)
        assert er.same_bits(a.extract_triangles(), tris)
        for name, _ in capi.MrhStats._fields_:
            if "ms" not in name:
                assert getattr(s0, name) == getattr(s1, name), name
        pu.feed(a, frames[-1])  # the camera and the pose are still the stream's: the same frame again lands on the same blocks
        pu.feed(b, frames[-1])
        assert pu.compare_maps(a, b, tol=0.0)["sdf_bit_exact"]
    finally:
        a.close()
        b.close()


def test_arguments_and_a_sharded_context(dense):
    e, pts = dense.e, dense.pts[:8]
    I, Z = np.eye(3, dtype=F), np.zeros(3, F)
    nan_R = I.copy()
    nan_R[1, 1] = np.nan
    for kw in (dict(R=nan_R, t=Z), dict(R=I, t=np.array([0, np.inf, 0], F))):
        with pytest.raises(capi.MrhError) as ei:
            e.query(pts, **kw)
        assert ei.value.code == capi.MRH_ERR_INVALID_ARG
    Fp = C.POINTER(C.c_float)
    out = [C.c_void_p() for _ in range(4)]
    refs = [C.byref(x) for x in out]
    bad = [capi.MrhQueryParams(2, 0), capi.MrhQueryParams(0, 4), capi.MrhQueryParams(0, 0, (C.c_uint32 * 2)(0, 1))]
    for p in bad:
        assert e.lib.mrh_query_points(e._ctx, C.byref(p), pts.ctypes.data, len(pts), None, None, *refs) == capi.MRH_ERR_INVALID_ARG
    ok = capi.MrhQueryParams(0, 3)
    assert e.lib.mrh_query_points(e._ctx, C.byref(ok), pts.ctypes.data, len(pts), I.ctypes.data_as(Fp), None, *refs) == capi.MRH_ERR_INVALID_ARG  # R without t
    assert e.lib.mrh_query_points(e._ctx, C.byref(ok), None, len(pts), None, None, *refs) == capi.MRH_ERR_INVALID_ARG                         # no points
    assert e.lib.mrh_query_points(e._ctx, C.byref(ok), pts.ctypes.data, capi.QUERY_MAX_POINTS + 1, None, None, *refs) == capi.MRH_ERR_INVALID_ARG
    assert b"limit 2^24" in e.lib.mrh_last_error(e._ctx)
    assert e.lib.mrh_query_points(e._ctx, None, pts.ctypes.data, len(pts), None, None, *refs) == capi.MRH_ERR_INVALID_ARG
    assert b"null argument" in e.lib.mrh_last_error(e._ctx)
    d_pts = hipmem.DeviceBuffer.from_numpy(pts)
    with pytest.raises(capi.MrhError) as ei:
        e.query_device(d_pts.ptr, len(pts))  # no d_dist / d_state
    assert ei.value.code == capi.MRH_ERR_INVALID_ARG
    assert e.lib.mrh_query_points(e._ctx, C.byref(ok), None, 0, None, None, *refs) == capi.MRH_OK and all(x.value is None for x in out)  # n = 0
    s = capi.Engine(capi.load_hip(), capi.Params(num_sdf_blocks=4096, shard_rank=0, shard_count=2, **mf.PARAMS))
    try:
        with pytest.raises(capi.MrhError) as ei:
            s.query(pts)
        assert ei.value.code == capi.MRH_ERR_UNSUPPORTED
    finally:
        s.close()


# ---- 9. the facade -------------------------------------------------------------------------------------------------------------

def test_geowrapper_query_points(monkeypatch):
    """The facade on a sphere fused from depth frames (it has no block import): world points, and sensor-frame points at the pose
    of the last setCurrPose."""
    monkeypatch.setenv("MRHASH_NUM_SDF_BLOCKS", "16384")
    from mrhash.src.pygeowrapper import GeoWrapper

    p, Kc = synth.CFG1_PARAMS, synth.CFG1
    g = GeoWrapper(sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=p["virtual_voxel_size"],
                   n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=1, viewer_active=False,
                   marching_cubes_threshold=p["marching_cubes_threshold"], min_weight_threshold=p["min_weight_threshold"], min_depth=0.1, max_depth=8.0)
    g.setCamera(Kc.fx, Kc.fy, Kc.cx, Kc.cy, Kc.rows, Kc.cols, 0.1, 8.0, 0)
    e = pu.make_engine(capi.load_hip(), Kc, dict(p, min_depth=0.1, max_depth=8.0), 16384)
    try:
        f = synth.cfg1_sphere()
        for _ in range(6):
            g.setCurrPose(f.t, f.q)
            g.setDepthImage(f.depth)
            g.setRGBImage(f.rgb)
            g.compute()
            pu.feed(e, f)
        rng = np.random.default_rng(9)
        world = rng.uniform([-0.31, -0.294, 0.805], [0.305, 0.31, 1.295], (400, 3)).astype(F)
        for smooth in (False, True):
            got = g.queryPoints(world, smooth=smooth)
            _assert_same(got, e.query(world, smooth=smooth), "GeoWrapper.queryPoints")
            assert np.mean((got[3] & qr.DIST) != 0) >= 0.2
        q = np.array([0.3, -0.5, 0.2, 0.7])
        g.setCurrPose(np.array([0.05, -0.1, 0.2], F), (q / np.linalg.norm(q)).astype(F))  # a general rotation; compute() is not called again
        pose = g.getCurrPose()
        R, t = pose[:3, :3].copy(), pose[:3, 3].copy()
        sensor = ((world.astype(np.float64) - t.astype(np.float64)) @ R.astype(np.float64)).astype(F)
        sensor[::40] = 0.0
        for smooth in (False, True):
            got = g.queryPoints(sensor, smooth=smooth, sensor_frame=True)
            _assert_same(got, e.query(sensor, R, t, smooth=smooth), "GeoWrapper.queryPoints, sensor frame")
            assert np.all(got[3][::40] == qr.REFUSED) and np.mean((got[3] & qr.DIST) != 0) >= 0.2
        assert g.queryPoints(np.zeros((0, 3), F))[0].shape == (0,)
        with pytest.raises(RuntimeError, match=r"GeoWrapper::queryPoints\|"):
            g.queryPoints(np.zeros((4, 2), F))
    finally:
        e.close()
        del g
