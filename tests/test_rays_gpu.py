"""GPU half of the ray queries (k_cast_rays in mrh_rays.h, include/mrhash_rays.h).

  kernel against kernel       every scene of tests/ray_fields.py cast as its own pixel rays, row-major: range, normals and colours are
                              the bytes of Engine.raycast / Engine.raycast_spherical of the same scene — the march, the jump with a
                              per-lane origin, the refinement, the normal and the colour against k_raycast, no restatement involved
  kernel against restatement  every output, counts and first_unknown included, against tests/rays_ref.py: the mixed batch of
                              tests/ray_batches.py (with a pose, without one, with per-ray ends) and one scene per group
  batch shape and order       a ray's bytes do not depend on the batch it is cast in
  output subsets, read-only, refusals, bindings

Maps are imported, not fused (the facade test fuses a sphere: GeoWrapper has no block import).  "ladder far" and "key_range" have
their cameras beyond D21's origin bound: there every ray is MRH_RAY_BAD (tests/test_rays.py: beyond_the_bound)."""
import ctypes as C

import numpy as np
import pytest

import independent as ind
import mc_fields as mf
import parity_utils as pu
import ray_batches as rb
import ray_fields as rf
import raycast_ref as rr
import rays_ref as yr
from mrhash_amd import capi, hipmem, synth
from test_rays import beyond_the_bound, pixel_rays

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = {g: rf.GROUPS[g]() for g in rf.GROUPS}
CASES = [pytest.param(g, i, id="%s" % s.name) for g in rf.GROUPS for i, s in enumerate(SCENES[g])]
# kernel against restatement: per group the scene with the fewest ray samples (the restatement marches them in Python)
RESTATED = {g: min(range(len(SCENES[g])), key=lambda i: SCENES[g][i].intr[4] * SCENES[g][i].intr[5] * (SCENES[g][i].max_depth - SCENES[g][i].min_depth) / SCENES[g][i].step)
            for g in rf.GROUPS}
RESTATED["steps"] = [s.name for s in SCENES["steps"]].index("steps 2 samples")  # "1 sample" cannot hit


def _engine(blocks, params, num_sdf_blocks=4096):
    e = pu.make_engine(capi.load_hip(), synth.CFG1, params, num_sdf_blocks)
    e.import_blocks(*mf.to_import(blocks))
    return e


@pytest.fixture(scope="module")
def field(request):
    g = request.param
    s = SCENES[g][0]
    e = _engine(s.blocks, s.params, rf.NUM_SDF_BLOCKS.get(g, 4096))
    yield g, e
    e.close()


def _cast_scene(e, s, **kw):
    """The scene's pixel rays (d_c from the render restatement's own expressions: they need no map), cast with the scene's pose."""
    o, dc = pixel_rays(s, rf.raycaster(s, ind.Map(s.params, {})))
    return o, dc, e.cast_rays(o, dc, s.max_depth, s.min_depth, s.step, R=s.R, t=s.t, normalize=False, **kw)


@pytest.mark.parametrize("field, i", CASES, indirect=["field"])
def test_pixel_rays_equal_the_render(field, i):
    g, e = field
    s = SCENES[g][i]
    if s.model == "spherical":
        want = e.raycast_spherical(*s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step)
    else:
        want = e.raycast(*s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step)
    o, dc, got = _cast_scene(e, s)
    n = len(o)
    if beyond_the_bound(s):
        assert np.all(got["status"] == capi.RAY_BAD) and not any(np.ascontiguousarray(got[k]).view(np.uint8).any() for k in yr.PLANES if k != "status")
        assert np.count_nonzero(want[0]) >= 8
        return
    render = {"range": want[0].reshape(n), "normals": want[1].reshape(n, 3), "rgb": want[2].reshape(n, 3)}
    yr.assert_same(got, render, s.name, planes=("range", "normals", "rgb"))
    assert np.array_equal((got["status"] & capi.RAY_HIT) != 0, render["range"] > 0)
    assert np.array_equal((got["status"] & capi.RAY_UNKNOWN) != 0, got["counts"][:, 1] > 0)
    print("%s: %d rays, %d hits, status %s" % (s.name, n, np.count_nonzero(render["range"]), np.bincount(got["status"], minlength=8)[:8]))


@pytest.mark.parametrize("field", list(rf.GROUPS), indirect=True)
def test_one_scene_per_group_equals_the_restatement(field):
    g, e = field
    s = SCENES[g][RESTATED[g]]
    m = rr.make_map(s.params, *e.dump_blocks())
    o, dc, got = _cast_scene(e, s)
    q = yr.RayQuery(m, s.min_depth, s.max_depth, s.step)
    want = q.cast(o, dc, R=s.R, t=s.t)
    yr.assert_same(got, want, s.name, events=q.rays)
    print("%s: %d rays x %d samples, %s" % (s.name, len(o), len(q.z), {ev: q.count(ev) for ev in yr.EVENTS if q.count(ev)}))


# ---- the mixed batch -----------------------------------------------------------------------------------------------------------

class Mixed:
    def __init__(self):
        self.b = rb.mixed_batch()
        self.e = _engine(rb.rays_blocks(), rb.PARAMS)
        self.m = rr.make_map(rb.PARAMS, *self.e.dump_blocks())
        self.kw = dict(max_range=self.b.max_range, min_range=self.b.min_range, step=self.b.step, normalize=False)
        self.full = self.e.cast_rays(self.b.origins, self.b.directions, tmax=self.b.tmax, **self.kw)

    def query(self):
        return yr.RayQuery(self.m, self.b.min_range, self.b.max_range, self.b.step, truncation=rb.PARAMS["sdf_truncation"])


@pytest.fixture(scope="module")
def mixed():
    x = Mixed()
    yield x
    x.e.close()


@pytest.mark.parametrize("how", ["tmax", "no pose", "pose"])
def test_the_mixed_batch_equals_the_restatement(mixed, how):
    b, q = mixed.b, mixed.query()
    if how == "tmax":
        got, want = mixed.full, q.cast(b.origins, b.directions, tmax=b.tmax)
        assert np.bincount(got["status"][got["status"] < 8], minlength=8).min() >= 4  # all eight combinations of HIT x UNKNOWN x INSIDE
    elif how == "no pose":
        got, want = mixed.e.cast_rays(b.origins, b.directions, **mixed.kw), q.cast(b.origins, b.directions)
    else:
        o, d = rb.sensor_frame(b)
        got = mixed.e.cast_rays(o, d, tmax=b.tmax, R=rb.POSE_R, t=rb.POSE_T, **mixed.kw)
        want = q.cast(o, d, tmax=b.tmax, R=rb.POSE_R, t=rb.POSE_T)
    yr.assert_same(got, want, how, events=q.rays)
    bad = np.flatnonzero(got["status"] & capi.RAY_BAD)
    assert 1 <= len(bad) <= len(b.origins) // 8
    print(how, np.bincount(got["status"], minlength=8)[:8], "bad", len(bad))


def test_a_ray_does_not_depend_on_its_batch(mixed):
    b, full = mixed.b, mixed.full
    for n in (1, 63, 64, 65, 257):
        got = mixed.e.cast_rays(b.origins[:n], b.directions[:n], tmax=b.tmax[:n], **mixed.kw)
        yr.assert_same(got, {k: v[:n] for k, v in full.items()}, "the first %d rays" % n)
    perm = np.random.default_rng(3).permutation(len(b.origins))
    got = mixed.e.cast_rays(b.origins[perm], b.directions[perm], tmax=b.tmax[perm], **mixed.kw)
    yr.assert_same(got, {k: v[perm] for k, v in full.items()}, "shuffled")


CANARY = 0xA5


def _canary(nbytes):
    return hipmem.DeviceBuffer.from_numpy(np.full(nbytes, CANARY, np.uint8))


def test_every_output_subset_equals_its_plane_of_the_full_cast(mixed):
    b, e, full = mixed.b, mixed.e, mixed.full
    n = len(b.origins)
    lean = e.cast_rays(b.origins, b.directions, tmax=b.tmax, normals=False, colors=False, counts=False, **mixed.kw)
    assert lean["normals"] is None and lean["rgb"] is None and lean["counts"] is None and lean["first_unknown"] is None
    yr.assert_same(lean, full, "range and status alone", planes=("range", "status"))  # the status bits do not need the counts
    d_o, d_d, d_t = (hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(x)) for x in (b.origins, b.directions, b.tmax))
    sizes = {"normals": 12 * n, "rgb": 3 * n, "counts": 8 * n, "first_unknown": 4 * n}
    for only in sizes:
        bufs = {k: _canary(v) for k, v in sizes.items()}
        d_r, d_s = _canary(4 * n), _canary(n)
        e.cast_rays_device(d_o.ptr, d_d.ptr, n, b.max_range, b.min_range, b.step, d_tmax=d_t.ptr, d_range=d_r.ptr, d_status=d_s.ptr,
                           **{"d_" + only: bufs[only].ptr})
        e.sync()
        assert d_r.to_numpy(np.uint8).tobytes() == full["range"].tobytes() and d_s.to_numpy(np.uint8).tobytes() == full["status"].tobytes(), only
        for k, buf in bufs.items():
            raw = buf.to_numpy(np.uint8)
            assert raw.tobytes() == np.ascontiguousarray(full[k]).tobytes() if k == only else np.all(raw == CANARY), (only, k)
    # an output bit without its pointer, and a pointer without its bit, both mean "not produced"
    bufs = {k: _canary(v) for k, v in sizes.items()}
    d_r, d_s = _canary(4 * n), _canary(n)
    p = capi.MrhRaysParams(b.min_range, b.max_range, b.step, 0)
    assert e.lib.mrh_cast_rays_device(e._ctx, C.byref(p), d_o.ptr, d_d.ptr, d_t.ptr, n, None, None, d_r.ptr, d_s.ptr, bufs["normals"].ptr, bufs["rgb"].ptr,
                                      bufs["counts"].ptr, bufs["first_unknown"].ptr) == capi.MRH_OK
    e.sync()
    assert all(np.all(buf.to_numpy(np.uint8) == CANARY) for buf in bufs.values())
    assert d_s.to_numpy(np.uint8).tobytes() == full["status"].tobytes()
    out = [C.c_void_p(1) for _ in range(6)]
    assert e.lib.mrh_cast_rays(e._ctx, C.byref(p), b.origins.ctypes.data, b.directions.ctypes.data, None, n, None, None, *[C.byref(x) for x in out]) == capi.MRH_OK
    assert out[0].value and out[1].value and all(x.value is None for x in out[2:])


def test_a_cast_only_reads(mixed):
    b, e = mixed.b, mixed.e
    s = rf.inside_out()[0]
    view = (*s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step)
    d0, v0 = e.dump_blocks()
    s0 = e.stats()
    before = e.raycast(*view)
    e.cast_rays(b.origins, b.directions, tmax=b.tmax, **mixed.kw)
    after = e.raycast(*view)
    s1 = e.stats()
    d1, v1 = e.dump_blocks()
    assert d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
    for name, _ in capi.MrhStats._fields_:
        if "ms" not in name:
            assert getattr(s0, name) == getattr(s1, name), name
    assert all(yr.same_bits(x, y) for x, y in zip(before, after)) and np.count_nonzero(before[0]) >= 8


def test_refusals_through_the_c_abi(mixed):
    b, e = mixed.b, mixed.e
    n = 8
    o, d = np.ascontiguousarray(b.origins[:n]), np.ascontiguousarray(b.directions[:n])
    Fp = C.POINTER(C.c_float)
    I, Z = np.eye(3, dtype=F), np.zeros(3, F)
    out = [C.c_void_p() for _ in range(6)]
    refs = [C.byref(x) for x in out]
    call = lambda p, po=o.ctypes.data, pd=d.ctypes.data, cnt=n, R=None, t=None: e.lib.mrh_cast_rays(e._ctx, p, po, pd, None, cnt, R, t, *refs)  # noqa: E731
    ok = capi.MrhRaysParams(0.0, 5.0, 0.0, 7)
    assert call(C.byref(ok)) == capi.MRH_OK
    bad = [capi.MrhRaysParams(0.0, 5.0, 0.0, 8), capi.MrhRaysParams(0.0, 5.0, 0.0, 7, (C.c_uint32 * 4)(0, 0, 0, 1)), capi.MrhRaysParams(-0.1, 5.0, 0.0, 7),
           capi.MrhRaysParams(2.0, 1.0, 0.0, 7), capi.MrhRaysParams(0.0, np.inf, 0.0, 7), capi.MrhRaysParams(0.0, 5.0, -1.0, 7), capi.MrhRaysParams(0.0, 5.0, 1e-6, 7)]
    for p in bad:
        assert call(C.byref(p)) == capi.MRH_ERR_INVALID_ARG, (p.min_range, p.max_range, p.step, p.outputs)
    assert b"2^20 samples" in e.lib.mrh_last_error(e._ctx)
    assert call(None) == capi.MRH_ERR_INVALID_ARG and b"null argument" in e.lib.mrh_last_error(e._ctx)
    assert call(C.byref(ok), po=None) == capi.MRH_ERR_INVALID_ARG
    assert call(C.byref(ok), pd=None) == capi.MRH_ERR_INVALID_ARG
    assert call(C.byref(ok), cnt=capi.RAYS_MAX_RAYS + 1) == capi.MRH_ERR_INVALID_ARG and b"limit 2^24" in e.lib.mrh_last_error(e._ctx)
    assert call(C.byref(ok), R=I.ctypes.data_as(Fp)) == capi.MRH_ERR_INVALID_ARG and b"both null or both set" in e.lib.mrh_last_error(e._ctx)
    nan_R = I.copy()
    nan_R[2, 0] = np.nan
    assert call(C.byref(ok), R=nan_R.ctypes.data_as(Fp), t=Z.ctypes.data_as(Fp)) == capi.MRH_ERR_INVALID_ARG and b"not finite" in e.lib.mrh_last_error(e._ctx)
    assert e.lib.mrh_cast_rays(None, C.byref(ok), o.ctypes.data, d.ctypes.data, None, n, None, None, *refs) == capi.MRH_ERR_INVALID_ARG
    d_o, d_d = hipmem.DeviceBuffer.from_numpy(o), hipmem.DeviceBuffer.from_numpy(d)
    with pytest.raises(capi.MrhError) as ei:
        e.cast_rays_device(d_o.ptr, d_d.ptr, n, 5.0, d_range=_canary(4 * n).ptr)  # no d_status
    assert ei.value.code == capi.MRH_ERR_INVALID_ARG
    # n = 0 succeeds with nothing launched, with and without inputs
    for x in out:
        x.value = 1
    assert call(C.byref(ok), po=None, pd=None, cnt=0) == capi.MRH_OK and all(x.value is None for x in out)
    empty = e.cast_rays(np.zeros((0, 3), F), np.zeros((0, 3), F), 5.0)
    assert empty["range"].shape == (0,) and empty["counts"].shape == (0, 2)
    e.cast_rays_device(0, 0, 0, 5.0, d_range=1, d_status=1)
    sh = capi.Engine(capi.load_hip(), capi.Params(num_sdf_blocks=4096, shard_rank=0, shard_count=2, **mf.PARAMS))
    try:
        with pytest.raises(capi.MrhError) as ei:
            sh.cast_rays(o, d, 5.0)
        assert ei.value.code == capi.MRH_ERR_UNSUPPORTED
    finally:
        sh.close()


# ---- bindings ------------------------------------------------------------------------------------------------------------------

def test_normalize_and_line_of_sight(mixed):
    b, e = mixed.b, mixed.e
    ok = np.all(np.isfinite(b.directions), axis=1) & np.any(b.directions != 0, axis=1)
    d = b.directions
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=F)  # the documented formula, float32 throughout
        unit = (d / ln[:, None]).astype(F)
    assert np.count_nonzero(np.abs(ln[ok] - 1) > 0.04) >= 64  # the batch's directions are not unit vectors
    kw = dict(max_range=b.max_range, min_range=b.min_range, step=b.step)
    got = e.cast_rays(b.origins, d, tmax=b.tmax, normalize=True, **kw)
    want = e.cast_rays(b.origins, unit, tmax=b.tmax, normalize=False, **kw)
    yr.assert_same(got, want, "normalize=True")
    assert np.array_equal(got["status"][~ok], np.full(np.count_nonzero(~ok), capi.RAY_BAD, np.uint8))
    # line of sight: the segments from each origin to its ray's end, or 2 m along it
    sel = np.flatnonzero(ok & np.all(np.isfinite(b.origins), axis=1) & (np.abs(b.origins[:, 0]) < 100))
    length = np.where(np.isfinite(b.tmax[sel]) & (b.tmax[sel] > 0), b.tmax[sel] * ln[sel], F(2.0)).astype(F)
    a = b.origins[sel]
    c = (a + unit[sel] * length[:, None]).astype(F)
    los = e.line_of_sight(a, c)
    seg = (c - a).astype(F)
    seg_len = np.sqrt((seg[:, 0] * seg[:, 0] + seg[:, 1] * seg[:, 1]) + seg[:, 2] * seg[:, 2], dtype=F)
    ref = e.cast_rays(a, seg, max_range=float(seg_len.max()), tmax=seg_len, normals=False, colors=False, counts=False)
    assert los.dtype == bool and np.array_equal(los, ref["status"] == 0)
    assert 4 <= np.count_nonzero(los) <= len(los) - 4, np.count_nonzero(los)
    assert not e.line_of_sight(a[:2], a[:2]).any()  # a segment of length 0 has no direction


def test_geowrapper_cast_rays(monkeypatch):
    """The facade on a sphere fused from depth frames (it has no block import): world rays, and sensor-frame rays at the pose of the
    last setCurrPose, against Engine.cast_rays byte for byte."""
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
        rng = np.random.default_rng(4)
        n = 300
        o = rng.uniform([-0.2, -0.2, 0.0], [0.2, 0.2, 0.3], (n, 3)).astype(F)
        d = (rng.uniform([-0.3, -0.3, 0.9], [0.3, 0.3, 1.1], (n, 3)) * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
        tmax = rng.uniform(0.3, 3.0, n).astype(F)
        names = ("range", "status", "normals", "rgb", "counts", "first_unknown")
        for normalize in (True, False):
            got = dict(zip(names, g.castRays(o, d, 2.5, 0.05, 0.0, tmax, normalize=normalize)))
            want = e.cast_rays(o, d, 2.5, 0.05, 0.0, tmax=tmax, normalize=normalize)
            yr.assert_same(got, want, "GeoWrapper.castRays, normalize=%s" % normalize)
            assert np.count_nonzero(got["status"] & capi.RAY_HIT) >= 30 and np.count_nonzero(got["counts"][:, 0]) >= 30
        q = np.array([0.3, -0.5, 0.2, 0.7])
        g.setCurrPose(np.array([0.05, -0.1, 0.2], F), (q / np.linalg.norm(q)).astype(F))
        pose = g.getCurrPose()
        R, t = pose[:3, :3].copy(), pose[:3, 3].copy()
        got = dict(zip(names, g.castRays(o, d, 2.5, sensor_frame=True)))
        yr.assert_same(got, e.cast_rays(o, d, 2.5, R=R, t=t), "GeoWrapper.castRays, sensor frame")
        assert g.castRays(np.zeros((0, 3), F), np.zeros((0, 3), F), 1.0)[0].shape == (0,)
        with pytest.raises(RuntimeError, match=r"GeoWrapper::castRays\|"):
            g.castRays(np.zeros((4, 2), F), np.zeros((4, 3), F), 1.0)
    finally:
        e.close()
        del g
