"""Scan normals on the GPU (mrh_normals.h, include/mrhash_normals.h) against the numpy restatement of DESIGN.md D12
(tests/normals_ref.py): the same bytes for every point and the same counts, through all three entry points; the
normal-direction SDF fed by the estimate builds the map the oracle builds from the restatement's normals; nothing else changes."""
import numpy as np
import pytest

import normals_ref as nr
import parity_utils as pu
from mrhash_amd import capi, hipmem, synth

pytestmark = pytest.mark.gpu
IDENT = (np.zeros(3, np.float32), np.array([0, 0, 0, 1], np.float32))


def _engine(lib, blocks=4096, **over):
    p = dict(synth.VBR_PARAMS, **over)
    e = capi.Engine(lib, capi.Params(num_sdf_blocks=blocks, **p))
    e.set_camera(1.0, 1.0, 0.0, 0.0, 1, 1, p["min_depth"], 100.0, model=1)
    e.set_pose(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    return e


def _scan(rows=128, cols=1024, noise=0.0, dropout=0.0):
    return synth.lidar_scan(synth.street_canyon(), *IDENT, rows=rows, cols=cols, noise_sigma=noise, max_range=100.0, dropout=dropout)


_PARAMS = {
    "noiseless": {}, "noisy": {}, "dropout_32x512": {}, "shuffled": {}, "translated_rho0.8": dict(radius=0.8),
    "rho0.1_min12": dict(radius=0.1, min_points=12), "gates": dict(min_spread=0.125, max_flatness=0.02), "empty": {}, "one": {},
    "tiled_1000003": {},
}
_scans = {}


def _case(name):
    """(points, parameters) of a named case; the scans are made once"""
    if "noisy" not in _scans:
        _scans["noisy"] = _scan(noise=0.02)
    noisy = _scans["noisy"]
    if name == "noiseless":
        pts = _scan()
    elif name == "dropout_32x512":
        pts = _scan(32, 512, dropout=0.1)
    elif name == "shuffled":  # an unorganised cloud
        pts = noisy[np.random.default_rng(1).permutation(len(noisy))]
    elif name == "translated_rho0.8":
        pts = noisy + np.array([-7000.0, 9000.0, 3.0], np.float32)
    elif name == "empty":
        pts = np.zeros((0, 3), np.float32)
    elif name == "one":
        pts = np.array([[4.0, -1.0, 0.5]], np.float32)
    elif name == "tiled_1000003":  # the scan eight times over, each copy with its own jitter
        big = np.tile(noisy, (8, 1))[:1_000_003]
        pts = (big + np.random.default_rng(2).normal(0.0, 0.01, size=big.shape)).astype(np.float32)
    else:
        pts = noisy
    return pts, _PARAMS[name]


@pytest.fixture(scope="module")
def engine(hip):
    e = _engine(hip)
    yield e
    e.close()


@pytest.mark.parametrize("name", list(_PARAMS))
def test_every_entry_point_gives_the_bytes_of_the_restatement(engine, name):
    pts, par = _case(name)
    want = nr.restate(pts, **par)
    e = engine
    # the current scan, uploaded
    e.upload_points(pts)
    info = e.estimate_normals(info=True, **par)
    got, info2 = e.get_normals()
    assert info == want.info and info2 == want.info
    assert got.shape == want.normals.shape and got.tobytes() == want.normals.tobytes()
    # the current scan, in device memory; the counts are picked up later, by get_normals
    d_pts = hipmem.DeviceBuffer.from_numpy(pts)
    e.set_points_device(d_pts.ptr, len(pts))
    assert e.estimate_normals(**par) is None
    got, info2 = e.get_normals()
    assert info2 == want.info and got.tobytes() == want.normals.tobytes()
    # caller's buffers on both sides
    d_out = hipmem.DeviceBuffer(max(pts.nbytes, 4))
    e.estimate_normals_device(d_pts.ptr, len(pts), d_out.ptr, **par)
    e.sync()
    assert d_out.to_numpy(np.float32, 3 * len(pts)).tobytes() == want.normals.tobytes()
    e.upload_points(np.zeros((0, 3), np.float32))  # the device buffer goes away with this test
    if name in ("noiseless", "noisy"):
        assert want.info["estimated"] > 0.8 * len(pts) and want.info["cells"] > 15000


def test_the_plain_accumulation_gives_the_same_bytes(hip, monkeypatch):
    """MRH_NORMALS_FOLD=0: every point adds its own sums to its cell instead of one lane per run of equal cells."""
    monkeypatch.setenv("MRH_NORMALS_FOLD", "0")
    e = _engine(hip)
    for name in ("noisy", "dropout_32x512", "shuffled", "rho0.1_min12"):
        pts, par = _case(name)
        want = nr.restate(pts, **par)
        e.upload_points(pts)
        assert e.estimate_normals(info=True, **par) == want.info
        assert e.get_normals()[0].tobytes() == want.normals.tobytes()
    e.close()


def test_arguments_and_state(hip):
    e = _engine(hip)
    with pytest.raises(capi.MrhError) as ei:
        e.estimate_normals()  # no scan yet
    assert ei.value.code == capi.MRH_ERR_STATE
    pts = _scan(32, 512)
    e.upload_points(pts)
    for bad in (dict(radius=-1.0), dict(radius=float("nan")), dict(min_spread=float("inf")), dict(max_flatness=1.0), dict(max_flatness=-0.5)):
        with pytest.raises(capi.MrhError) as ei:
            e.estimate_normals(**bad)
        assert ei.value.code == capi.MRH_ERR_INVALID_ARG, bad
    with pytest.raises(capi.MrhError) as ei:
        e.estimate_normals_device(0, 10, 0)
    assert ei.value.code == capi.MRH_ERR_INVALID_ARG
    d = hipmem.DeviceBuffer(64)
    with pytest.raises(capi.MrhError) as ei:
        e.estimate_normals_device(d.ptr, 1 << 24, d.ptr)
    assert ei.value.code == capi.MRH_ERR_CAPACITY
    e.estimate_normals_device(0, 0, 0)  # n = 0 is fine
    # normals that were uploaded come back as they were, with no counts
    up = synth.scan_normals(pts)
    e.upload_normals(up)
    got, info = e.get_normals()
    assert got.tobytes() == up.tobytes() and info == dict(points=0, estimated=0, fallback=0, missing=0, cells=0)
    e.close()


def _drive(n=6, rows=32, cols=512, noise=0.02):
    scene = synth.street_canyon()
    rng = np.random.default_rng(0)
    for t, q in synth.drive_poses(n):
        yield t, q, synth.lidar_scan(scene, t, q, rows=rows, cols=cols, noise_sigma=noise, rng=rng)


def test_normal_direction_sdf_from_estimated_normals_matches_the_oracle(hip, oracle):
    over = dict(projective_sdf=False, min_weight_threshold=1)
    a, b, c = _engine(hip, 131072, **over), _engine(hip, 131072, **over), _engine(oracle, 131072, **over)
    for t, q, pts in _drive():
        want = nr.restate(pts).normals
        for e in (a, b, c):
            e.set_pose(synth.quat_to_rot(q), t)
            e.upload_points(pts)
        a.estimate_normals()
        b.upload_normals(want)
        c.upload_normals(want)
        for e in (a, b, c):
            assert not e.integrate_points()
    a.sync(), b.sync()
    (da, va), (db, vb) = a.dump_blocks(), b.dump_blocks()
    assert len(da) > 800 and da.tobytes() == db.tobytes() and va.tobytes() == vb.tobytes()
    r = pu.compare_maps(a, c)
    assert r["weighted"] > 10000 and r["sdf_bit_exact"] and r["sumsq_bit_exact"]
    m = pu.compare_meshes(a, c)
    assert m["triangles"] > 0 and m["pos_bit_exact"]
    for e in (a, b, c):
        e.close()


def test_estimating_changes_nothing_else(hip):
    """On a projective map nobody reads the normals: a run that estimates them between its scans builds the same map, stats
    and error flags as one that does not."""
    runs = []
    for estimate in (False, True):
        e = _engine(hip, 131072, min_weight_threshold=1, n_frames_invalidate_voxels=3)
        for t, q, pts in _drive():
            e.set_pose(synth.quat_to_rot(q), t)
            e.upload_points(pts)
            if estimate:
                e.estimate_normals()
            assert not e.integrate_points()
            if estimate:
                e.estimate_normals(radius=0.3)
        e.sync()
        s = e.stats()
        skip = ("last_integrate_kernel_ms", "sum_integrate_kernel_ms", "last_mc_count_ms", "last_mc_emit_ms", "sum_front_kernel_ms")
        runs.append((e.dump_blocks(), {k: getattr(s, k) for k, _ in s._fields_ if k not in skip}, e.peek_error_flags()))
        e.close()
    (d0, v0), s0, f0 = runs[0]
    (d1, v1), s1, f1 = runs[1]
    assert len(d0) > 800 and d0.tobytes() == d1.tobytes() and v0.tobytes() == v1.tobytes()
    assert s0 == s1 and f0 == f1 == 0


def test_the_wrapper_estimates_when_asked(monkeypatch, tmp_path):
    """GeoWrapper(projective_sdf=False).setPointCloud(points, True); compute(): the normals are the restatement's, and the mesh
    is the one the (points, normals) overload builds from them."""
    monkeypatch.setenv("MRHASH_NUM_SDF_BLOCKS", "131072")
    from mrhash.src.pygeowrapper import GeoWrapper

    p = synth.VBR_PARAMS
    meshes = []
    for estimate in (True, False):
        g = GeoWrapper(sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=0.0, integration_weight_sample=1,
                       virtual_voxel_size=p["virtual_voxel_size"], n_frames_invalidate_voxels=0, voxel_extents_scale=1,
                       viewer_active=False, marching_cubes_threshold=1.5, min_weight_threshold=1, min_depth=0.2,
                       max_depth=100.0, projective_sdf=False)
        g.setCamera(1.0, 1.0, 0.0, 0.0, 1, 1, 0.2, 100.0, 1)
        for t, q, pts in _drive(3):
            want = nr.restate(pts).normals
            g.setCurrPose(t, q)
            if estimate:
                g.setPointCloud(pts, True)
                g.compute()
                got = g.getNormals()
                assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()
                assert g.getNormals().tobytes() == want.tobytes()  # the second call needs no read-back
            else:
                g.setPointCloud(pts, want)
                g.compute()
        g.extractMesh(str(tmp_path / f"n{int(estimate)}.ply"))
        meshes.append((g.getVertices(), g.getFaces()))
    assert len(meshes[0][1]) > 200
    assert np.array_equal(meshes[0][0], meshes[1][0]) and np.array_equal(meshes[0][1], meshes[1][1])
