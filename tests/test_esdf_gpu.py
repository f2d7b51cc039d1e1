"""GPU half of the distance field (mrh_esdf.h, include/mrhash_esdf.h): bit-exact against the restatement of
tests/esdf_ref.py on hand-built single- and multi-resolution maps, on a fused map and far from the origin, accurate against the
analytic sphere, free of side effects on the frame path, and reachable through the device variant and the GeoWrapper facade."""
import ctypes as C

import numpy as np
import pytest

import esdf_ref as er
import parity_utils as pu
import raycast_ref as rr
from mrhash_amd import capi, hipmem, synth

pytestmark = pytest.mark.gpu

K = synth.REPLICA_640
PARAMS = er.SPHERE_PARAMS
VS = np.float32(PARAMS["virtual_voxel_size"])
R_SPHERE = 12


def _engine(blocks, params=PARAMS, num_sdf_blocks=4096):
    e = pu.make_engine(capi.load_hip(), synth.CFG1, params, num_sdf_blocks)
    e.import_blocks(*er.to_import(blocks))
    return e


def _ref_map(e, params):
    d, v = e.dump_blocks()
    return rr.make_map(params, d, v)


def _check(e, m, origin, dims, R, **kw):
    """The GPU field of the box against the restatement on the map m, bit for bit; returns the GPU's (dist, state, d2)."""
    got = e.esdf(origin, dims, R, squared=True, **kw)
    want = er.esdf(m, origin, dims, R, **kw)
    for a, b, what in zip(got, want, ("dist", "state", "d2")):
        assert a.shape == (dims[2], dims[1], dims[0])
        assert er.same_bits(a, b), f"{what} differs at {int((a != b).sum())} of {a.size} cells (box {origin} {dims}, R {R})"
    return got


@pytest.fixture(scope="module")
def sphere():
    e = _engine(er.sphere_blocks())
    m = _ref_map(e, PARAMS)
    yield e, m
    e.close()


def test_sphere_is_bit_exact(sphere):
    e, m = sphere
    origin, dims = er.SPHERE_BOX
    dist, state, d2 = _check(e, m, origin, dims, R_SPHERE)
    assert np.any(state & er.SITE) and np.any(state & er.FAR) and np.any(state & er.INSIDE) and np.any((state & er.OBSERVED) == 0)


def test_sphere_accuracy(sphere):
    """Cells that are not far and whose true distance is within (R - 1) vs of the surface: |dist - (|p - c| - r)| <= vs + 1e-5.
    Derived: the cell that contains the nearest surface point is within sqrt(3)/2 vs of it, inside the band, so it is a site; and
    every site has the surface within vs.  The restatement reaches 0.985 vs on this input and compares 49 % of the box."""
    e, _ = sphere
    origin, dims = er.SPHERE_BOX
    dist, state, _ = e.esdf(origin, dims, R_SPHERE)
    true = np.linalg.norm(er.cells(origin, dims).astype(np.float64) * float(VS) - er.SPHERE_C, axis=-1) - er.SPHERE_R
    sel = ((state & er.FAR) == 0) & (np.abs(true) <= (R_SPHERE - 1) * float(VS))
    err = np.abs(dist.astype(np.float64) - true)[sel]
    print("sphere: %.1f %% of the box compared, max error %.4f vs" % (100.0 * sel.mean(), err.max() / float(VS)))
    assert sel.mean() >= 0.40, sel.mean()
    assert err.max() <= float(VS) + 1e-5, err.max() / float(VS)


@pytest.mark.parametrize("origin,dims,R", [
    ((-256, -1, -1), (512, 3, 2), 300),
    ((-1, -256, -1), (3, 512, 2), 300),
    ((-1, -1, -256), (2, 3, 512), 300),
    ((7, 0, 0), (1, 1, 1), 12),          # on a site
    ((100, 100, 100), (1, 1, 1), 12),    # on an absent block
    ((-32, -4, -4), (65, 9, 9), 1),
    ((-32, -4, -4), (65, 9, 9), 4095),
    ((100, 100, 100), (24, 24, 24), 12),  # all unknown, all far
])
def test_shapes_where_a_kernel_can_go_wrong(sphere, origin, dims, R):
    e, m = sphere
    dist, state, d2 = _check(e, m, origin, dims, R)
    if origin == (7, 0, 0):
        assert state[0, 0, 0] & er.SITE and d2[0, 0, 0] == 0
    if origin[0] == 100:
        assert np.all(state == er.FAR) and np.all(d2 == er.FAR_D2) and np.all(dist == VS * np.float32(R))
    if dims[0] == 65:
        assert np.any(state & er.SITE)


@pytest.mark.parametrize("where", ["first", "last", "centre"])
def test_one_site_in_a_40_cube(where):
    origin, n = np.array([-13, 5, -22]), 40
    s = {"first": origin, "last": origin + n - 1, "centre": origin + n // 2}[where]
    e = _engine(er.site_blocks([s]))
    try:
        dist, state, d2 = _check(e, _ref_map(e, PARAMS), tuple(origin), (n, n, n), 100)
        assert np.array_equal(d2, ((er.cells(origin, (n, n, n)) - s) ** 2).sum(-1))
        assert np.count_nonzero(state & er.SITE) == 1
    finally:
        e.close()


def test_band_weight_and_output_flags():
    """surface_band = 0.02 and min_weight = 2 on a map with weights 1 and 3; every combination of the optional outputs: a NULL
    pointer or a missing flag means "not produced", and the pointer handed back is NULL."""
    blocks = er.sphere_blocks()
    for k, v in blocks.items():
        v["weight"] = np.where((np.arange(512) + sum(k)) % 3 == 0, 1, 3)
    e = _engine(blocks)
    try:
        m = _ref_map(e, PARAMS)
        origin, dims = er.SPHERE_BOX
        want = _check(e, m, origin, dims, R_SPHERE, surface_band=0.02, min_weight=2)
        plain = er.esdf(m, origin, dims, R_SPHERE)
        assert not er.same_bits(want[1], plain[1]) and 0 < np.count_nonzero(want[1] & er.SITE) < np.count_nonzero(plain[1] & er.SITE)
        n = dims[0] * dims[1] * dims[2]
        for flags in range(4):
            for give_s in (False, True):
                for give_q in (False, True):
                    p = capi.MrhEsdfParams((C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims), R_SPHERE, 2, 0.02, flags)
                    pd, ps, pq = C.c_void_p(), C.c_void_p(1), C.c_void_p(1)
                    rc = e.lib.mrh_esdf(e._ctx, C.byref(p), C.byref(pd), C.byref(ps) if give_s else None, C.byref(pq) if give_q else None)
                    assert rc == capi.MRH_OK
                    got = np.frombuffer((C.c_char * (4 * n)).from_address(pd.value), dtype=np.float32)
                    assert er.same_bits(got, want[0].ravel())
                    if give_s and flags & capi.ESDF_STATE:
                        assert np.array_equal(np.frombuffer((C.c_char * n).from_address(ps.value), dtype=np.uint8), want[1].ravel())
                    elif give_s:
                        assert ps.value is None
                    if give_q and flags & capi.ESDF_SQUARED:
                        assert np.array_equal(np.frombuffer((C.c_char * (4 * n)).from_address(pq.value), dtype=np.uint32), want[2].ravel())
                    elif give_q:
                        assert pq.value is None
        dist, state, d2 = e.esdf(origin, dims, R_SPHERE, surface_band=0.02, min_weight=2, state=False, squared=False)
        assert state is None and d2 is None and er.same_bits(dist, want[0])
    finally:
        e.close()


def test_multi_resolution():
    """Four coarse blocks (resolution 1, 64 voxels) next to fine ones, carrying the same sphere."""
    params = dict(PARAMS, sdf_var_threshold=0.005)
    blocks = dict(er.sphere_blocks(params))
    coarse = [(0, 0, 0), (-1, 0, 0), (0, -1, -1), (-1, -1, 0)]
    lin = np.arange(64)
    for b in coarse:
        assert b in blocks
        v = np.stack([b[0] * 8 + 2 * (lin % 4), b[1] * 8 + 2 * ((lin // 4) % 4), b[2] * 8 + 2 * (lin // 16)], -1)
        vox = np.zeros(64, capi.VOXEL_DTYPE)
        vox["sdf"], vox["weight"] = er.sphere_sdf(params["virtual_voxel_size"], params["sdf_truncation"], v)[0], 1
        blocks[b] = (1, vox)
    e = _engine(blocks, params)
    try:
        d, _ = e.dump_blocks()
        assert int((d["resolution"] == 1).sum()) == 4
        m = _ref_map(e, params)
        origin, dims = er.SPHERE_BOX
        dist, state, d2 = _check(e, m, origin, dims, R_SPHERE)
        _, res, _, _ = er.lookup(m, origin, dims)
        assert np.any((res == 1) & ((state & er.SITE) != 0)), "no site cell lies in a coarse block"
        assert np.any((res == 0) & ((state & er.SITE) != 0))
        _check(e, m, (-3, -9, -2), (13, 11, 7), 3)  # a small box across a coarse / fine face
    finally:
        e.close()


# ---- a fused map ----------------------------------------------------------------------------------------------------------

def _box_on_two_walls(d, dims):
    """A box of `dims` cells laid over the fused blocks d so that it holds surface of two walls: per axis the block layer with
    the most fused blocks is taken as that axis' wall; the two axes with the fullest layers get their wall a quarter of the
    box's side away from the box's outer face, the third axis is centred on the blocks both walls share (else on the first
    wall's).  The caller asserts what the choice is meant to achieve."""
    b = np.stack([d["x"], d["y"], d["z"]], -1).astype(np.int64)
    layer, count = [], []
    for a in range(3):
        vals, cnt = np.unique(b[:, a], return_counts=True)
        layer.append(int(vals[np.argmax(cnt)]))
        count.append(int(cnt.max()))
    walls = sorted(np.argsort(count)[-2:])
    free = ({0, 1, 2} - set(walls)).pop()
    origin = [0, 0, 0]
    for a in walls:
        w = layer[a] * 8 + 4
        room_is_above = np.median(b[:, a]) * 8 > w
        origin[a] = w - (dims[a] // 4 if room_is_above else dims[a] - dims[a] // 4)
    on = (b[:, walls[0]] == layer[walls[0]])
    both = on & (b[:, walls[1]] == layer[walls[1]])
    pick = b[both] if both.any() else b[on]
    origin[free] = int(np.median(pick[:, free])) * 8 + 4 - dims[free] // 2
    return tuple(int(x) for x in origin), walls


def _wall_axes(state):
    """Axes along which some layer of the box is a wall: at least 30 % of the layer's cells are sites."""
    site = (state & er.SITE) != 0
    out = []
    for a, ax in ((0, 2), (1, 1), (2, 0)):  # axis x is array axis 2
        other = tuple(i for i in range(3) if i != ax)
        if (site.mean(axis=other) >= 0.30).any():
            out.append(a)
    return out


@pytest.fixture(scope="module")
def replica_map():
    params = dict(synth.REPLICA_PARAMS)
    e = pu.make_engine(capi.load_hip(), K, params, 131072)
    for f in synth.replica_stream(20):
        pu.feed(e, f)
    yield e, params
    e.close()


def test_fused_map_is_bit_exact(replica_map):
    e, params = replica_map
    d, v = e.dump_blocks()
    m = rr.make_map(params, d, v)
    dims = (96, 64, 48)
    origin, walls = _box_on_two_walls(d, dims)
    dist, state, d2 = _check(e, m, origin, dims, 32)  # min_weight 0: the context's threshold, 5
    frac = float(((state & er.SITE) != 0).mean())
    print("fused: box", origin, "walls on axes", walls, "sites %.3f" % frac, "wall axes found", _wall_axes(state))
    assert len(_wall_axes(state)) >= 2, "the box does not hold fused surface on two walls"
    assert 0.01 <= frac <= 0.50, frac


@pytest.mark.parametrize("bx0", [40000, 600000])
def test_far_from_the_origin(bx0):
    """Two adjacent blocks at block (bx0, -3, 7), where voxel -> block is the float detour and k_esdf_classify takes get_voxel_i per
    cell.  40000 is beyond the block_shift_limit mrh_create finds for a 2 cm voxel; 600000 puts the voxels above 2^22, which that
    limit can never reach (Map::block_shift_limit <= 2^22), so the per-cell path is taken whatever the probe found.  Observed,
    site and the site's sdf equal mrh_get_voxel cell by cell; the whole result equals the restatement."""
    params = dict(synth.CFG1_PARAMS, min_weight_threshold=1)
    vs, trunc = np.float32(params["virtual_voxel_size"]), np.float32(params["sdf_truncation"])
    rng = np.random.default_rng(5)
    blocks = {}
    for bx in (bx0, bx0 + 1):
        vox = np.zeros(512, capi.VOXEL_DTYPE)
        vox["sdf"] = rng.uniform(-trunc, trunc, 512).astype(np.float32)
        vox["sdf"][rng.integers(0, 512, 60)] = rng.uniform(-vs, vs, 60).astype(np.float32)
        vox["weight"] = rng.integers(0, 4, 512)
        blocks[(bx, -3, 7)] = vox
    e = _engine(blocks, params)
    try:
        origin, dims = (bx0 * 8 + 2, -25, 55), (12, 10, 9)
        dist, state, d2 = _check(e, _ref_map(e, params), origin, dims, 20)
        assert np.any(state & er.SITE) and np.any((state & er.OBSERVED) == 0)
        for k in range(dims[2]):
            for j in range(dims[1]):
                for i in range(dims[0]):
                    vox, found = e.get_voxel(origin[0] + i, origin[1] + j, origin[2] + k)
                    obs = found and int(vox["weight"]) >= 1
                    site = obs and abs(np.float32(vox["sdf"])) <= vs
                    assert bool(state[k, j, i] & er.OBSERVED) == obs and bool(state[k, j, i] & er.SITE) == site, (i, j, k)
                    if site:
                        assert dist[k, j, i].tobytes() == np.float32(vox["sdf"]).tobytes()
    finally:
        e.close()


# ---- reader contract, device variant, facade ------------------------------------------------------------------------------

def test_esdf_leaves_the_frame_path_alone():
    hip = capi.load_hip()
    params = dict(synth.REPLICA_PARAMS)
    frames = list(synth.replica_stream(8))
    a = pu.make_engine(hip, K, params, 65536)
    b = pu.make_engine(hip, K, params, 65536)
    dims = (48, 40, 32)
    try:
        for f in frames[:4]:
            pu.feed(a, f)
            pu.feed(b, f)
        origin, _ = _box_on_two_walls(b.dump_blocks()[0], dims)
        pu.feed(a, frames[4])
        pu.feed(b, frames[4])
        got = a.esdf(origin, dims, 8, min_weight=1, squared=True)  # between two frames of the pipelined stream, no sync
        d, v = a.dump_blocks()
        want = er.esdf(rr.make_map(params, d, v), origin, dims, 8, min_weight=1)
        assert all(er.same_bits(x, y) for x, y in zip(got, want)) and np.any(got[1] & er.SITE)
        for f in frames[5:]:
            pu.feed(a, f)
            a.esdf(origin, dims, 8)
            pu.feed(b, f)
        r = pu.compare_maps(a, b, tol=0.0)
        assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
        pu.compare_meshes(a, b, tol=0.0)
        # counters, the camera and the last extraction survive the call
        tris = a.extract_triangles()
        V, F, Cc = a.extract_mesh()
        s0 = a.stats()
        a.esdf(origin, dims, 8)
        s1 = a.stats()
        V2, F2, C2 = a.extract_mesh()
        assert er.same_bits(V, V2) and np.array_equal(F, F2) and er.same_bits(Cc, C2)
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


def test_arguments_and_a_sharded_context(sphere):
    e, _ = sphere
    good = dict(origin=(0, 0, 0), dims=(8, 8, 8), max_distance_voxels=4)
    bad = [dict(dims=(0, 8, 8)), dict(dims=(8, 513, 8)), dict(max_distance_voxels=0), dict(max_distance_voxels=4096),
           dict(origin=(-(1 << 23) - 1, 0, 0)), dict(origin=((1 << 23) - 4, 0, 0)), dict(surface_band=-0.01), dict(surface_band=float("nan")),
           dict(surface_band=float("inf")), dict(min_weight=-1)]
    for over in bad:
        with pytest.raises(capi.MrhError) as ei:
            e.esdf(**{**good, **over})
        assert ei.value.code == capi.MRH_ERR_INVALID_ARG, over
    p = capi.MrhEsdfParams((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8), 4, 0, 0.0, 4)  # an unknown output bit
    assert e.lib.mrh_esdf(e._ctx, C.byref(p), None, None, None) == capi.MRH_ERR_INVALID_ARG
    with pytest.raises(capi.MrhError) as ei:
        e.esdf_device(**good)  # no d_dist
    assert ei.value.code == capi.MRH_ERR_INVALID_ARG
    e.esdf((-(1 << 23), 0, 0), (4, 1, 1), 1)  # the limits themselves are inside
    e.esdf(((1 << 23) - 4, 0, 0), (4, 1, 1), 4095)
    s = capi.Engine(capi.load_hip(), capi.Params(num_sdf_blocks=4096, shard_rank=0, shard_count=2, **PARAMS))
    try:
        with pytest.raises(capi.MrhError) as ei:
            s.esdf(**good)
        assert ei.value.code == capi.MRH_ERR_UNSUPPORTED
    finally:
        s.close()


def test_device_variant_equals_the_host_call(sphere):
    e, _ = sphere
    origin, dims = er.SPHERE_BOX
    want = e.esdf(origin, dims, R_SPHERE, squared=True)
    n = dims[0] * dims[1] * dims[2]
    dd, ds, dq = hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(n), hipmem.DeviceBuffer(4 * n)
    e.esdf_device(origin, dims, R_SPHERE, d_dist=dd.ptr, d_state=ds.ptr, d_d2=dq.ptr)
    e.sync()
    assert er.same_bits(dd.to_numpy(np.float32), want[0].ravel())
    assert np.array_equal(ds.to_numpy(np.uint8), want[1].ravel())
    assert np.array_equal(dq.to_numpy(np.uint32), want[2].ravel())
    d2 = hipmem.DeviceBuffer(4 * n)
    e.esdf_device(origin, dims, R_SPHERE, d_dist=d2.ptr)  # state and d2 skipped
    e.esdf_device((-3, -9, -2), (13, 11, 7), 3, d_dist=dd.ptr)  # a smaller box right behind it reuses the scratch
    e.sync()
    assert er.same_bits(d2.to_numpy(np.float32), want[0].ravel())
    assert er.same_bits(dd.to_numpy(np.float32, 13 * 11 * 7), e.esdf((-3, -9, -2), (13, 11, 7), 3)[0].ravel())


def test_geowrapper_distance_field(monkeypatch):
    """The facade on a sphere fused from depth frames (it has no block import): the box follows the rounding rule and the field is
    the engine's."""
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
        lo, hi = np.array([-0.31, -0.294, 0.805], np.float32), np.array([0.305, 0.31, 1.295], np.float32)
        dist, state, origin, dims = g.distanceField(lo, hi, 0.6)
        vs = np.float64(np.float32(p["virtual_voxel_size"]))
        first, last = np.floor(lo.astype(np.float64) / vs + 0.5), np.floor(hi.astype(np.float64) / vs + 0.5)
        assert origin == tuple(int(x) for x in first) and dims == tuple(int(x) for x in last - first + 1)
        R = int(np.ceil(np.float64(np.float32(0.6)) / vs))
        want = e.esdf(origin, dims, R)
        assert dist.shape == (dims[2], dims[1], dims[0]) and state.dtype == np.uint8
        assert er.same_bits(dist, want[0]) and np.array_equal(state, want[1]) and np.any(state & er.SITE)
        with pytest.raises(RuntimeError, match=r"GeoWrapper::distanceField\|"):
            g.distanceField(lo, lo - 0.1, 0.6)
        with pytest.raises(RuntimeError, match=r"GeoWrapper::distanceField\|"):
            g.distanceField(lo, lo + np.float32(0.02 * 513), 0.6)
    finally:
        e.close()
        del g
