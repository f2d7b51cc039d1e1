"""GPU half of the free-space layer (mrh_freespace.h, include/mrhash_freespace.h): every comparison is byte for
byte against the restatement of tests/freespace_ref.py, through freespace_box over the whole layer — the two carves on hand-made
images and clouds, union / idempotence / order on the device, the box reader on hand-built maps, the segments, the frame path
left alone, and line_of_sight_free on the fused room."""
import ctypes as C

import numpy as np
import pytest

import esdf_ref as er
import freespace_ref as fr
import parity_utils as pu
import raycast_ref as rr
import rays_ref as yr
from mrhash_amd import capi, hipmem, synth

pytestmark = pytest.mark.gpu

F = np.float32
PARAMS = synth.CFG1_PARAMS
VS = F(PARAMS["virtual_voxel_size"])  # 0.02
I3, Z3 = np.eye(3, dtype=F), np.zeros(3, F)
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], F)  # a rotation with no zero where it matters
Z_TO_X = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], F)                       # the camera's z axis onto world x
MIN_D, MAX_D = 0.1, 1.5
CAM = (20.0, 24.0, 11.5, 7.5)  # fx, fy, cx, cy of the 16 x 24 image: a wide fan


def _image():
    """16 x 24 depths in 0.3 .. 1.3 m with one of each special value."""
    rng = np.random.default_rng(7)
    d = rng.uniform(0.3, 1.3, (16, 24)).astype(F)
    d[0, 0], d[0, 1], d[3, 5], d[4, 4], d[9, 20], d[15, 23], d[8, 8] = np.nan, 0.0, MIN_D, 0.05, 2.0, np.inf, -1.0
    return d


IMAGE = _image()
# (R, t): identity; a general rotation; outside the small layers, looking through them; so far out that samples fail the bound
POSES = [(I3, np.array([0.01, -0.02, -0.3], F)), (ROT, np.array([0.05, -0.02, 0.03], F)), (I3, np.array([0.0, 0.0, -1.0], F)),
         (Z_TO_X, np.array([20971.0, 0.0, 0.0], F))]
LAYERS = [((-20, -20, -20), (40, 40, 40)), ((-17, 0, -30), (33, 1, 65)), ((-1, -1, 2), (1, 1, 1))]


@pytest.fixture(scope="module")
def empty():
    """A context with an empty map: the carves and the layer bit of the box reader need no map."""
    e = pu.make_engine(capi.load_hip(), synth.CFG1, PARAMS, 4096)
    yield e
    e.close()


def _bits(e, layer_or_origin, dims=None):
    """The layer's bits [nz, ny, nx] through freespace_box over exactly its box."""
    origin = layer_or_origin.origin if dims is None else layer_or_origin
    dims = layer_or_origin.dims if dims is None else dims
    return (e.freespace_box(tuple(int(x) for x in origin), tuple(int(x) for x in dims)) & capi.FREE_FREE) != 0


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} cells differ"


@pytest.mark.parametrize("shift", [0, 1, 3])
@pytest.mark.parametrize("origin,dims", LAYERS)
def test_depth_carve_equals_the_restatement(empty, origin, dims, shift):
    e = empty
    e.freespace_create(origin, dims, shift)
    total = 0
    for pi, (R, t) in enumerate(POSES):
        for margin in (0.0, 0.05):
            e.freespace_clear()
            e.freespace_carve_depth(IMAGE, *CAM, R, t, MIN_D, MAX_D, margin=margin)
            want = fr.carve_depth(fr.Layer(origin, dims, shift), VS, IMAGE, *CAM, R, t, MIN_D, MAX_D, margin=margin)
            got = _bits(e, want)
            _same(got, want.bits, f"pose {pi}, margin {margin}")
            total += int(got.sum())
            if pi == 3:
                assert not got.any()  # everything the far camera sees of the layer's neighbourhood is beyond the bound or outside
    # a step larger than a cell (2.5 cells): cells are skipped
    step = float(F(2.5) * (VS * F(1 << shift)))
    e.freespace_clear()
    e.freespace_carve_depth(IMAGE, *CAM, *POSES[1], MIN_D, MAX_D, step=step)
    want = fr.carve_depth(fr.Layer(origin, dims, shift), VS, IMAGE, *CAM, *POSES[1], MIN_D, MAX_D, step=step)
    _same(_bits(e, want), want.bits, "explicit step")
    if dims == (40, 40, 40):
        assert total > 1000 and 0 < want.bits.sum() < fr.carve_depth(fr.Layer(origin, dims, shift), VS, IMAGE, *CAM, *POSES[1], MIN_D, MAX_D).bits.sum()
    if dims == (1, 1, 1) and shift == 3:
        assert total > 0  # the one cell (voxels -8 .. -1, -8 .. -1, 16 .. 23) is in front of the first camera


def _cloud(n, seed=3):
    """n sensor-frame points 0.2 .. 2 m out (beyond max_depth: carved to max_depth), the first ones replaced by the special cases."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)).astype(F)
    p = (p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0.2, 2.0, (n, 1))).astype(F)
    special = np.array([[0, 0, 0], [np.nan, 0.3, 0.3], [np.inf, 0, 0], [0.05, 0.05, 0.0], [0.0, 0.0, 1.9], [0.3, -np.inf, 0.1]], F)
    k = min(n, len(special)) if n >= 64 else 0
    p[:k] = special[:k]
    return p


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_points_carve_equals_the_restatement(empty, n):
    e = empty
    origin, dims, shift = (-20, -20, -20), (40, 40, 40), 1
    e.freespace_create(origin, dims, shift)
    pts = _cloud(n)
    for R, t, margin in ((I3, Z3, 0.0), (ROT, POSES[1][1], 0.05)):
        e.freespace_clear()
        e.freespace_carve_points(pts, R, t, MIN_D, MAX_D, margin=margin)
        want = fr.carve_points(fr.Layer(origin, dims, shift), VS, pts, R, t, MIN_D, MAX_D, margin=margin)
        got = _bits(e, want)
        _same(got, want.bits, f"{n} points, margin {margin}")
        assert bool(got.any()) == (n > 0)
        if n >= 64:  # the same cloud in another order, through the device form
            e.freespace_clear()
            shuffled = np.ascontiguousarray(pts[np.random.default_rng(5).permutation(n)])
            d_p = hipmem.DeviceBuffer.from_numpy(shuffled)
            e.freespace_carve_points_device(d_p.ptr, n, R, t, MIN_D, MAX_D, margin=margin)
            _same(_bits(e, want), want.bits, "shuffled, device form")


def test_union_idempotence_and_order_on_the_device(empty):
    e = empty
    origin, dims, shift = (-20, -20, -20), (40, 40, 40), 1
    e.freespace_create(origin, dims, shift)
    R, t = POSES[1]
    pts = _cloud(65)
    d_img, d_pts = hipmem.DeviceBuffer.from_numpy(IMAGE), hipmem.DeviceBuffer.from_numpy(pts)
    A = lambda: e.freespace_carve_depth_device(d_img.ptr, *CAM, 16, 24, R, t, MIN_D, MAX_D)  # noqa: E731
    B = lambda: e.freespace_carve_points_device(d_pts.ptr, 65, I3, Z3, MIN_D, MAX_D)        # noqa: E731
    want = fr.carve_depth(fr.Layer(origin, dims, shift), VS, IMAGE, *CAM, R, t, MIN_D, MAX_D)
    only_a = want.bits.copy()
    fr.carve_points(want, VS, pts, I3, Z3, MIN_D, MAX_D)
    assert only_a.sum() < want.bits.sum()
    for order in ((A, B), (B, A), (A, A, B), (A, B, A, B)):
        e.freespace_clear()
        for call in order:
            call()
        _same(_bits(e, want), want.bits, "order %d" % len(order))
    e.freespace_clear()
    assert not _bits(e, want).any()
    A()
    _same(_bits(e, want), only_a, "A alone")
    e.reset()  # mrh_reset clears the bits and keeps the box
    assert not _bits(e, want).any()
    B()
    A()
    _same(_bits(e, want), want.bits, "after the reset the box is still there")
    # create on top of a layer replaces it, empty
    e.freespace_create(origin, dims, 0)
    assert not _bits(e, fr.Layer(origin, dims, 0)).any()


# ---- the box reader on hand-built maps -----------------------------------------------------------------------------------------

BOX_PARAMS = er.SPHERE_PARAMS
BOX_VS = F(BOX_PARAMS["virtual_voxel_size"])  # 0.05


def _coarse_blocks(params):
    """The sphere with one coarse block (resolution 1, 64 voxels)."""
    blocks = dict(er.sphere_blocks(params))
    b, lin = (0, 0, 0), np.arange(64)
    assert b in blocks
    v = np.stack([b[0] * 8 + 2 * (lin % 4), b[1] * 8 + 2 * ((lin // 4) % 4), b[2] * 8 + 2 * (lin // 16)], -1)
    vox = np.zeros(64, capi.VOXEL_DTYPE)
    vox["sdf"], vox["weight"] = er.sphere_sdf(params["virtual_voxel_size"], params["sdf_truncation"], v)[0], 1
    blocks[b] = (1, vox)
    return blocks


def _weighted_sphere():
    blocks = er.sphere_blocks()
    for k, v in blocks.items():
        v["weight"] = np.where((np.arange(512) + sum(k)) % 3 == 0, 1, 3)
    return blocks


SCENES = {
    "sphere": lambda: (_weighted_sphere(), BOX_PARAMS),
    "sites": lambda: (er.site_blocks([(9, 2, 3), (-13, 5, -22), (0, 0, 0), (7, 7, 7)]), BOX_PARAMS),
    "coarse": lambda: (_coarse_blocks(dict(BOX_PARAMS, sdf_var_threshold=0.005)), dict(BOX_PARAMS, sdf_var_threshold=0.005)),
}


@pytest.fixture(scope="module", params=list(SCENES))
def scene(request):
    blocks, params = SCENES[request.param]()
    e = pu.make_engine(capi.load_hip(), synth.CFG1, params, 4096)
    e.import_blocks(*er.to_import(blocks))
    d, v = e.dump_blocks()
    yield request.param, e, rr.make_map(params, d, v)
    e.close()


def _box_cloud():
    """Rays from a sensor beside the sphere, through and past it (the carve does not care what the map holds)."""
    rng = np.random.default_rng(11)
    p = rng.normal(size=(96, 3)).astype(F)
    p[:, 0] = -np.abs(p[:, 0]) - 1.0  # towards -x, where the sphere is
    return (p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0.4, 1.6, (96, 1))).astype(F)


BOX_T = np.array([0.9, 0.1, 0.05], F)


def _carved(e, shift):
    """A layer over voxels -24 .. 23 per axis, carved by _box_cloud on the engine and in the restatement."""
    origin, dims = (-(24 >> shift),) * 3, (48 >> shift,) * 3
    e.freespace_create(origin, dims, shift)
    e.freespace_carve_points(_box_cloud(), I3, BOX_T, 0.05, 3.0)
    return fr.carve_points(fr.Layer(origin, dims, shift), BOX_VS, _box_cloud(), I3, BOX_T, 0.05, 3.0)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_box_reader_equals_the_restatement(scene, shift):
    name, e, m = scene
    layer = _carved(e, shift)
    n = 48 >> shift
    o = -(24 >> shift)
    seen = 0
    boxes = [((o - 1,) * 3, (n + 2,) * 3, {}),                                   # the whole layer padded by one cell: straddles it
             ((o + 1, o + 2, o + 1), (n - 3, n - 4, n - 2), {}),                 # inside
             ((o + n // 2, o - 3, o + 1), (n, 5, 3), {}),                        # straddling a face and a corner
             ((o + n + 2, o, o), (3, 2, 4), {}),                                 # entirely outside the layer
             ((o + n // 2, o + n // 2, o + n // 2), (1, 1, 1), {}),
             ((o - 1,) * 3, (n + 2,) * 3, dict(surface_band=0.02, min_weight=2))]
    for origin, dims, kw in boxes:
        got = e.freespace_box(origin, dims, **kw)
        want = fr.box(layer, m, origin, dims, **kw)
        assert got.shape == want.shape == (dims[2], dims[1], dims[0])
        _same(got, want, f"{name} s={shift} box {origin} {dims} {kw}")
        if not kw:
            seen |= int(np.bitwise_or.reduce(got.ravel()))
    full = e.freespace_box(*boxes[0][:2])
    for bit in (capi.FREE_FREE, capi.FREE_OBSERVED, capi.FREE_OCCUPIED, capi.FREE_FRONTIER):
        assert np.any(full & bit), f"{name} s={shift}: no cell has bit {bit}"
    assert np.any(full == 0) and np.all(e.freespace_box(*boxes[3][:2]) & capi.FREE_FREE == 0)
    if name == "sphere":  # the gates matter on the map with weights 1 and 3
        gated = e.freespace_box(*boxes[5][:2], **boxes[5][2])
        assert np.count_nonzero(gated & capi.FREE_OBSERVED) <= np.count_nonzero(full & capi.FREE_OBSERVED) and not np.array_equal(gated, full)
    # the device form writes the same bytes
    origin, dims, _ = boxes[0]
    buf = hipmem.DeviceBuffer.from_numpy(np.full(full.size, 0xA5, np.uint8))
    e.freespace_box_device(origin, dims, buf.ptr)
    e.sync()
    assert buf.to_numpy(np.uint8).tobytes() == full.tobytes()


@pytest.fixture(scope="module")
def sphere():
    blocks, params = SCENES["sphere"]()
    e = pu.make_engine(capi.load_hip(), synth.CFG1, params, 4096)
    e.import_blocks(*er.to_import(blocks))
    d, v = e.dump_blocks()
    yield e, rr.make_map(params, d, v)
    e.close()


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("origin,dims", [((-256, -1, -1), (512, 3, 2)), ((-1, -1, -256), (2, 3, 512))])
def test_long_boxes(sphere, origin, dims, shift):
    e, m = sphere
    layer = _carved(e, shift)
    got = e.freespace_box(origin, dims)
    _same(got, fr.box(layer, m, origin, dims), f"s={shift} box {origin} {dims}")
    assert np.any(got & capi.FREE_FREE) and np.any(got & capi.FREE_OBSERVED)


# ---- segments --------------------------------------------------------------------------------------------------------------------

def _hand_layer(e):
    """The layer of tests/test_freespace.py: s = 1, one return at (0.31, 0, 0) seen from the origin sets the cells 0 .. 7 on the x axis."""
    e.freespace_create((-2, -2, -2), (12, 4, 4), 1)
    e.freespace_carve_points(np.array([[0.31, 0.0, 0.0]], F), I3, Z3, 0.0, 5.0)
    return fr.carve_points(fr.Layer((-2, -2, -2), (12, 4, 4), 1), VS, [[0.31, 0.0, 0.0]], I3, Z3, 0.0, 5.0)


def test_segments(empty):
    e = empty
    layer = _hand_layer(e)
    _same(_bits(e, layer), layer.bits, "the hand layer")
    a = np.array([[0.0, 0, 0], [0.0, 0, 0], [0.1, 0, 0], [0.1, 0.1, 0], [0.0, 0, 0], [np.nan, 0, 0], [0.0, 0, 0], [0.0, 0, 0], [0, 20000.0, 0]], F)
    b = np.array([[0.31, 0, 0], [0.41, 0, 0], [0.1, 0, 0], [0.1, 0.1, 0], [1.01, 0, 0], [0.1, 0, 0], [0.1, np.inf, 0], [0.0, 3e4, 0], [0, 21000.0, 0]], F)
    status, counts = e.freespace_segments(a, b)
    assert status.tolist() == [0, 1, 0, 1, 1, 0x80, 0x80, 0x80, 0x80]  # the hand answers of the CPU test
    assert counts.tolist() == [[16, 16], [21, 16], [1, 1], [1, 0], [51, 16], [0, 0], [0, 0], [0, 0], [0, 0]]
    status, counts = e.freespace_segments([[0.0, 0, 0]], [[0.35, 0, 0]], step=0.1)
    assert status.tolist() == [0] and counts.tolist() == [[4, 4]]
    # n = 0, 1, 65 against the restatement, host form and device form
    rng = np.random.default_rng(2)
    for n in (0, 1, 65):
        sa = rng.uniform(-0.1, 0.4, (n, 3)).astype(F) * np.array([1, 0.1, 0.1], F)
        sb = rng.uniform(-0.1, 0.4, (n, 3)).astype(F) * np.array([1, 0.1, 0.1], F)
        if n == 65:
            sa[:9], sb[:9] = a, b
            sb[9] = sa[9]
        want = fr.segments(layer, VS, sa, sb)
        got = e.freespace_segments(sa, sb)
        assert got[0].shape == (n,) and got[1].shape == (n, 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), n
        if n:
            d_a, d_b = hipmem.DeviceBuffer.from_numpy(sa), hipmem.DeviceBuffer.from_numpy(sb)
            d_s, d_c = hipmem.DeviceBuffer.from_numpy(np.full(n, 0xA5, np.uint8)), hipmem.DeviceBuffer.from_numpy(np.full(8 * n, 0xA5, np.uint8))
            e.freespace_segments_device(d_a.ptr, d_b.ptr, n, d_s.ptr, d_c.ptr)
            e.sync()
            assert d_s.to_numpy(np.uint8).tobytes() == got[0].tobytes() and d_c.to_numpy(np.uint8).tobytes() == got[1].tobytes()
            d_c2 = hipmem.DeviceBuffer.from_numpy(np.full(8 * n, 0xA5, np.uint8))
            e.freespace_segments_device(d_a.ptr, d_b.ptr, n, d_s.ptr)  # no counts
            e.sync()
            assert d_s.to_numpy(np.uint8).tobytes() == got[0].tobytes() and np.all(d_c2.to_numpy(np.uint8) == 0xA5)
        else:
            e.freespace_segments_device(0, 0, 0, 1)
    assert np.any(want[0] == 0) and np.any(want[0] == 1) and np.any(want[0] == 0x80)


# ---- the frame path ----------------------------------------------------------------------------------------------------------------

def _room_layer(e, shift=3):
    """A layer over the synthetic room: 6.4 m per side at s = 3 (0.16 m cells), centred on the orbit."""
    n = 320 >> shift
    e.freespace_create((-(n // 2),) * 3, (n,) * 3, shift)
    return fr.Layer((-(n // 2),) * 3, (n,) * 3, shift)


CARVE = dict(min_depth=0.01, max_depth=6.0, margin=0.16)  # from the camera itself; a cell short of the surface


def test_carving_leaves_the_frame_path_alone():
    """Twelve frames integrated with a carve after every frame — host form, device form — and with no carve: the same blocks, the
    same counters, the same mesh.  The carves run between the frames of the pipelined stream and flush nothing (D22)."""
    hip = capi.load_hip()
    K = synth.CFG1
    frames = list(synth.replica_stream(12, K=K))
    engines = [pu.make_engine(hip, K, PARAMS, 65536) for _ in range(3)]
    host, dev, plain = engines
    try:
        _room_layer(host)
        _room_layer(dev)
        keep = []
        for f in frames:
            for e in engines:
                pu.feed(e, f)
            host.freespace_carve_depth(f.depth, K.fx, K.fy, K.cx, K.cy, f.R, f.t, **CARVE)
            keep.append(hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(f.depth, F)))
            dev.freespace_carve_depth_device(keep[-1].ptr, K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, f.R, f.t, **CARVE)
        dumps = [e.dump_blocks() for e in engines]
        assert len(dumps[2][0]) > 100
        for d, v in dumps[:2]:
            assert d.tobytes() == dumps[2][0].tobytes() and v.tobytes() == dumps[2][1].tobytes()
        stats = [e.stats() for e in engines]
        for name, _ in capi.MrhStats._fields_:
            if "ms" not in name:
                assert getattr(stats[0], name) == getattr(stats[2], name) and getattr(stats[1], name) == getattr(stats[2], name), name
        meshes = [(e.extract_triangles(),) + e.extract_mesh() for e in engines]
        assert len(meshes[2][0]) > 100 and len(meshes[2][1]) > 100
        for m in meshes[:2]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(m, meshes[2]))
        # and the two forms carved the same layer
        n = 320 >> 3
        box = ((-(n // 2),) * 3, (n,) * 3)
        a, b = host.freespace_box(*box), dev.freespace_box(*box)
        assert a.tobytes() == b.tobytes() and np.any(a & capi.FREE_FREE)
    finally:
        for e in engines:
            e.close()


def test_line_of_sight_free_on_the_fused_room():
    """The CFG1 128 x 128 synthetic room, 20 frames fused and carved with s = 3: Engine.line_of_sight_free over the 21 segments
    between seven camera positions equals the restatement.  Measured with the restatement on the map the CPU oracle fuses: all 21
    segments are free, where cast_rays alone (line_of_sight) reports none of them as observed free space — every one has
    unknown samples (status MRH_RAY_UNKNOWN) and none meets a surface."""
    hip = capi.load_hip()
    K = synth.CFG1
    frames = list(synth.replica_stream(20, K=K))
    e = pu.make_engine(hip, K, PARAMS, 65536)
    try:
        layer = _room_layer(e)
        for f in frames:
            pu.feed(e, f)
            e.freespace_carve_depth(f.depth, K.fx, K.fy, K.cx, K.cy, f.R, f.t, **CARVE)
            fr.carve_depth(layer, VS, f.depth, K.fx, K.fy, K.cx, K.cy, f.R, f.t, **CARVE)
        _same(_bits(e, layer), layer.bits, "the room's layer")
        stops = np.array([np.asarray(f.t, F) for f in frames][::3])
        assert len(stops) == 7
        i, j = np.triu_indices(len(stops), 1)
        a, b = stops[i], stops[j]
        got = e.line_of_sight_free(a, b)
        strict = e.line_of_sight(a, b)
        d, v = e.dump_blocks()
        seg = (b - a).astype(F)
        ln = np.sqrt((seg[:, 0] * seg[:, 0] + seg[:, 1] * seg[:, 1]) + seg[:, 2] * seg[:, 2], dtype=F)
        q = yr.RayQuery(rr.make_map(PARAMS, d, v), 0.0, float(ln.max()), 0.0, truncation=PARAMS["sdf_truncation"])
        cast = q.cast(a, capi.normalize_directions(seg), tmax=ln)["status"]
        want = fr.line_of_sight_free(layer, VS, cast, a, b)
        print("line_of_sight_free: %d of %d segments free, line_of_sight: %d" % (int(want.sum()), len(want), int(strict.sum())))
        assert got.dtype == bool and np.array_equal(got, want)
        assert np.any(want & ~strict), "no segment is free that cast_rays alone reports as not observed-free"
        # the frontier of the room's box is not empty
        n = 320 >> 3
        assert np.any(e.freespace_box((-(n // 2) - 1,) * 3, (n + 2,) * 3) & capi.FREE_FRONTIER)
    finally:
        e.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_through_the_c_abi():
    e = pu.make_engine(capi.load_hip(), synth.CFG1, PARAMS, 4096)
    err = lambda: e.lib.mrh_last_error(e._ctx).decode()  # noqa: E731
    Fp = C.POINTER(C.c_float)
    R, t = I3.ctypes.data_as(Fp), Z3.ctypes.data_as(Fp)
    cp = capi.MrhCarveParams(*CAM, 16, 24, MIN_D, MAX_D, 0.0, 0.0)
    bp = capi.MrhFreespaceBoxParams((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2), 0, 0.0)
    out = C.c_void_p()
    pts = _cloud(8)
    try:
        # no layer: MRH_ERR_STATE from every call but the create, with the plan check's text
        calls = {
            "mrh_freespace_clear": lambda: e.lib.mrh_freespace_clear(e._ctx),
            "mrh_freespace_destroy": lambda: e.lib.mrh_freespace_destroy(e._ctx),
            "mrh_freespace_carve_depth": lambda: e.lib.mrh_freespace_carve_depth(e._ctx, C.byref(cp), IMAGE.ctypes.data, R, t),
            "mrh_freespace_carve_depth_device": lambda: e.lib.mrh_freespace_carve_depth_device(e._ctx, C.byref(cp), 1, R, t),
            "mrh_freespace_carve_points": lambda: e.lib.mrh_freespace_carve_points(e._ctx, C.byref(cp), pts.ctypes.data, 8, R, t),
            "mrh_freespace_carve_points_device": lambda: e.lib.mrh_freespace_carve_points_device(e._ctx, C.byref(cp), 1, 8, R, t),
            "mrh_freespace_box": lambda: e.lib.mrh_freespace_box(e._ctx, C.byref(bp), C.byref(out)),
            "mrh_freespace_box_device": lambda: e.lib.mrh_freespace_box_device(e._ctx, C.byref(bp), 1),
            "mrh_freespace_segments": lambda: e.lib.mrh_freespace_segments(e._ctx, pts.ctypes.data, pts.ctypes.data, 8, 0.0, C.byref(out), None),
            "mrh_freespace_segments_device": lambda: e.lib.mrh_freespace_segments_device(e._ctx, 1, 1, 8, 0.0, 1, None),
        }
        for who, call in calls.items():
            assert call() == capi.MRH_ERR_STATE, who
            assert err() == who + ": the context has no free-space layer (call mrh_freespace_create)"
        assert e.lib.mrh_freespace_clear(None) == capi.MRH_ERR_INVALID_ARG
        # the create's limits
        with pytest.raises(capi.MrhError) as ei:
            e.freespace_create((0, 0, 0), (1025, 1, 1), 0)
        assert ei.value.code == capi.MRH_ERR_INVALID_ARG and "layer of 1025 x 1 x 1 cells (1 .. 1024 per side)" in str(ei.value)
        with pytest.raises(capi.MrhError) as ei:
            e.freespace_create((0, 0, 0), (4, 4, 4), 4)
        assert "cell_shift 4 (0 .. 3)" in str(ei.value)
        assert e.lib.mrh_freespace_create(e._ctx, None) == capi.MRH_ERR_INVALID_ARG and err() == "mrh_freespace_create: null argument"
        e.freespace_create((-2, -2, -2), (4, 4, 4), 1)
        for who, call in calls.items():
            if who != "mrh_freespace_destroy" and "device" not in who:
                assert call() == capi.MRH_OK, (who, err())
        # with a layer: the limits, each with its text
        bad = [(capi.MrhCarveParams(*CAM, 16, 24, MIN_D, MAX_D, 0.0, 0.0, (C.c_uint32 * 2)(0, 1)), "a reserved word is not 0"),
               (capi.MrhCarveParams(*CAM, 0, 24, MIN_D, MAX_D, 0.0, 0.0), "image of 0 x 24 pixels (1 .. 4096 per side)"),
               (capi.MrhCarveParams(0.0, 24.0, 11.5, 7.5, 16, 24, MIN_D, MAX_D, 0.0, 0.0), "bad intrinsics"),
               (capi.MrhCarveParams(*CAM, 16, 24, -0.1, MAX_D, 0.0, 0.0), "need 0 <= min_depth < max_depth"),
               (capi.MrhCarveParams(*CAM, 16, 24, MAX_D, MAX_D, 0.0, 0.0), "need 0 <= min_depth < max_depth"),
               (capi.MrhCarveParams(*CAM, 16, 24, MIN_D, MAX_D, 0.0, -0.01), "margin -0.01"),
               (capi.MrhCarveParams(*CAM, 16, 24, MIN_D, MAX_D, -1.0, 0.0), "the sample spacing must be > 0 (step -1)"),
               (capi.MrhCarveParams(*CAM, 16, 24, MIN_D, MAX_D, 1e-7, 0.0), "more than 2^20 samples per ray")]
        for p, text in bad:
            assert e.lib.mrh_freespace_carve_depth(e._ctx, C.byref(p), IMAGE.ctypes.data, R, t) == capi.MRH_ERR_INVALID_ARG, text
            assert err().startswith("mrh_freespace_carve_depth: ") and text in err(), err()
        assert e.lib.mrh_freespace_carve_depth(e._ctx, C.byref(cp), None, R, t) == capi.MRH_ERR_INVALID_ARG and err() == "mrh_freespace_carve_depth: null argument"
        nan_R = I3.copy()
        nan_R[1, 2] = np.nan
        assert e.lib.mrh_freespace_carve_points(e._ctx, C.byref(cp), pts.ctypes.data, 8, nan_R.ctypes.data_as(Fp), t) == capi.MRH_ERR_INVALID_ARG
        assert err() == "mrh_freespace_carve_points: pose is not finite"
        assert e.lib.mrh_freespace_carve_points(e._ctx, C.byref(cp), pts.ctypes.data, (1 << 24) + 1, R, t) == capi.MRH_ERR_INVALID_ARG
        assert err() == "mrh_freespace_carve_points: 16777217 points in one call (limit 2^24)"
        big = capi.MrhFreespaceBoxParams((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 513, 2), 0, 0.0)
        assert e.lib.mrh_freespace_box(e._ctx, C.byref(big), C.byref(out)) == capi.MRH_ERR_INVALID_ARG
        assert err() == "mrh_freespace_box: box of 2 x 513 x 2 cells (1 .. 512 per side)"
        assert e.lib.mrh_freespace_box(e._ctx, C.byref(bp), None) == capi.MRH_ERR_INVALID_ARG and err() == "mrh_freespace_box: null argument"
        assert e.lib.mrh_freespace_segments(e._ctx, pts.ctypes.data, pts.ctypes.data, 8, -1.0, C.byref(out), None) == capi.MRH_ERR_INVALID_ARG
        assert err() == "mrh_freespace_segments: the sample spacing must be > 0 (step -1)"
        assert e.lib.mrh_freespace_segments(e._ctx, None, pts.ctypes.data, 8, 0.0, C.byref(out), None) == capi.MRH_ERR_INVALID_ARG
        assert e.lib.mrh_freespace_segments_device(e._ctx, 1, 1, 8, 0.0, None, None) == capi.MRH_ERR_INVALID_ARG
        # destroy: no layer again
        e.freespace_destroy()
        assert calls["mrh_freespace_clear"]() == capi.MRH_ERR_STATE
    finally:
        e.close()
    sh = capi.Engine(capi.load_hip(), capi.Params(num_sdf_blocks=4096, shard_rank=0, shard_count=2, **PARAMS))
    try:
        with pytest.raises(capi.MrhError) as ei:
            sh.freespace_create((0, 0, 0), (4, 4, 4), 1)
        assert ei.value.code == capi.MRH_ERR_UNSUPPORTED and "sharded maps have no free-space layer (shard_count 2)" in str(ei.value)
    finally:
        sh.close()
