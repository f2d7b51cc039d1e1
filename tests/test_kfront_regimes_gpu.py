"""k_front's ray path against the CPU oracle on a 72 x 96 window (a second or two per case): ragged tile rows, direction components
that are exactly zero, invalid depths and depths at the integration distance, block coordinates of both signs, the float
voxel -> block form beyond Map::block_shift_limit, a tile whose blocks do not fit its LDS key set, and the same stream under every
instantiation that shares the ray helpers (serial, pipelined with a short reclaim period, multi-resolution, starve frames,
spherical, LiDAR scans, a two-shard map).  Each regime is first shown to occur, on the host, from the inputs or from the oracle's
block list; occupancy and payload are then compared bit for bit."""
import numpy as np
import pytest

import parity_utils as pu
from mrhash_amd import capi, synth

pytestmark = pytest.mark.gpu

# REPLICA_640's focal lengths; column 48 and row 36 look along u == 0 / v == 0 exactly (col - cx - 0.5 == 0)
K = synth.Intrinsics(synth.REPLICA_640.fx, synth.REPLICA_640.fy, 47.5, 35.5, 72, 96)
MAX_DEPTH = np.float32(3.5)  # = the integration distance (mrh_set_camera)
PARAMS = dict(synth.REPLICA_PARAMS, max_depth=float(MAX_DEPTH))
BLOCKS = 16384
TILE = 16          # mrh_pipe.h: kRayTile
SET_CAP = 1024     # mrh_pipe.h: kRayCap, keys of a tile's LDS set
IDENTITY = np.array([0, 0, 0, 1], np.float32)


def _frame(t, q, depth, seed, k=K):
    rgb = np.random.default_rng(seed).integers(0, 256, size=(k.rows, k.cols, 3), dtype=np.uint8)
    q = np.asarray(q, np.float64)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    return synth.Frame(np.asarray(t, np.float32), q, synth.quat_to_rot(q), depth.astype(np.float32), rgb)


def _tilted_plane(z_left=0.5, z_right=4.0):
    """depth image of the plane z = a + b x that the left image border sees at z_left and the right one at z_right"""
    u = (np.arange(K.cols, dtype=np.float64) - K.cx - 0.5) / K.fx
    b = (1.0 / z_left - 1.0 / z_right) / (u[-1] / z_left - u[0] / z_right)
    a = z_left * (1.0 - b * u[0])
    return np.repeat((a / (1.0 - b * u))[None, :], K.rows, axis=0)


def _depth():
    """the tilted plane (0.5 m .. 4 m; beyond 3.5 m it is out of range) with a band of depth 0 and a band at the integration
    distance and its two neighbours"""
    plane = _tilted_plane()
    plane[:4, :] = 0.0
    md = MAX_DEPTH
    band = np.array([md, np.nextafter(md, np.float32(np.inf)), np.nextafter(md, np.float32(0))], np.float32)
    plane = plane.astype(np.float32)
    plane[66:, :] = band[np.arange(K.cols) % 3][None, :]
    return plane


def _stream(poses):
    d = _depth()
    return [_frame(t, q, d, i + 1) for i, (t, q) in enumerate(poses)]


AXIS_POSES = [((0, 0, 0), IDENTITY), ((0.007, 0.003, 0), IDENTITY), ((0.01, 0, -0.2), IDENTITY)]
# looking along +x (with a roll), along -x and along -y from 1.5 m on the other side of the origin: the plane's 0.5 .. 3.5 m
# straddle the origin on the viewing axis, the image straddles it on the other two
s, c = np.sin, np.cos
ROTATED_POSES = [
    ((-1.5, 0.03, 0.02), (0.05 * s(0.83), s(0.83), 0.02, c(0.83))),     # yaw 95 degrees
    ((1.5, -0.02, 0.04), (0.0, s(-0.80), 0.03 * s(-0.80), c(-0.80))),   # yaw -92 degrees
    ((0.02, 1.5, -0.03), (s(0.77), 0.02, 0.0, c(0.77))),                # pitch 88 degrees
]
FAR = np.array([420.0, -310.0, 150.0], np.float32)  # tests/test_parity_gpu.py::test_far_from_origin, "far"


def _segments(f, params=PARAMS, k=K):
    """per pixel, in float64: the cleaned depth, dmin, dmax and the world direction of the segment (ray_setup)"""
    d = f.depth.astype(np.float64)
    d = np.where((d <= params["min_depth"]) | (d > params["max_depth"]), 0.0, d)
    tr = params["sdf_truncation"] + params["sdf_truncation_scale"] * d
    dmin, dmax = np.minimum(params["max_depth"], d - tr), np.minimum(params["max_depth"], d + tr)
    rays = synth.pixel_rays(k)  # (col - cx - 0.5) / fx, (row - cy - 0.5) / fy, 1
    return d, dmin, dmax, rays @ f.R.astype(np.float64).T


def _xyz(descs):
    return np.stack([descs["x"], descs["y"], descs["z"]], 1)


_REF = {}


def _reference(oracle, name, frames, k=K, blocks=BLOCKS, **over):
    """the oracle's map of `frames` under PARAMS + over, once per stream and parameter set; the engine is never fed again"""
    key = (name, tuple(sorted(over.items())))
    if key not in _REF:
        b = pu.make_engine(oracle, k, dict(PARAMS, **over), blocks)
        for f in frames:
            pu.feed(b, f)
        assert b.stats().error_flags == 0
        _REF[key] = b
    return _REF[key]


def _run(hip, frames, k=K, blocks=BLOCKS, **over):
    a = pu.make_engine(hip, k, dict(PARAMS, **over), blocks)
    for f in frames:
        pu.feed(a, f)
    a.sync()
    assert a.stats().error_flags == 0
    return a


def _same(a, b, at_least):
    r = pu.compare_maps(a, b)
    assert r["blocks"] > at_least and r["sdf_bit_exact"] and r["sumsq_bit_exact"], r
    return r


def check_ragged_and_zeros():
    frames = _stream(AXIS_POSES)
    assert K.rows % TILE != 0 and K.cols % TILE == 0
    d, dmin, dmax, dirs = _segments(frames[0])
    valid = d > 0
    assert (dirs[:, 48, 0] == 0).all() and (dirs[36, :, 1] == 0).all() and valid[:, 48].any() and valid[36, :].any()
    raw = frames[0].depth
    assert (raw == 0).any() and (raw > MAX_DEPTH).any() and (raw == MAX_DEPTH).any()
    assert (valid & (d + PARAMS["sdf_truncation"] > float(MAX_DEPTH))).sum() >= 64  # dmax is the clamp
    # the integration distance IS max_depth here, so a pixel that survives the cleaning has d - trunc < max_int_dist: `dmin >= dmax`
    # cannot hold for it; the pixels one ulp beyond max_depth leave through d == 0
    assert not (valid & (dmin >= dmax)).any() and (~valid & (raw > MAX_DEPTH)).sum() >= 64
    return frames


def check_mixed_signs(oracle):
    frames = _stream(ROTATED_POSES)
    pos, neg = np.zeros(3, bool), np.zeros(3, bool)
    for f in frames:
        d, _, _, dirs = _segments(f)
        pos |= (dirs[d > 0] > 1e-3).any(0)
        neg |= (dirs[d > 0] < -1e-3).any(0)
    assert pos.all() and neg.all(), (pos, neg)  # every step sign on every axis
    b = _reference(oracle, "rotated", frames)
    xyz = _xyz(b.dump_blocks()[0])
    assert ((xyz < 0).any(0) & (xyz == 0).any(0) & (xyz > 0).any(0)).all(), (xyz.min(0), xyz.max(0))
    return frames, b


def shift_limit(vs):
    """Map::block_shift_limit as mrh_create finds it (k_block_shift_limit), in numpy's float32"""
    vs = np.float32(vs)
    eps, mbs = np.float32(1e-5), np.float32(8.0) * vs
    v = np.arange(1 << 23, dtype=np.int32)
    bp = np.floor((v.astype(np.float32) * vs + eps) / mbs).astype(np.int32)
    pwn = (-v - np.where(v > 0, 7, 0)).astype(np.float32) * vs
    bn = np.where(pwn >= 0, np.floor((pwn + eps) / mbs), np.ceil((pwn - eps) / mbs)).astype(np.int32)
    bad = np.nonzero((bp != (v >> 3)) | (bn != ((-v) >> 3)))[0]
    first_bad = int(bad[0]) if len(bad) else 1 << 23
    lim = 1
    while (lim << 1) <= first_bad and lim < (1 << 22):
        lim <<= 1
    return 0 if first_bad <= 1 else lim


def check_far():
    lim = shift_limit(PARAMS["virtual_voxel_size"])
    frames = _stream(ROTATED_POSES)
    for f in frames:
        f.t = (f.t + FAR).astype(np.float32)
    reach = float(MAX_DEPTH) + 1.6  # camera within 1.6 m of the offset, rays no longer than max_depth
    voxel_min = (np.abs(FAR.astype(np.float64)) - reach) / PARAMS["virtual_voxel_size"]
    print("block_shift_limit", lim, "smallest |voxel| per axis", voxel_min)
    assert 0 < lim <= voxel_min.max()  # one axis beyond the limit sends all three through the float form: every point of every ray
    return frames


# a fronto-parallel wall at 3 m behind 1 m of truncation at 4 mm voxels: a ray crosses ~60 blocks, a tile well over a thousand
SAT_K = synth.Intrinsics(synth.REPLICA_640.fx, synth.REPLICA_640.fy, 23.5, 15.5, 32, 48)
SAT_OVER = dict(virtual_voxel_size=0.004, sdf_truncation=1.0, max_depth=4.5)
SAT_BLOCKS = 32768


def check_saturation(oracle):
    frames = [_frame(t, IDENTITY, np.full((SAT_K.rows, SAT_K.cols), 3.0), 7 + i, SAT_K) for i, t in enumerate([(0, 0, 0), (0.002, 0.001, 0)])]
    b = pu.make_engine(oracle, SAT_K, dict(PARAMS, **SAT_OVER), SAT_BLOCKS)
    pu.feed(b, frames[0])
    assert b.stats().error_flags == 0  # the pool holds every block of the frame
    xyz = _xyz(b.dump_blocks()[0]).astype(np.float64)
    ctr = (xyz * 8 + 3.5) * SAT_OVER["virtual_voxel_size"]  # identity pose: world == camera
    col = np.floor(SAT_K.fx * ctr[:, 0] / ctr[:, 2] + SAT_K.cx + 0.5).astype(int)
    row = np.floor(SAT_K.fy * ctr[:, 1] / ctr[:, 2] + SAT_K.cy + 0.5).astype(int)
    inside = (col >= 0) & (col < SAT_K.cols) & (row >= 0) & (row < SAT_K.rows)
    per_tile = np.bincount((row[inside] // TILE) * (SAT_K.cols // TILE) + col[inside] // TILE, minlength=6)
    print("blocks:", len(xyz), "distinct blocks whose centre projects into each tile:", per_tile.tolist())
    assert per_tile.max() > SET_CAP
    pu.feed(b, frames[1])
    assert b.stats().error_flags == 0
    return frames, b


def test_ragged_tiles_and_exact_zeros(hip, oracle):
    frames = check_ragged_and_zeros()
    _same(_run(hip, frames), _reference(oracle, "axis", frames), 100)


def test_negative_and_mixed_sign_coordinates(hip, oracle):
    frames, b = check_mixed_signs(oracle)
    _same(_run(hip, frames), b, 100)


def test_far_from_origin_takes_the_float_form(hip, oracle):
    frames = check_far()
    _same(_run(hip, frames), _reference(oracle, "far", frames), 100)


def test_tile_with_more_blocks_than_its_key_set(hip, oracle):
    frames, b = check_saturation(oracle)
    _same(_run(hip, frames, SAT_K, SAT_BLOCKS, **SAT_OVER), b, 4 * SET_CAP)


@pytest.mark.parametrize("env,over", [
    (dict(MRH_PIPE="0"), {}),
    (dict(MRH_PIPE="1", MRH_PIPE_PERIOD="2"), {}),
    ({}, dict(sdf_var_threshold=0.005)),
    ({}, dict(n_frames_invalidate_voxels=2)),
], ids=["serial", "pipe-period-2", "multi-resolution", "starve-period-2"])
def test_rotated_stream_under_every_instantiation(hip, oracle, monkeypatch, env, over):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    frames = _stream(ROTATED_POSES)
    _same(_run(hip, frames, **over), _reference(oracle, "rotated", frames, **over), 100)


def test_spherical_stream_32_x_128(hip, oracle):
    cam = synth.spherical_camera(32, 128)
    p = dict(synth.VBR_PARAMS, min_weight_threshold=1, n_frames_invalidate_voxels=100)
    engines = []
    for lib in (hip, oracle):
        e = capi.Engine(lib, capi.Params(num_sdf_blocks=BLOCKS, **p))
        e.set_camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["rows"], cam["cols"], p["min_depth"], 60.0, model=1)
        engines.append(e)
    scene = synth.street_canyon()
    for t, q in synth.drive_poses(3, step=0.5):
        depth, rgb = synth.spherical_range_image(scene, t, q, cam)
        for e in engines:
            e.set_pose(synth.quat_to_rot(q), t)
            e.upload_depth(depth)
            e.upload_rgb(rgb)
            assert not e.integrate()
    engines[0].sync()
    _same(engines[0], engines[1], 200)
    assert engines[0].stats().error_flags == 0


def test_lidar_scan_16_x_256(hip, oracle):
    """k_alloc3d walks its beams with the same helpers (mrh_lidar.h)"""
    p = dict(synth.VBR_PARAMS, min_weight_threshold=1)
    engines = [pu.make_lidar_engine(lib, p, 100.0) for lib in (hip, oracle)]
    scene = synth.street_canyon()
    t, q = synth.drive_poses(1, step=2.0)[0]
    pts = synth.lidar_scan(scene, t, q, rows=16, cols=256)
    for e in engines:
        e.set_pose(synth.quat_to_rot(q), t)
        e.upload_points(pts)
        assert not e.integrate_points()
    _same(engines[0], engines[1], 50)
    assert engines[0].stats().error_flags == 0


def test_two_shards_on_one_device(hip, oracle):
    """shard_count = 2: owns_block's hash decides inside the walk; the union of the two shard maps is the oracle's single map"""
    frames, b = check_mixed_signs(oracle)
    shards = [pu.make_engine(hip, K, PARAMS, BLOCKS, shard_rank=r, shard_count=2, shard_chunk_log2=1) for r in range(2)]
    for f in frames:
        for e in shards:
            pu.feed(e, f)
    parts = [e.dump_blocks() for e in shards]
    assert all(len(p[0]) > 20 for p in parts) and all(e.stats().error_flags == 0 for e in shards)
    d = np.concatenate([p[0] for p in parts])
    v = np.concatenate([p[1] for p in parts])
    order = np.lexsort((d["z"], d["y"], d["x"]))
    d0, v0 = b.dump_blocks()
    assert np.array_equal(d[order], d0) and np.array_equal(v[order].view(np.uint8), v0.view(np.uint8))
