"""k_back's per-block paths against the CPU oracle on a 96 x 72 window (a second or two per case): the wave-uniform early-out,
the three pixel-footprint classes of a block (no LDS tile, staged in two rounds, staged in one), pixels that no voxel may use
(depth 0, depth beyond the integration distance), the weight arithmetic at its limits, and the same stream under every
instantiation of the kernel the library chooses between (second residual step, serial, pipelined with a short reclaim period,
starve frames, multi-resolution, spherical).  Each regime is first shown to occur, on the host, from the oracle's block list."""
import numpy as np
import pytest

import parity_utils as pu
from mrhash_amd import capi, synth

pytestmark = pytest.mark.gpu

# REPLICA_640's focal lengths on a small window: a block (8 voxels of 1 cm) covers ~50 x 65 px at 0.5 m and ~9 x 11 px at 3.5 m
K = synth.Intrinsics(synth.REPLICA_640.fx, synth.REPLICA_640.fy, 48.0, 36.0, 72, 96)
MAX_DEPTH = np.float32(3.5)  # = the integration distance (mrh_set_camera)
PARAMS = dict(synth.REPLICA_PARAMS, max_depth=float(MAX_DEPTH))
BLOCKS = 16384
TILE_MAX_PX, ROUND_PX = 576, 256  # mrh_fast.h: kTileMaxPx, pixels staged by the first round of tile_issue / tile_commit
IDENTITY = np.array([0, 0, 0, 1], np.float32)


def _frame(t, depth, seed):
    rgb = np.random.default_rng(seed).integers(0, 256, size=(K.rows, K.cols, 3), dtype=np.uint8)
    return synth.Frame(np.asarray(t, np.float32), IDENTITY, synth.quat_to_rot(IDENTITY), depth.astype(np.float32), rgb)


def _tilted_plane(z_left=0.5, z_right=4.0):
    """depth image of the plane z = a + b x that the left image border sees at z_left and the right one at z_right"""
    u = (np.arange(K.cols, dtype=np.float64) - K.cx - 0.5) / K.fx  # x = z u along a pixel's ray
    b = (1.0 / z_left - 1.0 / z_right) / (u[-1] / z_left - u[0] / z_right)
    a = z_left * (1.0 - b * u[0])
    return np.repeat((a / (1.0 - b * u))[None, :], K.rows, axis=0)


def _stream():
    """frames 0, 1: the tilted plane (0.5 m .. 4 m, the part beyond 3.5 m is out of range) from two poses 7 mm apart, with a band
    of invalid pixels and a band at the integration distance and its two neighbours; frame 2: the camera has stepped back and
    a wall 0.45 m in front of it covers the left 60 columns, so the near blocks of the plane lie wholly behind a surface."""
    plane = _tilted_plane()
    plane[:4, :] = 0.0
    md = MAX_DEPTH
    band = np.array([md, np.nextafter(md, np.float32(np.inf)), np.nextafter(md, np.float32(0))], np.float32)
    plane = plane.astype(np.float32)
    plane[66:, :] = band[np.arange(K.cols) % 3][None, :]
    wall = plane.copy()
    wall[:, :60] = 0.45
    return [_frame((0, 0, 0), plane, 1), _frame((0.007, 0.003, 0), plane, 2), _frame((0.01, 0, -0.2), wall, 3)]


def _xyz(descs):
    return np.stack([descs["x"], descs["y"], descs["z"]], 1)


def _footprints(descs, f, vs):
    """Per block of `descs` (block coordinates): pixel footprint {c0, r0, w, h} and nearest corner z as front_sweep / wave_bbox
    state them, in float64; `sure` is false for a block within 1e-3 px of a rounding boundary or 1e-3 m of a depth bound (its
    class could differ in fp32: it is left out of the counts)."""
    Ri = f.R.astype(np.float64).T
    ti = -Ri @ f.t.astype(np.float64)
    corners = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], np.float64) * 7.0
    v = _xyz(descs)[:, None, :].astype(np.float64) * 8.0 + corners[None]
    pc = (v * vs) @ Ri.T + ti
    z = pc[..., 2]
    zmin, zmax = z.min(1), z.max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        uu = K.fx * pc[..., 0] / z + K.cx
        vv = K.fy * pc[..., 1] / z + K.cy
    edges = np.stack([uu.min(1), uu.max(1), vv.min(1), vv.max(1)], 1) + 0.5
    fl = np.floor(edges)
    c0, c1 = np.maximum(fl[:, 0] - 1, 0), np.minimum(fl[:, 1] + 1, K.cols - 1)
    r0, r1 = np.maximum(fl[:, 2] - 1, 0), np.minimum(fl[:, 3] + 1, K.rows - 1)
    w, h = c1 - c0 + 1, r1 - r0 + 1
    frac = edges - fl
    sure = (np.minimum(frac, 1 - frac).min(1) > 1e-3) & (zmin > 0.06) & (np.abs(zmin - float(MAX_DEPTH)) > 2e-3)
    listed = sure & (w > 0) & (h > 0) & (zmin <= float(MAX_DEPTH))  # in the image and in the depth range: on the visible list
    return dict(c0=c0.astype(int), r0=r0.astype(int), w=w.astype(int), h=h.astype(int), zmin=zmin, listed=listed)


def _regimes(descs, f, params):
    """blocks of the visible list by footprint class, and those the early-out provably takes: a tile, at least one usable pixel,
    and depth + truncation + 1e-4 <= zmin for every usable pixel of the footprint (with 1e-3 m to spare)"""
    fp = _footprints(descs, f, params["virtual_voxel_size"])
    area = fp["w"] * fp["h"]
    n = dict(no_tile=int((fp["listed"] & (area > TILE_MAX_PX)).sum()), two_rounds=int((fp["listed"] & (area > ROUND_PX) & (area <= TILE_MAX_PX)).sum()),
             one_round=int((fp["listed"] & (area <= ROUND_PX)).sum()), skipped=0, invalid_px=0, beyond_px=0)
    d = f.depth.astype(np.float64)
    d = np.where((d <= params["min_depth"]) | (d > params["max_depth"]), 0.0, d)
    for i in np.nonzero(fp["listed"] & (area <= TILE_MAX_PX))[0]:
        px = d[fp["r0"][i]:fp["r0"][i] + fp["h"][i], fp["c0"][i]:fp["c0"][i] + fp["w"][i]]
        raw = f.depth[fp["r0"][i]:fp["r0"][i] + fp["h"][i], fp["c0"][i]:fp["c0"][i] + fp["w"][i]]
        n["invalid_px"] += int((raw == 0).any())
        n["beyond_px"] += int((raw > MAX_DEPTH).any() and (raw == MAX_DEPTH).any() and ((raw < MAX_DEPTH) & (raw > 0)).any())
        ok = px > 0
        if ok.any() and (px[ok] + params["sdf_truncation"] + params["sdf_truncation_scale"] * px[ok] + 1e-4 + 1e-3 <= fp["zmin"][i]).all():
            n["skipped"] += 1
    return n


_REF = {}


def _reference(oracle, frames, **over):
    """the oracle's run of `frames` under PARAMS + over, once per parameter set: (engine, per-frame (updated voxels, compact blocks),
    block list before each frame).  The engine is never fed again."""
    key = tuple(sorted(over.items()))
    if key not in _REF:
        b = pu.make_engine(oracle, K, dict(PARAMS, **over), BLOCKS)
        per_frame, before = [], []
        for f in frames:
            before.append(b.dump_blocks()[0])
            pu.feed(b, f)
            s = b.stats()
            per_frame.append((int(s.last_updated_voxels), int(s.last_compact_blocks)))
        _REF[key] = (b, per_frame, before)
    return _REF[key]


def _run(hip, frames, counters=None, **over):
    a = pu.make_engine(hip, K, dict(PARAMS, **over), BLOCKS)
    if counters is not None:
        a.set_profile(True)
    for i, f in enumerate(frames):
        pu.feed(a, f)
        if counters is not None:
            s = a.stats()
            assert (int(s.last_updated_voxels), int(s.last_compact_blocks)) == counters[i], (i, s.last_updated_voxels, s.last_compact_blocks, counters[i])
    if counters is not None:
        a.set_profile(False)
    a.sync()
    assert a.stats().error_flags == 0
    return a


def test_early_out_and_every_footprint_class(hip, oracle):
    """Map and per-frame counters (voxels updated, blocks in the frustum) equal to the oracle's on a stream in which, counted on the
    host from the oracle's block list: blocks without a tile, blocks staged in two rounds and in one, blocks over invalid pixels
    and over the band around the integration distance all occur in frame 1, and frame 2 leaves blocks wholly behind the wall
    (a wrong skip, or a missed one that updates nothing, would show in the counters or the map)."""
    frames = _stream()
    b, per_frame, before = _reference(oracle, frames)
    n1, n2 = _regimes(before[1], frames[1], PARAMS), _regimes(before[2], frames[2], PARAMS)
    print("frame 1:", n1, "frame 2:", n2, "counters:", per_frame)
    assert n1["no_tile"] >= 4 and n1["two_rounds"] >= 8 and n1["one_round"] >= 50
    assert n1["invalid_px"] >= 4 and n1["beyond_px"] >= 4
    assert n2["skipped"] >= 8 and n1["skipped"] == 0
    assert all(u > 0 and m > 0 for u, m in per_frame)
    a = _run(hip, frames, counters=per_frame)
    r = pu.compare_maps(a, b)
    assert r["blocks"] > 100 and r["sdf_bit_exact"] and r["sumsq_bit_exact"]


@pytest.mark.parametrize("sample,wmax,n,top", [(255, 255, 2, 255), (1, 4, 6, 4)], ids=["sum-510", "clamp-at-4"])
def test_weight_sums_and_clamp(hip, oracle, sample, wmax, n, top):
    """The weighted mean divides by w0 + w1: 255 + 255 = 510 is the largest sum there is (the table of refined reciprocals ends
    there); weight_max 4 clamps from the fifth frame on.  The two poses alternate, so from the second frame on a lane's four
    voxels mix fresh ones (w0 = 0) with weighted ones — counted on the host from the oracle's dumps."""
    two = _stream()[:2]
    frames = [two[i & 1] for i in range(n)]
    over = dict(integration_weight_sample=sample, integration_weight_max=wmax)
    b = pu.make_engine(oracle, K, dict(PARAMS, **over), BLOCKS)
    pu.feed(b, frames[0])
    d0, v0 = b.dump_blocks()
    pu.feed(b, frames[1])
    d1, v1 = b.dump_blocks()
    # blocks are sorted by coordinate in both dumps: the weights of frame 0's blocks before and after frame 1, four x-adjacent voxels a row
    pos = {tuple(k): i for i, k in enumerate(_xyz(d1).tolist())}
    idx = np.array([pos.get(tuple(k), -1) for k in _xyz(d0).tolist()])
    w_before = v0["weight"][idx >= 0].reshape(-1, 4).astype(int)
    w_after = v1["weight"][idx[idx >= 0]].reshape(-1, 4).astype(int)
    s_before, s_after = v0["sdf"][idx >= 0].reshape(-1, 4), v1["sdf"][idx[idx >= 0]].reshape(-1, 4)
    fresh = (w_before == 0) & (w_after > 0)
    again = (w_before > 0) & ((w_after != w_before) | (s_after != s_before))  # a weighted voxel that frame 1 wrote
    mixed = int((fresh.any(1) & again.any(1)).sum())
    print("float4 groups mixing fresh and weighted voxels in frame 1:", mixed)
    assert mixed >= 100
    for f in frames[2:]:
        pu.feed(b, f)
    a = _run(hip, frames, **over)
    r = pu.compare_maps(a, b)
    assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
    assert a.dump_blocks()[1]["weight"].max() == top


@pytest.mark.parametrize("env,over", [
    (dict(MRH_SAFE_DIV="1"), {}),
    (dict(MRH_PIPE="0"), {}),
    (dict(MRH_PIPE="1", MRH_PIPE_PERIOD="2"), {}),
    ({}, dict(n_frames_invalidate_voxels=2)),
    ({}, dict(sdf_var_threshold=0.005)),
], ids=["safe-div", "serial", "pipe-period-2", "starve-period-2", "multi-resolution"])
def test_the_same_stream_under_every_instantiation(hip, oracle, monkeypatch, env, over):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    frames = _stream()
    b, _, _ = _reference(oracle, frames, **over)
    a = _run(hip, frames, **over)  # no statistics between the frames: reading them waits for the device, and a context that waits does not pipeline
    r = pu.compare_maps(a, b)
    assert r["blocks"] > 100 and r["sdf_bit_exact"] and r["sumsq_bit_exact"]


def test_spherical_stream_32_x_128(hip, oracle):
    """the spherical instantiation (every lookup a gather, no early-out): 32 x 128 range images of the street, GC every frame"""
    cam = synth.spherical_camera(32, 128)
    p = dict(synth.VBR_PARAMS, min_weight_threshold=1, n_frames_invalidate_voxels=100)
    engines = []
    for lib in (hip, oracle):
        e = capi.Engine(lib, capi.Params(num_sdf_blocks=BLOCKS, **p))
        e.set_camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["rows"], cam["cols"], p["min_depth"], 60.0, model=1)
        engines.append(e)
    a, b = engines
    scene = synth.street_canyon()
    for t, q in synth.drive_poses(3, step=0.5):
        depth, rgb = synth.spherical_range_image(scene, t, q, cam)
        for e in engines:
            e.set_pose(synth.quat_to_rot(q), t)
            e.upload_depth(depth)
            e.upload_rgb(rgb)
            assert not e.integrate()
    a.sync()
    r = pu.compare_maps(a, b)
    assert r["blocks"] > 200 and r["sdf_bit_exact"] and r["sumsq_bit_exact"]
    assert a.stats().error_flags == 0
