"""3DGS splat seeds on the GPU (mrh_splat.h) against the oracle: identical leaves (order included) and bit-identical
seeds.  The device decides node errors from exact integer statistics and evaluates the reference's fp32 summation
order only inside the rounding band around the threshold — the adversarial cases below put thresholds exactly on
node errors, and MRH_QTREE_LITERAL=1 forces the literal evaluation everywhere as a cross-check."""
import os

import numpy as np
import pytest

import parity_utils as pu
from mrhash_amd import capi, synth
from test_splat import np_node_error

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    return capi.load_hip()


@pytest.fixture(scope="module")
def oracle():
    return pu.oracle_lib()


def _same(a: capi.Engine, b: capi.Engine, thr, min_px):
    sa, sb = a.splat_seeds(thr, min_px), b.splat_seeds(thr, min_px)
    la, lb = a.qtree_leaves(), b.qtree_leaves()
    assert len(la) == len(lb), f"leaf count differs: {len(la)} vs {len(lb)}"
    assert np.array_equal(la, lb), "quad-tree leaves differ"
    assert len(sa) == len(sb), f"seed count differs: {len(sa)} vs {len(sb)}"
    assert sa.tobytes() == sb.tobytes(), "seeds differ"
    return len(la), len(sa)


def test_replica_stream_seeds_match_oracle(hip, oracle):
    """configs[1] stand-in, shipped parameters (configurations/params.json:9-10: thresh 0.1, min pixel size 1)."""
    K = synth.REPLICA_640
    a = pu.make_engine(hip, K, synth.REPLICA_PARAMS, num_sdf_blocks=65536)
    b = pu.make_engine(oracle, K, synth.REPLICA_PARAMS, num_sdf_blocks=65536)
    counts = []
    for f in synth.replica_stream(4):
        pu.feed(a, f)
        pu.feed(b, f)
        counts.append(_same(a, b, 0.1, 1))
    assert counts[0][1] > 1000 and all(c[0] > 1000 for c in counts)
    assert counts[1][1] < counts[0][1]  # after the first frame only newly seen surface seeds
    pu.compare_maps(a, b)  # seeding leaves the map alone
    a.close()
    b.close()


def _image_pair(hip, oracle, rows, cols, rgb, depth, params=None, blocks=32768):
    K = synth.Intrinsics(0.9 * cols, 0.9 * cols, cols / 2.0, rows / 2.0, rows, cols)
    out = []
    for lib in (hip, oracle):
        e = pu.make_engine(lib, K, dict(synth.CFG1_PARAMS, **(params or {})), num_sdf_blocks=blocks)
        e.set_pose(np.eye(3, dtype=F32), np.zeros(3, F32))
        e.upload_depth(depth)
        e.upload_rgb(rgb)
        assert not e.integrate()
        out.append(e)
    return out


@pytest.mark.parametrize("rows,cols", [(480, 640), (680, 1200), (61, 97), (33, 1), (1, 1), (7, 300), (256, 256)])
def test_image_shapes_thresholds_and_pixel_sizes(hip, oracle, rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    rgb = synth.textured_image(rows, cols, seed=cols)
    depth = (1.0 + 0.2 * rng.random((rows, cols))).astype(F32)
    depth[rng.random((rows, cols)) < 0.05] = 0.0
    a, b = _image_pair(hip, oracle, rows, cols, rgb, depth)
    scale = rows * cols / 307200.0
    for thr, min_px in [(0.1 * scale, 1), (0.01 * scale, 0), (0.0, 1), (1e-6 * scale, 3), (1e9, 1), (-1.0, 2), (0.003 * scale, 7)]:
        _same(a, b, thr, min_px)
    a.close()
    b.close()


def test_pure_noise_and_saturated_images(hip, oracle):
    rows, cols = 120, 160
    rng = np.random.default_rng(5)
    depth = np.full((rows, cols), 1.0, F32)
    for rgb in (rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8), np.full((rows, cols, 3), 255, np.uint8),
                np.zeros((rows, cols, 3), np.uint8), (rng.integers(0, 2, (rows, cols, 3)) * 255).astype(np.uint8)):
        a, b = _image_pair(hip, oracle, rows, cols, rgb, depth)
        for thr in (0.0, 1e-4, 0.02, 0.5):
            _same(a, b, thr, 1)
        a.close()
        b.close()


def test_thresholds_exactly_on_node_errors(hip, oracle):
    """err <= threshold with err == threshold (and one ulp either side): the device's exact-statistics shortcut cannot
    decide these, they must go through the literal summation order and agree with the oracle."""
    rows, cols = 96, 128
    rgb = synth.textured_image(rows, cols, seed=11)
    depth = np.full((rows, cols), 1.2, F32)
    a, b = _image_pair(hip, oracle, rows, cols, rgb, depth)
    nodes = [(0, 0, cols, rows), (0, 0, cols // 2, rows // 2), (cols // 2, rows // 2, cols - cols // 2, rows - rows // 2),
             (0, rows // 2, cols // 4, rows // 4), (cols // 2, 0, 16, 12), (64, 48, 8, 6)]
    for (x0, y0, w, h) in nodes:
        err = np_node_error(rgb, x0, y0, w, h)
        for thr in (err, np.nextafter(err, F32(np.inf)), np.nextafter(err, F32(-np.inf))):
            _same(a, b, float(thr), 1)
    a.close()
    b.close()


def test_literal_mode_gives_the_same_tree(hip, oracle):
    rows, cols = 240, 320
    rgb = synth.textured_image(rows, cols, seed=2)
    depth = np.full((rows, cols), 1.0, F32)
    os.environ["MRH_QTREE_LITERAL"] = "1"
    try:
        a, b = _image_pair(hip, oracle, rows, cols, rgb, depth)
    finally:
        del os.environ["MRH_QTREE_LITERAL"]
    c, _ = _image_pair(hip, oracle, rows, cols, rgb, depth)
    for thr, min_px in [(0.02, 1), (0.0005, 0)]:
        _same(a, b, thr, min_px)
        _same(c, b, thr, min_px)
    for e in (a, b, c, _):
        e.close()


def test_multires_map_and_moving_camera(hip, oracle):
    """Seeds on a variance-adaptive map (coarse blocks are looked up with the reference's index rule) under real poses."""
    K = synth.REPLICA_640
    params = dict(synth.REPLICA_PARAMS, sdf_var_threshold=0.01)
    a = pu.make_engine(hip, K, params, num_sdf_blocks=65536)
    b = pu.make_engine(oracle, K, params, num_sdf_blocks=65536)
    n = []
    for f in synth.replica_stream(5, noise_sigma=0.002):
        pu.feed(a, f)
        pu.feed(b, f)
        n.append(_same(a, b, 0.1, 1))
    assert n[-1][1] > 0
    a.close()
    b.close()


def test_first_seeding_call_and_a_camera_change_leave_the_other_buffers_alone(hip, oracle):
    """Round-2 advisor finding: the quad-tree (re)allocation branch of mrh_splat_seeds — first call, or another image shape —
    also released the soup / pack / halo / cloud buffers and the marching-cubes events while their capacities stayed, so the
    next extraction wrote triangles through a null pointer.  Sequence: integrate, extract, first seeding call, extract again,
    another camera shape, seed, extract, pack; every step against the oracle."""
    a = pu.make_engine(hip, synth.CFG1, dict(synth.CFG1_PARAMS), 16384)
    b = pu.make_engine(oracle, synth.CFG1, dict(synth.CFG1_PARAMS), 16384)
    f = synth.cfg1_sphere()
    for e in (a, b):
        pu.feed(e, f)
    a.set_profile(True)  # the marching-cubes launches carry events in profile mode: they must survive the seeding call, too
    m0 = pu.compare_meshes(a, b)
    _same(a, b, 0.002, 1)                      # first call: quad-tree buffers are allocated
    m1 = pu.compare_meshes(a, b)               # the soup buffer of the first extraction is still there
    assert m1["triangles"] == m0["triangles"] > 1000 and a.stats().last_mc_count_ms > 0
    a.set_sharding(0, 2, 1)
    ptr, n, dev = a.pack_blocks(capi.PACK_OWNER, 0)
    assert n > 0 and dev
    a.set_sharding(0, 1, 0)
    # another image shape: the quad-tree buffers are re-allocated
    K2 = synth.Intrinsics(96.0, 96.0, 48.0, 40.0, 80, 96)
    rng = np.random.default_rng(3)
    depth = (1.2 + 0.1 * rng.random((80, 96))).astype(F32)
    rgb = synth.textured_image(80, 96, seed=2)
    for e in (a, b):
        e.set_camera(K2.fx, K2.fy, K2.cx, K2.cy, K2.rows, K2.cols, 0.01, 30.0)
        e.set_pose(np.eye(3, dtype=F32), np.zeros(3, F32))
        e.upload_depth(depth)
        e.upload_rgb(rgb)
        assert not e.integrate()
    _same(a, b, 0.001, 1)
    pu.compare_meshes(a, b)
    a.set_sharding(0, 2, 1)
    ptr2, n2, _ = a.pack_blocks(capi.PACK_OWNER, 0)
    assert n2 >= n
    a.set_sharding(0, 1, 0)
    pu.compare_maps(a, b)
    a.close()
    b.close()


def test_seeding_with_alternating_image_shapes(hip, oracle):
    """One context seeded under two image shapes in turn (A, B, A, B): the quad-tree buffers are sized by the potential node
    count of the shape, so every call reallocates them — smaller, larger, smaller — and no call may find the size of another
    shape recorded over its buffers.  Seeds and leaves against the oracle after every call, the mesh at the end."""
    a = pu.make_engine(hip, synth.CFG1, dict(synth.CFG1_PARAMS), 16384)
    b = pu.make_engine(oracle, synth.CFG1, dict(synth.CFG1_PARAMS), 16384)
    p = capi.Params(num_sdf_blocks=16384, **synth.CFG1_PARAMS)
    KA, KB = synth.CFG1, synth.Intrinsics(96.0, 96.0, 48.0, 40.0, 80, 96)
    rng = np.random.default_rng(3)
    counts = []
    for i, zc in enumerate((None, 1.51)):
        fa = synth.cfg1_sphere() if zc is None else synth.cfg1_sphere(zc=zc)
        depth = (1.2 + 0.1 * rng.random((KB.rows, KB.cols))).astype(F32)
        rgb = synth.textured_image(KB.rows, KB.cols, seed=2 + i)
        for e in (a, b):
            e.set_camera(KA.fx, KA.fy, KA.cx, KA.cy, KA.rows, KA.cols, p.min_depth, p.max_depth)
            pu.feed(e, fa)
        counts.append(_same(a, b, 0.002, 1))
        for e in (a, b):
            e.set_camera(KB.fx, KB.fy, KB.cx, KB.cy, KB.rows, KB.cols, 0.01, 30.0)
            e.set_pose(np.eye(3, dtype=F32), np.zeros(3, F32))
            e.upload_depth(depth)
            e.upload_rgb(rgb)
            assert not e.integrate()
        counts.append(_same(a, b, 0.001, 1))
    assert all(leaves > 0 for leaves, _ in counts) and counts[0][1] > 0
    pu.compare_meshes(a, b)
    a.close()
    b.close()
