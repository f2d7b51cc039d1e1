"""The free-space layer's restatement (tests/freespace_ref.py) against answers written down by hand: which cells
a ray sets, where the frontier lies, what a site does to its cell, and the three properties the GPU tests rest on — a margin only
removes cells, two carves commute, a carve is idempotent.  No GPU."""
import numpy as np

import esdf_ref as er
import freespace_ref as fr
import raycast_ref as rr

VS = np.float32(0.02)
I3 = np.eye(3, dtype=np.float32)
Z3 = np.zeros(3, np.float32)


def _set_cells(layer):
    """The set cells of a layer as a sorted list of (x, y, z) in cell coordinates of the world (not of the layer)."""
    k, j, i = np.nonzero(layer.bits)
    return sorted((int(x + layer.origin[0]), int(y + layer.origin[1]), int(z + layer.origin[2])) for x, y, z in zip(i, j, k))


def test_one_ray_along_x_sets_the_cells_listed_and_all_are_frontier():
    """vs = 0.02, s = 1: a cell is 0.04 m.  One return at (0.31, 0, 0) seen from the origin: samples every 0.02 m (half a cell)
    at x = 0, 0.02, ..., 0.30 — voxels 0 .. 15 on the x axis, cells 0 .. 7.  Nothing else is known, so every one is a frontier."""
    layer = fr.Layer((-2, -2, -2), (12, 4, 4), 1)
    fr.carve_points(layer, VS, [[0.31, 0.0, 0.0]], I3, Z3, min_depth=0.0, max_depth=5.0)
    assert _set_cells(layer) == [(x, 0, 0) for x in range(8)]
    st = fr.box(layer, None, (-2, -2, -2), (12, 4, 4))
    assert np.array_equal(st != 0, layer.bits)
    assert np.all(st[layer.bits] == fr.FREE | fr.FRONTIER)
    # the same ray as the one pixel of a 1 x 1 image: c - cx - 0.5 = 0 with cx = -0.5, the camera's z axis turned onto world x
    R = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)
    img = fr.Layer((-2, -2, -2), (12, 4, 4), 1)
    fr.carve_depth(img, VS, [[0.31]], 1.0, 1.0, -0.5, -0.5, R, Z3, min_depth=0.0, max_depth=5.0)
    assert np.array_equal(img.bits, layer.bits)
    # a depth beyond max_depth carves up to max_depth; a NaN, a zero and a depth at min_depth carve nothing
    far = fr.Layer((-2, -2, -2), (12, 4, 4), 1)
    fr.carve_depth(far, VS, [[np.inf]], 1.0, 1.0, -0.5, -0.5, R, Z3, min_depth=0.0, max_depth=0.15)
    assert _set_cells(far) == [(x, 0, 0) for x in range(4)]  # x = 0 .. 0.14: voxels 0 .. 7
    for bad in (np.nan, 0.0, 0.1):
        none = fr.Layer((-2, -2, -2), (12, 4, 4), 1)
        fr.carve_depth(none, VS, [[bad]], 1.0, 1.0, -0.5, -0.5, R, Z3, min_depth=0.1, max_depth=5.0)
        assert not none.bits.any()


def test_step_larger_than_a_cell_skips_cells_and_the_box_clips():
    """s = 0, step 0.05 = 2.5 cells: samples at x = 0, 0.05, 0.10, 0.15 -> voxels 0, 3 (2.5 rounds away from zero), 5, 8 (7.5);
    the layer ends at cell 6, so 8 is dropped."""
    layer = fr.Layer((0, 0, 0), (7, 1, 1), 0)
    fr.carve_points(layer, VS, [[0.16, 0.0, 0.0]], I3, Z3, min_depth=0.0, max_depth=5.0, step=0.05)
    assert _set_cells(layer) == [(0, 0, 0), (3, 0, 0), (5, 0, 0)]


def test_fully_carved_group_has_its_frontier_on_the_shell():
    layer = fr.Layer((4, -9, 0), (3, 3, 3), 2)
    layer.bits[:] = True
    st = fr.box(layer, None, (3, -10, -1), (5, 5, 5))  # padded by one cell: the neighbours outside the layer are unknown
    inner = st[1:4, 1:4, 1:4]
    assert np.all(inner & fr.FREE) and np.all(st[0] == 0) and np.all(st[:, 0] == 0) and np.all(st[:, :, 4] == 0)
    want = np.ones((3, 3, 3), bool)
    want[1, 1, 1] = False
    assert np.array_equal((inner & fr.FRONTIER) != 0, want)
    # without the padding nothing unknown is inside the box: no frontier at all
    assert np.all(fr.box(layer, None, (4, -9, 0), (3, 3, 3)) == fr.FREE)


def test_a_site_makes_its_cell_occupied_and_not_a_frontier():
    """One site voxel (9, 2, 3) in a block of observed free space (block (1, 0, 0): voxels 8 .. 15, 0 .. 7, 0 .. 7), s = 1: the
    cell (4, 1, 1) is OCCUPIED, the block's other 63 cells are OBSERVED only.  With every cell of the box carved, the frontier is
    the free cells next to unknown space; the occupied cell is never one, and an observed neighbour does not open a frontier."""
    d, v = er.to_import(er.site_blocks([(9, 2, 3)]))
    m = rr.make_map(er.SPHERE_PARAMS, d, v)
    layer = fr.Layer((3, -1, -1), (6, 6, 6), 1)  # cells 3 .. 8: one cell of padding around the block's cells 4 .. 7, 0 .. 3, 0 .. 3
    st = fr.box(layer, m, (3, -1, -1), (6, 6, 6))
    assert st[2, 2, 1] == fr.OBSERVED | fr.OCCUPIED
    assert np.count_nonzero(st & fr.OCCUPIED) == 1 and np.count_nonzero(st & fr.OBSERVED) == 64 and not np.any(st & (fr.FREE | fr.FRONTIER))
    layer.bits[1:5, 1:5, 1:5] = True  # carve exactly the block's cells
    st = fr.box(layer, m, (3, -1, -1), (6, 6, 6))
    assert st[2, 2, 1] == fr.FREE | fr.OBSERVED | fr.OCCUPIED
    core = st[1:5, 1:5, 1:5]
    shell = np.ones((4, 4, 4), bool)
    shell[1:3, 1:3, 1:3] = False
    want = shell.copy()
    want[1, 1, 0] = False  # the occupied cell lies on the shell (x = 4 is the block's first cell): taken out
    assert np.array_equal((core & fr.FRONTIER) != 0, want)
    # a larger band makes more sites, a weight above the map's makes nothing observed
    assert np.count_nonzero(fr.box(layer, m, (3, -1, -1), (6, 6, 6), surface_band=1.0) & fr.OCCUPIED) == 64
    assert not np.any(fr.box(layer, m, (3, -1, -1), (6, 6, 6), min_weight=2) & (fr.OBSERVED | fr.OCCUPIED))


def _cloud(seed, n=40):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)).astype(np.float32)
    return (p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0.2, 0.9, (n, 1))).astype(np.float32)


def test_margin_subset_order_and_idempotence():
    A, B = _cloud(1), _cloud(2)
    R = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], np.float32)
    t = np.array([0.05, -0.02, 0.03], np.float32)
    new = lambda: fr.Layer((-12, -12, -12), (24, 24, 24), 1)
    carve = lambda L, pts, **kw: fr.carve_points(L, VS, pts, R, t, min_depth=0.05, max_depth=0.7, **kw)
    a = carve(new(), A)
    assert 100 < a.bits.sum() < a.bits.size
    am = carve(new(), A, margin=0.05)
    assert am.bits.sum() < a.bits.sum() and not np.any(am.bits & ~a.bits)
    ab, ba, aab = carve(carve(new(), A), B), carve(carve(new(), B), A), carve(carve(carve(new(), A), A), B)
    assert np.array_equal(ab.bits, ba.bits) and np.array_equal(ab.bits, aab.bits)
    assert np.array_equal(ab.bits, a.bits | carve(new(), B).bits)
    assert np.array_equal(carve(a.copy(), A).bits, a.bits)


def test_segments_by_hand():
    """The layer of the first test (cells 0 .. 7 on the x axis set, s = 1, half a cell = 0.02 m)."""
    layer = fr.Layer((-2, -2, -2), (12, 4, 4), 1)
    fr.carve_points(layer, VS, [[0.31, 0.0, 0.0]], I3, Z3, min_depth=0.0, max_depth=5.0)
    a = np.array([[0.0, 0, 0], [0.0, 0, 0], [0.1, 0, 0], [0.1, 0.1, 0], [0.0, 0, 0], [np.nan, 0, 0], [0.0, 0, 0], [0.0, 0, 0], [0, 20000.0, 0]], np.float32)
    b = np.array([[0.31, 0, 0], [0.41, 0, 0], [0.1, 0, 0], [0.1, 0.1, 0], [1.01, 0, 0], [0.1, 0, 0], [0.1, np.inf, 0], [0.0, 3e4, 0], [0, 21000.0, 0]], np.float32)
    status, counts = fr.segments(layer, VS, a, b)
    assert status.tolist() == [0, fr.SEG_UNKNOWN, 0, fr.SEG_UNKNOWN, fr.SEG_UNKNOWN, fr.SEG_BAD, fr.SEG_BAD, fr.SEG_BAD, fr.SEG_BAD]
    assert counts[0].tolist() == [16, 16]        # samples at x = 0 .. 0.30
    assert counts[1].tolist() == [21, 16]        # x = 0 .. 0.40: cells 8, 9 are in the layer and unset
    assert counts[2].tolist() == [1, 1]          # a point is one sample
    assert counts[3].tolist() == [1, 0]
    assert counts[4].tolist() == [51, 16]        # leaves the layer at x = 0.40 (cell 10): outside counts as not free
    # NaN; inf; 1.5 million samples; 50 000 samples the last of which lie beyond the bound 2^20 * 0.02 = 20 971.52 m
    assert counts[5:].tolist() == [[0, 0]] * 4
    # an explicit step: every 0.1 m along the set cells
    status, counts = fr.segments(layer, VS, [[0.0, 0, 0]], [[0.35, 0, 0]], step=0.1)
    assert status.tolist() == [0] and counts.tolist() == [[4, 4]]  # x = 0, 0.1, 0.2, 0.3


def test_sample_count_matches_the_literal_count():
    for z0, z1, step in ((0.0, 0.3, 0.1), (0.1, 5.0, 0.02), (0.0, 0.0, 0.5), (0.4, 6.0, 0.075), (0.0, 1000.0, 0.001)):
        z = fr.z_of(z0, step, np.arange(fr.MAX_SAMPLES + 1))
        n = int(np.count_nonzero(z <= np.float32(z1)))
        assert fr.sample_count(z0, z1, step) == (n if n <= fr.MAX_SAMPLES else 0)
    assert fr.sample_count(0.0, 1e9, 1e-3) == 0
