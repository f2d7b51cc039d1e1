"""CPU half of the point query (include/mrhash_query.h): the restatement of tests/query_ref.py pinned where the answer
is known without it — a linear field (SMOOTH reproduces it and its gradient exactly, MAP returns it at the centre of the eight-cell
cube), the piecewise-constant MAP field against the continuous SMOOTH one, the refusal rule — and the coverage conditions of the
GPU comparisons (tests/test_query_gpu.py), asserted here on the restatement alone."""
import numpy as np
import pytest

import mc_fields as mf
import query_ref as qr
from mrhash_amd import capi

F = np.float32
VS4 = F(2.0 ** -4)
LIN_A, LIN_C = np.array([0.5, -0.25, 0.125]), 0.0625  # dyadic: every value of the field below is exact in binary32


def linear_map():
    """A 4^3-block field at vs = 2^-4 whose voxel v (at world v vs) stores a . (v vs) + c, weight 1."""
    params = dict(mf.PARAMS, virtual_voxel_size=float(VS4))
    blocks = {}
    for b in mf.cluster((0, 0, 0), (4, 4, 4)):
        v = mf.block_voxels(b)
        blk = np.zeros(512, capi.VOXEL_DTYPE)
        blk["sdf"], blk["weight"], blk["rgb"] = (v * float(VS4)) @ LIN_A + LIN_C, 1, mf._rgb_of(v)
        blocks[b] = blk
    return qr.ref_map(params, blocks)


def linear_points(n=400, seed=11):
    """Points at odd 32nds of a voxel (no rounding tie anywhere), far enough inside for the gradient's stencils: P / vs in [3, 28]."""
    rng = np.random.default_rng(seed)
    q = rng.integers(3, 28, (n, 3)) + (2 * rng.integers(0, 16, (n, 3)) + 1) / 32.0
    return (q * float(VS4)).astype(F)  # exact


def test_smooth_reproduces_a_linear_field_and_its_gradient():
    m, P = linear_map(), linear_points()
    dist, grad, _, state = qr.query(m, P, smooth=True)
    assert np.all(state == (qr.BLOCK | qr.DIST | qr.GRAD))
    assert np.array_equal(dist.astype(np.float64), P.astype(np.float64) @ LIN_A + LIN_C)
    assert np.array_equal(grad.astype(np.float64), np.broadcast_to(LIN_A, grad.shape))


def test_map_is_the_linear_field_at_the_dual_cell_centre():
    m, P = linear_map(), linear_points()
    dist, grad, _, state = qr.query(m, P, smooth=False)
    assert np.all(state == (qr.BLOCK | qr.DIST | qr.GRAD))
    centre = qr.dual_centre(VS4, P)
    assert np.array_equal(dist.astype(np.float64), centre @ LIN_A + LIN_C)
    assert np.array_equal(grad.astype(np.float64), np.broadcast_to(LIN_A, grad.shape))
    assert np.any(dist.astype(np.float64) != P.astype(np.float64) @ LIN_A + LIN_C)  # ... which is not the field at P


def test_map_is_piecewise_constant_and_smooth_is_not():
    """Two points 0.15 voxel apart inside one dual cell: the MAP field returns the same bits, the SMOOTH field does not."""
    m = linear_map()
    P = (np.array([[10.6, 10.6, 10.6], [10.75, 10.6, 10.6]]) * float(VS4)).astype(F)
    assert np.array_equal(qr.dual_centre(VS4, P[0]), qr.dual_centre(VS4, P[1]))
    d_map, g_map, _, s_map = qr.query(m, P, smooth=False)
    d_smooth, _, _, s_smooth = qr.query(m, P, smooth=True)
    assert np.all(s_map & qr.DIST) and np.all(s_smooth & qr.DIST)
    assert d_map[0].tobytes() == d_map[1].tobytes() and g_map[0].tobytes() == g_map[1].tobytes()
    assert d_smooth[0].tobytes() != d_smooth[1].tobytes()
    # a sign field shows the same: the MAP value is the mean of eight cells whatever the position inside the dual cell
    m = qr.ref_map(mf.PARAMS, mf.sign_field(7))
    vs = float(mf.PARAMS["virtual_voxel_size"])
    P = (np.array([[10.6, 12.7, 9.55], [10.75, 12.7, 9.55]]) * vs).astype(F)
    d_map, _, _, s_map = qr.query(m, P, smooth=False)
    d_smooth, _, _, s_smooth = qr.query(m, P, smooth=True)
    assert np.all(s_map & qr.DIST) and np.all(s_smooth & qr.DIST)
    assert d_map[0].tobytes() == d_map[1].tobytes() and d_smooth[0].tobytes() != d_smooth[1].tobytes()


def test_refusal_rule():
    m = linear_map()
    bound = qr.bound(VS4)
    assert bound == F(65536.0)
    inside = mf.prevfloat(bound)
    nan, inf = F(np.nan), F(np.inf)
    pts = np.array([[nan, 1, 1], [1, nan, 1], [1, 1, nan], [inf, 1, 1], [1, -inf, 1], [1, 1, inf], [bound, 1, 1], [1, -bound, 1], [1, 1, bound],
                    [inside, 1, 1], [1, -inside, 1], [inside, inside, -inside], [0, 0, 0], [-0.0, 0.0, -0.0], [1, 1, 1]], F)
    refused = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], bool)
    I, Z = np.eye(3, dtype=F), np.zeros(3, F)
    for smooth in (False, True):
        dist, grad, rgbw, state = qr.query(m, pts, smooth=smooth)
        assert np.array_equal(state == qr.REFUSED, refused)
        assert np.array_equal((state & qr.REFUSED) != 0, refused)
        for out in (dist, grad, rgbw):  # +0 in every other output of a refused point
            assert not np.ascontiguousarray(out[refused]).view(np.uint8).any()
        # (0, 0, 0) is a position like any other without a pose: voxel (0, 0, 0), at the cluster's corner (the MAP stencil leaves it)
        assert state[12] & qr.BLOCK and state[13] == state[12] and bool(state[12] & qr.DIST) == smooth and state[14] & qr.DIST
        # with a pose the same input is a missing return, whatever the signs of its zeros; the rest is unchanged under the identity
        d2, g2, c2, s2 = qr.query(m, pts, R=I, t=Z, smooth=smooth)
        assert s2[12] == qr.REFUSED and s2[13] == qr.REFUSED and d2[12].tobytes() == F(0).tobytes()
        keep = np.ones(len(pts), bool)
        keep[12:14] = False
        assert qr.same_bits(s2[keep], state[keep]) and qr.same_bits(d2[keep], dist[keep]) and qr.same_bits(g2[keep], grad[keep])
    # a pose that moves a point across the bound: the test is on P, not on the input
    P, ref = qr.world_points(VS4, np.array([[inside, 0, 0], [1, 0, 0]], F), R=I, t=np.array([1024.0, 0, 0], F))
    assert list(ref) == [True, False]
    # a zero input with a pose is refused even where P = t is a good position
    assert list(qr.world_points(VS4, np.zeros((1, 3), F), R=I, t=np.array([1, 1, 1], F))[1]) == [True]


def test_outputs_not_asked_for():
    m = linear_map()
    P = linear_points(20)
    dist, grad, rgbw, state = qr.query(m, P, smooth=False, gradient=False, colour=False)
    full = qr.query(m, P, smooth=False)
    assert grad is None and rgbw is None and qr.same_bits(dist, full[0])
    assert np.array_equal(state, full[3] & ~np.uint8(qr.GRAD)) and np.all(full[3] & qr.GRAD)
    assert np.array_equal(full[2][:, 3], np.ones(20, np.uint8)) and full[2][:, :3].any()


# ---- the coverage conditions of the GPU comparisons, on the restatement alone --------------------------------------------------

VAR_PARAMS = dict(mf.PARAMS, sdf_var_threshold=0.005)
FIELDS = {
    "dense": (mf.PARAMS, dict()),
    "holes": (mf.PARAMS, dict(holes=0.03, starved=0.5, absent=0.1)),
    "variance_adaptive": (VAR_PARAMS, dict(holes=0.02, absent=0.1, coarse=0.4)),
}


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("smooth", [False, True])
def test_coverage_of_the_field_tests(name, smooth):
    """Measured with these points (of 1 500): dense MAP 1044 DIST / 845 GRAD, SMOOTH 1050; holes MAP 751 / 275, SMOOTH 759;
    variance-adaptive MAP 712 / 318, SMOOTH 723, COARSE 389."""
    params, kw = FIELDS[name]
    m = qr.ref_map(params, mf.sign_field(7, params=params, **kw))
    pts = qr.cluster_points(params["virtual_voxel_size"])
    assert len(pts) == qr.CLUSTER_POINTS
    cov = qr.coverage(qr.query(m, pts, smooth=smooth)[3])
    print(name, "SMOOTH" if smooth else "MAP", cov)
    assert cov["dist"] >= 0.40 and cov["grad"] >= 0.15 and cov["refused"] == 0
    if name == "variance_adaptive":
        assert cov["coarse"] >= 0.15
    else:
        assert cov["coarse"] == 0


@pytest.mark.parametrize("smooth", [False, True])
def test_coverage_of_the_ladder(smooth):
    """Measured (of 600): MAP 309 DIST / 76 GRAD, SMOOTH 308."""
    blocks, p = mf.ladder(0.05)
    pts = qr.ladder_points(blocks, 0.05)
    assert len(pts) == qr.LADDER_POINTS
    cov = qr.coverage(qr.query(qr.ref_map(p, blocks), pts, smooth=smooth)[3])
    print("ladder", "SMOOTH" if smooth else "MAP", cov)
    assert cov["dist"] >= 0.30 and cov["grad"] >= 0.08
