"""A restatement of render-free tracking (include/mrhash_sdftrack.h) in numpy, built from what the other
restatements already pin: track_ref's back-projection, exact sums, binary64 solve and pose update, and align_ref's per-sample
linearisation against the SMOOTH field — called with the sample's own distance s = 0, the pivot c = 0, tau = t and dist_max =
band, which is D20's reading of D19: q = P - 0 = P, e = 0 - d, and |e| = |d| < band passes the residual gate by itself.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

import align_ref as ar
import remap_ref as rm
import track_ref as tr

F = np.float32
D = np.float64
TRACK_OK, TRACK_LOST = 0, 1
MAX_POINTS = 1 << 24
GATES = ("range", "corners", "band", "lever")  # steps 3 (its three tests) and 6; align_ref's residual gate cannot reject
ZERO3 = np.zeros(3, F)


def defaults(band, iterations, min_pixels, sdf_truncation):
    """The parameter block with its zeros replaced (include/mrhash_sdftrack.h)."""
    return F(sdf_truncation) if F(band) == 0 else F(band), int(iterations) or 10, int(min_pixels) or 64


def depth_samples(depth, K, min_depth, max_depth):
    """Step 1 of the depth form for every pixel, raster order: (valid [n] bool, p_c [n, 3] f32).  K = (fx, fy, cx, cy, rows, cols)."""
    rows, cols = int(K[4]), int(K[5])
    Dv = np.ascontiguousarray(depth, F).reshape(rows * cols)
    r, c = np.mgrid[0:rows, 0:cols]
    with np.errstate(all="ignore"):
        ok = (Dv > F(min_depth)) & (Dv <= F(max_depth))  # a NaN fails
        dx, dy = tr._dir(K, r.ravel(), c.ravel())
        p = np.stack([(Dv * dx).astype(F), (Dv * dy).astype(F), Dv], -1)
    return ok, p


def point_samples(points, min_depth, max_depth):
    """Step 1 of the points form: (valid [n] bool, p_s [n, 3] f32)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        rho = np.sqrt((((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)).astype(F)
        ok = (rho > F(min_depth)) & (rho <= F(max_depth))  # (0, 0, 0), a NaN and an infinity fail
    return ok, p


def sample_terms(m: rm.Source, valid, p, R32, t32, band, max_depth):
    """Steps 2-6 for every sample: (accepted [n] bool, J~ [n, 6] int64, e~ [n] int64, rejected {gate: count among the valid})."""
    n = len(p)
    ok, Jt, et = np.zeros(n, bool), np.zeros((n, 6), np.int64), np.zeros(n, np.int64)
    idx = np.flatnonzero(valid)
    rejected = {k: 0 for k in GATES}
    if len(idx):
        o, J, e, rej = ar.sample_terms(m, p[idx], np.zeros(len(idx), F), ZERO3, R32, t32, band, band, tr.angle_scale(max_depth))
        assert rej["residual"] == 0  # |e| = |d| < band
        ok[idx], Jt[idx], et[idx] = o, J, e
        rejected = {k: rej[k] for k in GATES}
    return ok, Jt, et, rejected


def linearise(m, valid, p, R32, t32, band, max_depth, order=None) -> np.ndarray:
    ok, Jt, et, _ = sample_terms(m, valid, p, R32, t32, band, max_depth)
    return tr.sums_of(ok, Jt, et, order=order)


def fit(m, valid, p, max_depth, band, iterations, min_pixels, R_init, t_init) -> dict:
    """The loop of D14 over the samples (valid, p).  band, iterations and min_pixels are taken as given (see defaults()).  Returns R,
    t (float32), status, iterations_done, sums (int64 [32]), pixels, rms, valid (the samples step 1 accepted) and `rejected`: per
    gate, the valid samples it rejected over all linearisations."""
    R32, t32 = np.asarray(R_init, F).reshape(3, 3), np.asarray(t_init, F).reshape(3)
    R, t = R32.astype(D), t32.astype(D)
    status, done, sums = TRACK_LOST, 0, np.zeros(32, np.int64)
    rejected = {k: 0 for k in GATES}
    if len(p):  # an empty cloud is lost: nothing is linearised
        status = TRACK_OK
        for _ in range(int(iterations)):
            ok, Jt, et, rej = sample_terms(m, valid, p, R.astype(F), t.astype(F), band, max_depth)
            for k in GATES:
                rejected[k] += rej[k]
            sums = tr.sums_of(ok, Jt, et)
            xi = tr.solve(sums, max_depth, min_pixels)
            if xi is None:
                status = TRACK_LOST
                break
            R, t = tr.update(R, t, xi)
            done += 1
    n = int(sums[28])
    rms = float(np.sqrt(D(sums[27]) / D(n)) / D(262144.0)) if n else 0.0
    return dict(R=R.astype(F), t=t.astype(F), status=status, iterations_done=done, sums=sums, pixels=n, rms=rms, valid=int(np.count_nonzero(valid)),
                rejected=rejected)


def track_depth(params, blocks, depth, K, min_depth, max_depth, R_init, t_init, band=0.0, iterations=0, min_pixels=0) -> dict:
    """mrh_track_depth_sdf as D20 defines it, on the map (params, blocks) or on a ready rm.Source given as `blocks`."""
    m = blocks if isinstance(blocks, rm.Source) else rm.Source(params, blocks)
    band, iterations, min_pixels = defaults(band, iterations, min_pixels, params["sdf_truncation"])
    valid, p = depth_samples(depth, K, min_depth, max_depth)
    return fit(m, valid, p, max_depth, band, iterations, min_pixels, R_init, t_init)


def track_points(params, blocks, points, min_depth, max_depth, R_init, t_init, band=0.0, iterations=0, min_points=0) -> dict:
    """mrh_track_points_sdf as D20 defines it."""
    m = blocks if isinstance(blocks, rm.Source) else rm.Source(params, blocks)
    band, iterations, min_points = defaults(band, iterations, min_points, params["sdf_truncation"])
    valid, p = point_samples(points, min_depth, max_depth)
    assert len(p) <= MAX_POINTS
    return fit(m, valid, p, max_depth, band, iterations, min_points, R_init, t_init)


def same_result(got: dict, want: dict) -> list:
    """Names of the outputs of a call that differ in any bit."""
    bad = [k for k in ("R", "t", "sums") if not rm.same_bits(np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1))]
    bad += [k for k in ("status", "iterations_done", "pixels") if int(got[k]) != int(want[k])]
    bad += [k for k in ("rms",) if np.float64(got[k]).tobytes() != np.float64(want[k]).tobytes()]
    return bad


# ---- the corner view: align_ref's corner destination seen by a pinhole camera that looks at the vertex ----------------------------

VIEW_K = (60.0, 60.0, 32.0, 24.0, 48, 64)  # fx, fy, cx, cy, rows, cols
VIEW_NEAR, VIEW_FAR = 0.1, 3.0
VIEW_UP = np.array([0.1, 0.9, 0.3], D)


def corner_view():
    """(R [3, 3] f32, t [3] f32): the camera at vertex + 1.0 * axis — the vertex solves CORNER_N v = CORNER_O, the axis is the
    normalised sum of CORNER_N's rows, so the camera sits inside the corner (every n_i . x - o_i > 0) and sees all three planes —
    looking at the vertex: z forward, x right, y down with the up hint VIEW_UP."""
    vertex = np.linalg.solve(ar.CORNER_N, ar.CORNER_O)
    axis = ar.CORNER_N.sum(axis=0)
    axis /= np.linalg.norm(axis)
    eye = vertex + 1.0 * axis
    z = (vertex - eye) / np.linalg.norm(vertex - eye)
    x = np.cross(z, VIEW_UP)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], -1).astype(F), eye.astype(F)


def corner_depth(R, t, K=VIEW_K):
    """The analytic depth image of the corner from the pose (R, t): per pixel the ray (d_c as D14 states it, binary64 here) leaves the
    region min_i (n_i . x - o_i) > 0 at the smallest positive s with n_i . (t + s R d_c) = o_i; its depth is s (d_c.z = 1).  0 where
    there is none."""
    rows, cols = int(K[4]), int(K[5])
    r, c = np.mgrid[0:rows, 0:cols]
    d = np.stack([((c - K[2]) - 0.5) / K[0], ((r - K[3]) - 0.5) / K[1], np.ones_like(r, D)], -1)
    w = d @ np.asarray(R, F).astype(D).T
    num = ar.CORNER_O - ar.CORNER_N @ np.asarray(t, F).astype(D)  # [3]
    den = w @ ar.CORNER_N.T                                       # [rows, cols, 3]
    with np.errstate(all="ignore"):
        s = np.where(den < 0, num / den, np.inf)  # the camera is inside: only a ray that runs against n_i leaves through plane i
    s = np.where(s > 0, s, np.inf).min(axis=-1)
    return np.where(np.isfinite(s), s, 0.0).astype(F)


def view_start():
    """The start of the corner-view tests: 0.06 rad and 86.6 mm off the truth."""
    return ar.perturbed(*corner_view(), angle=0.06, dt=(0.05, -0.05, 0.05))


# ---- the destinations of the tests (tests/test_sdftrack.py asserts their coverage, tests/test_sdftrack_gpu.py compares) -------------

DESTINATIONS = ("truth", "adaptive_dst", "holes_dst", "far", "beyond", "plane")  # align_ref's scenes, their destination half
# two of this file's own, for the gates that no destination above reaches: the truth's map under a band a third of the truncation
# (the start lies outside it for most pixels), and a map whose stored distance is three times the true one (clamped), so that a
# gradient component passes 2 and the translation part of the row leaves the fixed-point range
GATE_SCENES = ("narrow_band", "steep")
# expected to converge with at least half of the valid pixels accepted.  holes_dst converges too, but with 5 % of its cells at
# weight 0 only 0.95^8 of the corner octets are complete and a little under half of the pixels give a row: it is the corners gate's scene
CONVERGING = ("truth", "adaptive_dst", "far")
LOST = ("beyond", "plane")
STEEP = 3.0
_cache = {}


def destination(name: str) -> dict:
    """dict(params, blocks, depth, K, R, t, R_true, t_true): a destination map of align_ref (its `dp`, `db`), the corner view's depth image of it
    and the perturbed start.  far / beyond: the map is moved by whole blocks, and the camera with it.  plane: a single plane seen
    head-on from 1 m — sliding along it costs nothing, so the pivot gate ends the first step."""
    if name in _cache:
        return _cache[name]
    s = ar.scene("truth" if name in GATE_SCENES else name)
    params, blocks = s["dp"], s["db"]
    kw = dict(band=0.05) if name == "narrow_band" else {}
    if name == "steep":
        trunc = F(params["sdf_truncation"])
        blocks = {b: v.copy() for b, v in blocks.items()}
        for v in blocks.values():
            v["sdf"] = np.clip((v["sdf"] * F(STEEP)).astype(F), -trunc, trunc)
    vs = float(F(params["virtual_voxel_size"]))
    if name == "plane":
        n, d = np.asarray(rm.PLANE_N, D), float(rm.PLANE_D)
        centre = np.full(3, 16 * vs)  # the middle of the 4^3 blocks
        foot = centre - (n @ centre - d) * n
        eye = foot + 1.0 * n
        z = -n
        x = np.cross(z, VIEW_UP)
        x /= np.linalg.norm(x)
        R_true, t_true = np.stack([x, np.cross(z, x), z], -1).astype(F), eye.astype(F)
        K = (60.0, 60.0, 8.0, 6.0, 12, 16)  # a narrow view: it stays on the 4^3 blocks
        rows, cols = K[4], K[5]
        r, c = np.mgrid[0:rows, 0:cols]
        dirs = np.stack([((c - K[2]) - 0.5) / K[0], ((r - K[3]) - 0.5) / K[1], np.ones_like(r, D)], -1) @ R_true.astype(D).T
        depth = ((d - n @ t_true.astype(D)) / (dirs @ n)).astype(F)
        R0, t0 = ar.perturbed(R_true, t_true, angle=0.01, dt=(0.005, -0.005, 0.005))
    else:
        R_true, t_true = corner_view()
        K = VIEW_K
        depth = corner_depth(R_true, t_true)
        shift = {"far": ar.FAR_SHIFT, "beyond": ar.BEYOND_SHIFT}.get(name)
        if shift is not None:
            t_true = (t_true.astype(D) + np.asarray(shift, D) * 8 * vs).astype(F)
        R0, t0 = ar.perturbed(R_true, t_true, angle=0.06, dt=(0.05, -0.05, 0.05))
    _cache[name] = dict(params=params, blocks=blocks, depth=depth, K=K, R=R0, t=t0, R_true=R_true, t_true=t_true, kw=kw)
    return _cache[name]


def run_destination(name: str, **kw) -> dict:
    s = destination(name)
    return track_depth(s["params"], s["blocks"], s["depth"], s["K"], VIEW_NEAR, VIEW_FAR, s["R"], s["t"], **dict(s["kw"], **kw))
