"""A restatement of scan tracking (include/mrhash_track.h) in numpy: the per-point linearisation of a sensor-frame
cloud against one spherical render of the map, in float32 without FMA.  Steps 6 to 9, the solve, the update and the loop are
D14's and come from tests/track_ref.py.  The model is given as its three sine-free images (range, world-frame normals and
sensor-frame points of one render from the initial pose): the GPU tests feed the library's own render, whose parity the raycast
tests pin, the CPU tests feed images of the analytic scenes (analytic_model) or the restatement of the render
(tests/raycast_sph_ref.py).  The arctangent and the arcsine are the oracle's orc_softmath (ops 2 and 3: include/mrh_softmath.h
compiled for the host), so the pixel a point falls into is the kernel's.

Test infrastructure only."""
from __future__ import annotations

import ctypes

import numpy as np

import parity_utils as pu
from track_ref import (D, E_ONE, F, J_LIMIT, J_ONE, TRACK_LOST, TRACK_OK, _rows3, angle_scale, defaults, pose_errors, solve, sums_of,  # noqa: F401
                       update)

_SOFT = []


def _softmath():
    if not _SOFT:
        o = pu.oracle_lib()
        o.orc_softmath.restype = ctypes.c_float
        o.orc_softmath.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_float]
        _SOFT.append(o.orc_softmath)
    return _SOFT[0]


def _atan2(y, x):
    f = _softmath()
    return np.array([f(2, float(a), float(b)) for a, b in zip(y, x)], F).reshape(len(y))


def _asin(x):
    f = _softmath()
    return np.array([f(3, float(a), 0.0) for a in x], F).reshape(len(x))


def _norm(x, y, z):
    return np.sqrt((((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)).astype(F)


def point_terms(points, K, min_depth, max_depth, dist_max, R32, t32, Rr, tr, Mr, Mn, Mp):
    """Steps 1-8 for every point of `points` [n, 3], in the order given: (accepted [n] bool, J~ [n, 6] int64, e~ [n] int64).
    K = (fx, fy, cx, cy, rows, cols) of the model render; Mr [rows, cols], Mn [rows, cols, 3], Mp [rows * cols, 3]."""
    rows, cols = int(K[4]), int(K[5])
    fx, fy, cx, cy = (F(v) for v in K[:4])
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(P)
    Mr = np.ascontiguousarray(Mr, F).reshape(rows, cols)
    Mn = np.ascontiguousarray(Mn, F).reshape(rows, cols, 3)
    Mp = np.ascontiguousarray(Mp, F).reshape(rows, cols, 3)
    R32 = np.asarray(R32, F).reshape(3, 3)
    Rr = np.asarray(Rr, F).reshape(3, 3)
    t32, tr = np.asarray(t32, F).reshape(3), np.asarray(tr, F).reshape(3)
    lo, hi = F(min_depth), F(max_depth)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        rp = _norm(x, y, z)
        ok = (rp > lo) & (rp <= hi)  # (0, 0, 0), a NaN and an infinity fail
        a = _rows3(R32, x, y, z)
        pw = [(a[i] + t32[i]).astype(F) for i in range(3)]
        w = [(pw[i] - tr[i]).astype(F) for i in range(3)]
        q = [((Rr[0][i] * w[0] + Rr[1][i] * w[1]).astype(F) + (Rr[2][i] * w[2]).astype(F)).astype(F) for i in range(3)]
        rq = _norm(*q)
        ok &= (rq > lo) & (rq <= hi)
        live = np.flatnonzero(ok)
        az, el = np.zeros(n, F), np.zeros(n, F)
        az[live] = _atan2(q[1][live], q[0][live])
        el[live] = _asin((q[2][live] / rq[live]).astype(F))
        u = (((fx * az).astype(F) + cx).astype(F) + F(1.0)).astype(F)
        v = (((fy * el).astype(F) + cy).astype(F) + F(1.0)).astype(F)
        ok &= (u >= 0) & (u < F(cols)) & (v >= 0) & (v < F(rows))
        c2 = np.where(ok, np.floor(u), 0).astype(np.int64)
        r2 = np.where(ok, np.floor(v), 0).astype(np.int64)
        ok &= Mr[r2, c2] != 0
        N = [Mn[r2, c2, i] for i in range(3)]
        ok &= ~((N[0] == 0) & (N[1] == 0) & (N[2] == 0))  # a hit without a gradient: no row, no count
        g = _rows3(Rr, Mp[r2, c2, 0], Mp[r2, c2, 1], Mp[r2, c2, 2])
        V = [(tr[i] + g[i]).astype(F) for i in range(3)]
        # steps 6-8 of D14
        dl = [(V[i] - pw[i]).astype(F) for i in range(3)]
        d2 = (((dl[0] * dl[0]).astype(F) + (dl[1] * dl[1]).astype(F)).astype(F) + (dl[2] * dl[2]).astype(F)).astype(F)
        ok &= d2 <= F(F(dist_max) * F(dist_max))  # a NaN is rejected
        e = (((N[0] * dl[0]).astype(F) + (N[1] * dl[1]).astype(F)).astype(F) + (N[2] * dl[2]).astype(F)).astype(F)
        J = [((a[1] * N[2]).astype(F) - (a[2] * N[1]).astype(F)).astype(F),
             ((a[2] * N[0]).astype(F) - (a[0] * N[2]).astype(F)).astype(F),
             ((a[0] * N[1]).astype(F) - (a[1] * N[0]).astype(F)).astype(F), N[0], N[1], N[2]]
        Sa = angle_scale(max_depth)
        Js = [(J[i] * (Sa if i < 3 else J_ONE)).astype(F) for i in range(6)]
        for i in range(6):
            ok &= np.abs(Js[i]) < J_LIMIT  # a NaN is rejected
        es = (e * E_ONE).astype(F)
        Jt = np.stack([np.where(ok, np.rint(Js[i]), 0).astype(np.int64) for i in range(6)], -1).reshape(n, 6)
        et = np.where(ok, np.rint(es), 0).astype(np.int64)
    return ok, Jt, et


def linearise(points, K, min_depth, max_depth, dist_max, R32, t32, Rr, tr, Mr, Mn, Mp, order=None) -> np.ndarray:
    return sums_of(*point_terms(points, K, min_depth, max_depth, dist_max, R32, t32, Rr, tr, Mr, Mn, Mp), order=order)


def track(points, K, min_depth, max_depth, dist_max, iterations, min_points, R_init, t_init, Mr, Mn, Mp) -> dict:
    """The loop of D14 over point_terms.  dist_max, iterations and min_points are taken as given (see defaults()).  Returns R, t
    (float32), status, iterations_done, sums (int64 [32]), pixels (points of the last linearisation), rms."""
    Rr = np.asarray(R_init, F).reshape(3, 3)
    tr = np.asarray(t_init, F).reshape(3)
    R, t = Rr.astype(D), tr.astype(D)
    status, done = TRACK_OK, 0
    sums = np.zeros(32, np.int64)
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    if len(P) == 0:
        status = TRACK_LOST  # an empty scan: no linearisation at all
    else:
        for _ in range(int(iterations)):
            sums = linearise(P, K, min_depth, max_depth, dist_max, R.astype(F), t.astype(F), Rr, tr, Mr, Mn, Mp)
            xi = solve(sums, max_depth, min_points)
            if xi is None:
                status = TRACK_LOST
                break
            R, t = update(R, t, xi)
            done += 1
    n = int(sums[28])
    rms = float(np.sqrt(D(sums[27]) / D(n)) / D(262144.0)) if n else 0.0
    return dict(R=R.astype(F), t=t.astype(F), status=status, iterations_done=done, sums=sums, pixels=n, rms=rms)


# ---- the analytic scenes as a model ------------------------------------------------------------------------------------

def analytic_model(scene, cam, R, t, max_range=np.inf):
    """(M_rho [rows, cols], M_n [rows, cols, 3], M_p [rows * cols, 3]) float32 of a mrhash_amd.synth scene seen from (R, t) by the
    spherical camera `cam` (synth.spherical_camera): the range along the directions of synth.spherical_range_image, the normal of
    the face hit (the nearest box plane, turned against the ray) and range times sensor direction.  A pixel whose 3 x 3
    neighbourhood spans two faces or leaves the image, or whose range exceeds max_range, is a miss (0)."""
    rows, cols = cam["rows"], cam["cols"]
    az = (np.arange(cols, dtype=D) - cam["cx"] - 0.5) / cam["fx"]
    el = (np.arange(rows, dtype=D) - cam["cy"] - 0.5) / cam["fy"]
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    d = np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], np.broadcast_to(se, (rows, cols))], -1)
    rng, pts = scene.cast_dirs(d, np.asarray(R, D), np.asarray(t, D))
    boxes = [scene.room] + list(scene.furniture)
    best = np.full(rng.shape, np.inf)
    face = np.zeros(rng.shape, np.int64)  # box * 6 + axis * 2 + side
    for bi, b in enumerate(boxes):
        for ax in range(3):
            for side, plane in enumerate((b.lo[ax], b.hi[ax])):
                dist = np.abs(pts[..., ax] - plane)
                better = dist < best
                best = np.where(better, dist, best)
                face = np.where(better, bi * 6 + ax * 2 + side, face)
    axis = (face % 6) // 2
    ray = pts - np.asarray(t, D)
    sign = -np.sign(np.take_along_axis(ray, axis[..., None], -1)[..., 0])  # against the ray: towards the sensor
    nrm = np.zeros(rng.shape + (3,), D)
    np.put_along_axis(nrm, axis[..., None], sign[..., None], -1)
    same = np.zeros(rng.shape, bool)
    same[1:-1, 1:-1] = True
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            same[1:-1, 1:-1] &= face[1 + dr:rows - 1 + dr, 1 + dc:cols - 1 + dc] == face[1:-1, 1:-1]
    same &= np.isfinite(rng) & (rng > 0) & (rng <= max_range)
    Mr = np.where(same, rng, 0.0).astype(F)
    Mp = (Mr[..., None] * d.astype(F)).astype(F).reshape(-1, 3)
    return Mr, np.where(same[..., None], nrm, 0.0).astype(F), Mp
