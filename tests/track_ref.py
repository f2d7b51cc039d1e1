"""A restatement of depth-frame tracking (include/mrhash_track.h) in numpy: the per-pixel linearisation in
float32 without FMA, the 29 exact int64 sums, the binary64 Cholesky solve and the pose update.  The model images (depth and
world-frame normals of one render from the initial pose) are inputs: the GPU tests feed the library's own render, whose parity
is pinned by the raycast tests, the CPU tests feed images of the analytic scenes (analytic_model).

Test infrastructure only."""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64
TRACK_OK, TRACK_LOST = 0, 1
N_SUMS = 29  # 21 of the upper triangle of sum J J^T (row-major), 6 of sum J e, sum e^2, n; sums[29:32] stay 0
J_ONE = F(16384.0)    # fixed-point scale of the normal part of a row
E_ONE = F(262144.0)   # ... of the residual
J_LIMIT = F(32768.0)


def defaults(dist_max, iterations, min_pixels, sdf_truncation):
    """The parameter block with its zeros replaced (include/mrhash_track.h)."""
    if F(dist_max) == 0:
        dist_max = min(F(F(2.0) * F(sdf_truncation)), F(1.0))
    return F(dist_max), int(iterations) or 10, int(min_pixels) or 64


def angle_scale(max_depth) -> np.float32:
    """S_a = 16384 / L with L the smallest power of two >= 2 * max_depth."""
    two_d = F(F(2.0) * F(max_depth))
    L = F(1.0)
    while L < two_d:
        L = F(L * F(2.0))
    while F(L * F(0.5)) >= two_d:
        L = F(L * F(0.5))
    return F(J_ONE / L)


def _dir(K, r, c):
    """d_c of pixel (r, c): (ifx * ((c - cx) - 0.5), ify * ((r - cy) - 0.5), 1), float32."""
    fx, fy, cx, cy = (F(v) for v in K[:4])
    ifx, ify = F(F(1.0) / fx), F(F(1.0) / fy)
    x = (ifx * ((c.astype(F) - cx) - F(0.5))).astype(F)
    y = (ify * ((r.astype(F) - cy) - F(0.5))).astype(F)
    return x, y


def _rows3(M, x, y, z):
    """M v per row, (M_i0 x + M_i1 y) + M_i2 z, float32."""
    return [((M[i][0] * x + M[i][1] * y).astype(F) + (M[i][2] * z).astype(F)).astype(F) for i in range(3)]


def pixel_terms(depth, K, min_depth, max_depth, dist_max, R32, t32, Rr, tr, Md, Mn):
    """Steps 1-8 for every pixel of `depth`, raster order: (accepted [n] bool, J~ [n, 6] int64, e~ [n] int64).
    K = (fx, fy, cx, cy, rows, cols)."""
    rows, cols = int(K[4]), int(K[5])
    fx, fy, cx, cy = (F(v) for v in K[:4])
    Dm = np.ascontiguousarray(depth, F).reshape(rows, cols)
    Md = np.ascontiguousarray(Md, F).reshape(rows, cols)
    Mn = np.ascontiguousarray(Mn, F).reshape(rows, cols, 3)
    R32 = np.asarray(R32, F).reshape(3, 3)
    Rr = np.asarray(Rr, F).reshape(3, 3)
    t32, tr = np.asarray(t32, F).reshape(3), np.asarray(tr, F).reshape(3)
    r, c = np.mgrid[0:rows, 0:cols]
    r, c = r.ravel(), c.ravel()
    Dv = Dm.ravel()
    with np.errstate(all="ignore"):
        ok = (Dv > F(min_depth)) & (Dv <= F(max_depth))
        dx, dy = _dir(K, r, c)
        px, py, pz = (Dv * dx).astype(F), (Dv * dy).astype(F), Dv
        a = _rows3(R32, px, py, pz)
        pw = [(a[i] + t32[i]).astype(F) for i in range(3)]
        w = [(pw[i] - tr[i]).astype(F) for i in range(3)]
        q = [((Rr[0][i] * w[0] + Rr[1][i] * w[1]).astype(F) + (Rr[2][i] * w[2]).astype(F)).astype(F) for i in range(3)]
        ok &= q[2] > F(min_depth)
        u = (((fx * (q[0] / q[2]).astype(F)).astype(F) + cx).astype(F) + F(1.0)).astype(F)
        v = (((fy * (q[1] / q[2]).astype(F)).astype(F) + cy).astype(F) + F(1.0)).astype(F)
        ok &= (u >= 0) & (u < F(cols)) & (v >= 0) & (v < F(rows))
        c2 = np.where(ok, np.floor(u), 0).astype(np.int64)
        r2 = np.where(ok, np.floor(v), 0).astype(np.int64)
        m = Md[r2, c2]
        ok &= m != 0
        ex, ey = _dir(K, r2, c2)
        g = _rows3(Rr, ex, ey, F(1.0))
        V = [(tr[i] + (m * g[i]).astype(F)).astype(F) for i in range(3)]
        N = [Mn[r2, c2, i] for i in range(3)]
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
        Jt = np.stack([np.where(ok, np.rint(Js[i]), 0).astype(np.int64) for i in range(6)], -1)
        et = np.where(ok, np.rint(es), 0).astype(np.int64)
    return ok, Jt, et


def sums_of(ok, Jt, et, order=None) -> np.ndarray:
    """Step 9: the 32 int64 words (29 sums, three zeros) over the accepted pixels, visited in `order`."""
    idx = np.flatnonzero(ok) if order is None else np.asarray(order)[ok[np.asarray(order)]]
    J, e = Jt[idx], et[idx]
    out = np.zeros(32, np.int64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            out[k] = np.sum(J[:, i] * J[:, j], dtype=np.int64)
            k += 1
    for i in range(6):
        out[21 + i] = np.sum(J[:, i] * e, dtype=np.int64)
    out[27] = np.sum(e * e, dtype=np.int64)
    out[28] = len(idx)
    return out


def linearise(depth, K, min_depth, max_depth, dist_max, R32, t32, Rr, tr, Md, Mn, order=None) -> np.ndarray:
    return sums_of(*pixel_terms(depth, K, min_depth, max_depth, dist_max, R32, t32, Rr, tr, Md, Mn), order=order)


def solve(sums, max_depth, min_pixels):
    """xi = (omega, v) in binary64 from the 32 words, or None: lost."""
    n = int(sums[28])
    if n < int(min_pixels):
        return None
    Sa = D(angle_scale(max_depth))
    s = [Sa, Sa, Sa, D(16384.0), D(16384.0), D(16384.0)]
    H = np.zeros((6, 6), D)
    k = 0
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i, 6):
                H[i, j] = H[j, i] = D(sums[k]) / (s[i] * s[j])
                k += 1
        b = [D(sums[21 + i]) / (s[i] * D(262144.0)) for i in range(6)]
        L = np.zeros((6, 6), D)
        for j in range(6):
            d = H[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not (np.isfinite(d) and d > H[j, j] * D(2.0) ** -20):
                return None
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                acc = H[i, j]
                for k in range(j):
                    acc = acc - L[i, k] * L[j, k]
                L[i, j] = acc / L[j, j]
        y = np.zeros(6, D)
        for i in range(6):
            acc = b[i]
            for k in range(i):
                acc = acc - L[i, k] * y[k]
            y[i] = acc / L[i, i]
        x = np.zeros(6, D)
        for i in range(5, -1, -1):
            acc = y[i]
            for k in range(i + 1, 6):
                acc = acc - L[k, i] * x[k]
            x[i] = acc / L[i, i]
    return x


def update(R, t, xi):
    """(R, t) <- (dR R, t + v), binary64; dR from the unit quaternion (omega / 2, 1) / |.| by Eigen's formula."""
    R = np.asarray(R, D).reshape(3, 3)
    t = np.asarray(t, D).reshape(3)
    hx, hy, hz = D(xi[0]) / D(2.0), D(xi[1]) / D(2.0), D(xi[2]) / D(2.0)
    nu = np.sqrt(((hx * hx + hy * hy) + hz * hz) + D(1.0))
    x, y, z, w = hx / nu, hy / nu, hz / nu, D(1.0) / nu
    tx, ty, tz = D(2.0) * x, D(2.0) * y, D(2.0) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = D(1.0)
    dR = [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]
    Rn = np.zeros((3, 3), D)
    for i in range(3):
        for j in range(3):
            Rn[i, j] = (dR[i][0] * R[0, j] + dR[i][1] * R[1, j]) + dR[i][2] * R[2, j]
    return Rn, np.array([t[0] + D(xi[3]), t[1] + D(xi[4]), t[2] + D(xi[5])], D)


def track(depth, K, min_depth, max_depth, dist_max, iterations, min_pixels, R_init, t_init, Md, Mn) -> dict:
    """The loop.  dist_max, iterations and min_pixels are taken as given (see defaults()).  Returns R, t (float32), status,
    iterations_done, sums (int64 [32]), pixels, rms."""
    Rr = np.asarray(R_init, F).reshape(3, 3)
    tr = np.asarray(t_init, F).reshape(3)
    R, t = Rr.astype(D), tr.astype(D)
    status, done = TRACK_OK, 0
    sums = np.zeros(32, np.int64)
    for _ in range(int(iterations)):
        sums = linearise(depth, K, min_depth, max_depth, dist_max, R.astype(F), t.astype(F), Rr, tr, Md, Mn)
        xi = solve(sums, max_depth, min_pixels)
        if xi is None:
            status = TRACK_LOST
            break
        R, t = update(R, t, xi)
        done += 1
    n = int(sums[28])
    rms = float(np.sqrt(D(sums[27]) / D(n)) / D(262144.0)) if n else 0.0
    return dict(R=R.astype(F), t=t.astype(F), status=status, iterations_done=done, sums=sums, pixels=n, rms=rms)


# ---- the analytic scenes as a model ------------------------------------------------------------------------------------

def analytic_model(scene, K, R, t):
    """(M_d [rows, cols] float32, M_n [rows, cols, 3] float32) of mrhash_amd.synth scenes seen from (R, t): depth from
    Scene.cast, the inward normal of the face hit (the nearest box plane; it faces the camera), and a miss (0) at the pixels
    whose 3 x 3 neighbourhood spans two faces or leaves the image."""
    depth, pts = scene.cast(K, np.asarray(R, D), np.asarray(t, D), 0.5)
    boxes = [scene.room] + list(scene.furniture)
    best = np.full(depth.shape, np.inf)
    face = np.zeros(depth.shape, np.int64)  # box * 6 + axis * 2 + side
    for bi, b in enumerate(boxes):
        for ax in range(3):
            for side, plane in enumerate((b.lo[ax], b.hi[ax])):
                dist = np.abs(pts[..., ax] - plane)
                better = dist < best
                best = np.where(better, dist, best)
                face = np.where(better, bi * 6 + ax * 2 + side, face)
    axis = (face % 6) // 2
    ray = pts - np.asarray(t, D)
    sign = -np.sign(np.take_along_axis(ray, axis[..., None], -1)[..., 0])  # against the ray: towards the camera
    nrm = np.zeros(depth.shape + (3,), D)
    np.put_along_axis(nrm, axis[..., None], sign[..., None], -1)
    same = np.zeros(depth.shape, bool)
    same[1:-1, 1:-1] = True
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            same[1:-1, 1:-1] &= face[1 + dr:face.shape[0] - 1 + dr, 1 + dc:face.shape[1] - 1 + dc] == face[1:-1, 1:-1]
    same &= np.isfinite(depth) & (depth > 0)
    return np.where(same, depth, 0.0).astype(F), np.where(same[..., None], nrm, 0.0).astype(F)


def rot_to_quat(R) -> np.ndarray:
    """(x, y, z, w), binary64, normalised (test helper; not part of D14)."""
    R = np.asarray(R, D).reshape(3, 3)
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    q = np.array([np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1]), w], D)
    return q / np.linalg.norm(q)


def pose_errors(R_est, t_est, R_true, t_true):
    """(translation error in metres, rotation error in degrees as 2 asin |vec(q_est * q_true^-1)|)."""
    qe, qt = rot_to_quat(R_est), rot_to_quat(R_true)
    xe, we = qe[:3], qe[3]
    xt, wt = -qt[:3], qt[3]  # the inverse of a unit quaternion
    vec = we * xt + wt * xe + np.cross(xe, xt)
    ang = 2.0 * np.arcsin(min(1.0, float(np.linalg.norm(vec))))
    return float(np.linalg.norm(np.asarray(t_est, D) - np.asarray(t_true, D))), float(np.rad2deg(ang))
