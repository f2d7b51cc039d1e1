"""LiDAR scan normals without the library: DESIGN.md D12 restated in numpy, and a textbook estimator to measure it against.

restate(points, ...)   D12 step by step — binary32 where D12 says binary32, int64 for the sums, float64 with a hand-written
                       cyclic Jacobi for the rest.  What the device must reproduce bit for bit.
textbook(points, ...)  the yardstick that is NOT the definition under test: the same cells, the same 27-cell neighbourhoods and
                       the same gate, but float64 moments of the unquantised points and numpy.linalg.eigh.

Both return a Result: normals float32 [n, 3], info (the five counts of mrh_normals_info) and, per occupied cell in ascending
key order, the packed key, the gate's decision and the cell normal, plus every point's cell index (-1: no cell).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

SWEEPS = 8
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))  # (p, q, the third index)
BIAS = 1 << 20
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


@dataclass
class Result:
    normals: np.ndarray      # float32 [n, 3]
    info: dict               # points, estimated, fallback, missing, cells
    keys: np.ndarray         # int64 [cells] ascending
    estimated: np.ndarray    # bool [cells]
    cell_normals: np.ndarray  # float64 [cells, 3] (unoriented)
    point_cell: np.ndarray   # int64 [n], -1 for a missing return or a point outside the key range


def _defaults(radius, min_points, min_spread, max_flatness):
    """0 = the default, as mrh_normals_params; floats pass through binary32 as they do through the C struct."""
    rho = np.float32(radius) if radius else np.float32(2.0) * np.float32(0.2)
    npts = int(min_points) if min_points else 5
    spread = float(np.float32(min_spread)) if min_spread else 0.0625
    flat = float(np.float32(max_flatness)) if max_flatness else 0.0625
    return rho, npts, spread, flat


def _ranges(p):
    """||p|| in binary32, left to right (steps 1 and 8)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        return np.sqrt(x * x + y * y + z * z)


def _cells(p, rho):
    """Step 2 for the returns p (binary32 [m, 3]): in-range flag, packed key (int64), local coordinate u (int64 [m, 3]),
    and the binary32 cell coordinate c."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = p / rho
        c = np.floor(s)
        ok = (np.abs(c) < np.float32(1048576.0)).all(axis=1)
        s, c = np.where(ok[:, None], s, np.float32(0)), np.where(ok[:, None], c, np.float32(0))
        u = np.minimum(1023, np.floor((s - c) * np.float32(1024.0)).astype(np.int64))
    ci = c.astype(np.int64) + BIAS
    key = ci[:, 0] | (ci[:, 1] << 21) | (ci[:, 2] << 42)
    return ok, key, u, c


def _group(key):
    """unique keys ascending, each point's cell index, and the (order, starts) that np.add.reduceat needs"""
    keys, inv = np.unique(key, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[order], np.arange(len(keys)))
    return keys, inv, order, starts


def _neighbours(keys):
    """for each of the 27 offsets d: (d, index of cell c + d in `keys` or -1)"""
    cx, cy, cz = keys & 0x1FFFFF, (keys >> 21) & 0x1FFFFF, (keys >> 42) & 0x1FFFFF
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                x, y, z = cx + dx, cy + dy, cz + dz
                ok = (x >= 0) & (x < (1 << 21)) & (y >= 0) & (y < (1 << 21)) & (z >= 0) & (z < (1 << 21))
                nk = x | (y << 21) | (z << 42)
                j = np.searchsorted(keys, nk)
                j = np.where(j < len(keys), j, 0)
                hit = ok & (keys[j] == nk)
                yield (dx, dy, dz), np.where(hit, j, -1)


def jacobi(A):
    """D12 step 6 on a stack of symmetric 3 x 3 float64 matrices: (eigenvalues ascending by (value, index), eigenvectors as
    columns in that order).  Only + - * / sqrt, in the order D12 writes them."""
    A = np.array(A, dtype=np.float64, copy=True).reshape(-1, 3, 3)
    V = np.broadcast_to(np.eye(3), A.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q, r in PAIRS:
                apq = A[:, p, q].copy()
                go = apq != 0.0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app, aqq = A[:, p, p] - t * apq, A[:, q, q] + t * apq
                arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                nrp, nrq = c * arp - s * arq, s * arp + c * arq
                A[:, p, p] = np.where(go, app, A[:, p, p])
                A[:, q, q] = np.where(go, aqq, A[:, q, q])
                A[:, p, q] = A[:, q, p] = np.where(go, 0.0, apq)
                A[:, r, p] = A[:, p, r] = np.where(go, nrp, arp)
                A[:, r, q] = A[:, q, r] = np.where(go, nrq, arq)
                for k in range(3):
                    vp, vq = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = np.where(go, c * vp - s * vq, vp)
                    V[:, k, q] = np.where(go, s * vp + c * vq, vq)
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
    order = np.argsort(lam, axis=1, kind="stable")  # stable: ties keep the lower index first
    lam = np.take_along_axis(lam, order, axis=1)
    V = np.take_along_axis(V, order[:, None, :], axis=2)
    return lam, V


def _assign(pts, rng, ret, point_cell, est, cell_normals):
    """Step 8 and the counts."""
    n = len(pts)
    out = np.zeros((n, 3), np.float32)
    has = point_cell >= 0
    is_est = np.zeros(n, bool)
    is_est[has] = est[point_cell[has]]
    fb = ret & ~is_est
    with np.errstate(all="ignore"):
        out[fb] = -(pts[fb] / rng[fb, None])
    cn = cell_normals.astype(np.float32)[point_cell[is_est]]
    p = pts[is_est]
    dot = cn[:, 0] * p[:, 0] + cn[:, 1] * p[:, 1] + cn[:, 2] * p[:, 2]
    out[is_est] = np.where((dot > 0)[:, None], -cn, cn)
    return out, int(is_est.sum()), int(fb.sum())


def restate(points, radius=0.0, min_points=0, min_spread=0.0, max_flatness=0.0) -> Result:
    rho, npts, spread, flat = _defaults(radius, min_points, min_spread, max_flatness)
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    rng = _ranges(pts)
    ret = (rng > 0) & np.isfinite(rng)                                   # step 1
    point_cell = np.full(n, -1, np.int64)
    idx = np.flatnonzero(ret)
    ok, key, u, _ = _cells(pts[idx], rho)                                # step 2
    idx, key, u = idx[ok], key[ok], u[ok]
    if len(idx) == 0:
        return Result(*_assign(pts, rng, ret, point_cell, np.zeros(0, bool), np.zeros((0, 3)))[:1],
                      dict(points=n, estimated=0, fallback=int(ret.sum()), missing=int((~ret).sum()), cells=0),
                      np.zeros(0, np.int64), np.zeros(0, bool), np.zeros((0, 3)), point_cell)
    keys, inv, order, starts = _group(key)
    point_cell[idx] = inv
    m = len(keys)
    # step 3: n, sum u, upper triangle of sum u u^T per cell, int64
    cnt = np.add.reduceat(np.ones(len(idx), np.int64)[order], starts)
    su = np.add.reduceat(u[order], starts, axis=0)
    uu = np.stack([u[:, i] * u[:, j] for i, j in UPPER], axis=1)
    sq = np.add.reduceat(uu[order], starts, axis=0)
    # step 4: the 27 cells, shifted exactly
    N = np.zeros(m, np.int64)
    S = np.zeros((m, 3), np.int64)
    Q = np.zeros((m, 6), np.int64)
    for d, j in _neighbours(keys):
        hit = j >= 0
        jj = np.where(hit, j, 0)
        c_ = np.where(hit, cnt[jj], 0)
        s_ = np.where(hit[:, None], su[jj], 0)
        q_ = np.where(hit[:, None], sq[jj], 0)
        a = 1024 * np.array(d, np.int64)
        N += c_
        S += s_ + c_[:, None] * a
        for k, (i, l) in enumerate(UPPER):
            Q[:, k] += q_[:, k] + s_[:, i] * a[l] + a[i] * s_[:, l] + c_ * (a[i] * a[l])
    assert int(np.abs(Q).max()) < 2 ** 53 and int(N.max()) < 2 ** 24
    # step 5: C_ij = (N Q_ij - S_i S_j) / (N N) in float64
    Nd, Sd, Qd = N.astype(np.float64), S.astype(np.float64), Q.astype(np.float64)
    NN = Nd * Nd
    A = np.zeros((m, 3, 3))
    for k, (i, l) in enumerate(UPPER):
        A[:, i, l] = A[:, l, i] = (Nd * Qd[:, k] - Sd[:, i] * Sd[:, l]) / NN
    lam, V = jacobi(A)                                                  # step 6
    thr = (1024.0 * spread) * (1024.0 * spread)
    est = (N >= npts) & (lam[:, 1] >= thr) & (lam[:, 0] <= flat * lam[:, 1])  # step 7
    cell_normals = V[:, :, 0]
    normals, n_est, n_fb = _assign(pts, rng, ret, point_cell, est, cell_normals)
    info = dict(points=n, estimated=n_est, fallback=n_fb, missing=int((~ret).sum()), cells=m)
    return Result(normals, info, keys, est, cell_normals, point_cell)


def textbook(points, radius=0.0, min_points=0, min_spread=0.0, max_flatness=0.0) -> Result:
    rho, npts, spread, flat = _defaults(radius, min_points, min_spread, max_flatness)
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    rng = _ranges(pts)
    ret = (rng > 0) & np.isfinite(rng)
    point_cell = np.full(n, -1, np.int64)
    idx = np.flatnonzero(ret)
    ok, key, _, c = _cells(pts[idx], rho)
    idx, key, c = idx[ok], key[ok], c[ok]
    keys, inv, order, starts = _group(key)
    point_cell[idx] = inv
    m = len(keys)
    # float64 moments of the unquantised points, in cell units relative to the point's own cell
    x = pts[idx].astype(np.float64) / float(rho) - c.astype(np.float64)
    cnt = np.add.reduceat(np.ones(len(idx))[order], starts)
    sx = np.add.reduceat(x[order], starts, axis=0)
    sxx = np.add.reduceat((x[:, :, None] * x[:, None, :])[order], starts, axis=0)
    N = np.zeros(m)
    S = np.zeros((m, 3))
    Q = np.zeros((m, 3, 3))
    for d, j in _neighbours(keys):
        hit = j >= 0
        jj = np.where(hit, j, 0)
        c_ = np.where(hit, cnt[jj], 0.0)
        s_ = np.where(hit[:, None], sx[jj], 0.0)
        q_ = np.where(hit[:, None, None], sxx[jj], 0.0)
        a = np.array(d, np.float64)
        N += c_
        S += s_ + c_[:, None] * a
        Q += q_ + s_[:, :, None] * a[None, None, :] + a[None, :, None] * s_[:, None, :] + c_[:, None, None] * np.outer(a, a)
    mean = S / N[:, None]
    C = Q / N[:, None, None] - mean[:, :, None] * mean[:, None, :]
    lam, V = np.linalg.eigh(C)
    est = (N >= npts) & (lam[:, 1] >= spread * spread) & (lam[:, 0] <= flat * lam[:, 1])
    cell_normals = V[:, :, 0]
    normals, n_est, n_fb = _assign(pts, rng, ret, point_cell, est, cell_normals)
    info = dict(points=n, estimated=n_est, fallback=n_fb, missing=int((~ret).sum()), cells=m)
    return Result(normals, info, keys, est, cell_normals, point_cell)
