"""A restatement of the free-space layer (include/mrhash_freespace.h) in numpy, on top of tests/independent.py
(world_to_voxel) and tests/esdf_ref.py (the observed / site rule of D16 on independent.Map): the layer as a boolean array, the
two carves, the state of a box of cells with its frontier, and the segments.  Every float is a numpy float32 and every
expression keeps the shape the definition gives it, so the results are compared bit for bit.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import esdf_ref as er
import independent as ind

F = np.float32
FREE, OBSERVED, OCCUPIED, FRONTIER = 1, 2, 4, 8
SEG_UNKNOWN, SEG_BAD = 1, 0x80
MAX_SAMPLES = 1 << 20


class Layer:
    """The box origin + [0, dims) of cells (x, y, z), 2^shift finest voxels per cell side; bits [nz, ny, nx] bool."""

    def __init__(self, origin, dims, shift):
        self.origin = np.array([int(x) for x in origin], np.int64)
        self.dims = np.array([int(x) for x in dims], np.int64)
        self.shift = int(shift)
        self.bits = np.zeros((int(dims[2]), int(dims[1]), int(dims[0])), bool)

    def copy(self):
        c = Layer(self.origin, self.dims, self.shift)
        c.bits = self.bits.copy()
        return c


def half_cell(vs, shift) -> np.float32:
    return F(0.5) * (F(vs) * F(1 << shift))


def bound(vs) -> np.float32:
    return F(1 << 20) * F(vs)


def z_of(z0, step, k):
    """z_k = z0 + k * step, each computed afresh (k a scalar or an integer array)."""
    return (F(z0) + (np.asarray(k).astype(F) * F(step)).astype(F)).astype(F)


def sample_count(z_min, z_max, step) -> int:
    """The k with z_k <= z_max for z_0 = z_min <= z_max, by bisection on k as the host counts them; 0: more than 2^20."""
    if z_of(z_min, step, MAX_SAMPLES) <= F(z_max):
        return 0
    lo, hi = 0, MAX_SAMPLES
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if z_of(z_min, step, mid) <= F(z_max):
            lo = mid
        else:
            hi = mid
    return hi


def cells_of(layer: Layer, vs, P):
    """Per point of P [n, 3] f32: (inside the bound, inside the layer's box, layer coordinates [n, 3])."""
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(P) < bound(vs), axis=1)
    Q = np.where(ok[:, None], P, F(0)).astype(F)  # nothing is converted to an integer unless it passed the bound
    v = np.asarray(ind.world_to_voxel(F(vs), Q)).astype(np.int64)
    c = (v >> layer.shift) - layer.origin
    inside = ok & np.all((c >= 0) & (c < layer.dims), axis=1)
    return ok, inside, c


def rotate(R, d):
    """d_w,a = (R[3a] d_x + R[3a+1] d_y) + R[3a+2] d_z for d [n, 3]."""
    R = np.asarray(R, F).reshape(3, 3)
    d = np.asarray(d, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((R[a, 0] * d[:, 0]).astype(F) + (R[a, 1] * d[:, 1]).astype(F)).astype(F) + (R[a, 2] * d[:, 2]).astype(F) for a in range(3)], -1).astype(F)


def _carve(layer: Layer, vs, t, d_w, end, active, min_depth, max_depth, step):
    t = np.asarray(t, F).reshape(3)
    n = sample_count(min_depth, max_depth, step)
    assert n > 0, "more than 2^20 samples"
    for k in range(n):
        z = z_of(min_depth, step, k)
        with np.errstate(invalid="ignore"):
            sel = active & (z <= end)
        if not sel.any():
            break  # z_k is monotone in k: no later sample of any ray is in
        with np.errstate(invalid="ignore", over="ignore"):
            P = (t[None, :] + (z * d_w[sel]).astype(F)).astype(F)
        _, inside, c = cells_of(layer, vs, P)
        c = c[inside]
        layer.bits[c[:, 2], c[:, 1], c[:, 0]] = True
    return layer


def carve_depth(layer: Layer, vs, depth, fx, fy, cx, cy, R, t, min_depth, max_depth, step=0.0, margin=0.0):
    depth = np.asarray(depth, F)
    rows, cols = depth.shape
    step = half_cell(vs, layer.shift) if step == 0 else F(step)
    ifx, ify = F(1) / F(fx), F(1) / F(fy)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    u = (ifx * ((c.astype(F) - F(cx)).astype(F) - F(0.5)).astype(F)).astype(F)
    v = (ify * ((r.astype(F) - F(cy)).astype(F) - F(0.5)).astype(F)).astype(F)
    d_w = rotate(R, np.stack([u.ravel(), v.ravel(), np.ones(rows * cols, F)], -1))
    D = depth.ravel()
    with np.errstate(invalid="ignore"):
        active = D > F(min_depth)  # NaN and D <= min_depth set nothing
        end = np.where(D > F(max_depth), F(max_depth), (D - F(margin)).astype(F)).astype(F)
    return _carve(layer, vs, t, d_w, end, active, min_depth, max_depth, step)


def carve_points(layer: Layer, vs, points, R, t, min_depth, max_depth, step=0.0, margin=0.0):
    p = np.asarray(points, F).reshape(-1, 3)
    if len(p) == 0:
        return layer
    step = half_cell(vs, layer.shift) if step == 0 else F(step)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rho = np.sqrt(((p[:, 0] * p[:, 0]).astype(F) + (p[:, 1] * p[:, 1]).astype(F)).astype(F) + (p[:, 2] * p[:, 2]).astype(F), dtype=F)
        active = np.isfinite(rho) & ~(rho <= F(min_depth))
        end = (np.fmin(rho, F(max_depth)).astype(F) - F(margin)).astype(F)
        ds = (p / rho[:, None]).astype(F)
    d_w = rotate(R, ds)
    return _carve(layer, vs, t, d_w, end, active, min_depth, max_depth, step)


def box(layer: Layer, m, origin, dims, min_weight=0, surface_band=0.0) -> np.ndarray:
    """The state bytes [nz, ny, nx] of the box origin + [0, dims) of cells on the map m (independent.Map / MultiMap, or None: empty)."""
    s = layer.shift
    origin = np.array([int(x) for x in origin], np.int64)
    dims = [int(x) for x in dims]
    nx, ny, nz = dims
    g = 1 << s
    if m is None:
        observed = site = np.zeros((nz, ny, nx), bool)
    else:
        st, _ = er.classify(m, tuple(origin * g), (nx * g, ny * g, nz * g), surface_band=surface_band, min_weight=min_weight)
        per_cell = lambda bit: ((st & bit) != 0).reshape(nz, g, ny, g, nx, g).any(axis=(1, 3, 5))
        observed, site = per_cell(er.OBSERVED), per_cell(er.SITE)
    c = er.cells(origin, dims) - layer.origin  # [nz, ny, nx, 3] layer coordinates
    inside = np.all((c >= 0) & (c < layer.dims), axis=-1)
    cc = np.where(inside[..., None], c, 0)
    free = inside & layer.bits[cc[..., 2], cc[..., 1], cc[..., 0]]
    state = (free * FREE + observed * OBSERVED + site * OCCUPIED).astype(np.uint8)
    known = free | observed
    open_ = np.zeros((nz, ny, nx), bool)
    for axis in range(3):
        n = known.shape[axis]
        if n < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        open_[tuple(lo)] |= ~known[tuple(hi)]
        open_[tuple(hi)] |= ~known[tuple(lo)]
    frontier = free & ~site & open_
    return (state | (frontier * FRONTIER).astype(np.uint8)).astype(np.uint8)


def segments(layer: Layer, vs, a, b, step=0.0):
    """(status u8 [n], counts u32 [n, 2] = (n_samples, n_free))."""
    a = np.asarray(a, F).reshape(-1, 3)
    b = np.asarray(b, F).reshape(-1, 3)
    step = half_cell(vs, layer.shift) if step == 0 else F(step)
    status, counts = np.zeros(len(a), np.uint8), np.zeros((len(a), 2), np.uint32)
    for i in range(len(a)):
        if not (np.all(np.isfinite(a[i])) and np.all(np.isfinite(b[i]))):
            status[i] = SEG_BAD
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            e = (b[i] - a[i]).astype(F)
            ln = np.sqrt(((e[0] * e[0]) + (e[1] * e[1])) + (e[2] * e[2]), dtype=F)
            d = np.zeros(3, F) if ln == 0 else (e / ln).astype(F)
        n = sample_count(0.0, ln, step)
        if n == 0:
            status[i] = SEG_BAD
            continue
        z = z_of(0.0, step, np.arange(n))
        with np.errstate(over="ignore", invalid="ignore"):
            P = (a[i][None, :] + (z[:, None] * d[None, :]).astype(F)).astype(F)
        ok, inside, c = cells_of(layer, vs, P)
        if not ok.all():
            status[i] = SEG_BAD
            continue
        c = c[inside]
        n_free = int(layer.bits[c[:, 2], c[:, 1], c[:, 0]].sum())
        counts[i] = (n, n_free)
        status[i] = 0 if n_free == n else SEG_UNKNOWN
    return status, counts


def line_of_sight_free(layer: Layer, vs, cast_status, a, b, step=0.0) -> np.ndarray:
    """Engine.line_of_sight_free from the status bytes of the ray cast (rays_ref or the engine's own): no HIT, no INSIDE, and
    every sample of the segment free."""
    seg, _ = segments(layer, vs, a, b, step)
    return ((np.asarray(cast_status) & 0x05) == 0) & (seg == 0)
