"""A restatement of the point query (include/mrhash_query.h) on top of tests/independent.py: the world -> voxel
-> block conversions of independent.world_to_voxel / voxel_to_block, and trilinearInterpolation, getVoxel and getVoxelSize
through independent.Map / MultiMap (numpy float32 scalars, no FMA).  The pose, the refusal rule and the SMOOTH field's lattice
are vectorised; the per-point evaluations are scalar.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import independent as ind

F = np.float32
FIELD_MAP, FIELD_SMOOTH = 0, 1
BLOCK, DIST, GRAD, COARSE, REFUSED = 1, 2, 4, 8, 0x80


def bound(vs) -> np.float32:
    """(float) (1 << 20) * vs"""
    return F(F(1 << 20) * F(vs))


def transform(R, t, xyz) -> np.ndarray:
    """P_a = ((R[3a] x + R[3a+1] y) + R[3a+2] z) + t[a], every operation rounded to binary32."""
    R, t, p = np.asarray(R, F).reshape(9), np.asarray(t, F).reshape(3), np.asarray(xyz, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((R[3 * a] * p[:, 0] + R[3 * a + 1] * p[:, 1]) + R[3 * a + 2] * p[:, 2]) + t[a] for a in range(3)], -1).astype(F)


def world_points(vs, xyz, R=None, t=None):
    """(P [n, 3], refused [n]): the positions that are queried and the refusal rule."""
    p = np.asarray(xyz, F).reshape(-1, 3)
    if R is None:
        P, missing = p, np.zeros(len(p), bool)
    else:
        P, missing = transform(R, t, p), np.all(p == 0, axis=-1)  # +-0 in every component: a missing return
    with np.errstate(invalid="ignore"):
        inside = np.all(np.abs(P) < bound(vs), axis=-1)  # NaN and +-Inf fail the comparison
    return P, missing | ~inside


def _voxel(m: ind.Map, p):
    """getVoxel(float3) with what the query reports of it: (sdf, weight, (r, g, b), found)."""
    v = m._w2v(p)
    b = tuple(int(c) for c in ind.voxel_to_block(np.array(v, ind.I), m.vs))
    e = m.blocks.get(b)
    if e is None:
        return F(0), 0, (0, 0, 0), False
    res, vox = e if isinstance(m, ind.MultiMap) else (0, e)
    lx, ly, lz = v[0] % 8, v[1] % 8, v[2] % 8
    c = vox[lz * 64 + ly * 8 + lx if res == 0 else (lz // 2) * 16 + (ly // 2) * 4 + (lx // 2)]
    return F(c["sdf"]), int(c["weight"]), tuple(int(x) for x in c["rgb"]), True


def _size(m: ind.Map, p):
    return m.voxel_size_at(p) if isinstance(m, ind.MultiMap) else m.vs


def _lerp(a, b, w):
    return F(a + F(w * F(b - a)))


def _map_field(m, P, h, gradient):
    ok, d = m.trilinear(P)
    if not ok:
        return F(0), np.zeros(3, F), 0
    g, st = np.zeros(3, F), DIST
    if gradient:
        for a in range(3):
            pp, pm = list(P), list(P)
            pp[a], pm[a] = F(P[a] + h), F(P[a] - h)
            okp, dp = m.trilinear(pp)
            okm, dm = m.trilinear(pm) if okp else (False, F(0))
            if not (okp and okm):
                return d, np.zeros(3, F), st
            g[a] = F(F(dp - dm) / F(h + h))
        st |= GRAD
    return d, g, st


def _smooth_field(m, P, h, gradient):
    u = [F(P[a] / h) for a in range(3)]
    f = [F(np.floor(u[a])) for a in range(3)]
    w = [F(u[a] - f[a]) for a in range(3)]
    s = np.zeros((2, 2, 2), F)  # [i, j, k]
    for k in range(2):
        for j in range(2):
            for i in range(2):
                pos = (F(F(f[0] + F(i)) * h), F(F(f[1] + F(j)) * h), F(F(f[2] + F(k)) * h))
                sdf, weight, _, found = _voxel(m, pos)
                if not found or weight == 0:
                    return F(0), np.zeros(3, F), 0
                s[i, j, k] = sdf
    c = [[_lerp(s[0, j, k], s[1, j, k], w[0]) for k in range(2)] for j in range(2)]  # [j][k]
    ck = [_lerp(c[0][k], c[1][k], w[1]) for k in range(2)]
    d = _lerp(ck[0], ck[1], w[2])
    g, st = np.zeros(3, F), DIST
    if gradient:
        e = [_lerp(F(s[1, 0, k] - s[0, 0, k]), F(s[1, 1, k] - s[0, 1, k]), w[1]) for k in range(2)]
        g[0] = F(_lerp(e[0], e[1], w[2]) / h)
        g[1] = F(_lerp(F(c[1][0] - c[0][0]), F(c[1][1] - c[0][1]), w[2]) / h)
        g[2] = F(F(ck[1] - ck[0]) / h)
        st |= GRAD
    return d, g, st


def query(m: ind.Map, xyz, R=None, t=None, smooth=False, gradient=True, colour=True):
    """(dist [n] f32, grad [n, 3] f32 or None, rgbw [n, 4] u8 or None, state [n] u8) as mrh_query_points defines them."""
    P, refused = world_points(m.vs, xyz, R, t)
    n = len(P)
    dist, grad, rgbw, state = np.zeros(n, F), np.zeros((n, 3), F), np.zeros((n, 4), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        if refused[i]:
            state[i] = REFUSED
            continue
        p = (F(P[i, 0]), F(P[i, 1]), F(P[i, 2]))
        h = _size(m, p)
        _, weight, rgb, found = _voxel(m, p)
        st = (BLOCK if found else 0) | (COARSE if h > m.vs else 0)
        if found:
            rgbw[i] = (*rgb, weight)
        d, g, bits = (_smooth_field if smooth else _map_field)(m, p, h, gradient)
        dist[i], grad[i], state[i] = d, g, st | bits
    return dist, grad if gradient else None, rgbw if colour else None, state


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ref_map(params: dict, blocks: dict):
    """independent.Map / MultiMap of hand-built blocks ({b: voxels[512]} with coarse blocks as (1, voxels[64]), as tests/mc_fields.py
    builds them)."""
    if float(params.get("sdf_var_threshold", 0.0)) > 0.0:
        return ind.MultiMap(params, {b: (v if isinstance(v, tuple) else (0, v)) for b, v in blocks.items()})
    assert not any(isinstance(v, tuple) for v in blocks.values())
    return ind.Map(params, blocks)


# ---- the point sets of the field tests (tests/test_query.py asserts the coverage on the restatement, tests/test_query_gpu.py compares) ----

CLUSTER_POINTS = 1500
LADDER_POINTS = 600


def cluster_points(vs, seed=3) -> np.ndarray:
    """1 500 world points for a 4^3-block cluster at the origin (voxels 0 .. 31, mc_fields.sign_field): lattice specials — voxel
    centres, half-voxel ties, block faces and corners, points whose P +- h leave the cluster — and uniform points over the cluster
    plus a rim of 1.5 voxels.  Positions are drawn in voxels (float64) and scaled by vs once."""
    rng = np.random.default_rng(seed)
    lo, hi = -0.5 - 1.5, 31.5 + 1.5
    special = [rng.integers(0, 32, (40, 3)).astype(np.float64),                                    # voxel centres
               rng.integers(0, 31, (40, 3)) + 0.5,                                                 # half-voxel ties on every axis
               rng.integers(0, 31, (30, 3)) + np.where(rng.random((30, 3)) < 0.5, 0.5, 0.0)]       # ... and on some
    faces = rng.uniform(0.0, 31.0, (40, 3))
    faces[np.arange(40), rng.integers(0, 3, 40)] = rng.choice([7.5, 8.0, 15.5, 16.0, 23.5, 24.0, 7.0], 40)  # on, and next to, a block face
    special.append(faces)
    special.append(rng.choice([7.5, 8.0, 15.5, 16.0, 23.5], (20, 3)))                              # block corners and edges
    leave = rng.uniform(2.0, 29.0, (50, 3))
    leave[np.arange(50), rng.integers(0, 3, 50)] = rng.choice([-1.5, -0.5, -0.4, 0.4, 0.5, 1.4, 1.6, 29.4, 30.4, 30.5, 30.6, 31.5, 31.6, 32.5], 50)
    special.append(leave)                                                                          # P +- h (or its stencil) leaves the cluster
    special = np.concatenate(special)
    uniform = rng.uniform(lo, hi, (CLUSTER_POINTS - len(special), 3))
    return (np.concatenate([special, uniform]) * float(vs)).astype(F)


def ladder_points(blocks: dict, vs, seed=4) -> np.ndarray:
    """600 world points within a voxel of randomly chosen blocks of mc_fields.ladder: uniform over the block's cells and a rim of
    one voxel."""
    rng = np.random.default_rng(seed)
    keys = np.array(sorted(blocks), np.int64)
    b = keys[rng.integers(0, len(keys), LADDER_POINTS)]
    q = b * 8.0 - 0.5 + rng.uniform(-1.0, 9.0, (LADDER_POINTS, 3))
    return (q * float(vs)).astype(F)


def coverage(state) -> dict:
    state = np.asarray(state)
    return {name: float(np.mean((state & bit) != 0)) for name, bit in (("block", BLOCK), ("dist", DIST), ("grad", GRAD), ("coarse", COARSE), ("refused", REFUSED))}


def dual_centre(vs, P):
    """The centre of the eight-cell cube the MAP field averages on a single-resolution map: (round(P / vs - 1/2) + 1/2) vs, in
    float64 (for points whose P / vs - 1/2 is no rounding tie)."""
    q = np.asarray(P, np.float64) / float(vs)
    return (np.round(q - 0.5) + 0.5) * float(vs)
