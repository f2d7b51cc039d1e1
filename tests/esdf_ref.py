"""A restatement of the distance-field definition (include/mrhash_esdf.h) in numpy, on top of
tests/independent.py: the cell lookup is getVoxel through independent.voxel_to_block and the blocks of independent.Map /
MultiMap (raycast_ref.make_map builds either from Engine.dump_blocks()); a coarse block is read with the writers' dense
index (lz // 2) * 16 + (ly // 2) * 4 + (lx // 2).

Two forms of the distance: `separable` (three windowed 1-D passes, used for the big comparisons) and `brute` (every cell
against every site, the definition read literally), which pins the separable form in tests/test_esdf.py.  Also the
hand-built maps the CPU and GPU tests share.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import independent as ind
from mrhash_amd import capi

F = np.float32
OBSERVED, SITE, INSIDE, FAR = 1, 2, 4, 8
FAR_D2 = 0xFFFFFFFF
_INF = np.int64(1) << 40


def cells(origin, dims) -> np.ndarray:
    """The voxel coordinates of the box, [nz, ny, nx, 3] (x fastest)."""
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    return np.stack([i + int(origin[0]), j + int(origin[1]), k + int(origin[2])], -1).astype(np.int64)


def lookup(m: ind.Map, origin, dims):
    """mrh_get_voxel for every cell of the box: (found bool, res int, sdf f32, weight int), each [nz, ny, nx]."""
    v = cells(origin, dims).reshape(-1, 3)
    b = ind.voxel_to_block(v, m.vs).astype(np.int64)
    n = len(v)
    found, res = np.zeros(n, bool), np.zeros(n, np.int64)
    sdf, weight = np.zeros(n, F), np.zeros(n, np.int64)
    ub, inv = np.unique(b, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    l = v % 8  # non-negative
    for u, key in enumerate(ub):
        if np.any(key < -(1 << 20)) or np.any(key >= (1 << 20)):
            continue  # outside the packed-key range: absent
        blk = m.blocks.get((int(key[0]), int(key[1]), int(key[2])))
        if blk is None:
            continue
        r, vox = blk if isinstance(blk, tuple) else (0, blk)
        sel = np.flatnonzero(inv == u)
        lx, ly, lz = l[sel, 0], l[sel, 1], l[sel, 2]
        li = lz * 64 + ly * 8 + lx if r == 0 else (lz // 2) * 16 + (ly // 2) * 4 + (lx // 2)
        found[sel], res[sel] = True, r
        sdf[sel], weight[sel] = vox["sdf"][li], vox["weight"][li]
    shape = (int(dims[2]), int(dims[1]), int(dims[0]))
    return found.reshape(shape), res.reshape(shape), sdf.reshape(shape), weight.reshape(shape)


def classify(m: ind.Map, origin, dims, surface_band=0.0, min_weight=0):
    """(state u8 with the observed / site / inside bits, sdf f32)."""
    found, res, sdf, weight = lookup(m, origin, dims)
    w_min = max(1, int(min_weight) if min_weight else m.min_w)
    observed = found & (weight >= w_min)
    band = np.full(sdf.shape, F(surface_band), F) if surface_band > 0 else (m.vs * (1 << res).astype(F)).astype(F)
    with np.errstate(invalid="ignore"):
        site = observed & (np.abs(sdf) <= band)
        inside = observed & (sdf < 0)
    state = (observed * OBSERVED + site * SITE + inside * INSIDE).astype(np.uint8)
    return state, sdf


def _pass(g: np.ndarray, axis: int, R: int) -> np.ndarray:
    """out[c] = min over |d| <= R of g[c + d] + d^2 along `axis` (cells outside the array do not exist)."""
    L = g.shape[axis]
    out = g.copy()
    for d in range(1, min(int(R), L - 1) + 1):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, L - d), slice(d, L)
        lo, hi = tuple(lo), tuple(hi)
        out[lo] = np.minimum(out[lo], g[hi] + d * d)
        out[hi] = np.minimum(out[hi], g[lo] + d * d)
    return out


def separable(site: np.ndarray, R: int) -> np.ndarray:
    """Squared distance to the nearest site by three 1-D passes (x, y, z), each reaching R cells: int64 [nz, ny, nx], >= 2^40 where
    no site lies within R on every axis.  Exact under the cap: a site within Euclidean distance R is within R on every axis."""
    g = np.where(site, np.int64(0), _INF)
    for axis in (2, 1, 0):
        g = _pass(g, axis, R)
    return g


def brute(site: np.ndarray) -> np.ndarray:
    """Squared distance to the nearest site of the box over all cell x site pairs (no reach): int64, >= 2^40 without a site."""
    shape = site.shape
    s = np.argwhere(site).astype(np.int64)  # (k, j, i)
    out = np.full(site.size, _INF, np.int64)
    if len(s) == 0:
        return out.reshape(shape)
    c = np.argwhere(np.ones(shape, bool)).astype(np.int64)
    step = max(1, (1 << 22) // len(s))
    for a in range(0, len(c), step):
        d = c[a:a + step, None, :] - s[None, :, :]
        out[a:a + step] = (d * d).sum(-1).min(1)
    return out.reshape(shape)


def finish(vs, state, sdf, d2, R):
    """(dist f32, state u8 with the far bit, d2 u32) from the squared distances."""
    R = int(R)
    far = d2 > R * R  # "no site" is >= 2^40
    site = (state & SITE) != 0
    assert not np.any(site & far) and not np.any(d2[site])
    mag = (F(vs) * np.sqrt(np.where(far, 0, d2).astype(F))).astype(F)
    mag = np.where(far, F(F(vs) * F(R)), mag).astype(F)
    dist = np.where((state & INSIDE) != 0, -mag, mag).astype(F)
    dist = np.where(site, sdf, dist).astype(F)
    return dist, (state | (far * FAR)).astype(np.uint8), np.where(far, FAR_D2, d2).astype(np.uint32)


def esdf(m: ind.Map, origin, dims, R, surface_band=0.0, min_weight=0, literal=False):
    """The definition: (dist f32, state u8, d2 u32), each [nz, ny, nx].  literal: the brute force instead of the separable form."""
    state, sdf = classify(m, origin, dims, surface_band, min_weight)
    site = (state & SITE) != 0
    return finish(m.vs, state, sdf, brute(site) if literal else separable(site, R), R)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- hand-built maps ------------------------------------------------------------------------------------------------------

SPHERE_PARAMS = dict(
    sdf_truncation=0.15, sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=0.05,
    n_frames_invalidate_voxels=0, voxel_extents_scale=1, marching_cubes_threshold=1.5, min_weight_threshold=1,
    sdf_var_threshold=0.0, vertices_merging_threshold=0.0, min_depth=0.01, max_depth=30.0,
)
SPHERE_C, SPHERE_R = np.array([0.02, -0.03, 0.04]), 0.35
SPHERE_BOX = ((-19, -13, -15), (41, 37, 29))


def _block_voxels(b):
    lin = np.arange(512)
    return np.stack([b[0] * 8 + lin % 8, b[1] * 8 + (lin // 8) % 8, b[2] * 8 + lin // 64], -1)


def sphere_sdf(vs, trunc, v):
    """clamp(|p - c| - r, +-trunc) at the voxels v [n, 3] (float64 arithmetic, rounded once), and the unclamped value."""
    d = np.linalg.norm(v.astype(np.float64) * float(vs) - SPHERE_C, axis=-1) - SPHERE_R
    return np.clip(d, -float(trunc), float(trunc)).astype(F), d


def sphere_blocks(params=SPHERE_PARAMS, weight=1) -> dict:
    """Every block that holds a voxel within the truncation of the sphere; all 512 voxels carry the clamped sdf and `weight`."""
    vs, trunc = params["virtual_voxel_size"], params["sdf_truncation"]
    reach = int(np.ceil((SPHERE_R + trunc + np.abs(SPHERE_C).max()) / vs / 8)) + 1
    out = {}
    for bx in range(-reach, reach + 1):
        for by in range(-reach, reach + 1):
            for bz in range(-reach, reach + 1):
                v = _block_voxels((bx, by, bz))
                sdf, d = sphere_sdf(vs, trunc, v)
                if np.any(np.abs(d) <= trunc):
                    blk = np.zeros(512, capi.VOXEL_DTYPE)
                    blk["sdf"], blk["weight"] = sdf, weight
                    blk["rgb"] = (v & 0xFF).astype(np.uint8)
                    out[(bx, by, bz)] = blk
    return out


def site_blocks(sites, params=SPHERE_PARAMS) -> dict:
    """Blocks whose voxels are observed free space (sdf = +trunc, weight 1) except the given voxels, which are sites (sdf 0)."""
    out = {}
    for s in sites:
        b = tuple(int(c) // 8 for c in s)  # floor
        blk = out.get(b)
        if blk is None:
            blk = out[b] = np.zeros(512, capi.VOXEL_DTYPE)
            blk["sdf"], blk["weight"] = F(params["sdf_truncation"]), 1
        blk["sdf"][(int(s[2]) % 8) * 64 + (int(s[1]) % 8) * 8 + int(s[0]) % 8] = 0
    return out


def to_import(blocks: dict):
    """(descs, voxels) for Engine.import_blocks from {(x, y, z): voxels[512]} or {(x, y, z): (resolution, voxels[512 or 64])}."""
    descs = np.zeros(len(blocks), capi.DESC_DTYPE)
    vox = np.zeros((len(blocks), 512), capi.VOXEL_DTYPE)
    for i, (k, v) in enumerate(sorted(blocks.items())):
        r, v = v if isinstance(v, tuple) else (0, v)
        descs[i] = (k[0], k[1], k[2], r)
        vox[i, :len(v)] = v
    return descs, vox
