"""A restatement of the raycast definition (include/mrhash_raycast.h) on top of tests/independent.py: the ray
and the back-projection of independent.Camera, the block test through independent.world_to_voxel / voxel_to_block, and
trilinearInterpolation, getVoxel and getVoxelSize through independent.Map / MultiMap (numpy float32 scalars, no FMA).

Rule 3's block test is vectorised over every sample of every ray; the scalar trilinear is called only where the sample's
block is in the map.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import independent as ind

F = np.float32
MAX_SAMPLES = 1 << 20
BISECTIONS = 3  # n_iteration_bisection (params.h:26)


def blocks_from_dump(d, v, multi: bool) -> dict:
    """Engine.dump_blocks() -> the blocks dict of independent.Map (as_dict) or MultiMap ((resolution, voxels[:512 or 64]))."""
    if not multi:
        return {(int(d["x"][i]), int(d["y"][i]), int(d["z"][i])): v[i].copy() for i in range(len(d))}
    return {(int(d["x"][i]), int(d["y"][i]), int(d["z"][i])): (int(d["resolution"][i]), v[i][: 512 if d["resolution"][i] == 0 else 64].copy())
            for i in range(len(d))}


def make_map(params: dict, d, v):
    multi = float(params.get("sdf_var_threshold", 0.0)) > 0.0
    blocks = blocks_from_dump(d, v, multi)
    return ind.MultiMap(params, blocks) if multi else ind.Map(params, blocks)


def sample_depths(min_depth, max_depth, step) -> np.ndarray:
    """z_k = min_depth + k * step (float32, each computed afresh) for k = 0, 1, ... while z_k <= max_depth."""
    z = (F(min_depth) + np.arange(MAX_SAMPLES + 1, dtype=np.uint32).astype(F) * F(step)).astype(F)
    n = int(np.count_nonzero(z <= F(max_depth)))
    if n > MAX_SAMPLES:
        raise ValueError("more than 2^20 samples per ray")
    return z[:n].copy()


class Raycaster:
    """One render: pinhole intrinsics, camera-to-world pose (R row-major, t), depth range and sample spacing."""

    def __init__(self, m: ind.Map, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step):
        self.m = m
        self.cam = ind.Camera(fx, fy, cx, cy, rows, cols, min_depth, max_depth)
        self.cam.set_pose(R, t)
        self.z = sample_depths(min_depth, max_depth, step)
        self.keys = np.array(sorted(self._key(np.array(k, np.int64)) for k in m.blocks), np.int64) if m.blocks else np.zeros(0, np.int64)
        self.multi = isinstance(m, ind.MultiMap)

    @staticmethod
    def _key(b):
        b = np.asarray(b, np.int64) + (1 << 20)
        return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]

    def directions(self, rows, cols) -> np.ndarray:
        """d_w = R d_c with d_c = inverse_projection(r, c, 1) (camera.cuh:88); every row summed left to right."""
        rows, cols = np.asarray(rows), np.asarray(cols)
        dc = self.cam.inverse_projection(rows, cols, np.ones(rows.shape, F))
        R = self.cam.R
        return np.stack([R[i, 0] * dc[..., 0] + R[i, 1] * dc[..., 1] + R[i, 2] * dc[..., 2] for i in range(3)], -1).astype(F)

    def point(self, d, z):  # P(z) = t + z d, per component
        t = self.cam.t
        return (F(t[0] + F(F(z) * d[0])), F(t[1] + F(F(z) * d[1])), F(t[2] + F(F(z) * d[2])))

    def sample_blocks(self, d) -> np.ndarray:
        """The block of every sample of the rays d [n, 3]: [n, K, 3] int64."""
        P = (self.cam.t[None, None, :] + self.z[None, :, None] * d[:, None, :]).astype(F)
        b = ind.voxel_to_block(ind.world_to_voxel(self.m.vs, P.reshape(-1, 3)), self.m.vs).astype(np.int64)
        return b.reshape(len(d), len(self.z), 3)

    def present(self, d) -> np.ndarray:
        """Rule 3's block test for every sample of the rays d [n, 3]: [n, K] bool."""
        b = self.sample_blocks(d)
        inside = np.all((b >= -(1 << 20)) & (b < (1 << 20)), axis=-1)
        return inside & np.isin(self._key(b), self.keys)

    def refine(self, d, a, ad, b, bd):  # findIntersectionBisection (vds.cu:348-383); None: the crossing is rejected
        c = a
        for _ in range(BISECTIONS):
            c = F(a + F(F(ad / F(ad - bd)) * F(b - a)))
            ok, cd = self.m.trilinear(self.point(d, c))
            if not ok:
                return None
            if F(ad * cd) > 0:
                a, ad = c, cd
            else:
                b, bd = c, cd
        return c

    def gradient(self, P):  # the central differences over one voxel of the local size; None: a trilinear of the stencil failed
        h = self.m.voxel_size_at(P) if self.multi else self.m.vs
        g = np.zeros(3, F)
        for a in range(3):
            pp, pm = list(P), list(P)
            pp[a], pm[a] = F(P[a] + h), F(P[a] - h)
            okp, dp = self.m.trilinear(pp)
            okm, dm = self.m.trilinear(pm)
            if not (okp and okm):
                return None
            g[a] = F(dp - dm)
        return g

    def normal(self, P):
        g = self.gradient(P)
        if g is None or F(F(g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) == 0:
            return np.zeros(3, F)
        return ind._normalize(g)

    def sample(self, k, ok, D, prev_valid, prev_d, gap):
        """Called by cast for every sample k in a present block, before rule 4 looks at it: its trilinear (ok, D), the state it
        meets, and whether absent samples lie between it and the previous present one.  Nothing here; tests/ray_fields.py counts."""

    def cast(self, d, present_row):
        """(depth, normal[3], rgb[3]) of one ray."""
        prev_valid, prev_d, prev_z, last = False, F(0), F(0), -2
        for k in np.flatnonzero(present_row):
            gap = k != last + 1
            if gap:
                prev_valid = False
            last = k
            z = self.z[k]
            ok, D = self.m.trilinear(self.point(d, z))
            self.sample(k, ok, D, prev_valid, prev_d, gap)
            if ok and prev_valid and prev_d > 0 and D <= 0:
                c = self.refine(d, prev_z, prev_d, z, D)
                if c is not None:
                    P = self.point(d, c)
                    return F(c), self.normal(P), np.array(self.m.get_voxel(P)[2], np.uint8)
            prev_valid, prev_d, prev_z = ok, D, z
        return F(0), np.zeros(3, F), np.zeros(3, np.uint8)

    def render(self, rows, cols):
        """The pixels (rows[i], cols[i]): depth [n], normals [n, 3], rgb [n, 3]."""
        rows, cols = np.asarray(rows).ravel(), np.asarray(cols).ravel()
        d = self.directions(rows, cols)
        depth = np.zeros(len(rows), F)
        nrm = np.zeros((len(rows), 3), F)
        rgb = np.zeros((len(rows), 3), np.uint8)
        chunk = 256
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for i0 in range(0, len(rows), chunk):
                pres = self.present(d[i0:i0 + chunk])
                for j in range(len(pres)):
                    depth[i0 + j], nrm[i0 + j], rgb[i0 + j] = self.cast(d[i0 + j], pres[j])
        return depth, nrm, rgb
