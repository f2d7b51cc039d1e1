"""The mixed batch of the ray-query tests (tests/test_rays.py asserts what it reaches on the restatement, tests/test_rays_gpu.py
casts it on the kernel): one variance-adaptive map of uniform slabs, so that a ray's fate can be read off the block table, and rays
of every kind D21 tells apart.

The map (rays_blocks), voxel size 0.05 m, blocks of 0.4 m:
  slabs    ray_fields' inside_out: x blocks [1, 3) -, [3, 6) +, [6, 8) -, [8, 10) +, [10, 12) -, y and z blocks -1 .. 1, block
           (6, 0, 0) removed
  coarse   x blocks [1, 3) + and [3, 5) -, y blocks 5 .. 7, z blocks -1 .. 1, every block coarse (h = 2 vs)
  rung     mc_fields' ladder rung at 2^12 blocks (1638 m out): its first four blocks along x +, the other three -

Every family below is one template ray and VARIANTS copies of it, shifted by fractions of a voxel in y and z and tilted slightly
(directions are NOT unit vectors: D21 takes them as given).  The families are interleaved, so every prefix of the batch mixes
them, and five bad rays stand at fixed places."""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import mc_fields as mf
import ray_fields as rf

F = np.float32
VS, BLOCK, T = rf.VS, rf.BLOCK, rf.T
PARAMS = rf.VAR_PARAMS
VARIANTS = 24
MIN_RANGE, MAX_RANGE, STEP = 0.0, 5.0, 0.0   # step 0: the default, half the truncation = 1.5 voxels
RUNG_K = 12

Batch = namedtuple("Batch", "origins directions tmax family min_range max_range step")  # family: the template's name per ray


def _rung():
    (k, side, coords), = [r for r in mf.ladder_rungs() if r[0] == RUNG_K and r[1] == 1]
    c = np.array(coords)
    return coords, c.min(0), c.max(0)


@lru_cache(maxsize=None)
def rays_blocks():
    blocks = {}
    for x0, x1, s in rf.INSIDE_OUT_SLABS:
        for b in mf.cluster((x0, -1, -1), (x1 - x0, 3, 3)):
            blocks[b] = mf._uniform_block(b, F(s) * T)
    del blocks[rf.REMOVED]
    for x0, x1, s in ((1, 3, 0.5), (3, 5, -0.25)):
        for b in mf.cluster((x0, 5, -1), (x1 - x0, 3, 3)):
            blocks[b] = (1, mf._uniform_block(b, F(s) * T, coarse=True))
    coords, lo, hi = _rung()
    for b in coords:
        blocks[b] = mf._uniform_block(b, F(0.5 if b[0] < lo[0] + 4 else -0.25) * T)
    return blocks


def _templates():
    """[(name, origin (voxels), direction, tmax)]; the origin's y = z = 10.25 voxels lies well inside block 1, x as stated."""
    inf = np.inf
    coords, lo, hi = _rung()
    ry, rz = (lo[1] + 1) * 8 + 3.3, (lo[2] + 1) * 8 + 3.3   # the rung's middle block in y and z
    return [
        ("free", (24.25, 10.25, 10.25), (1, 0, 0), 1.0),                  # inside the + slab, ends there: status 0
        ("hit", (30.25, 10.25, 10.25), (-1, 0, 0), inf),                  # back out of the + slab into the - slab at x block 3
        ("unknown", (30.25, 10.25, 10.25), (0, 1, 0), 1.5),               # sideways out of the + slab: first_unknown at k > 0
        ("inside", (10.25, 10.25, 10.25), (1, 0, 0), 0.5),                # inside the first - slab, ends there
        ("hit_unknown", (54.25, 2.25, 2.25), (-1, 0, 0), inf),            # from the removed block back through + into -
        ("hit_inside", (10.25, 10.25, 10.25), (1, 0, 0), inf),            # from the - slab through + to the front face at x block 6
        ("unknown_inside", (0.25, 10.25, 10.25), (1, 0, 0), 0.9),         # from the absent block 0 into the - slab: first_unknown at k = 0
        ("all_three", (0.25, 10.25, 10.25), (1, 0, 0), inf),              # ... and on through + to the front face
        ("ends_in_gap", (30.25, 2.25, 2.25), (1, 0, 0), 1.1),             # from + into the removed block (6, 0, 0) and ends inside it
        ("through_gap", (30.25, 2.25, 2.25), (1, 0, 0), inf),             # ... or goes on: the bracket is lost, hit at x block 10
        ("cut_short", (10.25, 10.25, 10.25), (1, 0, 0), 1.2),             # hit_inside's ray, ended before its hit
        ("rim", (30.25, -0.4, 2.25), (1, 0, 0), inf),                     # through the removed block with y in its quarter-voxel rim, d_y = 0
        ("coarse", (12.5, 48.5, 4.5), (1, 0, 0), inf),                    # in the coarse + slab, hits the coarse - slab
        ("rung", (lo[0] * 8 + 3.3, ry, rz), (1, 0, 0), inf),              # inside the rung's first block, hits its - part
        ("rung_outside", ((lo[0] - 3) * 8 + 3.3, ry, rz), (1, 0, 0), 4.0),  # three absent blocks in front of the rung
        ("oblique", (0.25, 2.25, -6.75), (1.0, 0.11, 0.23), inf),         # through everything at an angle, |d| > 1
    ]


NAMES = tuple(t[0] for t in _templates())  # ray j * len(NAMES) + NAMES.index(name) is variant j of the template, unless BAD took its place


def pairs(b, first, second):
    """[(i, j)]: the rays of templates `first` and `second` of one variant, where both are still in the batch."""
    n, a, c = len(NAMES), NAMES.index(first), NAMES.index(second)
    return [(v * n + a, v * n + c) for v in range(VARIANTS) if b.family[v * n + a] == first and b.family[v * n + c] == second]


BAD = (("bad_origin_nan", 5), ("bad_direction_inf", 20), ("bad_direction_zero", 41), ("bad_origin_bound", 70), ("bad_tmax_nan", 130))
ZERO_SAMPLES_AT = 99  # one ray with tmax < min_range: no sample


@lru_cache(maxsize=None)
def mixed_batch() -> Batch:
    tpl = _templates()
    o, d, tm, fam = [], [], [], []
    for j in range(VARIANTS):
        dy, dz = (j % 4) * 0.35, (j // 4) * 0.45          # voxels: stays inside the template's block
        tilt = np.array([0.0, 0.004 * (j % 3), 0.006 * (j % 5)])
        for name, ov, dv, t in tpl:
            oo = np.array(ov, np.float64)
            if name != "rim":
                oo[1] += dy
            oo[2] += dz
            o.append(oo * VS)
            d.append(np.array(dv, np.float64) * (1.0 + 0.05 * (j % 4)) + (tilt if name not in ("rim", "unknown") else 0.0))
            tm.append(t / (1.0 + 0.05 * (j % 4)) if np.isfinite(t) else t)  # the end is a multiple of d: the same place in metres
            fam.append(name)
    o, d, tm = np.array(o, F), np.array(d, F), np.array(tm, F)
    bound = F(F(1 << 20) * F(VS))
    for name, i in BAD:
        fam[i] = name
        if name == "bad_origin_nan":
            o[i, 1] = np.nan
        elif name == "bad_direction_inf":
            d[i, 2] = -np.inf
        elif name == "bad_direction_zero":
            d[i] = (0.0, -0.0, 0.0)
        elif name == "bad_origin_bound":
            o[i, 0] = bound   # |o| < bound fails at the bound itself
        else:
            tm[i] = np.nan
    fam[ZERO_SAMPLES_AT] = "zero_samples"
    tm[ZERO_SAMPLES_AT] = F(-0.5)
    return Batch(o, d, tm, tuple(fam), MIN_RANGE, MAX_RANGE, STEP)


POSE_R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)   # a quarter turn about z: every product is exact
POSE_T = np.array([0.5, -0.25, 0.125], F)


def sensor_frame(b: Batch):
    """(origins, directions) of the batch in the frame of the pose (POSE_R, POSE_T): R^T (o - t) and R^T d.  The world rays the
    kernel and the restatement rebuild from them differ from the batch's in the last bit at most; both rebuild them alike."""
    Rt = POSE_R.T.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):  # the bad rays carry NaN and Inf
        o = ((b.origins.astype(np.float64) - POSE_T.astype(np.float64)) @ Rt.T).astype(F)
        d = (b.directions.astype(np.float64) @ Rt.T).astype(F)
    return o, d
