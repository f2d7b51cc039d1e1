"""Hand-built maps for the marching-cubes extraction (mrh_mc.h), shared by tests/test_mc_fields.py (CPU: pins the oracle on
them) and tests/test_mc_fields_gpu.py (HIP library vs oracle, byte for byte).  Builders only: pure numpy, deterministic, no
library calls.  Every builder returns {(bx, by, bz): voxels[512]} — a coarse block is (1, voxels[64]) — which is what
esdf_ref.to_import takes, takes a `base` block offset, and fills `rgb` with varying bytes so that the colour interpolation
is compared as well.

A fused TSDF is smooth, single-signed along a ray, weighted inside the band only and close to the origin; these fields are
none of that, which is where the kernel's shortcuts (the sign prescreen, the known-stencil evaluations, the corner records)
and the reference's literal loop can part:

  case_gallery       every one of the 256 cube indices at a known voxel, at four lattice phases
  sparse_field       a clearly positive sea with a few odd cells: the field on which the sign prescreen drops voxels and a single
                     cell decides a triangle; its starved-only form isolates the class-16 rule of the wide window
  sign_field         i.i.d. signs, magnitudes on and next to the prescreen's thresholds, holes, starved cells, -0, absent
                     and coarse blocks
  odd_cell           one odd cell in a uniform sea, at block corners / edges / faces / depths 1..4 from a face
  neighbour_gallery  one fine, coarse or absent block in each of the 26 neighbour positions of a fine or coarse block
  ladder             blocks at 2^k, k = 8 .. 16, on both sides: the switches `staged` and `fine_known` of k_mc

No NaN and no Inf anywhere in these fields.  What the device post-process (the min-index hash of the vertex merge) does with
a NaN vertex has not been established; that is to be read from the code, not tried on a device."""
from __future__ import annotations

import numpy as np

from esdf_ref import SPHERE_PARAMS, to_import  # noqa: F401  (to_import: re-exported for the tests)
from mrhash_amd import capi

F = np.float32
PARAMS = dict(SPHERE_PARAMS)
DIRS26 = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def thresholds(params=PARAMS):
    """(sdf_bound, lo, hi) as the extraction computes them, in float32 without contraction: sdf_bound = trunc + trunc_scale *
    max_depth (mrh_extract.h mc_pass_shape), lo = 1e-3 sdf_bound, hi = 1.001 sdf_bound (mrh_mc.h k_mc)."""
    bound = F(F(params["sdf_truncation"]) + F(F(params["sdf_truncation_scale"]) * F(params["max_depth"])))
    return bound, F(F(1e-3) * bound), F(F(1.001) * bound)


def prevfloat(x):
    return np.nextafter(F(x), F(-np.inf))


def nextfloat(x):
    return np.nextafter(F(x), F(np.inf))


def magnitudes(params=PARAMS) -> np.ndarray:
    """{0.5 lo, prevfloat(lo), lo, 0.01, T / 3, T, hi, nextfloat(hi), 1.01 T}: on, just inside and just outside "clearly signed"."""
    T = F(params["sdf_truncation"])
    _, lo, hi = thresholds(params)
    return np.array([F(0.5) * lo, prevfloat(lo), lo, F(0.01), T / F(3), T, hi, nextfloat(hi), F(1.01) * T], F)


def _shift(base):
    return np.array(base, np.int64)


def _rgb_of(v):
    """Colour bytes from the voxel coordinates [n, 3]: neighbours differ in every channel."""
    v = v.astype(np.int64)
    return np.stack([(37 * v[:, 0] + 11 * v[:, 1] + 5 * v[:, 2]) & 0xFF, (7 * v[:, 0] + 41 * v[:, 1] + 13 * v[:, 2] + 64) & 0xFF,
                     (3 * v[:, 0] + 17 * v[:, 1] + 43 * v[:, 2] + 128) & 0xFF], -1).astype(np.uint8)


def block_voxels(b, coarse=False):
    """Voxel coordinates of the block's cells in storage order: 512 fine ones, or the 64 even ones of a coarse block."""
    side, sc = (4, 2) if coarse else (8, 1)
    lin = np.arange(side ** 3)
    return np.stack([b[0] * 8 + sc * (lin % side), b[1] * 8 + sc * ((lin // side) % side), b[2] * 8 + sc * (lin // (side * side))], -1)


def _uniform_block(b, sdf, weight=1, coarse=False):
    v = block_voxels(b, coarse)
    blk = np.zeros(len(v), capi.VOXEL_DTYPE)
    blk["sdf"], blk["weight"], blk["rgb"] = F(sdf), weight, _rgb_of(v)
    return blk


# ---- case gallery ----------------------------------------------------------------------------------------------------------

GALLERY_PHASES = (0, 2, 3, 1)  # local site coordinates {2, 6}, {4, 0}, {5, 1}, {3, 7}: interior, across the low and the high side
GALLERY_BLOCKS = 5


def gallery_site(case: int, phase: int):
    """Cell (relative to the field's first cell) of the site built for cube index `case`: 8 x 8 x 4 sites on a 4-cell pitch from
    cell 2 + phase; which site takes which case changes with the phase."""
    s = (37 * case + 11 * phase) & 255  # 37 is odd: a permutation of 0 .. 255
    return np.array([2 + phase + 4 * (s & 7), 2 + phase + 4 * ((s >> 3) & 7), 2 + phase + 4 * (s >> 6)], np.int64)


def case_gallery(phase: int, base=(0, 0, 0), params=PARAMS):
    """(blocks, sites): a 5^3-block field of weight-1 cells with sdf +0 and, around the site of case c, the eight cells at
    (+-1, +-1, +-1) holding -T where bit k of c is set and +T elsewhere (k: bit 0 = +x, bit 1 = +y, bit 2 = +z).  Corner k of the
    site's voxel then reads a trilinear value of -+T / 8 (one non-zero cell of eight, all weights 1/2): the voxel has cube index c.
    sites = [((vx, vy, vz), c)]."""
    assert 0 <= phase <= 3
    T = F(params["sdf_truncation"])
    n = GALLERY_BLOCKS * 8
    sdf = np.zeros((n, n, n), F)  # [x, y, z] relative cells
    o = _shift(base) * 8
    sites = []
    for c in range(256):
        s = gallery_site(c, phase)
        for k in range(8):
            d = np.array([1 if k & 1 else -1, 1 if k & 2 else -1, 1 if k & 4 else -1])
            q = s + d
            assert sdf[q[0], q[1], q[2]] == 0
            sdf[q[0], q[1], q[2]] = -T if (c >> k) & 1 else T
        sites.append((tuple(int(a) for a in s + o), c))
    blocks = {}
    for bx in range(GALLERY_BLOCKS):
        for by in range(GALLERY_BLOCKS):
            for bz in range(GALLERY_BLOCKS):
                b = (bx + int(base[0]), by + int(base[1]), bz + int(base[2]))
                v = block_voxels(b)
                r = v - o
                blk = np.zeros(512, capi.VOXEL_DTYPE)
                blk["sdf"], blk["weight"], blk["rgb"] = sdf[r[:, 0], r[:, 1], r[:, 2]], 1, _rgb_of(v)
                blocks[b] = blk
    return blocks, sites


# ---- random signed cells ---------------------------------------------------------------------------------------------------

def _random_cells(rng, b, coarse, holes, starved, params, zeros=0.02):
    v = block_voxels(b, coarse)
    n = len(v)
    mags = magnitudes(params)
    sdf = mags[rng.integers(0, len(mags), n)]
    sdf = np.where(rng.random(n) < 0.5, -sdf, sdf).astype(F)
    u = rng.random(n)
    sdf = np.where(u < zeros, F(0.0), sdf)                          # exactly +0
    sdf = np.where((u >= zeros) & (u < 1.25 * zeros), F(-0.0), sdf)  # and a quarter as many -0
    weight = rng.integers(1, 5, n)
    hole = rng.random(n) < holes
    keep = rng.random(n) < starved  # a starved cell: the weight is gone, the sdf stays
    zero = np.where(rng.random(n) < 0.25, F(-0.0), F(0.0))
    blk = np.zeros(n, capi.VOXEL_DTYPE)
    blk["sdf"] = np.where(hole & ~keep, zero, sdf)
    blk["weight"] = np.where(hole, 0, weight)
    blk["rgb"] = rng.integers(0, 256, (n, 3))
    return blk


def fill(coords, seed, holes=0.0, starved=0.0, absent=0.0, coarse=0.0, params=PARAMS, kinds=None, zeros=0.02):
    """sign_field's cells on the given block coordinates (sorted: the result does not depend on their order).  kinds: optional
    {coord: "fine" | "coarse" | "absent"} overriding the draw."""
    rng = np.random.default_rng(seed)
    blocks = {}
    for b in sorted(set(tuple(int(a) for a in c) for c in coords)):
        ua, uc = rng.random(), rng.random()
        kind = (kinds or {}).get(b) or ("absent" if ua < absent else ("coarse" if uc < coarse else "fine"))
        blk = _random_cells(rng, b, kind == "coarse", holes, starved, params, zeros)  # drawn for absent blocks too: one stream per layout
        if kind == "coarse":
            blocks[b] = (1, blk)
        elif kind == "fine":
            blocks[b] = blk
    return blocks


def cluster(base, dims):
    return [(int(base[0]) + x, int(base[1]) + y, int(base[2]) + z) for x in range(dims[0]) for y in range(dims[1]) for z in range(dims[2])]


def sign_field(seed, holes=0.0, starved=0.0, absent=0.0, coarse=0.0, base=(0, 0, 0), params=PARAMS, zeros=0.02):
    """A 4^3-block cluster: magnitudes from magnitudes(params), i.i.d. signs, a share `zeros` (2 %) of the cells exactly +0 and
    a quarter as many -0, weights 1 .. 4; a share `holes` of the cells has weight 0, of which a share `starved` keeps its sdf and
    the rest store +-0; a share `absent` of the blocks is missing and a share `coarse` has 64 voxels at resolution 1.  With many
    zeros AND holes a corner often falls back to a raw sample that is exactly 0: vertexInterp snaps such a vertex onto the corner
    (|d| < 1e-5), which gives bit-identical vertices and degenerate triangles for the mesh post-process to merge and drop."""
    return fill(cluster(base, (4, 4, 4)), seed, holes, starved, absent, coarse, params, zeros=zeros)


# ---- a clearly positive sea with sparse odd cells ---------------------------------------------------------------------------

def _sparse_cells(rng, b, coarse, odd, params, starved_only):
    v = block_voxels(b, coarse)
    n = len(v)
    T = F(params["sdf_truncation"])
    _, lo, hi = thresholds(params)
    if starved_only:
        sea = np.array([lo, nextfloat(lo), F(0.01)], F)
        odd_sdf, odd_w = np.array([-T, -hi, -T / F(3)], F), np.array([0, 0, 0])
    else:
        sea = np.array([lo, F(0.01), T / F(3), T, hi], F)  # all "clearly positive" (class 1)
        # an odd cell: clearly negative, just outside "clearly", +-0, or without weight (sdf 0, sdf kept: starved)
        odd_sdf = np.array([-lo, -T, -hi, -prevfloat(lo), -nextfloat(hi), F(0.5) * lo, F(0.0), F(-0.0), F(0.0), -T, -hi, T], F)
        odd_w = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0])
    pick = rng.integers(0, len(odd_sdf), n)
    is_odd = rng.random(n) < odd
    blk = np.zeros(n, capi.VOXEL_DTYPE)
    blk["sdf"] = np.where(is_odd, odd_sdf[pick], sea[rng.integers(0, len(sea), n)])
    blk["weight"] = np.where(is_odd, np.where(odd_w[pick] > 0, rng.integers(1, 5, n), 0), rng.integers(1, 5, n))
    blk["rgb"] = rng.integers(0, 256, (n, 3))
    return blk


def sparse_field(seed, odd=0.03, absent=0.0, coarse=0.0, base=(0, 0, 0), dims=(4, 4, 4), params=PARAMS, starved_only=False):
    """The prescreen's own field.  sign_field has both signs in every window, so the prescreen never drops a voxel of it; and
    one -T cell in a +T sea (odd_cell) cannot turn a trilinear corner value negative (7/8 T - 1/8 T > 0), so no triangle
    depends on it.  Here the sea is clearly positive with magnitudes from {lo, 0.01, T / 3, T, hi} and a share `odd` of the
    cells is odd: clearly negative (-lo, -T, -hi), just outside "clearly" (-prevfloat(lo), -nextfloat(hi), 0.5 lo), +-0, unseen
    (weight 0, sdf 0) or starved (weight 0, sdf -T, -hi or +T).  With odd = 0.03 about half of the 3^3 windows hold no odd cell
    (dropped), a third holds exactly one, at any of the 27 places, in the same or a neighbouring block; a hole sends corners to the
    raw sample, where ONE cell decides the sign; next to a coarse block a re-sample blends a starved cell in.
    starved_only: a sea of small clearly positive values (lo, nextfloat(lo), 0.01) whose only odd cells are starved ones with a large
    negative sdf.  No weighted cell is negative, so every triangle of such a map comes from a re-sample that blended a starved cell
    in (vds.cu:296-309) — the one thing the wide window's class-16 rule exists for."""
    rng = np.random.default_rng(seed)
    blocks = {}
    for b in sorted(cluster(base, dims)):
        ua, uc = rng.random(), rng.random()
        is_coarse = uc < coarse
        blk = _sparse_cells(rng, b, is_coarse, odd, params, starved_only)
        if ua >= absent:
            blocks[b] = (1, blk) if is_coarse else blk
    return blocks


# ---- one odd cell in a uniform sea -----------------------------------------------------------------------------------------

ODD_KINDS = ("minus_T", "half_lo", "unseen", "starved")
# local position of the odd cell in its cluster's centre block; one cluster per position (they must stay >= 8 cells apart)
ODD_POSITIONS = (
    [("corner", (x, y, z)) for z in (0, 7) for y in (0, 7) for x in (0, 7)]
    + [("edge", (4, 0, 0)), ("edge", (7, 4, 0)), ("edge", (0, 7, 4))]
    + [("face", (0, 4, 4)), ("face", (4, 7, 4)), ("face", (4, 4, 0))]
    + [("depth", (1, 4, 4)), ("depth", (2, 4, 4)), ("depth", (3, 4, 4))]  # 1, 2, 3 cells behind the -x face ...
    + [("interior", (4, 4, 4))]                                             # ... and 4: outside every 7^3 window across it
)
ODD_STRIDE = 5  # blocks from one cluster to the next: 3 + two absent


def odd_coarse_direction(pos):
    """The neighbour that the multi-resolution variant makes coarse: the one the odd cell lies against (-x for the cells inside)."""
    d = tuple(-1 if c == 0 else (1 if c == 7 else 0) for c in pos)
    return d if d != (0, 0, 0) else (-1, 0, 0)


def odd_cell(kind: str, base=(0, 0, 0), coarse_neighbour=False, params=PARAMS):
    """(blocks, cells): one 3^3-block cluster per entry of ODD_POSITIONS, every cell weighted with sdf +T, except the odd cell
    of the cluster's centre block: -T, 0.5 lo, (weight 0, sdf 0) or (weight 0, sdf -T).  coarse_neighbour: exactly one of the
    26 neighbours of each centre block is coarse (odd_coarse_direction), so that the 7^3 window is used.  cells = the odd voxels."""
    assert kind in ODD_KINDS
    T = F(params["sdf_truncation"])
    _, lo, _ = thresholds(params)
    sdf, weight = {"minus_T": (-T, 1), "half_lo": (F(0.5) * lo, 1), "unseen": (F(0), 0), "starved": (-T, 0)}[kind]
    blocks, cells = {}, []
    for i, (_, pos) in enumerate(ODD_POSITIONS):
        c0 = (int(base[0]) + ODD_STRIDE * i, int(base[1]), int(base[2]))
        centre = (c0[0] + 1, c0[1] + 1, c0[2] + 1)
        d = odd_coarse_direction(pos)
        for b in cluster(c0, (3, 3, 3)):
            is_coarse = coarse_neighbour and b == (centre[0] + d[0], centre[1] + d[1], centre[2] + d[2])
            blk = _uniform_block(b, T, 1, is_coarse)
            blocks[b] = (1, blk) if is_coarse else blk
        li = pos[2] * 64 + pos[1] * 8 + pos[0]
        blocks[centre]["sdf"][li], blocks[centre]["weight"][li] = sdf, weight
        cells.append((centre[0] * 8 + pos[0], centre[1] * 8 + pos[1], centre[2] * 8 + pos[2]))
    return blocks, cells


# ---- one block of another kind in each of the 26 neighbour positions --------------------------------------------------------

NEIGHBOUR_PAIRS = (("fine", "coarse"), ("coarse", "fine"), ("fine", "absent"), ("coarse", "absent"))


def neighbour_gallery(centre: str, other: str, base=(0, 0, 0), seed=26, params=PARAMS):
    """(blocks, layout): 26 clusters of 3^3 blocks, two absent blocks apart; every block is of kind `centre` except one neighbour
    of the cluster's centre block — a different one per cluster — which is of kind `other`.  Cells: sign_field's, 5 % holes, a
    fifth of them starved.  layout = [(centre block, direction)]."""
    kinds, layout, coords = {}, [], []
    for i, d in enumerate(DIRS26):
        c0 = (int(base[0]) + ODD_STRIDE * (i % 6), int(base[1]) + ODD_STRIDE * (i // 6), int(base[2]))
        mid = (c0[0] + 1, c0[1] + 1, c0[2] + 1)
        for b in cluster(c0, (3, 3, 3)):
            kinds[b] = centre
        kinds[(mid[0] + d[0], mid[1] + d[1], mid[2] + d[2])] = other
        coords += cluster(c0, (3, 3, 3))
        layout.append((mid, d))
    return fill(coords, seed, holes=0.05, starved=0.2, params=params, kinds=kinds), layout


# ---- the ladder: blocks where the extraction switches paths -----------------------------------------------------------------

LADDER_K = tuple(range(8, 17))


def ladder_rungs():
    """[(k, side, coords)]: for k = 8 .. 16 a cluster of 7 x 3 x 3 blocks with x = 2^k - 5 .. 2^k + 1 (side +1) and its mirror
    image at -2^k (side -1); y and z are small and change sign from rung to rung.  With amax = max |block coordinate| = |x|:
    k_mc stages a block iff (amax + 3) * 8 < block_shift_limit, a power of two in voxels — for a limit of 2^(k + 3) voxels that is
    amax < 2^k - 3, which rung k straddles — and evaluates known stencils iff (amax + 2) * 8 < 2^18, amax < 2^15 - 2: rung 15."""
    out = []
    for k in LADDER_K:
        sy, sz = (1 if k & 1 else -1), (1 if k & 2 else -1)
        y0, z0 = (1 if sy > 0 else -3) + sy * (k - 8), (2 if sz > 0 else -4) + sz * 2 * (k - 8)
        for side in (1, -1):
            xs = range((1 << k) - 5, (1 << k) + 2) if side > 0 else range(-(1 << k) - 1, -(1 << k) + 6)
            out.append((k, side, [(x, y0 + y, (z0 + z) * side) for x in xs for y in range(3) for z in range(3)]))
    return out


ORIGIN_CLUSTER = cluster((-2, -2, -2), (4, 4, 4))  # straddles the three sign changes of the block coordinates


def ladder(vs, coarse=0.0, seed=8, params=PARAMS):
    """(blocks, params with virtual_voxel_size = vs): every rung of ladder_rungs() and the origin cluster, sign_field's cells
    with 5 % holes (a fifth starved).  vs = 0.05 and 0.0625: the shift limit of 0.05 m falls on some rung whatever power of two
    it is (<= 2^19 voxels); with 2^-4 m it lies beyond the ladder, so rung 15 crosses the known-stencil bound while still staged."""
    coords = list(ORIGIN_CLUSTER)
    for _, _, c in ladder_rungs():
        coords += c
    p = dict(params, virtual_voxel_size=float(vs))
    return fill(coords, seed, holes=0.05, starved=0.2, coarse=coarse, params=p), p
