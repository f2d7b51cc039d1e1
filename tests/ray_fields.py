"""Hand-built scenes for the raycast (mrh_raycast.h), shared by tests/test_ray_fields.py (CPU: the scenes
reach the branches they are built for, counted on the restatement) and tests/test_ray_fields_gpu.py (HIP kernel vs restatement,
byte for byte).  Maps are tests/mc_fields.py pieces; nothing here is fused.

A fused room gives every ray a clean front face a few blocks into a dense map.  These scenes give the march what a room never
does: long absent stretches (the empty-space jump of ray_skip_absent against the restatement's literal march), directions with
a component of exactly 0, origins in the quarter-voxel rim of a block, rays that end in an absent block, crossings whose
previous sample is invalid, crossings whose refinement fails, back faces, samples that are exactly +-0, hits without a normal,
coarse blocks, blocks beyond the jump's two gates and at the last packed key.

  islands      three arms (+x, +y, +z): a positive slab, 4 absent blocks, a sign field with holes, a gap, a second sign field
  steps        islands at sample spacings of 0.1 voxel, the default and 10 voxels; rays of 1 and 2 samples; a ray end in the gap
  inside_out   slabs of alternating sign seen from behind, one block at a crossing removed
  zeros        a sign field with a quarter of its cells +-0, and slabs of exactly +0 and -0
  adaptive     fine and coarse blocks (mc_fields.neighbour_gallery, a variance-adaptive sign field) behind a positive slab
  ladder       rungs at 2^k blocks, k = 8 .. 16, with absent blocks, seen along +-x from both sides
  key_range    a rung that ends at the last packed block key
  shapes       islands at image sizes around the 8 x 8 wave and the 16 x 16 workgroup tile

CountingRaycaster / CountingSpherical return their parents' bytes and note, per ray, which of these events it met (EVENTS)."""
from __future__ import annotations

from collections import Counter, namedtuple
from functools import lru_cache

import numpy as np

import independent as ind
import mc_fields as mf
import raycast_ref as rr
from raycast_sph_ref import SphericalRaycaster

F = np.float32
PARAMS = mf.PARAMS
VAR_PARAMS = dict(mf.PARAMS, sdf_var_threshold=0.005)
VS = float(PARAMS["virtual_voxel_size"])
T = F(PARAMS["sdf_truncation"])
BLOCK = 8 * VS
SKIP_REACH_VOXELS = F(65000.0)  # kRaySkipReachVoxels (mrh_raycast.h)

Scene = namedtuple("Scene", "name blocks params model intr R t min_depth max_depth step")  # intr = (fx, fy, cx, cy, rows, cols)

EVENTS = (
    "jump",                    # an absent run of >= 2 consecutive samples in one block: the kernel may jump
    "jump_all_positive",       # ... on a ray with d > 0 on every axis
    "jump_negative_x", "jump_negative_y", "jump_negative_z",
    "jump_zero_inside",        # ... with a component of exactly 0 whose origin coordinate lies inside the block's shrunk box
    "jump_zero_rim",           # ... or in its quarter-voxel rim (no jump in that block)
    "jump_eligible",           # the kernel's two gates let the jump happen: reach < 65000 vs and bmax < block_shift_limit
    "jump_ineligible_reach", "jump_ineligible_shift",
    "ends_absent",             # the last sample lies in an absent block
    "beyond_keys",             # a sample lies in a block that no packed key can name
    "refine_rejected", "hit_after_rejection",
    "discarded_absent", "discarded_trilinear",  # valid D <= 0 after a valid D > 0 with only invalid samples in between
    "zero_taken",              # a crossing whose D is exactly 0 (always +0: see zeros_blocks)
    "prev_zero_not_taken",     # prev_d == 0 (either sign), D <= 0, both valid: not a crossing
    "back_face",               # prev_d < 0, D > 0, both valid
    "hit", "normal_stencil_failed", "normal_zero_length", "colour_absent", "hit_coarse",
)


def shift_limit(vs) -> int:
    """Map::block_shift_limit as mrh_create finds it (k_block_shift_limit), in numpy's float32."""
    vs = F(vs)
    eps, mbs = F(1e-5), F(8.0) * vs
    v = np.arange(1 << 23, dtype=np.int32)
    bp = np.floor((v.astype(F) * vs + eps) / mbs).astype(np.int32)
    pwn = (-v - np.where(v > 0, 7, 0)).astype(F) * vs
    bn = np.where(pwn >= 0, np.floor((pwn + eps) / mbs), np.ceil((pwn - eps) / mbs)).astype(np.int32)
    bad = np.nonzero((bp != (v >> 3)) | (bn != ((-v) >> 3)))[0]
    first_bad = int(bad[0]) if len(bad) else 1 << 23
    lim = 1
    while (lim << 1) <= first_bad and lim < (1 << 22):
        lim <<= 1
    return 0 if first_bad <= 1 else lim


_limits = {}


def _limit(vs):
    if float(vs) not in _limits:
        _limits[float(vs)] = shift_limit(vs)
    return _limits[float(vs)]


# ---- the counting restatement ------------------------------------------------------------------------------------------------

class _Counting:
    """Mixed in front of a Raycaster: render() returns the parent's bytes; `rays` holds one frozenset of EVENTS per rendered ray, in
    render order, and count(e) the rays with event e.  No arithmetic of the march is repeated here: refine, gradient and normal are
    wrapped, the rest is read off the sample blocks, present() and what cast hands to sample()."""

    def render(self, rows, cols):
        self.rays = []
        return super().render(rows, cols)

    def count(self, e):
        assert e in EVENTS, e
        return sum(1 for r in self.rays if e in r)

    def counts(self):
        c = Counter(e for r in self.rays for e in r)
        return {e: c[e] for e in EVENTS if c[e]}

    def sample_blocks(self, d):
        self._b = super().sample_blocks(d)
        self._i = 0
        return self._b

    def may_skip(self, d):
        """The kernel's per-ray gate, from the same float32 expressions."""
        t = self.cam.t
        reach = F(max(abs(t[0]), abs(t[1]), abs(t[2])) + F(self.cam.max_depth * max(abs(d[0]), abs(d[1]), abs(d[2]))))
        return bool(reach < F(SKIP_REACH_VOXELS * self.m.vs))

    def _jumps(self, d, pres, b):
        ab = ~pres
        run = ab[1:] & ab[:-1] & np.all(b[1:] == b[:-1], axis=-1)
        if not run.any():
            return
        ev = self._ev
        ev.add("jump")
        if np.all(d > 0):
            ev.add("jump_all_positive")
        for a, name in enumerate("xyz"):
            if d[a] < 0:
                ev.add("jump_negative_" + name)
        vs, t = self.m.vs, self.cam.t
        blocks = np.unique(b[1:][run], axis=0)
        for a in range(3):
            if d[a] == 0:
                lo = ((blocks[:, a] * 8).astype(F) - F(0.25)) * vs
                hi = ((blocks[:, a] * 8 + 7).astype(F) + F(0.25)) * vs
                inside = (t[a] >= lo) & (t[a] <= hi)
                if inside.any():
                    ev.add("jump_zero_inside")
                if (~inside).any():
                    ev.add("jump_zero_rim")
        m0 = blocks * 8
        bmax = np.maximum(np.abs(m0), np.abs(m0 + 7)).max(axis=-1)
        low = bmax < _limit(vs)
        if not self.may_skip(d):
            ev.add("jump_ineligible_reach")
        elif low.any():
            ev.add("jump_eligible")
        if (~low).any():
            ev.add("jump_ineligible_shift")

    def cast(self, d, present_row):
        self._ev = ev = set()
        b = self._b[self._i]
        self._i += 1
        self._jumps(d, present_row, b)
        if len(present_row) and not present_row[-1]:
            ev.add("ends_absent")
        if np.any((b < -(1 << 20)) | (b >= (1 << 20))):
            ev.add("beyond_keys")
        self._positive, self._between = False, set()  # the last valid sample was > 0; what made the samples since then invalid
        out = super().cast(d, present_row)
        if out[0] > 0:
            ev.add("hit")
            if "refine_rejected" in ev:
                ev.add("hit_after_rejection")
            P = self.point(d, out[0])
            blk = tuple(int(c) for c in ind.world_to_block(self.m.vs, np.array(P, F)))
            if blk not in self.m.blocks:
                ev.add("colour_absent")
            if self.multi and self.m.voxel_size_at(P) > self.m.vs:
                ev.add("hit_coarse")
        self.rays.append(frozenset(ev))
        return out

    def sample(self, k, ok, D, prev_valid, prev_d, gap):
        ev = self._ev
        if gap:
            self._between.add("discarded_absent")
        if not ok:
            self._between.add("discarded_trilinear")
            return
        if D <= 0 and self._positive and not prev_valid:
            ev.update(self._between)
        if prev_valid:
            if prev_d > 0 and D == 0:
                ev.add("zero_taken")
            if prev_d == 0 and D <= 0:
                ev.add("prev_zero_not_taken")
            if prev_d < 0 and D > 0:
                ev.add("back_face")
        self._positive, self._between = bool(D > 0), set()

    def refine(self, d, a, ad, b, bd):
        c = super().refine(d, a, ad, b, bd)
        if c is None:
            self._ev.add("refine_rejected")
        return c

    def gradient(self, P):
        g = super().gradient(P)
        if g is None:
            self._ev.add("normal_stencil_failed")
        return g

    def normal(self, P):
        n = super().normal(P)
        if not n.any() and "normal_stencil_failed" not in self._ev:
            self._ev.add("normal_zero_length")
        return n


class CountingRaycaster(_Counting, rr.Raycaster):
    pass


class CountingSpherical(_Counting, SphericalRaycaster):
    pass


def ref_map(params, blocks):
    """The restatement's map of a builder's blocks, through the same records the engine imports and dumps."""
    return rr.make_map(params, *mf.to_import(blocks))


def raycaster(s: Scene, m):
    cls = CountingSpherical if s.model == "spherical" else CountingRaycaster
    return cls(m, *s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step)


def pixels(s: Scene):
    r, c = np.mgrid[0:s.intr[4], 0:s.intr[5]]
    return r.ravel(), c.ravel()


# ---- poses and cameras ---------------------------------------------------------------------------------------------------------

def axis_rotation(a: int, sign: int) -> np.ndarray:
    """A signed axis permutation (det +1) that turns the camera's z into sign * e_a, its x into e_(a+1)."""
    R = np.zeros((3, 3), F)
    R[(a + 1) % 3, 0], R[(a + 2) % 3, 1], R[a, 2] = 1, sign, sign
    return R


def look_along(forward, roll_deg=0.0) -> np.ndarray:
    """A rotation whose third column is `forward` (normalised), rolled about it: no entry is 0 for a generic forward."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    up = np.array([0.0, 0.0, 1.0]) if abs(f[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, f)
    x /= np.linalg.norm(x)
    y = np.cross(f, x)
    c, s = np.cos(np.deg2rad(roll_deg)), np.sin(np.deg2rad(roll_deg))
    return np.stack([c * x + s * y, -s * x + c * y, f], -1).astype(F)


def pinhole(rows, cols, half_width=0.24):
    """Intrinsics whose centre pixel (rows // 2, cols // 2) looks along the camera's z exactly (cx = c - 0.5: u = 0) and whose
    longer side spans +-half_width at z = 1."""
    f = 0.5 * max(rows, cols) / half_width
    return (f, f, cols // 2 - 0.5, rows // 2 - 0.5, rows, cols)


def seam_camera(rows, cols, half_width=0.24):
    """Spherical intrinsics of a narrow sensor that looks along its own -x: the azimuths run across -pi, the seam of atan2 (as
    column 0 of synth.spherical_camera does), the elevations across 0."""
    f = 0.5 * max(rows, cols) / half_width
    return (f, f, cols // 2 - 0.5 + f * np.pi, rows // 2 - 0.5, rows, cols)


def seam_rotation(R: np.ndarray) -> np.ndarray:
    """The sensor-to-world rotation of a seam_camera that looks where the pinhole camera R looks: sensor -x = camera z, sensor y =
    camera x, sensor z = -camera y."""
    return (R.astype(np.float64) @ np.array([[0.0, 1, 0], [0, 0, -1], [-1, 0, 0]])).astype(F)


# ---- 1. islands ----------------------------------------------------------------------------------------------------------------

ARM_HALF = 2                                   # the arms' cross-section: blocks -2 .. 1 on both other axes
ARM_SLAB, ARM_FIELD1, ARM_FIELD2 = (2, 3), (7, 10), (13, 17)  # blocks along the arm; 4 and 3 absent blocks between them
INSIDE, RIM = F(3.3 * VS), F(-0.4 * VS)        # well inside block 0; in the rim of block 0 (voxel 0, below -0.25 voxel)
DEFAULT_STEP = float(F(0.5) * T)


def _arm_coords(a, w0, w1):
    out = []
    for w in range(w0, w1):
        for u in range(-ARM_HALF, ARM_HALF):
            for v in range(-ARM_HALF, ARM_HALF):
                c = [0, 0, 0]
                c[a], c[(a + 1) % 3], c[(a + 2) % 3] = w, u, v
                out.append(tuple(c))
    return out


@lru_cache(maxsize=None)
def islands_blocks(seed=11, holes=0.1, starved=0.5, absent=0.1, holes2=0.0):
    blocks = {}
    for a in range(3):
        for b in _arm_coords(a, *ARM_SLAB):
            blocks[b] = mf._uniform_block(b, F(0.5) * T)
        blocks.update(mf.fill(_arm_coords(a, *ARM_FIELD1), seed + 10 * a, holes=holes, starved=starved, absent=absent))
        blocks.update(mf.fill(_arm_coords(a, *ARM_FIELD2), seed + 10 * a + 1, holes=holes2))
    return blocks


def _axis_origin(a, sign, u):
    """On the axis of arm a, in front of the slab (sign +1) or 12 blocks behind the second field (sign -1); `u`: the coordinate on
    axis a + 1 (INSIDE or RIM), axis a + 2 is INSIDE."""
    t = np.zeros(3, F)
    t[a] = INSIDE if sign > 0 else F((8 * 29 + 3.3) * VS)
    t[(a + 1) % 3], t[(a + 2) % 3] = u, INSIDE
    return t


GENERIC_FORWARD = (1.0, 0.3, 0.25)
GENERIC_T = np.array([0.11, -0.93, -0.72], F)   # the axis of the generic view meets arm x's axis 3 m out


def generic_view(rows=16, cols=16):
    return pinhole(rows, cols), look_along(GENERIC_FORWARD, 17.0), GENERIC_T


def islands(rows=16, cols=16):
    blocks = islands_blocks()
    intr, R, t = generic_view(rows, cols)
    out = [Scene("islands generic", blocks, PARAMS, "pinhole", intr, R, t, 0.1, 8.0, DEFAULT_STEP)]
    for a in range(3):
        for sign in (1, -1):
            for u, where in ((INSIDE, "inside"), (RIM, "rim")):
                name = "islands %s%s %s" % ("+" if sign > 0 else "-", "xyz"[a], where)
                far = 7.5 if sign > 0 else 11.5
                out.append(Scene(name, blocks, PARAMS, "pinhole", pinhole(rows, cols), axis_rotation(a, sign), _axis_origin(a, sign, u), 0.1, far, DEFAULT_STEP))
    return out


# ---- 2. steps ------------------------------------------------------------------------------------------------------------------

def steps():
    blocks = islands_blocks()
    intr, R, t = generic_view(12, 12)
    one = lambda name, lo, hi, step, intr=intr: Scene("steps " + name, blocks, PARAMS, "pinhole", intr, R, t, lo, hi, step)  # noqa: E731
    # the rays of 1 and 2 samples: a narrow view along arm x's axis, every sample inside the second field
    few = lambda name, n: Scene("steps " + name, blocks, PARAMS, "pinhole", pinhole(12, 12, 0.1), axis_rotation(0, 1), _axis_origin(0, 1, INSIDE),  # noqa: E731
                                5.8, 5.8 + (n - 0.5) * DEFAULT_STEP, DEFAULT_STEP)
    return [
        one("0.1 voxel", 0.9, 3.6, 0.1 * VS),                      # 80 samples a block: the slab, the gap, the first field
        one("default", 0.1, 8.0, DEFAULT_STEP, generic_view()[0]),
        one("10 voxels", 0.1, 8.0, 10 * VS, generic_view()[0]),    # more than a block: nothing is jumped
        one("ends in the gap", 0.1, 2.2, DEFAULT_STEP),            # n_samples - 1 lies in an absent block
        few("1 sample", 1),
        few("2 samples", 2),
    ]


# ---- 3. inside_out -------------------------------------------------------------------------------------------------------------

INSIDE_OUT_SLABS = ((1, 3, -0.25), (3, 6, 0.5), (6, 8, -0.25), (8, 10, 0.5), (10, 12, -0.25))  # x0, x1, sdf / T
REMOVED = (6, 0, 0)  # the block at the first front face, on the camera's axis


@lru_cache(maxsize=None)
def inside_out_blocks():
    blocks = {}
    for x0, x1, s in INSIDE_OUT_SLABS:
        for b in mf.cluster((x0, -1, -1), (x1 - x0, 3, 3)):
            blocks[b] = mf._uniform_block(b, F(s) * T)
    del blocks[REMOVED]
    return blocks


INSIDE_OUT_T = np.array([0.11, 0.17, 0.13], F)


def inside_out(model="pinhole"):
    """From x = 0.11 m along +x with a slight tilt: - + - + - slabs.  The back face at x = 3 blocks is passed, the front face at 6
    is hit — except through the removed block (6, 0, 0), where the bracket loses its previous sample and the front face at 10 is hit."""
    blocks = inside_out_blocks()
    R = look_along((1.0, 0.04, 0.03), 5.0)
    if model == "spherical":
        return [Scene("inside_out spherical", blocks, PARAMS, model, seam_camera(16, 16, 0.3), seam_rotation(R), INSIDE_OUT_T, 0.1, 5.5, DEFAULT_STEP)]
    return [Scene("inside_out", blocks, PARAMS, model, pinhole(16, 16, 0.3), R, INSIDE_OUT_T, 0.1, 5.5, DEFAULT_STEP)]


# ---- 4. zeros ------------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def zeros_blocks(seed=5):
    """A sign field with a quarter of its cells +0 (and a sixteenth -0) at x = 2 .. 5, and beside it (y = 5 .. 8) four columns of
    uniform slabs along x, one block wide in y each:
      y = 5: +  then +0      a crossing whose D is exactly 0, deep enough in a constant region for a gradient of length 0
      y = 6: +  then -0      the same over cells that store -0
      y = 7: absent, +0, -   prev_d == 0 is no bracket: the - slab is not hit
      y = 8: absent, -0, -   the same over cells that store -0
    trilinearInterpolation never returns -0: its first sum c0 + c1 dd is -0 only if both terms are, and c0 = s0 = -0 makes
    c1 = s1 - s0 = s1 + 0, which is never -0; a later sum of a value that is not -0 and anything is not -0 either.  So D == -0 and
    prev_d == -0 do not occur on any map; cells of -0 act through a D of +0, which these columns pin."""
    blocks = mf.sign_field(seed, zeros=0.25, base=(2, -2, -2))
    cols = {5: ((2, 4, 0.5), (4, 6, 0.0)), 6: ((2, 4, 0.5), (4, 6, -0.0)), 7: ((3, 5, 0.0), (5, 7, -0.5)), 8: ((3, 5, -0.0), (5, 7, -0.5))}
    for y, slabs in cols.items():
        for x0, x1, s in slabs:
            for b in mf.cluster((x0, y, -1), (x1 - x0, 1, 3)):
                blocks[b] = mf._uniform_block(b, F(s) * T)
    # and a block at the origin, which no ray of the scene meets: a refinement that took prev_d == 0 for a bracket divides 0 by 0,
    # and where a NaN position converts to voxel (0, 0, 0) its trilinear then finds voxels instead of an absent block
    blocks[(0, 0, 0)] = mf._uniform_block((0, 0, 0), F(0.5) * T)
    return blocks


def zeros():
    blocks = zeros_blocks()
    R = look_along((1.0, 0.02, 0.03), 3.0)
    return [
        Scene("zeros field", blocks, PARAMS, "pinhole", pinhole(16, 16, 1.2), look_along((1.0, 0.05, 0.04), 11.0), np.array([0.07, -0.13, -0.21], F), 0.1, 4.0, DEFAULT_STEP),
        Scene("zeros slabs", blocks, PARAMS, "pinhole", pinhole(12, 24, 0.36), R, np.array([0.07, 2.77, 0.13], F), 0.1, 3.5, DEFAULT_STEP),
    ]


# ---- 5. adaptive ---------------------------------------------------------------------------------------------------------------

GALLERY_Z = (5, 11, 17, 23)  # the four neighbour galleries, 3 blocks thick, 3 absent blocks apart


@lru_cache(maxsize=None)
def adaptive_blocks():
    blocks = {}
    for (centre, other), z in zip(mf.NEIGHBOUR_PAIRS, GALLERY_Z):
        g, _ = mf.neighbour_gallery(centre, other, base=(0, 0, z), seed=26 + z, params=VAR_PARAMS)
        blocks.update(g)
    blocks.update(mf.sign_field(7, holes=0.02, absent=0.1, coarse=0.4, base=(-8, 0, 5), params=VAR_PARAMS))
    for b in mf.cluster((-8, 0, 2), (20, 12, 1)):
        blocks[b] = mf._uniform_block(b, F(0.5) * T)
    return blocks


def adaptive(model="pinhole"):
    blocks = adaptive_blocks()
    gallery_t = np.array([(8 * 6 + 3.3) * VS, (8 * 5 + 3.3) * VS, 0.11], F)
    field_t = np.array([(8 * -6 + 3.3) * VS, (8 * 2 + 3.3) * VS, 0.11], F)
    if model == "spherical":
        R = seam_rotation(look_along((0.05, 0.04, 1.0), 7.0))
        return [Scene("adaptive spherical", blocks, VAR_PARAMS, model, seam_camera(16, 16, 0.5), R, gallery_t, 0.1, 11.0, DEFAULT_STEP)]
    return [
        Scene("adaptive galleries", blocks, VAR_PARAMS, "pinhole", pinhole(24, 24, 0.5), axis_rotation(2, 1), gallery_t, 0.1, 11.0, DEFAULT_STEP),
        Scene("adaptive oblique", blocks, VAR_PARAMS, "pinhole", pinhole(16, 16, 0.5), look_along((0.12, 0.08, 1.0), 7.0), gallery_t, 0.1, 11.0, DEFAULT_STEP),
        Scene("adaptive field", blocks, VAR_PARAMS, "pinhole", pinhole(16, 16, 0.3), look_along((0.05, 0.04, 1.0), 7.0), field_t, 0.1, 4.5, DEFAULT_STEP),
    ]


# ---- 6. ladder -----------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def ladder_blocks(vs, seed=8, absent=0.15):
    """mf.ladder's cells on its rungs (and the origin cluster), with a share of every rung's blocks absent."""
    rng = np.random.default_rng(seed + 1)
    coords, kinds = list(mf.ORIGIN_CLUSTER), {}
    for _, _, c in mf.ladder_rungs():
        coords += c
        for b in c:
            if rng.random() < absent:
                kinds[b] = "absent"
    p = dict(PARAMS, virtual_voxel_size=float(vs))
    return mf.fill(coords, seed, holes=0.05, starved=0.2, params=p, kinds=kinds), p


LADDER_VS = (0.05, 0.0625, 0.02)
# block_shift_limit (shift_limit above) is 2^22 voxels at 0.05 m and at 2^-4 m: 8 vs is 8 RN(vs) exactly and the division is
# correctly rounded, so floor((v vs + eps) / (8 vs)) never leaves v >> 3 below the cap, and no rung of the ladder (<= 2^19 voxels)
# reaches it.  At 0.02 m the limit is 2^13 voxels = 2^10 blocks: rung 10 straddles it well inside the jump's reach (65000 voxels),
# so that voxel size is rendered on rungs 9 .. 11, with a step of 1.5 voxels (a block is 0.16 m there).
LADDER_RUNGS = {0.05: mf.LADDER_K, 0.0625: mf.LADDER_K, 0.02: (9, 10, 11)}


def _rung_frame(coords):
    c = np.array(coords)
    lo, hi = c.min(0), c.max(0)
    return lo, hi, (lo + hi + 1) * 4  # the rung's first and last block, the voxel coordinates of its centre


def ladder(vs, rows=10, cols=10):
    """Per rung and side two cameras on the rung's axis, 3 blocks outside either end, looking along +x and -x through it."""
    blocks, p = ladder_blocks(vs)
    step = DEFAULT_STEP if vs != 0.02 else 1.5 * vs
    out = []
    for k, side, coords in mf.ladder_rungs():
        if k not in LADDER_RUNGS[vs]:
            continue
        lo, hi, mid = _rung_frame(coords)
        for sign in (1, -1):
            x = (lo[0] - 3) * 8 + 3 if sign > 0 else (hi[0] + 4) * 8 + 3
            t = (np.array([x, mid[1] + 0.3, mid[2] + 0.3]) * float(vs)).astype(F)
            name = "ladder vs %g rung %d side %+d looking %sx" % (vs, k, side, "+" if sign > 0 else "-")
            out.append(Scene(name, blocks, p, "pinhole", pinhole(rows, cols, 0.35), axis_rotation(0, sign), t, 0.1, 14 * 8 * float(vs), step))
    return out


def ladder_wide(vs=0.05):
    """At rung 12 (2^12 blocks: 1638 m out at 0.05 m), one image with rays on both sides of the jump's reach test: the camera
    sits a block in front of the rung and looks along (1, 0.36, 0.1), so |d|_inf = d_x changes across the image, and max_depth
    is chosen so that |t|_inf + max_depth d_x crosses 65000 vs = 3250 m at the centre pixel.  Nearly all of the 11 000 samples
    of a ray lie in absent blocks beyond the rung."""
    blocks, p = ladder_blocks(vs)
    (k, side, coords), = [r for r in mf.ladder_rungs() if r[0] == 12 and r[1] == 1]
    lo, hi, mid = _rung_frame(coords)
    t = (np.array([(lo[0] - 1) * 8 + 3, mid[1] - 8.3, mid[2] - 2.3]) * float(vs)).astype(F)
    R = look_along((1.0, 0.36, 0.1), 4.0)
    far = (65000.0 * vs - float(t[0])) / float(R[0, 2])
    return [Scene("ladder wide", blocks, p, "pinhole", pinhole(12, 12, 0.3), R, t, 0.1, far, 0.15)]


@lru_cache(maxsize=None)
def _carried_rung(last_x, seed=8, absent_x=None):
    """The rung at +2^16 carried along x so that its last block is last_x, with ladder_blocks' share of absent blocks (and every
    block at x = absent_x)."""
    (k, side, coords), = [r for r in mf.ladder_rungs() if r[0] == 16 and r[1] == 1]
    shift = last_x - max(c[0] for c in coords)
    coords = [(c[0] + shift, c[1], c[2]) for c in coords]
    rng = np.random.default_rng(seed + 1)
    kinds = {b: "absent" for b in coords if rng.random() < 0.15 or b[0] == absent_x}
    return mf.fill(coords, seed, holes=0.05, starved=0.2, kinds=kinds), coords


FAR_ABSENT_X = (1 << 19) - 6


def ladder_far():
    """A rung that ends at block 2^19 - 2: the last place where every voxel still converts by the shift (bmax < 2^22), three
    octaves beyond the jump's reach.  A float32 position has 0.3 voxel between neighbours there, more than the quarter voxel
    ray_skip_absent keeps from a block's faces: only the reach test stands between these rays and a wrong jump.  Of the blocks
    below 2^19 every fifth one (2^19 - 6, - 11, ...) has a shrunk high face (8 b + 7.25) vs that converts to a voxel of block
    b + 1; the rung's blocks at x = 2^19 - 6 are absent, those behind them present."""
    blocks, coords = _carried_rung((1 << 19) - 2, absent_x=FAR_ABSENT_X)
    lo, hi, mid = _rung_frame(coords)
    out = []
    for sign in (1, -1):
        x = (lo[0] - 3) * 8 + 3 if sign > 0 else (hi[0] + 4) * 8 + 3
        t = (np.array([x, mid[1] + 0.3, mid[2] + 0.3]) * VS).astype(F)
        out.append(Scene("ladder far looking %sx" % ("+" if sign > 0 else "-"), blocks, PARAMS, "pinhole", pinhole(12, 12, 0.45), axis_rotation(0, sign), t, 0.1, 14 * BLOCK, 0.1 * VS))
    return out


# ---- 7. key_range --------------------------------------------------------------------------------------------------------------

def key_range():
    """A rung carried to the last packed key, x = 2^20 - 1, and a camera 3 blocks in front of it looking outward: the samples
    behind the rung lie in blocks x >= 2^20, which no key holds."""
    blocks, coords = _carried_rung((1 << 20) - 1)
    lo, hi, mid = _rung_frame(coords)
    t = (np.array([(lo[0] - 3) * 8 + 3, mid[1] + 0.3, mid[2] + 0.3]) * VS).astype(F)
    return [Scene("key_range", blocks, PARAMS, "pinhole", pinhole(12, 12, 0.35), axis_rotation(0, 1), t, 0.1, 14 * BLOCK, DEFAULT_STEP)]


# ---- 8. shapes -----------------------------------------------------------------------------------------------------------------

SHAPES = ((1, 1), (1, 17), (7, 9), (17, 33), (33, 16))


def shapes():
    blocks = islands_blocks()
    out = []
    for rows, cols in SHAPES:
        intr, R, t = generic_view(rows, cols)
        out.append(Scene("shapes %d x %d" % (rows, cols), blocks, PARAMS, "pinhole", intr, R, t, 0.1, 8.0, DEFAULT_STEP))
    return out


# ---- 9. spherical --------------------------------------------------------------------------------------------------------------

def islands_spherical():
    blocks = islands_blocks()
    _, R, t = generic_view()
    return [
        Scene("islands spherical generic", blocks, PARAMS, "spherical", seam_camera(16, 16), seam_rotation(R), t, 0.1, 8.0, DEFAULT_STEP),
        Scene("islands spherical +x", blocks, PARAMS, "spherical", seam_camera(16, 16), seam_rotation(axis_rotation(0, 1)), _axis_origin(0, 1, INSIDE), 0.1, 7.5, DEFAULT_STEP),
    ]


# ---- the groups: one map each, and what its renders have to reach -----------------------------------------------------------------

GROUPS = {
    "islands": islands,
    "steps": steps,
    "inside_out": inside_out,
    "zeros": zeros,
    "adaptive": adaptive,
    "ladder 0.05": lambda: ladder(0.05) + ladder_wide(0.05),
    "ladder 0.0625": lambda: ladder(0.0625),
    "ladder 0.02": lambda: ladder(0.02),
    "ladder far": ladder_far,
    "key_range": key_range,
    "shapes": shapes,
    "spherical islands": islands_spherical,
    "spherical inside_out": lambda: inside_out("spherical"),
    "spherical adaptive": lambda: adaptive("spherical"),
}
NUM_SDF_BLOCKS = {"adaptive": 8192, "spherical adaptive": 8192}  # 4096 elsewhere

_MARCH = ("jump", "jump_eligible", "ends_absent", "discarded_absent", "discarded_trilinear", "back_face", "normal_stencil_failed")
# rays of the group's renders together that meet the event, at least (8: the floor of every event that is not one designed ray)
FLOORS = {
    "islands": dict.fromkeys(_MARCH + ("jump_all_positive", "jump_negative_x", "jump_negative_y", "jump_negative_z", "jump_zero_inside", "jump_zero_rim",
                                       "refine_rejected", "hit_after_rejection"), 8),
    "steps": dict.fromkeys(_MARCH + ("refine_rejected",), 8),
    "inside_out": dict.fromkeys(("jump", "back_face", "discarded_absent", "ends_absent"), 8),
    "zeros": dict.fromkeys(("zero_taken", "prev_zero_not_taken", "normal_zero_length", "back_face"), 8),
    "adaptive": dict.fromkeys(_MARCH + ("hit_coarse", "refine_rejected", "hit_after_rejection", "jump_zero_inside"), 8),
    "ladder 0.05": dict.fromkeys(_MARCH + ("jump_ineligible_reach", "refine_rejected", "hit_after_rejection", "jump_negative_x", "jump_zero_inside"), 8),
    "ladder 0.0625": dict.fromkeys(_MARCH + ("jump_ineligible_reach", "refine_rejected", "hit_after_rejection", "jump_negative_x", "jump_zero_inside"), 8),
    "ladder 0.02": dict.fromkeys(_MARCH + ("jump_ineligible_shift", "refine_rejected", "hit_after_rejection"), 8),
    "ladder far": dict.fromkeys(("jump", "jump_ineligible_reach", "ends_absent", "back_face", "normal_stencil_failed"), 8),
    "key_range": dict.fromkeys(("jump", "jump_ineligible_shift", "jump_ineligible_reach", "beyond_keys", "ends_absent"), 8),
    "shapes": dict.fromkeys(_MARCH, 8),
    "spherical islands": dict.fromkeys(_MARCH + ("refine_rejected", "jump_zero_inside"), 8),
    "spherical inside_out": dict.fromkeys(("jump", "back_face", "discarded_absent"), 8),
    "spherical adaptive": dict.fromkeys(_MARCH + ("hit_coarse",), 8),
}
# images whose hit share is not held between 10 % and 90 %, and why
NO_HIT_SHARE = {
    "steps ends in the gap": "max_depth lies in the gap behind the positive slab: no ray can hit",
    "steps 1 sample": "a hit needs two samples",
    "shapes 1 x 1": "one ray",
}


def hit_share(caster) -> float:
    return caster.count("hit") / len(caster.rays)


def check_coverage(group: str, renders):
    """renders: [(scene, caster after render())] of every scene of the group.  Raises AssertionError where a floor is missed."""
    total = Counter()
    for s, rc in renders:
        total.update(rc.counts())
        if s.name not in NO_HIT_SHARE:
            assert 0.10 <= hit_share(rc) <= 0.90, (s.name, hit_share(rc))
    for e, floor in FLOORS[group].items():
        assert total[e] >= floor, (group, e, total[e], floor)
    return dict(total)
