"""A restatement of the ray queries (include/mrhash_rays.h) on top of tests/raycast_ref.py: the sample rule
(sample_depths), the refinement, the gradient and the normal are raycast_ref.Raycaster's (D11), taken as they are through
inheritance; the block test is its vectorised one with the ray's own origin.  What is restated here is what D21 adds: the pose of
the batch, the bad-ray test, the ray's own end, and the counts.  The march goes sample by sample, no jump.

Like ray_fields.CountingRaycaster it notes, per ray, which events the ray met (EVENTS).  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import independent as ind
import raycast_ref as rr

F = np.float32
HIT, UNKNOWN, INSIDE, BAD = 1, 2, 4, 0x80
SKIP_REACH_VOXELS = F(65000.0)  # kRaySkipReachVoxels (mrh_raycast.h)

EVENTS = (
    "hit", "unknown", "inside",
    "first_unknown_at_0", "first_unknown_later",
    "absent_run",            # >= 2 consecutive samples in one absent block: the kernel may jump
    "jump_eligible",         # ... and the ray passes the kernel's reach gate
    "ends_in_absent_run",    # the ray's own last sample lies in such a run while the batch's samples go on: the jump must be clamped
    "trilinear_failed", "refine_rejected",
    "cut_by_tmax",           # tmax_i < max_range took samples away
    "zero_samples",
    "bad_origin_nan", "bad_direction_inf", "bad_direction_zero", "bad_origin_bound", "bad_tmax_nan",
    "hit_coarse",
)


class RayQuery(rr.Raycaster):
    """One batch definition: the map, the range interval and the sample spacing.  cast() takes the rays."""

    def __init__(self, m, min_range, max_range, step, truncation=None):
        self.m = m
        self.multi = isinstance(m, ind.MultiMap)
        step = F(step) if F(step) != 0 else F(F(0.5) * F(truncation))  # step 0: half the context's sdf_truncation
        self.min_range, self.max_range, self.step = F(min_range), F(max_range), step
        self.z = rr.sample_depths(min_range, max_range, step)
        self.keys = np.array(sorted(self._key(np.array(k, np.int64)) for k in m.blocks), np.int64) if m.blocks else np.zeros(0, np.int64)
        self.bound = F(F(1 << 20) * F(m.vs))
        self._o = np.zeros(3, F)

    # ---- raycast_ref.Raycaster's hooks, with the ray's own origin ----
    def point(self, d, z):  # P(z) = o_w + z d_w, per component
        o = self._o
        return (F(o[0] + F(F(z) * d[0])), F(o[1] + F(F(z) * d[1])), F(o[2] + F(F(z) * d[2])))

    def blocks_of(self, o, d, n) -> np.ndarray:
        """The block of the first n samples of one ray: [n, 3] int64."""
        P = (o[None, :] + (self.z[:n, None] * d[None, :]).astype(F)).astype(F)
        return ind.voxel_to_block(ind.world_to_voxel(self.m.vs, P), self.m.vs).astype(np.int64)

    def present_of(self, b) -> np.ndarray:
        inside = np.all((b >= -(1 << 20)) & (b < (1 << 20)), axis=-1)
        return inside & np.isin(self._key(b), self.keys)

    def refine(self, d, a, ad, b, bd):
        c = super().refine(d, a, ad, b, bd)
        if c is None:
            self._ev.add("refine_rejected")
        return c

    # ---- D21 ----
    @staticmethod
    def transform(o, d, R, t):
        """o_w,a = ((R[a,0] o_x + R[a,1] o_y) + R[a,2] o_z) + t[a]; d_w,a = (R[a,0] d_x + R[a,1] d_y) + R[a,2] d_z."""
        R, t = np.asarray(R, F).reshape(3, 3), np.asarray(t, F).reshape(3)
        ow = np.stack([((R[a, 0] * o[:, 0] + R[a, 1] * o[:, 1]) + R[a, 2] * o[:, 2]) + t[a] for a in range(3)], -1).astype(F)
        dw = np.stack([(R[a, 0] * d[:, 0] + R[a, 1] * d[:, 1]) + R[a, 2] * d[:, 2] for a in range(3)], -1).astype(F)
        return ow, dw

    def _bad(self, o, d, tm):
        ev = self._ev
        if tm is not None and np.isnan(tm):
            ev.add("bad_tmax_nan")
        if np.isnan(o).any():
            ev.add("bad_origin_nan")
        elif not np.all(np.abs(o) < self.bound):
            ev.add("bad_origin_bound")
        if np.isinf(d).any():
            ev.add("bad_direction_inf")
        if not np.any(d != 0):
            ev.add("bad_direction_zero")
        return (tm is not None and np.isnan(tm)) or not np.all(np.abs(o) < self.bound) or not np.all(np.isfinite(d)) or not np.any(d != 0)

    def cast_one(self, o, d, tm):
        """(range, status, normal[3], rgb[3], n_free, n_unknown, first_unknown) of one world-frame ray."""
        self._ev = ev = set()
        zero3f, zero3b = np.zeros(3, F), np.zeros(3, np.uint8)
        if self._bad(o, d, tm):
            return F(0), BAD, zero3f, zero3b, 0, 0, F(0)
        self._o = o
        end = self.max_range if tm is None else min(F(tm), self.max_range)  # fminf: neither is NaN here
        n = int(np.count_nonzero(self.z <= end))
        if n < len(self.z):
            ev.add("cut_by_tmax")
        if n == 0:
            ev.add("zero_samples")
            return F(0), 0, zero3f, zero3b, 0, 0, F(0)
        b = self.blocks_of(o, d, n)
        pres = self.present_of(b)
        invalid = ~pres  # grows by the samples whose trilinear fails
        self._runs(o, d, end, b, pres, n)
        inside, K, hit = False, n, None
        n_free = 0
        prev_valid, prev_d, prev_z, last = False, F(0), F(0), -2
        for k in np.flatnonzero(pres):
            if k != last + 1:
                prev_valid = False
            last = k
            z = self.z[k]
            ok, D = self.m.trilinear(self.point(d, z))
            if ok and prev_valid and prev_d > 0 and D <= 0:
                c = self.refine(d, prev_z, prev_d, z, D)
                if c is not None:
                    K, hit = int(k), F(c)
                    break
            if not ok:
                invalid[k] = True
                ev.add("trilinear_failed")
            elif D > 0:
                n_free += 1
            else:
                inside = True
            prev_valid, prev_d, prev_z = ok, D, z
        unknown = np.flatnonzero(invalid[:K])
        n_unknown = len(unknown)
        first = self.z[unknown[0]] if n_unknown else F(0)
        status = (HIT if hit is not None else 0) | (UNKNOWN if n_unknown else 0) | (INSIDE if inside else 0)
        nrm, rgb, rng = zero3f, zero3b, F(0)
        if hit is not None:
            P = self.point(d, hit)
            rng, nrm, rgb = hit, self.normal(P), np.array(self.m.get_voxel(P)[2], np.uint8)
            ev.add("hit")
            if self.multi and self.m.voxel_size_at(P) > self.m.vs:
                ev.add("hit_coarse")
        if n_unknown:
            ev.add("unknown")
            ev.add("first_unknown_at_0" if unknown[0] == 0 else "first_unknown_later")
        if inside:
            ev.add("inside")
        return rng, status, nrm, rgb, n_free, n_unknown, first

    def _runs(self, o, d, end, b, pres, n):
        ab = ~pres
        run = ab[1:] & ab[:-1] & np.all(b[1:] == b[:-1], axis=-1)
        if not run.any():
            return
        ev = self._ev
        ev.add("absent_run")
        reach = F(max(abs(o[0]), abs(o[1]), abs(o[2])) + F(end * max(abs(d[0]), abs(d[1]), abs(d[2]))))
        if reach < F(SKIP_REACH_VOXELS * self.m.vs):
            ev.add("jump_eligible")
            if run[-1] and n < len(self.z):  # the next sample of the batch would lie in the same absent block, or beyond
                bn = self.blocks_of(o, d, n + 1)[n]
                if np.all(bn == b[n - 1]):
                    ev.add("ends_in_absent_run")

    def cast(self, origins, directions, tmax=None, R=None, t=None):
        """dict of range [n], status [n], normals [n, 3], rgb [n, 3], counts [n, 2], first_unknown [n]; self.rays: the events."""
        o = np.ascontiguousarray(origins, F).reshape(-1, 3)
        d = np.ascontiguousarray(directions, F).reshape(-1, 3)
        n = len(o)
        tm = None if tmax is None else np.ascontiguousarray(tmax, F).reshape(-1)
        out = {"range": np.zeros(n, F), "status": np.zeros(n, np.uint8), "normals": np.zeros((n, 3), F), "rgb": np.zeros((n, 3), np.uint8),
               "counts": np.zeros((n, 2), np.uint32), "first_unknown": np.zeros(n, F)}
        self.rays = []
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if R is not None:
                o, d = self.transform(o, d, R, t)
            for i in range(n):
                r = self.cast_one(o[i], d[i], None if tm is None else tm[i])
                out["range"][i], out["status"][i], out["normals"][i], out["rgb"][i] = r[0], r[1], r[2], r[3]
                out["counts"][i] = (r[4], r[5])
                out["first_unknown"][i] = r[6]
                self.rays.append(frozenset(self._ev))
        return out

    def count(self, e):
        assert e in EVENTS, e
        return sum(1 for r in self.rays if e in r)


PLANES = ("range", "status", "normals", "rgb", "counts", "first_unknown")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, want, what, planes=PLANES, events=None):
    """Every plane as bytes; a difference names its first rays and both values."""
    for name in planes:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        if same_bits(a, b):
            continue
        n = len(a)
        bad = np.flatnonzero(np.any(a.view(np.uint8).reshape(n, -1) != b.view(np.uint8).reshape(n, -1), axis=1))
        lines = ["ray %d: got %s, want %s%s" % (i, a[i], b[i], ", events %s" % sorted(events[i]) if events else "") for i in bad[:5]]
        raise AssertionError("%s: %s differs at %d of %d rays\n%s" % (what, name, len(bad), n, "\n".join(lines)))
