"""A restatement of map-to-map registration (include/mrhash_align.h) in numpy, vectorised: the source samples, the
SMOOTH field of D17 with its analytic gradient on the destination (remap_ref.Source's lookups, every operation on float32
arrays rounded one by one, no FMA), the per-sample linearisation, and track_ref's exact sums, binary64 solve and pose update.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

import remap_ref as rm
import track_ref as tr
from mrhash_amd import capi

F = np.float32
D = np.float64
ALIGN_OK, ALIGN_LOST = 0, 1
MAX_SAMPLES = 1 << 26
GATES = ("range", "corners", "band", "residual", "lever")  # steps 2, 3, 4, 5 and 7


def defaults(band, dist_max, iterations, min_samples, src_truncation, dst_truncation):
    """The parameter block with its zeros replaced (include/mrhash_align.h)."""
    if F(band) == 0:
        band = min(F(src_truncation), F(dst_truncation))
    if F(dist_max) == 0:
        dist_max = min(F(band), F(1.0))
    return F(band), F(dist_max), int(iterations) or 10, int(min_samples) or 64


def samples(params: dict, blocks: dict, band, min_weight=0, pivot=None, extent=0.0):
    """(P [n, 3] f32, s [n] f32, v [n, 3] int64) of the accepted cells, blocks in (x, y, z) order, cells in storage order.  The
    crop applies when extent > 0."""
    vs = F(params["virtual_voxel_size"])
    Ps, ss, vv = [], [], []
    for b, e in sorted(blocks.items()):
        res, vox = e if isinstance(e, tuple) else (0, e)
        side, k = (4, 2) if res else (8, 1)
        lin = np.arange(side ** 3)
        v = np.stack([b[0] * 8 + k * (lin % side), b[1] * 8 + k * ((lin // side) % side), b[2] * 8 + k * (lin // (side * side))], -1).astype(np.int64)
        vox = vox[: side ** 3]
        s = vox["sdf"].astype(F)
        P = (v.astype(F) * vs).astype(F)
        with np.errstate(invalid="ignore"):
            ok = (vox["weight"] >= max(1, int(min_weight))) & (np.abs(s) < F(band))
            if F(extent) > 0:
                c = np.asarray(pivot, F).reshape(3)
                ok &= np.all(np.abs((P - c).astype(F)) <= F(extent), axis=-1)
        Ps.append(P[ok]); ss.append(s[ok]); vv.append(v[ok])
    if not Ps:
        return np.zeros((0, 3), F), np.zeros(0, F), np.zeros((0, 3), np.int64)
    return np.concatenate(Ps), np.concatenate(ss), np.concatenate(vv)


def auto_pivot(v, vs):
    """(c [3] f32, extent f32) from the integer box of the accepted voxel coordinates v [n, 3] (n > 0)."""
    lo, hi = v.min(axis=0).astype(np.int64), v.max(axis=0).astype(np.int64)
    c = (((lo + hi) >> 1).astype(F) * F(vs)).astype(F)
    return c, F(F(int(((hi - lo) // 2).max()) + 1) * F(vs))


def _lerp(a, b, w):
    return (a + (w * (b - a).astype(F)).astype(F)).astype(F)


def field(m: rm.Source, W):
    """The SMOOTH field of D17 with its gradient at W [n, 3] f32 (every |W_a| below the bound): (found [n], d [n] f32, g [n, 3] f32);
    d and g are 0 where not found."""
    W = np.asarray(W, F).reshape(-1, 3)
    n = len(W)
    if len(m.keys) == 0:
        return np.zeros(n, bool), np.zeros(n, F), np.zeros((n, 3), F)
    h = m.voxel_size(W)
    u = (W / h[:, None]).astype(F)
    f = np.floor(u).astype(F)
    w = (u - f).astype(F)
    s = np.zeros((n, 8), F)
    good = np.ones(n, bool)
    for c in range(8):
        off = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], F)
        pos = ((f + off).astype(F) * h[:, None]).astype(F)
        r, l = m.voxel_at(pos)
        cell = m.vox[np.maximum(r, 0), l]
        good &= (r >= 0) & (cell["weight"] > 0)
        s[:, c] = cell["sdf"]
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(all="ignore"):
        c00, c10 = _lerp(s[:, 0], s[:, 1], wx), _lerp(s[:, 2], s[:, 3], wx)
        c01, c11 = _lerp(s[:, 4], s[:, 5], wx), _lerp(s[:, 6], s[:, 7], wx)
        c0, c1 = _lerp(c00, c10, wy), _lerp(c01, c11, wy)
        d = _lerp(c0, c1, wz)
        gx = (_lerp(_lerp((s[:, 1] - s[:, 0]).astype(F), (s[:, 3] - s[:, 2]).astype(F), wy),
                    _lerp((s[:, 5] - s[:, 4]).astype(F), (s[:, 7] - s[:, 6]).astype(F), wy), wz) / h).astype(F)
        gy = (_lerp((c10 - c00).astype(F), (c11 - c01).astype(F), wz) / h).astype(F)
        gz = ((c1 - c0).astype(F) / h).astype(F)
    g = np.stack([gx, gy, gz], -1)
    return good, np.where(good, d, F(0)).astype(F), np.where(good[:, None], g, F(0)).astype(F)


def sample_terms(dst: rm.Source, P, s, c, R32, tau32, band, dist_max, s_a):
    """Steps 1-7 for every sample: (accepted [n] bool, J~ [n, 6] int64, e~ [n] int64, rejected {gate: count})."""
    P, s = np.asarray(P, F).reshape(-1, 3), np.asarray(s, F).reshape(-1)
    c, tau32 = np.asarray(c, F).reshape(3), np.asarray(tau32, F).reshape(3)
    R32 = np.asarray(R32, F).reshape(3, 3)
    n = len(P)
    rejected = {}
    with np.errstate(all="ignore"):
        q = (P - c).astype(F)
        a = tr._rows3(R32, q[:, 0], q[:, 1], q[:, 2])
        W = np.stack([(a[i] + tau32[i]).astype(F) for i in range(3)], -1)
        ok = np.all(np.abs(W) < rm.bound(dst.vs), axis=-1)
        rejected["range"] = int(n - ok.sum())
        found, d, g = np.zeros(n, bool), np.zeros(n, F), np.zeros((n, 3), F)
        idx = np.flatnonzero(ok)
        if len(idx):
            found[idx], d[idx], g[idx] = field(dst, W[idx])
        rejected["corners"] = int((ok & ~found).sum())
        ok &= found
        inside = np.abs(d) < F(band)
        rejected["band"] = int((ok & ~inside).sum())
        ok &= inside
        e = (s - d).astype(F)
        near = np.abs(e) <= F(dist_max)
        rejected["residual"] = int((ok & ~near).sum())
        ok &= near
        gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
        J = [((a[1] * gz).astype(F) - (a[2] * gy).astype(F)).astype(F), ((a[2] * gx).astype(F) - (a[0] * gz).astype(F)).astype(F),
             ((a[0] * gy).astype(F) - (a[1] * gx).astype(F)).astype(F), gx, gy, gz]
        Js = [(J[i] * (F(s_a) if i < 3 else tr.J_ONE)).astype(F) for i in range(6)]
        lever = np.ones(n, bool)
        for i in range(6):
            lever &= np.abs(Js[i]) < tr.J_LIMIT  # a NaN is rejected
        rejected["lever"] = int((ok & ~lever).sum())
        ok &= lever
        es = (e * tr.E_ONE).astype(F)
        Jt = np.stack([np.where(ok, np.rint(Js[i]), 0).astype(np.int64) for i in range(6)], -1)
        et = np.where(ok, np.rint(es), 0).astype(np.int64)
    return ok, Jt, et, rejected


def linearise(dst, P, s, c, R32, tau32, band, dist_max, s_a, order=None) -> np.ndarray:
    ok, Jt, et, _ = sample_terms(dst, P, s, c, R32, tau32, band, dist_max, s_a)
    return tr.sums_of(ok, Jt, et, order=order)


def _rc(R, c):
    """R c in binary64, each row (R_i0 c_x + R_i1 c_y) + R_i2 c_z."""
    c = np.asarray(c, F).astype(D)
    return np.array([(R[i, 0] * c[0] + R[i, 1] * c[1]) + R[i, 2] * c[2] for i in range(3)], D)


def align(dst_params, dst_blocks, src_params, src_blocks, R_init, t_init, band=0.0, dist_max=0.0, iterations=0, min_samples=0, min_weight=0,
          pivot=None, extent=0.0) -> dict:
    """mrh_align_map as D19 defines it.  Returns R, t (float32), status, iterations_done, source_blocks, samples, accepted, rms,
    pivot, extent, sums (int64 [32]) and `rejected`: per gate, the samples it rejected over all linearisations."""
    band, dist_max, iterations, min_samples = defaults(band, dist_max, iterations, min_samples, src_params["sdf_truncation"], dst_params["sdf_truncation"])
    vs_s = F(src_params["virtual_voxel_size"])
    c = np.zeros(3, F) if pivot is None or not F(extent) > 0 else np.asarray(pivot, F).reshape(3)
    P, s, v = samples(src_params, src_blocks, band, min_weight, c, extent)
    assert len(P) <= MAX_SAMPLES
    extent = F(extent)
    if len(P) and not extent > 0:
        c, extent = auto_pivot(v, vs_s)
    R32, t32 = np.asarray(R_init, F).reshape(3, 3), np.asarray(t_init, F).reshape(3)
    R, t = R32.astype(D), t32.astype(D)
    status, done, sums = ALIGN_LOST, 0, np.zeros(32, np.int64)
    rejected = {k: 0 for k in GATES}
    if len(P):
        dst = rm.Source(dst_params, dst_blocks)
        s_a = tr.angle_scale(extent)
        tau = _rc(R, c) + t
        status = ALIGN_OK
        for _ in range(iterations):
            ok, Jt, et, rej = sample_terms(dst, P, s, c, R.astype(F), tau.astype(F), band, dist_max, s_a)
            for k in GATES:
                rejected[k] += rej[k]
            sums = tr.sums_of(ok, Jt, et)
            xi = tr.solve(sums, extent, min_samples)
            if xi is None:
                status = ALIGN_LOST
                break
            R, tau = tr.update(R, tau, xi)
            done += 1
        t = tau - _rc(R, c)
    n = int(sums[28])
    rms = float(np.sqrt(D(sums[27]) / D(n)) / D(262144.0)) if n else 0.0
    return dict(R=R.astype(F), t=t.astype(F), status=status, iterations_done=done, source_blocks=len(src_blocks), samples=len(P), accepted=n, rms=rms,
                pivot=np.asarray(c, F), extent=F(extent), sums=sums, rejected=rejected)


def same_result(got: dict, want: dict) -> list:
    """Names of the outputs of mrh_align_map that differ in any bit."""
    bad = [k for k in ("R", "t", "pivot", "sums") if not rm.same_bits(np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1))]
    bad += [k for k in ("status", "iterations_done", "samples", "accepted", "source_blocks") if int(got[k]) != int(want[k])]
    bad += [k for k in ("rms",) if np.float64(got[k]).tobytes() != np.float64(want[k]).tobytes()]
    bad += [k for k in ("extent",) if F(got[k]).tobytes() != F(want[k]).tobytes()]
    return bad


# ---- the corner scene: three planes, all six degrees of freedom observable -------------------------------------------------------

CORNER_N = rm.rotation((1, 2, 3), 0.4).astype(D)  # the planes' normals: its rows
CORNER_O = np.array([-0.3, -0.25, -0.35], D)
CORNER_RT = rm.rotation((0.2, 1, -0.3), 0.35)     # the truth: W = R_T P + t_T
CORNER_TT = np.array([0.4, -0.25, 0.15], F)
CORNER_BASE, CORNER_DIMS = (-3, -3, -3), (6, 6, 6)


def corner_sdf(W, trunc):
    """d(W) = clamp(min_i (n_i . W - o_i), +-trunc) in binary64 at W [n, 3]."""
    return np.clip((np.asarray(W, D) @ CORNER_N.T - CORNER_O).min(axis=-1), -float(trunc), float(trunc))


def corner_field(params, R=None, t=None, base=CORNER_BASE, dims=CORNER_DIMS, weight=3, shift=(0, 0, 0)) -> dict:
    """The corner scene sampled on dims blocks from `base`: the cell at voxel v holds d(R (v vs) + t), rounded to float32 once
    ((R, t) = None: the destination, sampled at W itself).  shift: a block offset added to the keys only, which moves the whole map
    by 8 shift voxels."""
    vs, trunc = float(F(params["virtual_voxel_size"])), float(F(params["sdf_truncation"]))
    blocks = {}
    for bx in range(dims[0]):
        for by in range(dims[1]):
            for bz in range(dims[2]):
                b = (base[0] + bx, base[1] + by, base[2] + bz)
                v = np.array(b, np.int64) * 8 + rm.LOCAL
                X = v * vs
                if R is not None:
                    X = X @ np.asarray(R, F).reshape(3, 3).astype(D).T + np.asarray(t, F).astype(D)
                blk = np.zeros(512, capi.VOXEL_DTYPE)
                blk["sdf"] = corner_sdf(X, trunc).astype(F)
                blk["weight"] = weight
                blk["rgb"] = np.stack([(37 * v[:, 0] + 11 * v[:, 1]) & 0xFF, (7 * v[:, 1] + 13 * v[:, 2]) & 0xFF, (3 * v[:, 0] + 43 * v[:, 2]) & 0xFF], -1)
                blocks[(b[0] + shift[0], b[1] + shift[1], b[2] + shift[2])] = blk
    return blocks


def perturbed(R, t, angle=0.1, axis=(1, -2, 0.5), dt=(0.09, -0.08, 0.09)):
    """A start off the pose (R, t): rotated by `angle` about `axis` (0.1 rad = 5.7 degrees) and shifted by dt (150 mm)."""
    dR = rm.rotation(axis, angle).astype(D)
    return (dR @ np.asarray(R, F).reshape(3, 3).astype(D)).astype(F), (np.asarray(t, F).astype(D) + np.asarray(dt, D)).astype(F)


# ---- the scenes of the tests (tests/test_align.py asserts their coverage on the restatement, tests/test_align_gpu.py compares) ----

def coarsen(blocks: dict, share, seed) -> dict:
    """A share of the fine blocks replaced by coarse ones that keep the cells at the even voxel coordinates."""
    rng = np.random.default_rng(seed)
    even = np.array([(2 * k) * 64 + (2 * j) * 8 + 2 * i for k in range(4) for j in range(4) for i in range(4)])
    return {b: ((1, v[even].copy()) if rng.random() < share else v) for b, v in sorted(blocks.items())}


def n_coarse(blocks: dict) -> int:
    return sum(isinstance(v, tuple) for v in blocks.values())


def with_holes(blocks: dict, seed=31, holes=0.05, starved=0.5, absent=0.05, random_blocks=0.04) -> dict:
    """mc_fields.fill's kinds laid over a field: its weight-0 cells (holes that store +-0, starved cells that keep an sdf) replace
    the field's, its absent blocks are dropped, and a few blocks are its random cells altogether (steep gradients, large residuals)."""
    import mc_fields as mf

    rnd = mf.fill(list(blocks), seed, holes=holes, starved=starved, absent=absent)
    rng = np.random.default_rng(seed + 1)
    out = {}
    for b in sorted(blocks):
        whole = rng.random() < random_blocks
        if b not in rnd:
            continue
        blk, r = blocks[b].copy(), rnd[b]
        hole = r["weight"] == 0
        blk[hole] = r[hole]
        out[b] = r if whole else blk
    return out


def shifted_truth(R, t, k, vs):
    """The pose between two maps that were both moved by k blocks: t + delta - R delta, delta = 8 k vs (binary64, rounded once)."""
    delta = np.asarray(k, D) * 8 * float(F(vs))
    return (np.asarray(t, F).astype(D) + delta - np.asarray(R, F).reshape(3, 3).astype(D) @ delta).astype(F)


FAR_SHIFT = (1 << 16, -(1 << 16), 1 << 16)  # the maps straddle +-2^16 blocks: voxel -> block leaves the shift for the float detour
BEYOND_SHIFT = ((1 << 17) + 8, 0, 0)        # |W_x| >= 2^20 voxels: past D17's bound
SCENES = ("truth", "start", "src_coarse_voxels", "src_fine_voxels", "adaptive_dst", "adaptive_src", "holes_dst", "min_weight", "pivot", "far", "beyond",
          "plane", "few", "empty")
LOST_SCENES = ("beyond", "plane", "few", "empty")
COUNTS = (1, 255, 256, 257)  # sample counts around one workgroup of the linearisation (source_with_count)
_cache = {}


def scene(name: str) -> dict:
    """dict(dp, db, sp, sb, R, t, kw): destination and source (params, blocks), the start and the other arguments of align()."""
    if name in _cache:
        return _cache[name]
    import mc_fields as mf

    P = mf.PARAMS
    VAR = dict(P, sdf_var_threshold=0.005)
    start = perturbed(CORNER_RT, CORNER_TT)
    s = dict(dp=P, sp=P, R=start[0], t=start[1], kw={})
    if name not in ("far", "beyond", "plane"):
        s["db"] = corner_field(P)
    if name not in ("src_coarse_voxels", "src_fine_voxels", "far", "beyond", "plane", "empty"):
        s["sb"] = corner_field(P, CORNER_RT, CORNER_TT)
    if name == "truth":
        s["R"], s["t"] = CORNER_RT, CORNER_TT
    elif name == "src_coarse_voxels":
        s["sp"] = dict(P, virtual_voxel_size=float(F(F(P["virtual_voxel_size"]) * F(2))))
        s["sb"] = corner_field(s["sp"], CORNER_RT, CORNER_TT, base=(-2, -2, -2), dims=(4, 4, 4))
    elif name == "src_fine_voxels":
        s["sp"] = dict(P, virtual_voxel_size=float(F(F(P["virtual_voxel_size"]) / F(1.5))))
        s["sb"] = corner_field(s["sp"], CORNER_RT, CORNER_TT, base=(-4, -4, -4), dims=(8, 8, 8))
    elif name == "adaptive_dst":
        s["dp"], s["db"] = VAR, coarsen(s["db"], 0.4, 41)
    elif name == "adaptive_src":
        s["sp"], s["sb"] = VAR, coarsen(s["sb"], 0.4, 42)
    elif name == "holes_dst":
        s["db"] = with_holes(s["db"])
    elif name == "min_weight":
        rng = np.random.default_rng(43)
        for b in sorted(s["sb"]):
            s["sb"][b]["weight"] = rng.integers(1, 5, 512)
        s["kw"] = dict(min_weight=3)
    elif name == "pivot":
        s["kw"] = dict(pivot=np.array([0.1, 0.2, -0.05], F), extent=0.6)
    elif name in ("far", "beyond"):
        k = FAR_SHIFT if name == "far" else BEYOND_SHIFT
        s["db"], s["sb"] = corner_field(P, shift=k), corner_field(P, CORNER_RT, CORNER_TT, shift=k)
        s["t"] = shifted_truth(s["R"], s["t"], k, P["virtual_voxel_size"])
    elif name == "plane":
        s["db"] = s["sb"] = rm.plane_field(rm.PLANE_N, rm.PLANE_D, P)
        s["R"], s["t"] = perturbed(rm.IDENTITY, np.zeros(3, F), angle=0.02, dt=(0.01, -0.01, 0.01))
    elif name == "few":
        s["R"], s["t"], s["kw"] = CORNER_RT, CORNER_TT, dict(min_samples=1000000)
    elif name == "empty":
        s["sb"] = {}
    _cache[name] = s
    return s


def run_scene(name: str, **kw) -> dict:
    s = scene(name)
    return align(s["dp"], s["db"], s["sp"], s["sb"], s["R"], s["t"], **dict(s["kw"], **kw))


def source_with_count(params: dict, blocks: dict, band, k: int, pivot):
    """(blocks, extent): the fine-block source thinned to exactly k samples — the k accepted cells nearest to `pivot` (maximum norm in
    float32, ties by list position) keep their weight, every other cell gets weight 0 — and the extent of the cube that holds them."""
    P, _, v = samples(params, blocks, band)
    dist = np.abs((P - np.asarray(pivot, F)).astype(F)).max(axis=-1)
    keep = np.lexsort((np.arange(len(P)), dist))[:k]
    out = {b: vox.copy() for b, vox in blocks.items()}
    for vox in out.values():
        vox["weight"] = 0
    for x, y, z in v[keep]:
        out[(x >> 3, y >> 3, z >> 3)]["weight"][(z & 7) * 64 + (y & 7) * 8 + (x & 7)] = 3
    return out, F(dist[keep[-1]])
