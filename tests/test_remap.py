"""CPU half of map-to-map resampling (include/mrhash_remap.h): the vectorised restatement of tests/remap_ref.py
pinned against the scalar point-query restatement (tests/query_ref.py), against the source map itself under the identity and
lattice-aligned translations, and against an analytic plane; and the coverage conditions of the GPU comparisons
(tests/test_remap_gpu.py), asserted here on the restatement alone."""
import functools

import numpy as np
import pytest

import mc_fields as mf
import query_ref as qr
import remap_ref as rm
from mrhash_amd import capi

F = np.float32
VS = mf.PARAMS["virtual_voxel_size"]
VAR_PARAMS = dict(mf.PARAMS, sdf_var_threshold=0.005)
VS4_PARAMS = dict(mf.PARAMS, virtual_voxel_size=2.0 ** -4)


def with_sumsq(blocks, seed=5):
    """The builders leave sum_squared at 0; a record carries nearest's: give every cell its own value."""
    rng = np.random.default_rng(seed)
    out = {}
    for b in sorted(blocks):
        v = blocks[b]
        res, vox = v if isinstance(v, tuple) else (0, v)
        vox = vox.copy()
        vox["sum_squared"] = rng.uniform(0.0, 4e-3, len(vox)).astype(F)
        out[b] = (res, vox) if isinstance(v, tuple) else vox
    return out


FIELDS = {
    "dense": lambda: (mf.PARAMS, with_sumsq(mf.sign_field(7))),
    "holes": lambda: (mf.PARAMS, with_sumsq(mf.sign_field(7, holes=0.03, starved=0.5, absent=0.1))),
    "adaptive": lambda: (VAR_PARAMS, with_sumsq(mf.sign_field(7, holes=0.02, absent=0.1, coarse=0.4, params=VAR_PARAMS))),
}


@functools.lru_cache(maxsize=None)
def generic(name, ratio=1.0, min_weight=0):
    params, blocks = FIELDS[name]()
    vs_d = 0.0 if ratio == 1.0 else float(F(F(VS) * F(ratio)))
    return rm.resample(params, blocks, rm.GENERIC_R, rm.GENERIC_T, vs_d, min_weight)


# ---- against the scalar query reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(FIELDS))
def test_samples_equal_the_scalar_smooth_query_and_nearest(name):
    """2 000 destination voxels drawn from the blocks of the generic pose: sdf and validity are query_ref's SMOOTH field
    at P, rgb / weight are query_ref._voxel's, sum_squared is that cell's."""
    params, blocks = FIELDS[name]()
    src = rm.Source(params, blocks)
    m = qr.ref_map(params, blocks)
    cand = rm.candidates(src, rm.GENERIC_R, rm.GENERIC_T, src.vs)
    rng = np.random.default_rng(21)
    d = generic(name)[0]  # half of the draws from the candidate blocks, half from the blocks that got a record
    kept = np.stack([d["x"], d["y"], d["z"]], -1).astype(np.int64)
    b = np.concatenate([cand[rng.integers(0, len(cand), 1000)], kept[rng.integers(0, len(kept), 1000)]])
    v = b * 8 + rng.integers(0, 8, (2000, 3))
    P = rm.source_positions(rm.GENERIC_R, rm.GENERIC_T, src.vs, v)
    valid, vox = rm.sample(src, P)
    dist, _, rgbw, state = qr.query(m, P, smooth=True, gradient=False)
    want = ((state & qr.DIST) != 0) & ((state & qr.BLOCK) != 0) & (rgbw[:, 3] >= 1)
    assert np.array_equal(valid, want)
    assert 0.1 < valid.mean() < 0.9, valid.mean()
    assert rm.same_bits(vox["sdf"][valid], dist[valid])
    assert np.array_equal(vox["rgb"][valid], rgbw[valid, :3]) and np.array_equal(vox["weight"][valid], rgbw[valid, 3])
    assert not vox[~valid].view(np.uint8).any()
    for i in np.flatnonzero(valid)[:300]:  # sum_squared: the cell query_ref._voxel reads
        vv = m._w2v(P[i])
        e = m.blocks[tuple(int(c) // 8 for c in vv)]
        res, cells = e if isinstance(e, tuple) else (0, e)
        l = [c % 8 for c in vv]
        li = l[2] * 64 + l[1] * 8 + l[0] if res == 0 else (l[2] // 2) * 16 + (l[1] // 2) * 4 + l[0] // 2
        assert vox["sum_squared"][i] == cells["sum_squared"][li]
    if name == "adaptive":
        assert np.any(state[valid] & qr.COARSE) and not np.all(state[valid] & qr.COARSE)


# ---- the identity and lattice-aligned translations -------------------------------------------------------------------------------

def _dense(blocks, what):
    a = np.zeros((32, 32, 32) + capi.VOXEL_DTYPE[what].shape, capi.VOXEL_DTYPE[what].base)
    for b, vox in blocks.items():
        v = mf.block_voxels(b)
        a[v[:, 0], v[:, 1], v[:, 2]] = vox[what]
    return a


@pytest.mark.parametrize("shift", [(0, 0, 0), (2, -1, 3), (-16, 0, 5)])
def test_identity_and_aligned_translations_copy_the_map(shift):
    """vs = 2^-4 and t = whole multiples of 8 vs: P is the lattice point itself, every weight of the interpolation is 0, and a
    valid voxel is the source voxel, bit for bit — valid exactly when the source cell and its seven +1 neighbours have weight > 0.
    One exception follows from D17's lerp a + w (b - a): at w = 0 a cell that stores -0 comes out as -0 + (+-0), which is +0
    unless the product is -0 too; such a cell must come out as a zero of either sign."""
    blocks = with_sumsq(mf.sign_field(7, holes=0.03, starved=0.5, params=VS4_PARAMS))
    vs = F(2.0 ** -4)
    t = (np.array(shift, np.float64) * 8 * float(vs)).astype(F)
    d, vox, info = rm.resample(VS4_PARAMS, blocks, rm.IDENTITY, t)
    w = _dense(blocks, "weight")
    ok = np.zeros((32, 32, 32), bool)
    ok[:31, :31, :31] = True
    for c in range(8):
        i, j, k = c & 1, (c >> 1) & 1, (c >> 2) & 1
        ok[:31, :31, :31] &= w[i:31 + i, j:31 + j, k:31 + k] > 0
    got = np.zeros((32, 32, 32), bool)
    sdf, ssq, rgb = _dense(blocks, "sdf"), _dense(blocks, "sum_squared"), _dense(blocks, "rgb")
    for n in range(len(d)):
        sv = mf.block_voxels((int(d["x"][n]) - shift[0], int(d["y"][n]) - shift[1], int(d["z"][n]) - shift[2]))  # the source voxels
        valid = vox[n]["weight"] > 0
        assert valid.any()
        assert np.all((sv[valid] >= 0) & (sv[valid] < 32))
        s = sv[valid]
        got[s[:, 0], s[:, 1], s[:, 2]] = True
        want_sdf, got_sdf = sdf[s[:, 0], s[:, 1], s[:, 2]], vox[n]["sdf"][valid]
        minus0 = want_sdf.view(np.uint32) == 0x80000000
        assert rm.same_bits(got_sdf[~minus0], want_sdf[~minus0]) and np.all(got_sdf[minus0] == 0)
        assert rm.same_bits(vox[n]["sum_squared"][valid], ssq[s[:, 0], s[:, 1], s[:, 2]])
        assert np.array_equal(vox[n]["rgb"][valid], rgb[s[:, 0], s[:, 1], s[:, 2]]) and np.array_equal(vox[n]["weight"][valid], w[s[:, 0], s[:, 1], s[:, 2]])
        assert not vox[n][~valid].view(np.uint8).any()
    assert np.array_equal(got, ok) and 0.5 < ok.mean() < 0.95
    assert info["valid_voxels"] == int(ok.sum())
    assert list(zip(d["x"], d["y"], d["z"])) == sorted(zip(d["x"], d["y"], d["z"])) and not d["resolution"].any()


# ---- an analytic plane -------------------------------------------------------------------------------------------------------------

def test_plane_field_under_the_generic_pose():
    """sdf = n . x - d, resampled: within 64 * 2^-24 * (max |W_a| + max |t_a| + max |sdf|) of n . R^T (W - t) - d in float64 — about
    ten roundings, each at most 2^-24 of a magnitude below that sum, slope 1, sqrt(3) for the three axes.  One voxel of slip would
    be 0.05 |n_a|, three orders of magnitude more."""
    d, vox, _ = rm.resample(mf.PARAMS, rm.plane_field(rm.PLANE_N, rm.PLANE_D, mf.PARAMS), rm.GENERIC_R, rm.GENERIC_T)
    err, tol, n = rm.plane_error(d, vox, rm.GENERIC_R, rm.GENERIC_T, VS)
    print(f"plane: max error {err:.3e}, tolerance {tol:.3e}, {n} valid voxels")
    assert n >= 20000 and err <= tol
    assert tol < 1e-3 * 0.05 * np.abs(rm.PLANE_N).min()


# ---- coverage of the named inputs ------------------------------------------------------------------------------------------------

def test_coverage_of_the_named_inputs():
    c = rm.counts(generic("dense")[1])
    print("dense", c)
    assert c["full"] >= 8 and c["partial"] >= 64
    c = rm.counts(generic("holes")[1])
    print("holes", c)
    assert c["partial"] >= 64
    c = rm.counts(generic("dense", 2.0)[1])
    print("vs_d = 2 vs_s", c)
    assert c["records"] >= 16
    c = rm.counts(generic("dense", 0.5)[1])
    print("vs_d = vs_s / 2", c)
    assert c["full"] >= 100
    c3 = rm.counts(generic("holes", 1.0, 3)[1])
    assert 0 < c3["valid"] < rm.counts(generic("holes")[1])["valid"]  # min_weight = 3 drops voxels, not all
    d, v, _ = generic("adaptive")
    assert rm.counts(v)["valid"] > 1000
