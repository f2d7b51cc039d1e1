"""GPU half of map-to-map registration (mrh_align.h, include/mrhash_align.h): every output of mrh_align_map bit for bit
against the restatement of tests/align_ref.py — pose, status, counts, rms, all 32 sums, pivot and extent — on the hand-built scenes
whose coverage tests/test_align.py asserts; end to end on two fused maps; the reader contract; every refusal; the facade.  Maps are
imported, not fused, unless said otherwise."""
import ctypes as C

import numpy as np
import pytest

import align_ref as ar
import esdf_ref as er
import mc_fields as mf
import parity_utils as pu
import remap_ref as rm
import track_ref as tr
from mrhash_amd import capi, synth

pytestmark = pytest.mark.gpu

F = np.float32


def _engine(blocks, params, num_sdf_blocks=4096):
    e = pu.make_engine(capi.load_hip(), synth.CFG1, params, num_sdf_blocks)
    if blocks:
        e.import_blocks(*er.to_import(blocks))
    return e


def _result(R, t, info):
    return dict(info, R=R, t=t)


def _assert_same(got, want, what):
    bad = ar.same_result(got, want)
    assert not bad, f"{what}: {bad} differ: " + "; ".join(f"{k}: {got[k]} vs {want[k]}" for k in bad)


class Pair:
    """Two engines on the imported maps of a scene."""

    def __init__(self, name):
        self.name, self.s = name, ar.scene(name)
        s = self.s
        self.dst, self.src = _engine(s["db"], s["dp"]), _engine(s["sb"], s["sp"])

    def check(self, what=None, **kw):
        s = self.s
        args = dict(s["kw"], **kw)
        want = ar.align(s["dp"], s["db"], s["sp"], s["sb"], s["R"], s["t"], **args)
        got = _result(*self.dst.align_map(self.src, s["R"], s["t"], **args))
        print(what or self.name, {k: got[k] for k in ("status", "iterations_done", "samples", "accepted", "rms")})
        _assert_same(got, want, what or self.name)
        return got

    def close(self):
        self.dst.close()
        self.src.close()


@pytest.fixture(scope="module")
def corner():
    """The corner scene's two maps; the start is given per call."""
    p = Pair("truth")
    yield p
    p.close()


# ---- 1. the corner scene -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [1, 10, 64])
@pytest.mark.parametrize("start", ["truth", "start"])
def test_corner_scene(corner, start, iterations):
    s = ar.scene(start)
    want = ar.run_scene(start, iterations=iterations)
    got = _result(*corner.dst.align_map(corner.src, s["R"], s["t"], iterations=iterations))
    _assert_same(got, want, f"{start}, {iterations} iterations")
    assert got["status"] == capi.ALIGN_OK and got["iterations_done"] == iterations
    assert got["accepted"] > 8192  # more than 32 rows of the partial slab reach k_track_finish
    if iterations >= 10:
        t_err, deg = tr.pose_errors(got["R"], got["t"], ar.CORNER_RT, ar.CORNER_TT)
        print(f"{start}: {deg:.5f} deg, {1e3 * t_err:.3f} mm, rms {got['rms']:.7f}")
        assert deg < 0.02 and t_err < 0.001


# ---- 2. other voxel sizes, coarse blocks, holes, min_weight, a given pivot, far from the origin ---------------------------------------

@pytest.mark.parametrize("name", ["src_coarse_voxels", "src_fine_voxels", "adaptive_dst", "adaptive_src", "holes_dst", "min_weight", "pivot", "far"])
def test_scene(name):
    p = Pair(name)
    try:
        for e, key in ((p.dst, "adaptive_dst"), (p.src, "adaptive_src")):
            if name == key:
                d, _ = e.dump_blocks()
                assert 0 < int((d["resolution"] == 1).sum()) < len(d)
        got = p.check()
        assert got["status"] == capi.ALIGN_OK and got["accepted"] >= 64
        if name == "far":
            assert np.abs(got["pivot"]).min() > 26000.0
    finally:
        p.close()


@pytest.mark.parametrize("k", ar.COUNTS)
def test_sample_counts_around_one_workgroup(corner, k):
    s, pivot = corner.s, ar.scene("pivot")["kw"]["pivot"]
    sb, extent = ar.source_with_count(s["sp"], s["sb"], 0.15, k, pivot)
    src = _engine(sb, s["sp"])
    try:
        kw = dict(pivot=pivot, extent=extent, iterations=2, min_samples=1)
        want = ar.align(s["dp"], s["db"], s["sp"], sb, s["R"], s["t"], **kw)
        got = _result(*corner.dst.align_map(src, s["R"], s["t"], **kw))
        _assert_same(got, want, f"{k} samples")
        assert got["samples"] == k
    finally:
        src.close()


# ---- 3. the lost cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ar.LOST_SCENES)
def test_lost_cases(name):
    p = Pair(name)
    try:
        got = p.check()
        assert got["status"] == capi.ALIGN_LOST and got["iterations_done"] == 0
        assert rm.same_bits(got["R"], np.asarray(p.s["R"], F).reshape(3, 3)) and rm.same_bits(got["t"], np.asarray(p.s["t"], F))
        if name == "empty":
            assert got["source_blocks"] == 0 and got["samples"] == 0
        if name == "beyond":
            assert got["samples"] > 0 and got["accepted"] == 0
    finally:
        p.close()


# ---- 4. end to end on fused maps, and the reader contract ---------------------------------------------------------------------------------

def _blocks_of(e):
    d, v = e.dump_blocks()
    return {(int(x["x"]), int(x["y"]), int(x["z"])): vox.copy() for x, vox in zip(d, v)}


def _feed(e, f, R=None, t=None):
    e.set_pose(f.R if R is None else R, f.t if t is None else t)
    e.upload_depth(f.depth)
    e.upload_rgb(f.rgb)
    e.integrate()


def test_end_to_end_on_fused_maps_and_the_reader_contract():
    """Frames 0 .. 5 of the synthetic room go into A, frames 3 .. 8 into B, whose frame is displaced by T.  align_map from a start
    2.3 degrees and 52 mm off: bit-identical to the restatement on the two dumps, and closer to T than the start in both the angle and
    the translation.  The last frame of either map was host-fed and kept back by mrh_integrate: it is in the map the call reads.
    Both maps, their counters and the last extraction are as before."""
    K, params = synth.CFG1, dict(synth.CFG1_PARAMS)
    frames = list(synth.replica_stream(9, K=K))
    T_R, T_t = ar.CORNER_RT.astype(np.float64), ar.CORNER_TT.astype(np.float64)
    lib = capi.load_hip()
    a, b = pu.make_engine(lib, K, params, 32768), pu.make_engine(lib, K, params, 32768)
    a2, b2 = pu.make_engine(lib, K, params, 32768), pu.make_engine(lib, K, params, 32768)  # twins that are synchronised after every frame
    try:
        for f in frames[:6]:
            _feed(a, f)
        for f in frames[:6]:
            _feed(a2, f)
            a2.sync()
        for f in frames[3:]:
            for e in (b, b2):
                _feed(e, f, T_R.T @ f.R.astype(np.float64), T_R.T @ (f.t.astype(np.float64) - T_t))
            b2.sync()
        R0, t0 = ar.perturbed(T_R.astype(F), T_t.astype(F), angle=0.04, dt=(0.03, -0.03, 0.03))
        got = _result(*a.align_map(b, R0, t0))  # no sync, no dump before it: the kept-back frames run first
        twin = _result(*a2.align_map(b2, R0, t0))
        _assert_same(got, twin, "a kept-back frame is in the map the call reads")
        A, B = _blocks_of(a), _blocks_of(b)
        assert got["source_blocks"] == len(B)
        want = ar.align(params, A, params, B, R0, t0)
        _assert_same(got, want, "fused maps")
        (t_0, a_0), (t_1, a_1) = tr.pose_errors(R0, t0, T_R, T_t), tr.pose_errors(got["R"], got["t"], T_R, T_t)
        print(f"end to end: {a_0:.4f} deg, {1e3 * t_0:.2f} mm -> {a_1:.4f} deg, {1e3 * t_1:.2f} mm; {got['accepted']} of {got['samples']} samples, rms {1e3 * got['rms']:.3f} mm")
        assert got["status"] == capi.ALIGN_OK and a_1 < a_0 and t_1 < t_0
        # the reader contract: both maps, the counters and the last extraction
        tris = [e.extract_triangles() for e in (a, b)]
        s1 = [e.stats() for e in (a, b)]
        again = _result(*a.align_map(b, R0, t0))
        _assert_same(again, got, "a second call")
        for e, s, tri in zip((a, b), s1, tris):
            s2 = e.stats()  # it holds the triangle count of the last extraction
            for name, _ in capi.MrhStats._fields_:
                if "ms" not in name:
                    assert getattr(s, name) == getattr(s2, name), name
            assert len(tri) > 0 and rm.same_bits(e.extract_triangles(), tri)
        A2, B2 = _blocks_of(a), _blocks_of(b)
        assert sorted(A) == sorted(A2) and sorted(B) == sorted(B2)
        assert all(rm.same_bits(A[k], A2[k]) for k in A) and all(rm.same_bits(B[k], B2[k]) for k in B)
        r = pu.compare_maps(a, a2, tol=0.0)
        assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
        _feed(a, frames[6])  # the camera and the pose are still the stream's
        _feed(a2, frames[6])
        assert pu.compare_maps(a, a2, tol=0.0)["sdf_bit_exact"]
    finally:
        for e in (a, b, a2, b2):
            e.close()


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------------

def test_arguments_and_unsupported_contexts(corner):
    dst, src, lib = corner.dst, corner.src, corner.dst.lib
    Fp = C.POINTER(C.c_float)
    R, t = ar.CORNER_RT.reshape(9).copy(), ar.CORNER_TT.copy()
    oR, ot, info = np.zeros(9, F), np.zeros(3, F), capi.MrhAlignInfo()
    ok = capi.MrhAlignParams()
    before = (dst.dump_blocks(), src.dump_blocks())

    def call(p=ok, d=dst._ctx, s=src._ctx, pR=R, pt=t, oR=oR, ot=ot, info=info):
        ptr = lambda x: None if x is None else x.ctypes.data_as(Fp)  # noqa: E731
        return lib.mrh_align_map(d, s, C.byref(p) if p is not None else None, ptr(pR), ptr(pt), ptr(oR), ptr(ot), C.byref(info) if info is not None else None)

    assert call() == capi.MRH_OK and info.status == capi.ALIGN_OK and info.iterations_done == 10
    assert call(info=None) == capi.MRH_OK  # the info is optional
    for kw in (dict(p=None), dict(pR=None), dict(pt=None), dict(oR=None), dict(ot=None), dict(s=None)):
        assert call(**kw) == capi.MRH_ERR_INVALID_ARG, kw
        assert b"null argument" in lib.mrh_last_error(dst._ctx)
    assert call(d=None) == capi.MRH_ERR_INVALID_ARG
    assert call(s=dst._ctx) == capi.MRH_ERR_INVALID_ARG and b"the destination is the source" in lib.mrh_last_error(dst._ctx)

    def params(**kw):
        p = capi.MrhAlignParams()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [(params(reserved=(C.c_uint32 * 3)(0, 0, 1)), b"reserved"), (params(min_weight=256), b"min_weight"), (params(band=-0.1), b"band"), (params(band=1.5), b"band"),
           (params(dist_max=2.0), b"gate"), (params(dist_max=float("nan")), b"gate"), (params(iterations=-1), b"iterations"), (params(iterations=65), b"iterations"),
           (params(pivot=(C.c_float * 3)(0, float("inf"), 0)), b"pivot"), (params(extent=-1.0), b"extent"), (params(extent=float("nan")), b"extent")]
    for p, word in bad:
        assert call(p=p) == capi.MRH_ERR_INVALID_ARG and word in lib.mrh_last_error(dst._ctx), word
    for i in range(12):
        R2, t2 = R.copy(), t.copy()
        (R2 if i < 9 else t2)[i if i < 9 else i - 9] = [np.nan, np.inf, -np.inf][i % 3]
        assert call(pR=R2, pt=t2) == capi.MRH_ERR_INVALID_ARG and b"not finite" in lib.mrh_last_error(dst._ctx)
    S = (np.eye(3, dtype=F) * F(1.5)).reshape(9)
    assert call(pR=S) == capi.MRH_ERR_INVALID_ARG and b"not a rotation" in lib.mrh_last_error(dst._ctx)
    sharded = capi.Engine(capi.load_hip(), capi.Params(num_sdf_blocks=4096, shard_rank=0, shard_count=2, **mf.PARAMS))
    try:
        for c in (lambda: sharded.align_map(src, R, t), lambda: dst.align_map(sharded, R, t)):
            with pytest.raises(capi.MrhError) as ei:
                c()
            assert ei.value.code == capi.MRH_ERR_UNSUPPORTED and "sharded" in str(ei.value)
    finally:
        sharded.close()
    after = (dst.dump_blocks(), src.dump_blocks())
    for (d0, v0), (d1, v1) in zip(before, after):  # none of the calls touched either map
        assert rm.same_bits(d0, d1) and rm.same_bits(v0, v1)


# ---- 6. the facade -----------------------------------------------------------------------------------------------------------------------

def test_geowrapper_align_map(monkeypatch):
    """The facade on two maps fused from depth frames (it has no block import): B against A from a pose given as fuseMap takes it,
    against Engine.align_map on twin engines fed the same frames."""
    monkeypatch.setenv("MRHASH_NUM_SDF_BLOCKS", "16384")
    from mrhash.src.pygeowrapper import GeoWrapper

    p, Kc = synth.CFG1_PARAMS, synth.CFG1

    def wrapper():
        g = GeoWrapper(sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=p["virtual_voxel_size"],
                       n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=1, viewer_active=False,
                       marching_cubes_threshold=p["marching_cubes_threshold"], min_weight_threshold=p["min_weight_threshold"], min_depth=0.1, max_depth=8.0)
        g.setCamera(Kc.fx, Kc.fy, Kc.cx, Kc.cy, Kc.rows, Kc.cols, 0.1, 8.0, 0)
        return g

    ga, gb = wrapper(), wrapper()
    ea, eb = [pu.make_engine(capi.load_hip(), Kc, dict(p, min_depth=0.1, max_depth=8.0), 16384) for _ in range(2)]
    try:
        f = synth.cfg1_sphere()
        for g, e, reps in ((ga, ea, 3), (gb, eb, 2)):
            for _ in range(reps):
                g.setCurrPose(f.t, f.q)
                g.setDepthImage(f.depth)
                g.setRGBImage(f.rgb)
                g.compute()
                pu.feed(e, f)
        q = np.array([0.004, -0.006, 0.003, 1.0])
        q = (q / np.linalg.norm(q)).astype(F)
        t = np.array([0.006, -0.004, 0.008], F)
        gb.setCurrPose(t, q)
        pose = gb.getCurrPose()  # the matrix the facade makes of (t, q)
        gb.setCurrPose(f.t, f.q)
        for kw in (dict(), dict(iterations=3, min_weight=2)):
            ot, oq, info = ga.alignMap(gb, t, q, **kw)
            R, t2, want = ea.align_map(eb, pose[:3, :3].copy(), pose[:3, 3].copy(), **kw)
            _assert_same(_result(R, ot, info), _result(R, t2, want), f"alignMap {kw}")
            assert info["samples"] > 1000
            assert np.allclose(synth.quat_to_rot(oq), R, atol=1e-6) and abs(float(np.linalg.norm(oq)) - 1) < 1e-6
        with pytest.raises(RuntimeError, match=r"GeoWrapper::alignMap\|"):
            ga.alignMap(gb, np.zeros(2, F), q)
        with pytest.raises(RuntimeError):
            ga.alignMap(ga, t, q)  # dst == src
    finally:
        ea.close()
        eb.close()
        del ga, gb
