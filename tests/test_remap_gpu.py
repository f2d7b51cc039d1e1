"""GPU half of map-to-map fusion (mrh_remap.h, include/mrhash_remap.h): the records of mrh_resample_map byte for byte
against the restatement of tests/remap_ref.py — descs, their order and all 512 x 12 bytes — on hand-built single- and
multi-resolution maps (tests/mc_fields.py) under the identity, translations and a general pose, at other voxel sizes, far from
the origin and past the two range limits; mrh_fuse_map against resample + unpack and against the oracle's merge; the reader
contract; every refusal, the facade and the device variant.  Maps are imported, not fused; the coverage conditions of
tests/test_remap.py are asserted again on what the GPU returned."""
import ctypes as C

import numpy as np
import pytest

import esdf_ref as er
import mc_fields as mf
import parity_utils as pu
import remap_ref as rm
from mrhash_amd import capi, hipmem, synth
from test_remap import FIELDS, VAR_PARAMS, with_sumsq

pytestmark = pytest.mark.gpu

F = np.float32
VS = mf.PARAMS["virtual_voxel_size"]
K = synth.REPLICA_640
ZERO_T = np.zeros(3, F)


def _engine(blocks, params, num_sdf_blocks=4096, lib=None):
    e = pu.make_engine(lib or capi.load_hip(), synth.CFG1, params, num_sdf_blocks)
    if blocks:
        e.import_blocks(*er.to_import(blocks))
    return e


def _assert_records(got, want, what):
    gd, gv, info = got
    wd, wv, winfo = want
    assert gd.dtype == wd.dtype and gv.dtype == wv.dtype
    gk, wk = [list(zip(d["x"].tolist(), d["y"].tolist(), d["z"].tolist())) for d in (gd, wd)]
    assert gk == wk, f"{what}: {len(gk)} records vs {len(wk)}; only on the GPU {sorted(set(gk) - set(wk))[:5]}, only in the restatement {sorted(set(wk) - set(gk))[:5]}"
    assert rm.same_bits(gd, wd), f"{what}: descs differ"
    if not rm.same_bits(gv, wv):
        a, b = gv.reshape(-1).view(np.uint8).reshape(-1, 12), wv.reshape(-1).view(np.uint8).reshape(-1, 12)
        bad = np.flatnonzero(np.any(a != b, axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} voxels differ, first at record {bad[0] // 512} voxel {bad[0] % 512}: "
                             f"{gv.reshape(-1)[bad[:3]]} vs {wv.reshape(-1)[bad[:3]]}")
    assert info["records"] == len(wd) == winfo["records"] and info["valid_voxels"] == winfo["valid_voxels"] and info["source_blocks"] == winfo["source_blocks"]
    assert info["candidate_blocks"] >= info["records"]


class Field:
    """An engine on an imported map and the blocks it was built from."""

    def __init__(self, params, blocks, num_sdf_blocks=4096):
        self.params, self.blocks = params, blocks
        self.e = _engine(blocks, params, num_sdf_blocks)

    def check(self, R, t, what, vs_d=0.0, min_weight=0):
        want = rm.resample(self.params, self.blocks, R, t, vs_d, min_weight)
        got = self.e.resample_map(R, t, vs_d, min_weight)
        _assert_records(got, want, what)
        c = rm.counts(got[1])
        print(what, c, got[2])
        return c


@pytest.fixture(scope="module")
def dense():
    f = Field(*FIELDS["dense"]())
    yield f
    f.e.close()


@pytest.fixture(scope="module")
def holes():
    f = Field(*FIELDS["holes"]())
    yield f
    f.e.close()


# ---- 1. one field, four poses ----------------------------------------------------------------------------------------------------

def test_identity(dense):
    c = dense.check(rm.IDENTITY, ZERO_T, "identity")
    assert c["records"] == 64 and c["valid"] == 31 ** 3


def test_translation_by_whole_blocks(dense):
    t = (np.array([3, -2, 1], F) * F(8) * F(VS)).astype(F)
    assert dense.check(rm.IDENTITY, t, "aligned translation")["valid"] >= 20000


def test_fractional_translation(dense):
    c = dense.check(rm.IDENTITY, np.array([0.013, -0.027, 0.041], F), "fractional translation")
    assert c["valid"] >= 25000 and c["partial"] >= 30


def test_generic_pose(dense):
    c = dense.check(rm.GENERIC_R, rm.GENERIC_T, "generic pose")
    assert c["full"] >= 8 and c["partial"] >= 64


# ---- 2. holes, starved cells, absent blocks, min_weight --------------------------------------------------------------------------

@pytest.mark.parametrize("min_weight", [0, 3])
def test_holes_starved_cells_and_absent_blocks(holes, min_weight):
    c = holes.check(rm.GENERIC_R, rm.GENERIC_T, f"holes, min_weight {min_weight}", min_weight=min_weight)
    assert c["partial"] >= (64 if min_weight == 0 else 1) and c["valid"] > 0


# ---- 3. a variance-adaptive source -------------------------------------------------------------------------------------------------

def test_variance_adaptive_source():
    f = Field(*FIELDS["adaptive"]())
    try:
        d, _ = f.e.dump_blocks()
        assert 0 < int((d["resolution"] == 1).sum()) < len(d)
        assert f.check(rm.GENERIC_R, rm.GENERIC_T, "adaptive source")["valid"] > 1000
    finally:
        f.e.close()


# ---- 4. other voxel sizes: the table-only path and a footprint beyond 3^3 ------------------------------------------------------------

def test_coarser_destination(dense):
    c = dense.check(rm.GENERIC_R, rm.GENERIC_T, "vs_d = 2 vs_s", vs_d=float(F(F(VS) * F(2))))
    assert c["records"] >= 16


def test_finer_destination(dense):
    c = dense.check(rm.GENERIC_R, rm.GENERIC_T, "vs_d = vs_s / 2", vs_d=float(F(F(VS) * F(0.5))))
    assert c["full"] >= 100


# ---- 5. far from the origin and past the limits ----------------------------------------------------------------------------------

def _rungs(ks, extra=()):
    """The origin cluster and the rungs k of mc_fields.ladder(0.05), cell for cell (fill draws per block in sorted order, so the
    sub-ladder is built from the whole one), plus blocks `extra` with cells of their own."""
    blocks, p = mf.ladder(0.05)
    keep = set(mf.ORIGIN_CLUSTER)
    for k, _, coords in mf.ladder_rungs():
        if k in ks:
            keep |= set(coords)
    out = {b: v for b, v in blocks.items() if b in keep}
    if extra:
        out.update(mf.fill(list(extra), 17, holes=0.05, starved=0.2, params=p))
    return with_sumsq(out), p


def test_ladder_under_a_translation():
    """Blocks at +-2^k, k = 8 .. 16: where voxel -> block changes from the shift to the float detour."""
    blocks, p = _rungs(set(mf.LADDER_K))
    f = Field(p, blocks, 8192)
    try:
        c = f.check(rm.IDENTITY, np.array([0.013, -0.027, 0.041], F), "ladder")
        assert c["records"] >= len(blocks) and c["valid"] >= 150 * len(blocks)
    finally:
        f.e.close()


def test_past_the_position_bound():
    """|P_a| < 2^20 vs_s: a cluster that straddles x = 2^17 blocks.  The voxels beyond are invalid, the blocks beyond absent."""
    edge = 1 << 17
    extra = [(x, y, z) for x in range(edge - 3, edge + 2) for y in range(2) for z in range(2)]
    blocks, p = _rungs({16}, extra)
    f = Field(p, blocks)
    try:
        t = np.array([0.2, 0.0, -0.8], F)  # half a block along x: the bound cuts through the records of one block layer
        d, v, _ = got = f.e.resample_map(rm.IDENTITY, t)
        _assert_records(got, rm.resample(p, blocks, rm.IDENTITY, t), "past the P bound")
        far = d["x"] >= edge - 4
        assert far.sum() >= 8
        P = rm.source_positions(rm.IDENTITY, t, p["virtual_voxel_size"], (np.stack([d["x"], d["y"], d["z"]], -1).astype(np.int64)[:, None, :] * 8 + rm.LOCAL[None]).reshape(-1, 3))
        beyond = ~np.all(np.abs(P) < rm.bound(p["virtual_voxel_size"]), axis=-1)
        assert beyond.any() and not v.reshape(-1)[beyond].view(np.uint8).any()
        assert int(d["x"].max()) <= edge + 1 and (v["weight"][far] > 0).any()
    finally:
        f.e.close()


def test_past_the_key_range():
    """A translation that carries the rung at +2^16 blocks across block 2^20: the records end at the last packed key."""
    blocks, p = _rungs({16})
    f = Field(p, blocks)
    try:
        shift = (1 << 20) - (1 << 16)
        t = np.array([F(shift) * F(8) * F(p["virtual_voxel_size"]), 0, 0], F)
        d, v, _ = got = f.e.resample_map(rm.IDENTITY, t)
        _assert_records(got, rm.resample(p, blocks, rm.IDENTITY, t), "past the key range")
        assert int(d["x"].max()) == (1 << 20) - 1 and (d["x"] > (1 << 20) - 8).sum() >= 9
    finally:
        f.e.close()


# ---- 6. an analytic plane ----------------------------------------------------------------------------------------------------------

def test_plane_field():
    blocks = rm.plane_field(rm.PLANE_N, rm.PLANE_D, mf.PARAMS)
    f = Field(mf.PARAMS, blocks)
    try:
        f.check(rm.GENERIC_R, rm.GENERIC_T, "plane")
        d, v, _ = f.e.resample_map(rm.GENERIC_R, rm.GENERIC_T)
        err, tol, n = rm.plane_error(d, v, rm.GENERIC_R, rm.GENERIC_T, VS)
        print(f"plane: max error {err:.3e}, tolerance {tol:.3e}, {n} valid voxels")
        assert n >= 20000 and err <= tol
    finally:
        f.e.close()


# ---- 7. mrh_fuse_map ---------------------------------------------------------------------------------------------------------------

def _same_dump(a, b, what):
    (da, va), (db, vb) = a, b
    assert rm.same_bits(da, db), f"{what}: descs differ ({len(da)} vs {len(db)})"
    assert rm.same_bits(va, vb), f"{what}: voxels differ"


@pytest.mark.parametrize("adaptive", [False, True])
def test_fuse_map_equals_resample_and_unpack_and_the_oracle(dense, adaptive):
    params = VAR_PARAMS if adaptive else mf.PARAMS
    dst_blocks = with_sumsq(mf.sign_field(9, holes=0.05, starved=0.3, coarse=0.4 if adaptive else 0.0, base=(1, 0, -1), params=params), seed=6)
    a, b, o = _engine(dst_blocks, params), _engine(dst_blocks, params), _engine(dst_blocks, params, lib=pu.oracle_lib())
    try:
        before = a.dump_blocks()
        info = a.fuse_map(dense.e, rm.GENERIC_R, rm.GENERIC_T)
        ptr, n, rinfo = dense.e.resample_map_device(rm.GENERIC_R, rm.GENERIC_T)
        taken = b.unpack_blocks(capi.UNPACK_MERGE, ptr, n, True)
        wd, wv, _ = rm.resample(dense.params, dense.blocks, rm.GENERIC_R, rm.GENERIC_T)
        rec = rm.records(wd, wv)
        taken_o = o.unpack_blocks(capi.UNPACK_MERGE, rec.ctypes.data, len(rec), False)
        print("fuse", info, "taken", taken, taken_o)
        assert info["records"] == n == len(rec) and {k: info[k] for k in rinfo if k != "taken"} == {k: rinfo[k] for k in rinfo if k != "taken"}
        assert info["taken"] == taken == taken_o and 0 < taken <= n
        if adaptive:
            assert taken < n  # a fine record onto a coarse block is not taken
        after = a.dump_blocks()
        _same_dump(after, b.dump_blocks(), "fuse_map vs resample + unpack")
        _same_dump(after, o.dump_blocks(), "fuse_map vs the oracle's merge of the restatement's records")
        assert len(after[0]) > len(before[0])
    finally:
        a.close()
        b.close()
        o.close()


# ---- 8. the reader contract --------------------------------------------------------------------------------------------------------

def test_resample_and_fuse_leave_the_source_alone(dense):
    hip = capi.load_hip()
    params = dict(synth.REPLICA_PARAMS)
    frames = list(synth.replica_stream(8))
    a = pu.make_engine(hip, K, params, 65536)
    b = pu.make_engine(hip, K, params, 65536)
    dst = pu.make_engine(hip, K, params, 65536)
    try:
        for f in frames[:5]:
            pu.feed(a, f)
            pu.feed(b, f)
        d0, v0, info0 = a.resample_map(rm.GENERIC_R, rm.GENERIC_T)  # between two frames of the pipelined stream, no sync
        assert info0["records"] > 1000 and info0["source_blocks"] == len(b.dump_blocks()[0])
        _same_dump(a.dump_blocks(), b.dump_blocks(), "the source after resample_map")
        pts = (np.random.default_rng(3).uniform(-1.5, 1.5, (300, 3))).astype(F)
        for f in frames[5:]:
            pu.feed(a, f)
            a.resample_map_device(rm.GENERIC_R, rm.GENERIC_T)
            dst.fuse_map(a, rm.IDENTITY, ZERO_T)
            pu.feed(b, f)
        r = pu.compare_maps(a, b, tol=0.0)
        assert r["sdf_bit_exact"] and r["sumsq_bit_exact"]
        pu.compare_meshes(a, b, tol=0.0)
        # counters, the last extraction and the last query result survive the calls
        tris = a.extract_triangles()
        V, Fc, Cc = a.extract_mesh()
        p = capi.MrhQueryParams(capi.QUERY_FIELD_SMOOTH, 3)
        out = [C.c_void_p() for _ in range(4)]
        assert a.lib.mrh_query_points(a._ctx, C.byref(p), pts.ctypes.data, len(pts), None, None, *[C.byref(x) for x in out]) == capi.MRH_OK
        sizes = (4 * len(pts), 12 * len(pts), 4 * len(pts), len(pts))
        q0 = [C.string_at(x.value, s) for x, s in zip(out, sizes)]
        s0 = a.stats()
        d1, v1, _ = a.resample_map(rm.GENERIC_R, rm.GENERIC_T)
        info = dst.fuse_map(a, rm.GENERIC_R, rm.GENERIC_T, min_weight=2)
        assert 0 < info["taken"] <= info["records"]
        s1 = a.stats()
        assert [C.string_at(x.value, s) for x, s in zip(out, sizes)] == q0
        V2, F2, C2 = a.extract_mesh()
        assert er.same_bits(V, V2) and np.array_equal(Fc, F2) and er.same_bits(Cc, C2)
        assert er.same_bits(a.extract_triangles(), tris)
        for name, _ in capi.MrhStats._fields_:
            if "ms" not in name:
                assert getattr(s0, name) == getattr(s1, name), name
        assert len(d1) > len(d0)
        pu.feed(a, frames[-1])  # the camera and the pose are still the stream's: the same frame again lands on the same blocks
        pu.feed(b, frames[-1])
        assert pu.compare_maps(a, b, tol=0.0)["sdf_bit_exact"]
    finally:
        a.close()
        b.close()
        dst.close()


# ---- 9. arguments, an empty source, the facade -----------------------------------------------------------------------------------

def test_arguments_and_unsupported_contexts(dense):
    e = dense.e
    lib = e.lib
    Fp = C.POINTER(C.c_float)
    R, t = rm.GENERIC_R.reshape(9).copy(), rm.GENERIC_T.copy()
    pR, pt = R.ctypes.data_as(Fp), t.ctypes.data_as(Fp)
    ptr, n, info = C.c_void_p(), C.c_uint64(), capi.MrhRemapInfo()
    ok = capi.MrhRemapParams(0.0, 0)
    other = _engine({}, mf.PARAMS)
    try:
        def resample(p=ok, pR=pR, pt=pt, ptr=C.byref(ptr), n=C.byref(n)):
            return lib.mrh_resample_map(e._ctx, C.byref(p) if p is not None else None, pR, pt, ptr, n, C.byref(info))

        assert resample() == capi.MRH_OK and n.value == 130
        assert lib.mrh_resample_map(e._ctx, C.byref(ok), pR, pt, C.byref(ptr), C.byref(n), None) == capi.MRH_OK  # the info is optional
        for kw in (dict(p=None), dict(pR=None), dict(pt=None), dict(ptr=None), dict(n=None)):
            assert resample(**kw) == capi.MRH_ERR_INVALID_ARG, kw
            assert b"null argument" in lib.mrh_last_error(e._ctx)
        assert lib.mrh_resample_map(None, C.byref(ok), pR, pt, C.byref(ptr), C.byref(n), None) == capi.MRH_ERR_INVALID_ARG
        assert lib.mrh_fuse_map(None, e._ctx, C.byref(ok), pR, pt, None) == capi.MRH_ERR_INVALID_ARG
        assert lib.mrh_fuse_map(other._ctx, None, C.byref(ok), pR, pt, None) == capi.MRH_ERR_INVALID_ARG
        bad = [capi.MrhRemapParams(0.0, 0, (C.c_uint32 * 2)(1, 0)), capi.MrhRemapParams(0.0, 0, (C.c_uint32 * 2)(0, 7)), capi.MrhRemapParams(0.0, 256),
               capi.MrhRemapParams(float(F(VS) * F(4.01)), 0), capi.MrhRemapParams(float(F(VS) * F(0.249)), 0), capi.MrhRemapParams(-1.0, 0)]
        for p in bad:
            assert resample(p=p) == capi.MRH_ERR_INVALID_ARG
            assert lib.mrh_fuse_map(other._ctx, e._ctx, C.byref(p), pR, pt, None) == capi.MRH_ERR_INVALID_ARG
        for i in range(12):
            R2, t2 = R.copy(), t.copy()
            (R2 if i < 9 else t2)[i % 9 if i < 9 else i - 9] = [np.nan, np.inf, -np.inf][i % 3]
            assert resample(pR=R2.ctypes.data_as(Fp), pt=t2.ctypes.data_as(Fp)) == capi.MRH_ERR_INVALID_ARG
            assert b"not finite" in lib.mrh_last_error(e._ctx)
        S = (np.eye(3, dtype=F) * F(1.5)).reshape(9)
        assert resample(pR=S.ctypes.data_as(Fp)) == capi.MRH_ERR_INVALID_ARG and b"not a rotation" in lib.mrh_last_error(e._ctx)
        assert lib.mrh_fuse_map(e._ctx, e._ctx, C.byref(ok), pR, pt, None) == capi.MRH_ERR_INVALID_ARG and b"the destination is the source" in lib.mrh_last_error(e._ctx)
        contradict = capi.MrhRemapParams(float(F(VS) * F(2)), 0)
        assert lib.mrh_fuse_map(other._ctx, e._ctx, C.byref(contradict), pR, pt, None) == capi.MRH_ERR_INVALID_ARG and b"contradicts" in lib.mrh_last_error(other._ctx)
        agree = capi.MrhRemapParams(float(F(VS)), 0)
        assert lib.mrh_fuse_map(other._ctx, e._ctx, C.byref(agree), pR, pt, C.byref(info)) == capi.MRH_OK and info.taken == info.records == 130
        wide = _engine({}, dict(mf.PARAMS, virtual_voxel_size=0.25, sdf_truncation=0.75))
        try:
            with pytest.raises(capi.MrhError) as ei:
                wide.fuse_map(e, rm.GENERIC_R, rm.GENERIC_T)  # ratio 5
            assert ei.value.code == capi.MRH_ERR_INVALID_ARG and "ratio" in str(ei.value)
        finally:
            wide.close()
        assert rm.same_bits(e.dump_blocks()[0], er.to_import(dense.blocks)[0])  # none of the refusals touched the source
        # an empty source: success, nothing to hand out
        empty = _engine({}, mf.PARAMS)
        try:
            ptr.value, n.value = 1, 99
            assert lib.mrh_resample_map(empty._ctx, C.byref(ok), pR, pt, C.byref(ptr), C.byref(n), C.byref(info)) == capi.MRH_OK
            assert ptr.value is None and n.value == 0 and info.source_blocks == 0 and info.records == 0
            d, v, i2 = empty.resample_map(rm.GENERIC_R, rm.GENERIC_T)
            assert d.shape == (0,) and v.shape == (0, 512) and d.dtype == capi.DESC_DTYPE and v.dtype == capi.VOXEL_DTYPE
            before = other.dump_blocks()
            assert other.fuse_map(empty, rm.GENERIC_R, rm.GENERIC_T) == dict(source_blocks=0, candidate_blocks=0, records=0, valid_voxels=0, taken=0)
            _same_dump(other.dump_blocks(), before, "an empty source leaves the destination alone")
        finally:
            empty.close()
        # sharded contexts, either side
        s = capi.Engine(capi.load_hip(), capi.Params(num_sdf_blocks=4096, shard_rank=0, shard_count=2, **mf.PARAMS))
        try:
            for call in (lambda: s.resample_map(rm.GENERIC_R, rm.GENERIC_T), lambda: s.fuse_map(e, rm.GENERIC_R, rm.GENERIC_T), lambda: other.fuse_map(s, rm.GENERIC_R, rm.GENERIC_T)):
                with pytest.raises(capi.MrhError) as ei:
                    call()
                assert ei.value.code == capi.MRH_ERR_UNSUPPORTED
        finally:
            s.close()
    finally:
        other.close()


def test_device_variant_points_at_the_records(dense):
    want = rm.resample(dense.params, dense.blocks, rm.GENERIC_R, rm.GENERIC_T, 0.0, 2)
    ptr, n, info = dense.e.resample_map_device(rm.GENERIC_R, rm.GENERIC_T, min_weight=2)
    assert ptr and n == len(want[0]) == info["records"]
    rec = np.frombuffer(hipmem.read(ptr, n * capi.RECORD_BYTES), capi.RECORD_DTYPE)
    assert rm.same_bits(rec, rm.records(want[0], want[1]))
    # the buffer is the context's until the next call: a second, smaller result reuses it
    ptr2, n2, _ = dense.e.resample_map_device(rm.IDENTITY, ZERO_T)
    assert ptr2 == ptr and n2 == 64


def test_geowrapper_fuse_map(monkeypatch):
    """The facade on two spheres fused from depth frames (it has no block import): B into A under a pose given as setCurrPose
    takes it, against Engine.fuse_map on twin engines fed the same frames."""
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
        q = np.array([0.05, -0.08, 0.03, 1.0])
        q = (q / np.linalg.norm(q)).astype(F)
        t = np.array([0.02, -0.01, 0.03], F)
        gb.setCurrPose(t, q)
        pose = gb.getCurrPose()  # the matrix the facade makes of (t, q)
        gb.setCurrPose(f.t, f.q)
        info = ga.fuseMap(gb, t, q)
        want = ea.fuse_map(eb, pose[:3, :3].copy(), pose[:3, 3].copy())
        assert info == want and info["taken"] == info["records"] > 50
        with pytest.raises(RuntimeError, match=r"GeoWrapper::fuseMap\|"):
            ga.fuseMap(gb, np.zeros(2, F), q)
        with pytest.raises(RuntimeError):
            ga.fuseMap(ga, t, q)  # dst == src
        world = np.random.default_rng(9).uniform([-0.31, -0.294, 0.805], [0.305, 0.31, 1.295], (400, 3)).astype(F)
        got, twin = ga.queryPoints(world, smooth=True), ea.query(world, smooth=True)  # the two maps after the fuse
        for x, y in zip(got, twin):
            assert rm.same_bits(x, y)
        assert np.mean((got[3] & capi.QUERY_DIST) != 0) >= 0.2
    finally:
        ea.close()
        eb.close()
        del ga, gb
