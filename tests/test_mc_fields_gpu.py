"""Marching cubes on the hand-built maps of tests/mc_fields.py: the HIP library against the oracle through the same capi.Engine,
BYTE for byte — the soup (positions and colours), triangle_blocks() (descriptors and counts) and V / F / C of extract_mesh().
The arithmetic spec is shared, so there is no tolerance, no masking of near-ties and no skipped block.

Every map is imported into both engines and extracted TWICE on the HIP side.  The first extraction finds the default record
buffer (128 records a block) too small on the dense maps and emits through k_mc<emit>; the buffer then grows to the demand and the
second extraction emits through k_mc_emit_records.  Where `dense` is set the test shows the overflow from triangle_blocks().

Both engines get a camera (pu.make_engine): without one sdf_bound is 0 and the sign prescreen silently does nothing.
tests/test_mc_fields.py pins the oracle on the same maps (all 256 cube cases, the independent restatement)."""
import numpy as np
import pytest

import mc_fields as mf
import parity_utils as pu
from mrhash_amd import capi, synth

pytestmark = pytest.mark.gpu

T = mf.PARAMS["sdf_truncation"]
MULTI = dict(sdf_var_threshold=0.5)
NEGATIVE = (-9, -11, -13)
SWITCHES = ("MRH_MC_NO_PRESCREEN", "MRH_MC_NO_RECORDS", "MRH_MC_NO_COARSE_KNOWN", "MRH_MC_RECORDS_PER_BLOCK", "MRH_MC_RADIX_SORT")


def _engine(lib, blocks, params, num_sdf_blocks=4096):
    e = pu.make_engine(lib, synth.CFG1, params, num_sdf_blocks)
    # the camera is set: a frame is refused for its missing images, not for a missing camera (both before the device is touched)
    with pytest.raises(capi.MrhError, match="images are required"):
        e.integrate()
    e.import_blocks(*mf.to_import(blocks))
    return e


def _outputs(e):
    tris = e.extract_triangles()
    td, tc = e.triangle_blocks()
    V, Fi, C = e.extract_mesh()
    return dict(p=tris["p"], c=tris["c"], descs=td, counts=tc, V=V, F=Fi, C=C)


def _assert_same(got, want, what):
    for k in ("descs", "counts", "p", "c", "V", "F", "C"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape, f"{what}: {k} has shape {a.shape}, expected {b.shape}"
        if a.tobytes() != b.tobytes():
            diff = a.reshape(-1).view(np.uint8).reshape(len(a), -1) != b.reshape(-1).view(np.uint8).reshape(len(b), -1)
            rows = np.flatnonzero(diff.any(1))
            raise AssertionError(f"{what}: {k} differs in {len(rows)} of {len(a)} rows ({int(diff.sum())} bytes), first rows {rows[:6].tolist()}:\n"
                                 f"{a[rows[:3]]}\nexpected\n{b[rows[:3]]}")


def _oracle_outputs(oracle, blocks, params):
    b = _engine(oracle, blocks, params)
    want = _outputs(b)
    b.close()
    return want


def check(hip, oracle, monkeypatch, blocks, params, dense=False, least=0, want=None):
    """Two extractions of the HIP library and a third without the prescreen, each against the oracle's one."""
    want = want or _oracle_outputs(oracle, blocks, params)
    n_tris = len(want["p"])
    print(f"{len(blocks)} blocks, {n_tris} triangles, busiest block {int(want['counts'].max()) if len(want['counts']) else 0}, "
          f"{len(want['V'])} vertices, {len(want['F'])} faces")
    assert n_tris >= least and len(want["descs"]) == len(blocks)
    if dense:
        # > 5 * 128 triangles in one block: more than 128 of its voxels bear triangles, each of them a candidate with a record.
        # And since these fields have both signs (or an "anything else" cell) in every window, every voxel is a candidate: the
        # demand is 512 records a block against a buffer of 128 a block.
        assert int(want["counts"].max()) > 5 * 128
    a = _engine(hip, blocks, params)
    try:
        _assert_same(_outputs(a), want, "first extraction (k_mc<emit> where the records overflow)")
        _assert_same(_outputs(a), want, "second extraction (k_mc_emit_records)")
        monkeypatch.setenv("MRH_MC_NO_PRESCREEN", "1")
        _assert_same(_outputs(a), want, "without the prescreen")
    except capi.MrhError as err:
        # an error return of the device path on these inputs: nothing more is started on a device that may have faulted
        pytest.exit(f"HIP library error on a hand-built map, session ended: {err}", returncode=3)
    finally:
        monkeypatch.delenv("MRH_MC_NO_PRESCREEN", raising=False)
    a.close()
    return want


# ---- every cube case ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("base", [(0, 0, 0), NEGATIVE], ids=["origin", "negative"])
@pytest.mark.parametrize("phase", mf.GALLERY_PHASES)
def test_case_gallery(hip, oracle, monkeypatch, phase, base):
    """All 256 rows of d_mc_tri through the 8-lane evaluation and mc_emit_vertices, sites inside blocks and across their faces,
    edges and corners (tests/test_mc_fields.py shows that every case is there)."""
    blocks, _ = mf.case_gallery(phase, base)
    check(hip, oracle, monkeypatch, blocks, mf.PARAMS, least=23000)


# ---- random signed cells ----------------------------------------------------------------------------------------------------------

# A covering subset of holes {0, 0.05, 0.3} x absent {0, 0.3} x min_weight_threshold {0, 1, 3} x marching_cubes_threshold {1.5, 0.8 T}
# x sdf_truncation_scale {0, 0.01} x vertices_merging_threshold {0, 0.013}: every value of every factor, and every pair of values of
# holes / min_weight / threshold / scale, occurs.  (holes, absent, min_weight, mc_threshold, scale, merge); a third of the holes starved.
SIGN_FIELD_CASES = [
    (0.0, 0.0, 1, 1.5, 0.0, 0.0),
    (0.05, 0.0, 1, 1.5, 0.0, 0.0),
    (0.3, 0.3, 1, 1.5, 0.0, 0.0),
    (0.05, 0.3, 0, 1.5, 0.0, 0.013),
    (0.3, 0.0, 0, 0.8 * T, 0.01, 0.0),
    (0.0, 0.3, 3, 0.8 * T, 0.0, 0.013),
    (0.05, 0.0, 3, 1.5, 0.01, 0.013),
    (0.3, 0.3, 3, 1.5, 0.01, 0.0),
    (0.0, 0.0, 0, 1.5, 0.01, 0.013),
    (0.05, 0.3, 1, 0.8 * T, 0.01, 0.0),
    (0.3, 0.0, 1, 0.8 * T, 0.0, 0.013),
    (0.0, 0.3, 1, 1.5, 0.01, 0.0),
    (0.05, 0.0, 0, 0.8 * T, 0.0, 0.0),
]


def _sign_params(min_w, thr, scale, merge, **extra):
    return dict(mf.PARAMS, min_weight_threshold=min_w, marching_cubes_threshold=thr, sdf_truncation_scale=scale, vertices_merging_threshold=merge, **extra)


@pytest.mark.parametrize("holes,absent,min_w,thr,scale,merge", SIGN_FIELD_CASES)
def test_sign_field(hip, oracle, monkeypatch, holes, absent, min_w, thr, scale, merge):
    p = _sign_params(min_w, thr, scale, merge)
    i = SIGN_FIELD_CASES.index((holes, absent, min_w, thr, scale, merge))
    blocks = mf.sign_field(100 + i, holes=holes, starved=0.3, absent=absent, base=(-2, -1, -3) if i % 2 else (0, 0, 0), params=p)
    check(hip, oracle, monkeypatch, blocks, p, dense=holes <= 0.05 and absent == 0.0 and thr == 1.5 and min_w <= 1, least=30)


@pytest.mark.parametrize("coarse,holes,scale,merge", [(0.1, 0.05, 0.0, 0.0), (0.5, 0.05, 0.0, 0.013), (0.9, 0.05, 0.0, 0.0), (0.5, 0.3, 0.01, 0.0)])
def test_sign_field_multiresolution(hip, oracle, monkeypatch, coarse, holes, scale, merge):
    """Coarse and fine blocks side by side: the wide window, checkVertexVoxels, the coarser re-sample, both known-stencil forms."""
    p = _sign_params(1, 1.5, scale, merge, **MULTI)
    blocks = mf.sign_field(int(200 + 10 * coarse), holes=holes, starved=0.5, coarse=coarse, base=(-2, -2, -2), params=p)
    n_coarse = sum(isinstance(v, tuple) for v in blocks.values())
    assert 0 < n_coarse < len(blocks)
    check(hip, oracle, monkeypatch, blocks, p, dense=coarse <= 0.5 and holes <= 0.05, least=1000)


@pytest.mark.parametrize("coarse,merge", [(0.0, 0.0), (0.0, 0.013), (0.4, 0.0)])
def test_snapped_vertices(hip, oracle, monkeypatch, coarse, merge):
    """A quarter of the cells exactly +-0 and a fifth without weight: corners fall back to raw samples that are exactly 0, vertexInterp
    snaps their vertices onto cube corners (|d| < 1e-5) — bit-identical vertices from many voxels and degenerate triangles, which
    the device post-process (the min-index hash of the per-tile de-duplication) must merge and drop exactly as the oracle does."""
    p = _sign_params(1, 1.5, 0.0, merge, **(MULTI if coarse else {}))
    blocks = mf.sign_field(500, holes=0.2, starved=0.3, coarse=coarse, base=(-2, -2, -1), params=p, zeros=0.2)
    want = check(hip, oracle, monkeypatch, blocks, p, least=5000)
    degenerate = len(want["p"]) - len(want["F"])
    shared = 3 * len(want["F"]) / max(1, len(want["V"]))
    print(f"{degenerate} triangles dropped by the post-process, {shared:.2f} face corners per vertex")
    assert degenerate > 500


# ---- the prescreen's fields --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coarse,absent,base,extra", [
    (0.0, 0.0, (0, 0, 0), {}),
    (0.0, 0.2, NEGATIVE, dict(sdf_truncation_scale=0.01)),
    (0.0, 0.0, (-3, -3, -3), dict(min_weight_threshold=3)),
    (0.0, 0.0, (-3, -3, -3), dict(min_weight_threshold=0)),
    (0.3, 0.0, (0, 0, 0), {}),
    (0.7, 0.2, NEGATIVE, {}),
    (0.5, 0.0, (-3, -3, -3), dict(sdf_truncation_scale=0.01)),
    (0.5, 0.1, (-3, -3, -3), dict(min_weight_threshold=3, marching_cubes_threshold=0.8 * T)),
])
def test_sparse_field(hip, oracle, monkeypatch, coarse, absent, base, extra):
    """A clearly positive sea with 6 % odd cells: the prescreen drops about a fifth of the voxels (0.94^27) and must drop none
    that a single odd cell — at any place of the 3^3 or 7^3 window, in this block or a neighbour — gives a triangle; check() also
    extracts with the prescreen off."""
    p = dict(mf.PARAMS, **extra, **(MULTI if coarse else {}))
    blocks = mf.sparse_field(int(300 + 10 * coarse + len(extra)), odd=0.06, absent=absent, coarse=coarse, base=base, dims=(5, 5, 5), params=p)
    check(hip, oracle, monkeypatch, blocks, p, least=300)


@pytest.mark.parametrize("coarse,odd,scale", [(0.3, 0.05, 0.0), (0.5, 0.1, 0.01), (0.8, 0.1, 0.0)])
def test_starved_cells_next_to_coarse_blocks(hip, oracle, monkeypatch, coarse, odd, scale):
    """No weighted cell of this map is negative: every triangle comes from a coarser re-sample that blended a starved cell's large
    negative sdf with a small positive one (vds.cu:296-309) — the wide window's class-16 rule must keep all of those voxels."""
    p = dict(mf.PARAMS, sdf_truncation_scale=scale, **MULTI)
    blocks = mf.sparse_field(int(350 + 10 * coarse), odd=odd, coarse=coarse, base=(-3, -2, -3), dims=(5, 5, 5), params=p, starved_only=True)
    v = np.concatenate([b[1] if isinstance(b, tuple) else b for b in blocks.values()])
    assert not np.any((v["weight"] > 0) & (v["sdf"] < 0)) and np.any((v["weight"] == 0) & (v["sdf"] < 0))
    check(hip, oracle, monkeypatch, blocks, p, least=1000)


@pytest.mark.parametrize("coarse_neighbour", [False, True], ids=["single", "coarse-neighbour"])
@pytest.mark.parametrize("kind", mf.ODD_KINDS)
def test_odd_cell(hip, oracle, monkeypatch, kind, coarse_neighbour):
    """One odd cell in a +T sea at block corners, edges, faces and depths.  One such cell cannot turn a trilinear corner value
    (7/8 T - 1/8 T > 0), so both sides must answer with an EMPTY mesh, with and without the prescreen; test_sparse_field is the
    case where triangles depend on single cells."""
    p = dict(mf.PARAMS, **(MULTI if coarse_neighbour else {}))
    blocks, _ = mf.odd_cell(kind, base=(-40, -1, -2), coarse_neighbour=coarse_neighbour, params=p)
    check(hip, oracle, monkeypatch, blocks, p)


@pytest.mark.parametrize("centre,other", mf.NEIGHBOUR_PAIRS)
def test_neighbour_gallery(hip, oracle, monkeypatch, centre, other):
    """A fine / coarse / absent block in each of the 26 neighbour positions: voxel_touches_coarse, coarse_voxel_in_coarse_cells,
    the three staging segments and the rim cells of every neighbour."""
    p = dict(mf.PARAMS, **MULTI)
    blocks, _ = mf.neighbour_gallery(centre, other, base=(-12, -7, -1), params=p)
    check(hip, oracle, monkeypatch, blocks, p, dense=centre == "fine", least=50000)


# ---- far from the origin -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coarse", [0.0, 0.4], ids=["single", "coarse0.4"])
@pytest.mark.parametrize("vs", [0.05, 0.0625])
def test_ladder(hip, oracle, monkeypatch, vs, coarse):
    """Blocks at +-2^k, k = 8 .. 16: some rung straddles `staged` ((amax + 3) * 8 < block_shift_limit) whatever the limit of a
    0.05 m voxel is, and rung 15 straddles the known-stencil bound (amax + 2) * 8 < 2^18 at 2^-4 m while still staged.  The float
    position -> voxel conversions round differently out there; the integer stencils must land on the same cells."""
    blocks, p = mf.ladder(vs, coarse=coarse)
    p = dict(p, **(MULTI if coarse else {}))
    check(hip, oracle, monkeypatch, blocks, p, dense=coarse == 0.0, least=300000)


# ---- every switch on its own ---------------------------------------------------------------------------------------------------------

def _switch_map(multi):
    p = dict(mf.PARAMS, **(MULTI if multi else {}))
    blocks = mf.sign_field(400 + multi, holes=0.05, starved=0.3, coarse=0.2 if multi else 0.0, base=(-2, -2, -2), params=p)
    blocks.update(mf.sparse_field(410 + multi, odd=0.06, coarse=0.4 if multi else 0.0, base=(4, -2, -2), dims=(3, 4, 4), params=p))  # 2 absent blocks apart
    return blocks, p


@pytest.fixture(scope="module")
def switch_reference(oracle):
    out = {}
    for multi in (0, 1):
        blocks, p = _switch_map(multi)
        out[multi] = (blocks, p, _oracle_outputs(oracle, blocks, p))
    return out


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("multi", [0, 1], ids=["single", "multi"])
def test_switches_change_nothing(hip, oracle, monkeypatch, switch_reference, multi, switch):
    """A fresh context under one switch (two-pass emit only, no prescreen, literal coarse voxels, a one-record-a-block buffer,
    the radix sort): the oracle's bytes on both extractions.  The map is a dense sign field and a sparse field side by side."""
    blocks, p, want = switch_reference[multi]
    monkeypatch.setenv(switch, "1")
    check(hip, oracle, monkeypatch, blocks, p, dense=True, least=20000, want=want)
