"""The hand-built extraction maps of tests/mc_fields.py on the CPU: the oracle produces every one of the 256 cube cases where the
gallery builds it, agrees bit for bit with the independent restatement (tests/independent.py) on blocks of each kind of map,
and the builders build what their names say.  tests/test_mc_fields_gpu.py then compares the HIP library with the oracle."""
import os
import re
import time

import numpy as np
import pytest

import independent as ind
import mc_fields as mf
import parity_utils as pu
from mrhash_amd import synth

F = np.float32
MULTI = dict(sdf_var_threshold=0.5)


def tri_table():
    txt = open(os.path.join(pu.ROOT, "include", "mrh_mc_tables.h")).read()
    rows = re.findall(r"\{((?:0x[0-9A-Fa-f]{2},?){16})\}", txt)
    table = [[int(x, 16) for x in r.split(",") if x] for r in rows[:256]]
    assert len(table) == 256 and table[0][0] == 0 and table[255][0] == 0
    return table


def extract(lib, blocks, params, num_sdf_blocks=4096):
    """(soup, block descriptors, per-block counts) of the map through the library's own import + extraction."""
    e = pu.make_engine(lib, synth.CFG1, params, num_sdf_blocks)
    e.import_blocks(*mf.to_import(blocks))
    tris = e.extract_triangles()
    td, tc = e.triangle_blocks()
    e.close()
    return tris, td, tc


# ---- the coverage claim: all 256 cases, exactly ------------------------------------------------------------------------------

@pytest.mark.parametrize("base", [(0, 0, 0), (-9, -11, -13)], ids=["origin", "negative"])
@pytest.mark.parametrize("phase", mf.GALLERY_PHASES)
def test_gallery_holds_every_cube_case(oracle, phase, base):
    """Triangles binned by the voxel nearest to their centroid: the site built for cube index c holds exactly d_mc_tri[c][0] of
    them, for all 256 c.  (A triangle's vertices lie on edges of its voxel's cube and never all on one face, so its centroid is
    strictly inside the cube: nearest voxel == emitting voxel, up to 1e-6 voxel of rounding against a margin of 1/6.)"""
    table = tri_table()
    blocks, sites = mf.case_gallery(phase, base)
    assert sorted(c for _, c in sites) == list(range(256)) and len({v for v, _ in sites}) == 256
    tris, _, _ = extract(oracle, blocks, mf.PARAMS)
    vox = np.rint(tris["p"].astype(np.float64).mean(1) / float(F(mf.PARAMS["virtual_voxel_size"]))).astype(np.int64)
    keys, counts = np.unique(vox, axis=0, return_counts=True)
    held = {tuple(int(a) for a in k): int(n) for k, n in zip(keys, counts)}
    wrong = [(v, c, table[c][0], held.get(v, 0)) for v, c in sites if held.get(v, 0) != table[c][0]]
    assert not wrong, wrong[:8]
    assert sum(table[c][0] for c in range(256)) == sum(held.get(v, 0) for v, _ in sites) > 700


# ---- oracle vs the independent restatement ------------------------------------------------------------------------------------

def _walk(m, table, key, res):
    side, sc = (8, 1) if res == 0 else (4, 2)
    got = []
    for li in range(side ** 3):
        pi = np.array([key[0] * 8 + sc * (li % side), key[1] * 8 + sc * ((li % (side * side)) // side), key[2] * 8 + sc * (li // (side * side))], np.int32)
        pf = ind.voxel_to_world(m.vs, pi)
        got.extend(ind.mc_voxel(m, table, (pf[0], pf[1], pf[2])))
    gp = np.array([[vert[0] for vert in tri] for tri in got], F).reshape(-1, 3, 3)
    gc = np.array([[vert[1] for vert in tri] for tri in got], F).reshape(-1, 3, 3)
    return gp, gc


def _compare_blocks(oracle, blocks, params, pick, least=1):
    """Oracle soup of the picked blocks against the python walk over the same voxels: positions and colours bit-equal.
    pick(keys in canonical order, counts, blocks) -> indices."""
    tris, td, tc = extract(oracle, blocks, params)
    multi = params.get("sdf_var_threshold", 0) > 0
    if multi:
        m = ind.MultiMap(params, {k: (v if isinstance(v, tuple) else (0, v)) for k, v in blocks.items()})
    else:
        m = ind.Map(params, blocks)
    table = tri_table()
    keys = [(int(td["x"][i]), int(td["y"][i]), int(td["z"][i])) for i in range(len(td))]
    assert keys == sorted(blocks)
    starts = np.concatenate([[0], np.cumsum(tc.astype(np.int64))])
    checked = 0
    for bi in pick(keys, tc.astype(np.int64), blocks):
        key = keys[bi]
        res = int(td["resolution"][bi])
        assert res == (1 if isinstance(blocks[key], tuple) else 0)
        want = tris[starts[bi]: starts[bi + 1]]
        gp, gc = _walk(m, table, key, res)
        assert len(gp) == len(want) >= least, (key, res, len(gp), len(want))
        assert np.array_equal(gp.view(np.uint32), want["p"].view(np.uint32)), (key, res)
        assert np.array_equal(gc.view(np.uint32), want["c"].view(np.uint32)), (key, res)
        checked += len(want)
    return checked


def _busiest(n):
    return lambda keys, tc, blocks: list(np.argsort(-tc, kind="stable")[:n])


def _is_coarse(blocks, k):
    return isinstance(blocks.get(k), tuple)


def _fine_next_to_coarse_and_coarse(keys, tc, blocks):
    """The busiest fine block with a coarse neighbour and the busiest coarse block."""
    order = np.argsort(-tc, kind="stable")
    fine = next(i for i in order if not _is_coarse(blocks, keys[i])
                and any(_is_coarse(blocks, (keys[i][0] + d[0], keys[i][1] + d[1], keys[i][2] + d[2])) for d in mf.DIRS26))
    coarse = next(i for i in order if _is_coarse(blocks, keys[i]))
    return [fine, coarse]


def test_oracle_matches_the_independent_restatement_on_the_hand_built_maps(oracle):
    """Eleven blocks, voxel by voxel in python (the walk is slow, about 1 s a block: the time is printed): a gallery block
    whose sites cross its faces, the two busiest blocks of a sign field with holes, a sparse field (the raw-sample fallback decides
    signs there), a fine block next to a coarse one and a coarse block of two multi-resolution fields, and — at a 2^-4 m voxel —
    the blocks of ladder rung 15 on either side of the known-stencil bound, whose positions round differently from the origin's."""
    t0 = time.time()
    n = 0
    blocks, _ = mf.case_gallery(2)
    n += _compare_blocks(oracle, blocks, mf.PARAMS, lambda keys, tc, b: [keys.index((2, 2, 2))], least=100)
    n += _compare_blocks(oracle, mf.sign_field(2, holes=0.05, starved=0.3), mf.PARAMS, _busiest(2), least=500)
    n += _compare_blocks(oracle, mf.sparse_field(5, odd=0.03), mf.PARAMS, _busiest(2), least=10)
    pm = dict(mf.PARAMS, **MULTI)
    n += _compare_blocks(oracle, mf.sign_field(4, holes=0.05, starved=0.3, coarse=0.5), pm, _fine_next_to_coarse_and_coarse, least=50)
    n += _compare_blocks(oracle, mf.sparse_field(6, odd=0.05, coarse=0.5), pm, _fine_next_to_coarse_and_coarse)
    blocks, p = mf.ladder(0.0625)
    k15 = [c for k, side, c in mf.ladder_rungs() if k == 15 and side == 1][0]
    rung = {b: blocks[b] for b in k15 if b in blocks}  # the whole rung (the walk reads the neighbours); two blocks of its middle row
    x_known, x_literal = (1 << 15) - 3, (1 << 15) - 2  # (amax + 2) * 8 < 2^18  <=>  amax < 2^15 - 2
    y, z = k15[0][1] + 1, k15[0][2] + 1
    n += _compare_blocks(oracle, rung, p, lambda keys, tc, b: [keys.index((x_known, y, z)), keys.index((x_literal, y, z))], least=200)
    dt = time.time() - t0
    print("independent walk: %d triangles compared in %.1f s" % (n, dt))
    assert n > 3000


# ---- the builders build what they say ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [0.0, 0.01])
def test_magnitudes_bracket_the_float32_thresholds(scale):
    p = dict(mf.PARAMS, sdf_truncation_scale=scale)
    bound, lo, hi = mf.thresholds(p)
    assert bound.dtype == lo.dtype == hi.dtype == F
    assert float(bound) == pytest.approx(0.15 + scale * 30.0, rel=1e-6)
    assert mf.prevfloat(lo) < lo < mf.nextfloat(lo) and mf.prevfloat(hi) < hi < mf.nextfloat(hi)
    assert F(F(1e-3) * bound) == lo and F(F(1.001) * bound) == hi
    m = mf.magnitudes(p)
    assert m.dtype == F and np.all(np.isfinite(m)) and np.all(m > 0)
    clearly = (m >= lo) & (m <= hi)  # the kernel's test
    assert list(clearly[:3]) == [False, False, True] and list(clearly[6:8]) == [True, False]
    assert {float(lo), float(hi), float(mf.prevfloat(lo)), float(mf.nextfloat(hi))} <= set(float(x) for x in m)


def _all_voxels(blocks):
    return np.concatenate([v[1] if isinstance(v, tuple) else v for v in blocks.values()])


def test_fields_are_finite_deterministic_and_varied():
    a = mf.sign_field(7, holes=0.3, starved=0.5, absent=0.3, coarse=0.4, base=(-2, 3, -1))
    b = mf.sign_field(7, holes=0.3, starved=0.5, absent=0.3, coarse=0.4, base=(-2, 3, -1))
    assert sorted(a) == sorted(b) and all(np.array_equal(_all_voxels({k: a[k]}), _all_voxels({k: b[k]})) for k in a)
    assert 20 < len(a) < 60 and 5 < sum(isinstance(v, tuple) for v in a.values()) < len(a) - 5
    assert all(len(v[1]) == 64 and v[0] == 1 for v in a.values() if isinstance(v, tuple))
    v = _all_voxels(a)
    bits = v["sdf"].view(np.uint32)
    assert np.all(np.isfinite(v["sdf"]))
    hole = v["weight"] == 0
    assert 0.25 < hole.mean() < 0.35 and set(np.unique(v["weight"][~hole])) == {1, 2, 3, 4}
    assert np.any(hole & (bits == 0)) and np.any(hole & (bits == 0x80000000)) and np.any(hole & ((bits & 0x7FFFFFFF) != 0))  # +0, -0, starved
    assert np.any(~hole & (bits == 0)) and np.any(~hole & (bits == 0x80000000))
    assert set(np.abs(v["sdf"][~hole & ((bits & 0x7FFFFFFF) != 0)]).tolist()) == set(mf.magnitudes().tolist())
    assert len(np.unique(v["rgb"], axis=0)) > 1000
    for blocks in (mf.sparse_field(1, coarse=0.3), mf.odd_cell("starved", coarse_neighbour=True)[0], mf.neighbour_gallery("coarse", "fine")[0],
                   mf.ladder(0.05, coarse=0.4)[0], mf.case_gallery(3, (-9, -11, -13))[0]):
        v = _all_voxels(blocks)
        assert np.all(np.isfinite(v["sdf"])) and len(np.unique(v["rgb"], axis=0)) > 250


def test_sparse_field_windows():
    """About half of the 3^3 windows of the default sparse field hold no odd cell, and single odd cells occur at all 27 places."""
    blocks = mf.sparse_field(3, odd=0.03)
    _, lo, hi = mf.thresholds()
    n = 32
    odd = np.zeros((n, n, n), bool)
    for b, blk in blocks.items():
        v = mf.block_voxels(b)
        o = (blk["weight"] == 0) | ~((blk["sdf"] >= lo) & (blk["sdf"] <= hi))
        odd[v[:, 0], v[:, 1], v[:, 2]] = o
    assert 0.02 < odd.mean() < 0.04
    c = np.zeros((n - 2, n - 2, n - 2), int)
    places = []
    for i, d in enumerate([(0, 0, 0)] + mf.DIRS26):
        w = odd[1 + d[0]: n - 1 + d[0], 1 + d[1]: n - 1 + d[1], 1 + d[2]: n - 1 + d[2]]
        c += w
        places.append(w)
    assert 0.35 < (c == 0).mean() < 0.55
    assert all(np.any(w & (c == 1)) for w in places)


def test_odd_cell_positions():
    kinds = [k for k, _ in mf.ODD_POSITIONS]
    assert kinds.count("corner") == 8 and kinds.count("edge") == 3 and kinds.count("face") == 3 and kinds.count("interior") >= 1
    pos = dict()
    for k, p in mf.ODD_POSITIONS:
        on = sum(c in (0, 7) for c in p)
        assert on == {"corner": 3, "edge": 2, "face": 1, "depth": 0, "interior": 0}[k], (k, p)
        pos.setdefault(k, set()).add(p)
    assert len(pos["corner"]) == 8
    assert {tuple(i for i, c in enumerate(p) if c not in (0, 7)) for p in pos["edge"]} == {(0,), (1,), (2,)}  # one edge along each axis
    assert {tuple(i for i, c in enumerate(p) if c in (0, 7)) for p in pos["face"]} == {(0,), (1,), (2,)}
    assert sorted(p[0] for p in pos["depth"] | pos["interior"]) == [1, 2, 3, 4]
    T = F(mf.PARAMS["sdf_truncation"])
    for kind in mf.ODD_KINDS:
        for cn in (False, True):
            blocks, cells = mf.odd_cell(kind, base=(-7, 2, -1), coarse_neighbour=cn)
            assert len(cells) == len(mf.ODD_POSITIONS) and len(blocks) == 27 * len(cells)
            c = np.array(cells)
            gap = np.abs(c[:, None, :] - c[None, :, :]).max(-1) + 1000 * np.eye(len(c), dtype=int)
            assert gap.min() >= 8
            assert sum(isinstance(v, tuple) for v in blocks.values()) == (len(cells) if cn else 0)
            v = _all_voxels({k: b for k, b in blocks.items() if not isinstance(b, tuple)})
            is_sea = (v["sdf"] == T) & (v["weight"] == 1)
            assert (~is_sea).sum() == len(cells)
            if cn:  # the coarse block is a neighbour of the block that holds the odd cell
                for cell in cells:
                    b = tuple(a >> 3 for a in cell)
                    assert sum(_is_coarse(blocks, (b[0] + d[0], b[1] + d[1], b[2] + d[2])) for d in mf.DIRS26) == 1


@pytest.mark.parametrize("centre,other", mf.NEIGHBOUR_PAIRS)
def test_neighbour_gallery_uses_all_26_directions(centre, other):
    blocks, layout = mf.neighbour_gallery(centre, other, base=(3, -4, 5))
    assert sorted(d for _, d in layout) == sorted(mf.DIRS26) and len(layout) == 26

    def kind(b):
        return "absent" if b not in blocks else ("coarse" if _is_coarse(blocks, b) else "fine")

    for mid, d in layout:
        assert kind(mid) == centre
        for e in mf.DIRS26:
            assert kind((mid[0] + e[0], mid[1] + e[1], mid[2] + e[2])) == (other if e == d else centre)
        for e in mf.DIRS26:  # two absent blocks around every cluster
            for r in (2, 3):
                assert kind((mid[0] + r * e[0], mid[1] + r * e[1], mid[2] + r * e[2])) == "absent"
    assert len(blocks) == 26 * (26 if other == "absent" else 27)


def test_ladder_rungs_span_their_boundaries():
    rungs = mf.ladder_rungs()
    assert sorted({k for k, _, _ in rungs}) == list(range(8, 17)) and len(rungs) == 18
    signs = set()
    for k, side, coords in rungs:
        c = np.array(coords)
        assert len(coords) == 63 and len(set(coords)) == 63
        amax = np.abs(c).max(1)
        assert np.array_equal(amax, np.abs(c[:, 0]))  # x decides
        assert sorted(set((side * c[:, 0]).tolist())) == list(range((1 << k) - 5, (1 << k) + 2))
        staged = (amax + 3) * 8 < (1 << (k + 3))  # k_mc's `staged` for a shift limit of 2^(k + 3) voxels
        assert staged.any() and (~staged).any(), k
        if k == 15:
            known = (amax + 2) * 8 < (1 << 18)  # fine_known / coarse_known
            assert known.any() and (~known).any()
            assert np.all((amax + 3) * 8 < (1 << 20))  # ... while staged, where the shift limit lies beyond the ladder (2^-4 m)
        signs.add((k, int(np.sign(c[0, 1] + 1)), int(np.sign(c[0, 2] + side))))
    assert len({s[1] for s in signs}) == 2 and len({s[2] for s in signs}) == 2
    o = np.array(mf.ORIGIN_CLUSTER)
    assert all(set(np.sign(o[:, a]).tolist()) >= {-1, 0, 1} or set(np.sign(o[:, a]).tolist()) >= {-1, 1} for a in range(3))
    for vs in (0.05, 0.0625):
        blocks, p = mf.ladder(vs)
        assert p["virtual_voxel_size"] == vs and len(blocks) == 18 * 63 + 64
        assert np.abs(np.array(list(blocks))).max() < (1 << 20)  # inside the packed-key range
