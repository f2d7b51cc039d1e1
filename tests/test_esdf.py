"""CPU half of the distance field (include/mrhash_esdf.h): the separable form of the restatement
(tests/esdf_ref.py) equals the brute force over all cell x site pairs bit for bit, the restatement gives the known answers on
hand-built maps, and the header, the binding and the exported symbols agree."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest

import esdf_ref as er
import independent as ind
from mrhash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = er.SPHERE_PARAMS
VS = np.float32(PARAMS["virtual_voxel_size"])
THREE_SITES = [(-17, -11, -14), (3, 5, -2), (21, 23, 13)]  # the first and the last cell of SPHERE_BOX and one in between


def _plane_map():
    import test_raycast as tr

    return ind.Map(tr.PARAMS, tr.plane_blocks())


@pytest.fixture(scope="module")
def maps():
    return {"sphere": ind.Map(PARAMS, er.sphere_blocks()), "plane": _plane_map(), "sites": ind.Map(PARAMS, er.site_blocks(THREE_SITES))}


# boxes per map: the 41 x 37 x 29 box placed where the map has surface, a single cell and a thin slab
BOXES = {
    "sphere": [er.SPHERE_BOX, ((7, 0, 0), (1, 1, 1)), ((5, 0, -1), (5, 1, 3))],
    "plane": [((-16, -15, 36), (41, 37, 29)), ((0, 0, 50), (1, 1, 1)), ((-2, 3, 49), (5, 1, 3))],
    "sites": [((-17, -11, -14), (41, 37, 29)), ((3, 5, -2), (1, 1, 1)), ((1, 5, -3), (5, 1, 3))],
}


@pytest.mark.parametrize("name", ["sphere", "plane", "sites"])
def test_separable_equals_brute_force(maps, name):
    m = maps[name]
    for origin, dims in BOXES[name]:
        mw = 1 if name == "plane" else 0  # the plane's voxels have weight 1 under a threshold of 5
        state, sdf = er.classify(m, origin, dims, min_weight=mw)
        site = (state & er.SITE) != 0
        assert site.any(), (name, origin, dims)
        literal = er.brute(site)
        for R in (1, 3, 12, 600):
            want = er.finish(m.vs, state, sdf, literal, R)
            got = er.finish(m.vs, state, sdf, er.separable(site, R), R)
            for a, b, what in zip(got, want, ("dist", "state", "d2")):
                assert er.same_bits(a, b), (name, origin, dims, R, what)
            assert all(er.same_bits(a, b) for a, b in zip(got, er.esdf(m, origin, dims, R, min_weight=mw)))


def test_one_site_gives_the_squared_distance_everywhere():
    s = np.array([4, -3, 6])
    origin, dims = (-10, -12, -5), (30, 25, 20)
    m = ind.Map(PARAMS, er.site_blocks([s]))
    dist, state, d2 = er.esdf(m, origin, dims, 600)
    want = ((er.cells(origin, dims) - s) ** 2).sum(-1)
    assert np.array_equal(d2, want)
    k, j, i = s[2] - origin[2], s[1] - origin[1], s[0] - origin[0]
    assert state[k, j, i] == er.OBSERVED | er.SITE and dist[k, j, i] == 0 and np.count_nonzero(state & er.SITE) == 1
    assert not np.any(state & er.FAR)
    off = want > 0
    assert er.same_bits(np.abs(dist[off]), (VS * np.sqrt(want[off].astype(np.float32))).astype(np.float32))
    # unobserved cells (outside the site's block) are positive, like observed free space
    assert np.all(dist[off] > 0) and np.any((state & er.OBSERVED) == 0)


def test_plane_gives_the_distance_to_its_layer():
    import test_raycast as tr

    m = _plane_map()
    origin, dims = (-16, -16, 40), (32, 32, 24)  # inside the plane's blocks in x and y: every column sees the plane
    dist, state, d2 = er.esdf(m, origin, dims, 12, min_weight=1)
    vs = np.float32(tr.PARAMS["virtual_voxel_size"])
    kz = er.cells(origin, dims)[..., 2]
    site = (state & er.SITE) != 0
    layers = np.unique(kz[site])  # the voxel layers with |1 - z| <= vs around z = 1 m = voxel 50: whole layers, adjacent
    assert 50 in layers and 1 <= len(layers) <= 3 and np.array_equal(layers, np.arange(layers[0], layers[-1] + 1))
    assert np.array_equal(site, np.isin(kz, layers))
    off = ~site
    gap = np.abs(kz[..., None] - layers).min(-1)
    assert er.same_bits(np.abs(dist[off]), (vs * gap[off].astype(np.float32)).astype(np.float32))
    assert np.all(dist[off & (kz > 50)] < 0) and np.all(dist[off & (kz < 50)] > 0)
    assert np.array_equal(d2[off], (gap ** 2)[off]) and not np.any(state & er.FAR)


def test_a_box_without_a_site_is_far_everywhere():
    m = ind.Map(PARAMS, er.sphere_blocks())
    R = 7
    dist, state, d2 = er.esdf(m, (-2, -2, -2), (4, 4, 4), R)  # the sphere's core: clamped at -trunc, observed, inside
    assert np.all(state == er.OBSERVED | er.INSIDE | er.FAR) and np.all(d2 == er.FAR_D2)
    assert np.all(dist == -(VS * np.float32(R)))
    dist, state, d2 = er.esdf(m, (100, 100, 100), (3, 4, 5), R)  # no block at all
    assert np.all(state == er.FAR) and np.all(d2 == er.FAR_D2) and np.all(dist == VS * np.float32(R))


@pytest.mark.parametrize("corner", [0, 1])
def test_a_site_in_the_first_and_in_the_last_cell(corner):
    origin, dims = np.array([-5, 3, -9]), np.array([12, 7, 10])
    s = origin if corner == 0 else origin + dims - 1
    m = ind.Map(PARAMS, er.site_blocks([s]))
    dist, state, d2 = er.esdf(m, origin, dims, 600)
    assert np.array_equal(d2, ((er.cells(origin, dims) - s) ** 2).sum(-1))
    at = (0, 0, 0) if corner == 0 else tuple(dims[::-1] - 1)
    assert state[at] & er.SITE and d2[at] == 0
    assert all(er.same_bits(a, b) for a, b in zip((dist, state, d2), er.esdf(m, origin, dims, 600, literal=True)))


def test_the_reach_is_inclusive():
    """d2 == R^2 is not far, R^2 + 1 is: R = 5 with the cells at offsets (5, 0, 0), (3, 4, 0) (25) and (5, 1, 0) (26)."""
    m = ind.Map(PARAMS, er.site_blocks([(0, 0, 0)]))
    dist, state, d2 = er.esdf(m, (-6, -6, -6), (13, 13, 13), 5)
    c = 6
    for off, far in (((5, 0, 0), False), ((3, 4, 0), False), ((0, -5, 0), False), ((5, 1, 0), True), ((3, 3, 3), True), ((0, 0, 6), True)):
        k, j, i = c + off[2], c + off[1], c + off[0]
        n2 = sum(x * x for x in off)
        assert bool(state[k, j, i] & er.FAR) == far, off
        assert d2[k, j, i] == (er.FAR_D2 if far else n2)
        assert dist[k, j, i] == (VS * np.float32(5) if far else VS * np.sqrt(np.float32(n2)))


def test_band_weight_and_coarse_lookup():
    """surface_band and min_weight replace the defaults, and a coarse block answers with the voxel that covers the cell."""
    blocks = er.site_blocks([(1, 1, 1)])
    blocks[(0, 0, 0)]["sdf"][0] = 0.019
    blocks[(0, 0, 0)]["weight"][0] = 3
    m = ind.Map(PARAMS, blocks)
    st, _ = er.classify(m, (0, 0, 0), (2, 2, 2))
    assert st[0, 0, 0] & er.SITE and st[1, 1, 1] & er.SITE  # default band: one voxel (5 cm)
    st, _ = er.classify(m, (0, 0, 0), (2, 2, 2), surface_band=0.01)
    assert not st[0, 0, 0] & er.SITE and st[1, 1, 1] & er.SITE
    st, _ = er.classify(m, (0, 0, 0), (2, 2, 2), min_weight=2)
    assert st[0, 0, 0] == er.OBSERVED | er.SITE and st[1, 1, 1] == 0
    coarse = np.zeros(64, capi.VOXEL_DTYPE)
    coarse["sdf"], coarse["weight"] = np.arange(64, dtype=np.float32), 1
    mm = ind.MultiMap(dict(PARAMS, sdf_var_threshold=0.005), {(0, 0, 0): (1, coarse)})
    found, res, sdf, _ = er.lookup(mm, (0, 0, 0), (8, 8, 8))
    k, j, i = np.mgrid[0:8, 0:8, 0:8]
    assert found.all() and np.all(res == 1) and np.array_equal(sdf, ((k // 2) * 16 + (j // 2) * 4 + i // 2).astype(np.float32))
    st, _ = er.classify(mm, (0, 0, 0), (8, 8, 8))
    assert np.count_nonzero(st & er.SITE) == 8  # sdf 0 only: the band of a coarse voxel is 2 vs = 0.1 m


# ---- header and binding -------------------------------------------------------------------------------------------------

def test_esdf_header_and_binding_agree_and_the_library_exports_them(hip):
    hdr = open(os.path.join(ROOT, "include", "mrhash_esdf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mrh_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == sorted(capi.ESDF_SYMBOLS)
    for name in declared:
        assert hasattr(hip, name), f"libmrhash_hip.so does not export {name}"


def test_esdf_param_struct_matches_header():
    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "mrhash_esdf.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %u %u %u %u %u %u\\n", sizeof(mrh_esdf_params), offsetof(mrh_esdf_params, dims),
                 offsetof(mrh_esdf_params, max_distance_voxels), offsetof(mrh_esdf_params, min_weight),
                 offsetof(mrh_esdf_params, surface_band), offsetof(mrh_esdf_params, outputs), MRH_ESDF_STATE, MRH_ESDF_SQUARED,
                 MRH_ESDF_OBSERVED, MRH_ESDF_SITE, MRH_ESDF_INSIDE, MRH_ESDF_FAR);
          return 0;
        }"""
    )
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "probe.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    P = capi.MrhEsdfParams
    assert got == [C.sizeof(P), P.dims.offset, P.max_distance_voxels.offset, P.min_weight.offset, P.surface_band.offset, P.outputs.offset,
                   capi.ESDF_STATE, capi.ESDF_SQUARED, capi.ESDF_OBSERVED, capi.ESDF_SITE, capi.ESDF_INSIDE, capi.ESDF_FAR]
    assert got[0] == 40
    assert (er.OBSERVED, er.SITE, er.INSIDE, er.FAR, er.FAR_D2) == (capi.ESDF_OBSERVED, capi.ESDF_SITE, capi.ESDF_INSIDE, capi.ESDF_FAR, capi.ESDF_FAR_D2)


def test_esdf_without_a_context_is_an_invalid_argument(hip):
    p = capi.MrhEsdfParams((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8), 4, 0, 0.0, 3)
    out = C.c_void_p()
    assert hip.mrh_esdf(None, C.byref(p), C.byref(out), None, None) == capi.MRH_ERR_INVALID_ARG
    assert hip.mrh_esdf(None, None, None, None, None) == capi.MRH_ERR_INVALID_ARG
    assert hip.mrh_esdf_device(None, C.byref(p), None, None, None) == capi.MRH_ERR_INVALID_ARG
