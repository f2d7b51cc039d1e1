"""CPU half of the scan normals (include/mrhash_normals.h): the header, the binding and the exported symbols
agree, the two structs have the C layout, the restatement (tests/normals_ref.py: restate) gives the known answers on hand-built
clouds, agrees with a textbook estimator (normals_ref.textbook) and finds the faces of the analytic street scene."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest

import normals_ref as nr
from mrhash_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = np.float32(0.4)
IDENT = (np.zeros(3, np.float32), np.array([0, 0, 0, 1], np.float32))


def test_normals_header_and_binding_agree_and_the_library_exports_them(hip):
    hdr = open(os.path.join(ROOT, "include", "mrhash_normals.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mrh_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == sorted(capi.NORMALS_SYMBOLS) and len(declared) == 3
    for name in declared:
        assert hasattr(hip, name), f"libmrhash_hip.so does not export {name}"


def test_normals_structs_match_header():
    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "mrhash_normals.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mrh_normals_params), offsetof(mrh_normals_params, min_points),
                 offsetof(mrh_normals_params, min_spread), offsetof(mrh_normals_params, max_flatness), sizeof(mrh_normals_info),
                 offsetof(mrh_normals_info, estimated), offsetof(mrh_normals_info, cells));
          return 0;
        }"""
    )
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "probe.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    P, I = capi.MrhNormalsParams, capi.MrhNormalsInfo
    assert got == [C.sizeof(P), P.min_points.offset, P.min_spread.offset, P.max_flatness.offset, C.sizeof(I), I.estimated.offset, I.cells.offset]
    assert got[0] == 16 and got[4] == 40


def test_estimate_without_a_context_is_an_invalid_argument(hip):
    assert hip.mrh_estimate_normals(None, None, None) == capi.MRH_ERR_INVALID_ARG
    assert hip.mrh_estimate_normals_device(None, None, None, 0, None) == capi.MRH_ERR_INVALID_ARG
    n, p = C.c_uint64(), C.c_void_p()
    assert hip.mrh_get_normals(None, C.byref(p), C.byref(n), None) == capi.MRH_ERR_INVALID_ARG


# ---- hand cases for the restatement ------------------------------------------------------------------------------------------

def _lattice(origin, e1, e2, n=9, spacing=float(RHO) / 8):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return (np.asarray(origin, np.float64) + spacing * (i[..., None] * np.asarray(e1, np.float64) + j[..., None] * np.asarray(e2, np.float64))).reshape(-1, 3).astype(np.float32)


def _reversed_beam(p):
    p = np.asarray(p, np.float32)
    r = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
    return -(p / r[:, None])


def test_a_lattice_on_a_horizontal_plane_gives_the_vertical_exactly():
    pts = _lattice((2.0, -0.2, -1.7), (1, 0, 0), (0, 1, 0))
    r = nr.restate(pts)
    assert r.info == dict(points=81, estimated=81, fallback=0, missing=0, cells=r.info["cells"]) and r.info["cells"] >= 1
    assert np.array_equal(r.normals, np.tile(np.array([[0, 0, 1]], np.float32), (81, 1)))
    # seen from below, the same plane faces down
    up = nr.restate(pts * np.array([1, 1, -1], np.float32))
    assert np.array_equal(up.normals, np.tile(np.array([[0, 0, -1]], np.float32), (81, 1)))


def test_too_few_points_take_the_reversed_beam_bit_for_bit():
    pts = np.array([[5.0, 0.1, 0.2], [5.05, 0.15, 0.2], [5.0, 0.2, 0.25], [5.1, 0.1, 0.3]], np.float32)
    r = nr.restate(pts)
    assert r.info["fallback"] == 4 and r.info["estimated"] == 0
    assert r.normals.tobytes() == _reversed_beam(pts).tobytes()


def test_missing_returns_map_to_zero():
    pts = _lattice((2.0, -0.2, -1.7), (1, 0, 0), (0, 1, 0))
    pts[[3, 40, 80]] = 0.0
    pts[7] = (np.nan, 1.0, 1.0)
    pts[9] = (np.inf, 1.0, 1.0)
    r = nr.restate(pts)
    assert r.info["missing"] == 5 and r.info["estimated"] == 76
    assert not r.normals[[3, 7, 9, 40, 80]].any() and not np.isnan(r.normals).any()
    assert np.array_equal(r.normals[0], np.array([0, 0, 1], np.float32))


def test_a_straight_line_fails_the_spread_gate():
    k = np.arange(40, dtype=np.float64)[:, None]
    pts = (np.array([3.0, 1.0, -0.5]) + 0.02 * k * np.array([0.6, 0.8, 0.0])).astype(np.float32)
    r = nr.restate(pts)
    assert r.info["estimated"] == 0 and r.info["fallback"] == 40
    assert r.normals.tobytes() == _reversed_beam(pts).tobytes()
    # the same cloud passes once the gate asks for no spread at all but a tiny one, so it was the spread gate that refused
    assert nr.restate(pts, min_spread=1e-6, max_flatness=0.99).info["estimated"] > 0


def test_two_perpendicular_planes_in_one_neighbourhood_fail_the_flatness_gate():
    floor = _lattice((2.0, 0.0, -1.0), (1, 0, 0), (0, 1, 0))
    wall = _lattice((2.0, 0.0, -1.0), (0, 1, 0), (0, 0, 1))
    pts = np.concatenate([floor, wall])
    r = nr.restate(pts)
    assert r.info["estimated"] == 0 and r.info["fallback"] == len(pts)
    assert nr.restate(floor).info["estimated"] == 81 and nr.restate(wall).info["estimated"] == 81


def test_a_cell_outside_the_key_range_takes_the_reversed_beam():
    near = _lattice((3.0, 0.0, -1.0), (1, 0, 0), (0, 1, 0), spacing=0.0625)
    far = near + np.array([3.0e5 - 3.0, 0, 0], np.float32)  # 3e5 / 0.25 = 1.2e6 cells >= 2^20; the lattice survives binary32 there
    assert len(np.unique(far, axis=0)) == 81
    r = nr.restate(np.concatenate([near, far]), radius=0.25)
    assert (r.point_cell[:81] >= 0).all() and (r.point_cell[81:] == -1).all()
    assert r.info["estimated"] == 81 and r.info["fallback"] == 81
    assert r.normals[81:].tobytes() == _reversed_beam(far).tobytes()


def test_the_order_of_the_points_does_not_matter():
    pts = synth.lidar_scan(synth.street_canyon(), *IDENT, rows=32, cols=512, noise_sigma=0.02, max_range=100.0, dropout=0.05)
    perm = np.random.default_rng(3).permutation(len(pts))
    a, b = nr.restate(pts), nr.restate(pts[perm])
    assert a.info == b.info and a.info["estimated"] > 5000 and a.info["missing"] > 100
    assert a.normals[perm].tobytes() == b.normals.tobytes()


def test_jacobi_agrees_with_eigh_on_random_symmetric_matrices():
    rng = np.random.default_rng(0)
    M = rng.normal(size=(500, 3, 3))
    A = M @ M.transpose(0, 2, 1)
    lam, V = nr.jacobi(A)
    ref = np.linalg.eigvalsh(A)
    assert np.allclose(lam, ref, rtol=1e-12, atol=1e-12)
    assert np.allclose(np.einsum("nij,nj->ni", A, V[:, :, 0]), lam[:, :1] * V[:, :, 0], atol=1e-10)


# ---- the restatement against the textbook estimator, and both against the analytic scene -----------------------------------------

@pytest.fixture(scope="module", params=[0.0, 0.02], ids=["noiseless", "noisy"])
def scan(request):
    pts = synth.lidar_scan(synth.street_canyon(), *IDENT, rows=128, cols=1024, noise_sigma=request.param, max_range=100.0)
    return request.param, pts, nr.restate(pts), nr.textbook(pts)


def test_restate_and_textbook_decide_alike_and_agree_within_half_a_degree(scan):
    """Bound: a float64 probe of D12 steps 2-5 and 7 with eigh gave identical gates and at most 0.089 deg (noiseless) and
    0.231 deg (noisy) between the quantised and the unquantised moments; 0.5 deg is about twice the larger value, the margin
    covers Jacobi against eigh and nothing else.  Measured here: 0.0887 deg and 0.2313 deg, identical gates on both scans."""
    noise, pts, a, b = scan
    assert np.array_equal(a.keys, b.keys)
    assert np.array_equal(a.estimated, b.estimated)
    e = a.estimated
    cos = np.abs((a.cell_normals[e] * b.cell_normals[e]).sum(axis=1)).clip(0, 1)
    worst = float(np.degrees(np.arccos(cos)).max())
    print(f"noise {noise}: {int(e.sum())} estimated cells of {len(e)}, max angle restate/textbook {worst:.4f} deg")
    assert worst <= 0.5


def _true_normals_ok(pts, normals, tol, max_deg=5.0):
    """per point: does `normals` lie within max_deg of the normal of a face of the scene the point lies on (within tol)?  Also
    whether the point was matched to a face at all."""
    scene = synth.street_canyon()
    p = pts.astype(np.float64)
    n = normals.astype(np.float64)
    good = np.zeros(len(p), bool)
    matched = np.zeros(len(p), bool)
    cmin = np.cos(np.radians(max_deg))
    for box in [scene.room] + list(scene.furniture):
        lo, hi = np.array(box.lo), np.array(box.hi)
        inside = ((p >= lo - tol) & (p <= hi + tol)).all(axis=1)
        for a in range(3):
            for v in (lo[a], hi[a]):
                on = inside & (np.abs(p[:, a] - v) <= tol)
                matched |= on
                good |= on & (np.abs(n[:, a]) >= cmin)
    return good, matched


def test_the_definition_finds_the_faces_of_the_analytic_scene(scan):
    """Textbook alone first (so that the comparison is not vacuous): it estimates at least 0.80 of the 128 x 1024 scan and is
    within 5 deg of the true face normal on at least 0.97 of those.  The product definition then gives up at most 0.01 on either
    share.  Measured: estimated 0.8629 / 0.8595 (noiseless / noisy), within 5 deg 0.9905 / 0.9907, the same for both estimators."""
    noise, pts, a, b = scan
    tol = 1e-4 if noise == 0.0 else 0.1
    ret = np.linalg.norm(pts, axis=1) > 0
    shares = {}
    for name, r in (("textbook", b), ("restate", a)):
        est = (r.point_cell >= 0)
        est[est] = r.estimated[r.point_cell[est]]
        good, matched = _true_normals_ok(pts, r.normals, tol)
        assert matched[ret].all()
        shares[name] = (est.sum() / len(pts), good[est].sum() / est.sum())
        print(f"noise {noise} {name}: estimated {shares[name][0]:.4f}, within 5 deg of the truth {shares[name][1]:.4f}")
    assert shares["textbook"][0] >= 0.80 and shares["textbook"][1] >= 0.97
    assert shares["restate"][0] >= shares["textbook"][0] - 0.01
    assert shares["restate"][1] >= shares["textbook"][1] - 0.01
