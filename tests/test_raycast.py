"""CPU half of the raycast (include/mrhash_raycast.h): the header, the binding and the exported symbols agree,
the parameter block has the C layout, and the restatement (tests/raycast_ref.py) gives the known answers on hand-built maps."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest

import independent as ind
import raycast_ref as rr
from mrhash_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = capi.VOXEL_DTYPE


def test_raycast_header_and_binding_agree_and_the_library_exports_them(hip):
    hdr = open(os.path.join(ROOT, "include", "mrhash_raycast.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mrh_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == sorted(capi.RAYCAST_SYMBOLS)
    for name in declared:
        assert hasattr(hip, name), f"libmrhash_hip.so does not export {name}"


def test_raycast_param_struct_matches_header():
    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "mrhash_raycast.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(mrh_raycast_params), offsetof(mrh_raycast_params, rows),
                 offsetof(mrh_raycast_params, min_depth), offsetof(mrh_raycast_params, step), offsetof(mrh_raycast_params, outputs),
                 offsetof(mrh_raycast_params, cy), MRH_RAYCAST_NORMALS, MRH_RAYCAST_COLORS);
          return 0;
        }"""
    )
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "probe.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    P = capi.MrhRaycastParams
    assert got == [C.sizeof(P), P.rows.offset, P.min_depth.offset, P.step.offset, P.outputs.offset, P.cy.offset,
                   capi.RAYCAST_NORMALS, capi.RAYCAST_COLORS]
    assert got[0] == 40


def test_raycast_without_a_context_is_an_invalid_argument(hip):
    p = capi.MrhRaycastParams(100.0, 100.0, 3.5, 3.5, 8, 8, 0.1, 2.0, 0.0, 3)
    R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (C.c_float * 3)(0, 0, 0)
    out = C.c_void_p()
    assert hip.mrh_raycast(None, C.byref(p), R, t, C.byref(out), None, None) == capi.MRH_ERR_INVALID_ARG
    assert hip.mrh_raycast_device(None, C.byref(p), R, t, None, None, None) == capi.MRH_ERR_INVALID_ARG


# ---- known answers of the restatement ----------------------------------------------------------------------------------

PARAMS = dict(synth.CFG1_PARAMS)  # 2 cm voxels, 6 cm truncation
VS, TRUNC = np.float32(PARAMS["virtual_voxel_size"]), np.float32(PARAMS["sdf_truncation"])
# an 8 x 8 camera whose pixel (4, 4) looks straight down +z; every ray reaches z = 1 m within the blocks below
CAM = dict(fx=100.0, fy=100.0, cx=3.5, cy=3.5, rows=8, cols=8)
# samples z_48 = 0.9825 and z_49 = 1.0025 bracket the plane; the reference's trilinear (weights 1/2, vds.cu:318-320) gives the
# stair values +-vs/2 there, and three regula-falsi steps from a = 1 - 7/8 vs, b = 1 + 1/8 vs land on z = 1 exactly
RANGE = dict(min_depth=0.0225, max_depth=2.0, step=0.02)


def plane_blocks(z_blocks=(5, 6, 7), xy_blocks=range(-2, 2)):
    """A plane at z = 1 m: every voxel sdf = clamp(1 - z_voxel, +-trunc), weight 1, rgb = (x, y, z) & 0xFF of the voxel."""
    lin = np.arange(512)
    lx, ly, lz = lin % 8, (lin // 8) % 8, lin // 64
    out = {}
    for bx in xy_blocks:
        for by in xy_blocks:
            for bz in z_blocks:
                v = np.zeros(512, VOXEL)
                zv = ((bz * 8 + lz).astype(np.float32) * VS).astype(np.float32)
                sdf = (np.float32(1.0) - zv).astype(np.float32)
                v["sdf"] = np.where(sdf >= 0, np.minimum(TRUNC, sdf), np.maximum(-TRUNC, sdf))
                v["weight"] = 1
                v["rgb"] = np.stack([(bx * 8 + lx) & 0xFF, (by * 8 + ly) & 0xFF, (bz * 8 + lz) & 0xFF], -1).astype(np.uint8)
                out[(bx, by, bz)] = v
    return out


def render(blocks, R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32)):
    rc = rr.Raycaster(ind.Map(PARAMS, blocks), CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["rows"], CAM["cols"], R, t, **RANGE)
    r, c = np.mgrid[0:8, 0:8]
    return rc.render(r, c)


def test_restatement_hits_a_plane_at_its_distance_with_its_normal():
    depth, nrm, rgb = render(plane_blocks())
    assert np.all(np.abs(depth - 1.0) <= 1e-5), depth
    assert np.all(np.abs(nrm - np.array([0, 0, -1], np.float32)) <= 1e-5), nrm
    assert np.all(rgb[:, 2] == 50)  # the voxel at z = 1 m


def test_restatement_a_ray_that_misses_gives_zeros():
    R = np.diag([-1.0, 1.0, -1.0]).astype(np.float32)  # looking down -z, away from the plane
    depth, nrm, rgb = render(plane_blocks(), R=R)
    assert not depth.any() and not nrm.any() and not rgb.any()


def test_restatement_a_removed_block_in_front_of_the_plane_changes_nothing():
    want = render(plane_blocks())
    got = render(plane_blocks(z_blocks=(6, 7)))
    for a, b in zip(want, got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_restatement_a_removed_block_at_the_crossing_removes_the_hit():
    depth, nrm, rgb = render(plane_blocks(z_blocks=(5, 7)))  # the plane's own block (voxels z = 48 .. 55) is gone
    assert not depth.any() and not nrm.any() and not rgb.any()


def test_restatement_moves_a_hit_to_the_next_crossing():
    """Two planes (z = 1 m in blocks 5-7, z = 1.5 m in blocks 8-10): without the first plane's block the second one is hit."""
    far = {}
    for k, v in plane_blocks(z_blocks=(8, 9, 10)).items():
        v = v.copy()
        zv = ((k[2] * 8 + np.arange(512) // 64).astype(np.float32) * VS).astype(np.float32)
        sdf = (np.float32(1.5) - zv).astype(np.float32)
        v["sdf"] = np.where(sdf >= 0, np.minimum(TRUNC, sdf), np.maximum(-TRUNC, sdf))
        far[k] = v
    near = plane_blocks(z_blocks=(5, 7))
    depth, _, _ = render({**near, **far})
    assert np.all(np.abs(depth - 1.5) <= 0.5 * VS), depth


def test_restatement_rejects_more_than_2_20_samples():
    with pytest.raises(ValueError):
        rr.sample_depths(0.1, 30.0, 1e-6)
    assert len(rr.sample_depths(0.1, 2.0, 0.5)) == 4
