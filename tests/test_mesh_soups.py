"""The mesh post-process on the hand-built soups of tests/mesh_soups.py, on the CPU.

Three statements of MeshExtractor::processTriangles meet here: the vectorised numpy restatement (mesh_soups.process), a literal
Python transliteration of mesh_extractor.cpp:9-76, :156-259 below (one loop, two dicts), and the oracle through
Engine.process_triangles.  The smallest soups also have their V / F / C written out by hand.  Everything is compared byte for byte.
tests/test_mesh_soups_gpu.py runs the same soups through the HIP library.

The cell index is defined once in mrhash_amd/csrc/mrh_meshkey.h; tests/host/meshkey_check.cpp walks it over its edges under
ASan + UBSan + float-cast-overflow, as a process of its own.
"""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mesh_soups as ms
from mrhash_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = np.float32(ms.EPS_EXACT)
f32, f64 = np.float32, np.float64


def col(*idx):
    """The colour the builders give soup vertex i."""
    return np.array([[i, 0.5 * i, -(i % 1024)] for i in idx], f64).reshape(-1, 3)


def faces(rows):
    return np.array(rows, np.int32).reshape(-1, 3)


def case(name, eps=0.0, *args):
    return next(c for c in ms.CASES if c.name == name and c.eps == eps and c.args == args)


# ---- a literal transliteration: slow, and nothing in common with the vectorised one -----------------------------------------------

def literal(soup, eps):
    eps = float(f32(eps))
    inv_eps = 1.0 / eps if eps != 0.0 else 0.0
    vmap, V, C, corner = {}, [], [], []
    for v in soup.reshape(-1):
        p = [float(x) for x in v["p"]]
        if eps == 0.0:
            key = struct.pack("<3d", *p)
        else:
            key = []
            for x in p:
                q = x * inv_eps
                q = math.floor(q) if math.isfinite(q) else q
                key.append(int(q) if -2147483648.0 <= q < 2147483648.0 else ms.INT32_MIN)
            key = tuple(key)
        idx = None if any(math.isnan(x) for x in p) else vmap.get(key)
        if idx is None:
            idx = len(V)
            if not any(math.isnan(x) for x in p):
                vmap[key] = idx
            V.append(p)
            C.append([float(x) for x in v["c"]])
        corner.append(idx)
    seen, F = set(), []
    for t in range(len(corner) // 3):
        f = tuple(corner[3 * t: 3 * t + 3])
        if f[0] == f[1] or f[0] == f[2] or f[1] == f[2] or f in seen:
            continue
        seen.add(f)
        F.append(f)
    return np.array(V, f64).reshape(-1, 3), np.array(F, np.int32).reshape(-1, 3), np.array(C, f64).reshape(-1, 3)


@pytest.mark.parametrize("c", ms.SMALL_CASES, ids=lambda c: c.id)
def test_restatement_equals_the_literal_loop(c):
    ms.assert_same_mesh(ms.expected(c), literal(ms.soup(c), c.eps), c.id)


# ---- answers written by hand --------------------------------------------------------------------------------------------------------

TRI = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
Q = float("nan")
HAND = {
    "single-eps0": (TRI, [[0, 1, 2]], col(0, 1, 2)),
    "one_key-eps0": ([[1, 2, 3]], [], col(0)),
    "one_key-eps0.25": ([[1, 2, 3]], [], col(0)),
    # -0 and +0 stay two vertices and keep their sign; in one cell they are one vertex (the first: +0)
    "signed_zero-eps0": ([[0.0, 1, 2], [-0.0, 1, 2], [5, 5, 5], [6, 6, 6]], [[0, 1, 2], [1, 0, 3]], col(0, 1, 2, 5)),
    "signed_zero-eps0.25": ([[0.0, 1, 2], [5, 5, 5], [6, 6, 6]], [], col(0, 2, 5)),
    # every NaN vertex is its own, bit-identical ones and a later repeat included; their faces stay
    "nan-eps0": ([[Q, 1, 2], [1, Q, 2], [1, 2, Q], [Q, Q, Q], [Q, Q, Q], [0, 0, 0], [Q, 1, 2], [7, 7, 7]],
                 [[0, 1, 2], [3, 4, 5], [6, 5, 7]], col(0, 1, 2, 3, 4, 5, 6, 8)),
    "rotated_face-eps0": (TRI, [[0, 1, 2], [1, 2, 0], [0, 2, 1]], col(0, 1, 2)),
    "degenerate_repeat-eps0": (TRI, [[0, 1, 2]], col(0, 2, 8)),
    "one_face_many-eps0": (TRI, [[0, 1, 2]], col(0, 1, 2)),
    # cells 0, -1, 1, -2, then 0.25 eps -> cell 0 and -0.25 eps -> cell -1 (truncation would put both into cell 0)
    "cells_negative-eps0.25": ([[0.125, 0.125, 0.125], [-0.125, 0.125, 0.125], [0.375, 0.125, 0.125], [-0.375, 0.125, 0.125]],
                               [[0, 1, 2], [3, 0, 1]], col(0, 1, 2, 3)),
    # cells per soup vertex: -2 -3 -2 | -3 -1 -2 | -1 -2 0 | -1 0 -1 | 1 0 1 | 0 2 1 | 2 1 100
    "cell_edges-eps0.25": ([[-0.5, 0, 0], [ms.below(-0.5), 0, 0], [-0.25, 0, 0], [0.0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [25.0, 0, 0]],
                           [[1, 2, 0], [2, 0, 3], [3, 5, 4], [5, 4, 6]], col(0, 1, 4, 8, 12, 16, 20)),
    # triangle 0 lies in one cell; V and C are the FIRST position and colour of each cell
    "first_wins-eps0.25": (f32([[0.1, 0.2, 0.3], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]) * E, [[0, 1, 2], [1, 2, 0]], col(0, 4, 5)),
    "degenerate_by_merge-eps0.25": (f32([[0.1, 0, 0], [5.25, 0, 0], [7.5, 0, 0], [9.5, 0, 0]]) * E, [[2, 1, 3]], col(0, 2, 3, 5)),
    "degenerate_by_merge-eps0": (f32([[0.1, 0, 0], [0.6, 0, 0], [5.25, 0, 0], [7.5, 0, 0], [5.5, 0, 0], [9.5, 0, 0]]) * E,
                                 [[0, 1, 2], [3, 4, 5]], col(0, 1, 2, 3, 4, 5)),
    # +-3, +-2.5, +-inf share the cell INT32_MIN and are soup vertex 0; 2.0, 0.0 and 1.0 (soup vertex 16) are in range
    "out_of_range-eps1e-09": ([[3, 0, 0], [2, 0, 0], [0, 0, 0], [1, 0, 0]], [[0, 1, 2], [0, 2, 1], [0, 3, 2]], col(0, 1, 2, 16)),
}
HAND["nan_eps-eps0.25"] = HAND["nan_eps-eps0.013"] = HAND["nan-eps0"]
for _k in ("cells_negative", "first_wins", "degenerate_by_merge"):  # the same indices at eps = 0.013; positions from the soup
    HAND[_k + "-eps0.013"] = (None,) + HAND[_k + "-eps0.25"][1:]


@pytest.mark.parametrize("cid", sorted(HAND))
def test_restatement_equals_the_hand_written_answer(cid):
    c = ms.BY_ID[cid]
    V, F, C = HAND[cid]
    if V is None:
        first = {"cells_negative": [0, 1, 2, 3], "first_wins": [0, 4, 5], "degenerate_by_merge": [0, 2, 3, 5]}[c.name]
        V = ms.soup(c)["p"].reshape(-1, 3)[first]
    V = np.asarray(V, f32).astype(f64).reshape(-1, 3)  # every hand-written coordinate is a float32 value
    ms.assert_same_mesh(ms.expected(c), (V, faces(F), C), cid)


def test_signed_zero_keeps_the_sign_bit():
    V = ms.expected(case("signed_zero"))[0]
    assert V[:2, 0].view(np.uint64).tolist() == [0, 1 << 63]


def test_nan_vertices_keep_the_quiet_nan_pattern():
    V = ms.expected(case("nan"))[0]
    assert set(V[np.isnan(V)].view(np.uint64).tolist()) == {0x7FF8000000000000}


def test_structured_soups_by_their_construction():
    """Soups too long to write out: what their construction says about V, F and C."""
    V, F, C = ms.expected(case("all_distinct_tile"))
    ms.assert_same_mesh((V, F, C), (ms.distinct_points(513).astype(f64), faces(np.arange(513)), ms.colours(513).astype(f64)), "all_distinct_tile")
    # straddle: the four repeats vanish; every vertex after one moves up
    keep = np.setdiff1d(np.arange(1704), list(ms.STRADDLE_SAME))
    old_to_new = np.zeros(1704, np.int64)
    old_to_new[keep] = np.arange(1700)
    for later, first in ms.STRADDLE_SAME.items():
        old_to_new[later] = old_to_new[first]
    f = old_to_new.reshape(-1, 3)
    f = f[[t for t in range(568) if t not in (170, 343)]]  # (510, 511, 512) and (1029, 1030, 1031) became degenerate
    for eps in (0.0, ms.EPS_EXACT):
        ms.assert_same_mesh(ms.expected(case("straddle", eps)), (ms.distinct_points(1704)[keep].astype(f64), faces(f), ms.colours(1704)[keep].astype(f64)), "straddle")
    # reversed repeats: the first 2048 vertices with THEIR colours
    for eps in (0.0, ms.EPS_EXACT):
        V, F, C = ms.expected(case("reversed_repeats", eps))
        assert V.tobytes() == ms.distinct_points(2048).astype(f64).tobytes() and C.tobytes() == ms.colours(2048).astype(f64).tobytes()
        # triangle 682 is soup vertices 2046, 2047, 2048 = A[2046], A[2047], A[2047]: degenerate; the rest differ in phase or direction
        assert len(F) == 2047 and len(np.unique(F, axis=0)) == 2047 and not (F == [2046, 2047, 2047]).all(axis=1).any()
    V, F, C = ms.expected(case("low_bits"))
    assert len(V) == 4096 and C.tobytes() == ms.colours(4096).astype(f64).tobytes() and np.array_equal(F, (np.arange(4098) % 4096).reshape(-1, 3))
    V, F, C = ms.expected(case("specials"))
    assert len(V) == 9 and np.array_equal(F, [[0, 1, 2], [3, 4, 5], [6, 7, 8], [1, 2, 3], [4, 5, 6], [7, 8, 0]]) and C.tobytes() == col(*range(9)).tobytes()
    assert V[:, 0].astype(f32).tobytes() == ms.SPECIAL_VALUES.tobytes()
    # repeated_face: faces 300 and 5000 go, the order of the rest stays; their vertices never became vertices
    V, F, C = ms.expected(case("repeated_face"))
    kept_t = np.setdiff1d(np.arange(5001), ms.REPEATED_AT)
    assert np.array_equal(F, np.arange(3 * 4999).reshape(-1, 3)) and np.array_equal(V[::3, 0], kept_t)
    assert C.tobytes() == ms.colours(3 * 5001).reshape(-1, 3, 3)[kept_t].reshape(-1, 3).astype(f64).tobytes()
    # face_tiles: tile 1 (repeats) and tile 3 (degenerate) vanish, tile 4 keeps its even faces
    V, F, C = ms.expected(case("face_tiles"))
    T = ms.FACE_TILE
    kept_t = np.concatenate([np.arange(T), np.arange(2 * T, 3 * T), np.arange(4 * T, 5 * T, 2), np.arange(5 * T, 5 * T + 100)])
    first_corner = ms.soup(case("face_tiles"))["p"][kept_t, 0, 0]
    assert len(F) == len(kept_t) and np.array_equal(V[F[:, 0], 0], first_corner)
    for nv in ms.NV_EXACT:
        V, F, C = ms.expected(case("nv_exact", 0.0, nv))
        assert len(V) == nv and C.tobytes() == ms.colours(nv).astype(f64).tobytes()


def test_large_soups_have_the_sizes_they_are_for():
    """1025 vertex tiles / 1025 face tiles, every tile with first occurrences and repeats; the staging chunk edges."""
    assert (3 * ms.VERTEX_TILES_NT + 511) // 512 == 1025 and (ms.FACE_TILES_NT + 255) // 256 == 1025
    assert [nv * 12 % 65536 for nv in ms.NV_EXACT] == [65532, 8, 0, 12]
    for c in ms.LARGE_CASES:
        s = ms.soup(c)
        V, F, C = ms.expected(c)
        n = 3 * len(s)
        rep = ms.representatives(s, c.eps)
        firsts = np.add.reduceat((rep == np.arange(n)).astype(np.int64), np.arange(0, n, 512))
        print(f"{c.id}: {len(s)} triangles -> {len(V)} vertices, {len(F)} faces; first occurrences per tile {firsts.min()} .. {firsts.max()}")
        assert 0 < firsts[:-1].min() and firsts.max() < 512  # (the last tile holds 1 or 3 soup vertices)
        assert len(s) // 16 < len(s) - len(F) < len(s) // 2
        if c.eps:
            assert len(V) < len(ms.expected(c._replace(eps=0.0))[0])  # distinct positions share cells


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", ms.CASES, ids=lambda c: c.id)
def test_oracle_equals_the_restatement(oracle, c):
    with capi.Engine(oracle, ms.mesh_params(c.eps)) as e:
        ms.assert_same_mesh(ms.run_engine(e, ms.soup(c)), ms.expected(c), c.id)


def test_oracle_run_merge_equals_the_restatement(oracle):
    descs, counts, s = ms.runs()
    d, n, permuted = ms.permute_runs(descs, counts, s)
    with capi.Engine(oracle, ms.mesh_params(0.0)) as e:
        e.process_triangle_runs(descs, counts, s.ctypes.data, len(s), False)
        td, tc = e.triangle_blocks()
        assert td.tobytes() == d.tobytes() and tc.tobytes() == n.tobytes()
        ms.assert_same_mesh(e.extract_mesh(), ms.process(permuted, 0.0), "runs")
        with pytest.raises(capi.MrhError):
            e.process_triangle_runs(descs, counts, s.ctypes.data, len(s) - 1, False)


def test_no_triangles_after_some_gives_three_empty_arrays(oracle):
    with capi.Engine(oracle, ms.mesh_params(0.0)) as e:
        assert len(ms.run_engine(e, ms.soup(case("straddle")))[0]) == 1700
        V, F, C = ms.run_engine(e, np.zeros((0, 3), capi.TRI_DTYPE))
        assert (V.shape, F.shape, C.shape) == ((0, 3), (0, 3), (0, 3))
        assert V.dtype == f64 and F.dtype == np.int32 and C.dtype == f64


# ---- the cell index on its own -------------------------------------------------------------------------------------------------------

def test_mesh_cell_under_asan_ubsan(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host check"
    exe = str(tmp_path / "meshkey_check")
    # the sanitizer runtimes are linked statically: the program then runs the same whatever the environment preloads
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                            "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "mrhash_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "meshkey_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out
    assert "meshkey_check: 0 failures" in r.stdout
    for mark in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: "):
        assert mark not in out, out


def test_mesh_cell_has_one_definition():
    """The kernels and the host restatement call mesh_cell; no double -> int conversion of a floored coordinate is left beside it."""
    csrc = os.path.join(ROOT, "mrhash_amd", "csrc")
    mesh, extract = open(os.path.join(csrc, "mrh_mesh.h")).read(), open(os.path.join(csrc, "mrh_extract.h")).read()
    assert mesh.count("mesh_cell(floor(") == 3 and extract.count("mesh_cell(std::floor(") == 1
    assert "(int) floor(" not in mesh and "(int32_t) std::floor(" not in extract
    key = open(os.path.join(csrc, "mrh_meshkey.h")).read()
    assert [l for l in key.splitlines() if l.startswith("#include")] == ["#include <cstdint>"]
