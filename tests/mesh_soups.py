"""Hand-built triangle soups for the mesh post-process (MeshExtractor::processTriangles: mrhash_amd/csrc/mrh_mesh.h on the device,
process_triangles in mrh_extract.h on the host, the oracle), and an independent numpy restatement of it.

The restatement is written from mesh_extractor.cpp:9-76, :156-259 and the canonical choice D4, not from the kernels:

  key             eps == 0: the position's bit pattern (-0 and +0 stay apart); else the cell floor((double) p * (1.0 / (double) eps))
                  per coordinate, converted to int32 where it lies in [-2^31, 2^31) and INT32_MIN elsewhere (+-inf included:
                  what the reference's x86-64 build computes; mrhash_amd/csrc/mrh_meshkey.h)
  NaN             a vertex with a NaN coordinate is its own representative, in both modes
  representative  the smallest soup index that carries the key; new indices in the order of first occurrence; V and C are the
                  representative's position and colour
  faces           dropped if two corner indices are equal; after that dropped if the ordered triple occurred before

A marching-cubes soup never holds what these soups are about: equal positions with different colours (every builder colours a soup
vertex by its soup index, so a wrong representative shows in C), NaN / inf / -0 / denormals, cells next to zero, corners of one
triangle in one cell, repeated and rotated faces, whole tiles of dropped faces, chosen vertex counts, more than 1024 tiles.

Builders return (nt, 3) arrays of capi.TRI_DTYPE.  CASES lists every (soup, eps) the tests run; soup() and expected() cache.
"""
from __future__ import annotations

import functools
from typing import Callable, NamedTuple

import numpy as np

from mrhash_amd import capi

INT32_MIN = -(1 << 31)
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
EPS_EXACT = 0.25     # cell arithmetic is exact: answers can be written by hand
EPS_ROUNDED = 0.013  # the eps of the parity tests: 1 / eps and p / eps round
EPS_TINY = 1e-9      # |p| >= 2.147 leaves the int range
EPS_LATTICE = 1.5    # integer coordinates, two or one lattice points per cell and axis, 1 / eps rounds


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def _first_of_group(cols) -> np.ndarray:
    """For rows given as equally long uint32 columns: the smallest row index with the same row.  Two columns are packed into one
    uint64 and replaced by a dense group id before the next column joins (np.unique on rows is ~10 x slower at 10^6 rows)."""
    n = len(cols[0])
    if n == 0:
        return np.zeros(0, np.int64)
    gid = cols[0].astype(np.uint64)
    first = None
    for c in cols[1:]:
        packed = (gid << np.uint64(32)) | c.astype(np.uint64)
        _, first, gid = np.unique(packed, return_index=True, return_inverse=True)  # return_index: the FIRST occurrence (stable sort)
        gid = gid.reshape(-1).astype(np.uint64)
    if first is None:
        _, first, gid = np.unique(gid, return_index=True, return_inverse=True)
    return first[gid.reshape(-1).astype(np.int64)]


def cells(p32: np.ndarray, eps) -> np.ndarray:
    """int32 cell per coordinate for a float32 array, by the rule in the module's header."""
    e = np.float64(np.float32(eps))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(p32.astype(np.float64) * (1.0 / e))
        inside = (q >= -2147483648.0) & (q < 2147483648.0)  # NaN fails both
        return np.where(inside, np.where(inside, q, 0.0).astype(np.int64), INT32_MIN).astype(np.int32)


def representatives(soup: np.ndarray, eps) -> np.ndarray:
    """rep[i] = the soup vertex that stands for soup vertex i."""
    P = np.ascontiguousarray(soup["p"]).reshape(-1, 3)
    n = len(P)
    keys = P.view(np.uint32) if float(eps) == 0.0 else cells(P, eps).view(np.uint32)
    rep = np.arange(n, dtype=np.int64)
    ok = np.flatnonzero(~np.isnan(P).any(axis=1))
    rep[ok] = ok[_first_of_group([keys[ok, 0], keys[ok, 1], keys[ok, 2]])]
    return rep


def process(soup: np.ndarray, eps):
    """(V f64[nv, 3], F i32[nf, 3], C f64[nv, 3]) of a soup."""
    soup = np.ascontiguousarray(soup, dtype=capi.TRI_DTYPE).reshape(-1, 3)
    P = soup["p"].reshape(-1, 3)
    Col = soup["c"].reshape(-1, 3)
    n = len(P)
    rep = representatives(soup, eps)
    is_first = rep == np.arange(n)
    new_index = np.cumsum(is_first) - 1
    corner = new_index[rep].astype(np.int32).reshape(-1, 3)
    V = P[is_first].astype(np.float64)
    Cc = Col[is_first].astype(np.float64)
    proper = np.flatnonzero((corner[:, 0] != corner[:, 1]) & (corner[:, 0] != corner[:, 2]) & (corner[:, 1] != corner[:, 2]))
    f = corner[proper].view(np.uint32)
    new_face = _first_of_group([f[:, 0], f[:, 1], f[:, 2]]) == np.arange(len(proper))
    F = np.ascontiguousarray(corner[proper[new_face]], dtype=np.int32).reshape(-1, 3)
    return np.ascontiguousarray(V).reshape(-1, 3), F, np.ascontiguousarray(Cc).reshape(-1, 3)


# ---- building blocks ------------------------------------------------------------------------------------------------------------

def colours(n: int, start: int = 0) -> np.ndarray:
    """The colour of soup vertex i: a function of i alone, exact in float32 up to 2^24 vertices."""
    i = np.arange(start, start + n, dtype=np.int64)
    return np.stack([i, 0.5 * i, -(i % 1024)], axis=1).astype(np.float32)


def soup_of(points) -> np.ndarray:
    """Soup vertices (n, 3), n a multiple of 3, in soup order -> the soup, coloured by soup index."""
    P = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    assert len(P) % 3 == 0
    s = np.zeros(len(P), capi.TRI_DTYPE)
    s["p"] = P
    s["c"] = colours(len(P))
    return s.reshape(-1, 3)


def xs(values) -> np.ndarray:
    """Points (x, 0, 0)."""
    v = np.asarray(values, np.float32)
    return np.stack([v, np.zeros_like(v), np.zeros_like(v)], axis=1)


def below(x) -> np.float32:
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def distinct_points(n: int, start: int = 0) -> np.ndarray:
    i = np.arange(start, start + n, dtype=np.int64)
    return np.stack([i, i % 7, -(i % 3)], axis=1).astype(np.float32)


# ---- small soups, any mode ------------------------------------------------------------------------------------------------------

def single(eps=0.0):
    return soup_of([[0, 0, 0], [1, 0, 0], [0, 1, 0]])


def all_distinct_tile(eps=0.0):
    """513 distinct vertices: the 512-vertex LDS tile at its highest load, and one vertex alone in tile 1."""
    return soup_of(distinct_points(513))


def one_key(eps=0.0):
    """2048 triangles, every corner at one position: one vertex, no face, maximal contention on one slot."""
    return soup_of(np.tile(np.array([[1, 2, 3]], np.float32), (2048 * 3, 1)))


STRADDLE_SAME = {512: 511, 1600: 5, 1700: 5, 1031: 1030}  # soup vertex -> the earlier vertex it repeats


def straddle(eps=0.0):
    """Repeats across a tile edge (511 | 512), from a later tile back to an early one, twice out of one tile (5 <- 1600, 1700), and
    next to each other (1030, 1031)."""
    P = distinct_points(1704)
    for later, first in STRADDLE_SAME.items():
        P[later] = P[first]
    return soup_of(P)


def reversed_repeats(eps=0.0):
    """4 tiles of distinct vertices, then the same positions in reverse order (other colours: the soup index), twice."""
    A = distinct_points(2048)
    return soup_of(np.concatenate([A, A[::-1], A[::-1]]))


def signed_zero(eps=0.0):
    return soup_of([[0.0, 1, 2], [-0.0, 1, 2], [5, 5, 5], [-0.0, 1, 2], [0.0, 1, 2], [6, 6, 6]])


def nan(eps=0.0):
    """Quiet NaN in x, in y, in z, in all three; two bit-identical NaN vertices; one of them again in a later triangle."""
    q = QNAN
    return soup_of([[q, 1, 2], [1, q, 2], [1, 2, q],
                    [q, q, q], [q, q, q], [0, 0, 0],
                    [q, 1, 2], [0, 0, 0], [7, 7, 7]])


SPECIAL_VALUES = np.array([np.inf, -np.inf, 1e-40, np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1.0,
                           np.nextafter(np.float32(1.0), np.float32(2.0)), -1e-40, 0.0], np.float32)


def specials(eps=0.0):
    """+-inf, denormals, FLT_MAX, the smallest normal, 1.0 and its neighbour, in every coordinate; then all nine vertices again,
    rotated by one."""
    v = SPECIAL_VALUES
    A = np.stack([v, np.roll(v, -1), np.roll(v, -2)], axis=1)
    return soup_of(np.concatenate([A, np.roll(A, -1, axis=0)]))


def low_bits(eps=0.0):
    """4096 vertices whose keys differ only in the low mantissa bits of x (then the first two again: a multiple of 3)."""
    i = np.arange(4098, dtype=np.uint32) % 4096
    x = (np.uint32(0x3F800000) + i).view(np.float32)
    return soup_of(np.stack([x, np.ones_like(x), np.full_like(x, 2.0)], axis=1))


# ---- small soups about the cells ----------------------------------------------------------------------------------------------------

def cells_negative(eps):
    """Cells 0, -1, 1, -2 and a second point in cells 0 and -1: floor and truncation differ at -0.5 eps and -0.25 eps."""
    e = np.float32(eps)
    P = xs(np.array([0.5, -0.5, 1.5, -1.5, 0.25, -0.25], np.float32) * e)
    P[:, 1:] = np.float32(0.5) * e
    return soup_of(P)


CELL_EDGE_KS = (-2, -1, 0, 1, 2)


def cell_edges(eps):
    """k eps, the float just below it, and the middles of the two cells they fall into."""
    e = np.float32(eps)
    pts = []
    for k in CELL_EDGE_KS:
        pts += [np.float32(k) * e, below(np.float32(k) * e), np.float32(k + 0.5) * e, np.float32(k - 0.5) * e]
    pts.append(np.float32(100) * e)
    return soup_of(xs(pts))


def first_wins(eps):
    """Distinct positions and colours in one cell: triangle 0 lies in cell (0, 0, 0) altogether, triangles 1 and 2 visit the cells
    (0, 0, 0), (1, 0, 0), (0, 1, 0) in two orders."""
    e = np.float32(eps)
    return soup_of(np.array([[0.1, 0.2, 0.3], [0.9, 0.8, 0.7], [0.5, 0.5, 0.5],
                             [0.4, 0.4, 0.4], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5],
                             [1.9, 0.1, 0.1], [0.1, 1.9, 0.9], [0.6, 0.6, 0.6]], np.float32) * e)


def degenerate_by_merge(eps):
    """Two corners of triangle 0 in one cell (dropped with eps, kept without); triangle 1 is an ordinary one."""
    e = np.float32(eps) if float(eps) != 0.0 else np.float32(EPS_EXACT)
    return soup_of(np.array([[0.1, 0, 0], [0.6, 0, 0], [5.25, 0, 0], [7.5, 0, 0], [5.5, 0, 0], [9.5, 0, 0]], np.float32) * e)


def out_of_range(eps):
    """eps = 1e-9: +-3, +-2.5 and +-inf leave the int range (cell INT32_MIN, one vertex); 2.0, 1.0 and 0.0 are in range."""
    inf = np.inf
    return soup_of(xs([3, 2.0, 0.0, -3, 2.0, 0.0, 2.5, 0.0, 2.0, -2.5, inf, -inf, inf, 0.0, 2.0, -inf, 1.0, 0.0]))


# ---- faces ----------------------------------------------------------------------------------------------------------------------

def _distinct_triangles(nt: int, start: int = 0) -> np.ndarray:
    """(nt, 3, 3) points: triangle t = (t, 0, 0), (t, 1, 0), (t, 0, 1), shifted by start."""
    t = np.arange(start, start + nt, dtype=np.float32)
    z, o = np.zeros_like(t), np.ones_like(t)
    return np.stack([np.stack([t, z, z], 1), np.stack([t, o, z], 1), np.stack([t, z, o], 1)], axis=1)


REPEATED_AT = (300, 5000)


def repeated_face(eps=0.0):
    T = _distinct_triangles(5001)
    for t in REPEATED_AT:
        T[t] = T[0]
    return soup_of(T.reshape(-1, 3))


def rotated_face(eps=0.0):
    a, b, c = [0, 0, 0], [1, 0, 0], [0, 1, 0]
    return soup_of([a, b, c, b, c, a, a, c, b])


def degenerate_repeat(eps=0.0):
    a, b, c = [0, 0, 0], [1, 0, 0], [0, 1, 0]
    return soup_of([a, a, b, a, a, b, a, b, c])


def one_face_many(eps=0.0):
    return soup_of(np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (4096, 1)))


FACE_TILE = 256


def face_tiles(eps=0.0):
    """256-face tiles: kept | repeats of face 0 | kept | degenerate | every other one a repeat | 100 kept."""
    T = _distinct_triangles(5 * FACE_TILE + 100)
    T[FACE_TILE: 2 * FACE_TILE] = T[0]
    T[3 * FACE_TILE: 4 * FACE_TILE, 2] = T[3 * FACE_TILE: 4 * FACE_TILE, 0]
    T[4 * FACE_TILE + 1: 5 * FACE_TILE: 2] = T[1]
    return soup_of(T.reshape(-1, 3))


# ---- sizes ----------------------------------------------------------------------------------------------------------------------

VERTEX_TILES_NT = 174763  # 524 289 soup vertices: 1025 vertex tiles of 512, k_tile_scan's second trip
FACE_TILES_NT = 262145    # 1025 face tiles of 256


def lattice(nt: int, eps=0.0):
    """Integer lattice points, negative and positive, drawn with repeats: soup vertex i draws from the first i / 2 + 32 points, so about
    a third of every tile are first occurrences and the rest repeat points of any earlier tile; an eighth of the triangles is copied
    from other triangles.  Repeats, first occurrences and dropped faces in every tile."""
    rng = np.random.default_rng(nt)
    n = 3 * nt
    J = (rng.random(n) * (np.arange(n) // 2 + 32)).astype(np.int64).reshape(nt, 3)
    src, dst = rng.integers(0, nt, nt // 8), rng.integers(0, nt, nt // 8)
    J[dst] = J[src]
    j = J.reshape(-1)
    return soup_of(np.stack([j % 128 - 64, (j // 128) % 128 - 64, j // 16384 - 8], axis=1).astype(np.float32))


NV_EXACT = (5461, 5462, 16384, 16385)  # nv * 12 bytes on both sides of one and of three 64 KiB staging chunks


def nv_exact(nv: int, eps=0.0):
    """Exactly nv merged vertices: soup vertex i lies at lattice point i % nv."""
    n = (nv + 300 + 2) // 3 * 3
    i = np.arange(n, dtype=np.int64) % nv
    return soup_of(np.stack([i % 128, i // 128, np.zeros_like(i)], axis=1).astype(np.float32))


# ---- the cases ------------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    build: Callable
    args: tuple
    eps: float

    @property
    def id(self) -> str:
        return self.name + "".join(f"-{a}" for a in self.args) + f"-eps{self.eps:g}"


ANY_MODE = (single, all_distinct_tile, one_key, straddle, reversed_repeats, signed_zero, nan, specials, low_bits, repeated_face,
            rotated_face, degenerate_repeat, one_face_many, face_tiles)
CELL_SOUPS = (cells_negative, cell_edges, first_wins, degenerate_by_merge)

SMALL_CASES = ([Case(b.__name__, b, (), 0.0) for b in ANY_MODE]
               + [Case("degenerate_by_merge", degenerate_by_merge, (), 0.0)]
               + [Case(b.__name__, b, (), e) for e in (EPS_EXACT, EPS_ROUNDED) for b in CELL_SOUPS]
               + [Case("nan_eps", nan, (), e) for e in (EPS_EXACT, EPS_ROUNDED)]
               + [Case(b.__name__, b, (), EPS_EXACT) for b in (straddle, reversed_repeats, one_key, specials, signed_zero, face_tiles)]
               + [Case("specials", specials, (), EPS_TINY), Case("out_of_range", out_of_range, (), EPS_TINY)]
               + [Case("nv_exact", nv_exact, (nv,), 0.0) for nv in NV_EXACT])
LARGE_CASES = [Case("lattice", lattice, (nt,), e) for nt in (VERTEX_TILES_NT, FACE_TILES_NT) for e in (0.0, EPS_LATTICE)]
CASES = SMALL_CASES + LARGE_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


@functools.lru_cache(maxsize=None)
def _soup(name, build, args, eps):
    s = build(*args, eps)
    s.setflags(write=False)
    return s


def soup(case: Case) -> np.ndarray:
    return _soup(*case)


@functools.lru_cache(maxsize=None)
def _expected(case: Case):
    out = process(soup(case), case.eps)
    for a in out:
        a.setflags(write=False)
    return out


def expected(case: Case):
    """(V, F, C) of the restatement, computed once per process and read-only."""
    return _expected(case)


def assert_same_mesh(got, want, what: str):
    """V, F, C byte for byte: no tolerance, no skipped row."""
    for name, a, b in zip("VFC", got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name} is {a.dtype}{a.shape}, expected {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            rows = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
            raise AssertionError(f"{what}: {name} differs in {len(rows)} of {len(a)} rows, first rows {rows[:6].tolist()}:\n{a[rows[:3]]}\n"
                                 f"expected\n{b[rows[:3]]}")


def mesh_params(eps) -> capi.Params:
    """The post-process reads vertices_merging_threshold alone; a small map keeps the context cheap."""
    return capi.Params(sdf_truncation=0.08, virtual_voxel_size=0.02, vertices_merging_threshold=float(eps), num_sdf_blocks=1024)


def run_engine(e: capi.Engine, s: np.ndarray):
    e.process_triangles(s)
    return e.extract_mesh()


# ---- hand-built runs for mrh_process_triangle_runs --------------------------------------------------------------------------------

def runs():
    """(descs, counts, soup): 8193 runs of one triangle (k_permute_runs' grid is 8192 workgroups), zero-count runs, two pairs of runs
    at one block position, one run of 100 triangles, blocks in scrambled order, the last run ending at nt."""
    rng = np.random.default_rng(7)
    n_single = 8193
    pos = np.stack([np.arange(n_single) % 32 - 16, (np.arange(n_single) // 32) % 32 - 16, np.arange(n_single) // 1024 - 4], axis=1)
    pos = pos[rng.permutation(n_single)]
    counts = np.ones(n_single, np.uint32)
    extra_pos = np.array([[100, 0, 0], [-100, 5, 5], [3, 3, 3], [3, 3, 3], [0, 0, 0], [50, 50, 50], [-16, -16, -4], [200, 0, 0]])
    extra_counts = np.array([100, 0, 4, 2, 0, 7, 3, 5], np.uint32)  # (3, 3, 3) twice; (0, 0, 0) and (-16, -16, -4) also among the single runs
    at = np.array([0, 17, 4000, 4001, 5000, 8000, 8100, n_single])  # where the extras go in; the last one ends the input
    pos = np.insert(pos, at, extra_pos, axis=0)
    counts = np.insert(counts, at, extra_counts)
    assert counts[-1] == 5 and counts[0] == 100
    descs = np.zeros(len(pos), capi.DESC_DTYPE)
    descs["x"], descs["y"], descs["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    descs["resolution"] = np.arange(len(pos)) % 2  # rides along, no part of the order
    nt = int(counts.sum())
    j = rng.integers(0, nt, size=3 * nt)  # repeats across runs
    s = soup_of(np.stack([j % 64, (j // 64) % 64, j // 4096], axis=1).astype(np.float32))
    return descs, counts, s


def permute_runs(descs, counts, s):
    """The canonical order in numpy: runs sorted by (x, y, z), equal positions in input order."""
    order = np.lexsort((descs["z"], descs["y"], descs["x"]))  # stable
    start = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    idx = np.concatenate([np.arange(start[i], start[i] + counts[i]) for i in order]).astype(np.int64)
    return descs[order], counts[order], s[idx]
