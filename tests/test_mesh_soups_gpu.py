"""The mesh post-process of the HIP library on the hand-built soups of tests/mesh_soups.py, BYTE for byte against the numpy
restatement (tests/test_mesh_soups.py pins the restatement to a literal transliteration, to hand-written answers and to the oracle).

Every soup goes through Engine.process_triangles on the three ways out of the post-process: the eight kernels of mrh_mesh.h with
the fp32 staging of k_stage_out (default), the same kernels with doubles over the link (MRH_MESH_F64_LINK=1) and the host
restatement of mrh_extract.h (MRH_MESH_HOST=1).  The switches are read when the context is made.  Then one context takes a
sequence of soups that shrink and grow (the speculative read-back into the last soup's buffers, the index tables the last
read-back left empty, MRH_MESH_FILL=1 against it), and mrh_process_triangle_runs takes hand-built runs.

An error return of the device path ends the session: nothing more is started on a device that may have faulted.
"""
import numpy as np
import pytest

import mesh_soups as ms
from mrhash_amd import capi, hipmem

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "f64-link": "MRH_MESH_F64_LINK", "host": "MRH_MESH_HOST"}


def _engine(hip, monkeypatch, eps, path="staged"):
    switch = PATHS[path]
    if switch:
        monkeypatch.setenv(switch, "1")
    try:
        return capi.Engine(hip, ms.mesh_params(eps))
    finally:
        if switch:
            monkeypatch.delenv(switch)


def _guarded(fn, *args):
    try:
        return fn(*args)
    except capi.MrhError as err:
        pytest.exit(f"HIP library error on a hand-built soup, session ended: {err}", returncode=3)


# ---- every soup, three paths ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("c", ms.CASES, ids=lambda c: c.id)
def test_soup(hip, monkeypatch, c, path):
    e = _engine(hip, monkeypatch, c.eps, path)
    got = _guarded(ms.run_engine, e, ms.soup(c))
    print(f"{c.id} [{path}]: {len(ms.soup(c))} triangles -> {len(got[0])} vertices, {len(got[1])} faces")
    ms.assert_same_mesh(got, ms.expected(c), f"{c.id} [{path}]")
    e.close()


@pytest.mark.parametrize("path", PATHS)
def test_no_triangles_after_some_gives_three_empty_arrays(hip, monkeypatch, path):
    e = _engine(hip, monkeypatch, 0.0, path)
    c = ms.BY_ID["straddle-eps0"]
    ms.assert_same_mesh(_guarded(ms.run_engine, e, ms.soup(c)), ms.expected(c), c.id)
    V, F, C = _guarded(ms.run_engine, e, np.zeros((0, 3), capi.TRI_DTYPE))
    assert (V.shape, F.shape, C.shape) == ((0, 3), (0, 3), (0, 3))
    ms.assert_same_mesh(_guarded(ms.run_engine, e, ms.soup(c)), ms.expected(c), c.id + " again")
    e.close()


# ---- one context, soups that shrink and grow ------------------------------------------------------------------------------------------

def _sequence(eps):
    by = {(c.name, c.args): c for c in ms.CASES if c.eps == 0.0}
    order = [("lattice", (ms.VERTEX_TILES_NT,)), ("single", ()), ("straddle", ()), ("one_key", ()), ("lattice", (ms.FACE_TILES_NT,)), ("all_distinct_tile", ())]
    return [by[k]._replace(eps=eps) for k in order]


@pytest.fixture(scope="module")
def fresh_results(hip):
    """Each soup of the sequence through a context of its own (default path), once per eps."""
    out = {}
    for eps in (0.0, ms.EPS_LATTICE):
        for c in _sequence(eps):
            with capi.Engine(hip, ms.mesh_params(eps)) as e:
                out[c.id] = _guarded(ms.run_engine, e, ms.soup(c))
            ms.assert_same_mesh(out[c.id], ms.expected(c), f"{c.id} [fresh context]")
    return out


@pytest.mark.parametrize("eps", [0.0, ms.EPS_LATTICE], ids=["exact", "eps1.5"])
@pytest.mark.parametrize("variant", ["default", "fill", "twice"])
def test_context_reuse(hip, monkeypatch, fresh_results, variant, eps):
    """1025 vertex tiles -> 1 triangle -> ... -> 1025 face tiles -> 171 triangles in ONE context: every read-back goes
    speculatively into the buffers of the soup before it (too large, then too small: the second launch), the index tables are
    those the last read-back cleared for ITS size, and the scratch arena moves when it grows.  `fill`: MRH_MESH_FILL=1 fills the
    tables every time.  `twice`: every soup a second time, into staging that fits exactly."""
    if variant == "fill":
        monkeypatch.setenv("MRH_MESH_FILL", "1")
    e = capi.Engine(hip, ms.mesh_params(eps))
    for c in _sequence(eps):
        for k in range(2 if variant == "twice" else 1):
            ms.assert_same_mesh(_guarded(ms.run_engine, e, ms.soup(c)), fresh_results[c.id], f"{c.id} in a used context ({variant}, call {k})")
    e.close()


# ---- mrh_process_triangle_runs ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run_case():
    descs, counts, s = ms.runs()
    d, n, permuted = ms.permute_runs(descs, counts, s)
    assert len(descs) == 8193 + 8 and (counts == 0).sum() == 2 and counts.max() == 100
    return descs, counts, s, d, n, permuted, ms.process(permuted, 0.0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("source", ["host", "device"])
def test_triangle_runs(hip, monkeypatch, run_case, source, path):
    """Scrambled blocks, zero-count runs, two runs at one position (input order), a run of 100, 8193 runs of one triangle
    (k_permute_runs' grid-stride loop), the last run ending at nt; the soup from host memory and from the caller's device memory."""
    descs, counts, s, d, n, permuted, want = run_case
    e = _engine(hip, monkeypatch, 0.0, path)
    if source == "device":
        # the caller's own device memory, as the suite allocates it everywhere: a torch tensor needs torch initialised before the
        # library is loaded (mrhash_amd/_runtime.py), which a session that shares one `hip` fixture cannot promise
        keep = hipmem.DeviceBuffer.from_numpy(s)
        ptr = keep.ptr
    else:
        keep, ptr = s, s.ctypes.data
    _guarded(e.process_triangle_runs, descs, counts, ptr, len(s), source == "device")
    mptr, mn, mdev = e.triangles_device()
    assert mn == len(s) and mdev
    merged = np.frombuffer(hipmem.read(mptr, mn * 72), dtype=capi.TRI_DTYPE).reshape(mn, 3)
    assert merged.tobytes() == permuted.tobytes(), "the permuted soup"
    td, tc = e.triangle_blocks()
    assert td.tobytes() == d.tobytes() and tc.tobytes() == n.tobytes()
    ms.assert_same_mesh(e.extract_mesh(), want, f"runs from {source} memory [{path}]")
    del keep
    e.close()


def test_triangle_runs_refuses_counts_that_do_not_add_up(hip, run_case):
    descs, counts, s = run_case[:3]
    with capi.Engine(hip, ms.mesh_params(0.0)) as e:
        with pytest.raises(capi.MrhError, match=f"the counts add up to {len(s)} triangles, {len(s) - 1} given"):
            e.process_triangle_runs(descs, counts, s.ctypes.data, len(s) - 1, False)
        V, F, C = e.extract_mesh()
        assert len(V) == 0 and len(F) == 0 and len(C) == 0
