"""CPU half of render-free tracking (include/mrhash_sdftrack.h): the header and its binding; the restatement of
tests/sdftrack_ref.py on the corner view, from the truth and from a start 3.4 degrees and 87 mm off; the order-freedom of the sums;
the depth form against the points form; and the coverage conditions of the GPU comparisons (tests/test_sdftrack_gpu.py), asserted
here on the restatement alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as ar
import remap_ref as rm
import sdftrack_ref as sr
import track_ref as tr
from mrhash_amd import capi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What the binary32 restatement measures on the corner view after ten iterations, from the perturbed start (3.44 degrees, 86.6 mm)
# and from the truth alike: rms of e, translation and rotation error.  After three iterations from the start it stands at
# 2.135 mm rms, 1.082 mm and 0.0095 degrees.  The bias comes from the kinks of the trilinear field at the plane intersections.
VIEW_RMS, VIEW_T_ERR, VIEW_DEG = 0.0020366, 0.0010678, 0.011567


# ---- header and binding ------------------------------------------------------------------------------------------------------------

def test_sdftrack_header_is_plain_c_and_bound():
    """include/mrhash_sdftrack.h is a C header of its own: a C compiler accepts it by itself, capi binds every symbol it declares with
    a struct of the C size, and mrhash_hip.h, whose symbols tests/test_abi.py pins, declares none of them."""
    inc = os.path.join(ROOT, "include")
    path = os.path.join(inc, "mrhash_sdftrack.h")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-x", "c", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mrh_[a-z_]+)\s*\(", hdr))) == sorted(capi.SDFTRACK_SYMBOLS)
    assert re.findall(r'#include\s+"([^"]+)"', hdr) == ["mrhash_track.h"]
    for other in sorted(os.listdir(inc)):
        if other != "mrhash_sdftrack.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, other)).read(), flags=re.S)  # comments may point here
            assert not re.search(r"mrh_sdftrack|mrh_track_\w+_sdf", text), other
    assert not set(capi.SDFTRACK_SYMBOLS) & set(capi.ABI_SYMBOLS)
    lib = capi.load_hip()
    for name in capi.SDFTRACK_SYMBOLS:
        assert hasattr(lib, name), f"libmrhash_hip.so does not export {name}"
    P = capi.MrhSdftrackParams
    assert C.sizeof(P) == 48 and (P.rows.offset, P.min_depth.offset, P.band.offset, P.iterations.offset, P.min_pixels.offset, P.reserved.offset) == (16, 24, 32, 36, 40, 44)


# ---- the corner view ---------------------------------------------------------------------------------------------------------------

def test_the_corner_view_sees_all_three_planes_with_every_pixel():
    R, t = sr.corner_view()
    assert np.allclose(R.astype(np.float64).T @ R.astype(np.float64), np.eye(3), atol=1e-6) and np.linalg.det(R.astype(np.float64)) > 0.99
    depth = sr.corner_depth(R, t)
    assert depth.shape == (48, 64) and np.all(depth > sr.VIEW_NEAR) and np.all(depth <= sr.VIEW_FAR)
    valid, p = sr.depth_samples(depth, sr.VIEW_K, sr.VIEW_NEAR, sr.VIEW_FAR)
    assert valid.all() and len(p) == 3072
    W = p.astype(np.float64) @ R.astype(np.float64).T + t.astype(np.float64)
    dist = W @ ar.CORNER_N.T - ar.CORNER_O
    assert np.abs(dist.min(axis=-1)).max() < 1e-6            # every pixel lies on the corner's surface
    assert np.all(np.bincount(dist.argmin(axis=-1), minlength=3) > 300)  # ... and every plane has its share
    vertex = np.linalg.solve(ar.CORNER_N, ar.CORNER_O)
    assert abs(float(np.linalg.norm(t.astype(np.float64) - vertex)) - 1.0) < 1e-6


@pytest.mark.parametrize("name", ["start", "truth"])
def test_corner_view_converges(name):
    """From 3.44 degrees and 86.6 mm off, and from the truth, after three iterations and after ten: rms and both errors within twice
    what the restatement measured when the constants above were taken (the factor covers the fixed-point rounding between starts)."""
    s = sr.destination("truth")
    R0, t0 = (s["R"], s["t"]) if name == "start" else (s["R_true"], s["t_true"])
    t_0, a_0 = tr.pose_errors(R0, t0, s["R_true"], s["t_true"])
    if name == "start":
        assert 3.4 < a_0 < 3.5 and 0.086 < t_0 < 0.087
    m = rm.Source(s["params"], s["blocks"])
    for iterations in (3, 10):
        r = sr.track_depth(s["params"], m, s["depth"], s["K"], sr.VIEW_NEAR, sr.VIEW_FAR, R0, t0, iterations=iterations)
        t_1, a_1 = tr.pose_errors(r["R"], r["t"], s["R_true"], s["t_true"])
        print(f"{name}, {iterations} iterations: {a_0:.4f} deg, {1e3 * t_0:.2f} mm -> {a_1:.5f} deg, {1e3 * t_1:.3f} mm; rms {r['rms']:.7f}, {r['pixels']} of {r['valid']} pixels")
        assert r["status"] == sr.TRACK_OK and r["iterations_done"] == iterations
        assert r["valid"] == 3072 and r["pixels"] == 3072  # twelve rows of the partial slab, every pixel within the band
        assert r["rms"] <= 2 * VIEW_RMS and t_1 <= 2 * VIEW_T_ERR and a_1 <= 2 * VIEW_DEG


def test_sums_do_not_depend_on_the_point_order():
    s = sr.destination("truth")
    m = rm.Source(s["params"], s["blocks"])
    valid, p = sr.depth_samples(s["depth"], s["K"], sr.VIEW_NEAR, sr.VIEW_FAR)
    want = sr.linearise(m, valid, p, s["R"], s["t"], 0.15, sr.VIEW_FAR)
    rng = np.random.default_rng(5)
    for order in (np.arange(len(p))[::-1], rng.permutation(len(p))):
        assert np.array_equal(sr.linearise(m, valid, p, s["R"], s["t"], 0.15, sr.VIEW_FAR, order=order), want)
        v2, p2 = sr.point_samples(p[order], sr.VIEW_NEAR, sr.VIEW_FAR)
        assert np.array_equal(sr.linearise(m, v2, p2, s["R"], s["t"], 0.15, sr.VIEW_FAR), want)  # a shuffled cloud
    assert want[28] == 3072 and not want[29:].any()


def test_the_points_form_fed_the_valid_pixels_gives_the_depth_forms_sums():
    """p_c of the valid pixels as a cloud: the same a = R32 p, so the same rows, bit for bit — sums and poses.  The largest range of a
    pixel (|p_c| <= 1.2 here) stays below max_depth = 3, so the range gate of the points form passes what the depth gate passed;
    the image carries invalid pixels of every kind, which the cloud does not get."""
    s = sr.destination("truth")
    depth = dirty_depth(s["depth"])
    valid, p = sr.depth_samples(depth, s["K"], sr.VIEW_NEAR, sr.VIEW_FAR)
    assert 0 < valid.sum() < len(valid)
    cloud = p[valid]
    v2, _ = sr.point_samples(cloud, sr.VIEW_NEAR, sr.VIEW_FAR)
    assert v2.all()
    for iterations in (1, 4):
        a = sr.track_depth(s["params"], s["blocks"], depth, s["K"], sr.VIEW_NEAR, sr.VIEW_FAR, s["R"], s["t"], iterations=iterations)
        b = sr.track_points(s["params"], s["blocks"], cloud, sr.VIEW_NEAR, sr.VIEW_FAR, s["R"], s["t"], iterations=iterations)
        assert not sr.same_result(a, b) and a["pixels"] > 2000


def dirty_depth(depth):
    """The image with a 0, a negative value, a NaN, both infinities and a value beyond max_depth among the valid pixels, and a row
    of zeros."""
    d = np.array(depth, F).copy()
    d[3, 5], d[7, 60], d[20, 31], d[21, 32], d[22, 33], d[40, 2] = 0.0, -1.0, np.nan, np.inf, -np.inf, F(sr.VIEW_FAR) + F(0.5)
    d[30, :] = 0.0
    return d


def test_invalid_inputs_are_dropped_at_step_one_and_nothing_is_lost_with_the_pose():
    s = sr.destination("truth")
    d = dirty_depth(s["depth"])
    valid, _ = sr.depth_samples(d, s["K"], sr.VIEW_NEAR, sr.VIEW_FAR)
    assert valid.sum() == 3072 - 6 - 64
    r = sr.track_depth(s["params"], s["blocks"], d, s["K"], sr.VIEW_NEAR, sr.VIEW_FAR, s["R"], s["t"], iterations=2)
    assert r["status"] == sr.TRACK_OK and r["pixels"] == r["valid"] == 3002
    pts = np.array([[0, 0, 0], [np.nan, 0, 1], [1, np.inf, 0], [0.01, 0.01, 0.01], [0, 0, 9.0], [0.3, 0.4, 0.5]], F)
    v, _ = sr.point_samples(pts, sr.VIEW_NEAR, sr.VIEW_FAR)
    assert v.tolist() == [False, False, False, False, False, True]
    for r in (sr.track_depth(s["params"], s["blocks"], np.zeros((48, 64), F), s["K"], sr.VIEW_NEAR, sr.VIEW_FAR, s["R"], s["t"]),
              sr.track_points(s["params"], s["blocks"], np.zeros((0, 3), F), sr.VIEW_NEAR, sr.VIEW_FAR, s["R"], s["t"]),
              sr.track_points(s["params"], s["blocks"], pts[:5], sr.VIEW_NEAR, sr.VIEW_FAR, s["R"], s["t"])):
        assert r["status"] == sr.TRACK_LOST and r["iterations_done"] == 0 and r["pixels"] == 0 and r["rms"] == 0.0 and not r["sums"].any()
        assert rm.same_bits(r["R"], s["R"]) and rm.same_bits(r["t"], s["t"])


# ---- the scenes of the GPU comparisons ---------------------------------------------------------------------------------------------

def test_every_gate_rejects_somewhere_and_converging_scenes_keep_half_of_their_pixels():
    """Over the destinations and the two gate scenes, two iterations each as the GPU test runs them: the range bound, the corners,
    the band and the lever each reject a valid sample somewhere; an accepted row stays inside the fixed-point range; a scene that
    is expected to converge accepts at least half of its valid pixels in the last linearisation and ends nearer the truth."""
    total = {k: 0 for k in sr.GATES}
    for name in sr.DESTINATIONS + sr.GATE_SCENES:
        s = sr.destination(name)
        r = sr.run_destination(name, iterations=2)
        print(name, r["status"], r["iterations_done"], r["pixels"], "of", r["valid"], r["rejected"])
        for k in sr.GATES:
            total[k] += r["rejected"][k]
        assert r["valid"] >= 64
        valid, p = sr.depth_samples(s["depth"], s["K"], sr.VIEW_NEAR, sr.VIEW_FAR)
        band = sr.defaults(s["kw"].get("band", 0.0), 0, 0, s["params"]["sdf_truncation"])[0]
        ok, Jt, et, _ = sr.sample_terms(rm.Source(s["params"], s["blocks"]), valid, p, s["R"], s["t"], band, sr.VIEW_FAR)
        assert np.abs(Jt).max(initial=0) < 32768 and np.abs(et).max(initial=0) <= (1 << 18), name
        if name in sr.CONVERGING:
            assert r["status"] == sr.TRACK_OK and r["pixels"] >= 0.5 * r["valid"], name
            (t_0, a_0), (t_1, a_1) = tr.pose_errors(s["R"], s["t"], s["R_true"], s["t_true"]), tr.pose_errors(r["R"], r["t"], s["R_true"], s["t_true"])
            assert t_1 < t_0 and a_1 < a_0, name
        if name in sr.LOST:
            assert r["status"] == sr.TRACK_LOST and r["iterations_done"] == 0
            assert rm.same_bits(r["R"], s["R"]) and rm.same_bits(r["t"], s["t"])
    print(total)
    assert all(total[k] > 0 for k in sr.GATES), total
    beyond, plane = sr.run_destination("beyond"), sr.run_destination("plane")
    assert beyond["pixels"] == 0 and beyond["rejected"]["range"] == beyond["valid"] == 3072
    assert plane["pixels"] >= 64 and tr.solve(plane["sums"], sr.VIEW_FAR, 64) is None  # enough pixels: it is the pivot that fails
    few = sr.run_destination("truth", min_pixels=1000000)
    assert few["status"] == sr.TRACK_LOST and few["iterations_done"] == 0 and 64 <= few["pixels"] < 1000000
    assert 0 < ar.n_coarse(sr.destination("adaptive_dst")["blocks"]) < len(sr.destination("adaptive_dst")["blocks"])
