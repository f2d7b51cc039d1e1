"""bench.py's options and output files, without a GPU: what a plain run does by default, --steps / --warmup checks, the frames of a
run longer than one orbit, and the files --dump-outputs writes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from mrhash_amd import capi, synth  # noqa: E402


def test_a_plain_run_is_the_default_and_full_is_asked_for():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs == ""
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "x"], ["--multi", "--dump-outputs", "x"]])
def test_arguments_a_run_cannot_honour_are_refused(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_a_run_longer_than_the_orbit_repeats_its_frames(monkeypatch):
    monkeypatch.setattr(bench, "ORBIT_FRAMES", 3)
    frames = bench.replica_orbit(5)
    assert len(frames) == 3
    scene = synth.replica_room()
    for f, (t, q) in zip(frames, synth.orbit_poses(3)):  # the threaded render is the serial one
        g = synth.render(scene, synth.REPLICA_640, t, q, depth_scaling=6553.5)
        assert np.array_equal(f.depth, g.depth) and np.array_equal(f.rgb, g.rgb) and np.array_equal(f.t, g.t)


def _fake_map(n, seed=1):
    rng = np.random.default_rng(seed)
    descs = np.zeros(n, capi.DESC_DTYPE)
    descs["x"], descs["y"], descs["z"] = np.arange(n), rng.integers(-50, 50, n), rng.integers(-50, 50, n)
    vox = np.zeros((n, 512), capi.VOXEL_DTYPE)
    vox["sdf"] = rng.standard_normal((n, 512)).astype(np.float32)
    vox["sum_squared"] = rng.random((n, 512)).astype(np.float32)
    vox["weight"] = rng.integers(0, 3, (n, 512))
    vox["rgb"] = rng.integers(0, 256, (n, 512, 3))
    return descs, vox


def test_dumped_outputs_are_float_arrays_of_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BLOCKS", 16)
    monkeypatch.setattr(bench, "DUMP_MAX_BLOCKS", 100)
    for n in (40, 300):
        descs, vox = _fake_map(n)
        sizes = bench.dump_outputs(str(tmp_path / f"a{n}"), descs, vox)
        bench.dump_outputs(str(tmp_path / f"b{n}"), descs, vox)
        assert sum(sizes.values()) <= 64 << 20
        names = sorted(fn for fn in os.listdir(tmp_path / f"a{n}"))
        assert names == sorted(k + ".npy" for k in sizes)
        out = {fn[:-4]: np.load(tmp_path / f"a{n}" / fn) for fn in names}
        again = {fn[:-4]: np.load(tmp_path / f"b{n}" / fn) for fn in names}
        assert all(a.dtype in (np.float32, np.float64) for a in out.values())
        assert all(out[k].tobytes() == again[k].tobytes() for k in out)
        assert len(out["block_coords"]) == min(n, 100) and out["sample_sdf"].shape == (16, 512) and out["sample_rgb"].shape == (16, 512, 3)
        # the sample's rows are blocks of the map, with their own voxels
        rows = np.searchsorted(descs["x"], out["sample_coords"][:, 0].astype(np.int64))
        assert np.array_equal(descs["x"][rows], out["sample_coords"][:, 0]) and np.array_equal(vox["sdf"][rows], out["sample_sdf"])
        assert np.array_equal(vox["weight"][rows].astype(np.float32), out["sample_weight"])


def test_the_dump_limits_fit_the_size_allowed():
    per_block, per_sample = 3 * 8 + 8 + 8, 512 * (4 + 4 + 4 + 12) + 3 * 8
    assert bench.DUMP_MAX_BLOCKS * per_block + bench.DUMP_SAMPLE_BLOCKS * per_sample <= bench.DUMP_LIMIT_BYTES == 64 << 20
