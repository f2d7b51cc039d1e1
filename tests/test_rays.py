"""CPU half of the ray queries (include/mrhash_rays.h): the restatement of tests/rays_ref.py pinned three ways.

  identity   cast with the pixel rays of a render it must return the render restatement's bytes (tests/raycast_ref.py,
             tests/raycast_sph_ref.py): depth or range, normals and colours, for scenes of every group of tests/ray_fields.py
  by hand    axis-aligned rays through uniform slabs whose sample states follow from the block table: the counts, first_unknown
             and the status against literals
  coverage   the mixed batch of tests/ray_batches.py reaches every kind of ray the GPU tests compare the kernel on

Identity casts the FIRST and the LAST scene of every group (24 of the 69 scenes; the restatement marches in Python, every scene
again would double the minute tests/test_ray_fields.py already takes).  Dropped: the scenes in between — islands' axis views
except "-z rim", steps' "default", "10 voxels", "ends in the gap" and "1 sample", "adaptive oblique", the ladders' inner rungs,
shapes 1 x 17, 7 x 9 and 17 x 33.  tests/test_rays_gpu.py casts every scene, kernel against kernel.

Two groups cannot be identical to their render: see beyond_the_bound."""
import numpy as np
import pytest

import ray_batches as rb
import ray_fields as rf
import rays_ref as yr
import test_ray_fields as trf

F = np.float32


def pixel_rays(s, rc):
    """The sensor-frame rays of the scene's pixels, row-major: origin (0, 0, 0), d_c exactly as the render's restatement has it."""
    rows, cols = rf.pixels(s)
    if s.model == "spherical":
        dc = rc.sensor_directions(rows, cols)
    else:
        dc = rc.cam.inverse_projection(rows, cols, np.ones(rows.shape, F)).astype(F)
    return np.zeros_like(dc), dc


def beyond_the_bound(s) -> bool:
    """D21 refuses a ray whose origin is not within (float) (1 << 20) * vs of the world origin on every axis; the renders have no
    such rule.  The cameras of "ladder far" (2^22 voxels out) and "key_range" (2^23) stand beyond it: there the identity cannot
    hold by D21's own text, and what D21 says instead is asserted — every ray is MRH_RAY_BAD and every other output +0."""
    return not np.all(np.abs(np.asarray(s.t, F)) < F(F(1 << 20) * F(s.params["virtual_voxel_size"])))


def picked(group):
    scenes = rf.GROUPS[group]()
    return [scenes[0]] if len(scenes) == 1 else [scenes[0], scenes[-1]]


@pytest.mark.parametrize("group", list(rf.GROUPS))
def test_pixel_rays_return_the_renders_bytes(group):
    m = None
    done = {x[0].name: x for x in trf._cache.get(group, [])}  # what tests/test_ray_fields.py rendered in this session, if it ran
    for s in picked(group):
        m = m or rf.ref_map(s.params, s.blocks)
        if s.name in done:
            _, rc, want = done[s.name]
        else:
            rc = rf.raycaster(s, m)
            want = rc.render(*rf.pixels(s))
        o, dc = pixel_rays(s, rc)
        if s.model == "pinhole":
            assert np.all(dc[:, 2] == 1)  # the range along d_c is the depth
        q = yr.RayQuery(m, s.min_depth, s.max_depth, s.step)
        got = q.cast(o, dc, R=s.R, t=s.t)
        assert len(q.z) == len(rc.z)
        if beyond_the_bound(s):
            assert np.all(got["status"] == yr.BAD) and not any(np.ascontiguousarray(got[k]).view(np.uint8).any() for k in yr.PLANES if k != "status"), s.name
            assert np.count_nonzero(want[0]) >= 8  # the render has no such bound: it sees the rung
            print("%-48s %4d rays, all beyond the bound" % (s.name, len(o)))
            continue
        for name, a, b in (("range", got["range"], want[0]), ("normals", got["normals"], want[1]), ("rgb", got["rgb"], want[2])):
            assert yr.same_bits(a, b), (s.name, name)
        hits = got["status"] & yr.HIT
        assert np.array_equal(hits != 0, want[0] > 0), s.name
        print("%-48s %4d rays, %d hits" % (s.name, len(o), int(np.count_nonzero(hits))))


# ---- by hand -------------------------------------------------------------------------------------------------------------------
# Step 0.1 m = 2 voxels from an origin at a quarter voxel: sample k lies at voxel 2 k + 0.25 of its axis (or 24.25 - 2 k going
# back), its trilinear reads voxels 2 k and 2 k + 1 there, and a pair never straddles a block face or a slab face (even voxels).

def _hand(m, o_vox, d, tmax, max_range):
    q = yr.RayQuery(m, 0.0, max_range, 0.1)
    o = (np.array(o_vox, np.float64) * rf.VS).astype(F)
    r = q.cast(o[None], np.array(d, F)[None], tmax=None if tmax is None else [tmax])
    return int(r["counts"][0, 0]), int(r["counts"][0, 1]), r["first_unknown"][0], int(r["status"][0]), r["range"][0]


def test_inside_out_by_hand():
    """Slabs along x (voxels): absent < 8, - 8 .. 23, + 24 .. 47, - 48 .. 63, + 64 .. 79, - 80 .. 95; block (6, 0, 0) = voxels 48 .. 55
    of y, z block 0 is removed."""
    m = rf.ref_map(rf.PARAMS, rf.inside_out_blocks())
    # y, z in block 1: k = 0 .. 3 absent, 4 .. 11 inside the - slab, 12 .. 23 free, k = 24 closes the bracket
    free, unknown, first, status, rng = _hand(m, (0.25, 10.25, 10.25), (1, 0, 0), None, 4.05)
    assert (free, unknown, status) == (12, 4, yr.HIT | yr.UNKNOWN | yr.INSIDE) and first == 0 and 2.3 < rng < 2.4
    # y, z in block 0: the removed block takes k = 24 .. 27 (voxels 48 .. 55) and the bracket; k = 28 .. 31 are inside the - slab
    # behind it, 32 .. 39 free, k = 40 closes the bracket at voxel 80
    free, unknown, first, status, rng = _hand(m, (0.25, 2.25, 2.25), (1, 0, 0), None, 4.05)
    assert (free, unknown, status) == (20, 8, yr.HIT | yr.UNKNOWN | yr.INSIDE) and first == 0 and 3.9 < rng < 4.0
    # from inside the + slab, 11 samples (voxels 24 .. 45): line of sight
    assert _hand(m, (24.25, 10.25, 10.25), (1, 0, 0), 1.05, 4.05)[:4] == (11, 0, 0, 0)
    # backwards: k = 0 reads voxels 24, 25 (+), k = 1 voxels 22, 23 (-) and closes the bracket
    free, unknown, first, status, rng = _hand(m, (24.25, 10.25, 10.25), (-1, 0, 0), None, 4.05)
    assert (free, unknown, first, status) == (1, 0, 0, yr.HIT) and 0 < rng < 0.1
    # the same ray ended before its second sample: no hit, one free sample
    assert _hand(m, (24.25, 10.25, 10.25), (-1, 0, 0), 0.05, 4.05)[:4] == (1, 0, 0, 0)
    # no sample at all
    assert _hand(m, (24.25, 10.25, 10.25), (-1, 0, 0), -1.0, 4.05) == (0, 0, 0, 0, 0)


def test_islands_slab_by_hand():
    """The + slab of arm x: x blocks 2, 3, y and z blocks -2 .. 1 (voxels -16 .. 15); nothing beside it at x block 2."""
    m = rf.ref_map(rf.PARAMS, rf.islands_blocks())
    # along +y from y voxel 0.25: k = 0 .. 7 read voxels <= 15 (free), k = 8 .. 12 lie beyond the slab
    free, unknown, first, status, rng = _hand(m, (20.25, 0.25, 2.25), (0, 1, 0), None, 1.25)
    assert (free, unknown, status, rng) == (8, 5, yr.UNKNOWN, 0) and first == F(8) * F(0.1)
    # from y voxel -19.75: k = 0, 1 in front of the slab, 2 .. 17 free, 18 .. 20 beyond it
    free, unknown, first, status, rng = _hand(m, (20.25, -19.75, 2.25), (0, 1, 0), None, 2.05)
    assert (free, unknown, first, status, rng) == (16, 5, 0, yr.UNKNOWN, 0)
    # ... ended inside the slab: first_unknown stays z_0 = +0, two unknown samples
    assert _hand(m, (20.25, -19.75, 2.25), (0, 1, 0), 0.95, 2.05)[:4] == (8, 2, 0, yr.UNKNOWN)


# ---- coverage ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    b = rb.mixed_batch()
    m = rf.ref_map(rb.PARAMS, rb.rays_blocks())
    q = yr.RayQuery(m, b.min_range, b.max_range, b.step, truncation=rb.PARAMS["sdf_truncation"])
    return b, m, q, q.cast(b.origins, b.directions, tmax=b.tmax)


def test_the_mixed_batch_reaches_every_kind_of_ray(mixed):
    b, m, q, out = mixed
    n = len(b.origins)
    status = out["status"]
    fam = np.array(b.family)
    assert n >= 257, n  # the GPU tests cast its first 1, 63, 64, 65 and 257 rays
    print({e: q.count(e) for e in yr.EVENTS})
    good = status[(status & yr.BAD) == 0]
    for combo in range(8):  # HIT x UNKNOWN x INSIDE
        assert np.count_nonzero(good == combo) >= 4, (combo, np.count_nonzero(good == combo))
    for e in ("first_unknown_at_0", "first_unknown_later", "ends_in_absent_run", "jump_eligible", "trilinear_failed", "hit_coarse", "cut_by_tmax"):
        assert q.count(e) >= 4, (e, q.count(e))
    assert q.count("zero_samples") >= 1
    # each kind of bad ray, once, where the batch says; nothing else is bad; at most an eighth of the batch
    for name, i in rb.BAD:
        assert status[i] == yr.BAD and name in q.rays[i], (name, i, status[i], q.rays[i])
    bad = np.flatnonzero(status & yr.BAD)
    assert sorted(bad) == sorted(i for _, i in rb.BAD) and 8 * len(bad) <= n
    for plane in ("range", "normals", "rgb", "counts", "first_unknown"):
        assert not np.ascontiguousarray(out[plane][bad]).view(np.uint8).any(), plane
    # a ray that the unbounded cast hits but whose own end comes first: cut_short is hit_inside ended early
    cut = rb.pairs(b, "hit_inside", "cut_short")
    assert len(cut) >= 4
    for i, j in cut:
        assert np.array_equal(b.origins[i], b.origins[j]) and np.array_equal(b.directions[i], b.directions[j])
        assert status[i] & yr.HIT and b.tmax[j] < out["range"][i] and not status[j] & yr.HIT and out["range"][j] == 0
        assert out["counts"][j, 0] <= out["counts"][i, 0]
    # a ray that ends inside an absent block after a stretch the kernel may jump: its unknown samples stop at its own end
    gap = rb.pairs(b, "ends_in_gap", "through_gap")
    assert len(gap) >= 4 and all("ends_in_absent_run" in q.rays[i] for i, _ in gap)
    for i, j in gap:
        assert 0 < out["counts"][i, 1] < out["counts"][j, 1], (i, j, out["counts"][i], out["counts"][j])
    # origins: inside a block, in a block's quarter-voxel rim on an axis the ray does not move along, at the rung, in a coarse block
    rim = np.flatnonzero(fam == "rim")
    y = b.origins[rim, 1] / F(rf.VS)
    assert len(rim) >= 4 and np.all((y > -0.5) & (y < -0.25)) and np.all(b.directions[rim, 1] == 0) and all("absent_run" in q.rays[i] for i in rim)
    rung = np.flatnonzero((fam == "rung") | (fam == "rung_outside"))
    assert np.all(b.origins[rung, 0] > 1000) and np.count_nonzero(status[rung] & yr.HIT) >= 4 and all("jump_eligible" in q.rays[i] for i in rung if fam[i] == "rung_outside")
    assert np.count_nonzero(status[fam == "coarse"] & yr.HIT) >= 4 and all("hit_coarse" in q.rays[i] for i in np.flatnonzero(fam == "coarse"))
    assert any(isinstance(v, tuple) and v[0] == 1 for v in rb.rays_blocks().values())
    # the zero-sample ray is not bad
    z = rb.ZERO_SAMPLES_AT
    assert status[z] == 0 and not out["counts"][z].any() and "zero_samples" in q.rays[z]


def test_status_and_counts_agree(mixed):
    b, m, q, out = mixed
    status, counts = out["status"], out["counts"]
    ok = (status & yr.BAD) == 0
    assert np.array_equal((status[ok] & yr.UNKNOWN) != 0, counts[ok, 1] > 0)
    assert np.array_equal((status[ok] & yr.HIT) != 0, out["range"][ok] > 0)
    assert np.all(out["first_unknown"][counts[:, 1] == 0] == 0)
    assert np.all(counts.sum(axis=1) <= len(q.z))


def test_a_pose_and_no_pose_describe_the_same_rays(mixed):
    """The batch in the sensor frame of a quarter turn: the same families come out (the world rays differ in the last bit at most)."""
    b, m, q, out = mixed
    o, d = rb.sensor_frame(b)
    posed = yr.RayQuery(m, b.min_range, b.max_range, b.step, truncation=rb.PARAMS["sdf_truncation"]).cast(o[:64], d[:64], tmax=b.tmax[:64], R=rb.POSE_R, t=rb.POSE_T)
    same = posed["status"] == out["status"][:64]
    assert np.count_nonzero(same) >= 60, np.flatnonzero(~same)
