"""CPU half of the raycast scenes (tests/ray_fields.py): every scene reaches the branches it is built for.  Counted on the
restatement alone (tests/raycast_ref.py, tests/raycast_sph_ref.py through the counting subclasses), on the maps as the builders
give them; tests/test_ray_fields_gpu.py repeats the counts on what the engine dumps and compares the kernel's bytes.

Not reachable on any map, and therefore not asserted (ray_fields.zeros_blocks and test_a_hit_reads_its_colour_from_a_present_block
say why): a sample whose trilinear value is -0, and a hit whose colour comes from an absent block."""
import numpy as np
import pytest

import ray_fields as rf

F = np.float32

_cache = {}


def rendered(group):
    """[(scene, caster, outputs)] of the group's scenes, rendered once per session."""
    if group not in _cache:
        out, m = [], None
        for s in rf.GROUPS[group]():
            m = m or rf.ref_map(s.params, s.blocks)
            rc = rf.raycaster(s, m)
            out.append((s, rc, rc.render(*rf.pixels(s))))
            assert len(rc.rays) == s.intr[4] * s.intr[5] <= 1000
            print("%-48s %4d rays x %5d samples, hit share %.2f  %s" % (s.name, len(rc.rays), len(rc.z), rf.hit_share(rc), rc.counts()))
        _cache[group] = out
    return _cache[group]


def covered(group):
    r = rendered(group)
    total = rf.check_coverage(group, [(s, rc) for s, rc, _ in r])
    print(group, "TOTAL", total)
    return r, total


def by_name(r, name):
    (hit,) = [x for x in r if x[0].name == name]
    return hit


def test_islands():
    """13 renders of 16 x 16 (a generic pose; +-x, +-y, +-z from an origin well inside a block and from one in a rim).  Rays with
    the event, all renders together: jump 3328 (every ray), all-positive 537, negative x / y / z 1504 / 1505 / 1516, a zero component
    with the origin inside the shrunk box 282 and in the rim 96, ends in an absent block 3252, refinement rejected 36 (18 hit
    later), crossing discarded behind an absent block 860 and behind a failed trilinear 1165, back faces 921, hits 1590 (787 without
    a normal because a stencil trilinear failed); hit share 0.34 .. 0.62 per image."""
    r, _ = covered("islands")
    for s, rc, _ in r:
        if s.name == "islands generic":
            d = rc.directions(*rf.pixels(s))
            assert not (d == 0).any() and not (np.abs(rc.cam.R) < 1e-3).any()
            continue
        # the centre row and column of an axis-aligned view have a component of exactly 0, on both other axes
        d = rc.directions(*rf.pixels(s))
        assert ((d == 0).sum(axis=1) == 1).sum() == 30 and ((d == 0).sum(axis=1) == 2).sum() == 1
        assert rc.count("jump_zero_inside") >= 8
        assert (rc.count("jump_zero_rim") >= 8) == s.name.endswith("rim"), s.name
        assert rc.count("jump_eligible") == 256  # close to the origin: both gates open
    for a in "xyz":  # each axis is looked along in both directions
        assert by_name(r, "islands -%s inside" % a)[1].count("jump_negative_" + a) == 256
        assert by_name(r, "islands +%s inside" % a)[1].count("jump_negative_" + a) == 0


def test_steps():
    """0.1 voxel: 144 rays x 541 samples, every ray with a jumpable run of up to 80 samples a block, 59 hits.  Default: as islands'
    generic view.  10 voxels: 16 samples a ray, no two consecutive samples in one block (no jump), 37 hits, 10 rejected
    refinements.  Ends in the gap: all 144 rays end in an absent block behind the slab.  1 sample: no hit is possible.
    2 samples: 24 hits of 144."""
    r, _ = covered("steps")
    fine, default, coarse, gap, one, two = r
    assert fine[1].count("jump") == len(fine[1].rays) and fine[1].count("jump_eligible") == len(fine[1].rays) and len(fine[1].z) > 500
    assert coarse[1].count("jump") == 0 and coarse[0].step > rf.BLOCK and coarse[1].count("hit") >= 8
    assert gap[1].count("ends_absent") == len(gap[1].rays) and gap[1].count("hit") == 0 and gap[1].count("jump") == len(gap[1].rays)
    assert len(one[1].z) == 1 and one[1].count("hit") == 0
    assert len(two[1].z) == 2 and two[1].count("hit") >= 8


def test_inside_out():
    """256 rays: all 256 pass a back face first; 174 hit (spherical: 166); 24 lose the first front face to the removed block (the
    crossing is discarded behind an absent sample; spherical: 23) and 9 to a trilinear that fails along that block's edge (10);
    those that hit at all hit the front face at block 10 instead; 40 hits have no normal (39)."""
    for group in ("inside_out", "spherical inside_out"):
        r, _ = covered(group)
        (s, rc, out), = r
        depth = out[0]
        d = rc.directions(*rf.pixels(s))
        x = rc.cam.t[0] + depth * d[:, 0]
        lost = np.array(["discarded_absent" in e or "discarded_trilinear" in e for e in rc.rays])  # through the removed block, or along its edge
        hit = depth > 0
        first, second = 6 * rf.BLOCK, 10 * rf.BLOCK
        assert np.all(np.abs(x[hit & ~lost] - first) < rf.VS), "a ray that keeps its bracket hits the first front face"
        assert (hit & lost).sum() >= 8 and np.all(np.abs(x[hit & lost] - second) < rf.VS), "a ray that loses it hits the second"
        assert np.all(x[hit] > 3 * rf.BLOCK + rf.VS), "the back face at block 3 is no hit"
        assert rc.count("back_face") >= rc.count("hit")


def test_zeros():
    """The field (a quarter of the cells +0, a sixteenth -0): 115 hits of 256, 6 rays with prev_d == 0 not taken.  The slabs: 153 of
    288 rays take a crossing whose D is exactly 0, 68 of them deep enough in the constant region for a gradient of length 0, and
    135 rays meet prev_d == 0, D <= 0 and do not hit."""
    r, _ = covered("zeros")
    s, rc, out = by_name(r, "zeros slabs")
    depth, nrm = out[0], out[1]
    taken = np.array(["zero_taken" in e for e in rc.rays])
    refused = np.array(["prev_zero_not_taken" in e for e in rc.rays])
    flat = np.array(["normal_zero_length" in e for e in rc.rays])
    assert np.all(depth[taken] > 0) and not np.any(depth[refused] > 0) and not np.any(taken & refused)
    assert flat.sum() >= 8 and np.all(depth[flat] > 0) and not nrm[flat].any()
    # both kinds of zero cell are behind these rays: the columns y = 5 / 7 store +0, y = 6 / 8 store -0
    y = np.floor(((rc.cam.t[1] + 1.8 * rc.directions(*rf.pixels(s))[:, 1]) / rf.VS + 0.5) / 8).astype(int)  # the block row 1.8 m out
    for event, cols in ((taken, (5, 6)), (refused, (7, 8))):
        for c in cols:
            assert (event & (y == c)).sum() >= 8, (c, (event & (y == c)).sum())


def test_adaptive():
    """Three renders (24 x 24 along +z through the four neighbour galleries, 16 x 16 obliquely, 16 x 16 into the variance-adaptive
    sign field): 710 hits of 1088, 296 of them in a coarse block (h = 2 vs), 464 without a normal, 22 rejected refinements.  The
    spherical render of the galleries: 162 hits of 256, 69 in a coarse block."""
    r, _ = covered("adaptive")
    assert any(isinstance(v, tuple) and v[0] == 1 for v in r[0][0].blocks.values())
    covered("spherical adaptive")


def test_a_hit_reads_its_colour_from_a_present_block():
    """A hit's point P is where the refinement's last trilinear succeeded, so the eight voxels round((P -+ h / 2) / vs) carry
    weight.  Per axis one of those two is round(P / vs), getVoxel's voxel: its block is present.  (In a coarse block h = 2 vs and
    P's own block is that present coarse block.)  So "valid hit, absent colour block" does not occur; every hit of every scene
    confirms it."""
    for group in rf.GROUPS:
        for s, rc, _ in rendered(group):
            assert rc.count("colour_absent") == 0, s.name


@pytest.mark.parametrize("vs", rf.LADDER_VS)
def test_ladder(vs):
    """Rungs 8 .. 16 on both sides, looked through along +x and -x, 100 rays each.  At 0.05 m and 2^-4 m block_shift_limit is
    2^22 voxels, beyond the ladder (ray_fields.LADDER_RUNGS says why), so there the per-ray reach decides: every ray of rungs 8 .. 12
    may jump, no ray of rungs 13 .. 16 may.  At 0.02 m the limit is 2^13 voxels: rung 9 jumps, rung 10 has blocks on both sides of
    the limit on every ray, rung 11 never jumps.  The wide render at rung 12 (0.05 m): 64 rays may jump, 80 may not.  Rays with a
    jumpable run / that may jump / kept from it by the reach / by the shift limit: 3744 / 2064 / 1680 / 0 at 0.05 m, 3600 / 2000 /
    1600 / 0 at 2^-4 m, 1200 / 800 / 0 / 800 at 0.02 m; hits 2513, 2615 and 809; rejected refinements 148, 78 and 37."""
    r, _ = covered("ladder %g" % vs)
    lim = rf.shift_limit(vs)
    assert lim == (1 << 13 if vs == 0.02 else 1 << 22)
    for s, rc, _ in r:
        if s.name == "ladder wide":
            assert rc.count("jump_eligible") >= 8 and rc.count("jump_ineligible_reach") >= 8
            continue
        k, n = int(s.name.split("rung ")[1].split()[0]), len(rc.rays)
        assert rc.count("jump") == n
        if vs == 0.02:
            assert rc.count("jump_eligible") == (n if k <= 10 else 0) and rc.count("jump_ineligible_shift") == (n if k >= 10 else 0), s.name
        else:
            assert rc.count("jump_eligible") == (n if k <= 12 else 0) and rc.count("jump_ineligible_reach") == (n if k >= 13 else 0), s.name


def test_ladder_far_and_key_range():
    """The rung below 2^19 blocks: all 288 rays are beyond the reach and have absent runs in blocks below the shift limit.  The
    rung at the last key: all 144 rays have samples in blocks x >= 2^20 and end there; 101 hit."""
    covered("ladder far")
    (s, rc, _), = covered("key_range")[0]
    assert max(b[0] for b in s.blocks) == (1 << 20) - 1
    assert rc.count("beyond_keys") == len(rc.rays)


def test_shapes():
    """1 x 1, 1 x 17, 7 x 9, 17 x 33 and 33 x 16 pixels of the generic view: 1, 13, 38, 331 and 290 hits."""
    r, _ = covered("shapes")
    assert [(s.intr[4], s.intr[5]) for s, _, _ in r] == list(rf.SHAPES)


def test_spherical_islands():
    """Two 16 x 16 renders whose azimuths run across -pi: 112 and 126 hits; the row of elevation 0 of the axis-aligned one has a
    component of exactly 0."""
    r, _ = covered("spherical islands")
    for s, rc, out in r:
        az = rc.cam.ifx * ((np.arange(16, dtype=F) - rc.cam.cx) - F(0.5))
        assert az.min() < -np.pi < az.max()
        rng, pts = out[0], out[3]
        assert not np.ascontiguousarray(pts[rng == 0]).view(np.uint8).any(), "a miss is +0 in all three components"


def test_the_counting_raycaster_returns_its_parents_bytes():
    s = rf.zeros()[1]
    m = rf.ref_map(s.params, s.blocks)
    r, c = rf.pixels(s)
    want = rf.rr.Raycaster(m, *s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step).render(r[:60], c[:60])
    got = rf.raycaster(s, m).render(r[:60], c[:60])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want, got)) and np.count_nonzero(want[0]) > 8
