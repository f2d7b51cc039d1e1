"""GPU half of the raycast scenes (tests/ray_fields.py): k_raycast<false> and k_raycast<true> (mrh_raycast.h) against the literal
restatement, byte for byte, in every image of every scene — depth or range, normals, colours and, for the spherical camera,
points.  The restatement marches sample by sample; the kernel jumps over absent blocks (ray_skip_absent), so parity on these maps
is the test of the jump's rounding argument, of its two gates, and of rule 4's and rule 5's branches.  Maps are imported, not
fused; the restatement's map is the engine's own dump; the coverage of tests/test_ray_fields.py is asserted again on it.

What byte parity cannot see, by construction: the refusals of ray_skip_absent that only make it more careful.  A sample in a
block's rim, an origin coordinate in the rim on an axis with d == 0, a last index one too high: in each case the samples a jump
would skip still lie between two points of the same absent block, so skipping them changes no bit.  Likewise the reach gate:
wherever voxels still convert by the shift (below 2^22) a float32 position is at most 0.3 voxel off, a wrongly skipped sample then
lies within half a voxel of the absent block, and its trilinear reaches into that block and fails anyway ("ladder far" is built on
the blocks where the shrunk face converts to the next block).  Builds with each of these four checks removed render every scene
here identically; builds that take prev_d == 0 for a bracket, or stop at a rejected refinement, do not ("zeros"; "islands",
"adaptive", "shapes")."""
import numpy as np
import pytest

import mc_fields as mf
import parity_utils as pu
import ray_fields as rf
import raycast_ref as rr
from mrhash_amd import capi, hipmem, synth

pytestmark = pytest.mark.gpu

IMAGES = ("depth", "normals", "colours", "points")
SCENES = {g: rf.GROUPS[g]() for g in rf.GROUPS}
CASES = [pytest.param(g, i, id="%s" % s.name) for g in rf.GROUPS for i, s in enumerate(SCENES[g])]
RESTATED = {}  # (group, i) -> (caster, images): rendered once, on the map the group's engine dumped


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


class Field:
    """One group: an engine on its imported map, the restatement's map of the engine's dump, the restatement's renders."""

    def __init__(self, group):
        self.group, self.scenes = group, SCENES[group]
        s = self.scenes[0]
        self.e = pu.make_engine(capi.load_hip(), synth.CFG1, s.params, rf.NUM_SDF_BLOCKS.get(group, 4096))
        self.e.import_blocks(*mf.to_import(s.blocks))
        d, v = self.e.dump_blocks()
        assert len(d) == len(s.blocks)
        self.m = rr.make_map(s.params, d, v)

    def restated(self, i):
        """(caster, images) of scene i: flat [n], [n, 3], [n, 3] and, spherical, [n, 3]."""
        if (self.group, i) not in RESTATED:
            s = self.scenes[i]
            rc = rf.raycaster(s, self.m)
            RESTATED[self.group, i] = (rc, rc.render(*rf.pixels(s)))
        return RESTATED[self.group, i]

    def kernel(self, i, **kw):
        s = self.scenes[i]
        if s.model == "spherical":
            return self.e.raycast_spherical(*s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step, points=True, **kw)
        return self.e.raycast(*s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step, **kw)


@pytest.fixture(scope="module")
def field(request):
    f = Field(request.param)
    yield f
    f.e.close()


def assert_parity(s, rc, got, want):
    """Every image as bytes; a difference names its first pixels, both values and the events the restatement met on those rays."""
    n, cols = s.intr[4] * s.intr[5], s.intr[5]
    for name, a, b in zip(IMAGES, got, want):
        a = np.ascontiguousarray(a).reshape(n, -1)
        b = np.ascontiguousarray(b).reshape(n, -1)
        assert a.dtype == b.dtype and a.shape == b.shape, (s.name, name, a.dtype, a.shape, b.shape)
        if _same_bits(a, b):
            continue
        bad = np.flatnonzero(np.any(a.view(np.uint8).reshape(n, -1) != b.view(np.uint8).reshape(n, -1), axis=1))
        lines = ["pixel (%d, %d): kernel %s, restatement %s, events %s" % (p // cols, p % cols, a[p], b[p], sorted(rc.rays[p])) for p in bad[:5]]
        raise AssertionError("%s: %s differs at %d of %d pixels\n%s" % (s.name, name, len(bad), n, "\n".join(lines)))


@pytest.mark.parametrize("field, i", CASES, indirect=["field"])
def test_parity(field, i):
    s = field.scenes[i]
    rc, want = field.restated(i)
    got = field.kernel(i)
    assert got[0].shape == (s.intr[4], s.intr[5])
    print("%s: %d rays, hit share %.2f, %s" % (s.name, len(rc.rays), rf.hit_share(rc), rc.counts()))
    assert_parity(s, rc, got, want)


@pytest.mark.parametrize("group", list(rf.GROUPS))
def test_coverage_on_the_dumped_map(group):
    """The floors of tests/test_ray_fields.py, on the restatement of the map the engine held (rendered by test_parity; rendered
    here when this test runs alone)."""
    if any((group, i) not in RESTATED for i in range(len(SCENES[group]))):
        f = Field(group)
        try:
            for i in range(len(f.scenes)):
                f.restated(i)
        finally:
            f.e.close()
    total = rf.check_coverage(group, [(s, RESTATED[group, i][0]) for i, s in enumerate(SCENES[group])])
    print(group, total)


@pytest.mark.parametrize("field", ["shapes"], indirect=True)
def test_every_output_subset_equals_its_plane_of_the_full_render(field):
    """17 x 33: depth only, normals only, colours only (the latter two through the device call, which alone can leave depth out)."""
    i = list(rf.SHAPES).index((17, 33))
    s = field.scenes[i]
    rc, want = field.restated(i)
    full = field.kernel(i)
    assert_parity(s, rc, full, want)
    depth, nrm, rgb = field.kernel(i, normals=False, colors=False)
    assert nrm is None and rgb is None and _same_bits(depth, full[0])
    n = s.intr[4] * s.intr[5]
    args = (*s.intr, s.R, s.t, s.min_depth, s.max_depth, s.step)
    dn, dc = hipmem.DeviceBuffer(12 * n), hipmem.DeviceBuffer(3 * n)
    field.e.raycast_device(*args, d_normals=dn.ptr)
    field.e.raycast_device(*args, d_rgb=dc.ptr)
    field.e.sync()
    assert _same_bits(dn.to_numpy(np.float32), full[1].ravel()), "normals only"
    assert np.array_equal(dc.to_numpy(np.uint8), full[2].ravel()), "colours only"
    assert np.count_nonzero(full[0]) >= 8 and full[1].any() and full[2].any()
