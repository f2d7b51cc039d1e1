"""The Python surface of the drop-in class, pinned: the names `GeoWrapper` has and pybind11's signature text of each — argument
names, order, defaults and overloads — against tests/golden/geowrapper_surface.json, which was written from the binding as it
was before its helpers (one float-array alias, one pose parser, one vector-to-array function) replaced the copies.  No GPU is
needed: the module loads the library, and a context is only created by the constructor."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "geowrapper_surface.json")


def surface(cls):
    names = sorted(n for n in dir(cls) if not n.startswith("__"))
    return {"names": names, "docs": {n: getattr(cls, n).__doc__ for n in names}, "init": cls.__init__.__doc__}


def test_names_and_signatures_are_the_recorded_ones(hip):
    from mrhash.src.pygeowrapper import GeoWrapper

    want = json.load(open(GOLDEN))
    got = surface(GeoWrapper)
    assert got["names"] == want["names"]
    for n in want["names"]:
        assert got["docs"][n] == want["docs"][n], n
    assert got["init"] == want["init"]


def test_constructing_without_a_device_raises():
    import torch

    from mrhash_amd import hipmem

    if torch.cuda.is_available() or hipmem.device_count() > 0:  # the HIP runtime's own count: torch may have been built for another one
        pytest.skip("a HIP device is present; the no-device path cannot be exercised here")
    from mrhash.src.pygeowrapper import GeoWrapper

    with pytest.raises(RuntimeError):
        GeoWrapper(sdf_truncation=0.06, sdf_truncation_scale=0.0, integration_weight_sample=1, virtual_voxel_size=0.02, n_frames_invalidate_voxels=2,
                   voxel_extents_scale=1, viewer_active=False, marching_cubes_threshold=1.5, min_weight_threshold=5, min_depth=0.01, max_depth=30.0)
