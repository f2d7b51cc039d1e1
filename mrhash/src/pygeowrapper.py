"""Drop-in for the reference's nanobind module `mrhash.src.pygeowrapper`.  Beyond the reference's surface GeoWrapper has raycast,
distanceField, queryPoints, fuseMap, alignMap, trackDepthImage / trackPointCloud and their render-free forms trackDepthImageSDF /
trackPointCloudSDF (mrhash_amd/csrc/geowrapper.h)."""
from mrhash_amd._runtime import torch_first as _torch_first

_torch_first()  # torch's HIP runtime (if torch is installed) has to initialise before this library's: mrhash_amd/_runtime.py
from mrhash_amd.pygeowrapper import GeoWrapper  # noqa: E402,F401
