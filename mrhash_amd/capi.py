"""ctypes binding of the C ABI declared in include/mrhash_hip.h.

`Engine` drives any shared library that implements that ABI.  The product library is
`mrhash_amd/csrc/libmrhash_hip.so` (hand-written gfx950 HIP kernels); tests additionally load
the CPU oracle (`oracle/_build/libmrh_oracle.so`) through the very same class so that parity
tests run identical host code against both.  Nothing in this module falls back from one to
the other: `load_hip()` raises if the HIP library is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_LIB_PATH = os.path.join(_ROOT, "mrhash_amd", "csrc", "libmrhash_hip.so")

MRH_ABI_VERSION = 3

MRH_OK = 0
MRH_PENDING_EXCHANGE = 1
MRH_ERR_INVALID_ARG = -1
MRH_ERR_DEVICE = -2
MRH_ERR_NO_DEVICE = -3
MRH_ERR_CAPACITY = -4
MRH_ERR_STATE = -5
MRH_ERR_UNSUPPORTED = -6
MRH_ERR_OUT_OF_RANGE = -7

PINHOLE, SPHERICAL = 0, 1


class MrhParams(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("sdf_truncation", C.c_float),
        ("sdf_truncation_scale", C.c_float),
        ("integration_weight_sample", C.c_int32),
        ("integration_weight_max", C.c_int32),
        ("virtual_voxel_size", C.c_float),
        ("n_frames_invalidate_voxels", C.c_int32),
        ("voxel_extents_scale", C.c_int32),
        ("marching_cubes_threshold", C.c_float),
        ("min_weight_threshold", C.c_uint8),
        ("projective_sdf", C.c_uint8),
        ("reserved0", C.c_uint8 * 2),
        ("min_depth", C.c_float),
        ("max_depth", C.c_float),
        ("sdf_var_threshold", C.c_float),
        ("vertices_merging_threshold", C.c_float),
        ("num_sdf_blocks", C.c_uint64),
        ("hash_slots", C.c_uint64),
        ("max_triangles", C.c_uint64),
        ("device_id", C.c_int32),
        ("shard_rank", C.c_int32),
        ("shard_count", C.c_int32),
        ("shard_chunk_log2", C.c_int32),
    ]


class MrhStats(C.Structure):
    _fields_ = [
        ("frames_integrated", C.c_uint64),
        ("num_sdf_blocks", C.c_uint64),
        ("occupied_fine", C.c_uint64),
        ("occupied_coarse", C.c_uint64),
        ("free_fine", C.c_int64),
        ("free_coarse", C.c_int64),
        ("last_compact_blocks", C.c_uint64),
        ("last_updated_voxels", C.c_uint64),
        ("last_inserted_blocks", C.c_uint64),
        ("last_freed_blocks", C.c_uint64),
        ("total_updated_voxels", C.c_uint64),
        ("total_compact_blocks", C.c_uint64),
        ("last_triangles", C.c_uint64),
        ("last_integrate_kernel_ms", C.c_float),
        ("sum_integrate_kernel_ms", C.c_float),
        ("n_integrate_kernel", C.c_uint64),
        ("error_flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("hash_slots", C.c_uint64),
        ("tombstones", C.c_uint64),
        ("max_probe_length", C.c_uint32),
        ("rehash_count", C.c_uint32),
        ("last_mc_count_ms", C.c_float),
        ("last_mc_emit_ms", C.c_float),
        ("last_mc_blocks", C.c_uint64),
        ("sum_front_kernel_ms", C.c_float),
        ("reserved1", C.c_uint32),
        ("n_front_kernel", C.c_uint64),
    ]


VOXEL_DTYPE = np.dtype(
    [("sdf", "<f4"), ("sum_squared", "<f4"), ("rgb", "u1", (3,)), ("weight", "u1")], align=False
)
assert VOXEL_DTYPE.itemsize == 12
DESC_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("resolution", "<i4")])
RECORD_DTYPE = np.dtype([("desc", DESC_DTYPE), ("voxels", VOXEL_DTYPE, (512,))])  # mrh_block_record
RECORD_BYTES = 6160
PACK_HALO, PACK_OWNER = 0, 1
UNPACK_HALO, UNPACK_MERGE = 0, 1
DROP_HALO, DROP_FOREIGN, DROP_ALL = 0, 1, 2
TRI_DTYPE = np.dtype([("p", "<f4", (3,)), ("c", "<f4", (3,))])  # one vertex; a triangle is 3 of them
SEED_DTYPE = np.dtype([("p", "<f4", (3,)), ("scale", "<f4"), ("rgb", "u1", (3,)), ("pad", "u1")])  # mrh_splat_seed, 20 bytes
LEAF_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("width", "<i4"), ("height", "<i4")])  # mrh_qtree_leaf
assert TRI_DTYPE.itemsize == 24

# every symbol include/mrhash_hip.h declares
ABI_SYMBOLS = (
    "mrh_create mrh_destroy mrh_reset mrh_last_error mrh_set_camera mrh_set_pose mrh_upload_depth "
    "mrh_upload_rgb mrh_set_depth_device mrh_set_rgb_device mrh_integrate mrh_integrate_resume mrh_exchange_buffer mrh_sync "
    "mrh_upload_points mrh_upload_normals mrh_set_points_device mrh_integrate_points mrh_set_scan_layout mrh_detect_scan_layout mrh_stream_out mrh_get_free_blocks "
    "mrh_splat_seeds mrh_get_qtree_leaves mrh_peek_free_blocks mrh_peek_error_flags "
    "mrh_set_sharding mrh_pack_blocks mrh_unpack_blocks mrh_drop_blocks "
    "mrh_extract_triangles mrh_extract_mesh mrh_mesh_merge_begin mrh_mesh_merge_end mrh_get_stats mrh_set_profile mrh_dump_blocks "
    "mrh_get_voxel mrh_import_blocks mrh_get_triangle_blocks mrh_get_triangles_device mrh_process_triangle_runs mrh_process_triangles mrh_selftest_division mrh_version"
).split()


# every symbol include/mrhash_comm.h declares (the HIP library only: the oracle has no communicator)
COMM_SYMBOLS = (
    "mrh_comm_unique_id mrh_comm_create mrh_comm_destroy mrh_comm_last_error mrh_comm_size mrh_comm_barrier mrh_comm_allreduce_f64 "
    "mrh_comm_allgather_bytes mrh_comm_attach mrh_comm_exchange_halo mrh_comm_merge_submaps mrh_comm_gather_mesh mrh_comm_phase_times mrh_comm_status"
).split()
COMM_ID_BYTES = 128
COMM_SUM, COMM_MAX, COMM_MIN = 0, 1, 2

# every symbol include/mrhash_raycast.h declares (the HIP library only: the oracle does not render)
RAYCAST_SYMBOLS = ("mrh_raycast mrh_raycast_device mrh_raycast_spherical mrh_raycast_spherical_device").split()
RAYCAST_NORMALS, RAYCAST_COLORS, RAYCAST_POINTS = 1, 2, 4


class MrhRaycastParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("rows", C.c_int32), ("cols", C.c_int32),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("step", C.c_float), ("outputs", C.c_uint32)]


# every symbol include/mrhash_esdf.h declares (the HIP library only: the oracle has no distance field)
ESDF_SYMBOLS = ("mrh_esdf mrh_esdf_device").split()
ESDF_STATE, ESDF_SQUARED = 1, 2
ESDF_OBSERVED, ESDF_SITE, ESDF_INSIDE, ESDF_FAR = 1, 2, 4, 8
ESDF_FAR_D2 = 0xFFFFFFFF


class MrhEsdfParams(C.Structure):
    _fields_ = [("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("max_distance_voxels", C.c_int32), ("min_weight", C.c_int32),
                ("surface_band", C.c_float), ("outputs", C.c_uint32)]


# every symbol include/mrhash_query.h declares (the HIP library only: the oracle has no point query)
QUERY_SYMBOLS = ("mrh_query_points mrh_query_points_device").split()
QUERY_FIELD_MAP, QUERY_FIELD_SMOOTH = 0, 1
QUERY_GRADIENT, QUERY_COLOUR = 1, 2
QUERY_BLOCK, QUERY_DIST, QUERY_GRAD, QUERY_COARSE, QUERY_REFUSED = 1, 2, 4, 8, 0x80
QUERY_MAX_POINTS = 1 << 24


class MrhQueryParams(C.Structure):
    _fields_ = [("field", C.c_int32), ("outputs", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# every symbol include/mrhash_rays.h declares (the HIP library only: the oracle has no ray query)
RAYS_SYMBOLS = ("mrh_cast_rays mrh_cast_rays_device").split()
RAYS_NORMALS, RAYS_COLORS, RAYS_COUNTS = 1, 2, 4
RAY_HIT, RAY_UNKNOWN, RAY_INSIDE, RAY_BAD = 1, 2, 4, 0x80
RAYS_MAX_RAYS = 1 << 24


class MrhRaysParams(C.Structure):
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("step", C.c_float), ("outputs", C.c_uint32), ("reserved", C.c_uint32 * 4)]


# every symbol include/mrhash_freespace.h declares (the HIP library only: the oracle has no free-space layer)
FREESPACE_SYMBOLS = ("mrh_freespace_create mrh_freespace_clear mrh_freespace_destroy mrh_freespace_carve_depth mrh_freespace_carve_depth_device "
                     "mrh_freespace_carve_points mrh_freespace_carve_points_device mrh_freespace_box mrh_freespace_box_device mrh_freespace_segments "
                     "mrh_freespace_segments_device").split()
FREE_FREE, FREE_OBSERVED, FREE_OCCUPIED, FREE_FRONTIER = 1, 2, 4, 8
FREE_SEG_UNKNOWN, FREE_SEG_BAD = 1, 0x80


class MrhFreespaceParams(C.Structure):
    _fields_ = [("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("cell_shift", C.c_int32), ("reserved", C.c_uint32)]


class MrhCarveParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("rows", C.c_int32), ("cols", C.c_int32),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("step", C.c_float), ("margin", C.c_float), ("reserved", C.c_uint32 * 2)]


class MrhFreespaceBoxParams(C.Structure):
    _fields_ = [("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("min_weight", C.c_int32), ("surface_band", C.c_float), ("reserved", C.c_uint32 * 2)]


def normalize_directions(directions) -> np.ndarray:
    """d / len per ray in float32, len = sqrt((dx * dx + dy * dy) + dz * dz): what cast_rays(normalize=True) does on the host (a zero
    direction becomes NaN and is a bad ray)."""
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
        return (d / ln[:, None]).astype(np.float32)


# every symbol include/mrhash_remap.h declares (the HIP library only: the oracle has no map-to-map fusion)
REMAP_SYMBOLS = ("mrh_resample_map mrh_fuse_map").split()


class MrhRemapParams(C.Structure):
    _fields_ = [("dst_voxel_size", C.c_float), ("min_weight", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class MrhRemapInfo(C.Structure):
    _fields_ = [("source_blocks", C.c_uint64), ("candidate_blocks", C.c_uint64), ("records", C.c_uint64), ("valid_voxels", C.c_uint64), ("taken", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# every symbol include/mrhash_align.h declares (the HIP library only: the oracle has no registration)
ALIGN_SYMBOLS = ("mrh_align_map").split()
ALIGN_OK, ALIGN_LOST = 0, 1


class MrhAlignParams(C.Structure):
    _fields_ = [("band", C.c_float), ("dist_max", C.c_float), ("iterations", C.c_int32), ("min_samples", C.c_uint32), ("min_weight", C.c_uint32),
                ("pivot", C.c_float * 3), ("extent", C.c_float), ("reserved", C.c_uint32 * 3)]


class MrhAlignInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations_done", C.c_int32), ("source_blocks", C.c_uint64), ("samples", C.c_uint64), ("accepted", C.c_uint64),
                ("rms", C.c_double), ("pivot", C.c_float * 3), ("extent", C.c_float), ("sums", C.c_int64 * 32)]

    def as_dict(self) -> dict:
        return dict(status=int(self.status), iterations_done=int(self.iterations_done), source_blocks=int(self.source_blocks), samples=int(self.samples),
                    accepted=int(self.accepted), rms=float(self.rms), pivot=np.array(self.pivot[:], dtype=np.float32), extent=np.float32(self.extent),
                    sums=np.array(self.sums[:], dtype=np.int64))


# every symbol include/mrhash_track.h declares (the HIP library only: the oracle does not track)
TRACK_SYMBOLS = ("mrh_track_depth mrh_track_depth_device mrh_track_scan mrh_track_scan_device").split()
TRACK_OK, TRACK_LOST = 0, 1


class MrhTrackParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("rows", C.c_int32), ("cols", C.c_int32),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("step", C.c_float), ("dist_max", C.c_float),
                ("iterations", C.c_int32), ("min_pixels", C.c_uint32)]


class MrhTrackInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations_done", C.c_int32), ("pixels", C.c_uint64), ("rms", C.c_double), ("sums", C.c_int64 * 32)]

    def as_dict(self) -> dict:
        return dict(status=int(self.status), iterations_done=int(self.iterations_done), pixels=int(self.pixels), rms=float(self.rms),
                    sums=np.array(self.sums[:], dtype=np.int64))


# every symbol include/mrhash_sdftrack.h declares (the HIP library only); the info and the status values are tracking's
SDFTRACK_SYMBOLS = ("mrh_track_depth_sdf mrh_track_depth_sdf_device mrh_track_points_sdf mrh_track_points_sdf_device").split()


class MrhSdftrackParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("rows", C.c_int32), ("cols", C.c_int32),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("band", C.c_float), ("iterations", C.c_int32), ("min_pixels", C.c_uint32),
                ("reserved", C.c_uint32)]


# every symbol include/mrhash_normals.h declares (the HIP library only: the oracle is given its normals)
NORMALS_SYMBOLS = ("mrh_estimate_normals_device mrh_estimate_normals mrh_get_normals").split()


class MrhNormalsParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("min_points", C.c_uint32), ("min_spread", C.c_float), ("max_flatness", C.c_float)]


class MrhNormalsInfo(C.Structure):
    _fields_ = [("points", C.c_uint64), ("estimated", C.c_uint64), ("fallback", C.c_uint64), ("missing", C.c_uint64), ("cells", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MrhCommStatus(C.Structure):
    _fields_ = [("rccl_ranks", C.c_int), ("rccl_rank", C.c_int), ("rccl_device", C.c_int), ("rccl_version", C.c_int), ("async_error", C.c_int),
                ("async_error_string", C.c_char * 64), ("library_path", C.c_char * 256)]


class MrhCommMergeInfo(C.Structure):
    _fields_ = [("blocks_sent", C.c_uint64), ("blocks_received", C.c_uint64), ("bytes_sent", C.c_uint64), ("blocks_kept", C.c_uint64)]


class MrhCommPhases(C.Structure):
    _fields_ = [("pack_ms", C.c_float), ("counts_ms", C.c_float), ("collective_ms", C.c_float), ("unpack_ms", C.c_float),
                ("bytes_out", C.c_uint64), ("bytes_in", C.c_uint64), ("allreduce_ms_sum", C.c_float), ("allreduce_count", C.c_uint32)]


class MrhError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mrh error {code}: {msg}")
        self.code = code


def _declare(lib: C.CDLL) -> C.CDLL:
    P = C.POINTER
    lib.mrh_create.argtypes = [P(MrhParams), P(C.c_void_p)]
    lib.mrh_destroy.argtypes = [C.c_void_p]
    lib.mrh_reset.argtypes = [C.c_void_p]
    lib.mrh_last_error.argtypes = [C.c_void_p]
    lib.mrh_last_error.restype = C.c_char_p
    lib.mrh_set_camera.argtypes = [C.c_void_p] + [C.c_float] * 4 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
    lib.mrh_set_pose.argtypes = [C.c_void_p, P(C.c_float), P(C.c_float)]
    lib.mrh_upload_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.mrh_upload_rgb.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.mrh_set_depth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.mrh_set_rgb_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.mrh_integrate.argtypes = [C.c_void_p, C.c_int]
    lib.mrh_upload_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.mrh_upload_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.mrh_set_points_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.mrh_integrate_points.argtypes = [C.c_void_p, C.c_int]
    lib.mrh_set_scan_layout.argtypes = [C.c_void_p, C.c_int]
    lib.mrh_detect_scan_layout.argtypes = [C.c_void_p, C.c_uint64]
    lib.mrh_get_free_blocks.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_int64)]
    lib.mrh_peek_free_blocks.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_int64), P(C.c_uint64)]
    lib.mrh_stream_out.argtypes = [C.c_void_p, P(C.c_float), C.c_float, C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_uint64)]
    lib.mrh_splat_seeds.argtypes = [C.c_void_p, C.c_float, C.c_int, P(C.c_void_p), P(C.c_uint64)]
    lib.mrh_get_qtree_leaves.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_uint64)]
    lib.mrh_peek_error_flags.argtypes = [C.c_void_p, P(C.c_uint32)]
    lib.mrh_set_sharding.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.mrh_pack_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_void_p), P(C.c_uint64), P(C.c_int)]
    lib.mrh_unpack_blocks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int, P(C.c_uint64)]
    lib.mrh_drop_blocks.argtypes = [C.c_void_p, C.c_int, P(C.c_uint64)]
    lib.mrh_integrate_resume.argtypes = [C.c_void_p]
    lib.mrh_exchange_buffer.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_uint64), P(C.c_int)]
    lib.mrh_sync.argtypes = [C.c_void_p]
    lib.mrh_extract_triangles.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_uint64)]
    lib.mrh_extract_mesh.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_uint64), P(C.c_void_p), P(C.c_uint64), P(C.c_void_p)]
    lib.mrh_mesh_merge_begin.argtypes = [C.c_void_p]
    lib.mrh_mesh_merge_end.argtypes = [C.c_void_p, P(C.c_uint64)]
    lib.mrh_get_stats.argtypes = [C.c_void_p, P(MrhStats)]
    lib.mrh_set_profile.argtypes = [C.c_void_p, C.c_int]
    lib.mrh_dump_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_uint64)]
    lib.mrh_get_voxel.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, P(C.c_int)]
    lib.mrh_import_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.mrh_get_triangle_blocks.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_void_p), P(C.c_uint64)]
    lib.mrh_process_triangles.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.mrh_get_triangles_device.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_uint64), P(C.c_int)]
    lib.mrh_process_triangle_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    lib.mrh_selftest_division.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, P(C.c_uint64)]
    lib.mrh_version.argtypes = []
    lib.mrh_version.restype = C.c_char_p
    for name in ABI_SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("mrh_last_error", "mrh_version"):
            fn.restype = C.c_int
    if hasattr(lib, "mrh_comm_create"):  # include/mrhash_comm.h
        lib.mrh_comm_unique_id.argtypes = [C.c_void_p]
        lib.mrh_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_void_p)]
        lib.mrh_comm_destroy.argtypes = [C.c_void_p]
        lib.mrh_comm_last_error.argtypes = [C.c_void_p]
        lib.mrh_comm_last_error.restype = C.c_char_p
        lib.mrh_comm_size.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int)]
        lib.mrh_comm_barrier.argtypes = [C.c_void_p]
        lib.mrh_comm_allreduce_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        lib.mrh_comm_allgather_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.mrh_comm_attach.argtypes = [C.c_void_p, C.c_void_p]
        lib.mrh_comm_exchange_halo.argtypes = [C.c_void_p, P(C.c_uint64)]
        lib.mrh_comm_merge_submaps.argtypes = [C.c_void_p, C.c_int, P(MrhCommMergeInfo)]
        lib.mrh_comm_gather_mesh.argtypes = [C.c_void_p, C.c_int, P(C.c_uint64)]
        lib.mrh_comm_phase_times.argtypes = [C.c_void_p, P(MrhCommPhases)]
        lib.mrh_comm_status.argtypes = [C.c_void_p, P(MrhCommStatus)]
        for name in COMM_SYMBOLS:
            if name != "mrh_comm_last_error":
                getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_raycast"):  # include/mrhash_raycast.h
        lib.mrh_raycast.argtypes = [C.c_void_p, P(MrhRaycastParams), P(C.c_float), P(C.c_float), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p)]
        lib.mrh_raycast_device.argtypes = [C.c_void_p, P(MrhRaycastParams), P(C.c_float), P(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mrh_raycast_spherical.argtypes = lib.mrh_raycast.argtypes + [P(C.c_void_p)]
        lib.mrh_raycast_spherical_device.argtypes = lib.mrh_raycast_device.argtypes + [C.c_void_p]
        for name in RAYCAST_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_esdf"):  # include/mrhash_esdf.h
        lib.mrh_esdf.argtypes = [C.c_void_p, P(MrhEsdfParams), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p)]
        lib.mrh_esdf_device.argtypes = [C.c_void_p, P(MrhEsdfParams), C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ESDF_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_query_points"):  # include/mrhash_query.h
        lib.mrh_query_points.argtypes = [C.c_void_p, P(MrhQueryParams), C.c_void_p, C.c_uint64, P(C.c_float), P(C.c_float), P(C.c_void_p), P(C.c_void_p),
                                         P(C.c_void_p), P(C.c_void_p)]
        lib.mrh_query_points_device.argtypes = [C.c_void_p, P(MrhQueryParams), C.c_void_p, C.c_uint64, P(C.c_float), P(C.c_float), C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
        for name in QUERY_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_cast_rays"):  # include/mrhash_rays.h
        lib.mrh_cast_rays.argtypes = [C.c_void_p, P(MrhRaysParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_float), P(C.c_float)] + [P(C.c_void_p)] * 6
        lib.mrh_cast_rays_device.argtypes = [C.c_void_p, P(MrhRaysParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_float), P(C.c_float)] + [C.c_void_p] * 6
        for name in RAYS_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_freespace_create"):  # include/mrhash_freespace.h
        F = P(C.c_float)
        lib.mrh_freespace_create.argtypes = [C.c_void_p, P(MrhFreespaceParams)]
        lib.mrh_freespace_clear.argtypes = [C.c_void_p]
        lib.mrh_freespace_destroy.argtypes = [C.c_void_p]
        lib.mrh_freespace_carve_depth.argtypes = [C.c_void_p, P(MrhCarveParams), C.c_void_p, F, F]
        lib.mrh_freespace_carve_depth_device.argtypes = lib.mrh_freespace_carve_depth.argtypes
        lib.mrh_freespace_carve_points.argtypes = [C.c_void_p, P(MrhCarveParams), C.c_void_p, C.c_uint64, F, F]
        lib.mrh_freespace_carve_points_device.argtypes = lib.mrh_freespace_carve_points.argtypes
        lib.mrh_freespace_box.argtypes = [C.c_void_p, P(MrhFreespaceBoxParams), P(C.c_void_p)]
        lib.mrh_freespace_box_device.argtypes = [C.c_void_p, P(MrhFreespaceBoxParams), C.c_void_p]
        lib.mrh_freespace_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, P(C.c_void_p), P(C.c_void_p)]
        lib.mrh_freespace_segments_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p]
        for name in FREESPACE_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_resample_map"):  # include/mrhash_remap.h
        lib.mrh_resample_map.argtypes = [C.c_void_p, P(MrhRemapParams), P(C.c_float), P(C.c_float), P(C.c_void_p), P(C.c_uint64), P(MrhRemapInfo)]
        lib.mrh_fuse_map.argtypes = [C.c_void_p, C.c_void_p, P(MrhRemapParams), P(C.c_float), P(C.c_float), P(MrhRemapInfo)]
        for name in REMAP_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_align_map"):  # include/mrhash_align.h
        lib.mrh_align_map.argtypes = [C.c_void_p, C.c_void_p, P(MrhAlignParams), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(MrhAlignInfo)]
        lib.mrh_align_map.restype = C.c_int
    if hasattr(lib, "mrh_track_depth"):  # include/mrhash_track.h
        lib.mrh_track_depth.argtypes = [C.c_void_p, P(MrhTrackParams), C.c_void_p, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                        P(MrhTrackInfo)]
        lib.mrh_track_depth_device.argtypes = lib.mrh_track_depth.argtypes
        names = TRACK_SYMBOLS[:2]
        if hasattr(lib, "mrh_track_scan"):  # an A/B build from before scan tracking has the depth pair only (tools/bench_with_lib.py)
            lib.mrh_track_scan.argtypes = lib.mrh_track_depth.argtypes[:3] + [C.c_size_t] + lib.mrh_track_depth.argtypes[3:]
            lib.mrh_track_scan_device.argtypes = lib.mrh_track_scan.argtypes
            names = TRACK_SYMBOLS
        for name in names:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_track_depth_sdf"):  # include/mrhash_sdftrack.h
        lib.mrh_track_depth_sdf.argtypes = [C.c_void_p, P(MrhSdftrackParams), C.c_void_p, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                            P(MrhTrackInfo)]
        lib.mrh_track_depth_sdf_device.argtypes = lib.mrh_track_depth_sdf.argtypes
        lib.mrh_track_points_sdf.argtypes = lib.mrh_track_depth_sdf.argtypes[:3] + [C.c_size_t] + lib.mrh_track_depth_sdf.argtypes[3:]
        lib.mrh_track_points_sdf_device.argtypes = lib.mrh_track_points_sdf.argtypes
        for name in SDFTRACK_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mrh_estimate_normals"):  # include/mrhash_normals.h
        lib.mrh_estimate_normals_device.argtypes = [C.c_void_p, P(MrhNormalsParams), C.c_void_p, C.c_uint64, C.c_void_p]
        lib.mrh_estimate_normals.argtypes = [C.c_void_p, P(MrhNormalsParams), P(MrhNormalsInfo)]
        lib.mrh_get_normals.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_uint64), P(MrhNormalsInfo)]
        for name in NORMALS_SYMBOLS:
            getattr(lib, name).restype = C.c_int
    return lib


def _copy_out(ptr: C.c_void_p, count: int, dtype, shape) -> np.ndarray:
    """A numpy copy, shaped `shape`, of the `count` elements of `dtype` a call handed out at `ptr` (the memory stays the library's).
    A null pointer holds nothing: the first dimension becomes 0."""
    if not ptr.value:
        count, shape = 0, (0,) + tuple(shape)[1:]
    if count == 0:
        return np.zeros(shape, dtype)
    return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr.value), dtype=dtype).reshape(shape).copy()


def load_library(path: str) -> C.CDLL:
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found - build it first (python -c 'import __graft_entry__ as g; g.build()')"
        )
    return _declare(C.CDLL(path))


_hip_lib: Optional[C.CDLL] = None


def load_hip() -> C.CDLL:
    """The product library. Raises (never falls back) when it has not been built."""
    global _hip_lib
    if _hip_lib is None:
        from ._runtime import torch_first

        torch_first()  # see _runtime.py: torch's HIP runtime has to initialise before this library's
        _hip_lib = load_library(HIP_LIB_PATH)
    return _hip_lib


class Comm:
    """RCCL communicator behind the C ABI (include/mrhash_comm.h): one per process / GPU.  `unique_id()` on one rank, the 128
    bytes handed to the others by the host (mrhash_amd.parallel.rendezvous), then `Comm(lib, id, rank, world, device)`."""

    def __init__(self, lib: C.CDLL, uid: bytes, rank: int, world: int, device_id: int = 0):
        self.lib, self.rank, self.world, self.device_id = lib, rank, world, device_id
        self._comm = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        rc = lib.mrh_comm_create(buf, rank, world, device_id, C.byref(self._comm))
        if rc != MRH_OK:
            raise MrhError(rc, lib.mrh_comm_last_error(None).decode())

    @staticmethod
    def unique_id(lib: C.CDLL) -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        rc = lib.mrh_comm_unique_id(buf)
        if rc != MRH_OK:
            raise MrhError(rc, lib.mrh_comm_last_error(None).decode())
        return bytes(buf)

    def _check(self, rc: int):
        if rc != MRH_OK:
            raise MrhError(rc, self.lib.mrh_comm_last_error(self._comm).decode())

    def barrier(self):
        self._check(self.lib.mrh_comm_barrier(self._comm))

    def allreduce(self, values, op: int = COMM_SUM) -> np.ndarray:
        a = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64).copy()
        self._check(self.lib.mrh_comm_allreduce_f64(self._comm, a.ctypes.data, a.size, op))
        return a

    def allgather_i64(self, values) -> np.ndarray:
        """[world, len(values)] int64: every rank's `values`."""
        a = np.ascontiguousarray(np.atleast_1d(values), dtype=np.int64)
        out = np.empty((self.world, a.size), dtype=np.int64)
        self._check(self.lib.mrh_comm_allgather_bytes(self._comm, a.ctypes.data, a.nbytes, out.ctypes.data))
        return out

    def status(self) -> dict:
        """What RCCL itself says about this communicator (mrh_comm_status): ranks it sees, its rank and device, the pending
        asynchronous error, version and library path."""
        st = MrhCommStatus()
        self._check(self.lib.mrh_comm_status(self._comm, C.byref(st)))
        return {"rccl_ranks": int(st.rccl_ranks), "rccl_rank": int(st.rccl_rank), "rccl_device": int(st.rccl_device), "rccl_version": int(st.rccl_version),
                "async_error": int(st.async_error), "async_error_string": st.async_error_string.decode(), "library_path": st.library_path.decode()}

    def close(self):
        if self._comm:
            self.lib.mrh_comm_destroy(self._comm)
            self._comm = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class Params:
    sdf_truncation: float
    sdf_truncation_scale: float = 0.0
    integration_weight_sample: int = 1
    integration_weight_max: int = 255
    virtual_voxel_size: float = 0.01
    n_frames_invalidate_voxels: int = 0
    voxel_extents_scale: int = 1
    marching_cubes_threshold: float = 1.5
    min_weight_threshold: int = 5
    projective_sdf: bool = True
    min_depth: float = 0.01
    max_depth: float = 30.0
    sdf_var_threshold: float = 0.0
    vertices_merging_threshold: float = 0.0
    num_sdf_blocks: int = 0
    hash_slots: int = 0
    max_triangles: int = 0
    device_id: int = 0
    shard_rank: int = 0
    shard_count: int = 1
    shard_chunk_log2: int = 0

    def to_c(self) -> MrhParams:
        p = MrhParams()
        p.abi_version = MRH_ABI_VERSION
        for f in (
            "sdf_truncation sdf_truncation_scale integration_weight_sample integration_weight_max "
            "virtual_voxel_size n_frames_invalidate_voxels voxel_extents_scale marching_cubes_threshold "
            "min_weight_threshold min_depth max_depth sdf_var_threshold vertices_merging_threshold "
            "num_sdf_blocks hash_slots max_triangles device_id shard_rank shard_count shard_chunk_log2"
        ).split():
            setattr(p, f, getattr(self, f))
        p.projective_sdf = 1 if self.projective_sdf else 0
        return p


class Engine:
    """One fusion context behind the C ABI (HIP product library or, in tests, the oracle)."""

    def __init__(self, lib: C.CDLL, params: Params):
        self.lib = lib
        # a private copy: set_sharding / comm_merge_submaps record the context's sharding here, and a caller that builds
        # several engines from one Params object must not find the later ones sharded like the first
        self.params = replace(params)
        self._ctx = C.c_void_p()
        cp = params.to_c()
        rc = lib.mrh_create(C.byref(cp), C.byref(self._ctx))
        if rc != MRH_OK:
            raise MrhError(rc, lib.mrh_last_error(None).decode())
        self._keep = []  # device tensors referenced by *_device setters
        self._comm_ref = None  # keeps an attached Comm alive

    # -- helpers -------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != MRH_OK:
            raise MrhError(rc, self.lib.mrh_last_error(self._ctx).decode())

    def close(self):
        if self._ctx:
            self.lib.mrh_destroy(self._ctx)
            self._ctx = C.c_void_p()
            self._comm_ref = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- inputs --------------------------------------------------------------------------------
    def set_camera(self, fx, fy, cx, cy, rows, cols, min_depth, max_depth, model=PINHOLE):
        self._check(self.lib.mrh_set_camera(self._ctx, fx, fy, cx, cy, rows, cols, min_depth, max_depth, model))

    def set_pose(self, R: np.ndarray, t: np.ndarray):
        R = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        self._check(
            self.lib.mrh_set_pose(self._ctx, R.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float)))
        )

    def upload_depth(self, depth: np.ndarray):
        if depth.ndim != 2:
            raise RuntimeError("setDepthImage|input should be a 2D numpy array")
        d = np.ascontiguousarray(depth, dtype=np.float32)
        self._check(self.lib.mrh_upload_depth(self._ctx, d.ctypes.data, d.shape[0], d.shape[1]))

    def upload_rgb(self, rgb: np.ndarray):
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise RuntimeError("setRGBImage|input should be a 3D numpy array with 3 channels")
        r = np.ascontiguousarray(rgb, dtype=np.uint8)
        self._check(self.lib.mrh_upload_rgb(self._ctx, r.ctypes.data, r.shape[0], r.shape[1]))

    def set_depth_device(self, ptr: int, rows: int, cols: int):
        self._check(self.lib.mrh_set_depth_device(self._ctx, ptr, rows, cols))

    def set_rgb_device(self, ptr: int, rows: int, cols: int):
        self._check(self.lib.mrh_set_rgb_device(self._ctx, ptr, rows, cols))

    # -- hot path ------------------------------------------------------------------------------
    def upload_points(self, xyz: np.ndarray):
        """GeoWrapper.setPointCloud: float32 [N, 3] points in the sensor frame (copied)."""
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise RuntimeError("GeoWrapper::setPointCloud|input should be a 2D numpy array with 3 columns")
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        self._check(self.lib.mrh_upload_points(self._ctx, a.ctypes.data, a.shape[0]))

    def upload_normals(self, nxyz: np.ndarray):
        """One normal per point of the current scan, float32 [N, 3] (copied): the normal-direction SDF (projective_sdf = False)."""
        a = np.ascontiguousarray(nxyz, dtype=np.float32).reshape(-1, 3)
        self._check(self.lib.mrh_upload_normals(self._ctx, a.ctypes.data, a.shape[0]))

    def set_points_device(self, ptr: int, n: int):
        self._check(self.lib.mrh_set_points_device(self._ctx, ptr, n))

    def set_scan_layout(self, row_len: int):
        """Points per row of the caller's organised scans (0: look at host clouds, < 0: never): a hint for the beam order, never for the result."""
        self._check(self.lib.mrh_set_scan_layout(self._ctx, int(row_len)))

    def integrate_points(self, n_frames_invalidate: int = -1) -> bool:
        """One scan.  Returns True when a sharded context stopped for the starve z-buffer reduction (see integrate())."""
        rc = self.lib.mrh_integrate_points(self._ctx, n_frames_invalidate)
        if rc == MRH_PENDING_EXCHANGE:
            return True
        self._check(rc)
        return False

    def integrate(self, n_frames_invalidate: int = -1) -> bool:
        """Enqueues one frame.  Returns True when a sharded context stopped for a min-reduction over ranks
        (MRH_PENDING_EXCHANGE): reduce `exchange_buffer()` and call `integrate_resume()` until it returns False
        (mrhash_amd.parallel.integrate does this)."""
        rc = self.lib.mrh_integrate(self._ctx, n_frames_invalidate)
        if rc == MRH_PENDING_EXCHANGE:
            return True
        self._check(rc)
        return False

    def integrate_resume(self) -> bool:
        rc = self.lib.mrh_integrate_resume(self._ctx)
        if rc == MRH_PENDING_EXCHANGE:
            return True
        self._check(rc)
        return False

    def exchange_buffer(self) -> Tuple[int, int, bool]:
        """(pointer, number of int64 elements, is_device_memory) of the buffer awaiting a MIN all-reduce."""
        ptr, n, dev = C.c_void_p(), C.c_uint64(), C.c_int()
        self._check(self.lib.mrh_exchange_buffer(self._ctx, C.byref(ptr), C.byref(n), C.byref(dev)))
        return int(ptr.value), int(n.value), bool(dev.value)

    def sync(self):
        self._check(self.lib.mrh_sync(self._ctx))

    def reset(self):
        self._check(self.lib.mrh_reset(self._ctx))

    def set_profile(self, enabled: bool):
        self._check(self.lib.mrh_set_profile(self._ctx, 1 if enabled else 0))

    def stats(self) -> MrhStats:
        s = MrhStats()
        self._check(self.lib.mrh_get_stats(self._ctx, C.byref(s)))
        return s

    # -- outputs -------------------------------------------------------------------------------
    def extract_triangles(self, soup: bool = True):
        """[T, 3] structured array of vertices (p[3], c[3]) in canonical triangle order.  soup=False: marching cubes and
        the mesh post-process run, the triangle soup stays on the device and only the triangle count is returned."""
        ptr = C.c_void_p()
        n = C.c_uint64()
        if not soup:
            self._check(self.lib.mrh_extract_triangles(self._ctx, None, C.byref(n)))
            return int(n.value)
        self._check(self.lib.mrh_extract_triangles(self._ctx, C.byref(ptr), C.byref(n)))
        return _copy_out(ptr, 3 * n.value, TRI_DTYPE, (n.value, 3))

    def extract_mesh(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(V f64[nv,3], F i32[nf,3], C f64[nv,3]) of the last extract_triangles()."""
        pv, pf, pc = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nv, nf = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mrh_extract_mesh(self._ctx, C.byref(pv), C.byref(nv), C.byref(pf), C.byref(nf), C.byref(pc)))
        return (_copy_out(pv, 3 * nv.value, np.float64, (nv.value, 3)), _copy_out(pf, 3 * nf.value, np.int32, (nf.value, 3)),
                _copy_out(pc, 3 * nv.value, np.float64, (nv.value, 3)))

    def mesh_merge_begin(self):
        """MeshExtractor::merge_mesh_: until mesh_merge_end() every extract_triangles() adds to the running mesh."""
        self._check(self.lib.mrh_mesh_merge_begin(self._ctx))

    def mesh_merge_end(self) -> int:
        n = C.c_uint64()
        self._check(self.lib.mrh_mesh_merge_end(self._ctx, C.byref(n)))
        return int(n.value)

    def free_blocks(self) -> Tuple[int, int]:
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.mrh_get_free_blocks(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def splat_seeds(self, qtree_thresh: float = 0.1, qtree_min_pixel_size: int = 1) -> np.ndarray:
        """3DGS splat seeds of the current frame (call after integrate()): quad-tree over the colour image, one seed
        per leaf whose centre lands in a voxel of weight 1.  Returns a SEED_DTYPE array in canonical (leaf) order."""
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self.lib.mrh_splat_seeds(self._ctx, qtree_thresh, qtree_min_pixel_size, C.byref(ptr), C.byref(n)))
        return _copy_out(ptr, n.value, SEED_DTYPE, (n.value,))

    def qtree_leaves(self) -> np.ndarray:
        """Leaves of the quad-tree of the last splat_seeds() call, canonical order (LEAF_DTYPE)."""
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self.lib.mrh_get_qtree_leaves(self._ctx, C.byref(ptr), C.byref(n)))
        return _copy_out(ptr, n.value, LEAF_DTYPE, (n.value,))

    def peek_free_blocks(self) -> Tuple[int, int, int]:
        """(free fine, free coarse, frames behind) without waiting for the device (mrh_peek_free_blocks)."""
        a, b, n = C.c_int64(), C.c_int64(), C.c_uint64()
        self._check(self.lib.mrh_peek_free_blocks(self._ctx, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def peek_error_flags(self) -> int:
        f = C.c_uint32()
        self._check(self.lib.mrh_peek_error_flags(self._ctx, C.byref(f)))
        return int(f.value)

    # -- multi-GPU: RCCL behind the C ABI (include/mrhash_comm.h) -----------------------------------
    def attach_comm(self, comm: Optional["Comm"]):
        """While attached, a tile-sharded context runs the starve all-reduces itself (integrate() never returns True)."""
        self._check(self.lib.mrh_comm_attach(self._ctx, comm._comm if comm is not None else None))
        self._comm_ref = comm

    def comm_exchange_halo(self) -> int:
        n = C.c_uint64()
        self._check(self.lib.mrh_comm_exchange_halo(self._ctx, C.byref(n)))
        return int(n.value)

    def comm_merge_submaps(self, chunk_log2: int = 3) -> dict:
        info = MrhCommMergeInfo()
        self._check(self.lib.mrh_comm_merge_submaps(self._ctx, chunk_log2, C.byref(info)))
        self.params.shard_chunk_log2 = chunk_log2
        return {"sent": int(info.blocks_sent), "received": int(info.blocks_received), "bytes": int(info.bytes_sent), "kept": int(info.blocks_kept)}

    def comm_gather_mesh(self, root: int = 0) -> int:
        n = C.c_uint64()
        self._check(self.lib.mrh_comm_gather_mesh(self._ctx, root, C.byref(n)))
        return int(n.value)

    def comm_phase_times(self) -> dict:
        p = MrhCommPhases()
        self._check(self.lib.mrh_comm_phase_times(self._ctx, C.byref(p)))
        return {k: (float(getattr(p, k)) if k.endswith("_ms") or k.endswith("_sum") else int(getattr(p, k))) for k, _ in MrhCommPhases._fields_}

    # -- multi-GPU block exchange ----------------------------------------------------------------
    def set_sharding(self, rank: int, count: int, chunk_log2: int = 0):
        self._check(self.lib.mrh_set_sharding(self._ctx, rank, count, chunk_log2))
        self.params.shard_rank, self.params.shard_count, self.params.shard_chunk_log2 = rank, count, chunk_log2

    def pack_blocks(self, mode: int, rank_arg: int = 0) -> Tuple[int, int, bool]:
        """(pointer to mrh_block_record[n], n, is_device_memory); the buffer belongs to the context until the next pack."""
        ptr, n, dev = C.c_void_p(), C.c_uint64(), C.c_int()
        self._check(self.lib.mrh_pack_blocks(self._ctx, mode, rank_arg, C.byref(ptr), C.byref(n), C.byref(dev)))
        return int(ptr.value or 0), int(n.value), bool(dev.value)

    def unpack_blocks(self, mode: int, ptr: int, n: int, is_device: bool) -> int:
        taken = C.c_uint64()
        self._check(self.lib.mrh_unpack_blocks(self._ctx, mode, ptr, n, 1 if is_device else 0, C.byref(taken)))
        return int(taken.value)

    def drop_blocks(self, mode: int) -> int:
        n = C.c_uint64()
        self._check(self.lib.mrh_drop_blocks(self._ctx, mode, C.byref(n)))
        return int(n.value)

    def stream_out(self, center, radius: float) -> Tuple[np.ndarray, np.ndarray]:
        """Streamer device half: blocks at distance >= radius from `center` (radius < 0: all) are copied out, ordered by
        block position, and removed from the device map.  Returns (descs, voxels[n, 512])."""
        cen = (C.c_float * 3)(*[float(v) for v in center])
        n = C.c_uint64()
        self._check(self.lib.mrh_stream_out(self._ctx, cen, radius, None, None, 0, C.byref(n)))
        descs = np.zeros(n.value, dtype=DESC_DTYPE)
        vox = np.zeros((n.value, 512), dtype=VOXEL_DTYPE)
        if n.value:
            self._check(self.lib.mrh_stream_out(self._ctx, cen, radius, descs.ctypes.data, vox.ctypes.data, n.value, C.byref(n)))
        return descs, vox

    def dump_blocks(self) -> Tuple[np.ndarray, np.ndarray]:
        """Canonical dump: (descs sorted by (x,y,z), voxels[n,512]) in the reference Voxel layout."""
        n = C.c_uint64()
        self._check(self.lib.mrh_dump_blocks(self._ctx, None, None, 0, C.byref(n)))
        cap = max(int(n.value), 1)
        descs = np.zeros(cap, dtype=DESC_DTYPE)
        voxels = np.zeros((cap, 512), dtype=VOXEL_DTYPE)
        self._check(self.lib.mrh_dump_blocks(self._ctx, descs.ctypes.data, voxels.ctypes.data, cap, C.byref(n)))
        descs, voxels = descs[: n.value], voxels[: n.value]
        order = np.lexsort((descs["z"], descs["y"], descs["x"]))
        return descs[order], voxels[order]

    def import_blocks(self, descs: np.ndarray, voxels: np.ndarray):
        """Inverse of dump_blocks (restore a map, or bring halo blocks of other shards in)."""
        d = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
        v = np.ascontiguousarray(voxels, dtype=VOXEL_DTYPE).reshape(len(d), 512)
        self._check(self.lib.mrh_import_blocks(self._ctx, d.ctypes.data, v.ctypes.data, len(d)))

    def triangle_blocks(self) -> Tuple[np.ndarray, np.ndarray]:
        """(descs, per-block triangle counts) of the last extract_triangles(), canonical block order."""
        pd, pc, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self.lib.mrh_get_triangle_blocks(self._ctx, C.byref(pd), C.byref(pc), C.byref(n)))
        return _copy_out(pd, n.value, DESC_DTYPE, (n.value,)), _copy_out(pc, n.value, np.uint32, (n.value,))

    def triangles_device(self) -> Tuple[int, int, bool]:
        """(pointer, number of triangles, is_device_memory) of the soup of the last extraction / run merge, where the library keeps it."""
        ptr, n, dev = C.c_void_p(), C.c_uint64(), C.c_int()
        self._check(self.lib.mrh_get_triangles_device(self._ctx, C.byref(ptr), C.byref(n), C.byref(dev)))
        return int(ptr.value or 0), int(n.value), bool(dev.value)

    def process_triangle_runs(self, descs: np.ndarray, counts: np.ndarray, tris_ptr: int, n_tris: int, is_device: bool):
        """Per-block triangle runs of all ranks (descs / counts: host arrays; triangles: one buffer, device or host) ->
        canonical order + mesh post-process (rank 0 of a sharded extraction)."""
        d = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        self._check(self.lib.mrh_process_triangle_runs(self._ctx, d.ctypes.data, c.ctypes.data, len(d), tris_ptr, n_tris, 1 if is_device else 0))

    def process_triangles(self, tris: np.ndarray):
        t = np.ascontiguousarray(tris, dtype=TRI_DTYPE).reshape(-1, 3)
        self._check(self.lib.mrh_process_triangles(self._ctx, t.ctypes.data, len(t)))

    def selftest_division(self, samples: int = 1 << 26, seed: int = 1) -> int:
        n = C.c_uint64()
        self._check(self.lib.mrh_selftest_division(self._ctx, samples, seed, C.byref(n)))
        return int(n.value)

    # -- rendering (include/mrhash_raycast.h) ------------------------------------------------------
    @staticmethod
    def _raycast_args(fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step, normals, colors, points=False):
        p = MrhRaycastParams(fx, fy, cx, cy, int(rows), int(cols), min_depth, max_depth, step,
                             (RAYCAST_NORMALS if normals else 0) | (RAYCAST_COLORS if colors else 0) | (RAYCAST_POINTS if points else 0))
        R = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        return p, R, t

    def raycast(self, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, normals=True, colors=True):
        """Renders the map from the camera-to-world pose (R, t) with a pinhole camera (mrh_raycast).  Returns
        numpy copies (depth f32 [rows, cols], normals f32 [rows, cols, 3] or None, rgb u8 [rows, cols, 3] or None); a pixel
        without a hit is 0 in all three.  step = 0: half the context's truncation."""
        p, R, t = self._raycast_args(fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step, normals, colors)
        pd, pn, pc = C.c_void_p(), C.c_void_p(), C.c_void_p()
        F = C.POINTER(C.c_float)
        self._check(self.lib.mrh_raycast(self._ctx, C.byref(p), R.ctypes.data_as(F), t.ctypes.data_as(F), C.byref(pd),
                                         C.byref(pn) if normals else None, C.byref(pc) if colors else None))
        n = int(rows) * int(cols)

        depth = _copy_out(pd, n, np.float32, (rows, cols))
        nrm = _copy_out(pn, 3 * n, np.float32, (rows, cols, 3)) if normals else None
        rgb = _copy_out(pc, 3 * n, np.uint8, (rows, cols, 3)) if colors else None
        return depth, nrm, rgb

    def raycast_device(self, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, d_depth=0, d_normals=0, d_rgb=0):
        """mrh_raycast_device: enqueues the render into caller device buffers (integer pointers, e.g. hipmem.DeviceBuffer.ptr;
        0 = skip that image).  Ordered on the context's stream; finished by sync() or any blocking call."""
        p, R, t = self._raycast_args(fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step, bool(d_normals), bool(d_rgb))
        F = C.POINTER(C.c_float)
        self._check(self.lib.mrh_raycast_device(self._ctx, C.byref(p), R.ctypes.data_as(F), t.ctypes.data_as(F), d_depth or None,
                                                d_normals or None, d_rgb or None))

    def raycast_spherical(self, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, normals=True, colors=True, points=False):
        """Renders the map from the sensor-to-world pose (R, t) with a spherical camera (mrh_raycast_spherical):
        fx / fy in pixels per radian, cx / cy as set_camera(..., model=1) means them, min_depth / max_depth / step ranges along
        the ray.  Returns numpy copies (range f32 [rows, cols], normals f32 [rows, cols, 3] or None, rgb u8 [rows, cols, 3] or
        None, points f32 [rows * cols, 3] or None); the points are the crossings in the SENSOR frame, an organised scan of `cols`
        points per row that upload_points takes as it is.  A pixel without a hit is 0 in all four."""
        p, R, t = self._raycast_args(fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step, normals, colors, points)
        pd, pn, pc, pp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        F = C.POINTER(C.c_float)
        self._check(self.lib.mrh_raycast_spherical(self._ctx, C.byref(p), R.ctypes.data_as(F), t.ctypes.data_as(F), C.byref(pd),
                                                   C.byref(pn) if normals else None, C.byref(pc) if colors else None,
                                                   C.byref(pp) if points else None))
        n = int(rows) * int(cols)

        rng = _copy_out(pd, n, np.float32, (rows, cols))
        nrm = _copy_out(pn, 3 * n, np.float32, (rows, cols, 3)) if normals else None
        rgb = _copy_out(pc, 3 * n, np.uint8, (rows, cols, 3)) if colors else None
        pts = _copy_out(pp, 3 * n, np.float32, (n, 3)) if points else None
        return rng, nrm, rgb, pts

    def raycast_spherical_device(self, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, d_range=0, d_normals=0, d_rgb=0,
                                 d_points=0):
        """mrh_raycast_spherical_device: as raycast_device; d_points ([rows * cols, 3] float32) can go to set_points_device of
        another context after sync()."""
        p, R, t = self._raycast_args(fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step, bool(d_normals), bool(d_rgb), bool(d_points))
        F = C.POINTER(C.c_float)
        self._check(self.lib.mrh_raycast_spherical_device(self._ctx, C.byref(p), R.ctypes.data_as(F), t.ctypes.data_as(F), d_range or None,
                                                          d_normals or None, d_rgb or None, d_points or None))

    # -- distance fields (include/mrhash_esdf.h) ------------------------------------------------------
    @staticmethod
    def _esdf_params(origin, dims, max_distance_voxels, surface_band, min_weight, state, squared):
        o, n = [int(x) for x in origin], [int(x) for x in dims]
        if len(o) != 3 or len(n) != 3:
            raise ValueError("esdf: origin and dims are triples (x, y, z)")
        return MrhEsdfParams((C.c_int32 * 3)(*o), (C.c_int32 * 3)(*n), int(max_distance_voxels), int(min_weight), float(surface_band),
                             (ESDF_STATE if state else 0) | (ESDF_SQUARED if squared else 0))

    def esdf(self, origin, dims, max_distance_voxels, surface_band=0.0, min_weight=0, state=True, squared=False):
        """The Euclidean signed distance field of the box of finest voxels origin + [0, dims) (x, y, z), exact up to
        max_distance_voxels (mrh_esdf); only sites inside the box are seen, so pad it by the reach.  Returns
        numpy copies shaped [nz, ny, nx]: (dist f32 in metres, state u8 or None, d2 u32 or None).  State bits: ESDF_OBSERVED,
        ESDF_SITE, ESDF_INSIDE, ESDF_FAR; d2 of a far cell is ESDF_FAR_D2."""
        p = self._esdf_params(origin, dims, max_distance_voxels, surface_band, min_weight, state, squared)
        pd, ps, pq = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.mrh_esdf(self._ctx, C.byref(p), C.byref(pd), C.byref(ps) if state else None, C.byref(pq) if squared else None))
        nx, ny, nz = (int(x) for x in dims)
        n = nx * ny * nz
        box = (nz, ny, nx)
        return _copy_out(pd, n, np.float32, box), _copy_out(ps, n, np.uint8, box) if state else None, _copy_out(pq, n, np.uint32, box) if squared else None

    def esdf_device(self, origin, dims, max_distance_voxels, surface_band=0.0, min_weight=0, d_dist=0, d_state=0, d_d2=0):
        """mrh_esdf_device: enqueues the field into caller device buffers (integer pointers, e.g. hipmem.DeviceBuffer.ptr:
        [n] f32, [n] u8, [n] u32 with n = nx * ny * nz; d_dist is required, 0 = skip for the other two).  Ordered on the
        context's stream; finished by sync() or any blocking call."""
        p = self._esdf_params(origin, dims, max_distance_voxels, surface_band, min_weight, bool(d_state), bool(d_d2))
        self._check(self.lib.mrh_esdf_device(self._ctx, C.byref(p), d_dist or None, d_state or None, d_d2 or None))

    # -- point queries (include/mrhash_query.h) ------------------------------------------------------
    @staticmethod
    def _query_args(R, t, smooth, gradient, colour):
        if (R is None) != (t is None):
            raise ValueError("query: give both R and t, or neither")
        p = MrhQueryParams(QUERY_FIELD_SMOOTH if smooth else QUERY_FIELD_MAP, (QUERY_GRADIENT if gradient else 0) | (QUERY_COLOUR if colour else 0))
        F = C.POINTER(C.c_float)
        if R is None:
            return p, None, None, None
        R = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        return p, R.ctypes.data_as(F), t.ctypes.data_as(F), (R, t)  # the last: keeps the arrays alive across the call

    def query(self, points, R=None, t=None, smooth=False, gradient=True, colour=True):
        """TSDF distance, gradient and colour at points [n, 3] (mrh_query_points): world-frame points, or with
        (R, t) sensor-frame points and their sensor-to-world pose ((0, 0, 0) is then a missing return and refused).  smooth =
        False: the map's own field, the reference's trilinearInterpolation — piecewise constant inside a dual cell; smooth =
        True: the continuous field with its analytic gradient.  Returns numpy copies (dist f32 [n], grad f32 [n, 3] or None,
        rgbw u8 [n, 4] = r, g, b, weight or None, state u8 [n]: QUERY_BLOCK | QUERY_DIST | QUERY_GRAD | QUERY_COARSE |
        QUERY_REFUSED)."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(pts)
        p, pR, pt, _keep = self._query_args(R, t, smooth, gradient, colour)
        pd, pg, pc, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.mrh_query_points(self._ctx, C.byref(p), pts.ctypes.data if n else None, n, pR, pt, C.byref(pd), C.byref(pg) if gradient else None,
                                              C.byref(pc) if colour else None, C.byref(ps)))
        return (_copy_out(pd, n, np.float32, (n,)), _copy_out(pg, 3 * n, np.float32, (n, 3)) if gradient else None,
                _copy_out(pc, 4 * n, np.uint8, (n, 4)) if colour else None, _copy_out(ps, n, np.uint8, (n,)))

    def query_device(self, d_points, n, R=None, t=None, smooth=False, d_dist=0, d_grad=0, d_rgbw=0, d_state=0):
        """mrh_query_points_device: enqueues the query of n points at d_points ([n, 3] f32) into caller device buffers (integer
        pointers, e.g. hipmem.DeviceBuffer.ptr: [n] f32, [n, 3] f32, [n, 4] u8, [n] u8; d_dist and d_state are required, 0 = skip
        for the other two).  Ordered on the context's stream; finished by sync() or any blocking call."""
        p, pR, pt, _keep = self._query_args(R, t, smooth, bool(d_grad), bool(d_rgbw))
        self._check(self.lib.mrh_query_points_device(self._ctx, C.byref(p), d_points or None, int(n), pR, pt, d_dist or None, d_grad or None,
                                                     d_rgbw or None, d_state or None))

    # -- ray queries (include/mrhash_rays.h) ----------------------------------------------------------
    def _rays_args(self, max_range, min_range, step, R, t, normals, colors, counts):
        if (R is None) != (t is None):
            raise ValueError("cast_rays: give both R and t, or neither")
        p = MrhRaysParams(float(min_range), float(max_range), float(step), (RAYS_NORMALS if normals else 0) | (RAYS_COLORS if colors else 0) | (RAYS_COUNTS if counts else 0))
        if R is None:
            return p, None, None, None
        pR, pt, keep = self._pose_args(R, t)
        return p, pR, pt, keep

    def cast_rays(self, origins, directions, max_range, min_range=0.0, step=0.0, tmax=None, R=None, t=None, normals=True, colors=True, counts=True,
                  normalize=True):
        """Casts the rays origins [n, 3], directions [n, 3] through the map (mrh_cast_rays): world-frame rays, or with
        (R, t) sensor-frame rays and their sensor-to-world pose.  Samples lie at min_range + k * step (step 0 = half the truncation)
        up to max_range and, with tmax [n], up to each ray's own end.  normalize = True divides every direction on the host, in
        float32, by len = sqrt((dx * dx + dy * dy) + dz * dz) (normalize_directions), so ranges are metres; the C ABI never
        normalises: with normalize = False a range counts multiples of the direction.  Neighbouring rays of the list share a
        wave: order them so that neighbours are close in space.  Returns a dict of numpy copies: range f32 [n], status u8 [n]
        (RAY_HIT | RAY_UNKNOWN | RAY_INSIDE | RAY_BAD; 0 = every sample was observed free space), normals f32 [n, 3], rgb u8
        [n, 3], counts u32 [n, 2] = (n_free, n_unknown), first_unknown f32 [n]; an output that was not asked for is None."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        if len(d) != n:
            raise ValueError("cast_rays: %d origins, %d directions" % (n, len(d)))
        if normalize:
            d = normalize_directions(d)
        tm = None
        if tmax is not None:
            tm = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            if len(tm) != n:
                raise ValueError("cast_rays: %d rays, %d ends" % (n, len(tm)))
        p, pR, pt, _keep = self._rays_args(max_range, min_range, step, R, t, normals, colors, counts)
        pr, ps, pn, pc, pk, pf = (C.c_void_p() for _ in range(6))
        self._check(self.lib.mrh_cast_rays(self._ctx, C.byref(p), o.ctypes.data if n else None, d.ctypes.data if n else None,
                                           tm.ctypes.data if tm is not None and n else None, n, pR, pt, C.byref(pr), C.byref(ps), C.byref(pn) if normals else None,
                                           C.byref(pc) if colors else None, C.byref(pk) if counts else None, C.byref(pf) if counts else None))
        return {"range": _copy_out(pr, n, np.float32, (n,)), "status": _copy_out(ps, n, np.uint8, (n,)),
                "normals": _copy_out(pn, 3 * n, np.float32, (n, 3)) if normals else None, "rgb": _copy_out(pc, 3 * n, np.uint8, (n, 3)) if colors else None,
                "counts": _copy_out(pk, 2 * n, np.uint32, (n, 2)) if counts else None, "first_unknown": _copy_out(pf, n, np.float32, (n,)) if counts else None}

    def cast_rays_device(self, d_origins, d_directions, n, max_range, min_range=0.0, step=0.0, d_tmax=0, R=None, t=None, d_range=0, d_status=0, d_normals=0,
                         d_rgb=0, d_counts=0, d_first_unknown=0):
        """mrh_cast_rays_device: enqueues the cast of n rays at d_origins, d_directions ([n, 3] f32; d_tmax [n] f32 or 0) into caller
        device buffers (integer pointers, e.g. hipmem.DeviceBuffer.ptr: [n] f32, [n] u8, [n, 3] f32, [n, 3] u8, [n, 2] u32, [n] f32;
        d_range and d_status are required, 0 = skip for the others).  Directions are used as given.  Ordered on the context's
        stream; finished by sync() or any blocking call."""
        p, pR, pt, _keep = self._rays_args(max_range, min_range, step, R, t, bool(d_normals), bool(d_rgb), bool(d_counts or d_first_unknown))
        self._check(self.lib.mrh_cast_rays_device(self._ctx, C.byref(p), d_origins or None, d_directions or None, d_tmax or None, int(n), pR, pt, d_range or None,
                                                  d_status or None, d_normals or None, d_rgb or None, d_counts or None, d_first_unknown or None))

    def line_of_sight(self, a, b, step=0.0):
        """bool [n]: the segment a[i] -> b[i] ([n, 3] each, world frame) is free of surfaces AND of unobserved space.  One cast_rays
        with o = a, the unit direction towards b, tmax = |b - a| (float32, the norm of normalize_directions), min_range = 0, and
        the test status == 0.  A segment of length 0 has no direction: it is a bad ray, hence False."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        d = (np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3) - a).astype(np.float32)
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
        if len(a) == 0:
            return np.zeros(0, bool)
        finite = ln[np.isfinite(ln)]
        reach = float(finite.max()) if len(finite) else 0.0
        out = self.cast_rays(a, d, max_range=reach, min_range=0.0, step=step, tmax=ln, normals=False, colors=False, counts=False, normalize=True)
        return out["status"] == 0

    # -- the free-space layer (include/mrhash_freespace.h) ----------------------------------------------
    def freespace_create(self, origin, dims, cell_shift=3):
        """mrh_freespace_create: an empty layer over the box of cells origin + [0, dims) (x, y, z); a cell is
        2^cell_shift finest voxels per side.  Replaces an existing layer."""
        o, n = [int(x) for x in origin], [int(x) for x in dims]
        if len(o) != 3 or len(n) != 3:
            raise ValueError("freespace_create: origin and dims are triples (x, y, z)")
        p = MrhFreespaceParams((C.c_int32 * 3)(*o), (C.c_int32 * 3)(*n), int(cell_shift), 0)
        self._check(self.lib.mrh_freespace_create(self._ctx, C.byref(p)))

    def freespace_clear(self):
        """Every bit of the layer 0; the box stays."""
        self._check(self.lib.mrh_freespace_clear(self._ctx))

    def freespace_destroy(self):
        """The context has no layer afterwards."""
        self._check(self.lib.mrh_freespace_destroy(self._ctx))

    @staticmethod
    def _carve_params(fx, fy, cx, cy, rows, cols, min_depth, max_depth, step, margin):
        return MrhCarveParams(float(fx), float(fy), float(cx), float(cy), int(rows), int(cols), float(min_depth), float(max_depth), float(step), float(margin))

    def freespace_carve_depth(self, depth, fx, fy, cx, cy, R, t, min_depth, max_depth, step=0.0, margin=0.0):
        """Carves the depth image [rows, cols] f32 seen from the camera-to-world pose (R, t) into the layer (mrh_freespace_carve_depth):
        every pixel's ray sets the cells of its samples min_depth + k * step (step 0 = half a cell) up to depth - margin, or up to
        max_depth where the pixel saw nothing nearer.  Blocks; does not flush kept-back or pipelined frames."""
        d = np.ascontiguousarray(depth, dtype=np.float32)
        if d.ndim != 2:
            raise ValueError("freespace_carve_depth: the image is a 2D array")
        p = self._carve_params(fx, fy, cx, cy, d.shape[0], d.shape[1], min_depth, max_depth, step, margin)
        pR, pt, _keep = self._pose_args(R, t)
        self._check(self.lib.mrh_freespace_carve_depth(self._ctx, C.byref(p), d.ctypes.data, pR, pt))

    def freespace_carve_depth_device(self, d_depth, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, margin=0.0):
        """mrh_freespace_carve_depth_device: the same from a device image [rows, cols] f32 (an integer pointer).  Enqueues on the
        context's stream; the image must stay valid until sync() or a blocking call."""
        p = self._carve_params(fx, fy, cx, cy, rows, cols, min_depth, max_depth, step, margin)
        pR, pt, _keep = self._pose_args(R, t)
        self._check(self.lib.mrh_freespace_carve_depth_device(self._ctx, C.byref(p), d_depth or None, pR, pt))

    def freespace_carve_points(self, points, R, t, min_depth, max_depth, step=0.0, margin=0.0):
        """Carves the sensor-frame points [n, 3] f32 seen from the sensor-to-world pose (R, t) (mrh_freespace_carve_points): every
        point's ray from the sensor sets the cells of its samples up to min(range, max_depth) - margin.  Blocks."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        p = self._carve_params(0, 0, 0, 0, 0, 0, min_depth, max_depth, step, margin)
        pR, pt, _keep = self._pose_args(R, t)
        self._check(self.lib.mrh_freespace_carve_points(self._ctx, C.byref(p), pts.ctypes.data if len(pts) else None, len(pts), pR, pt))

    def freespace_carve_points_device(self, d_points, n, R, t, min_depth, max_depth, step=0.0, margin=0.0):
        """mrh_freespace_carve_points_device: the same from a device list [n, 3] f32 (an integer pointer).  Enqueues."""
        p = self._carve_params(0, 0, 0, 0, 0, 0, min_depth, max_depth, step, margin)
        pR, pt, _keep = self._pose_args(R, t)
        self._check(self.lib.mrh_freespace_carve_points_device(self._ctx, C.byref(p), d_points or None, int(n), pR, pt))

    @staticmethod
    def _freespace_box_params(origin, dims, min_weight, surface_band):
        o, n = [int(x) for x in origin], [int(x) for x in dims]
        if len(o) != 3 or len(n) != 3:
            raise ValueError("freespace_box: origin and dims are triples (x, y, z)")
        return MrhFreespaceBoxParams((C.c_int32 * 3)(*o), (C.c_int32 * 3)(*n), int(min_weight), float(surface_band))

    def freespace_box(self, origin, dims, min_weight=0, surface_band=0.0):
        """The state byte of every cell of the box origin + [0, dims) of cells (mrh_freespace_box): a numpy copy [nz, ny, nx] u8 of
        FREE_FREE | FREE_OBSERVED | FREE_OCCUPIED | FREE_FRONTIER.  The frontier looks at neighbours inside the box only: pad by one
        cell.  The box may extend beyond the layer."""
        p = self._freespace_box_params(origin, dims, min_weight, surface_band)
        ps = C.c_void_p()
        self._check(self.lib.mrh_freespace_box(self._ctx, C.byref(p), C.byref(ps)))
        nx, ny, nz = (int(x) for x in dims)
        return _copy_out(ps, nx * ny * nz, np.uint8, (nz, ny, nx))

    def freespace_box_device(self, origin, dims, d_state, min_weight=0, surface_band=0.0):
        """mrh_freespace_box_device: enqueues the box into the caller's device buffer of nx * ny * nz bytes (an integer pointer)."""
        p = self._freespace_box_params(origin, dims, min_weight, surface_band)
        self._check(self.lib.mrh_freespace_box_device(self._ctx, C.byref(p), d_state or None))

    def freespace_segments(self, a, b, step=0.0):
        """The segments a[i] -> b[i] ([n, 3] each, world frame) against the layer (mrh_freespace_segments): samples every `step`
        (0 = half a cell) from a.  Returns numpy copies (status u8 [n]: 0 = every sample lies in a free cell, FREE_SEG_UNKNOWN,
        FREE_SEG_BAD; counts u32 [n, 2] = (n_samples, n_free))."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        n = len(a)
        if len(b) != n:
            raise ValueError("freespace_segments: %d starts, %d ends" % (n, len(b)))
        ps, pc = C.c_void_p(), C.c_void_p()
        self._check(self.lib.mrh_freespace_segments(self._ctx, a.ctypes.data if n else None, b.ctypes.data if n else None, n, float(step), C.byref(ps), C.byref(pc)))
        return _copy_out(ps, n, np.uint8, (n,)), _copy_out(pc, 2 * n, np.uint32, (n, 2))

    def freespace_segments_device(self, d_a, d_b, n, d_status, d_counts=0, step=0.0):
        """mrh_freespace_segments_device: n segments from device lists into caller device buffers ([n] u8 required, [n, 2] u32 or 0;
        integer pointers).  Enqueues."""
        self._check(self.lib.mrh_freespace_segments_device(self._ctx, d_a or None, d_b or None, int(n), float(step), d_status or None, d_counts or None))

    def line_of_sight_free(self, a, b, step=0.0):
        """bool [n]: the segment a[i] -> b[i] crosses no surface (cast_rays: status & (RAY_HIT | RAY_INSIDE) == 0, with
        line_of_sight's ray) AND every sample of it lies in a carved cell (freespace_segments: status 0).  Where line_of_sight
        asks the map for observed free space, which it only knows near surfaces, this asks the free-space layer."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        if len(a) == 0:
            return np.zeros(0, bool)
        d = (b - a).astype(np.float32)
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
        finite = ln[np.isfinite(ln)]
        reach = float(finite.max()) if len(finite) else 0.0
        cast = self.cast_rays(a, d, max_range=reach, min_range=0.0, step=0.0, tmax=ln, normals=False, colors=False, counts=False, normalize=True)["status"]
        seg, _ = self.freespace_segments(a, b, step)
        return ((cast & (RAY_HIT | RAY_INSIDE)) == 0) & (seg == 0)  # a == b is a bad ray and a one-sample segment: the point's cell decides

    # -- map-to-map fusion (include/mrhash_remap.h) ----------------------------------------------------
    @staticmethod
    def _pose_args(R, t):
        F = C.POINTER(C.c_float)
        R = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        return R.ctypes.data_as(F), t.ctypes.data_as(F), (R, t)  # the last: keeps the arrays alive across the call

    def resample_map_device(self, R, t, voxel_size=0.0, min_weight=0):
        """mrh_resample_map: this map, whose frame lies at W = R P + t in the destination's world, resampled onto
        the lattice of `voxel_size` (0 = its own).  Returns (device pointer to mrh_block_record[n], n, info dict); the records
        are ordered by block position and belong to the context until its next resample_map / fuse_map as a source."""
        p = MrhRemapParams(float(voxel_size), int(min_weight))
        pR, pt, _keep = self._pose_args(R, t)
        ptr, n, info = C.c_void_p(), C.c_uint64(), MrhRemapInfo()
        self._check(self.lib.mrh_resample_map(self._ctx, C.byref(p), pR, pt, C.byref(ptr), C.byref(n), C.byref(info)))
        return int(ptr.value or 0), int(n.value), info.as_dict()

    def resample_map(self, R, t, voxel_size=0.0, min_weight=0):
        """resample_map_device copied to the host: (descs, voxels [n, 512], info) with the dtypes of dump_blocks."""
        ptr, n, info = self.resample_map_device(R, t, voxel_size, min_weight)
        from . import hipmem

        rec = np.frombuffer(hipmem.read(ptr, n * RECORD_BYTES), dtype=RECORD_DTYPE)
        return rec["desc"].copy(), rec["voxels"].copy(), info

    def fuse_map(self, src: "Engine", R, t, min_weight=0) -> dict:
        """mrh_fuse_map: `src`, whose frame lies at W = R P + t in this map's world, resampled at this map's voxel size and
        merged into it (MRH_UNPACK_MERGE).  Returns the info dict; `taken` = records this map took."""
        p = MrhRemapParams(0.0, int(min_weight))
        pR, pt, _keep = self._pose_args(R, t)
        info = MrhRemapInfo()
        self._check(self.lib.mrh_fuse_map(self._ctx, src._ctx, C.byref(p), pR, pt, C.byref(info)))
        return info.as_dict()

    # -- map-to-map registration (include/mrhash_align.h) ----------------------------------------------
    def align_map(self, src: "Engine", R, t, band=0.0, dist_max=0.0, iterations=0, min_samples=0, min_weight=0, pivot=None, extent=0.0):
        """mrh_align_map: estimates the pose W = R P + t of `src`'s frame in this map's world from the start (R, t),
        by SDF-to-SDF registration of the two maps; what fuse_map then takes.  Blocks.  0 = the default of a parameter; `pivot`
        and `extent` crop the source's samples to a cube and set the lever (extent 0: both automatic).  Returns (R float32 [3, 3],
        t float32 [3], info) with info = {status (ALIGN_OK / ALIGN_LOST), iterations_done, source_blocks, samples, accepted, rms,
        pivot, extent, sums int64 [32]}; a lost alignment returns the pose from before the step that failed."""
        c = np.zeros(3, np.float32) if pivot is None else np.ascontiguousarray(pivot, dtype=np.float32).reshape(3)
        p = MrhAlignParams(band, dist_max, int(iterations), int(min_samples), int(min_weight), (C.c_float * 3)(*[float(x) for x in c]), extent)
        pR, pt, _keep = self._pose_args(R, t)
        out_R, out_t, info = np.zeros(9, np.float32), np.zeros(3, np.float32), MrhAlignInfo()
        F = C.POINTER(C.c_float)
        self._check(self.lib.mrh_align_map(self._ctx, src._ctx, C.byref(p), pR, pt, out_R.ctypes.data_as(F), out_t.ctypes.data_as(F), C.byref(info)))
        return out_R.reshape(3, 3), out_t, info.as_dict()

    # -- tracking (include/mrhash_track.h) ------------------------------------------------------------
    def _track(self, fn, obs, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step, dist_max, iterations, min_pixels):
        """obs: the arguments between the parameter block and the pose — (depth pointer,) or (points pointer, n)."""
        p = MrhTrackParams(fx, fy, cx, cy, int(rows), int(cols), min_depth, max_depth, step, dist_max, int(iterations), int(min_pixels))
        R = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        out_R, out_t, info = np.zeros(9, np.float32), np.zeros(3, np.float32), MrhTrackInfo()
        F = C.POINTER(C.c_float)
        self._check(fn(self._ctx, C.byref(p), *obs, R.ctypes.data_as(F), t.ctypes.data_as(F), out_R.ctypes.data_as(F),
                       out_t.ctypes.data_as(F), C.byref(info)))
        return out_R.reshape(3, 3), out_t, info.as_dict()

    def track_depth(self, depth, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, dist_max=0.0, iterations=0, min_pixels=0):
        """Estimates the camera-to-world pose of the depth image (float32 [rows, cols], metres) by point-to-plane ICP against
        one render of the map from the initial pose (R, t) (mrh_track_depth).  Blocks.  0 = the default of
        step, dist_max, iterations (10) and min_pixels (64).  Returns (R float32 [3, 3], t float32 [3], info) with info =
        {status (TRACK_OK / TRACK_LOST), iterations_done, pixels, rms, sums int64 [32]}; a lost track returns the pose from
        before the step that failed."""
        d = np.ascontiguousarray(depth, dtype=np.float32)
        if d.size != int(rows) * int(cols):
            raise ValueError(f"track_depth: depth has {d.size} pixels, rows * cols = {int(rows) * int(cols)}")
        return self._track(self.lib.mrh_track_depth, (d.ctypes.data,), fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step, dist_max,
                           iterations, min_pixels)

    def track_depth_device(self, ptr_depth: int, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, dist_max=0.0, iterations=0,
                           min_pixels=0):
        """mrh_track_depth_device: as track_depth with the image already on the device (integer pointer, e.g.
        hipmem.DeviceBuffer.ptr, [rows * cols] float32).  Blocks too: the solve is on the host."""
        return self._track(self.lib.mrh_track_depth_device, (ptr_depth or None,), fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step,
                           dist_max, iterations, min_pixels)

    def track_scan(self, points, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, dist_max=0.0, iterations=0, min_points=0):
        """Estimates the sensor-to-world pose of a scan (float32 [n, 3], sensor frame, organised or not; (0, 0, 0) = no return) by
        point-to-plane ICP against one spherical render of the map from the initial pose (R, t) (mrh_track_scan).
        fx .. cols are the spherical intrinsics of that render as raycast_spherical takes them, min_depth / max_depth ranges.
        Blocks.  Returns what track_depth returns; info["pixels"] counts points."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        return self._track(self.lib.mrh_track_scan, (pts.ctypes.data, len(pts)), fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step,
                           dist_max, iterations, min_points)

    def track_scan_device(self, ptr_points: int, n: int, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step=0.0, dist_max=0.0,
                          iterations=0, min_points=0):
        """mrh_track_scan_device: as track_scan with the cloud already on the device (integer pointer, [n, 3] float32), e.g. the
        points image of raycast_spherical_device after sync().  Blocks too."""
        return self._track(self.lib.mrh_track_scan_device, (ptr_points or None, int(n)), fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth,
                           step, dist_max, iterations, min_points)

    # -- render-free tracking (include/mrhash_sdftrack.h) ----------------------------------------------
    def _track_sdf(self, fn, obs, K, R, t, min_depth, max_depth, band, iterations, min_pixels):
        """obs: the arguments between the parameter block and the pose — (depth pointer,) or (points pointer, n); K = (fx, fy, cx, cy,
        rows, cols), zeros for the points form."""
        fx, fy, cx, cy, rows, cols = K
        p = MrhSdftrackParams(fx, fy, cx, cy, int(rows), int(cols), min_depth, max_depth, band, int(iterations), int(min_pixels), 0)
        R = np.ascontiguousarray(R, dtype=np.float32).reshape(9)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        out_R, out_t, info = np.zeros(9, np.float32), np.zeros(3, np.float32), MrhTrackInfo()
        F = C.POINTER(C.c_float)
        self._check(fn(self._ctx, C.byref(p), *obs, R.ctypes.data_as(F), t.ctypes.data_as(F), out_R.ctypes.data_as(F),
                       out_t.ctypes.data_as(F), C.byref(info)))
        return out_R.reshape(3, 3), out_t, info.as_dict()

    def track_depth_sdf(self, depth, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, band=0.0, iterations=0, min_pixels=0):
        """Estimates the camera-to-world pose of the depth image (float32 [rows, cols], metres) by registering its back-projected
        pixels against the map's distance field, without a render (mrh_track_depth_sdf), from the start (R, t).
        Blocks.  0 = the default of band (the truncation), iterations (10) and min_pixels (64).  A pixel further than `band`
        from the surface gives no row.  Returns what track_depth returns."""
        d = np.ascontiguousarray(depth, dtype=np.float32)
        if d.size != int(rows) * int(cols):
            raise ValueError(f"track_depth_sdf: depth has {d.size} pixels, rows * cols = {int(rows) * int(cols)}")
        return self._track_sdf(self.lib.mrh_track_depth_sdf, (d.ctypes.data,), (fx, fy, cx, cy, rows, cols), R, t, min_depth, max_depth, band, iterations,
                               min_pixels)

    def track_depth_sdf_device(self, ptr_depth: int, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, band=0.0, iterations=0, min_pixels=0):
        """mrh_track_depth_sdf_device: as track_depth_sdf with the image already on the device (integer pointer, [rows * cols]
        float32).  Blocks too: the solve is on the host."""
        return self._track_sdf(self.lib.mrh_track_depth_sdf_device, (ptr_depth or None,), (fx, fy, cx, cy, rows, cols), R, t, min_depth, max_depth, band,
                               iterations, min_pixels)

    def track_points_sdf(self, points, R, t, min_depth, max_depth, band=0.0, iterations=0, min_points=0):
        """Estimates the sensor-to-world pose of a cloud (float32 [n, 3], sensor frame, any order, any sensor; (0, 0, 0) = no return)
        against the map's distance field (mrh_track_points_sdf): no camera model, no field of view, no seam.
        min_depth / max_depth are ranges.  Blocks.  Returns what track_depth returns; info["pixels"] counts points."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        return self._track_sdf(self.lib.mrh_track_points_sdf, (pts.ctypes.data, len(pts)), (0.0, 0.0, 0.0, 0.0, 0, 0), R, t, min_depth, max_depth, band,
                               iterations, min_points)

    def track_points_sdf_device(self, ptr_points: int, n: int, R, t, min_depth, max_depth, band=0.0, iterations=0, min_points=0):
        """mrh_track_points_sdf_device: as track_points_sdf with the cloud already on the device (integer pointer, [n, 3] float32,
        read as it lies).  Blocks too."""
        return self._track_sdf(self.lib.mrh_track_points_sdf_device, (ptr_points or None, int(n)), (0.0, 0.0, 0.0, 0.0, 0, 0), R, t, min_depth, max_depth,
                               band, iterations, min_points)

    # -- scan normals (include/mrhash_normals.h) ----------------------------------------------------
    def estimate_normals(self, radius=0.0, min_points=0, min_spread=0.0, max_flatness=0.0, info=False):
        """Estimates one normal per point of the current scan (upload_points / set_points_device) on the device, into the
        context's normal buffer: what upload_normals would otherwise be given (mrh_estimate_normals).  0 = the
        default of a parameter.  info=True blocks and returns the counts {points, estimated, fallback, missing, cells}."""
        p = MrhNormalsParams(radius, int(min_points), min_spread, max_flatness)
        out = MrhNormalsInfo()
        self._check(self.lib.mrh_estimate_normals(self._ctx, C.byref(p), C.byref(out) if info else None))
        return out.as_dict() if info else None

    def estimate_normals_device(self, ptr_xyz: int, n: int, ptr_out: int, radius=0.0, min_points=0, min_spread=0.0, max_flatness=0.0):
        """mrh_estimate_normals_device: normals of the n points at device pointer ptr_xyz into device pointer ptr_out ([n, 3]
        float32 each).  Ordered on the context's stream; finished by sync() or any blocking call."""
        p = MrhNormalsParams(radius, int(min_points), min_spread, max_flatness)
        self._check(self.lib.mrh_estimate_normals_device(self._ctx, C.byref(p), ptr_xyz or None, int(n), ptr_out or None))

    def get_normals(self):
        """(normals float32 [N, 3] as a numpy copy, counts of the estimate that made them): the context's normal buffer."""
        ptr, n, info = C.c_void_p(), C.c_uint64(), MrhNormalsInfo()
        self._check(self.lib.mrh_get_normals(self._ctx, C.byref(ptr), C.byref(n), C.byref(info)))
        k = int(n.value)
        return _copy_out(ptr, 3 * k, np.float32, (k, 3)), info.as_dict()

    def get_voxel(self, vx: int, vy: int, vz: int):
        out = np.zeros(1, dtype=VOXEL_DTYPE)
        found = C.c_int()
        self._check(self.lib.mrh_get_voxel(self._ctx, vx, vy, vz, out.ctypes.data, C.byref(found)))
        return out[0], bool(found.value)
