/*
 * mrhash_remap.h — map-to-map fusion: a map resampled under a rigid pose onto another lattice, as block records, and merged
 * into a second map (libmrhash_hip.so, kernels in mrhash_amd/csrc/mrh_remap.h).
 *
 * A second session, a second robot, a sub-map closed by a loop closure or a frame-sharded rank whose poses were corrected
 * afterwards each leave a second map whose frame differs from the first by a rigid transform — the one mrh_align_map
 * (mrhash_align.h) estimates from the two maps; mrh_track_depth / mrh_track_scan estimate the pose of one frame, not of a map.
 * mrh_unpack_blocks(MRH_UNPACK_MERGE) folds sub-maps only when their lattices coincide;
 * mrh_resample_map evaluates the source map on the destination's lattice and hands the result over as mrh_block_record, in the
 * order mrh_pack_blocks produces, so that the existing merge takes it.  mrh_fuse_map is the two in one call.  The reference has
 * no such call; the definition is this project's.  DESIGN.md D18 is the normative statement, tests/remap_ref.py restates it in
 * numpy.
 *
 * (R, t) is the pose of the source map's frame in the destination's world: W = R P + t.  R must be a rotation (or a reflection):
 * |R R^T - I| <= 2^-10 in every entry.  All arithmetic is binary32 without contraction.  vs_s: the source's finest voxel size,
 * vs_d: the destination's.  Per destination voxel v = 8 b + (lx, ly, lz) of block b, stored at voxels[lz * 64 + ly * 8 + lx]:
 *   W        its world position, (float) v_a * vs_d per axis (voxel_to_world)
 *   P        its position in the source frame, P_a = ((R[a] (W_x - t_x) + R[3 + a] (W_y - t_y)) + R[6 + a] (W_z - t_z)): the
 *            transpose of R applied directly
 *   range    the voxel is invalid unless fabsf(P_a) < (float) (1 << 20) * vs_s on all three axes (the bound of mrhash_query.h,
 *            evaluated before any float -> int conversion)
 *   sdf      the SMOOTH field of mrhash_query.h at P on the source map, h = getVoxelSize(P), the corners read through getVoxel
 *            (coarse blocks answer); valid only when all eight corners are found with weight > 0
 *   nearest  getVoxel(P); valid only when it is found with weight >= max(1, min_weight).  rgb, weight and sum_squared are
 *            nearest's, unchanged
 * An invalid voxel is all zero bits.  A record — always resolution 0 — is produced for exactly the destination blocks inside the
 * packed-key range (+-2^20 blocks) that have at least one valid voxel, ordered by block position (x, then y, then z).
 *
 * Conventions as in mrhash_hip.h.  mrh_resample_map enters like every other reader of the map (see mrhash_raycast.h): a host-fed
 * frame that mrh_integrate kept back runs first, pipelined frames in flight are integrated ahead of the call.  It only reads the
 * source: camera, pose, images, counters, mrh_stats, the last extraction and the results of the other readers stay as they were.
 * Blocks of the source that a wrapper's host chunk grid has paged out (GeoWrapper's streamer) are not in the device map and take
 * no part; mrh_fuse_map merges into the destination's device map only.
 *
 * Errors, all raised before either map is touched: MRH_ERR_INVALID_ARG for a null context / parameter block / R / t / required
 * out-pointer, a reserved word that is not 0, min_weight > 255, a pose that is not finite or not a rotation, a ratio
 * dst_voxel_size / source voxel size outside [1/4, 4], dst == src, contexts on different devices, a dst_voxel_size that
 * contradicts dst; MRH_ERR_STATE while an exchange is pending on either context; MRH_ERR_UNSUPPORTED when either context is
 * sharded (shard_count > 1).  MRH_ERR_CAPACITY when the candidate list or the records of one call would pass 2^31 - 1 entries.
 */
#ifndef MRHASH_REMAP_H
#define MRHASH_REMAP_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mrh_remap_params {
  float    dst_voxel_size;   /* finest voxel size of the destination lattice; 0 = the source's            */
  uint32_t min_weight;       /* a resampled voxel needs nearest.weight >= max(1, min_weight); <= 255      */
  uint32_t reserved[2];      /* must be 0                                                                 */
} mrh_remap_params;          /* 16 bytes */

typedef struct mrh_remap_info {
  uint64_t source_blocks;    /* live blocks of the source                                                 */
  uint64_t candidate_blocks; /* distinct destination blocks the candidates pass named                     */
  uint64_t records;          /* of them, blocks with at least one valid voxel = records produced          */
  uint64_t valid_voxels;     /* valid voxels in all records                                               */
  uint64_t taken;            /* mrh_fuse_map only: records the destination took (mrh_unpack_blocks)       */
} mrh_remap_info;

/* Resamples src under (R, t) onto the lattice of p->dst_voxel_size.  Blocks.  *out_records is DEVICE memory owned by src, valid
 * until the next mrh_resample_map / mrh_fuse_map on src or mrh_destroy; an empty result (an empty source included, for which
 * nothing is launched) gives *out_n = 0 and *out_records = NULL.  out_info may be NULL. */
int mrh_resample_map(mrh_ctx* src, const mrh_remap_params* p, const float R_row_major[9], const float t[3],
                     const mrh_block_record** out_records, uint64_t* out_n, mrh_remap_info* out_info);

/* Resamples src at dst's voxel size (p->dst_voxel_size must be 0 or equal to it) and runs the records through dst's
 * MRH_UNPACK_MERGE path: exactly what mrh_resample_map followed by mrh_unpack_blocks(dst, MRH_UNPACK_MERGE, records, n, 1, ..)
 * gives, dst's own rules on a variance-adaptive map included (a fine record onto a coarse block is not taken).  src's stream is
 * synchronised before dst's stream reads the records.  Blocks.  out_info may be NULL. */
int mrh_fuse_map(mrh_ctx* dst, mrh_ctx* src, const mrh_remap_params* p, const float R_row_major[9], const float t[3],
                 mrh_remap_info* out_info);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_REMAP_H */
