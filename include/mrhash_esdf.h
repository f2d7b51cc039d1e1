/*
 * mrhash_esdf.h — distance fields for planners: the exact Euclidean signed distance field (ESDF) of a box of the fused map
 * (libmrhash_hip.so, kernels in mrhash_amd/csrc/mrh_esdf.h).
 *
 * The TSDF answers "how far is the nearest surface" only inside its truncation band.  mrh_esdf answers it for every
 * finest-resolution voxel of a box, up to a reach R, in four launches and one copy.  The reference has no distance field; the
 * definition is this project's.  DESIGN.md D16 is the normative statement, tests/esdf_ref.py restates it in numpy.
 *
 * Box: the cells v = origin + (i, j, k), 0 <= i < dims[0], 0 <= j < dims[1], 0 <= k < dims[2], in the voxel coordinates of
 * mrh_get_voxel (voxel v sits at world v * vs, vs the finest voxel size).  Per cell:
 *   s        the voxel mrh_get_voxel(v) reports; on a variance-adaptive map a cell inside a coarse block reads the coarse voxel
 *            that covers it (res = 1).  Blocks that are absent, paged out or out of key range: found = 0
 *   observed found && weight >= w_min, w_min = min_weight, or the context's min_weight_threshold when min_weight == 0; at least 1
 *   site     observed && |sdf| <= band, band = surface_band when that is > 0, else vs * 2^res.  A NaN sdf is no site
 *   inside   observed && sdf < 0
 *   d2       min over the site cells s OF THIS BOX of |v - s|^2 (an integer);  far: no site, or d2 > R^2
 *   dist     a site: its own sdf (the field is continuous through the surface);  not far: sgn * (vs * sqrtf((float) d2));
 *            far: sgn * (vs * (float) R);  sgn = inside ? -1 : +1.  binary32, no contraction, correctly rounded square root
 *   state    bit 0 observed, bit 1 site, bit 2 inside, bit 3 far
 *   d2 out   0 for a site, the exact integer for a cell that is not far, 0xFFFFFFFF for a far cell
 * All outputs have x fastest: index (k * dims[1] + j) * dims[0] + i.
 *
 * SITES OUTSIDE THE BOX ARE NOT SEEN.  A cell's distance is exact with respect to the map only where the nearest surface
 * lies inside the box: pad the box by R on every side of the region whose distances are needed.
 *
 * Limits: 1 <= dims <= MRH_ESDF_MAX_SIDE per axis, 1 <= max_distance_voxels <= MRH_ESDF_MAX_REACH, origin and
 * origin + dims - 1 within [-2^23, 2^23) per axis, surface_band finite and >= 0, min_weight >= 0, no unknown output bit.
 *
 * Conventions as in mrhash_hip.h.  Both calls enter like every other reader of the map (see mrhash_raycast.h): a host-fed frame
 * that mrh_integrate kept back runs first, pipelined frames in flight are integrated ahead of the call.  Nothing of the frame
 * path changes: camera, pose, images, counters, mrh_stats, the last extraction and the raycast and tracking buffers stay as
 * they were.  The scratch and result buffers grow on demand and are released by mrh_destroy.
 *
 * Errors: MRH_ERR_INVALID_ARG for a null context / parameter block or a parameter outside the limits, before the map is
 * touched; MRH_ERR_STATE while an exchange is pending; MRH_ERR_UNSUPPORTED on a sharded context (shard_count > 1).
 */
#ifndef MRHASH_ESDF_H
#define MRHASH_ESDF_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_ESDF_STATE   1u   /* produce the state bytes           */
#define MRH_ESDF_SQUARED 2u   /* produce the squared distances d2  */
#define MRH_ESDF_MAX_SIDE  512
#define MRH_ESDF_MAX_REACH 4095

#define MRH_ESDF_OBSERVED 1u  /* bits of a state byte */
#define MRH_ESDF_SITE     2u
#define MRH_ESDF_INSIDE   4u
#define MRH_ESDF_FAR      8u

typedef struct mrh_esdf_params {
  int32_t  origin[3];             /* first cell of the box, finest voxels                               */
  int32_t  dims[3];               /* cells per axis, 1 .. 512                                           */
  int32_t  max_distance_voxels;   /* the reach R, 1 .. 4095                                             */
  int32_t  min_weight;            /* 0 = the context's min_weight_threshold                             */
  float    surface_band;          /* metres; 0 = one voxel of the block's own resolution                */
  uint32_t outputs;               /* MRH_ESDF_* bits; dist is always produced                           */
} mrh_esdf_params;                /* 40 bytes */

/* Computes the field of the box.  Blocks.  The results are host buffers owned by ctx until the next mrh_esdf or mrh_destroy:
 * dist [n] f32, state [n] u8, d2 [n] u32 with n = dims[0] * dims[1] * dims[2].  A NULL out-pointer = not wanted; state / d2
 * are only produced when their MRH_ESDF_* bit is set as well (else the out-pointer is set to NULL).  The field is computed
 * whichever outputs are asked for: a NULL out_dist only saves its copy to the host. */
int mrh_esdf(mrh_ctx* ctx, const mrh_esdf_params* p, const float** out_dist, const uint8_t** out_state, const uint32_t** out_d2);

/* The same into caller device buffers ([n] f32, [n] u8, [n] u32; d_dist is required, d_state / d_d2 may be NULL = skip and
 * also need their MRH_ESDF_* bit).  Enqueues on the context's stream: ordered after every earlier call, finished by mrh_sync
 * or any blocking call; the buffers must stay valid until then. */
int mrh_esdf_device(mrh_ctx* ctx, const mrh_esdf_params* p, float* d_dist, uint8_t* d_state, uint32_t* d_d2);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_ESDF_H */
