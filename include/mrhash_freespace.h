/*
 * mrhash_freespace.h — the free-space layer: observed free space carved from depth frames and scans, the state of a box of
 * cells with its frontier, and free-space segments (libmrhash_hip.so, kernels in mrhash_amd/csrc/mrh_freespace.h).
 *
 * The map stores blocks near surfaces only: space further than the truncation from every surface has no block, however often a
 * sensor looked through it, and every reader of the map (mrhash_esdf.h, mrhash_query.h, mrhash_rays.h) reports it as unknown.
 * The layer is a separate, opt-in structure on the context that knows exactly this: a dense bit grid over a box of cells, one bit
 * per cell, set when a sensor ray passed through the cell before it ended.  Frames and scans carve it, the readers below consult
 * it.  Integration, the table and every other reader stay as they are: nothing changes for a caller who never creates a layer.
 * The reference has no such structure; the definition is this project's.  DESIGN.md D22 is the normative statement,
 * tests/freespace_ref.py restates it in numpy.
 *
 * CELLS.  A cell is 2^s finest voxels per side, s = cell_shift in {0, 1, 2, 3}: cell c covers the voxels c * 2^s ..
 * c * 2^s + 2^s - 1 per axis, in the voxel coordinates of mrh_get_voxel, so a cell never straddles an 8^3 brick of voxel space.
 * The cell of a world point P is world_to_voxel(vs, P) >> s per axis (arithmetic shift), world_to_voxel being the conversion of
 * the render, the point queries and the ray queries.
 *
 * All arithmetic is binary32 without contraction.
 *
 * CARVING.  A ray is sampled at z_k = min_depth + k * step (each computed afresh), k = 0, 1, ... while z_k <= end; step 0 = half
 * a cell, 0.5f * (vs * (float) (1 << s)), computed once on the host; at most MRH_FREESPACE_MAX_SAMPLES samples z_k <= max_depth,
 * counted on the host as for the render.
 *   depth, pixel (r, c) with value D
 *              NaN or D <= min_depth: nothing.  D > max_depth (+inf too): end = max_depth (the ray saw nothing up to the limit).
 *              Else end = D - margin.  The ray is the render's (mrhash_raycast.h, D11): d_c = (ifx * ((c - cx) - 0.5),
 *              ify * ((r - cy) - 0.5), 1) with ifx = 1 / fx, ify = 1 / fy, d_w,a = (R[3a] d_c,x + R[3a+1] d_c,y) + R[3a+2] d_c,z,
 *              P(z)_a = t[a] + z * d_w,a
 *   points, sensor-frame point p = (x, y, z)
 *              rho = sqrtf((x * x + y * y) + z * z).  rho not finite or rho <= min_depth: nothing (the missing return (0, 0, 0)).
 *              end = fminf(rho, max_depth) - margin, d_s = (x / rho, y / rho, z / rho), d_w = R d_s in the same row shape, the
 *              same samples and P.  The points form ignores fx .. cols
 *   sample     unless fabsf(P_a) < bound on every axis, bound = (float) (1 << 20) * vs as for the point and ray queries (a NaN
 *              fails; the test runs before any float -> int conversion), the sample sets nothing.  Otherwise the bit of the
 *              cell of P is set when the cell lies in the layer's box
 * Bits are only ever set, with a bitwise OR: the layer after a call is a pure function of the set of (ray, sample) pairs, whatever
 * the launch shape, the order of the rays or the order of two carves.  A carve does not read the map.
 *
 * THE STATE OF A CELL (mrh_freespace_box), one byte:
 *   MRH_FREE_FREE      the layer's bit; 0 outside the layer's box
 *   MRH_FREE_OBSERVED  some voxel of the cell is observed by the distance field's rule (mrhash_esdf.h, D16: found by
 *                      mrh_get_voxel with weight >= w_min, w_min = max(1, min_weight ? min_weight : min_weight_threshold)); a
 *                      coarse voxel answers for the cells it covers
 *   MRH_FREE_OCCUPIED  some voxel of the cell is a D16 site: observed with fabsf(sdf) <= band, band = surface_band or, when that
 *                      is 0, one voxel of the block's own resolution
 *   MRH_FREE_FRONTIER  FREE and not OCCUPIED, and at least one of the six face neighbours INSIDE THE REQUESTED BOX has neither
 *                      FREE nor OBSERVED.  Neighbours outside the requested box are not looked at: pad the box by one cell
 *
 * SEGMENTS.  Per segment a -> b: L = sqrtf((dx * dx + dy * dy) + dz * dz) of b - a, d = (b - a) / L per component, or the zero
 * vector when L == 0; samples z_k = k * step while z_k <= L (step 0 = half a cell), P(z)_a = a_a + z * d_a.  counts = (n_samples,
 * n_free), n_free the samples whose cell lies in the layer with its bit set; status 0 when every sample is free, else
 * MRH_FREE_SEG_UNKNOWN; MRH_FREE_SEG_BAD with counts (0, 0) for an endpoint that is not finite, more than
 * MRH_FREESPACE_MAX_SAMPLES samples, or a sample outside the bound.  A point is the segment a == b: one sample.  Segments read
 * the layer alone.
 *
 * Conventions as in mrhash_hip.h.  ORDER.  A carve neither reads nor changes the map, and its buffers are its own and the readers'
 * staging pair, which the frame path never touches: it does NOT flush a frame that mrh_integrate kept back, and pipelined frames
 * stay in flight.  It is meant to be called once per frame next to mrh_integrate.  mrh_freespace_box reads the map and enters like
 * every other reader (see mrhash_raycast.h); mrh_freespace_segments reads the layer alone and enters like a carve.  Everything
 * runs on the context's stream: a reader sees every carve issued before it.  mrh_reset clears the bits of an existing layer and
 * keeps its box; mrh_destroy releases the layer.
 *
 * Errors, in this order: MRH_ERR_INVALID_ARG for a null context / parameter block / required pointer; MRH_ERR_STATE while an
 * exchange is pending; MRH_ERR_UNSUPPORTED on a sharded context (shard_count > 1); MRH_ERR_STATE when the context has no layer
 * (every call but mrh_freespace_create); then MRH_ERR_INVALID_ARG for the limits of the call in the order its parameter block
 * lists them.
 */
#ifndef MRHASH_FREESPACE_H
#define MRHASH_FREESPACE_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_FREESPACE_MAX_SIDE     1024          /* cells per side of a layer                          */
#define MRH_FREESPACE_MAX_CELLS    (1u << 28)    /* cells of a layer: 32 MiB of bits                   */
#define MRH_FREESPACE_MAX_SHIFT    3
#define MRH_FREESPACE_BOX_MAX_SIDE 512           /* cells per side of a box of mrh_freespace_box       */
#define MRH_FREESPACE_MAX_SAMPLES  (1u << 20)    /* samples of one ray or one segment                  */
#define MRH_FREESPACE_MAX_POINTS   (1u << 24)    /* points of one carve, segments of one call          */

#define MRH_FREE_FREE     0x01u    /* bits of a cell's state byte */
#define MRH_FREE_OBSERVED 0x02u
#define MRH_FREE_OCCUPIED 0x04u
#define MRH_FREE_FRONTIER 0x08u

#define MRH_FREE_SEG_UNKNOWN 0x01u /* a segment's status: some sample is not known to be free          */
#define MRH_FREE_SEG_BAD     0x80u /* an endpoint is not finite, too many samples, outside the bound   */

typedef struct mrh_freespace_params {
  int32_t  origin[3];              /* first cell of the box, in cells                                   */
  int32_t  dims[3];                /* 1 .. MRH_FREESPACE_MAX_SIDE each, product <= MRH_FREESPACE_MAX_CELLS */
  int32_t  cell_shift;             /* s: a cell is 2^s finest voxels per side, 0 .. 3                   */
  uint32_t reserved;               /* must be 0                                                         */
} mrh_freespace_params;            /* 32 bytes */

typedef struct mrh_carve_params {
  float    fx, fy, cx, cy;         /* depth form: the pinhole camera; ignored by the points form        */
  int32_t  rows, cols;             /* depth form: the image; ignored by the points form                 */
  float    min_depth, max_depth;   /* 0 <= min_depth < max_depth                                        */
  float    step;                   /* sample spacing; 0 = half a cell                                   */
  float    margin;                 /* >= 0: a ray stops this far in front of its measurement            */
  uint32_t reserved[2];            /* must be 0                                                         */
} mrh_carve_params;                /* 48 bytes */

typedef struct mrh_freespace_box_params {
  int32_t  origin[3];              /* first cell of the box, in cells                                   */
  int32_t  dims[3];                /* 1 .. MRH_FREESPACE_BOX_MAX_SIDE each; may extend beyond the layer */
  int32_t  min_weight;             /* 0 = the context's min_weight_threshold                            */
  float    surface_band;           /* 0 = one voxel of the block's own resolution                       */
  uint32_t reserved[2];            /* must be 0                                                         */
} mrh_freespace_box_params;        /* 40 bytes */

/* Allocates and zeroes a layer over the box origin + [0, dims) of cells; replaces an existing layer.  origin * 2^s and
 * (origin + dims) * 2^s - 1 must lie within [-2^23, 2^23) per axis.  The zeroing is enqueued behind whatever still uses the old
 * layer; a layer larger than every earlier one waits for the stream before it allocates. */
int mrh_freespace_create(mrh_ctx* ctx, const mrh_freespace_params* p);
/* Every bit 0, the box stays (enqueues). */
int mrh_freespace_clear(mrh_ctx* ctx);
/* The context has no layer afterwards (blocks); mrh_destroy does the same. */
int mrh_freespace_destroy(mrh_ctx* ctx);

/* Carves a depth image of p->rows x p->cols f32 seen from the pose (R row-major, t: camera in world).  Blocks. */
int mrh_freespace_carve_depth(mrh_ctx* ctx, const mrh_carve_params* p, const float* depth_host, const float R_row_major[9], const float t[3]);
/* The same from a device image.  Enqueues on the context's stream: ordered after every earlier call, finished by mrh_sync or any
 * blocking call; the image must stay valid until then. */
int mrh_freespace_carve_depth_device(mrh_ctx* ctx, const mrh_carve_params* p, const float* d_depth, const float R_row_major[9], const float t[3]);
/* Carves n sensor-frame points [n * 3] f32 seen from the pose; n <= MRH_FREESPACE_MAX_POINTS, n == 0 succeeds with nothing
 * launched (the list may be NULL).  Blocks. */
int mrh_freespace_carve_points(mrh_ctx* ctx, const mrh_carve_params* p, const float* points_host, uint64_t n, const float R_row_major[9], const float t[3]);
/* The same from a device list (enqueues). */
int mrh_freespace_carve_points_device(mrh_ctx* ctx, const mrh_carve_params* p, const float* d_points, uint64_t n, const float R_row_major[9], const float t[3]);

/* The state byte of every cell of the box, x fastest: [dims[2]][dims[1]][dims[0]] u8.  Blocks; the result is a host buffer owned
 * by ctx until the next mrh_freespace_box or mrh_destroy. */
int mrh_freespace_box(mrh_ctx* ctx, const mrh_freespace_box_params* p, const uint8_t** out_state);
/* The same into a caller device buffer of dims[0] * dims[1] * dims[2] bytes (enqueues). */
int mrh_freespace_box_device(mrh_ctx* ctx, const mrh_freespace_box_params* p, uint8_t* d_state);

/* n segments a -> b, a_host and b_host [n * 3] f32 world frame, n <= MRH_FREESPACE_MAX_POINTS.  Blocks; status [n] u8 and counts
 * [n * 2] u32 = (n_samples, n_free) are host buffers owned by ctx until the next mrh_freespace_segments or mrh_destroy (a NULL
 * out-pointer = not wanted).  n == 0 succeeds with nothing launched (the out-pointers are set to NULL). */
int mrh_freespace_segments(mrh_ctx* ctx, const float* a_host, const float* b_host, uint64_t n, float step, const uint8_t** out_status,
                           const uint32_t** out_counts);
/* The same from and into device buffers; d_status is required, d_counts may be NULL (enqueues). */
int mrh_freespace_segments_device(mrh_ctx* ctx, const float* d_a, const float* d_b, uint64_t n, float step, uint8_t* d_status, uint32_t* d_counts);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_FREESPACE_H */
