/*
 * mrhash_query.h — point queries: the TSDF distance, its gradient and the colour of the fused map at a list of arbitrary
 * positions (libmrhash_hip.so, kernels in mrhash_amd/csrc/mrh_query.h).
 *
 * The map can be meshed, rendered, tracked against and turned into a distance field over a box; a trajectory optimiser, a
 * scan-to-map residual, the colouring of a LiDAR cloud or the scoring of a map against a ground-truth cloud have a LIST of
 * positions instead.  The reference has no such call; the definition is this project's.  DESIGN.md D17 is the normative
 * statement, tests/query_ref.py restates it in numpy.
 *
 * TWO FIELDS.  The reference's trilinearInterpolation (vds.cu:260-338) — the field the mesh and the render are built on —
 * places its eight samples at pos - h/2 + {0, 1} h and takes its weights relative to pos - h/2, so every weight is exactly 1/2:
 * its value is the mean of eight cells and PIECEWISE CONSTANT inside each dual cell (two points 0.15 voxel apart return the
 * same bits).  MRH_QUERY_FIELD_MAP returns that field, bit for bit what marching cubes and the raycast see.  A planner or a
 * registration needs a continuous field: MRH_QUERY_FIELD_SMOOTH interpolates the eight voxels around the point with their
 * true weights and has an analytic gradient.  It reproduces a linear field and its gradient exactly.
 *
 * All arithmetic is binary32 without contraction.  Per point (x, y, z):
 *   P        the world position.  Without a pose: (x, y, z).  With a pose (sensor frame, R row-major and t sensor-to-world):
 *            P_a = ((R[3a] x + R[3a+1] y) + R[3a+2] z) + t[a]; an input that is exactly (+-0, +-0, +-0) is a missing return,
 *            the scan convention, and is refused
 *   refused  unless fabsf(P_a) < bound on all three axes, bound = (float) (1 << 20) * vs (vs: the finest voxel size), computed
 *            once on the host; NaN and +-Inf fail the comparison, which runs before any float -> int conversion.  A refused
 *            point has state = MRH_QUERY_REFUSED and +0 in every other output.  The bound leaves room for every sample a query
 *            takes: the farthest lies within 5 vs of P (P +- 2 vs of the gradient on a coarse block, + 2 vs of its stencil, +
 *            the coarser re-sample), so voxel coordinates stay below 2^20 + 8 (int32 holds 2^31) and block coordinates below
 *            2^17 + 2 (a packed key holds [-2^20, 2^20))
 *   h        the local voxel size (getVoxelSize, vds.cu:236-240): vs, or 2 vs inside a coarse block of a variance-adaptive map
 *   nearest  the voxel that covers P (getVoxel, vds.cu:163-205).  Blocks that are absent or paged out: not found
 *   state    MRH_QUERY_BLOCK when nearest was found, MRH_QUERY_COARSE when h > vs, MRH_QUERY_DIST / _GRAD as below
 *   rgbw     r, g, b, weight of nearest; 0, 0, 0, 0 when it was not found
 *   MAP      dist = trilinearInterpolation(P), MRH_QUERY_DIST when it succeeds (all eight samples have weight > 0).  Gradient,
 *            evaluated only with DIST and when wanted: g_a = (D(P + h e_a) - D(P - h e_a)) / (h + h), the offset points being
 *            P_a +- h as in the raycast's normal; MRH_QUERY_GRAD when all six evaluations succeed, else the gradient is +0
 *   SMOOTH   per axis u = P_a / h, f = floorf(u), w = u - f; the corners ((f_x + i) h, (f_y + j) h, (f_z + k) h) are read with
 *            getVoxel, so the voxel that covers the position answers, coarse or fine.  MRH_QUERY_DIST when all eight are found
 *            with weight > 0.  lerp(a, b, t) = a + t (b - a).  dist: lerp along x for the four (j, k), then along y, then
 *            along z.  g_x = lerp_z(lerp_y(s_1jk - s_0jk)) / h; g_y: lerp along x, difference along y, lerp along z, / h;
 *            g_z: lerp along x, lerp along y, difference along z, / h.  MRH_QUERY_GRAD = MRH_QUERY_DIST when wanted
 * Outputs that are not produced, or are invalid, are +0.
 *
 * Conventions as in mrhash_hip.h.  Both calls enter like every other reader of the map (see mrhash_raycast.h): a host-fed frame
 * that mrh_integrate kept back runs first, pipelined frames in flight are integrated ahead of the call.  The calls only read the
 * map.  Nothing of the frame path changes: camera, pose, images, counters, mrh_stats, the last extraction and the raycast,
 * tracking and distance-field results stay as they were.  The result buffers grow on demand and are released by mrh_destroy.
 *
 * Errors: MRH_ERR_INVALID_ARG for a null context / parameter block / required pointer, an unknown field or output bit, a
 * reserved word that is not 0, n > MRH_QUERY_MAX_POINTS, R without t (or t without R) or a pose that is not finite, before the
 * map is touched; MRH_ERR_STATE while an exchange is pending; MRH_ERR_UNSUPPORTED on a sharded context (shard_count > 1).
 */
#ifndef MRHASH_QUERY_H
#define MRHASH_QUERY_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_QUERY_FIELD_MAP    0   /* the reference's trilinearInterpolation: what the mesh and the render see */
#define MRH_QUERY_FIELD_SMOOTH 1   /* true trilinear weights, analytic gradient                                */

#define MRH_QUERY_GRADIENT 1u      /* produce the gradient [n * 3] f32        */
#define MRH_QUERY_COLOUR   2u      /* produce r, g, b, weight [n * 4] u8      */
#define MRH_QUERY_MAX_POINTS (1u << 24)

#define MRH_QUERY_BLOCK   0x01u    /* bits of a state byte: the voxel that covers P is in the map */
#define MRH_QUERY_DIST    0x02u    /* dist is valid                                               */
#define MRH_QUERY_GRAD    0x04u    /* the gradient is valid                                       */
#define MRH_QUERY_COARSE  0x08u    /* P lies in a coarse block (h = 2 vs)                         */
#define MRH_QUERY_REFUSED 0x80u    /* a missing return, not finite, or outside the bound          */

typedef struct mrh_query_params {
  int32_t  field;                  /* MRH_QUERY_FIELD_*                                           */
  uint32_t outputs;                /* MRH_QUERY_GRADIENT | MRH_QUERY_COLOUR; dist and state are always produced */
  uint32_t reserved[2];            /* must be 0                                                   */
} mrh_query_params;                /* 16 bytes */

/* Queries n points xyz_host [n * 3] f32.  R and t are both NULL (the points are in the world frame) or both set (the points are
 * in the sensor frame, R [9] row-major and t [3] the sensor-to-world pose).  Blocks.  The results are host buffers owned by ctx
 * until the next mrh_query_points or mrh_destroy: dist [n] f32, grad [n * 3] f32, rgbw [n * 4] u8, state [n] u8.  A NULL
 * out-pointer = not wanted; grad / rgbw are only produced when their MRH_QUERY_* bit is set as well (else the out-pointer is set
 * to NULL).  The gradient is evaluated when its bit is set: a NULL out_grad only saves its copy to the host.  n == 0 succeeds
 * with nothing launched (every out-pointer is set to NULL; xyz_host may be NULL). */
int mrh_query_points(mrh_ctx* ctx, const mrh_query_params* p, const float* xyz_host, uint64_t n, const float R_row_major[9], const float t[3],
                     const float** out_dist, const float** out_grad, const uint8_t** out_rgbw, const uint8_t** out_state);

/* The same from a device buffer d_xyz [n * 3] f32 into caller device buffers ([n] f32, [n * 3] f32, [n * 4] u8, [n] u8; d_dist
 * and d_state are required, d_grad / d_rgbw may be NULL = skip and also need their MRH_QUERY_* bit; the gradient is evaluated,
 * and MRH_QUERY_GRAD reported, only when it is written).  Enqueues on the context's stream: ordered after every earlier call,
 * finished by mrh_sync or any blocking call; the buffers must stay valid until then. */
int mrh_query_points_device(mrh_ctx* ctx, const mrh_query_params* p, const float* d_xyz, uint64_t n, const float R_row_major[9], const float t[3],
                            float* d_dist, float* d_grad, uint8_t* d_rgbw, uint8_t* d_state);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_QUERY_H */
