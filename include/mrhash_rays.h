/*
 * mrhash_rays.h — ray queries: a list of arbitrary rays cast through the fused map (libmrhash_hip.so, kernel in
 * mrhash_amd/csrc/mrh_rays.h).
 *
 * Every ray of mrhash_raycast.h belongs to an image: it shares its origin with the other rays of the image and takes its
 * direction from a row and a column of a pinhole or a spherical camera.  A planner's segment A -> B (is it free of surfaces AND of
 * unobserved space?), the information gain of a candidate view (how many samples along the ray are still unknown?), a per-beam
 * LiDAR table, a fisheye camera or several sensors in one batch fit neither model.  Here every ray has its own origin, its own
 * direction and, optionally, its own end, and reports what it crossed besides what it hit.  The reference has no such call; the
 * definition is this project's.  DESIGN.md D21 is the normative statement, tests/rays_ref.py restates it in numpy.
 *
 * All arithmetic is binary32 without contraction.  Per ray i with origin o, direction d and, when given, end tmax_i:
 *   o_w, d_w   without a pose: o, d.  With a pose (R row-major and t, sensor-to-world, for the whole batch):
 *              o_w,a = ((R[3a] o_x + R[3a+1] o_y) + R[3a+2] o_z) + t[a],  d_w,a = (R[3a] d_x + R[3a+1] d_y) + R[3a+2] d_z
 *   P(z)       o_w + z d_w per component.  THE DIRECTION IS USED AS GIVEN, it is not normalised: z counts multiples of d, as the
 *              range of the spherical render does.  With a unit direction z is metres
 *   samples    z_k = min_range + k * step (each computed afresh), k = 0, 1, ... while z_k <= max_range — at most
 *              MRH_RAYS_MAX_SAMPLES, counted on the host as for the render — and, per ray, while z_k <= end_i,
 *              end_i = tmax given ? fminf(tmax_i, max_range) : max_range.  min_range >= 0 (0: a segment starts at its origin);
 *              step 0 = 0.5 * sdf_truncation.  A ray with no sample (end_i < min_range) is not bad: status 0, counts 0
 *   bad ray    a component of o_w or d_w that is not finite; d_w == (+-0, +-0, +-0); not (fabsf(o_w,a) < bound) on some axis,
 *              bound = (float) (1 << 20) * vs as for point queries (mrhash_query.h), computed once on the host; tmax_i is NaN.
 *              The test runs before any float -> int conversion.  A bad ray is not marched: status = MRH_RAY_BAD, every other
 *              output +0
 *   valid, hit, refinement, normal, colour
 *              rules 3 - 5 of the render (mrhash_raycast.h), word for word, with P(z) above: a sample is valid
 *              when its block is in the map and trilinearInterpolation succeeds there; a hit is the first pair of consecutive
 *              valid samples with D(z_{k-1}) > 0 and D(z_k) <= 0 whose refinement (three steps) succeeds; range is the refined
 *              z, 0 without a hit; the normal and the colour are taken at P(range)
 *   K_i        the index of the sample that closes the accepted bracket (a hit), else the ray's number of samples
 *   n_unknown  the number of k < K_i whose sample is invalid (block absent, key out of range, or trilinear failed)
 *   n_free     the number of k < K_i whose sample is valid with D > 0
 *   first_unknown  z_k of the first invalid sample with k < K_i, else +0
 *   status     MRH_RAY_HIT; MRH_RAY_UNKNOWN (n_unknown > 0); MRH_RAY_INSIDE (some k < K_i is valid with D <= 0: the origin is
 *              behind a surface, a back face was crossed, or a crossing was rejected); MRH_RAY_BAD.
 *              status == 0  <=>  every sample of the ray was observed free space
 * The status bits are exact whether or not the counts are asked for.
 *
 * ORDER.  The kernel takes one lane per ray and a wave takes 64 consecutive rays OF THE CALLER'S ORDER: rays that are neighbours
 * in the list should be neighbours in space (the render's 8 x 8 tiles are such an order).  The library does not sort or reorder.
 * A ray's outputs do not depend on its neighbours.
 *
 * Conventions as in mrhash_hip.h.  Both calls enter like every other reader of the map (see mrhash_raycast.h): a host-fed frame
 * that mrh_integrate kept back runs first, pipelined frames in flight are integrated ahead of the call.  The calls only read the
 * map.  Nothing of the frame path changes: camera, pose, images, counters, mrh_stats, the last extraction and every other
 * reader's results stay as they were.  The scratch and result buffers grow on demand and are released by mrh_destroy.
 *
 * Errors, in this order, before the map is touched: MRH_ERR_INVALID_ARG for a null context / parameter block / required pointer;
 * MRH_ERR_STATE while an exchange is pending; MRH_ERR_UNSUPPORTED on a sharded context (shard_count > 1); then
 * MRH_ERR_INVALID_ARG for a reserved word that is not 0, an unknown output bit, a bad range (need 0 <= min_range <= max_range,
 * both finite), a bad step, more than MRH_RAYS_MAX_SAMPLES samples, n > MRH_RAYS_MAX_RAYS, R without t (or t without R), a pose
 * that is not finite.
 */
#ifndef MRHASH_RAYS_H
#define MRHASH_RAYS_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_RAYS_NORMALS 1u        /* produce the world-frame normal of the hit [n * 3] f32          */
#define MRH_RAYS_COLORS  2u        /* produce the colour of the hit [n * 3] u8                        */
#define MRH_RAYS_COUNTS  4u        /* produce n_free, n_unknown [n * 2] u32 and first_unknown [n] f32 */
#define MRH_RAYS_MAX_RAYS    (1u << 24)
#define MRH_RAYS_MAX_SAMPLES (1u << 20)

#define MRH_RAY_HIT     0x01u      /* bits of a status byte: range, normal and colour are those of a hit */
#define MRH_RAY_UNKNOWN 0x02u      /* a sample before the hit (or the end) is unobserved                 */
#define MRH_RAY_INSIDE  0x04u      /* a sample before the hit (or the end) is valid with D <= 0          */
#define MRH_RAY_BAD     0x80u      /* not finite, a zero direction, outside the bound, or tmax is NaN    */

typedef struct mrh_rays_params {
  float    min_range, max_range;   /* 0 <= min_range <= max_range, multiples of the direction           */
  float    step;                   /* sample spacing; 0 = 0.5 * sdf_truncation                          */
  uint32_t outputs;                /* MRH_RAYS_*; range and status are always produced                  */
  uint32_t reserved[4];            /* must be 0                                                         */
} mrh_rays_params;                 /* 32 bytes */

/* Casts n rays: origins_host and dirs_host [n * 3] f32, tmax_host [n] f32 or NULL (every ray ends at max_range).  R and t are
 * both NULL (world-frame rays) or both set (sensor-frame rays, R [9] row-major and t [3] the sensor-to-world pose).  Blocks.  The
 * results are host buffers owned by ctx until the next mrh_cast_rays or mrh_destroy: range [n] f32, status [n] u8, normals
 * [n * 3] f32, rgb [n * 3] u8, counts [n * 2] u32 (n_free, n_unknown per ray), first_unknown [n] f32.  A NULL out-pointer = not
 * wanted; normals / rgb / counts and first_unknown are only produced when their MRH_RAYS_* bit is set as well (else the
 * out-pointer is set to NULL).  n == 0 succeeds with nothing launched (every out-pointer is set to NULL; the inputs may be NULL). */
int mrh_cast_rays(mrh_ctx* ctx, const mrh_rays_params* p, const float* origins_host, const float* dirs_host, const float* tmax_host, uint64_t n,
                  const float R_row_major[9], const float t[3], const float** out_range, const uint8_t** out_status, const float** out_normals,
                  const uint8_t** out_rgb, const uint32_t** out_counts, const float** out_first_unknown);

/* The same from device buffers (d_tmax may be NULL) into caller device buffers; d_range and d_status are required, the others may
 * be NULL = skip and also need their MRH_RAYS_* bit (d_counts and d_first_unknown are written when MRH_RAYS_COUNTS is set and
 * the pointer is given, each on its own).  Enqueues on the context's stream: ordered after every earlier call, finished by
 * mrh_sync or any blocking call; the buffers must stay valid until then. */
int mrh_cast_rays_device(mrh_ctx* ctx, const mrh_rays_params* p, const float* d_origins, const float* d_dirs, const float* d_tmax, uint64_t n,
                         const float R_row_major[9], const float t[3], float* d_range, uint8_t* d_status, float* d_normals, uint8_t* d_rgb,
                         uint32_t* d_counts, float* d_first_unknown);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_RAYS_H */
