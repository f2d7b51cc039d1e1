/*
 * mrhash_raycast.h — rendering the fused map from a camera: per-pixel depth, world-frame normal and colour of the first
 * zero crossing of the TSDF along each pixel ray (libmrhash_hip.so, kernel in mrhash_amd/csrc/mrh_raycast.h), for the pinhole
 * model (mrh_raycast) and for the spherical model of LiDAR scans and range images (mrh_raycast_spherical: range, and the
 * predicted scan as sensor-frame points).
 *
 * The reference has the pieces of such a raycaster (findIntersectionLinear / findIntersectionBisection, vds.cu:340-383;
 * n_iteration_bisection = 3, params.h:26; struct RayCastSample, vhu.cuh:40-44) but no kernel that uses them.  The
 * definition below assembles its trilinearInterpolation (vds.cu:260-338) and findIntersectionBisection into one pixel
 * function; DESIGN.md D11 is the normative statement, tests/raycast_ref.py restates it in numpy.
 *
 * Per pixel (r, c), binary32 throughout, no FMA contraction:
 *   ray     d_c = (ifx * ((c - cx) - 0.5), ify * ((r - cy) - 0.5), 1), d_w = R d_c, P(z) = t + z d_w   (camera.cuh:88)
 *   samples z_k = min_depth + k * step, k = 0, 1, ... while z_k <= max_depth (at most 2^20 samples)
 *   valid   the block of P(z_k) (finest voxel size) is in the map AND trilinearInterpolation(P(z_k)) succeeds
 *   hit     the first k with sample k-1 valid, D > 0 and sample k valid, D <= 0 (back faces are ignored), refined by 3
 *           bisection steps (vds.cu:348-383); a failed trilinear inside the refinement rejects the crossing
 *   depth   camera z of the refined crossing (metres); normal = normalised central difference of the TSDF over one voxel of
 *           the local size (world frame); rgb = colour of the voxel at the crossing.  No hit: 0, (0,0,0), (0,0,0).
 *
 * The spherical camera (MRH_CAMERA_SPHERICAL: LiDAR scans and range images) renders through mrh_raycast_spherical[_device];
 * DESIGN.md D13 is the normative statement, tests/raycast_sph_ref.py restates it.  Everything is as above but:
 *   ray     az = ifx * ((c - cx) - 0.5), el = ify * ((r - cy) - 0.5), d_c = (cos az cos el, sin az cos el, sin el) with sine and
 *           cosine from mrh_sincosf (mrh_softmath.h; camera.cuh:91-99 with d = 1), d_w = R d_c, P(rho) = t + rho d_w
 *   samples rho_k = min_depth + k * step: min_depth, max_depth and step are RANGES along the ray, as mrh_set_camera means
 *           them for the spherical model
 *   range   the refined rho itself (it is not re-normalised by |d_w|); a miss is 0
 *   points  (MRH_RAYCAST_POINTS) rho * d_c per pixel: the crossing in the SENSOR frame, exactly the point the integration's
 *           back-projection gives range rho at pixel (r, c).  A miss is (0, 0, 0), the missing-return convention: the image
 *           is an organised scan of `cols` points per row that mrh_upload_points / mrh_set_points_device (with
 *           mrh_set_scan_layout(cols)) take as it is.
 * Intrinsics for which a corner pixel's |az| or |el| exceeds MRH_SM_SINCOS_MAX (8192 rad, the range on which mrh_sincosf is
 * specified) are refused.
 *
 * Conventions as in mrhash_hip.h.  All four calls enter like every other reader of the map: a host-fed frame that
 * mrh_integrate kept back runs first, pipelined frames in flight are integrated ahead of the raycast and the zombies
 * nobody wanted are reclaimed — so a raycast between two mrh_integrate calls restarts the frame pipeline, as any other
 * map reader does.  Blocks paged out to the host (mrh_stream_out) are not in the map and are not rendered.  The raycast
 * changes nothing of the frame path: camera, pose, images, counters, mrh_stats and the last extraction stay as they
 * were.  Its own device and pinned host buffers grow on demand and are released by mrh_destroy.
 *
 * Errors: MRH_ERR_INVALID_ARG for a null context / parameter block / pose, a bad parameter or more than 2^20 samples per
 * ray; MRH_ERR_STATE while an exchange is pending; MRH_ERR_UNSUPPORTED on a sharded context (shard_count > 1).
 */
#ifndef MRHASH_RAYCAST_H
#define MRHASH_RAYCAST_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_RAYCAST_NORMALS 1u
#define MRH_RAYCAST_COLORS  2u
#define MRH_RAYCAST_POINTS  4u   /* spherical entry points only; mrh_raycast keeps refusing it */
#define MRH_RAYCAST_MAX_SIDE 4096
#define MRH_RAYCAST_MAX_SAMPLES (1u << 20)

typedef struct mrh_raycast_params {
  float    fx, fy, cx, cy;          /* intrinsics of the virtual camera (pinhole: pixels; spherical: fx, fy in pixels per
                                       radian, cx, cy as mrh_set_camera(..., MRH_CAMERA_SPHERICAL) means them)        */
  int32_t  rows, cols;              /* 1 .. 4096 each                                           */
  float    min_depth, max_depth;    /* 0 < min_depth < max_depth (metres: camera z; spherical, range along the ray) */
  float    step;                    /* metres along camera z (spherical: along the ray); 0 = 0.5 * sdf_truncation   */
  uint32_t outputs;                 /* MRH_RAYCAST_* bits; depth / range is always produced     */
} mrh_raycast_params;               /* 40 bytes */

/* Renders the map from the camera-to-world pose (R row-major, t; the convention of mrh_set_pose).  Blocks.  The images
 * are host buffers owned by ctx until the next raycast of either kind or mrh_destroy: depth [rows * cols] f32, normals
 * [rows * cols * 3] f32, rgb [rows * cols * 3] u8, row-major.  A NULL out-pointer = not wanted; normals / rgb are only
 * produced when their MRH_RAYCAST_* bit is set as well (else the out-pointer is set to NULL). */
int mrh_raycast(mrh_ctx* ctx, const mrh_raycast_params* p, const float R_row_major[9], const float t[3],
                const float** out_depth, const float** out_normals, const uint8_t** out_rgb);

/* The same into caller device buffers ([H*W] f32, [H*W*3] f32, [H*W*3] u8; NULL = skip, and normals / rgb also need their
 * MRH_RAYCAST_* bit).  Enqueues on the context's stream: ordered after every earlier call, finished by mrh_sync or any
 * blocking call; the buffers must stay valid until then. */
int mrh_raycast_device(mrh_ctx* ctx, const mrh_raycast_params* p, const float R_row_major[9], const float t[3],
                       float* d_depth, float* d_normals, uint8_t* d_rgb);

/* The same for the spherical camera model: range [rows * cols] f32, normals and rgb as above, points [rows * cols * 3] f32
 * (sensor frame, needs MRH_RAYCAST_POINTS).  The contract is mrh_raycast's; the host images are owned by ctx until the next
 * raycast of either kind. */
int mrh_raycast_spherical(mrh_ctx* ctx, const mrh_raycast_params* p, const float R_row_major[9], const float t[3],
                          const float** out_range, const float** out_normals, const uint8_t** out_rgb, const float** out_points);

/* ... and into caller device buffers, as mrh_raycast_device.  d_points [H*W*3] f32 can be handed to mrh_set_points_device of
 * any context on the same device once this context's stream has been synchronised (mrh_sync). */
int mrh_raycast_spherical_device(mrh_ctx* ctx, const mrh_raycast_params* p, const float R_row_major[9], const float t[3],
                                 float* d_range, float* d_normals, uint8_t* d_rgb, float* d_points);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_RAYCAST_H */
