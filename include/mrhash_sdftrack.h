/*
 * mrhash_sdftrack.h — render-free tracking: the pose of a pinhole depth frame or of a cloud of sensor-frame points, registered
 * directly against the map's signed-distance field (libmrhash_hip.so; kernels in mrhash_amd/csrc/mrh_sdftrack.h, solve in
 * mrhash_amd/csrc/mrh_tracksolve.h).  The trackers of mrhash_track.h associate every pixel with one render of the map; here the
 * observation's points are samples whose own signed distance is 0 and the residual is the map's distance at them (point-to-SDF
 * tracking in the sense of Bylow et al., RSS 2013): no render, no camera model for the points form, no field-of-view limit and no
 * azimuth seam.  Its limit is the truncation band: a point further than `band` from the surface gives no row.  The reference
 * has no tracker; DESIGN.md D20 is the normative statement and tests/sdftrack_ref.py restates it in numpy.  Every sum is an exact
 * integer and the solve is a fixed sequence of IEEE operations, so the result is reproducible bit for bit.
 *
 * State    R (3 x 3) and t in binary64, starting as the binary32 inputs widened; a linearisation uses R32 = (float) R, t32 = (float) t.
 *          Device arithmetic is binary32, no FMA contraction, sums left to right as parenthesised.  vs: the finest voxel size.
 * Depth form, per pixel (r, c) of the depth image D:
 *   1  step 1 of mrhash_track.h: accept only D > min_depth && D <= max_depth (a NaN fails); d_c = (ifx * ((c - cx) - 0.5),
 *      ify * ((r - cy) - 0.5), 1) with ifx = 1 / fx, ify = 1 / fy; p_c = (D d_c.x, D d_c.y, D)
 *   2  a = R32 p_c, each row (R_i0 x + R_i1 y) + R_i2 z; W = a + t32
 *   3  rejected unless fabsf(W_a) < (float) (1 << 20) * vs on all axes (the bound of mrhash_query.h, before any conversion);
 *      h = getVoxelSize(W); d, g = the SMOOTH distance and gradient of mrhash_query.h at W; rejected unless all eight corners
 *      are found with weight > 0; rejected unless fabsf(d) < band
 *   4  e = 0 - d: the sample's own distance is 0.  There is no separate residual gate; band <= 1 keeps |e~| <= 2^18
 *   5  J = (a x g, g), the cross product ((a_y g_z - a_z g_y), (a_z g_x - a_x g_z), (a_x g_y - a_y g_x)): the rotation is about
 *      the sensor centre
 *   6  fixed point as step 8 of mrhash_track.h: S_a = 16384 / L, L the smallest power of two >= 2 * max_depth; J~_i = (int)
 *      rint(J_i * S_a) for i < 3, (int) rint(J_i * 16384) for i >= 3, e~ = (int) rint(e * 262144); rejected unless every scaled
 *      |J_i| < 32768
 *   7  the 29 exact 64-bit sums of step 9 of mrhash_track.h over the accepted pixels; sums[29 .. 31] are 0
 * Points form, per point p_s = (x, y, z):
 *   1  steps 1-2 of "Scans" in mrhash_track.h: rho_p = sqrtf((x^2 + y^2) + z^2); accept only rho_p > min_depth && rho_p <=
 *      max_depth ((0, 0, 0), a NaN, an infinity fail); a = R32 p_s; W = a + t32
 *   2  steps 3-7 of the depth form.  fx .. cols are not read
 * Solve, update and loop are exactly those of mrhash_track.h: lost if n < min_pixels or at a pivot that is not finite or not
 * above 2^-20 of its diagonal entry; R <- dR R, t <- t + v; `iterations` times, no early exit.  A lost step ends the loop with
 * the pose from before that step: status MRH_TRACK_LOST, and the call still returns MRH_OK.  No point (n = 0) or an image
 * without an accepted pixel is lost with the pose as given.
 * Limits   images up to MRH_RAYCAST_MAX_SIDE^2 pixels, up to 2^24 points, up to 64 iterations: |J~ J~| <= 2^30, |J~ e~| < 2^33 and
 *          e~^2 <= 2^36 per sample, so every sum fits a signed 64-bit word as in mrhash_track.h.
 *
 * Conventions as in mrhash_hip.h.  The calls are readers of the map with exactly the contract of mrhash_track.h: a frame that
 * mrh_integrate kept back runs first and the frame pipeline restarts; camera, pose, images, counters, mrh_stats and the last
 * extraction stay as they were; the observation comes with the call, and the frame path's uploaded image and the current scan
 * are neither read nor replaced.  mrh_track_info and MRH_TRACK_OK / MRH_TRACK_LOST are those of mrhash_track.h.
 *
 * Errors, all raised before the map is touched: MRH_ERR_INVALID_ARG for a null argument (out_info may be NULL; n = 0 needs no
 * points), more than 2^24 points, a reserved word that is not 0, a bad parameter (depth form: the image shape and intrinsics by
 * the raycast's rules; 0 < min_depth < max_depth; band outside (0, 1]; more than 64 iterations), a pose that is not finite;
 * MRH_ERR_STATE while an exchange is pending; MRH_ERR_UNSUPPORTED on a sharded context (shard_count > 1).
 */
#ifndef MRHASH_SDFTRACK_H
#define MRHASH_SDFTRACK_H

#include "mrhash_track.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_SDFTRACK_MAX_POINTS (1u << 24)

typedef struct mrh_sdftrack_params {
  float    fx, fy, cx, cy;          /* depth form only; the points calls do not read them                  */
  int32_t  rows, cols;              /* depth form only: 1 .. MRH_RAYCAST_MAX_SIDE each                     */
  float    min_depth, max_depth;    /* camera z (depth form) / range (points form); 0 < min < max, metres  */
  float    band;                    /* a sample needs |d| < band; (0, 1] m; 0 = the context's sdf_truncation */
  int32_t  iterations;              /* 1 .. 64; 0 = 10                                                     */
  uint32_t min_pixels;              /* fewer accepted pixels / points = lost; 0 = 64                       */
  uint32_t reserved;                /* must be 0                                                           */
} mrh_sdftrack_params;              /* 48 bytes */

/* Estimates the camera-to-world pose of the depth image (host, [rows * cols] f32, metres, row-major) starting from
 * (R_init row-major, t_init), in the convention of mrh_set_pose.  The image is copied through pinned staging.  Blocks.
 * out_R [9] and out_t [3] receive (float) R and (float) t; out_info may be NULL. */
int mrh_track_depth_sdf(mrh_ctx* ctx, const mrh_sdftrack_params* p, const float* depth_host, const float R_init[9], const float t_init[3],
                        float out_R[9], float out_t[3], mrh_track_info* out_info);

/* The same with the image already on the device ([rows * cols] f32 on the context's device; it must stay valid until the call
 * returns).  Blocks too: the solve is on the host. */
int mrh_track_depth_sdf_device(mrh_ctx* ctx, const mrh_sdftrack_params* p, const float* d_depth, const float R_init[9], const float t_init[3],
                               float out_R[9], float out_t[3], mrh_track_info* out_info);

/* Estimates the sensor-to-world pose of n points (host, [n * 3] f32, metres, sensor frame, in any order, from any number of
 * sensors; a missing return is (0, 0, 0)).  n <= 2^24; n = 0 returns MRH_OK with status MRH_TRACK_LOST and the pose as given.
 * min_pixels and mrh_track_info.pixels count points.  The cloud is copied through pinned staging.  Blocks. */
int mrh_track_points_sdf(mrh_ctx* ctx, const mrh_sdftrack_params* p, const float* points_host, size_t n, const float R_init[9],
                         const float t_init[3], float out_R[9], float out_t[3], mrh_track_info* out_info);

/* The same with the cloud already on the device ([n * 3] f32 on the context's device, read as it lies; it must stay valid until
 * the call returns).  Blocks too. */
int mrh_track_points_sdf_device(mrh_ctx* ctx, const mrh_sdftrack_params* p, const float* d_points, size_t n, const float R_init[9],
                                const float t_init[3], float out_R[9], float out_t[3], mrh_track_info* out_info);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_SDFTRACK_H */
