/*
 * mrhash_track.h — the pose of a pinhole depth frame or of a LiDAR scan from the fused map: point-to-plane ICP against one raycast
 * of the map (libmrhash_hip.so; kernels in mrhash_amd/csrc/mrh_track.h, solve in mrhash_amd/csrc/mrh_tracksolve.h).  The reference has no
 * tracker; DESIGN.md D14 is the normative statement and tests/track_ref.py restates it in numpy.  Every sum is an exact
 * integer and the solve is a fixed sequence of IEEE operations, so the result is reproducible bit for bit.
 *
 * Model    one mrh_raycast render from (R_r, t_r) = (R_init, t_init) with the same intrinsics, size, depth
 *          range and step: depth M_d and world-frame normals M_n.  Rendered once per call.
 * State    R (3 x 3) and t in binary64, starting as the binary32 inputs widened; a linearisation uses R32 = (float) R, t32 = (float) t.
 * Per pixel (r, c) of the depth image D, binary32, no FMA contraction, sums left to right as parenthesised:
 *   1  accept only D > min_depth && D <= max_depth (a NaN fails); d_c = (ifx * ((c - cx) - 0.5), ify * ((r - cy) - 0.5), 1) with
 *      ifx = 1 / fx, ify = 1 / fy; p_c = (D d_c.x, D d_c.y, D)
 *   2  a = R32 p_c, each row (R_i0 x + R_i1 y) + R_i2 z; p_w = a + t32
 *   3  q = R_r^T (p_w - t_r), the same sum shape; reject unless q.z > min_depth
 *   4  u = (fx * (q.x / q.z) + cx) + 1, v = (fy * (q.y / q.z) + cy) + 1: the pixel whose render ray passes closest; reject unless
 *      0 <= u < cols and 0 <= v < rows (tested in float); c' = (int) floor(u), r' = (int) floor(v)
 *   5  m = M_d[r', c'], reject if m == 0; V = t_r + m * (R_r d_c(r', c')); N = M_n[r', c']
 *   6  delta = V - p_w; reject unless (dx^2 + dy^2) + dz^2 <= dist_max * dist_max; e = (N.x dx + N.y dy) + N.z dz
 *   7  J = (a x N, N) with (a x N).x = a.y N.z - a.z N.y and cyclic: the rotation is about the camera centre
 *   8  fixed point: S_a = 16384 / L, L the smallest power of two >= 2 * max_depth; J~_i = (int) rint(J_i * S_a) for i < 3,
 *      (int) rint(J_i * 16384) for i >= 3, e~ = (int) rint(e * 262144); reject unless every |J_i * scale| < 32768
 *   9  29 exact 64-bit sums over the accepted pixels: the upper triangle of sum J~ J~^T (row-major 00, 01, .., 05, 11, .., 55),
 *      sum J~ e~ (6), sum e~^2, the count n.  They are mrh_track_info.sums[0 .. 28]; sums[29 .. 31] are 0.
 * Solve    (host, binary64) lost if n < min_pixels.  H_ij = H~_ij / (s_i s_j), b_i = b~_i / (s_i 2^18), s = (S_a, S_a, S_a, 2^14,
 *          2^14, 2^14).  Column Cholesky j = 0 .. 5: d = H_jj - L_j0^2 - .. - L_j,j-1^2; lost unless d is finite and
 *          d > H_jj 2^-20; L_jj = sqrt(d), L_ij = (H_ij - sum_{k<j} L_ik L_jk) / L_jj, every sum subtracted term by term, k ascending.
 *          Forward and back substitution in the same style give xi = (omega, v).
 * Update   h = omega / 2, nu = sqrt(((h.x^2 + h.y^2) + h.z^2) + 1), unit quaternion (h / nu, 1 / nu), dR its rotation matrix
 *          (Eigen's toRotationMatrix formula in binary64), R <- dR R (row by column, left to right), t <- t + v.
 * Loop     `iterations` times linearise, solve, update; no early exit on a small step.  A lost step ends the loop with the pose
 *          from before that step: status MRH_TRACK_LOST, and the call still returns MRH_OK.
 *
 * Scans    (mrh_track_scan; DESIGN.md D15 is normative, tests/track_scan_ref.py restates it) n sensor-frame points p_s against one
 *          mrh_raycast_spherical render (D13) from (R_r, t_r): range M_rho, world-frame normals M_n, sensor-frame points M_p.
 *          Everything above holds except steps 1-5, which read per point:
 *   1  rho_p = sqrtf((x^2 + y^2) + z^2); accept only rho_p > min_depth && rho_p <= max_depth ((0, 0, 0), a NaN, an infinity fail)
 *   2  a = R32 p_s; p_w = a + t32
 *   3  q = R_r^T (p_w - t_r); rho_q = sqrtf((q.x^2 + q.y^2) + q.z^2); accept only rho_q > min_depth && rho_q <= max_depth
 *   4  az = mrh_atan2f(q.y, q.x), el = mrh_asinf(q.z / rho_q) (mrh_softmath.h); u = (fx * az + cx) + 1, v = (fy * el + cy) + 1;
 *      the same bounds test and floor; no azimuth wrap
 *   5  reject if M_rho[r', c'] == 0 or if N = M_n[r', c'] is the zero vector (a hit without a gradient gives no row and does not
 *      count); V = t_r + R_r M_p[r', c'] (the product in the row shape, then added to t_r)
 *          mrh_track_info.pixels and min_pixels count points.  A map that is to be tracked against needs a truncation that
 *          renders the ground: without it height is unobservable and the pivot gate reports MRH_TRACK_LOST.
 *
 * Conventions as in mrhash_hip.h.  The tracker is a reader of the map with exactly the raycast's contract (mrhash_raycast.h):
 * a frame that mrh_integrate kept back runs first and the frame pipeline restarts; camera, pose, images, counters, mrh_stats
 * and the last extraction stay as they were; the depth image or the cloud comes with the call, and the frame path's uploaded image, the
 * current scan (mrh_upload_points / mrh_set_points_device), its normals and its layout are neither read nor replaced.  Its device
 * and pinned buffers grow on demand and are released by mrh_destroy.
 *
 * Errors: MRH_ERR_INVALID_ARG for a null argument, a bad parameter (the raycast's rules, dist_max outside (0, 1], more than 64
 * iterations, more than 2^24 points); MRH_ERR_STATE while an exchange is pending; MRH_ERR_UNSUPPORTED on a sharded context (shard_count > 1).
 */
#ifndef MRHASH_TRACK_H
#define MRHASH_TRACK_H

#include "mrhash_raycast.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_TRACK_OK   0   /* every iteration was solved and applied */
#define MRH_TRACK_LOST 1   /* a step found too few pixels or a degenerate system; the pose is the one before that step */
#define MRH_TRACK_MAX_ITERATIONS 64

typedef struct mrh_track_params {
  float    fx, fy, cx, cy;          /* intrinsics of the model render (and of the depth image); scans: spherical */
  int32_t  rows, cols;              /* 1 .. MRH_RAYCAST_MAX_SIDE each                                     */
  float    min_depth, max_depth;    /* 0 < min_depth < max_depth (metres, camera z)                        */
  float    step;                    /* sample spacing of the model render; 0 = 0.5 * sdf_truncation        */
  float    dist_max;                /* association gate in (0, 1] metres; 0 = min(2 * sdf_truncation, 1)   */
  int32_t  iterations;              /* 1 .. 64; 0 = 10                                                     */
  uint32_t min_pixels;              /* fewer accepted pixels = lost; 0 = 64                                */
} mrh_track_params;                 /* 48 bytes */

typedef struct mrh_track_info {
  int32_t  status;                  /* MRH_TRACK_*                                                         */
  int32_t  iterations_done;         /* updates applied                                                     */
  uint64_t pixels;                  /* n of the last linearisation performed                               */
  double   rms;                     /* sqrt(sum e~^2 / n) / 2^18 of that linearisation, metres (0 if n = 0) */
  int64_t  sums[32];                /* its 29 sums, then three zeros                                       */
} mrh_track_info;                   /* 280 bytes */

/* Estimates the camera-to-world pose of the depth image (host, [rows * cols] f32, metres, row-major) starting from
 * (R_init row-major, t_init), in the convention of mrh_set_pose.  The image is copied through pinned staging.  Blocks.
 * out_R [9] and out_t [3] receive (float) R and (float) t; out_info may be NULL. */
int mrh_track_depth(mrh_ctx* ctx, const mrh_track_params* p, const float* depth_host, const float R_init[9], const float t_init[3],
                    float out_R[9], float out_t[3], mrh_track_info* out_info);

/* The same with the image already on the device ([rows * cols] f32 on the context's device; it must stay valid until the call
 * returns).  Blocks too: the solve is on the host. */
int mrh_track_depth_device(mrh_ctx* ctx, const mrh_track_params* p, const float* d_depth, const float R_init[9], const float t_init[3],
                           float out_R[9], float out_t[3], mrh_track_info* out_info);

/* Estimates the sensor-to-world pose of a LiDAR scan: n points (host, [n * 3] f32, metres, sensor frame, organised or not;
 * a missing return is (0, 0, 0)) against one spherical render of the map (see "Scans" above).  p->fx .. p->cols are the
 * spherical intrinsics of that render as mrh_raycast_spherical takes them, min_depth / max_depth are ranges, min_pixels counts
 * points.  n <= 2^24; n = 0 returns MRH_OK with status MRH_TRACK_LOST and the pose as given.  The cloud is copied through
 * pinned staging.  Blocks. */
int mrh_track_scan(mrh_ctx* ctx, const mrh_track_params* p, const float* points_host, size_t n, const float R_init[9], const float t_init[3],
                   float out_R[9], float out_t[3], mrh_track_info* out_info);

/* The same with the cloud already on the device ([n * 3] f32 on the context's device, e.g. the points image of
 * mrh_raycast_spherical_device; it must stay valid until the call returns).  Blocks too. */
int mrh_track_scan_device(mrh_ctx* ctx, const mrh_track_params* p, const float* d_points, size_t n, const float R_init[9], const float t_init[3],
                          float out_R[9], float out_t[3], mrh_track_info* out_info);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_TRACK_H */
