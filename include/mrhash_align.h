/*
 * mrhash_align.h — map-to-map registration: the rigid transform between two maps, estimated from the maps alone
 * (libmrhash_hip.so, kernels in mrhash_amd/csrc/mrh_align.h).
 *
 * mrh_fuse_map (mrhash_remap.h) merges a second map into a first under a rigid transform (R, t); mrh_align_map estimates that
 * transform.  It minimises, over the transform, the squared difference between the two signed-distance fields at the source
 * map's near-surface voxels (SDF-to-SDF registration), by Gauss-Newton steps with the fixed-point sums, the binary64 Cholesky
 * solve and the pose update of the tracker (mrhash_track.h).  No depth frame is needed: a sub-map whose frames are gone, a map
 * restored from disk or a frame-sharded rank's sub-map are aligned as they stand.  The reference has no registration; the
 * definition is this project's.  DESIGN.md D19 is the normative statement, tests/align_ref.py restates it in numpy.
 *
 * (R, t) is the pose of the source map's frame in the destination's world, W = R P + t: the convention of mrhash_remap.h.  All
 * device arithmetic is binary32 without contraction, sums parenthesised left to right.  vs_s: the source's finest voxel size,
 * vs_d: the destination's.
 *
 * Source samples, once per call: for every live block of src on the device, of resolution r at position b, k = 1 << r, and every
 * stored voxel l (0 .. 8 / k - 1 per axis) the cell sits at the integer voxel coordinate v = 8 b + k l.  The cell is accepted iff
 * weight >= max(1, min_weight), fabsf(s) < band for its sdf s (a NaN fails) and, when extent > 0 was given,
 * fabsf(P_a - c_a) <= extent on all three axes.  The sample is (P, s), P_a = (float) v_a * vs_s.
 *
 * Pivot c (source frame) and extent: the caller's when extent > 0.  Otherwise, from the integer bounding box lo, hi of the
 * accepted v: c_a = (float) ((lo_a + hi_a) >> 1) * vs_s (a signed 64-bit sum) and extent = (float) (max_a (hi_a - lo_a) / 2 + 1)
 * * vs_s.  The fixed-point scale of the rotation part is S_a = 16384 / L, L the smallest power of two >= 2 extent.
 *
 * State: R in binary64 (the input widened) and tau = R c + t in binary64, each row ((R_i0 c_x + R_i1 c_y) + R_i2 c_z) + t_i.
 * A linearisation uses R32 = (float) R and tau32 = (float) tau.  Per sample:
 *   1  q = P - c;  a = R32 q, each row (R_i0 x + R_i1 y) + R_i2 z;  W = a + tau32
 *   2  rejected unless fabsf(W_a) < (float) (1 << 20) * vs_d on all axes (the bound of mrhash_query.h, before any conversion)
 *   3  h = getVoxelSize(W) on dst; d, g = the SMOOTH distance and gradient of mrhash_query.h at W on dst; rejected unless all
 *      eight corners are found with weight > 0
 *   4  rejected unless fabsf(d) < band
 *   5  e = s - d; rejected unless fabsf(e) <= dist_max
 *   6  J = (a x g, g), the cross product ((a_y g_z - a_z g_y), (a_z g_x - a_x g_z), (a_x g_y - a_y g_x)): the rotation is about
 *      the pivot
 *   7  J~_i = (int) rint(J_i * S_a) for i < 3, (int) rint(J_i * 16384) for i >= 3, e~ = (int) rint(e * 262144); rejected unless
 *      every scaled |J_i| < 32768
 *   8  the 29 exact 64-bit sums of mrhash_track.h over the accepted samples: 21 of the upper triangle of sum J~ J~^T (row-major),
 *      6 of sum J~ e~, sum e~^2, the count; sums[29 .. 31] are 0
 * With at most 2^26 samples every sum fits a signed 64-bit word: |sum J~ J~| < 2^56, |sum J~ e~| < 2^59 and sum e~^2 < 2^62
 * (|e~| <= 2^18 since dist_max <= 1).
 *
 * `iterations` times: linearise, solve (too few samples, sums[28] < min_samples, or a pivot of the Cholesky factorisation that
 * is not finite or not above 2^-20 of its diagonal entry: lost), update (R, tau) <- (dR R, tau + v) as mrhash_track.h does; no
 * early exit.  A lost step ends the loop with the pose from before it and status MRH_ALIGN_LOST; the call still returns MRH_OK.
 * The result is t = tau - R c in binary64 (the same row shape, subtracted from tau); out_R and out_t are (float) R, (float) t.
 * An empty sample list gives MRH_ALIGN_LOST with the pose as given, and nothing is launched on dst.
 *
 * Conventions as in mrhash_hip.h.  Both contexts enter like every other reader of the map (see mrhash_raycast.h): a host-fed
 * frame that mrh_integrate kept back runs first.  The call only reads both maps: camera, pose, images, counters, mrh_stats, the
 * last extraction and the results of the other readers stay as they were on both.  Blocks of the source that a wrapper's host
 * chunk grid has paged out are not in the device map and take no part.
 *
 * Errors, all raised before either map is touched: MRH_ERR_INVALID_ARG for a null argument (out_info may be NULL), a parameter
 * outside its range, a reserved word that is not 0, a pose that is not finite or not a rotation (|R R^T - I| <= 2^-10 in every
 * entry, as mrhash_remap.h), dst == src, contexts on different devices; MRH_ERR_STATE while an exchange is pending on either
 * context; MRH_ERR_UNSUPPORTED when either context is sharded (shard_count > 1).  MRH_ERR_CAPACITY when the sample list would
 * pass 2^26 entries.
 */
#ifndef MRHASH_ALIGN_H
#define MRHASH_ALIGN_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRH_ALIGN_OK 0
#define MRH_ALIGN_LOST 1
#define MRH_ALIGN_MAX_ITERATIONS 64
#define MRH_ALIGN_MAX_SAMPLES (1u << 26)

typedef struct mrh_align_params {
  float    band;             /* a cell / a sample needs |sdf| < band; 0 = min(src, dst sdf_truncation); (0, 1] m           */
  float    dist_max;         /* gate on |e|; 0 = min(band, 1); (0, 1]                                                      */
  int32_t  iterations;       /* 1 .. 64; 0 = 10                                                                            */
  uint32_t min_samples;      /* fewer accepted samples: lost; 0 = 64                                                       */
  uint32_t min_weight;       /* a cell needs weight >= max(1, min_weight); <= 255                                          */
  float    pivot[3];         /* with extent > 0: the pivot c, source frame; finite                                         */
  float    extent;           /* > 0: crop |P_a - c_a| <= extent and lever of the fixed point; 0 = automatic; >= 0, finite  */
  uint32_t reserved[3];      /* must be 0                                                                                  */
} mrh_align_params;          /* 48 bytes */

typedef struct mrh_align_info {
  int32_t  status;           /* MRH_ALIGN_OK / MRH_ALIGN_LOST                                                              */
  int32_t  iterations_done;  /* updates applied                                                                            */
  uint64_t source_blocks;    /* live blocks of the source                                                                  */
  uint64_t samples;          /* source samples gathered                                                                    */
  uint64_t accepted;         /* samples of the last linearisation performed that passed every gate (= sums[28])            */
  double   rms;              /* of e over them, metres                                                                     */
  float    pivot[3];         /* the pivot and the extent used                                                              */
  float    extent;
  int64_t  sums[32];         /* of the last linearisation performed                                                        */
} mrh_align_info;            /* 312 bytes */

/* Estimates the pose of src's frame in dst's world from the initial (R_init, t_init).  Blocks.  out_info may be NULL. */
int mrh_align_map(mrh_ctx* dst, mrh_ctx* src, const mrh_align_params* p, const float R_init[9], const float t_init[3],
                  float out_R[9], float out_t[3], mrh_align_info* out_info);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_ALIGN_H */
