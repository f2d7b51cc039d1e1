/*
 * mrhash_normals.h — one surface normal per point of a LiDAR scan, estimated on the device (libmrhash_hip.so, kernels in
 * mrhash_amd/csrc/mrh_normals.h): what the normal-direction SDF (projective_sdf = 0) needs and mrh_upload_normals otherwise
 * has to be given.
 *
 * The reference estimates them on the CPU (GeoWrapper::setPointCloud with compute_normals, geowrapper.cpp:374-404: the smallest
 * eigenvector of a MAD-tree leaf of at most b_max = 0.4 m, turned towards the sensor, one normal per leaf).  Its tree is not
 * reproduced; what is kept is its nature — one plane per small neighbourhood, shared by the points in it, oriented per point —
 * its leaf size and its orientation rule.  DESIGN.md D12 is the normative statement, tests/normals_ref.py restates it in numpy.
 *
 * Per scan of n points (binary32, sensor frame: the sensor is the origin), rho = radius, no FMA contraction:
 *   missing    ||p|| = sqrt(x x + y y + z z) is not a positive finite number (a (0,0,0) return, a NaN): normal (0,0,0)
 *   cell       per component s = p / rho, c = floor(s), u = min(1023, (int) floor((s - c) 1024)); any |c| >= 2^20: fallback
 *   sums       per cell, exact integers: n, sum u, sum u u^T
 *   plane      of a cell: the sums of the 27 cells c + {-1,0,1}^3 shifted into its coordinate; covariance and a cyclic Jacobi
 *              eigen-decomposition (8 sweeps) in binary64; the cell normal is the eigenvector of the smallest eigenvalue
 *   gate       estimated iff N >= min_points, lambda1 >= (1024 min_spread)^2 and lambda0 <= max_flatness lambda1
 *   per point  estimated: the cell normal as binary32, negated when n . p > 0; else the fallback -p / ||p|| (the reversed
 *              beam: under it the normal-direction SDF is the projective one)
 * The result does not depend on the order of the points.
 *
 * Conventions as in mrhash_hip.h.  Nothing here reads or changes the map: frames in flight are not waited for, the frame
 * pipeline is not restarted, counters, mrh_stats and error flags stay as they were, and a sharded context is served like
 * any other.  The feature's device scratch (a cell table of 2 n slots and 4 bytes per point) grows on demand and is
 * released by mrh_destroy.
 *
 * Errors: MRH_ERR_INVALID_ARG for a null context or a null buffer with n > 0, a negative or non-finite parameter or
 * max_flatness >= 1; MRH_ERR_STATE when there is no current scan; MRH_ERR_CAPACITY for n >= 2^24 (the limit of
 * mrh_integrate_points).  n = 0 is MRH_OK.
 */
#ifndef MRHASH_NORMALS_H
#define MRHASH_NORMALS_H

#include "mrhash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mrh_normals_params {   /* 0 = the default, each */
  float    radius;        /* rho: side of a cell in metres; a neighbourhood is 3 x 3 x 3 cells.  Default 2 * virtual_voxel_size */
  uint32_t min_points;    /* fewest points in the 27 cells for an estimate.  Default 5                                            */
  float    min_spread;    /* smallest sqrt(lambda1), as a fraction of rho: a line of points is no plane.  Default 1 / 16          */
  float    max_flatness;  /* largest lambda0 / lambda1, < 1: an edge or a clump is no plane.  Default 1 / 16                      */
} mrh_normals_params;     /* 16 bytes */

typedef struct mrh_normals_info {
  uint64_t points;        /* n                                                        */
  uint64_t estimated;     /* points that took their cell's plane normal                */
  uint64_t fallback;      /* points that took the reversed beam                        */
  uint64_t missing;       /* points without a return: normal (0,0,0)                   */
  uint64_t cells;         /* occupied cells                                            */
} mrh_normals_info;       /* 40 bytes; points = estimated + fallback + missing */

/* Normals of the n points at d_xyz into d_nxyz (device buffers, [n][3] f32 each; they may not overlap).  Enqueues on the
 * context's stream: ordered after every earlier call, finished by mrh_sync or any blocking call; the buffers must stay valid
 * until then.  p = NULL: every default. */
int mrh_estimate_normals_device(mrh_ctx* ctx, const mrh_normals_params* p, const float* d_xyz, uint64_t n, float* d_nxyz);

/* Normals of the CURRENT scan (mrh_upload_points or mrh_set_points_device) into the context's normal buffer: afterwards the
 * scan has one normal per point exactly as after mrh_upload_normals.  Blocks only when out_info is not NULL. */
int mrh_estimate_normals(mrh_ctx* ctx, const mrh_normals_params* p, mrh_normals_info* out_info);

/* Blocking read-back of the context's normal buffer (mrh_estimate_normals or mrh_upload_normals): [*out_n][3] f32 in host
 * memory owned by ctx until the next mrh_get_normals or mrh_destroy.  out_info (may be NULL): the counts of the
 * mrh_estimate_normals that filled the buffer, all zero when mrh_upload_normals did. */
int mrh_get_normals(mrh_ctx* ctx, const float** out_nxyz, uint64_t* out_n, mrh_normals_info* out_info);

#ifdef __cplusplus
}
#endif

#endif /* MRHASH_NORMALS_H */
