// mrh_readerplan.h — the argument plans of the features that only read the map (mrh_readers.h: raycast, distance field, tracking,
// render-free tracking, point queries, ray queries, the free-space layer, map-to-map fusion and registration)
// and of the scan normals (mrh_points.h): the plain structs their kernels take, and per feature one function that turns the caller's
// parameter block plus the few context values it depends on — each passed by value — into that struct, or into an error code and
// the message the C ABI reports for it.  Plain host C++17, no HIP header, no mrh_ctx: the kernel headers include it for the
// structs, mrh_capi.hip for the plans, and tests/host/readerplan_check.cpp compiles it on its own.  Built with -ffp-contract=off
// like everything else.  The order of the checks is part of the contract: null block, pending exchange, sharded
// context, then the limits in the order written.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/mrh_softmath.h"
#include "../../include/mrhash_align.h"
#include "../../include/mrhash_esdf.h"
#include "../../include/mrhash_freespace.h"
#include "../../include/mrhash_normals.h"
#include "../../include/mrhash_query.h"
#include "../../include/mrhash_rays.h"
#include "../../include/mrhash_remap.h"
#include "../../include/mrhash_sdftrack.h"
#include "../../include/mrhash_track.h"

namespace mrh {

// k_raycast's camera (mrh_raycast.h)
struct RayCam {
  float ifx, ify, cx, cy;  // ifx = 1 / fx, ify = 1 / fy (host, IEEE)
  int rows, cols;
  float min_depth, max_depth, step;
  uint32_t n_samples;      // samples z_k <= max_depth, validated on the host: 1 .. 2^20
  float R[9], t[3];        // camera in world (row-major R)
};

// the box of the distance-field kernels (mrh_esdf.h)
struct EsdfBox {
  int ox, oy, oz;   // origin, finest voxels
  int nx, ny, nz;   // 1 .. 512 each
  uint32_t reach;   // R, 1 .. 4095 voxels
  int w_min;        // observed: weight >= w_min (>= 1)
  float band;       // site: |sdf| <= band; 0 = one voxel of the block's own resolution
};

// what k_query takes (mrh_query.h): the point count, the refusal bound and the sensor-to-world pose of a posed call
struct QueryArgs {
  uint32_t n;          // points, 1 .. 2^24 when the kernel runs
  float bound;         // (float) (1 << 20) * vs: a point is refused unless |P_a| < bound on every axis
  bool smooth, posed;  // the field; the points are in the sensor frame
  uint32_t outputs;    // MRH_QUERY_* bits
  float R[9], t[3];    // sensor in world (row-major R); identity and 0 when !posed
};

// what k_cast_rays takes (mrh_rays.h): the ray count, the samples of the batch, the refusal bound and the sensor-to-world pose
struct RaysArgs {
  uint32_t n;           // rays, 1 .. 2^24 when the kernel runs
  float min_range, max_range, step;
  uint32_t n_samples;   // samples z_k <= max_range, validated on the host: 1 .. 2^20
  float bound;          // (float) (1 << 20) * vs: a ray is bad unless |o_w,a| < bound on every axis
  bool posed;           // the rays are in the sensor frame
  uint32_t outputs;     // MRH_RAYS_* bits
  float R[9], t[3];     // sensor in world (row-major R); identity and 0 when !posed
};

// what the map-to-map kernels take (mrh_remap.h): the pose of the source frame in the destination's world, the destination
// lattice, the range bound on the source side and the size of a source block's candidate box
struct RemapArgs {
  float R[9], t[3];   // W = R P + t (row-major R); the sample kernels apply the transpose to W - t
  double F[9];        // (R^T)^-1 in binary64, row-major: W = F P + t inverts the sample kernels' P = R^T (W - t) whatever R is
  float vs_d;         // finest voxel size of the destination lattice
  float bound;        // (float) (1 << 20) * vs_s: a voxel is invalid unless |P_a| < bound on every axis
  uint32_t w_min;     // max(1, min_weight)
  int per_axis;       // destination blocks per axis a source block's candidate box holds at most (remap_per_axis)
};

// what k_align_gather takes (mrh_align.h): the pose-independent gates of a source cell
struct AlignGather {
  float vs_s;         // finest voxel size of the source
  float band;         // a cell needs fabsf(sdf) < band
  uint32_t w_min;     // ... and weight >= w_min = max(1, min_weight)
  bool crop;          // the caller gave pivot and extent: fabsf(P_a - c_a) <= extent on every axis
  float c[3], extent;
};

// what k_align_linearise takes (mrh_align.h): the estimate the linearisation is taken at and the gates of D19
struct AlignLin {
  float R[9], tau[3];  // R32 and tau32 = (float) (R c + t)
  float c[3];          // the pivot, source frame
  float band, dist_max;
  float s_a;           // mrh_track::angle_scale(extent)
  float bound;         // (float) (1 << 20) * vs_d: a sample is rejected unless |W_a| < bound on every axis
  uint32_t n;          // samples, 1 .. 2^26
};

// what k_sdftrack_depth_linearise and k_sdftrack_points_linearise take (mrh_sdftrack.h): the observation's gates, the gates of
// D20 and the estimate the linearisation is taken at
struct SdfTrackLin {
  float ifx, ify, cx, cy;  // depth form: ifx = 1 / fx, ify = 1 / fy (host, IEEE)
  int rows, cols;          // depth form: the image
  uint32_t n;              // points form: points, 1 .. 2^24
  float min_depth, max_depth;
  float band;
  float s_a;               // mrh_track::angle_scale(max_depth)
  float bound;             // (float) (1 << 20) * vs: a sample is rejected unless |W_a| < bound on every axis
  float R[9], t[3];        // R32 and t32
};

// the free-space layer (mrh_freespace.h, include/mrhash_freespace.h): its box of cells and the shape of its words.  A word is a
// 4 x 4 x 2 brick of cells (bit = x & 3 | (y & 3) << 2 | (z & 1) << 4), bricks x fastest
struct FreeLayer {
  int ox, oy, oz;       // origin, cells
  int nx, ny, nz;       // 1 .. 1024 each
  int shift;            // s: a cell is 2^s finest voxels per side
  int nbx, nby;         // bricks along x and y: (nx + 3) / 4, (ny + 3) / 4
  uint32_t n_words;     // nbx * nby * ((nz + 1) / 2)
};

// what k_freespace_carve takes: the camera (the points form uses its samples and pose alone), the ray count of the points form,
// the margin and the refusal bound
struct CarveArgs {
  RayCam cam;           // n_samples: samples z_k <= max_depth; step: the default filled in
  uint32_t n;           // points form: points, 1 .. 2^24
  float margin;
  float bound;          // (float) (1 << 20) * vs: a sample sets nothing unless |P_a| < bound on every axis
};

// what k_freespace_classify and k_freespace_frontier take: the box in cells, and the same box in finest voxels with the two gates
// of D16 as esdf_classify reads them (vox.reach is unused)
struct FreeBox {
  int ox, oy, oz;       // origin, cells
  int nx, ny, nz;       // 1 .. 512 each
  EsdfBox vox;          // origin << s, dims << s, w_min, band
};

// what k_freespace_segments takes
struct SegArgs {
  uint32_t n;           // segments, 1 .. 2^24
  float step;           // the default filled in
  float bound;          // (float) (1 << 20) * vs
};

// the parameters of the normal-estimation kernels (mrh_normals.h), defaults filled in
struct NrmPar {
  float rho;            // cell side (metres)
  uint32_t min_points;  // gate: points in the 27 cells
  double min_l1;        // gate: (1024 min_spread)^2, units of (rho / 1024)^2
  double max_flat;      // gate: lambda0 <= max_flat * lambda1
};

}  // namespace mrh

namespace mrh_plan {
namespace {  // internal to whoever includes the header, like mrh_xplan.h: the library exports none of it

constexpr size_t kMsgBytes = 512;  // = fail()'s buffer: a message passes through it unchanged

// fail() without a context: formats into msg[kMsgBytes] and returns the code
inline int refuse(char* msg, const int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, kMsgBytes, fmt, ap);
  va_end(ap);
  return code;
}

// What every reader needs of the map before its own limits: no exchange pending, one shard.  `lacks`: what a sharded map does not
// get from this feature, in the feature's own words
inline int whole_map(char* msg, const char* who, const char* lacks, const int pending, const int shard_count) {
  if (pending) return refuse(msg, MRH_ERR_STATE, "%s: an exchange is pending (call mrh_integrate_resume)", who);
  if (shard_count > 1) return refuse(msg, MRH_ERR_UNSUPPORTED, "%s: sharded maps %s (shard_count %d)", who, lacks, shard_count);
  return MRH_OK;
}

inline float ray_z_host(const float min_depth, const float step, const uint32_t k) { return min_depth + (float) k * step; }  // = ray_z (mrh_raycast.h)

// samples z_k <= z_max of a march that starts at z_0 = z_min <= z_max: z_k is monotone in k (two monotone roundings), so the count is
// found by bisection on k.  0: more than 2^20
inline uint32_t ray_sample_count(const float z_min, const float z_max, const float step) {
  if (ray_z_host(z_min, step, MRH_RAYCAST_MAX_SAMPLES) <= z_max) return 0;
  uint32_t lo = 0, hi = MRH_RAYCAST_MAX_SAMPLES;  // z(lo) <= z_max < z(hi)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ray_z_host(z_min, step, mid) <= z_max) lo = mid;
    else hi = mid;
  }
  return hi;
}

// a pose (R, t) whose twelve numbers are finite
inline int finite_pose(char* msg, const char* who, const float* R, const float* t) {
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(R[i])) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(t[i])) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  return MRH_OK;
}

// the arguments every raycast entry point shares (and tracking, through its model render); fills the kernel's camera.
// model: MRH_CAMERA_*; truncation: the context's sdf_truncation, for the default step
inline int raycast(char* msg, const char* who, const int model, const mrh_raycast_params* p, const float* R, const float* t, const float truncation,
                   const int pending, const int shard_count, mrh::RayCam* rc) {
  if (!p || !R || !t) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (const int e = whole_map(msg, who, "are not rendered", pending, shard_count)) return e;
  if (p->rows < 1 || p->rows > MRH_RAYCAST_MAX_SIDE || p->cols < 1 || p->cols > MRH_RAYCAST_MAX_SIDE)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: image of %d x %d pixels (1 .. %d per side)", who, p->rows, p->cols, MRH_RAYCAST_MAX_SIDE);
  if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || p->fx == 0.f || p->fy == 0.f || !std::isfinite(p->cx) || !std::isfinite(p->cy))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: bad intrinsics", who);
  if (!(p->min_depth > 0.f) || !(p->max_depth > p->min_depth) || !std::isfinite(p->max_depth))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: need 0 < min_depth < max_depth (got %g, %g)", who, (double) p->min_depth, (double) p->max_depth);
  const uint32_t known = MRH_RAYCAST_NORMALS | MRH_RAYCAST_COLORS | (model == MRH_CAMERA_SPHERICAL ? MRH_RAYCAST_POINTS : 0u);
  if (p->outputs & ~known) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: unknown output bits 0x%x", who, p->outputs);
  const float step = p->step == 0.f ? 0.5f * truncation : p->step;
  if (!(step > 0.f) || !std::isfinite(step)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the sample spacing must be > 0 (step %g)", who, (double) step);
  if (const int e = finite_pose(msg, who, R, t)) return e;
  const uint32_t n_samples = ray_sample_count(p->min_depth, p->max_depth, step);
  if (!n_samples)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: more than 2^20 samples per ray (min_depth %g, max_depth %g, step %g)", who, (double) p->min_depth,
                  (double) p->max_depth, (double) step);
  rc->ifx = 1.0f / p->fx;
  rc->ify = 1.0f / p->fy;
  rc->cx = p->cx; rc->cy = p->cy;
  rc->rows = p->rows; rc->cols = p->cols;
  if (model == MRH_CAMERA_SPHERICAL) {
    // every pixel's azimuth and elevation within the range mrh_sincosf is specified on: the kernel's expressions (ray_dir_sensor)
    // at the corner pixels — they are monotone in the column and in the row, so the corners bound every pixel
    const float az0 = rc->ifx * (((float) 0 - rc->cx) - 0.5f), az1 = rc->ifx * (((float) (rc->cols - 1) - rc->cx) - 0.5f);
    const float el0 = rc->ify * (((float) 0 - rc->cy) - 0.5f), el1 = rc->ify * (((float) (rc->rows - 1) - rc->cy) - 0.5f);
    const float worst = std::fmax(std::fmax(std::fabs(az0), std::fabs(az1)), std::fmax(std::fabs(el0), std::fabs(el1)));
    if (!(worst <= MRH_SM_SINCOS_MAX))
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a pixel's azimuth or elevation reaches %g rad (sine and cosine are specified up to %g)", who,
                    (double) worst, (double) MRH_SM_SINCOS_MAX);
  }
  rc->min_depth = p->min_depth; rc->max_depth = p->max_depth; rc->step = step;
  rc->n_samples = n_samples;
  for (int i = 0; i < 9; i++) rc->R[i] = R[i];
  for (int i = 0; i < 3; i++) rc->t[i] = t[i];
  return MRH_OK;
}

// the arguments both distance-field entry points share; fills the kernels' box.  min_weight_threshold: the context's, the default of w_min
inline int esdf(char* msg, const char* who, const mrh_esdf_params* p, const int min_weight_threshold, const int pending, const int shard_count,
                mrh::EsdfBox* bx) {
  if (!p) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (const int e = whole_map(msg, who, "have no distance field", pending, shard_count)) return e;
  for (int a = 0; a < 3; a++) {
    if (p->dims[a] < 1 || p->dims[a] > MRH_ESDF_MAX_SIDE)
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: box of %d x %d x %d cells (1 .. %d per side)", who, p->dims[0], p->dims[1], p->dims[2], MRH_ESDF_MAX_SIDE);
    const int64_t lo = p->origin[a], hi = lo + p->dims[a] - 1;
    if (lo < -(1ll << 23) || hi >= (1ll << 23))
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: axis %d of the box spans voxels %lld .. %lld, outside [-2^23, 2^23)", who, a, (long long) lo, (long long) hi);
  }
  if (p->max_distance_voxels < 1 || p->max_distance_voxels > MRH_ESDF_MAX_REACH)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: max_distance_voxels %d (1 .. %d)", who, p->max_distance_voxels, MRH_ESDF_MAX_REACH);
  if (!std::isfinite(p->surface_band) || p->surface_band < 0.f) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: surface_band %g", who, (double) p->surface_band);
  if (p->min_weight < 0) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: min_weight %d", who, p->min_weight);
  if (p->outputs & ~(MRH_ESDF_STATE | MRH_ESDF_SQUARED)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: unknown output bits 0x%x", who, p->outputs);
  bx->ox = p->origin[0]; bx->oy = p->origin[1]; bx->oz = p->origin[2];
  bx->nx = p->dims[0]; bx->ny = p->dims[1]; bx->nz = p->dims[2];
  bx->reach = (uint32_t) p->max_distance_voxels;
  bx->w_min = std::max(1, p->min_weight ? p->min_weight : min_weight_threshold);
  bx->band = p->surface_band;
  return MRH_OK;
}

// One tracking call with its defaults filled in: the model render's camera, the gate, the iteration count, the fewest pixels
struct Track {
  mrh::RayCam cam;
  float dist_max;
  int iterations;
  uint32_t min_pixels;
};
// model: MRH_CAMERA_PINHOLE (a depth image) or MRH_CAMERA_SPHERICAL (a scan of n points); have_obs: the image or the cloud was
// given (an empty scan needs none); have_out: both pose outputs were
inline int track(char* msg, const char* who, const int model, const mrh_track_params* p, const bool have_obs, const size_t n, const bool have_out,
                 const float* R0, const float* t0, const float truncation, const int pending, const int shard_count, Track* out) {
  const bool scan = model == MRH_CAMERA_SPHERICAL;
  if (!p || (!have_obs && !(scan && n == 0)) || !have_out) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (scan && n > ((size_t) 1 << 24)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %zu points in one scan (limit 2^24)", who, n);
  const mrh_raycast_params rp = {p->fx, p->fy, p->cx, p->cy, p->rows, p->cols, p->min_depth, p->max_depth, p->step,
                                 MRH_RAYCAST_NORMALS | (scan ? MRH_RAYCAST_POINTS : 0u)};
  if (const int e = raycast(msg, who, model, &rp, R0, t0, truncation, pending, shard_count, &out->cam)) return e;
  out->dist_max = p->dist_max == 0.f ? std::fmin(2.f * truncation, 1.f) : p->dist_max;
  if (!(out->dist_max > 0.f && out->dist_max <= 1.f))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the gate must lie in (0, 1] m (dist_max %g)", who, (double) out->dist_max);
  if (p->iterations < 0 || p->iterations > MRH_TRACK_MAX_ITERATIONS)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %d iterations (1 .. %d, 0 = 10)", who, p->iterations, MRH_TRACK_MAX_ITERATIONS);
  out->iterations = p->iterations ? p->iterations : 10;
  out->min_pixels = p->min_pixels ? p->min_pixels : 64u;
  return MRH_OK;
}

// ---- render-free tracking (include/mrhash_sdftrack.h) ----

// One render-free tracking call with its defaults filled in
struct Sdftrack {
  bool depth_form;
  float ifx, ify, cx, cy;  // depth form; zeros for the points form
  int rows, cols;
  float min_depth, max_depth, band;
  int iterations;
  uint32_t min_pixels;
};
// depth_form: a depth image of p->rows x p->cols pixels, else a cloud of n points; have_obs: the image or the cloud was given (an
// empty cloud needs none); have_out: both pose outputs were; truncation: the context's sdf_truncation, the default band.  The
// order: null argument -> more than 2^24 points -> pending, sharded -> reserved word -> (depth form) image shape, intrinsics ->
// depth range -> band -> iterations -> the pose
inline int sdftrack(char* msg, const char* who, const bool depth_form, const mrh_sdftrack_params* p, const bool have_obs, const size_t n, const bool have_out,
                    const float* R0, const float* t0, const float truncation, const int pending, const int shard_count, Sdftrack* out) {
  if (!p || (!have_obs && (depth_form || n != 0)) || !have_out || !R0 || !t0) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (!depth_form && n > (size_t) MRH_SDFTRACK_MAX_POINTS) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %zu points in one call (limit 2^24)", who, n);
  if (const int e = whole_map(msg, who, "are not tracked against", pending, shard_count)) return e;
  if (p->reserved) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  out->depth_form = depth_form;
  out->ifx = out->ify = out->cx = out->cy = 0.f;
  out->rows = out->cols = 0;
  if (depth_form) {
    if (p->rows < 1 || p->rows > MRH_RAYCAST_MAX_SIDE || p->cols < 1 || p->cols > MRH_RAYCAST_MAX_SIDE)
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: image of %d x %d pixels (1 .. %d per side)", who, p->rows, p->cols, MRH_RAYCAST_MAX_SIDE);
    if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || p->fx == 0.f || p->fy == 0.f || !std::isfinite(p->cx) || !std::isfinite(p->cy))
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: bad intrinsics", who);
    out->ifx = 1.0f / p->fx; out->ify = 1.0f / p->fy;
    out->cx = p->cx; out->cy = p->cy;
    out->rows = p->rows; out->cols = p->cols;
  }
  if (!(p->min_depth > 0.f) || !(p->max_depth > p->min_depth) || !std::isfinite(p->max_depth))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: need 0 < min_depth < max_depth (got %g, %g)", who, (double) p->min_depth, (double) p->max_depth);
  out->min_depth = p->min_depth; out->max_depth = p->max_depth;
  out->band = p->band == 0.f ? truncation : p->band;
  if (!(out->band > 0.f && out->band <= 1.f)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the band must lie in (0, 1] m (band %g)", who, (double) out->band);
  if (p->iterations < 0 || p->iterations > MRH_TRACK_MAX_ITERATIONS)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %d iterations (1 .. %d, 0 = 10)", who, p->iterations, MRH_TRACK_MAX_ITERATIONS);
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(R0[i])) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(t0[i])) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  out->iterations = p->iterations ? p->iterations : 10;
  out->min_pixels = p->min_pixels ? p->min_pixels : 64u;
  return MRH_OK;
}

// the arguments both point-query entry points share; fills the kernel's arguments.  have_points: the point list was given (n == 0
// needs none); have_out: the required outputs were (the blocking call has none: true); voxel_size: the context's
// virtual_voxel_size, for the refusal bound
inline int query(char* msg, const char* who, const mrh_query_params* p, const bool have_points, const bool have_out, const uint64_t n, const float* R,
                 const float* t, const float voxel_size, const int pending, const int shard_count, mrh::QueryArgs* out) {
  if (!p || (!have_points && n != 0) || !have_out) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (const int e = whole_map(msg, who, "are not queried", pending, shard_count)) return e;
  if (p->field != MRH_QUERY_FIELD_MAP && p->field != MRH_QUERY_FIELD_SMOOTH) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: unknown field %d", who, p->field);
  if (p->outputs & ~(MRH_QUERY_GRADIENT | MRH_QUERY_COLOUR)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: unknown output bits 0x%x", who, p->outputs);
  if (p->reserved[0] || p->reserved[1]) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  if (n > MRH_QUERY_MAX_POINTS) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %llu points in one call (limit 2^24)", who, (unsigned long long) n);
  if ((R != nullptr) != (t != nullptr)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: R and t are both null or both set", who);
  out->posed = R != nullptr;
  for (int i = 0; i < 9; i++) {
    out->R[i] = out->posed ? R[i] : (i % 4 == 0 ? 1.f : 0.f);
    if (!std::isfinite(out->R[i])) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  }
  for (int i = 0; i < 3; i++) {
    out->t[i] = out->posed ? t[i] : 0.f;
    if (!std::isfinite(out->t[i])) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  }
  out->n = (uint32_t) n;
  out->bound = (float) (1 << 20) * voxel_size;
  out->smooth = p->field == MRH_QUERY_FIELD_SMOOTH;
  out->outputs = p->outputs;
  return MRH_OK;
}

// the arguments both ray-query entry points share (include/mrhash_rays.h); fills the kernel's arguments.  have_rays:
// origins and directions were given (n == 0 needs none); have_out: the required outputs were (the blocking call has none: true);
// truncation: the context's sdf_truncation, for the default step; voxel_size: its virtual_voxel_size, for the refusal bound.  The
// sample count and the pose test are the render's (ray_sample_count, finite_pose).  The order: null argument -> pending, sharded
// -> reserved words -> output bits -> range -> step -> samples -> n -> R/t pairing -> the pose
inline int rays(char* msg, const char* who, const mrh_rays_params* p, const bool have_rays, const bool have_out, const uint64_t n, const float* R,
                const float* t, const float truncation, const float voxel_size, const int pending, const int shard_count, mrh::RaysArgs* out) {
  if (!p || (!have_rays && n != 0) || !have_out) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (const int e = whole_map(msg, who, "take no ray queries", pending, shard_count)) return e;
  if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3]) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  if (p->outputs & ~(MRH_RAYS_NORMALS | MRH_RAYS_COLORS | MRH_RAYS_COUNTS)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: unknown output bits 0x%x", who, p->outputs);
  if (!(p->min_range >= 0.f) || !(p->max_range >= p->min_range) || !std::isfinite(p->max_range))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: need 0 <= min_range <= max_range (got %g, %g)", who, (double) p->min_range, (double) p->max_range);
  const float step = p->step == 0.f ? 0.5f * truncation : p->step;
  if (!(step > 0.f) || !std::isfinite(step)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the sample spacing must be > 0 (step %g)", who, (double) step);
  const uint32_t n_samples = ray_sample_count(p->min_range, p->max_range, step);
  if (!n_samples)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: more than 2^20 samples per ray (min_range %g, max_range %g, step %g)", who, (double) p->min_range,
                  (double) p->max_range, (double) step);
  if (n > MRH_RAYS_MAX_RAYS) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %llu rays in one call (limit 2^24)", who, (unsigned long long) n);
  if ((R != nullptr) != (t != nullptr)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: R and t are both null or both set", who);
  out->posed = R != nullptr;
  if (out->posed)
    if (const int e = finite_pose(msg, who, R, t)) return e;
  for (int i = 0; i < 9; i++) out->R[i] = out->posed ? R[i] : (i % 4 == 0 ? 1.f : 0.f);
  for (int i = 0; i < 3; i++) out->t[i] = out->posed ? t[i] : 0.f;
  out->n = (uint32_t) n;
  out->min_range = p->min_range; out->max_range = p->max_range; out->step = step;
  out->n_samples = n_samples;
  out->bound = (float) (1 << 20) * voxel_size;
  out->outputs = p->outputs;
  return MRH_OK;
}
static_assert(MRH_RAYS_MAX_SAMPLES == MRH_RAYCAST_MAX_SAMPLES, "one sample count serves the render and the ray queries");

// ---- the free-space layer (include/mrhash_freespace.h) ----

// what every free-space call but the create needs after whole_map: a layer
inline int freespace_layer(char* msg, const char* who, const bool have_layer, const int pending, const int shard_count) {
  if (const int e = whole_map(msg, who, "have no free-space layer", pending, shard_count)) return e;
  if (!have_layer) return refuse(msg, MRH_ERR_STATE, "%s: the context has no free-space layer (call mrh_freespace_create)", who);
  return MRH_OK;
}

// half a cell: the default sample spacing of the carves and of the segments
inline float freespace_half_cell(const float voxel_size, const int shift) { return 0.5f * (voxel_size * (float) (1 << shift)); }

// mrh_freespace_create; fills the layer's box and word shape.  The order: null argument -> pending, sharded -> reserved word ->
// cell_shift -> dims per axis -> the cell count -> the voxel span per axis
inline int freespace_create(char* msg, const char* who, const mrh_freespace_params* p, const int pending, const int shard_count, mrh::FreeLayer* out) {
  if (!p) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (const int e = whole_map(msg, who, "have no free-space layer", pending, shard_count)) return e;
  if (p->reserved) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  if (p->cell_shift < 0 || p->cell_shift > MRH_FREESPACE_MAX_SHIFT) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: cell_shift %d (0 .. %d)", who, p->cell_shift, MRH_FREESPACE_MAX_SHIFT);
  for (int a = 0; a < 3; a++)
    if (p->dims[a] < 1 || p->dims[a] > MRH_FREESPACE_MAX_SIDE)
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: layer of %d x %d x %d cells (1 .. %d per side)", who, p->dims[0], p->dims[1], p->dims[2], MRH_FREESPACE_MAX_SIDE);
  const uint64_t cells = (uint64_t) p->dims[0] * (uint64_t) p->dims[1] * (uint64_t) p->dims[2];
  if (cells > (uint64_t) MRH_FREESPACE_MAX_CELLS)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: layer of %llu cells (limit 2^28)", who, (unsigned long long) cells);
  for (int a = 0; a < 3; a++) {
    const int64_t lo = (int64_t) p->origin[a] * (1ll << p->cell_shift), hi = ((int64_t) p->origin[a] + p->dims[a]) * (1ll << p->cell_shift) - 1;
    if (lo < -(1ll << 23) || hi >= (1ll << 23))
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: axis %d of the layer spans voxels %lld .. %lld, outside [-2^23, 2^23)", who, a, (long long) lo, (long long) hi);
  }
  out->ox = p->origin[0]; out->oy = p->origin[1]; out->oz = p->origin[2];
  out->nx = p->dims[0]; out->ny = p->dims[1]; out->nz = p->dims[2];
  out->shift = p->cell_shift;
  out->nbx = (out->nx + 3) / 4; out->nby = (out->ny + 3) / 4;
  out->n_words = (uint32_t) out->nbx * (uint32_t) out->nby * (uint32_t) ((out->nz + 1) / 2);  // <= 256 * 256 * 512
  return MRH_OK;
}

// the arguments the four carves share; fills the kernel's arguments.  depth_form: a depth image of p->rows x p->cols pixels, else
// a cloud of n points; have_obs: the image or the cloud was given (an empty cloud needs none); voxel_size and shift: the default
// step and the bound.  The sample count and the pose test are the render's.  The order: null argument -> more than 2^24 points ->
// pending, sharded, no layer -> reserved words -> (depth form) image shape, intrinsics -> depth range -> margin -> step -> the
// pose -> samples
inline int freespace_carve(char* msg, const char* who, const bool depth_form, const mrh_carve_params* p, const bool have_obs, const uint64_t n, const float* R,
                           const float* t, const bool have_layer, const float voxel_size, const int shift, const int pending, const int shard_count,
                           mrh::CarveArgs* out) {
  if (!p || (!have_obs && (depth_form || n != 0)) || !R || !t) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (!depth_form && n > (uint64_t) MRH_FREESPACE_MAX_POINTS) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %llu points in one call (limit 2^24)", who, (unsigned long long) n);
  if (const int e = freespace_layer(msg, who, have_layer, pending, shard_count)) return e;
  if (p->reserved[0] || p->reserved[1]) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  mrh::RayCam& rc = out->cam;
  rc.ifx = rc.ify = rc.cx = rc.cy = 0.f;
  rc.rows = rc.cols = 0;
  if (depth_form) {
    if (p->rows < 1 || p->rows > MRH_RAYCAST_MAX_SIDE || p->cols < 1 || p->cols > MRH_RAYCAST_MAX_SIDE)
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: image of %d x %d pixels (1 .. %d per side)", who, p->rows, p->cols, MRH_RAYCAST_MAX_SIDE);
    if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || p->fx == 0.f || p->fy == 0.f || !std::isfinite(p->cx) || !std::isfinite(p->cy))
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: bad intrinsics", who);
    rc.ifx = 1.0f / p->fx; rc.ify = 1.0f / p->fy;
    rc.cx = p->cx; rc.cy = p->cy;
    rc.rows = p->rows; rc.cols = p->cols;
  }
  if (!(p->min_depth >= 0.f) || !(p->max_depth > p->min_depth) || !std::isfinite(p->max_depth))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: need 0 <= min_depth < max_depth (got %g, %g)", who, (double) p->min_depth, (double) p->max_depth);
  if (!(p->margin >= 0.f) || !std::isfinite(p->margin)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: margin %g", who, (double) p->margin);
  const float step = p->step == 0.f ? freespace_half_cell(voxel_size, shift) : p->step;
  if (!(step > 0.f) || !std::isfinite(step)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the sample spacing must be > 0 (step %g)", who, (double) step);
  if (const int e = finite_pose(msg, who, R, t)) return e;
  const uint32_t n_samples = ray_sample_count(p->min_depth, p->max_depth, step);
  if (!n_samples)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: more than 2^20 samples per ray (min_depth %g, max_depth %g, step %g)", who, (double) p->min_depth,
                  (double) p->max_depth, (double) step);
  rc.min_depth = p->min_depth; rc.max_depth = p->max_depth; rc.step = step;
  rc.n_samples = n_samples;
  for (int i = 0; i < 9; i++) rc.R[i] = R[i];
  for (int i = 0; i < 3; i++) rc.t[i] = t[i];
  out->n = depth_form ? 0u : (uint32_t) n;
  out->margin = p->margin;
  out->bound = (float) (1 << 20) * voxel_size;
  return MRH_OK;
}
static_assert(MRH_FREESPACE_MAX_SAMPLES == MRH_RAYCAST_MAX_SAMPLES, "one sample count serves the render and the carves");

// the arguments both box readers share; fills the kernels' box.  have_out: the required output was given.  The order: null argument
// -> pending, sharded, no layer -> reserved words -> dims per axis, the voxel span per axis -> surface_band -> min_weight
inline int freespace_box(char* msg, const char* who, const mrh_freespace_box_params* p, const bool have_out, const bool have_layer, const int shift,
                         const int min_weight_threshold, const int pending, const int shard_count, mrh::FreeBox* out) {
  if (!p || !have_out) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (const int e = freespace_layer(msg, who, have_layer, pending, shard_count)) return e;
  if (p->reserved[0] || p->reserved[1]) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  for (int a = 0; a < 3; a++) {
    if (p->dims[a] < 1 || p->dims[a] > MRH_FREESPACE_BOX_MAX_SIDE)
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: box of %d x %d x %d cells (1 .. %d per side)", who, p->dims[0], p->dims[1], p->dims[2], MRH_FREESPACE_BOX_MAX_SIDE);
    const int64_t lo = (int64_t) p->origin[a] * (1ll << shift), hi = ((int64_t) p->origin[a] + p->dims[a]) * (1ll << shift) - 1;
    if (lo < -(1ll << 23) || hi >= (1ll << 23))
      return refuse(msg, MRH_ERR_INVALID_ARG, "%s: axis %d of the box spans voxels %lld .. %lld, outside [-2^23, 2^23)", who, a, (long long) lo, (long long) hi);
  }
  if (!std::isfinite(p->surface_band) || p->surface_band < 0.f) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: surface_band %g", who, (double) p->surface_band);
  if (p->min_weight < 0) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: min_weight %d", who, p->min_weight);
  out->ox = p->origin[0]; out->oy = p->origin[1]; out->oz = p->origin[2];
  out->nx = p->dims[0]; out->ny = p->dims[1]; out->nz = p->dims[2];
  mrh::EsdfBox& v = out->vox;
  v.ox = p->origin[0] * (1 << shift); v.oy = p->origin[1] * (1 << shift); v.oz = p->origin[2] * (1 << shift);
  v.nx = p->dims[0] << shift; v.ny = p->dims[1] << shift; v.nz = p->dims[2] << shift;
  v.reach = 0;
  v.w_min = std::max(1, p->min_weight ? p->min_weight : min_weight_threshold);
  v.band = p->surface_band;
  return MRH_OK;
}

// the arguments both segment calls share.  have_in: both endpoint lists were given (n == 0 needs none); have_out: the required
// output was (the blocking call has none: true).  The order: null argument -> pending, sharded, no layer -> n -> step
inline int freespace_segments(char* msg, const char* who, const bool have_in, const bool have_out, const uint64_t n, const float step_in, const bool have_layer,
                              const float voxel_size, const int shift, const int pending, const int shard_count, mrh::SegArgs* out) {
  if ((!have_in && n != 0) || !have_out) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (const int e = freespace_layer(msg, who, have_layer, pending, shard_count)) return e;
  if (n > (uint64_t) MRH_FREESPACE_MAX_POINTS) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %llu segments in one call (limit 2^24)", who, (unsigned long long) n);
  const float step = step_in == 0.f ? freespace_half_cell(voxel_size, shift) : step_in;
  if (!(step > 0.f) || !std::isfinite(step)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the sample spacing must be > 0 (step %g)", who, (double) step);
  out->n = (uint32_t) n;
  out->step = step;
  out->bound = (float) (1 << 20) * voxel_size;
  return MRH_OK;
}

// ---- map-to-map fusion (include/mrhash_remap.h) ----

constexpr uint64_t kRemapMaxEntries = 0x7FFFFFFFull;  // candidate slots and records of one call: what mrh_unpack_blocks takes, and 32-bit indices
constexpr uint64_t kRemapRecordBytes = 6160;          // sizeof(mrh_block_record)
constexpr double kRemapRotationTol = 1.0 / 1024.0;    // |R R^T - I| per entry

// a pose (R, t) that is finite and whose R is a rotation or a reflection: |R R^T - I| <= 2^-10 in every entry
inline int rigid_pose(char* msg, const char* who, const float* R, const float* t) {
  if (const int e = finite_pose(msg, who, R, t)) return e;
  double worst = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double g = 0.0;
      for (int k = 0; k < 3; k++) g += (double) R[3 * i + k] * (double) R[3 * j + k];
      worst = std::fmax(worst, std::fabs(g - (i == j ? 1.0 : 0.0)));
    }
  if (!(worst <= kRemapRotationTol)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: R is not a rotation (|R R^T - I| reaches %g)", who, worst);
  return MRH_OK;
}

// Destination blocks per axis that the candidate box of ONE source block can meet, ratio = vs_d / vs_s.  The box
// is the axis-aligned bound of the block's cube, transformed: the cube has 8 source voxels a side and is grown by one on each
// side beyond the shift limit (10), its bound is at most sqrt(3) (1 + 2^-9) times that wide (|R R^T - I| <= 2^-10); the box is
// grown on each side by one destination voxel, and by the rounding allowance of at most half a destination voxel plus 1.75
// source voxels (k_remap_candidates).  An interval of length L blocks meets at most floor(L) + 2 blocks.
inline int remap_per_axis(const double ratio) {
  const double len = (10.0 * 1.7320508075688774 * (1.0 + 1.0 / 512.0) / ratio + 2.0 * (1.5 + 1.75 / ratio)) / 8.0;
  return (int) std::floor(len) + 2;
}

// the arguments mrh_resample_map and mrh_fuse_map share; fills the kernels' arguments.  have_out: the required out-pointers were
// given (mrh_fuse_map has none: true).  src_*: the source context's voxel size, pending exchange and shard count.  fuse: the
// call has a destination — same_ctx (dst == src), same_device, and dst_*: the destination's
inline int remap(char* msg, const char* who, const mrh_remap_params* p, const float* R, const float* t, const bool have_out, const float src_vs,
                 const int src_pending, const int src_shards, const bool fuse, const bool same_ctx, const bool same_device, const float dst_vs,
                 const int dst_pending, const int dst_shards, mrh::RemapArgs* out) {
  if (!p || !R || !t || !have_out) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (fuse && same_ctx) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the destination is the source", who);
  if (fuse && !same_device) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the two contexts are on different devices", who);
  if (const int e = whole_map(msg, who, "are not resampled", src_pending, src_shards)) return e;
  if (fuse)
    if (const int e = whole_map(msg, who, "take no resampled map", dst_pending, dst_shards)) return e;
  if (p->reserved[0] || p->reserved[1]) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  if (p->min_weight > 255u) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: min_weight %u (0 .. 255)", who, p->min_weight);
  if (const int e = rigid_pose(msg, who, R, t)) return e;
  if (!std::isfinite(p->dst_voxel_size) || p->dst_voxel_size < 0.f) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: dst_voxel_size %g", who, (double) p->dst_voxel_size);
  if (fuse && p->dst_voxel_size != 0.f && p->dst_voxel_size != dst_vs)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: dst_voxel_size %g contradicts the destination's %g", who, (double) p->dst_voxel_size, (double) dst_vs);
  const float vs_d = fuse ? dst_vs : (p->dst_voxel_size == 0.f ? src_vs : p->dst_voxel_size);
  const double ratio = (double) vs_d / (double) src_vs;
  if (!(ratio >= 0.25 && ratio <= 4.0))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: voxel sizes %g (destination) and %g (source): the ratio must lie in [1/4, 4]", who, (double) vs_d, (double) src_vs);
  // (R^T)^-1 = cof(R^T) / det = cof(R)^T / det, in binary64.  |det| >= 0.99 under the rotation test
  const double a = R[0], b = R[1], c = R[2], d = R[3], e = R[4], f = R[5], g = R[6], h = R[7], i = R[8];
  const double cof[9] = {e * i - f * h, f * g - d * i, d * h - e * g, c * h - b * i, a * i - c * g, b * g - a * h, b * f - c * e, c * d - a * f, a * e - b * d};
  const double det = a * cof[0] + b * cof[1] + c * cof[2];
  // inverse(M)_ij = cof(M)_ji / det; for M = R^T, cof(M) = cof(R)^T, so inverse(R^T)_ij = cof(R)_ij / det
  for (int k = 0; k < 9; k++) out->F[k] = cof[k] / det;
  for (int k = 0; k < 9; k++) out->R[k] = R[k];
  for (int k = 0; k < 3; k++) out->t[k] = t[k];
  out->vs_d = vs_d;
  out->bound = (float) (1 << 20) * src_vs;
  out->w_min = p->min_weight > 1u ? p->min_weight : 1u;
  out->per_axis = remap_per_axis(ratio);
  return MRH_OK;
}

// candidate slots of a call over n_src live source blocks: per_axis^3 each, at most 2^31 - 1 in all
inline int remap_slots(char* msg, const char* who, const uint64_t n_src, const int per_axis, uint64_t* slots) {
  const uint64_t each = (uint64_t) per_axis * (uint64_t) per_axis * (uint64_t) per_axis;
  if (per_axis < 1 || per_axis > 64 || n_src > kRemapMaxEntries || n_src * each > kRemapMaxEntries)
    return refuse(msg, MRH_ERR_CAPACITY, "%s: %llu source blocks with %llu candidate slots each (limit 2^31 - 1 slots)", who, (unsigned long long) n_src, (unsigned long long) each);
  *slots = n_src * each;
  return MRH_OK;
}

// bytes of n records, at most 2^31 - 1 of them
inline int remap_record_bytes(char* msg, const char* who, const uint64_t n, uint64_t* bytes) {
  if (n > kRemapMaxEntries) return refuse(msg, MRH_ERR_CAPACITY, "%s: %llu records in one call (limit 2^31 - 1)", who, (unsigned long long) n);
  *bytes = n * kRemapRecordBytes;  // < 2^31 * 2^13: no overflow
  return MRH_OK;
}

// ---- map-to-map registration (include/mrhash_align.h) ----

// One registration call with its defaults filled in
struct Align {
  float band, dist_max;
  int iterations;
  uint32_t min_samples, w_min;
  bool crop;               // the caller gave pivot and extent
  float pivot[3], extent;  // the caller's when crop, else zeros until align_auto_pivot
};
// have_out: both pose outputs were given.  same_ctx: dst == src.  *_truncation: the contexts' sdf_truncation, for the default
// band.  The order: null argument -> dst == src -> devices -> pending, sharded (source, then destination) -> reserved words ->
// min_weight -> band -> dist_max -> iterations -> pivot -> extent -> the pose
inline int align(char* msg, const char* who, const mrh_align_params* p, const float* R, const float* t, const bool have_out, const bool same_ctx,
                 const bool same_device, const float src_truncation, const int src_pending, const int src_shards, const float dst_truncation,
                 const int dst_pending, const int dst_shards, Align* out) {
  if (!p || !R || !t || !have_out) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (same_ctx) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the destination is the source", who);
  if (!same_device) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the two contexts are on different devices", who);
  if (const int e = whole_map(msg, who, "are not aligned", src_pending, src_shards)) return e;
  if (const int e = whole_map(msg, who, "are not aligned to", dst_pending, dst_shards)) return e;
  if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: a reserved word is not 0", who);
  if (p->min_weight > 255u) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: min_weight %u (0 .. 255)", who, p->min_weight);
  out->band = p->band == 0.f ? std::fmin(src_truncation, dst_truncation) : p->band;
  if (!(out->band > 0.f && out->band <= 1.f)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the band must lie in (0, 1] m (band %g)", who, (double) out->band);
  out->dist_max = p->dist_max == 0.f ? std::fmin(out->band, 1.f) : p->dist_max;
  if (!(out->dist_max > 0.f && out->dist_max <= 1.f))
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the gate must lie in (0, 1] m (dist_max %g)", who, (double) out->dist_max);
  if (p->iterations < 0 || p->iterations > MRH_ALIGN_MAX_ITERATIONS)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: %d iterations (1 .. %d, 0 = 10)", who, p->iterations, MRH_ALIGN_MAX_ITERATIONS);
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(p->pivot[i])) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: pivot is not finite", who);
  if (!std::isfinite(2.0f * p->extent) || p->extent < 0.f) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: extent %g", who, (double) p->extent);  // 2 extent: the lever
  if (const int e = rigid_pose(msg, who, R, t)) return e;
  out->iterations = p->iterations ? p->iterations : 10;
  out->min_samples = p->min_samples ? p->min_samples : 64u;
  out->w_min = p->min_weight > 1u ? p->min_weight : 1u;
  out->crop = p->extent > 0.f;
  for (int i = 0; i < 3; i++) out->pivot[i] = out->crop ? p->pivot[i] : 0.f;
  out->extent = p->extent;
  return MRH_OK;
}

// the sample list of one call: at most 2^26 entries of 16 bytes (the bounds of the 64-bit sums, mrhash_align.h)
inline int align_sample_bytes(char* msg, const char* who, const uint64_t n, uint64_t* bytes) {
  if (n > (uint64_t) MRH_ALIGN_MAX_SAMPLES) return refuse(msg, MRH_ERR_CAPACITY, "%s: %llu source samples in one call (limit 2^26)", who, (unsigned long long) n);
  *bytes = n * 16ull;
  return MRH_OK;
}

// the automatic pivot and extent from the integer box lo, hi of the accepted voxel coordinates (D19)
inline void align_auto_pivot(const int lo[3], const int hi[3], const float vs_s, float c[3], float* extent) {
  int64_t half = 0;
  for (int a = 0; a < 3; a++) {
    c[a] = (float) (((int64_t) lo[a] + (int64_t) hi[a]) >> 1) * vs_s;
    half = std::max(half, ((int64_t) hi[a] - (int64_t) lo[a]) / 2);
  }
  *extent = (float) (half + 1) * vs_s;
}

// tau = R c + t and back, binary64, each row ((R_i0 c_x + R_i1 c_y) + R_i2 c_z) (+ t_i | subtracted from tau_i)
inline void align_tau(const double R[9], const float c[3], const double t[3], double tau[3]) {
  for (int i = 0; i < 3; i++) tau[i] = ((R[3 * i] * (double) c[0] + R[3 * i + 1] * (double) c[1]) + R[3 * i + 2] * (double) c[2]) + t[i];
}
inline void align_t(const double R[9], const float c[3], const double tau[3], double t[3]) {
  for (int i = 0; i < 3; i++) t[i] = tau[i] - ((R[3 * i] * (double) c[0] + R[3 * i + 1] * (double) c[1]) + R[3 * i + 2] * (double) c[2]);
}

// the normals' parameter block (null: every default) with its defaults filled in, as the kernels take it.  n: points of the scan;
// voxel_size: the context's virtual_voxel_size, for the default cell side
inline int normals(char* msg, const char* who, const mrh_normals_params* p, const uint64_t n, const float voxel_size, mrh::NrmPar* out) {
  mrh_normals_params q = {0.f, 0u, 0.f, 0.f};
  if (p) q = *p;
  auto bad = [](float v) { return !(v >= 0.f) || !std::isfinite(v); };
  if (bad(q.radius) || bad(q.min_spread) || bad(q.max_flatness) || q.max_flatness >= 1.f)
    return refuse(msg, MRH_ERR_INVALID_ARG, "%s: bad parameter (radius %g, min_spread %g, max_flatness %g)", who, (double) q.radius, (double) q.min_spread, (double) q.max_flatness);
  if (n >= (1ull << 24)) return refuse(msg, MRH_ERR_CAPACITY, "%s: %llu points in one scan (limit 2^24 - 1)", who, (unsigned long long) n);
  out->rho = q.radius == 0.f ? 2.0f * voxel_size : q.radius;
  if (!(out->rho > 0.f) || !std::isfinite(out->rho)) return refuse(msg, MRH_ERR_INVALID_ARG, "%s: the cell side must be > 0 (radius %g)", who, (double) out->rho);
  out->min_points = q.min_points == 0u ? 5u : q.min_points;
  const double spread = 1024.0 * (q.min_spread == 0.f ? 0.0625 : (double) q.min_spread);
  out->min_l1 = spread * spread;
  out->max_flat = q.max_flatness == 0.f ? 0.0625 : (double) q.max_flatness;
  return MRH_OK;
}

}  // namespace
}  // namespace mrh_plan
