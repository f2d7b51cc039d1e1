// mrh_sdftrack.h — render-free tracking: the linearisation of point-to-SDF tracking of a depth frame or a cloud of sensor-frame
// points against the map's own distance field (include/mrhash_sdftrack.h; DESIGN.md §4.15 and D20, which is normative;
// tests/sdftrack_ref.py restates it).  The reference has no tracker: the definition is this project's.  The field is D17's SMOOTH
// field with its analytic gradient (smooth_field, mrh_query.h), the fixed-point step, the sums and their reduction the tracker's
// (track_fix, track_reduce_store, k_track_finish, mrh_track.h), the loop, the solve and the pose update the host's
// (mrh_tracksolve.h); all are used as they stand.  No render: the observation's points are samples of signed distance 0.
//
// k_sdftrack_depth_linearise    one lane per depth pixel on the tracker's tile grid — a wave64 an 8 x 8 tile, a workgroup of four
//                               waves a 16 x 16 tile — so neighbouring lanes back-project to neighbouring surface points and their
//                               eight corners come from the same few blocks.  The back-projection stays in registers: no sample
//                               list is written.
// k_sdftrack_points_linearise   one lane per point, a 1-D grid of 256-lane workgroups, three loads from the caller's [n, 3] buffer
//                               as it lies: no float4 copy.
// Both run steps 1-6 of D20 per lane in registers (binary32, no FMA contraction), call smooth_field with neigh_none as
// k_align_linearise does, and end in track_reduce_store: one row of the partial slab per workgroup.  They only read the map:
// plain vector loads and stores, every loop bounded, no atomics, no scratch.
//
// Bounds of the sums, at most 2^24 samples: |J~| < 2^15, so |J~ J~| < 2^30 and the 21 sums stay below 2^54; |e~| <= 2^18 (|e| = |d| <
// band <= 1), |J~ e~| < 2^33, the 6 sums below 2^57; e~^2 <= 2^36, its sum at most 2^60.  All fit a signed 64-bit word.
#pragma once

#include "mrh_query.h"
#include "mrh_readerplan.h"  // SdfTrackLin
#include "mrh_track.h"

namespace mrh {

constexpr int kSdfTrackLanes = 256;  // four wave64s: what track_reduce_store reduces

// steps 2-6 of D20 for one sample whose rotated sensor-frame position is a = R32 p.  False: rejected.
__device__ __forceinline__ bool sdftrack_sample(const Map& m, const Tab& t, const SdfTrackLin& k, const f3 a, int J[6], int& e_fix) {
  const f3 W = mk3(a.x + k.t[0], a.y + k.t[1], a.z + k.t[2]);
  if (!(fabsf(W.x) < k.bound && fabsf(W.y) < k.bound && fabsf(W.z) < k.bound)) return false;  // NaN and Inf fail; before any conversion
  Neigh nb = neigh_none();
  nb.shift_limit = m.block_shift_limit;
  const float h = get_voxel_size_f(m, t, nb, W);
  float d = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  if (!smooth_field(m, t, nb, W, h, true, d, gx, gy, gz)) return false;
  if (!(fabsf(d) < k.band)) return false;
  const float e = 0.f - d;  // the sample's own distance is 0
  const float Jf[6] = {(a.y * gz - a.z * gy) * k.s_a, (a.z * gx - a.x * gz) * k.s_a, (a.x * gy - a.y * gx) * k.s_a,
                       gx * mrh_track::kJOne, gy * mrh_track::kJOne, gz * mrh_track::kJOne};
  return track_fix(Jf, e, J, e_fix);
}

// the depth form: a 2-D grid of 16 x 16 tiles, the pixel (r, c) as in k_track_linearise
__global__ __launch_bounds__(kSdfTrackLanes) void k_sdftrack_depth_linearise(const Map m, const Tab t, const SdfTrackLin k, const float* __restrict__ depth,
                                                                            i64* __restrict__ slab) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * kRenderTile + (wave & 1) * 8 + (lane & 7);
  const int r = blockIdx.y * kRenderTile + (wave >> 1) * 8 + (lane >> 3);
  int J[6] = {0, 0, 0, 0, 0, 0}, e = 0;
  bool ok = r < k.rows && c < k.cols;
  if (ok) {
    const float D = depth[(size_t) r * (size_t) k.cols + (size_t) c];
    ok = D > k.min_depth && D <= k.max_depth;  // a NaN fails
    if (ok) {
      const float dx = k.ifx * (((float) c - k.cx) - 0.5f), dy = k.ify * (((float) r - k.cy) - 0.5f);
      ok = sdftrack_sample(m, t, k, track_rows(k.R, D * dx, D * dy, D), J, e);
    }
  }
  track_reduce_store(J, e, ok, slab);
}

// the points form: one lane per point, a 1-D grid of ceil(n / 256) workgroups
__global__ __launch_bounds__(kSdfTrackLanes) void k_sdftrack_points_linearise(const Map m, const Tab t, const SdfTrackLin k, const float* __restrict__ pts,
                                                                             i64* __restrict__ slab) {
  const u32 i = blockIdx.x * (u32) kSdfTrackLanes + threadIdx.x;
  int J[6] = {0, 0, 0, 0, 0, 0}, e = 0;
  bool ok = i < k.n;
  if (ok) {
    const float x = pts[3 * (size_t) i + 0], y = pts[3 * (size_t) i + 1], z = pts[3 * (size_t) i + 2];
    const float rp = sqrtf((x * x + y * y) + z * z);
    ok = rp > k.min_depth && rp <= k.max_depth;  // (0, 0, 0), a NaN and an infinity fail
    if (ok) ok = sdftrack_sample(m, t, k, track_rows(k.R, x, y, z), J, e);
  }
  track_reduce_store(J, e, ok, slab);
}

}  // namespace mrh
