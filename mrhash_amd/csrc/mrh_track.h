// mrh_track.h — depth-frame and scan tracking against the raycast map: the linearisation of point-to-plane ICP (include/mrhash_track.h;
// DESIGN.md §4.9 and D14, which is normative; tests/track_ref.py restates it).  The reference has no tracker: the definition is
// this project's.  The model images come from k_raycast<false> (mrh_raycast.h), unchanged; the loop, the solve and the pose update
// are the host's (mrh_tracksolve.h).  Map-to-map registration (mrh_align.h) reuses track_fix, track_reduce_store and k_track_finish.
//
// k_track_linearise: one lane per depth pixel, a wave64 an 8 x 8 tile and a workgroup of four waves a 16 x 16 tile as in k_raycast,
// so that the gathers from the model images stay within a few rows of a few tiles.  Steps 1-8 of D14 run per lane in registers
// (binary32, no FMA contraction) and end in a fixed-point row J~ (6 x int, |J~| <= 2^15) and residual e~ (|e~| <= 2^18 + 1 for the
// render's normals, which are unit vectors or zero, and |delta| <= dist_max <= 1).  A lane whose pixel is rejected contributes zeros.
//
// The sums are exact integers, so their value does not depend on the shape of the reduction.  Bounds, with at most 2^24 pixels
// (MRH_RAYCAST_MAX_SIDE^2): |J~ J~| <= 2^30 per pixel, the 21 sums of J~ J~^T stay below 2^54; |J~ e~| < 2^34, the 6 sums of J~ e~
// below 2^58; e~^2 < 2^37, its sum below 2^61; n <= 2^24.  All fit a signed 64-bit word.
//
// Reduction: the 29 values (padded to 32) are reduced across the wave by a transposing butterfly — in step s a lane keeps one half of
// its values and sends the other half to lane ^ (1 << s), so the five steps move 16 + 8 + 4 + 2 + 1 64-bit words per lane instead
// of 5 x 32, and leave word bitrev5(lane & 31) summed over each half of the wave; one more exchange adds the halves.  The four
// waves meet in 1 KiB of LDS and every workgroup writes one row of 32 words into the partial slab with plain vector stores: no
// atomics of any kind (29 shared words under one 64-bit atomic per workgroup each are the contended shape), no scratch.
// k_track_finish, one workgroup, sums the slab's rows into the 32 words the host reads from pinned memory.
//
// k_track_scan_linearise (tests/track_scan_ref.py): the same for a LiDAR scan — one lane per sensor-frame
// point, a 1-D grid of 256-lane workgroups — against the range, normals and points images of k_raycast<true>.  Steps 6-8
// (track_row) and the reduction (track_reduce_store) are shared with the depth kernel; n <= 2^24 points keeps the bounds above.
#pragma once

#include "mrh_raycast.h"
#include "mrh_tracksolve.h"

namespace mrh {

typedef long long i64;

struct TrackLin {
  float fx, fy, cx, cy, ifx, ify;  // ifx = 1 / fx, ify = 1 / fy (host, IEEE)
  int rows, cols;
  float min_depth, max_depth;
  float dmax2;       // dist_max * dist_max (binary32)
  float s_a;         // mrh_track::angle_scale(max_depth)
  float Rr[9], tr[3];  // the pose the model was rendered from
  float R[9], t[3];    // the estimate this linearisation is taken at
};

__device__ __forceinline__ f3 track_rows(const float* M, const float x, const float y, const float z) {  // (M_i0 x + M_i1 y) + M_i2 z
  return mk3((M[0] * x + M[1] * y) + M[2] * z, (M[3] * x + M[4] * y) + M[5] * z, (M[6] * x + M[7] * y) + M[8] * z);
}

// the fixed-point step (D14 step 8, D19 step 7: align_sample, mrh_align.h): the row and the residual to integers.  False: |Jf_i| >= 2^15
__device__ __forceinline__ bool track_fix(const float Jf[6], const float e, int J[6], int& e_fix) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (!(fabsf(Jf[i]) < 32768.0f)) return false;  // a NaN is rejected
#pragma unroll
  for (int i = 0; i < 6; ++i) J[i] = (int) rintf(Jf[i]);
  e_fix = (int) rintf(e * mrh_track::kEOne);
  return true;
}

// steps 6-8 of D14, shared by the depth image and the scan (D15): the gate, the residual and the fixed-point row.  False: rejected.
__device__ __forceinline__ bool track_row(const TrackLin& k, const f3 a, const f3 pw, const f3 V, const f3 N, int J[6], int& e_fix) {
  const f3 dl = mk3(V.x - pw.x, V.y - pw.y, V.z - pw.z);
  if (!((dl.x * dl.x + dl.y * dl.y) + dl.z * dl.z <= k.dmax2)) return false;  // a NaN is rejected
  const float e = (N.x * dl.x + N.y * dl.y) + N.z * dl.z;
  const float Jf[6] = {(a.y * N.z - a.z * N.y) * k.s_a, (a.z * N.x - a.x * N.z) * k.s_a, (a.x * N.y - a.y * N.x) * k.s_a,
                       N.x * mrh_track::kJOne, N.y * mrh_track::kJOne, N.z * mrh_track::kJOne};
  return track_fix(Jf, e, J, e_fix);
}

// steps 1-8 of D14 for the pixel (r, c), which lies inside the image.  False: rejected.
__device__ __forceinline__ bool track_pixel(const TrackLin& k, const float* __restrict__ depth, const float* __restrict__ Md, const float* __restrict__ Mn,
                                            const int r, const int c, int J[6], int& e_fix) {
  const float D = depth[(size_t) r * (size_t) k.cols + (size_t) c];
  if (!(D > k.min_depth && D <= k.max_depth)) return false;  // a NaN fails
  const float dx = k.ifx * (((float) c - k.cx) - 0.5f), dy = k.ify * (((float) r - k.cy) - 0.5f);
  const f3 a = track_rows(k.R, D * dx, D * dy, D);
  const f3 pw = mk3(a.x + k.t[0], a.y + k.t[1], a.z + k.t[2]);
  const f3 w = mk3(pw.x - k.tr[0], pw.y - k.tr[1], pw.z - k.tr[2]);
  const float qx = (k.Rr[0] * w.x + k.Rr[3] * w.y) + k.Rr[6] * w.z;  // R_r^T w
  const float qy = (k.Rr[1] * w.x + k.Rr[4] * w.y) + k.Rr[7] * w.z;
  const float qz = (k.Rr[2] * w.x + k.Rr[5] * w.y) + k.Rr[8] * w.z;
  if (!(qz > k.min_depth)) return false;
  const float u = (k.fx * (qx / qz) + k.cx) + 1.0f, v = (k.fy * (qy / qz) + k.cy) + 1.0f;
  if (!(u >= 0.f && u < (float) k.cols && v >= 0.f && v < (float) k.rows)) return false;  // in float, before any conversion
  const int c2 = (int) floorf(u), r2 = (int) floorf(v);  // 0 .. cols - 1, 0 .. rows - 1 by the test above
  const size_t pix = (size_t) r2 * (size_t) k.cols + (size_t) c2;
  const float m = Md[pix];
  if (m == 0.f) return false;
  const float ex = k.ifx * (((float) c2 - k.cx) - 0.5f), ey = k.ify * (((float) r2 - k.cy) - 0.5f);
  const f3 g = track_rows(k.Rr, ex, ey, 1.f);
  const f3 V = mk3(k.tr[0] + m * g.x, k.tr[1] + m * g.y, k.tr[2] + m * g.z);
  const f3 N = mk3(Mn[3 * pix + 0], Mn[3 * pix + 1], Mn[3 * pix + 2]);
  return track_row(k, a, pw, V, N, J, e_fix);
}

// steps 1-8 of D15 for point i of the cloud (i < n).  Mr, Mn, Mp: range, world-frame normals and sensor-frame points of the
// spherical render from (Rr, tr); k.fx .. k.cy, rows, cols are that render's.  False: rejected.
__device__ __forceinline__ bool track_point(const TrackLin& k, const float* __restrict__ pts, const float* __restrict__ Mr, const float* __restrict__ Mn,
                                            const float* __restrict__ Mp, const size_t i, int J[6], int& e_fix) {
  const float x = pts[3 * i + 0], y = pts[3 * i + 1], z = pts[3 * i + 2];
  const float rp = sqrtf((x * x + y * y) + z * z);
  if (!(rp > k.min_depth && rp <= k.max_depth)) return false;  // (0, 0, 0), a NaN and an infinity fail
  const f3 a = track_rows(k.R, x, y, z);
  const f3 pw = mk3(a.x + k.t[0], a.y + k.t[1], a.z + k.t[2]);
  const f3 w = mk3(pw.x - k.tr[0], pw.y - k.tr[1], pw.z - k.tr[2]);
  const float qx = (k.Rr[0] * w.x + k.Rr[3] * w.y) + k.Rr[6] * w.z;  // R_r^T w
  const float qy = (k.Rr[1] * w.x + k.Rr[4] * w.y) + k.Rr[7] * w.z;
  const float qz = (k.Rr[2] * w.x + k.Rr[5] * w.y) + k.Rr[8] * w.z;
  const float rq = sqrtf((qx * qx + qy * qy) + qz * qz);
  if (!(rq > k.min_depth && rq <= k.max_depth)) return false;
  const float az = mrh_atan2f(qy, qx), el = mrh_asinf(qz / rq);  // project_point_m's expressions
  const float u = (k.fx * az + k.cx) + 1.0f, v = (k.fy * el + k.cy) + 1.0f;
  if (!(u >= 0.f && u < (float) k.cols && v >= 0.f && v < (float) k.rows)) return false;  // in float, before any conversion
  const int c2 = (int) floorf(u), r2 = (int) floorf(v);  // 0 .. cols - 1, 0 .. rows - 1 by the test above
  const size_t pix = (size_t) r2 * (size_t) k.cols + (size_t) c2;
  if (Mr[pix] == 0.f) return false;
  const f3 N = mk3(Mn[3 * pix + 0], Mn[3 * pix + 1], Mn[3 * pix + 2]);
  if (N.x == 0.f && N.y == 0.f && N.z == 0.f) return false;  // a hit without a gradient: no row, and no count
  const f3 g = track_rows(k.Rr, Mp[3 * pix + 0], Mp[3 * pix + 1], Mp[3 * pix + 2]);
  const f3 V = mk3(k.tr[0] + g.x, k.tr[1] + g.y, k.tr[2] + g.z);
  return track_row(k, a, pw, V, N, J, e_fix);
}

__device__ __forceinline__ i64 track_xor64(const i64 v, const int mask) {
  const int lo = __shfl_xor((int) (v & 0xFFFFFFFFll), mask), hi = __shfl_xor((int) (v >> 32), mask);
  return (i64) (((unsigned long long) (unsigned) hi << 32) | (unsigned long long) (unsigned) lo);
}

// Step 9 for one workgroup of four waves, every lane of which arrives: the 29 products of the lane's row (zeros unless ok) summed
// over the workgroup into row blockIdx.y * gridDim.x + blockIdx.x of the slab (32 words per row).
__device__ __forceinline__ void track_reduce_store(int J[6], int e, const bool ok, i64* __restrict__ slab) {
  __shared__ i64 part[4][mrh_track::kSumWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = 0;
    e = 0;
  }
  i64 v[mrh_track::kSumWords];
  {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) v[n++] = (i64) J[i] * (i64) J[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[mrh_track::kSumB + i] = (i64) J[i] * (i64) e;
    v[mrh_track::kSumEE] = (i64) e * (i64) e;
    v[mrh_track::kSumN] = ok ? 1 : 0;
    v[29] = v[30] = v[31] = 0;
  }
  // the transposing butterfly: after step s the lane holds 16 >> s words, those whose index bit (4 - s) equals its lane bit s
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int half = 16 >> s;
    const bool up = (lane >> s) & 1;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const i64 send = up ? v[i] : v[i + half], keep = up ? v[i + half] : v[i];
      v[i] = keep + track_xor64(send, 1 << s);
    }
  }
  v[0] += track_xor64(v[0], 32);
  if (lane < 32) part[wave][__brev((unsigned) lane) >> 27] = v[0];
  __syncthreads();
  if (threadIdx.x < mrh_track::kSumWords) {
    const int i = threadIdx.x;
    slab[((size_t) blockIdx.y * gridDim.x + blockIdx.x) * mrh_track::kSumWords + i] = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
  }
}

// the depth image: a 2-D grid of 16 x 16 tiles
__global__ __launch_bounds__(256) void k_track_linearise(const TrackLin k, const float* __restrict__ depth, const float* __restrict__ Md,
                                                         const float* __restrict__ Mn, i64* __restrict__ slab) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * kRenderTile + (wave & 1) * 8 + (lane & 7);
  const int r = blockIdx.y * kRenderTile + (wave >> 1) * 8 + (lane >> 3);
  int J[6] = {0, 0, 0, 0, 0, 0}, e = 0;
  bool ok = r < k.rows && c < k.cols;
  if (ok) ok = track_pixel(k, depth, Md, Mn, r, c, J, e);
  track_reduce_store(J, e, ok, slab);
}

// the scan (D15): one lane per point, a 1-D grid of ceil(n / 256) workgroups; the cloud need not be organised, so the gathers from
// the model images go where the points project
__global__ __launch_bounds__(256) void k_track_scan_linearise(const TrackLin k, const float* __restrict__ pts, const unsigned n, const float* __restrict__ Mr,
                                                              const float* __restrict__ Mn, const float* __restrict__ Mp, i64* __restrict__ slab) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  int J[6] = {0, 0, 0, 0, 0, 0}, e = 0;
  bool ok = i < n;
  if (ok) ok = track_point(k, pts, Mr, Mn, Mp, (size_t) i, J, e);
  track_reduce_store(J, e, ok, slab);
}

// one workgroup of 1024: thread (stripe, word) adds the rows stripe, stripe + 32, ... of its word, the stripes meet in LDS
__global__ __launch_bounds__(1024) void k_track_finish(const i64* __restrict__ slab, const int n_rows, i64* __restrict__ out) {
  __shared__ i64 part[32][mrh_track::kSumWords];
  const int word = threadIdx.x & 31, stripe = threadIdx.x >> 5;
  // a plain loop: eight independent accumulators per thread were measured and dropped (11.5 against 10.2 us per launch at 1 200
  // rows) — the launch, the barrier and the store into host memory are the kernel's time, not the 300 KB it reads
  i64 acc = 0;
  for (int row = stripe; row < n_rows; row += 32) acc += slab[(size_t) row * mrh_track::kSumWords + word];
  part[stripe][word] = acc;
  __syncthreads();
  if (threadIdx.x < mrh_track::kSumWords) {
    i64 sum = 0;
#pragma unroll
    for (int s = 0; s < 32; ++s) sum += part[s][threadIdx.x];
    out[threadIdx.x] = sum;
  }
}

}  // namespace mrh
