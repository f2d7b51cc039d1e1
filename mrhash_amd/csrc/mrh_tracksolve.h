// mrh_tracksolve.h — the host half of every pose fit (tracking, include/mrhash_track.h; map-to-map registration,
// include/mrhash_align.h, D19): the fixed-point scale, the binary64 Cholesky solve of the 6 x 6 normal equations from the 29 exact
// integer sums, the pose update, and the Gauss-Newton loop around them (Fit, fit_run, fit_report) with the linearisation as the
// caller's callable.  Plain C++, no HIP, no context: mrh_readers.h runs it with callables that launch kernels, tests/host/
// track_solve_check.cpp compiles it on its own and replays recorded sums.  Built with -ffp-contract=off like everything else:
// every product and every sum below rounds once, in the order written (tests/track_ref.py restates it).
#pragma once

#include <cmath>
#include <cstdint>

namespace mrh_track {

constexpr int kSumWords = 32;  // 21 of the upper triangle of sum J J^T (row-major), 6 of sum J e, sum e^2, n, three zeros
constexpr int kSumB = 21, kSumEE = 27, kSumN = 28;
constexpr float kJOne = 16384.0f;   // fixed-point scale of the normal part of a row (2^14)
constexpr float kEOne = 262144.0f;  // ... of the residual (2^18)

// S_a = 16384 / L, L the smallest power of two >= 2 * max_depth: the lever arm |a| of a pixel is below sqrt(3) max_depth in
// practice and any row with |a x N| S_a >= 2^15 is rejected by the kernel
inline float angle_scale(const float max_depth) {
  const float two_d = 2.0f * max_depth;
  float L = 1.0f;
  while (L < two_d) L = L * 2.0f;
  while (L * 0.5f >= two_d) L = L * 0.5f;
  return kJOne / L;
}

// xi = (omega, v).  False: lost (too few pixels, or a pivot that is not finite or not above 2^-20 of its diagonal entry)
inline bool solve(const int64_t sums[kSumWords], const float s_a, const uint32_t min_pixels, double xi[6]) {
  if (sums[kSumN] < (int64_t) min_pixels) return false;
  const double s[6] = {(double) s_a, (double) s_a, (double) s_a, (double) kJOne, (double) kJOne, (double) kJOne};
  double H[6][6], b[6], L[6][6] = {};
  int k = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) H[i][j] = H[j][i] = (double) sums[k++] / (s[i] * s[j]);
  for (int i = 0; i < 6; i++) b[i] = (double) sums[kSumB + i] / (s[i] * (double) kEOne);
  for (int j = 0; j < 6; j++) {
    double d = H[j][j];
    for (int q = 0; q < j; q++) d = d - L[j][q] * L[j][q];
    if (!(std::isfinite(d) && d > H[j][j] * 0x1p-20)) return false;
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < 6; i++) {
      double acc = H[i][j];
      for (int q = 0; q < j; q++) acc = acc - L[i][q] * L[j][q];
      L[i][j] = acc / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double acc = b[i];
    for (int q = 0; q < i; q++) acc = acc - L[i][q] * y[q];
    y[i] = acc / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double acc = y[i];
    for (int q = i + 1; q < 6; q++) acc = acc - L[q][i] * xi[q];
    xi[i] = acc / L[i][i];
  }
  return true;
}

// (R, t) <- (dR R, t + v): dR is the rotation matrix of the unit quaternion (omega / 2, 1) / |.|, by the formula of pose_from
// (geowrapper.cpp) in binary64; no trigonometric function
inline void update(double R[9], double t[3], const double xi[6]) {
  const double hx = xi[0] / 2.0, hy = xi[1] / 2.0, hz = xi[2] / 2.0;
  const double nu = std::sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0);
  const double x = hx / nu, y = hy / nu, z = hz / nu, w = 1.0 / nu;
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double dR[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)};
  double Rn[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rn[3 * i + j] = (dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j];
  for (int i = 0; i < 9; i++) R[i] = Rn[i];
  for (int i = 0; i < 3; i++) t[i] = t[i] + xi[3 + i];
}

// rms of the point-to-plane residual over the accepted pixels, metres
inline double rms(const int64_t sums[kSumWords]) {
  return sums[kSumN] > 0 ? std::sqrt((double) sums[kSumEE] / (double) sums[kSumN]) / (double) kEOne : 0.0;
}

// ---- the loop (D14 "Loop"; D15 and D19 by reference) ----------------------------------------------------------------------------
constexpr int kFitOk = 0, kFitLost = 1;  // the value of MRH_TRACK_OK / _LOST and of MRH_ALIGN_OK / _LOST (mrh_readers.h asserts it)
// What a fit owns: the pose in binary64, the sums of the last linearisation, the status and the number of updates applied.  A
// fit that is never run — an empty observation — stays lost, with zero sums and the start pose
struct Fit {
  double R[9], t[3];
  int64_t sums[kSumWords] = {};
  int status = kFitLost, done = 0;
  Fit(const float R0[9], const float t0[3]) {
    for (int i = 0; i < 9; i++) R[i] = (double) R0[i];
    for (int i = 0; i < 3; i++) t[i] = (double) t0[i];
  }
};

// `iterations` steps on f.  linearise(R32, t32, sums) takes the linearisation at (float) of the state and fills the 32 sums, or
// returns a negative error, which ends the loop and is returned as it is.  A step that solve refuses ends the loop as lost: the
// pose is the one from before that step, f.done its index, f.sums its sums.  Returns f.status otherwise: OK after the last update
template <typename Linearise>
inline int fit_run(Fit& f, const int iterations, const float s_a, const uint32_t min_count, Linearise&& linearise) {
  for (int it = 0; it < iterations; it++) {
    float R32[9], t32[3];
    for (int i = 0; i < 9; i++) R32[i] = (float) f.R[i];
    for (int i = 0; i < 3; i++) t32[i] = (float) f.t[i];
    const int e = linearise(R32, t32, f.sums);
    if (e < 0) return e;
    double xi[6];
    if (!solve(f.sums, s_a, min_count, xi)) return f.status = kFitLost;
    update(f.R, f.t, xi);
    f.done++;
  }
  return f.status = kFitOk;
}

// What a call reports of a fit: the pose narrowed to binary32 and, into the caller's info struct (null: not wanted), status,
// updates, rms and sums under the names mrh_track_info and mrh_align_info share; `count` is the struct's field for n
template <typename Info>
inline void fit_report(const Fit& f, float out_R[9], float out_t[3], Info* info, uint64_t Info::*count) {
  for (int i = 0; i < 9; i++) out_R[i] = (float) f.R[i];
  for (int i = 0; i < 3; i++) out_t[i] = (float) f.t[i];
  if (!info) return;
  info->status = f.status;
  info->iterations_done = f.done;
  info->*count = (uint64_t) f.sums[kSumN];
  info->rms = rms(f.sums);
  for (int i = 0; i < kSumWords; i++) info->sums[i] = f.sums[i];
}

}  // namespace mrh_track
