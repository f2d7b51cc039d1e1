// gw_pose.h — the pose conversions of the GeoWrapper facade: (t, q) as setCurrPose takes it <-> the row-major 4 x 4 the facade
// keeps <-> (R, t) as the C ABI takes it.  Pure host arithmetic: the standard library only, checked by tests/host/gw_check.cpp.
#pragma once

#include <array>
#include <cmath>

namespace gw {

// Eigen::Quaternionf(qw,qx,qy,qz).toRotationMatrix() (Eigen 3.4.0 Quaternion.h), float arithmetic, no normalisation
inline std::array<float, 16> pose_from(const std::array<float, 3>& t, const std::array<float, 4>& q) {
  const float x = q[0], y = q[1], z = q[2], w = q[3];
  const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  return {1.f - (tyy + tzz), txy - twz, txz + twy, t[0],
          txy + twz, 1.f - (txx + tzz), tyz - twx, t[1],
          txz - twy, tyz + twx, 1.f - (txx + tyy), t[2],
          0.f, 0.f, 0.f, 1.f};
}

// a 4 x 4 row-major pose as the C ABI takes it: the rotation (row-major) and the translation
struct PoseRt { float R[9], t[3]; };
inline PoseRt split_pose(const std::array<float, 16>& T) { return {{T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, {T[3], T[7], T[11]}}; }

// unit quaternion (qx, qy, qz, qw) of a rotation matrix (row-major), by the branch with the largest divisor, normalised; w >= 0.
// The wrapper's own conversion: D14 ends at the matrix.
inline std::array<float, 4> quat_from(const float R[9]) {
  const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7], m22 = R[8];
  double x, y, z, w;
  const double tr = m00 + m11 + m22;
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(tr + 1.0);
    w = 0.25 * s; x = (m21 - m12) / s; y = (m02 - m20) / s; z = (m10 - m01) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = 2.0 * std::sqrt(1.0 + m00 - m11 - m22);
    w = (m21 - m12) / s; x = 0.25 * s; y = (m01 + m10) / s; z = (m02 + m20) / s;
  } else if (m11 > m22) {
    const double s = 2.0 * std::sqrt(1.0 + m11 - m00 - m22);
    w = (m02 - m20) / s; x = (m01 + m10) / s; y = 0.25 * s; z = (m12 + m21) / s;
  } else {
    const double s = 2.0 * std::sqrt(1.0 + m22 - m00 - m11);
    w = (m10 - m01) / s; x = (m02 + m20) / s; y = (m12 + m21) / s; z = 0.25 * s;
  }
  const double n = std::sqrt(x * x + y * y + z * z + w * w) * (w < 0.0 ? -1.0 : 1.0);
  return {(float) (x / n), (float) (y / n), (float) (z / n), (float) (w / n)};
}

}  // namespace gw
