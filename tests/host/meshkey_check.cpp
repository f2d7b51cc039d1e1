// meshkey_check.cpp — mrh::mesh_cell (mrhash_amd/csrc/mrh_meshkey.h), the cell index of the vertex merge, on its own: a plain
// C++17 program that includes the header alone, for tests/test_mesh_soups.py (g++, ASan + UBSan + -fsanitize=float-cast-overflow:
// a conversion outside the int range anywhere in mesh_cell is reported).
//
// Checked: both ends of the int range and the doubles next to them on either side, +-inf, NaN, +-0, +-0.5, the largest and the
// smallest doubles; inside the range, mesh_cell against the plain conversion; the coordinates of the soup out_of_range
// (tests/mesh_soups.py: eps = 1e-9, +-3.0 -> INT32_MIN) through floor(p * inv_eps) as the callers compute it.
// stdout: one line per failure, then "meshkey_check: <n> failures".
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "mrh_meshkey.h"

namespace {

int failures = 0;

void expect(const double x, const int32_t want) {
  const int32_t got = mrh::mesh_cell(x);
  if (got == want) return;
  failures++;
  printf("FAILED mesh_cell(%.17g) = %d, expected %d\n", x, (int) got, (int) want);
}

}  // namespace

int main() {
  const double two31 = 2147483648.0, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // the upper end: 2^31 is out, the double below it is in (and truncates to INT32_MAX)
  expect(two31, INT32_MIN);
  expect(std::nextafter(two31, inf), INT32_MIN);
  expect(std::nextafter(two31, 0.0), INT32_MAX);
  expect(two31 - 1.0, INT32_MAX);
  // the lower end: -2^31 is in, the double below it is out
  expect(-two31, INT32_MIN);
  expect(std::nextafter(-two31, 0.0), INT32_MIN + 1);  // -2147483647.9999995 truncates towards zero
  expect(-two31 + 1.0, INT32_MIN + 1);
  expect(std::nextafter(-two31, -inf), INT32_MIN);
  expect(-two31 - 1.0, INT32_MIN);
  // no number at all
  expect(inf, INT32_MIN);
  expect(-inf, INT32_MIN);
  expect(nan, INT32_MIN);
  expect(-nan, INT32_MIN);
  expect(std::numeric_limits<double>::max(), INT32_MIN);
  expect(-std::numeric_limits<double>::max(), INT32_MIN);
  // around zero
  expect(0.0, 0);
  expect(-0.0, 0);
  expect(0.5, 0);
  expect(-0.5, 0);  // the conversion truncates; the callers floor first (floor(-0.5) = -1)
  expect(std::floor(-0.5), -1);
  expect(std::numeric_limits<double>::denorm_min(), 0);
  expect(-std::numeric_limits<double>::denorm_min(), 0);
  // inside the range: the plain conversion, for integral and other values on a ladder of magnitudes
  for (int e = 0; e <= 30; e++)
    for (const double f : {1.0, 1.25, 1.5, 1.999999}) {
      const double x = std::ldexp(f, e);
      if (x >= two31) continue;
      expect(x, (int32_t) x);
      expect(-x, (int32_t) -x);
      expect(std::floor(x), (int32_t) std::floor(x));
      expect(std::floor(-x), (int32_t) std::floor(-x));
    }
  // as the callers compute it: eps = 1e-9f
  const double eps = (double) 1e-9f, inv_eps = 1.0 / eps;
  expect(std::floor(3.0 * inv_eps), INT32_MIN);
  expect(std::floor(-3.0 * inv_eps), INT32_MIN);
  expect(std::floor(2.5 * inv_eps), INT32_MIN);
  expect(std::floor(-2.5 * inv_eps), INT32_MIN);
  expect(std::floor((double) std::numeric_limits<float>::infinity() * inv_eps), INT32_MIN);
  expect(std::floor(-(double) std::numeric_limits<float>::infinity() * inv_eps), INT32_MIN);
  const double two = std::floor(2.0 * inv_eps), minus_two = std::floor(-2.0 * inv_eps);
  if (!(two < two31 && minus_two >= -two31)) { failures++; printf("FAILED 2.0 / 1e-9f is expected inside the int range (%.17g)\n", two); }
  expect(two, (int32_t) two);
  expect(minus_two, (int32_t) minus_two);
  printf("meshkey_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
