// sdftrackplan_check.cpp — the argument plan of render-free tracking (mrh_plan::sdftrack; mrhash_amd/csrc/mrh_readerplan.h) on its
// own: a plain C++17 program that includes the header alone, for tests/test_sdftrackplan.py (g++ -ffp-contract=off, ASan + UBSan).
//
// Checked: every refusal of include/mrhash_sdftrack.h with its code and, where the C ABI's text is fixed, its message; the order
// null argument -> more than 2^24 points -> pending -> sharded -> reserved word -> (depth form) image shape -> intrinsics -> depth
// range -> band -> iterations -> finite pose; what the points form does not read; the defaults; the 4096 and 2^24 caps and the
// bounds of the 64-bit sums under them.
// stdout: one line per failure, then "sdftrackplan_check: <n> failures".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "mrh_readerplan.h"

namespace {

int failures = 0;
char msg[mrh_plan::kMsgBytes];

void expect(const bool ok, const char* what, const long long a = 0, const long long b = 0) {
  if (ok) return;
  failures++;
  printf("FAILED %s (%lld, %lld) [%s]\n", what, a, b, msg);
}
void expect_msg(const int rc, const int code, const char* text) {
  if (rc == code && !strcmp(msg, text)) return;
  failures++;
  printf("FAILED message: code %d, \"%s\"\n  expected %d, \"%s\"\n", rc, msg, code, text);
}

// 0.7 rad about (1, 2, 3) / sqrt(14), rounded to binary32
const float kR[9] = {0.781639159f, -0.482929289f, 0.394739807f, 0.550117254f, 0.832030118f, -0.0713924989f, -0.293957889f, 0.272956342f, 0.916015089f};
const float kT[3] = {0.31f, -0.17f, 0.23f};
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

mrh_sdftrack_params camera() {
  mrh_sdftrack_params p = {};
  p.fx = 600.f; p.fy = 590.f; p.cx = 319.5f; p.cy = 239.5f; p.rows = 480; p.cols = 640; p.min_depth = 0.1f; p.max_depth = 8.f;
  return p;
}

struct Call {
  bool depth_form = true;
  mrh_sdftrack_params p = camera();
  const float* R = kR; const float* t = kT;
  bool have_params = true, have_obs = true, have_out = true;
  size_t n = 0;
  float trunc = 0.15f; int pending = 0, shards = 1;
  const char* who() const { return depth_form ? "mrh_track_depth_sdf" : "mrh_track_points_sdf"; }
  int run(mrh_plan::Sdftrack* a) const { return mrh_plan::sdftrack(msg, who(), depth_form, have_params ? &p : nullptr, have_obs, n, have_out, R, t, trunc, pending, shards, a); }
};

Call points(const size_t n) {
  Call c;
  c.depth_form = false;
  c.n = n;
  c.p = {};  // the points calls do not read fx .. cols
  c.p.min_depth = 0.5f; c.p.max_depth = 60.f;
  return c;
}

void defaults() {
  mrh_plan::Sdftrack a;
  Call c;
  expect(c.run(&a) == MRH_OK, "a depth call with every default");
  expect(a.depth_form && a.band == 0.15f && a.iterations == 10 && a.min_pixels == 64u, "band, iterations, min_pixels", a.iterations);
  expect(a.ifx == 1.0f / 600.f && a.ify == 1.0f / 590.f && a.cx == 319.5f && a.cy == 239.5f && a.rows == 480 && a.cols == 640, "the camera");
  expect(a.min_depth == 0.1f && a.max_depth == 8.f, "the depth range");
  c.p.band = 1.f; c.p.iterations = 64; c.p.min_pixels = 7u;
  expect(c.run(&a) == MRH_OK && a.band == 1.f && a.iterations == 64 && a.min_pixels == 7u, "given values are kept; band 1 is accepted");
  c.p.band = 0.f; c.trunc = 2.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "band"), "a default band above 1 m is refused like a given one");
  c.trunc = 0.15f; c.p.iterations = 1;
  expect(c.run(&a) == MRH_OK && a.iterations == 1, "one iteration");
  c.p.rows = c.p.cols = 1;
  expect(c.run(&a) == MRH_OK && a.rows == 1 && a.cols == 1, "one pixel");
  c.p.rows = c.p.cols = MRH_RAYCAST_MAX_SIDE;
  expect(c.run(&a) == MRH_OK && a.rows == 4096 && a.cols == 4096, "4096 x 4096 pixels fit");

  Call q = points(131072);
  expect(q.run(&a) == MRH_OK && !a.depth_form && a.band == 0.15f && a.iterations == 10 && a.min_pixels == 64u, "a points call with every default");
  expect(a.rows == 0 && a.cols == 0 && a.ifx == 0.f && a.ify == 0.f && a.cx == 0.f && a.cy == 0.f, "no camera in the points form");
  expect(a.min_depth == 0.5f && a.max_depth == 60.f, "the range gate");
  q.p.fx = kNaN; q.p.fy = 0.f; q.p.cx = kInf; q.p.rows = -5; q.p.cols = 1 << 30;
  expect(q.run(&a) == MRH_OK && a.rows == 0 && a.ifx == 0.f, "the points calls do not read fx .. cols");
  q = points(0);
  q.have_obs = false;
  expect(q.run(&a) == MRH_OK, "an empty cloud needs no pointer");
  q = points((size_t) 1 << 24);
  expect(q.run(&a) == MRH_OK, "2^24 points fit");
  expect(sizeof(mrh_sdftrack_params) == 48 && sizeof(mrh_track_info) == 280, "struct sizes");
}

void refusals() {
  mrh_plan::Sdftrack a;
  { Call c; c.have_params = false; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: null argument"); }
  { Call c; c.R = nullptr; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: null argument"); }
  { Call c; c.t = nullptr; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: null argument"); }
  { Call c; c.have_out = false; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: null argument"); }
  { Call c; c.have_obs = false; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: null argument"); }
  { Call c = points(1); c.have_obs = false; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_points_sdf: null argument"); }
  { Call c = points(((size_t) 1 << 24) + 1); expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_points_sdf: 16777217 points in one call (limit 2^24)"); }
  { Call c = points(std::numeric_limits<size_t>::max()); expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "limit 2^24"), "the largest count is refused, not wrapped"); }
  { Call c; c.n = std::numeric_limits<size_t>::max(); expect(c.run(&a) == MRH_OK, "the depth form does not read n"); }
  { Call c; c.pending = 1; expect_msg(c.run(&a), MRH_ERR_STATE, "mrh_track_depth_sdf: an exchange is pending (call mrh_integrate_resume)"); }
  { Call c = points(9); c.shards = 2; expect_msg(c.run(&a), MRH_ERR_UNSUPPORTED, "mrh_track_points_sdf: sharded maps are not tracked against (shard_count 2)"); }
  for (const uint32_t bad : {1u, 0x80000000u}) { Call c; c.p.reserved = bad; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: a reserved word is not 0"); }
  for (const int bad : {0, -1, MRH_RAYCAST_MAX_SIDE + 1, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()}) {
    { Call c; c.p.rows = bad; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "pixels (1 .. 4096 per side)"), "bad rows", bad); }
    { Call c; c.p.cols = bad; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "pixels (1 .. 4096 per side)"), "bad cols", bad); }
  }
  for (const float bad : {0.f, kNaN, kInf, -kInf}) {
    { Call c; c.p.fx = bad; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: bad intrinsics"); }
    { Call c; c.p.fy = bad; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: bad intrinsics"); }
    if (bad != 0.f) { Call c; c.p.cx = bad; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: bad intrinsics"); }
    if (bad != 0.f) { Call c; c.p.cy = bad; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_track_depth_sdf: bad intrinsics"); }
  }
  for (const bool depth_form : {true, false}) {
    const struct { float lo, hi; } bad[] = {{0.f, 8.f}, {-1.f, 8.f}, {kNaN, 8.f}, {8.f, 8.f}, {8.f, 0.1f}, {0.1f, kNaN}, {0.1f, kInf}};
    for (const auto& b : bad) {
      Call c = depth_form ? Call() : points(9);
      c.p.min_depth = b.lo; c.p.max_depth = b.hi;
      expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "need 0 < min_depth < max_depth"), "a bad depth range");
    }
    for (const float b : {-0.1f, 1.0001f, kNaN, kInf, -kInf}) {
      Call c = depth_form ? Call() : points(9);
      c.p.band = b;
      expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the band must lie in (0, 1] m"), "a bad band");
    }
    for (const int b : {-1, 65, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()}) {
      Call c = depth_form ? Call() : points(9);
      c.p.iterations = b;
      expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "iterations (1 .. 64, 0 = 10)"), "a bad iteration count", b);
    }
    for (int i = 0; i < 12; i++)
      for (const float b : {kNaN, kInf, -kInf}) {
        float R[9], t[3];
        memcpy(R, kR, sizeof R); memcpy(t, kT, sizeof t);
        (i < 9 ? R[i] : t[i - 9]) = b;
        Call c = depth_form ? Call() : points(9);
        c.R = R; c.t = t;
        expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "pose is not finite"), "a pose that is not finite", i);
      }
  }
}

void precedence() {
  mrh_plan::Sdftrack a;
  const float Rn[9] = {kNaN, 0, 0, 0, 1, 0, 0, 0, 1};
  Call c = points(((size_t) 1 << 24) + 1);  // wrong in every respect the points form reads
  c.have_out = false; c.pending = 1; c.shards = 2; c.p.reserved = 1u; c.p.min_depth = -1.f; c.p.band = 2.f; c.p.iterations = 99; c.R = Rn;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "null argument"), "null argument first");
  c.have_out = true;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "limit 2^24"), "then the point count");
  c.n = 100;
  expect(c.run(&a) == MRH_ERR_STATE, "then a pending exchange");
  c.pending = 0;
  expect(c.run(&a) == MRH_ERR_UNSUPPORTED && strstr(msg, "are not tracked against"), "then a sharded context");
  c.shards = 1;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "reserved word"), "then the reserved word");
  c.p.reserved = 0u;
  c.depth_form = true; c.p.rows = 0; c.p.cols = 640; c.p.fx = 0.f;  // the depth form reads the camera before the depth range
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "image of 0 x 640"), "then the image shape");
  c.p.rows = 480;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "bad intrinsics"), "then the intrinsics");
  c.p.fx = c.p.fy = 600.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "min_depth"), "then the depth range");
  c.p.min_depth = 0.1f; c.p.max_depth = 8.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the band"), "then the band");
  c.p.band = 0.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "99 iterations"), "then the iterations");
  c.p.iterations = 0;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not finite"), "then the pose");
  c.R = kR;
  expect(c.run(&a) == MRH_OK, "and then it runs");
}

void sums_fit() {
  // the bounds the header states, with |J~| < 2^15, |e~| <= 2^18 and 2^24 samples — points, or 4096^2 pixels — and 64 iterations,
  // which do not add up: every linearisation starts its sums at 0
  const long long J = (1ll << 15) - 1, E = 1ll << 18, n = (long long) MRH_SDFTRACK_MAX_POINTS;
  expect(n == (long long) MRH_RAYCAST_MAX_SIDE * MRH_RAYCAST_MAX_SIDE, "an image has at most as many samples as a cloud");
  expect(J * J < (1ll << 30) && (1ll << 30) * n == (1ll << 54) && J * E < (1ll << 33) && (1ll << 33) * n == (1ll << 57) && E * E == (1ll << 36) &&
             (1ll << 36) * n == (1ll << 60),
         "the sums fit a signed 64-bit word");
  expect((n + 255) / 256 <= 0x7FFFFFFFll && (4096 / 16) * (4096 / 16) == 65536, "the slab's rows fit an int");
}

}  // namespace

int main() {
  defaults();
  refusals();
  precedence();
  sums_fit();
  printf("sdftrackplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
