// readerplan_check.cpp — the argument plans of the map readers and of the scan normals (mrhash_amd/csrc/mrh_readerplan.h) on their
// own: a plain C++17 program that includes the header alone, for tests/test_readerplan.py (g++ -ffp-contract=off, ASan + UBSan).
//
// Checked: the sample count against a literal linear count (one sample, a step that does not divide the range, a step far below an
// ulp of max_depth, both sides of 2^20 samples, a grid); the spherical angle bound on both sides of MRH_SM_SINCOS_MAX; the box of a
// distance field at its last accepted and first rejected dims, origin and reach; the default of w_min; the tracking defaults and
// limits; the order null block -> pending -> sharded -> limits with each case's error code; one message per feature, literally.
// stdout: one line per failure, then "readerplan_check: <n> failures".
#include <cmath>
#include <cstdio>
#include <cstring>

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

const float kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZ[3] = {0, 0, 0};

mrh_raycast_params ray_params(const float min_depth, const float max_depth, const float step) {
  return mrh_raycast_params{50.f, 50.f, 39.5f, 29.5f, 60, 80, min_depth, max_depth, step, MRH_RAYCAST_NORMALS};
}
int plan_ray(const mrh_raycast_params& p, const int model, mrh::RayCam* rc, const float truncation = 0.04f) {
  return mrh_plan::raycast(msg, "mrh_raycast", model, &p, kI, kZ, truncation, 0, 1, rc);
}

// the definition: how many k = 0, 1, .. have z_k <= max_depth, counted one by one (stops above the limit)
uint32_t linear_count(const float min_depth, const float max_depth, const float step) {
  uint32_t k = 0;
  while (k <= MRH_RAYCAST_MAX_SAMPLES && min_depth + (float) k * step <= max_depth) k++;
  return k;
}
void check_samples(const float min_depth, const float max_depth, const float step, const long long want = -1) {
  const uint32_t n = linear_count(min_depth, max_depth, step);
  if (want >= 0) expect((long long) n == want, "the case has the sample count it was built for", n, want);
  mrh::RayCam rc;
  const int e = plan_ray(ray_params(min_depth, max_depth, step), MRH_CAMERA_PINHOLE, &rc);
  if (n > MRH_RAYCAST_MAX_SAMPLES) expect(e == MRH_ERR_INVALID_ARG && strstr(msg, "more than 2^20 samples"), "above 2^20 samples is refused", e);
  else expect(e == MRH_OK && rc.n_samples == n, "n_samples equals the linear count", rc.n_samples, n);
}

void sample_counts() {
  check_samples(1.f, 1.5f, 1.f, 1);                   // exactly one sample
  check_samples(0.1f, 8.f, 0.07f);                    // the step does not divide the range
  check_samples(4095.99f, 4096.f, 1e-6f);             // a step far below one ulp of max_depth (2^-11): z_k stays put for many k
  const float s = 1.f / 1024.f;                       // z_k = 1 + k / 1024 is exact up to k = 2^20
  check_samples(1.f, 1.f + 1048575.f * s, s, 1 << 20);        // the last accepted case: 2^20 samples
  check_samples(1.f, 1.f + 1048576.f * s, s, (1 << 20) + 1);  // the first rejected one: z(2^20) <= max_depth
  for (const float lo : {0.05f, 0.3f, 1.f})
    for (const float hi : {0.5f, 3.f, 8.1f, 30.f})
      for (const float step : {0.00001f, 0.003f, 0.02f, 0.07f, 1.f, 100.f})
        if (hi > lo) check_samples(lo, hi, step);
  mrh::RayCam rc;  // step 0: half the truncation
  expect(plan_ray(ray_params(0.1f, 8.f, 0.f), MRH_CAMERA_PINHOLE, &rc, 0.25f) == MRH_OK && rc.step == 0.125f && rc.n_samples == linear_count(0.1f, 8.f, 0.125f),
         "the default step is half the truncation", rc.n_samples);
}

void spherical_bound() {
  // fx = fy = 1: a pixel's angle is ((index - c) - 0.5), exact for the values below; 8192 has an ulp of 2^-10
  const float ulp = 1.f / 1024.f;
  mrh::RayCam rc;
  mrh_raycast_params p = {1.f, 1.f, -8191.5f, 0.f, 1, 2, 0.1f, 8.f, 0.05f, MRH_RAYCAST_POINTS};
  expect(plan_ray(p, MRH_CAMERA_SPHERICAL, &rc) == MRH_OK, "an azimuth of exactly 8192 rad is accepted");
  p.cx = -8191.5f - ulp;
  expect(plan_ray(p, MRH_CAMERA_SPHERICAL, &rc) == MRH_ERR_INVALID_ARG && strstr(msg, "azimuth or elevation"), "an azimuth one ulp above 8192 rad is refused");
  p.cx = 8191.5f;  // column 0: -8192
  expect(plan_ray(p, MRH_CAMERA_SPHERICAL, &rc) == MRH_OK, "an azimuth of exactly -8192 rad is accepted");
  p.cx = 8191.5f + ulp;
  expect(plan_ray(p, MRH_CAMERA_SPHERICAL, &rc) == MRH_ERR_INVALID_ARG, "an azimuth one ulp below -8192 rad is refused");
  p = mrh_raycast_params{1.f, 1.f, 0.f, -8191.5f, 2, 1, 0.1f, 8.f, 0.05f, 0u};
  expect(plan_ray(p, MRH_CAMERA_SPHERICAL, &rc) == MRH_OK, "an elevation of exactly 8192 rad is accepted");
  p.cy = -8192.5f;
  expect_msg(mrh_plan::raycast(msg, "mrh_raycast_spherical", MRH_CAMERA_SPHERICAL, &p, kI, kZ, 0.04f, 0, 1, &rc), MRH_ERR_INVALID_ARG,
             "mrh_raycast_spherical: a pixel's azimuth or elevation reaches 8193 rad (sine and cosine are specified up to 8192)");
  expect(plan_ray(p, MRH_CAMERA_PINHOLE, &rc) == MRH_OK, "the bound belongs to the spherical model");
  p.outputs = MRH_RAYCAST_POINTS; p.cy = 0.f;
  expect(plan_ray(p, MRH_CAMERA_PINHOLE, &rc) == MRH_ERR_INVALID_ARG && plan_ray(p, MRH_CAMERA_SPHERICAL, &rc) == MRH_OK, "the points bit too");
}

mrh_esdf_params box_params() { return mrh_esdf_params{{-8, 0, 8}, {20, 30, 40}, 16, 0, 0.f, MRH_ESDF_STATE}; }
int plan_box(const mrh_esdf_params& p, mrh::EsdfBox* bx, const int threshold = 5) { return mrh_plan::esdf(msg, "mrh_esdf", &p, threshold, 0, 1, bx); }

void esdf_box() {
  mrh::EsdfBox bx;
  for (int a = 0; a < 3; a++) {
    struct { int dims; long long origin; int reach; bool ok; } cases[] = {
        {1, 0, 16, true}, {MRH_ESDF_MAX_SIDE, 0, 16, true}, {0, 0, 16, false}, {MRH_ESDF_MAX_SIDE + 1, 0, 16, false},
        {20, -(1ll << 23), 16, true}, {20, -(1ll << 23) - 1, 16, false}, {20, (1ll << 23) - 20, 16, true}, {20, (1ll << 23) - 19, 16, false},
        {MRH_ESDF_MAX_SIDE, (1ll << 23) - MRH_ESDF_MAX_SIDE, 16, true}, {1, (1ll << 23) - 1, 16, true}, {1, 1ll << 23, 16, false},
        {20, 0, 1, true}, {20, 0, MRH_ESDF_MAX_REACH, true}, {20, 0, 0, false}, {20, 0, MRH_ESDF_MAX_REACH + 1, false}};
    for (const auto& k : cases) {
      mrh_esdf_params p = box_params();
      p.dims[a] = k.dims; p.origin[a] = (int32_t) k.origin; p.max_distance_voxels = k.reach;
      const int e = plan_box(p, &bx);
      expect(e == (k.ok ? MRH_OK : MRH_ERR_INVALID_ARG), "a box at its limit", a, k.dims * 100000000000ll + k.origin);
      if (e == MRH_OK) {
        const int o[3] = {bx.ox, bx.oy, bx.oz}, n[3] = {bx.nx, bx.ny, bx.nz};
        expect(o[a] == k.origin && n[a] == k.dims && bx.reach == (uint32_t) k.reach, "the box carries the block's values", a);
      }
    }
  }
  mrh_esdf_params p = box_params();
  expect(plan_box(p, &bx, 5) == MRH_OK && bx.w_min == 5, "w_min defaults to the context's threshold", bx.w_min);
  expect(plan_box(p, &bx, 0) == MRH_OK && bx.w_min == 1, "... and is at least 1", bx.w_min);
  p.min_weight = 7;
  expect(plan_box(p, &bx, 5) == MRH_OK && bx.w_min == 7, "a given min_weight wins", bx.w_min);
  p.min_weight = -1;
  expect(plan_box(p, &bx, 5) == MRH_ERR_INVALID_ARG, "a negative min_weight is refused");
  p = box_params();
  p.origin[1] = 8388600; p.dims[1] = 10;
  expect_msg(plan_box(p, &bx), MRH_ERR_INVALID_ARG, "mrh_esdf: axis 1 of the box spans voxels 8388600 .. 8388609, outside [-2^23, 2^23)");
}

mrh_track_params track_params() { return mrh_track_params{50.f, 50.f, 39.5f, 29.5f, 60, 80, 0.1f, 8.f, 0.f, 0.f, 0, 0u}; }
int plan_track(const mrh_track_params& p, const int model, const bool have_obs, const size_t n, mrh_plan::Track* t, const float truncation = 0.04f) {
  return mrh_plan::track(msg, "mrh_track_depth", model, &p, have_obs, n, true, kI, kZ, truncation, 0, 1, t);
}

void tracking() {
  mrh_plan::Track t;
  mrh_track_params p = track_params();
  expect(plan_track(p, MRH_CAMERA_PINHOLE, true, 0, &t) == MRH_OK && t.dist_max == 2.f * 0.04f && t.iterations == 10 && t.min_pixels == 64u,
         "defaults: the gate is twice the truncation, 10 iterations, 64 pixels", t.iterations, t.min_pixels);
  expect(t.cam.step == 0.02f && t.cam.rows == 60 && t.cam.cols == 80 && t.cam.n_samples == linear_count(0.1f, 8.f, 0.02f), "the model render is the raycast plan's");
  expect(plan_track(p, MRH_CAMERA_PINHOLE, true, 0, &t, 0.7f) == MRH_OK && t.dist_max == 1.f, "the default gate is capped at 1 m");
  p.dist_max = 0.3f; p.iterations = MRH_TRACK_MAX_ITERATIONS; p.min_pixels = 7u;
  expect(plan_track(p, MRH_CAMERA_PINHOLE, true, 0, &t) == MRH_OK && t.dist_max == 0.3f && t.iterations == MRH_TRACK_MAX_ITERATIONS && t.min_pixels == 7u,
         "given values are kept");
  p.iterations = MRH_TRACK_MAX_ITERATIONS + 1;
  expect(plan_track(p, MRH_CAMERA_PINHOLE, true, 0, &t) == MRH_ERR_INVALID_ARG, "65 iterations are refused");
  p.iterations = -1;
  expect(plan_track(p, MRH_CAMERA_PINHOLE, true, 0, &t) == MRH_ERR_INVALID_ARG, "-1 iterations are refused");
  p = track_params();
  p.dist_max = 1.f;
  expect(plan_track(p, MRH_CAMERA_PINHOLE, true, 0, &t) == MRH_OK, "a gate of 1 m is accepted");
  p.dist_max = 1.5f;
  expect_msg(plan_track(p, MRH_CAMERA_PINHOLE, true, 0, &t), MRH_ERR_INVALID_ARG, "mrh_track_depth: the gate must lie in (0, 1] m (dist_max 1.5)");
  p = track_params();
  expect(plan_track(p, MRH_CAMERA_PINHOLE, false, 0, &t) == MRH_ERR_INVALID_ARG && !strcmp(msg, "mrh_track_depth: null argument"), "a depth image is required");
  expect(plan_track(p, MRH_CAMERA_SPHERICAL, false, 0, &t) == MRH_OK, "an empty scan needs no cloud");
  expect(plan_track(p, MRH_CAMERA_SPHERICAL, false, 1, &t) == MRH_ERR_INVALID_ARG, "one point does");
  expect(plan_track(p, MRH_CAMERA_SPHERICAL, true, (size_t) 1 << 24, &t) == MRH_OK, "2^24 points are accepted");
  expect(plan_track(p, MRH_CAMERA_SPHERICAL, true, ((size_t) 1 << 24) + 1, &t) == MRH_ERR_INVALID_ARG && strstr(msg, "limit 2^24"), "2^24 + 1 are refused");
  expect(mrh_plan::track(msg, "mrh_track_scan", MRH_CAMERA_SPHERICAL, &p, true, 100, false, kI, kZ, 0.04f, 0, 1, &t) == MRH_ERR_INVALID_ARG, "the pose outputs are required");
}

void precedence() {
  mrh::RayCam rc;
  mrh::EsdfBox bx;
  mrh_plan::Track t;
  mrh_raycast_params rp = ray_params(0.1f, 8.f, 0.05f);
  rp.rows = 0;  // beyond its limits as well
  mrh_esdf_params ep = box_params();
  ep.dims[0] = 0;
  mrh_track_params tp = track_params();
  tp.rows = 0;
  const size_t big = ((size_t) 1 << 24) + 1;
  // raycast: null block (or pose), pending, sharded, limits
  expect(mrh_plan::raycast(msg, "r", 0, nullptr, kI, kZ, 0.04f, 1, 2, &rc) == MRH_ERR_INVALID_ARG && !strcmp(msg, "r: null argument"), "raycast: null block first");
  expect(mrh_plan::raycast(msg, "r", 0, &rp, nullptr, kZ, 0.04f, 1, 2, &rc) == MRH_ERR_INVALID_ARG && !strcmp(msg, "r: null argument"), "raycast: null pose first");
  expect_msg(mrh_plan::raycast(msg, "mrh_raycast_device", 0, &rp, kI, kZ, 0.04f, 1, 2, &rc), MRH_ERR_STATE, "mrh_raycast_device: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(mrh_plan::raycast(msg, "mrh_raycast", 0, &rp, kI, kZ, 0.04f, 0, 2, &rc), MRH_ERR_UNSUPPORTED, "mrh_raycast: sharded maps are not rendered (shard_count 2)");
  expect_msg(mrh_plan::raycast(msg, "mrh_raycast", 0, &rp, kI, kZ, 0.04f, 0, 1, &rc), MRH_ERR_INVALID_ARG, "mrh_raycast: image of 0 x 80 pixels (1 .. 4096 per side)");
  // distance field
  expect(mrh_plan::esdf(msg, "e", nullptr, 5, 2, 4, &bx) == MRH_ERR_INVALID_ARG && !strcmp(msg, "e: null argument"), "esdf: null block first");
  expect(mrh_plan::esdf(msg, "e", &ep, 5, 2, 4, &bx) == MRH_ERR_STATE, "esdf: then the pending exchange");
  expect_msg(mrh_plan::esdf(msg, "mrh_esdf", &ep, 5, 0, 4, &bx), MRH_ERR_UNSUPPORTED, "mrh_esdf: sharded maps have no distance field (shard_count 4)");
  expect_msg(mrh_plan::esdf(msg, "mrh_esdf_device", &ep, 5, 0, 1, &bx), MRH_ERR_INVALID_ARG, "mrh_esdf_device: box of 0 x 30 x 40 cells (1 .. 512 per side)");
  // tracking: null, the scan's size, then the raycast plan's order, then its own limits
  tp.dist_max = 2.f;
  expect(mrh_plan::track(msg, "t", 1, nullptr, true, big, true, kI, kZ, 0.04f, 1, 2, &t) == MRH_ERR_INVALID_ARG && !strcmp(msg, "t: null argument"), "track: null block first");
  expect(mrh_plan::track(msg, "t", 1, &tp, true, big, true, kI, kZ, 0.04f, 1, 2, &t) == MRH_ERR_INVALID_ARG && strstr(msg, "limit 2^24"), "track: then the scan's size");
  expect(mrh_plan::track(msg, "t", 1, &tp, true, 100, true, kI, kZ, 0.04f, 1, 2, &t) == MRH_ERR_STATE, "track: then the pending exchange");
  expect_msg(mrh_plan::track(msg, "mrh_track_scan", 1, &tp, true, 100, true, kI, kZ, 0.04f, 0, 2, &t), MRH_ERR_UNSUPPORTED, "mrh_track_scan: sharded maps are not rendered (shard_count 2)");
  expect(mrh_plan::track(msg, "t", 1, &tp, true, 100, true, kI, kZ, 0.04f, 0, 1, &t) == MRH_ERR_INVALID_ARG && strstr(msg, "image of 0 x 80"), "track: then the render's limits");
  tp.rows = 60;
  expect(mrh_plan::track(msg, "t", 1, &tp, true, 100, true, kI, kZ, 0.04f, 0, 1, &t) == MRH_ERR_INVALID_ARG && strstr(msg, "the gate"), "track: then its own");
}

void normals() {
  mrh::NrmPar par;
  expect(mrh_plan::normals(msg, "n", nullptr, 1000, 0.05f, &par) == MRH_OK && par.rho == 0.1f && par.min_points == 5u && par.min_l1 == 4096.0 && par.max_flat == 0.0625,
         "defaults: two voxels, 5 points, 1 / 16, 1 / 16");
  const mrh_normals_params q = {0.4f, 9u, 0.5f, 0.25f};
  expect(mrh_plan::normals(msg, "n", &q, (1ull << 24) - 1, 0.05f, &par) == MRH_OK && par.rho == 0.4f && par.min_points == 9u && par.min_l1 == 512.0 * 512.0 && par.max_flat == 0.25,
         "given values are kept; 2^24 - 1 points are accepted");
  expect_msg(mrh_plan::normals(msg, "mrh_estimate_normals", &q, 1ull << 24, 0.05f, &par), MRH_ERR_CAPACITY, "mrh_estimate_normals: 16777216 points in one scan (limit 2^24 - 1)");
  const mrh_normals_params bad = {0.4f, 9u, 0.5f, 1.f};
  expect(mrh_plan::normals(msg, "n", &bad, 1ull << 24, 0.05f, &par) == MRH_ERR_INVALID_ARG, "a bad parameter is reported before the size");
}

}  // namespace

int main() {
  sample_counts();
  spherical_bound();
  esdf_box();
  tracking();
  precedence();
  normals();
  printf("readerplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
