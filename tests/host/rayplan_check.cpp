// rayplan_check.cpp — the argument plan of the ray queries (mrh_plan::rays, mrhash_amd/csrc/mrh_readerplan.h) on its own: a plain
// C++17 program that includes the header alone, for tests/test_rayplan.py (g++ -ffp-contract=off, ASan + UBSan).
//
// Checked: the order null argument -> pending -> sharded -> reserved words -> output bits -> range -> step -> samples -> n -> R/t
// pairing -> finite pose, with each case's error code; the limits of n and of the sample count on both sides; min_range == 0
// accepted; the messages, literally; the kernel's arguments (identity pose for a world-frame call, the pose as given otherwise, the
// default step, the sample count against a literal march) and the refusal bound (float) (1 << 20) * vs.
// stdout: one line per failure, then "rayplan_check: <n> failures".
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

const float kR[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, kT[3] = {1.5f, -2.f, 0.25f};
const char* kWho = "mrh_cast_rays";
const float kTrunc = 0.15f, kVs = 0.05f;

const mrh_rays_params kGood = {0.f, 5.f, 0.f, MRH_RAYS_NORMALS | MRH_RAYS_COLORS | MRH_RAYS_COUNTS, {0u, 0u, 0u, 0u}};
mrh_rays_params good() { return kGood; }
int plan(const mrh_rays_params& p, const uint64_t n, const float* R, const float* t, mrh::RaysArgs* a, const float vs = kVs) {
  return mrh_plan::rays(msg, kWho, &p, true, true, n, R, t, kTrunc, vs, 0, 1, a);
}

// the samples of a batch by the literal march
uint32_t literal_count(const float lo, const float hi, const float step) {
  uint32_t k = 0;
  while (lo + (float) k * step <= hi) k++;
  return k;
}

void arguments() {
  mrh::RaysArgs a;
  mrh_rays_params p = good();
  expect(plan(p, 100, nullptr, nullptr, &a) == MRH_OK && a.n == 100u && !a.posed && a.outputs == 7u, "a world-frame call", a.n);
  expect(a.min_range == 0.f && a.max_range == 5.f && a.step == 0.5f * kTrunc, "step 0 is half the truncation");
  expect(a.n_samples == literal_count(0.f, 5.f, 0.5f * kTrunc), "the sample count is the literal march's", a.n_samples, literal_count(0.f, 5.f, 0.5f * kTrunc));
  bool identity = true;
  for (int i = 0; i < 9; i++) identity = identity && a.R[i] == (i % 4 == 0 ? 1.f : 0.f);
  expect(identity && a.t[0] == 0.f && a.t[1] == 0.f && a.t[2] == 0.f, "a world-frame call carries the identity pose");
  p.outputs = 0u; p.step = 0.1f; p.min_range = 0.3f;
  expect(plan(p, 7, kR, kT, &a) == MRH_OK && a.n == 7u && a.posed && a.outputs == 0u && a.step == 0.1f && a.min_range == 0.3f, "a posed call", a.n);
  expect(!memcmp(a.R, kR, sizeof kR) && !memcmp(a.t, kT, sizeof kT), "the pose is carried as given");
  for (const float step : {0.1f, 0.075f, 0.013f, 1.f, 7.f})
    for (const float lo : {0.f, 0.1f, 2.5f}) {
      p = good(); p.step = step; p.min_range = lo;
      expect(plan(p, 1, nullptr, nullptr, &a) == MRH_OK && a.n_samples == literal_count(lo, 5.f, step), "sample counts", a.n_samples, literal_count(lo, 5.f, step));
    }
  // the bound: one product in binary32, whatever the voxel size
  for (const float vs : {0.05f, 0.0625f, 0.02f, 0.1f, 1e-3f, 3.f}) {
    expect(plan(good(), 1, nullptr, nullptr, &a, vs) == MRH_OK && a.bound == 1048576.f * vs, "bound = (float) (1 << 20) * vs", (long long) a.bound);
    expect(std::isfinite(a.bound) && a.bound > 0.f, "the bound is finite and positive");
  }
  expect(plan(good(), 1, nullptr, nullptr, &a, 0.0625f) == MRH_OK && a.bound == 65536.f, "vs = 2^-4: the bound is 2^16 m");
}

void limits() {
  mrh::RaysArgs a;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  expect(plan(good(), 0, nullptr, nullptr, &a) == MRH_OK && a.n == 0u, "n = 0 is accepted");
  expect(mrh_plan::rays(msg, kWho, &kGood, false, true, 0, nullptr, nullptr, kTrunc, kVs, 0, 1, &a) == MRH_OK, "n = 0 needs no rays");
  expect_msg(mrh_plan::rays(msg, kWho, &kGood, false, true, 1, nullptr, nullptr, kTrunc, kVs, 0, 1, &a), MRH_ERR_INVALID_ARG, "mrh_cast_rays: null argument");
  expect(plan(good(), MRH_RAYS_MAX_RAYS, nullptr, nullptr, &a) == MRH_OK && a.n == MRH_RAYS_MAX_RAYS, "2^24 rays are accepted", a.n);
  expect_msg(plan(good(), (uint64_t) MRH_RAYS_MAX_RAYS + 1, nullptr, nullptr, &a), MRH_ERR_INVALID_ARG, "mrh_cast_rays: 16777217 rays in one call (limit 2^24)");
  expect(plan(good(), 1ull << 40, nullptr, nullptr, &a) == MRH_ERR_INVALID_ARG, "a count beyond 32 bits is refused, not truncated");
  // the range: min_range == 0 and a range of one sample are fine
  mrh_rays_params p = good();
  p.min_range = 0.f; p.max_range = 0.f;
  expect(plan(p, 1, nullptr, nullptr, &a) == MRH_OK && a.n_samples == 1u, "min_range = max_range = 0: one sample", a.n_samples);
  p.min_range = -0.f;
  expect(plan(p, 1, nullptr, nullptr, &a) == MRH_OK, "-0 is 0");
  p = good(); p.min_range = -1e-6f;
  expect_msg(plan(p, 1, nullptr, nullptr, &a), MRH_ERR_INVALID_ARG, "mrh_cast_rays: need 0 <= min_range <= max_range (got -1e-06, 5)");
  p = good(); p.min_range = 6.f;
  expect(plan(p, 1, nullptr, nullptr, &a) == MRH_ERR_INVALID_ARG, "min_range > max_range is refused");
  for (const float bad : {nan, inf, -inf}) {
    p = good(); p.max_range = bad;
    expect(plan(p, 1, nullptr, nullptr, &a) == MRH_ERR_INVALID_ARG && strstr(msg, "min_range <= max_range"), "a max_range that is not finite");
    p = good(); p.min_range = bad;
    expect(plan(p, 1, nullptr, nullptr, &a) == MRH_ERR_INVALID_ARG && strstr(msg, "min_range <= max_range"), "a min_range that is not finite");
  }
  for (const float bad : {nan, inf, -inf, -0.1f}) {
    p = good(); p.step = bad;
    expect(plan(p, 1, nullptr, nullptr, &a) == MRH_ERR_INVALID_ARG && strstr(msg, "sample spacing"), "a bad step");
  }
  // the sample count: 2^20 samples are accepted, one more is not (step 1, exact in binary32)
  p = good(); p.step = 1.f; p.max_range = 1048575.f;
  expect(plan(p, 1, nullptr, nullptr, &a) == MRH_OK && a.n_samples == MRH_RAYS_MAX_SAMPLES, "2^20 samples are accepted", a.n_samples);
  p.max_range = 1048576.f;
  expect_msg(plan(p, 1, nullptr, nullptr, &a), MRH_ERR_INVALID_ARG, "mrh_cast_rays: more than 2^20 samples per ray (min_range 0, max_range 1.04858e+06, step 1)");
  p = good(); p.outputs = 8u;
  expect_msg(plan(p, 1, nullptr, nullptr, &a), MRH_ERR_INVALID_ARG, "mrh_cast_rays: unknown output bits 0x8");
  for (int i = 0; i < 4; i++) {
    p = good(); p.reserved[i] = 1u << (7 * i);
    expect_msg(plan(p, 1, nullptr, nullptr, &a), MRH_ERR_INVALID_ARG, "mrh_cast_rays: a reserved word is not 0");
  }
  expect_msg(plan(good(), 1, kR, nullptr, &a), MRH_ERR_INVALID_ARG, "mrh_cast_rays: R and t are both null or both set");
  expect(plan(good(), 1, nullptr, kT, &a) == MRH_ERR_INVALID_ARG, "t without R is refused");
  for (int i = 0; i < 12; i++)
    for (const float bad : {nan, inf, -inf}) {
      float R[9], t[3];
      memcpy(R, kR, sizeof R); memcpy(t, kT, sizeof t);
      (i < 9 ? R[i] : t[i - 9]) = bad;
      expect(plan(good(), 1, R, t, &a) == MRH_ERR_INVALID_ARG && !strcmp(msg, "mrh_cast_rays: pose is not finite"), "a pose that is not finite is refused", i);
    }
}

void precedence() {
  mrh::RaysArgs a;
  mrh_rays_params p = good();  // wrong in every later respect as well
  p.reserved[2] = 1u; p.outputs = 0xF0u; p.min_range = -1.f; p.step = -1.f;
  const uint64_t big = (uint64_t) MRH_RAYS_MAX_RAYS + 1;
  const float nan = std::numeric_limits<float>::quiet_NaN(), Rn[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 1};
  auto run = [&](const mrh_rays_params* q, const bool rays, const bool out, const uint64_t n, const float* R, const float* t, const int pending, const int shards) {
    return mrh_plan::rays(msg, "q", q, rays, out, n, R, t, kTrunc, kVs, pending, shards, &a);
  };
  expect(run(nullptr, true, true, big, Rn, nullptr, 1, 2) == MRH_ERR_INVALID_ARG && !strcmp(msg, "q: null argument"), "null block first");
  expect(run(&p, false, true, big, Rn, nullptr, 1, 2) == MRH_ERR_INVALID_ARG && !strcmp(msg, "q: null argument"), "null rays too");
  expect(run(&p, true, false, big, Rn, nullptr, 1, 2) == MRH_ERR_INVALID_ARG && !strcmp(msg, "q: null argument"), "a null required output too");
  expect_msg(mrh_plan::rays(msg, "mrh_cast_rays_device", &p, true, true, big, Rn, nullptr, kTrunc, kVs, 1, 2, &a), MRH_ERR_STATE,
             "mrh_cast_rays_device: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(mrh_plan::rays(msg, kWho, &p, true, true, big, Rn, nullptr, kTrunc, kVs, 0, 2, &a), MRH_ERR_UNSUPPORTED,
             "mrh_cast_rays: sharded maps take no ray queries (shard_count 2)");
  expect(run(&p, true, true, big, Rn, nullptr, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "reserved word"), "then the reserved words");
  p.reserved[2] = 0u;
  expect(run(&p, true, true, big, Rn, nullptr, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "unknown output bits 0xf0"), "then the output bits");
  p.outputs = MRH_RAYS_COUNTS;
  expect(run(&p, true, true, big, Rn, nullptr, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "min_range <= max_range"), "then the range");
  p.min_range = 0.f;
  expect(run(&p, true, true, big, Rn, nullptr, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "sample spacing"), "then the step");
  p.step = 1e-6f;
  expect(run(&p, true, true, big, Rn, nullptr, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "2^20 samples"), "then the sample count");
  p.step = 0.f;
  expect(run(&p, true, true, big, Rn, nullptr, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "limit 2^24"), "then n");
  expect(run(&p, true, true, 10, Rn, nullptr, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "both null or both set"), "then the pairing");
  expect(run(&p, true, true, 10, Rn, kT, 0, 1) == MRH_ERR_INVALID_ARG && strstr(msg, "not finite"), "then the pose");
  expect(run(&p, true, true, 10, kR, kT, 0, 1) == MRH_OK, "and a call that is right in everything passes");
}

// the render's plan still says what it said: the shared sample count and pose test (readerplan_check.cpp has the rest)
void render_shares_the_helpers() {
  mrh::RayCam rc;
  const mrh_raycast_params rp = {500.f, 500.f, 320.f, 240.f, 4, 4, 0.1f, 5.f, 0.075f, 0u};
  expect(mrh_plan::raycast(msg, "r", MRH_CAMERA_PINHOLE, &rp, kR, kT, kTrunc, 0, 1, &rc) == MRH_OK && rc.n_samples == literal_count(0.1f, 5.f, 0.075f),
         "the render counts its samples as before", rc.n_samples);
  mrh::RaysArgs a;
  mrh_rays_params p = good();
  p.min_range = 0.1f; p.step = 0.075f;
  expect(plan(p, 1, nullptr, nullptr, &a) == MRH_OK && a.n_samples == rc.n_samples, "the same range gives the ray query the render's count", a.n_samples, rc.n_samples);
}

}  // namespace

int main() {
  arguments();
  limits();
  precedence();
  render_shares_the_helpers();
  printf("rayplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
