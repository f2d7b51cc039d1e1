// queryplan_check.cpp — the argument plan of the point queries (mrh_plan::query, mrhash_amd/csrc/mrh_readerplan.h) on its own: a
// plain C++17 program that includes the header alone, for tests/test_queryplan.py (g++ -ffp-contract=off, ASan + UBSan).
//
// Checked: the order null argument -> pending -> sharded -> field -> output bits -> reserved words -> n -> R/t pairing -> finite
// pose, with each case's error code; the limits of n on both sides; the messages, literally; the kernel's arguments (identity pose
// for a world-frame call, the pose as given otherwise, the field, the outputs) and the refusal bound (float) (1 << 20) * vs.
// stdout: one line per failure, then "queryplan_check: <n> failures".
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
const char* kWho = "mrh_query_points";

const mrh_query_params kGood = {MRH_QUERY_FIELD_MAP, MRH_QUERY_GRADIENT | MRH_QUERY_COLOUR, {0u, 0u}};
mrh_query_params good() { return kGood; }
int plan(const mrh_query_params& p, const uint64_t n, const float* R, const float* t, mrh::QueryArgs* q, const float vs = 0.05f) {
  return mrh_plan::query(msg, kWho, &p, true, true, n, R, t, vs, 0, 1, q);
}

void arguments() {
  mrh::QueryArgs q;
  mrh_query_params p = good();
  expect(plan(p, 100, nullptr, nullptr, &q) == MRH_OK && q.n == 100u && !q.posed && !q.smooth && q.outputs == 3u, "a world-frame MAP call", q.n);
  bool identity = true;
  for (int i = 0; i < 9; i++) identity = identity && q.R[i] == (i % 4 == 0 ? 1.f : 0.f);
  expect(identity && q.t[0] == 0.f && q.t[1] == 0.f && q.t[2] == 0.f, "a world-frame call carries the identity pose");
  p.field = MRH_QUERY_FIELD_SMOOTH; p.outputs = 0u;
  expect(plan(p, 7, kR, kT, &q) == MRH_OK && q.n == 7u && q.posed && q.smooth && q.outputs == 0u, "a posed SMOOTH call", q.n);
  expect(!memcmp(q.R, kR, sizeof kR) && !memcmp(q.t, kT, sizeof kT), "the pose is carried as given");
  // the bound: one product in binary32, whatever the voxel size
  for (const float vs : {0.05f, 0.0625f, 0.02f, 0.1f, 1e-3f, 3.f}) {
    expect(plan(good(), 1, nullptr, nullptr, &q, vs) == MRH_OK && q.bound == 1048576.f * vs, "bound = (float) (1 << 20) * vs", (long long) q.bound);
    expect(std::isfinite(q.bound) && q.bound > 0.f, "the bound is finite and positive");
  }
  expect(plan(good(), 1, nullptr, nullptr, &q, 0.0625f) == MRH_OK && q.bound == 65536.f, "vs = 2^-4: the bound is 2^16 m");
}

void limits() {
  mrh::QueryArgs q;
  expect(plan(good(), 0, nullptr, nullptr, &q) == MRH_OK && q.n == 0u, "n = 0 is accepted");
  expect(mrh_plan::query(msg, kWho, &kGood, false, true, 0, nullptr, nullptr, 0.05f, 0, 1, &q) == MRH_OK, "n = 0 needs no point list");
  expect(mrh_plan::query(msg, kWho, &kGood, false, true, 1, nullptr, nullptr, 0.05f, 0, 1, &q) == MRH_ERR_INVALID_ARG && !strcmp(msg, "mrh_query_points: null argument"),
         "one point does");
  expect(plan(good(), MRH_QUERY_MAX_POINTS, nullptr, nullptr, &q) == MRH_OK && q.n == MRH_QUERY_MAX_POINTS, "2^24 points are accepted", q.n);
  expect_msg(plan(good(), (uint64_t) MRH_QUERY_MAX_POINTS + 1, nullptr, nullptr, &q), MRH_ERR_INVALID_ARG, "mrh_query_points: 16777217 points in one call (limit 2^24)");
  expect(plan(good(), 1ull << 40, nullptr, nullptr, &q) == MRH_ERR_INVALID_ARG, "a count beyond 32 bits is refused, not truncated");
  mrh_query_params p = good();
  p.field = 2;
  expect_msg(plan(p, 1, nullptr, nullptr, &q), MRH_ERR_INVALID_ARG, "mrh_query_points: unknown field 2");
  p.field = -1;
  expect(plan(p, 1, nullptr, nullptr, &q) == MRH_ERR_INVALID_ARG, "field -1 is refused");
  p = good(); p.outputs = 4u;
  expect_msg(plan(p, 1, nullptr, nullptr, &q), MRH_ERR_INVALID_ARG, "mrh_query_points: unknown output bits 0x4");
  p = good(); p.reserved[1] = 1u;
  expect_msg(plan(p, 1, nullptr, nullptr, &q), MRH_ERR_INVALID_ARG, "mrh_query_points: a reserved word is not 0");
  p = good(); p.reserved[0] = 0x80000000u;
  expect(plan(p, 1, nullptr, nullptr, &q) == MRH_ERR_INVALID_ARG, "the other reserved word too");
  expect_msg(plan(good(), 1, kR, nullptr, &q), MRH_ERR_INVALID_ARG, "mrh_query_points: R and t are both null or both set");
  expect(plan(good(), 1, nullptr, kT, &q) == MRH_ERR_INVALID_ARG, "t without R is refused");
  for (int i = 0; i < 12; i++)
    for (const float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()}) {
      float R[9], t[3];
      memcpy(R, kR, sizeof R); memcpy(t, kT, sizeof t);
      (i < 9 ? R[i] : t[i - 9]) = bad;
      expect(plan(good(), 1, R, t, &q) == MRH_ERR_INVALID_ARG && !strcmp(msg, "mrh_query_points: pose is not finite"), "a pose that is not finite is refused", i);
    }
}

void precedence() {
  mrh::QueryArgs q;
  mrh_query_params p = good();  // wrong in every later respect as well
  p.field = 9; p.outputs = 0xF0u; p.reserved[0] = 1u;
  const uint64_t big = (uint64_t) MRH_QUERY_MAX_POINTS + 1;
  const float nan = std::numeric_limits<float>::quiet_NaN(), Rn[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 1};
  expect(mrh_plan::query(msg, "q", nullptr, true, true, big, Rn, nullptr, 0.05f, 1, 2, &q) == MRH_ERR_INVALID_ARG && !strcmp(msg, "q: null argument"), "null block first");
  expect(mrh_plan::query(msg, "q", &p, false, true, big, Rn, nullptr, 0.05f, 1, 2, &q) == MRH_ERR_INVALID_ARG && !strcmp(msg, "q: null argument"), "a null point list too");
  expect(mrh_plan::query(msg, "q", &p, true, false, big, Rn, nullptr, 0.05f, 1, 2, &q) == MRH_ERR_INVALID_ARG && !strcmp(msg, "q: null argument"), "a null required output too");
  expect_msg(mrh_plan::query(msg, "mrh_query_points_device", &p, true, true, big, Rn, nullptr, 0.05f, 1, 2, &q), MRH_ERR_STATE,
             "mrh_query_points_device: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(mrh_plan::query(msg, kWho, &p, true, true, big, Rn, nullptr, 0.05f, 0, 2, &q), MRH_ERR_UNSUPPORTED, "mrh_query_points: sharded maps are not queried (shard_count 2)");
  expect(mrh_plan::query(msg, "q", &p, true, true, big, Rn, nullptr, 0.05f, 0, 1, &q) == MRH_ERR_INVALID_ARG && strstr(msg, "unknown field"), "then the field");
  p.field = MRH_QUERY_FIELD_SMOOTH;
  expect(mrh_plan::query(msg, "q", &p, true, true, big, Rn, nullptr, 0.05f, 0, 1, &q) == MRH_ERR_INVALID_ARG && strstr(msg, "unknown output bits 0xf0"), "then the output bits");
  p.outputs = MRH_QUERY_COLOUR;
  expect(mrh_plan::query(msg, "q", &p, true, true, big, Rn, nullptr, 0.05f, 0, 1, &q) == MRH_ERR_INVALID_ARG && strstr(msg, "reserved word"), "then the reserved words");
  p.reserved[0] = 0u;
  expect(mrh_plan::query(msg, "q", &p, true, true, big, Rn, nullptr, 0.05f, 0, 1, &q) == MRH_ERR_INVALID_ARG && strstr(msg, "limit 2^24"), "then n");
  expect(mrh_plan::query(msg, "q", &p, true, true, 10, Rn, nullptr, 0.05f, 0, 1, &q) == MRH_ERR_INVALID_ARG && strstr(msg, "both null or both set"), "then the pairing");
  expect(mrh_plan::query(msg, "q", &p, true, true, 10, Rn, kT, 0.05f, 0, 1, &q) == MRH_ERR_INVALID_ARG && strstr(msg, "not finite"), "then the pose");
}

}  // namespace

int main() {
  arguments();
  limits();
  precedence();
  printf("queryplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
