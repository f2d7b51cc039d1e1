// alignplan_check.cpp — the argument plan of map-to-map registration (mrh_plan::align, align_sample_bytes, align_auto_pivot, align_tau,
// align_t; mrhash_amd/csrc/mrh_readerplan.h) on its own: a plain C++17 program that includes the header alone, for
// tests/test_alignplan.py (g++ -ffp-contract=off, ASan + UBSan).
//
// Checked: every refusal of include/mrhash_align.h with its code and, where the C ABI's text is fixed, its message; the order
// null argument -> dst == src -> devices -> pending, sharded (source, then destination) -> reserved words -> min_weight -> band ->
// dist_max -> iterations -> pivot -> extent -> finite pose -> rotation; the defaults; the 2^26 cap of the sample list; the integer-box
// rule of the automatic pivot; tau = R c + t and back.
// stdout: one line per failure, then "alignplan_check: <n> failures".
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
const char* kWho = "mrh_align_map";
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

struct Call {
  mrh_align_params p = {};
  const float* R = kR; const float* t = kT;
  bool have_out = true, same_ctx = false, same_device = true;
  float src_trunc = 0.15f; int src_pending = 0, src_shards = 1;
  float dst_trunc = 0.2f; int dst_pending = 0, dst_shards = 1;
  int run(mrh_plan::Align* a) const {
    return mrh_plan::align(msg, kWho, &p, R, t, have_out, same_ctx, same_device, src_trunc, src_pending, src_shards, dst_trunc, dst_pending, dst_shards, a);
  }
};

void defaults() {
  mrh_plan::Align a;
  Call c;
  expect(c.run(&a) == MRH_OK, "a call with every default");
  expect(a.band == 0.15f && a.dist_max == 0.15f && a.iterations == 10 && a.min_samples == 64u && a.w_min == 1u, "band, dist_max, iterations, min_samples, w_min", a.iterations);
  expect(!a.crop && a.extent == 0.f && a.pivot[0] == 0.f && a.pivot[1] == 0.f && a.pivot[2] == 0.f, "no crop");
  c.src_trunc = 0.3f;
  expect(c.run(&a) == MRH_OK && a.band == 0.2f && a.dist_max == 0.2f, "the band is the smaller truncation");
  c.src_trunc = 4.f; c.dst_trunc = 2.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "band"), "a default band above 1 m is refused like a given one");
  c.p.band = 1.f;
  expect(c.run(&a) == MRH_OK && a.band == 1.f && a.dist_max == 1.f, "band 1 is accepted; dist_max = min(band, 1)");
  c.p.band = 0.4f; c.p.dist_max = 0.05f; c.p.iterations = 64; c.p.min_samples = 7u; c.p.min_weight = 255u;
  c.p.pivot[0] = 1.f; c.p.pivot[1] = -2.f; c.p.pivot[2] = 3.f; c.p.extent = 0.5f;
  expect(c.run(&a) == MRH_OK && a.band == 0.4f && a.dist_max == 0.05f && a.iterations == 64 && a.min_samples == 7u && a.w_min == 255u, "given values are kept");
  expect(a.crop && a.extent == 0.5f && a.pivot[0] == 1.f && a.pivot[1] == -2.f && a.pivot[2] == 3.f, "pivot and extent are the caller's");
  c.p.extent = 0.f;
  expect(c.run(&a) == MRH_OK && !a.crop && a.pivot[0] == 0.f, "a pivot without an extent is not used");
  c.p.iterations = 1; c.p.min_weight = 1u;
  expect(c.run(&a) == MRH_OK && a.iterations == 1 && a.w_min == 1u, "one iteration");
  expect(sizeof(mrh_align_params) == 48 && sizeof(mrh_align_info) == 312, "struct sizes");
}

void refusals() {
  mrh_plan::Align a;
  { expect_msg(mrh_plan::align(msg, kWho, nullptr, kR, kT, true, false, true, 0.15f, 0, 1, 0.15f, 0, 1, &a), MRH_ERR_INVALID_ARG, "mrh_align_map: null argument"); }
  { Call c; c.R = nullptr; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: null argument"); }
  { Call c; c.t = nullptr; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: null argument"); }
  { Call c; c.have_out = false; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: null argument"); }
  { Call c; c.same_ctx = true; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: the destination is the source"); }
  { Call c; c.same_device = false; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: the two contexts are on different devices"); }
  { Call c; c.src_pending = 1; expect_msg(c.run(&a), MRH_ERR_STATE, "mrh_align_map: an exchange is pending (call mrh_integrate_resume)"); }
  { Call c; c.dst_pending = 1; expect_msg(c.run(&a), MRH_ERR_STATE, "mrh_align_map: an exchange is pending (call mrh_integrate_resume)"); }
  { Call c; c.src_shards = 2; expect_msg(c.run(&a), MRH_ERR_UNSUPPORTED, "mrh_align_map: sharded maps are not aligned (shard_count 2)"); }
  { Call c; c.dst_shards = 4; expect_msg(c.run(&a), MRH_ERR_UNSUPPORTED, "mrh_align_map: sharded maps are not aligned to (shard_count 4)"); }
  for (int i = 0; i < 3; i++) { Call c; c.p.reserved[i] = 1u << (i * 15); expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: a reserved word is not 0"); }
  { Call c; c.p.min_weight = 256u; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: min_weight 256 (0 .. 255)"); }
  for (const float bad : {-0.1f, 1.0001f, kNaN, kInf, -kInf}) {
    { Call c; c.p.band = bad; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the band must lie in (0, 1] m"), "a bad band"); }
    { Call c; c.p.dist_max = bad; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the gate must lie in (0, 1] m"), "a bad dist_max"); }
  }
  for (const int bad : {-1, 65, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()}) {
    Call c; c.p.iterations = bad;
    expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "iterations (1 .. 64, 0 = 10)"), "a bad iteration count", bad);
  }
  for (int i = 0; i < 3; i++)
    for (const float bad : {kNaN, kInf, -kInf}) {
      Call c; c.p.pivot[i] = bad;
      expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: pivot is not finite");
    }
  for (const float bad : {-1.f, kNaN, kInf, std::numeric_limits<float>::max()}) {  // the last: 2 extent, the lever, is not finite
    Call c; c.p.extent = bad;
    expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "extent"), "a bad extent");
  }
  for (int i = 0; i < 12; i++)
    for (const float bad : {kNaN, kInf, -kInf}) {
      float R[9], t[3];
      memcpy(R, kR, sizeof R); memcpy(t, kT, sizeof t);
      (i < 9 ? R[i] : t[i - 9]) = bad;
      Call c; c.R = R; c.t = t;
      expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_align_map: pose is not finite");
    }
  { const float S[9] = {1.01f, 0, 0, 0, 1.01f, 0, 0, 0, 1.01f}; Call c; c.R = S; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not a rotation"), "a scaling is refused"); }
  { const float Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; Call c; c.R = Z; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not a rotation"), "a singular R is refused"); }
  { const float E[9] = {1.0005f, 0, 0, 0, 1, 0, 0, 0, 1}; Call c; c.R = E; expect(c.run(&a) == MRH_ERR_INVALID_ARG, "|R R^T - I| just above 2^-10"); }
  { const float E[9] = {1.0004f, 0, 0, 0, 1, 0, 0, 0, 1}; Call c; c.R = E; expect(c.run(&a) == MRH_OK, "... and just below"); }
}

void precedence() {
  mrh_plan::Align a;
  const float Rn[9] = {kNaN, 0, 0, 0, 1, 0, 0, 0, 1}, S[9] = {2, 0, 0, 0, 2, 0, 0, 0, 2};
  Call c;  // wrong in every respect
  c.have_out = false; c.same_ctx = true; c.same_device = false; c.src_pending = 1; c.src_shards = 2; c.dst_pending = 1; c.dst_shards = 2;
  c.p.reserved[2] = 1u; c.p.min_weight = 999u; c.p.band = -1.f; c.p.dist_max = 2.f; c.p.iterations = 99; c.p.pivot[1] = kNaN; c.p.extent = -1.f; c.R = Rn;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "null argument"), "null argument first");
  c.have_out = true;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the destination is the source"), "then dst == src");
  c.same_ctx = false;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "different devices"), "then the devices");
  c.same_device = true;
  expect(c.run(&a) == MRH_ERR_STATE, "then a pending exchange on the source");
  c.src_pending = 0;
  expect(c.run(&a) == MRH_ERR_UNSUPPORTED && strstr(msg, "are not aligned (shard"), "then a sharded source");
  c.src_shards = 1;
  expect(c.run(&a) == MRH_ERR_STATE, "then a pending exchange on the destination");
  c.dst_pending = 0;
  expect(c.run(&a) == MRH_ERR_UNSUPPORTED && strstr(msg, "are not aligned to"), "then a sharded destination");
  c.dst_shards = 1;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "reserved word"), "then the reserved words");
  c.p.reserved[2] = 0u;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "min_weight 999"), "then min_weight");
  c.p.min_weight = 0u;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the band"), "then the band");
  c.p.band = 0.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the gate"), "then dist_max");
  c.p.dist_max = 0.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "99 iterations"), "then the iterations");
  c.p.iterations = 0;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "pivot"), "then the pivot");
  c.p.pivot[1] = 0.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "extent"), "then the extent");
  c.p.extent = 0.f;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not finite"), "then the pose");
  c.R = S;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not a rotation"), "then the rotation");
  c.R = kR;
  expect(c.run(&a) == MRH_OK, "and then it runs");
}

void sample_cap() {
  uint64_t bytes = 0;
  expect(mrh_plan::align_sample_bytes(msg, kWho, 0, &bytes) == MRH_OK && bytes == 0, "no sample, no byte");
  expect(mrh_plan::align_sample_bytes(msg, kWho, 18635, &bytes) == MRH_OK && bytes == 18635ull * 16, "16 bytes a sample", (long long) bytes);
  expect(mrh_plan::align_sample_bytes(msg, kWho, 1ull << 26, &bytes) == MRH_OK && bytes == 1ull << 30, "2^26 samples fit", (long long) bytes);
  expect_msg(mrh_plan::align_sample_bytes(msg, kWho, (1ull << 26) + 1, &bytes), MRH_ERR_CAPACITY, "mrh_align_map: 67108865 source samples in one call (limit 2^26)");
  expect(mrh_plan::align_sample_bytes(msg, kWho, 0xFFFFFFFFFFFFFFFFull, &bytes) == MRH_ERR_CAPACITY, "a count beyond 64 bits of bytes is refused, not wrapped");
  // the bounds the header states, with |J~| < 2^15, |e~| <= 2^18 and 2^26 samples
  const long long J = (1ll << 15) - 1, E = 1ll << 18, n = 1ll << 26;
  expect(J * J < (1ll << 30) && (1ll << 30) * n == (1ll << 56) && J * E < (1ll << 33) && (1ll << 33) * n == (1ll << 59) && E * E == (1ll << 36) &&
             (1ll << 36) * n == (1ll << 62),
         "the sums fit a signed 64-bit word");
}

void pivots() {
  float c[3], e = 0.f;
  { const int lo[3] = {-24, -16, -8}, hi[3] = {23, 27, 12};
    mrh_plan::align_auto_pivot(lo, hi, 0.05f, c, &e);
    expect(c[0] == -1.f * 0.05f && c[1] == 5.f * 0.05f && c[2] == 2.f * 0.05f && e == 24.f * 0.05f, "the box of the corner scene"); }
  { const int lo[3] = {-7, 0, 1}, hi[3] = {-4, 3, 2};  // -11 >> 1 = -6: the shift rounds down
    mrh_plan::align_auto_pivot(lo, hi, 0.05f, c, &e);
    expect(c[0] == -6.f * 0.05f && c[1] == 1.f * 0.05f && c[2] == 1.f * 0.05f && e == 2.f * 0.05f, "an odd negative sum"); }
  { const int big = 1 << 23, lo[3] = {big - 1, -big, 5}, hi[3] = {big, -big + 9, 5};  // the sum of two coordinates leaves 32 bits
    const int lo2[3] = {std::numeric_limits<int>::max() - 1, std::numeric_limits<int>::min(), 0}, hi2[3] = {std::numeric_limits<int>::max(), std::numeric_limits<int>::min() + 2, 0};
    mrh_plan::align_auto_pivot(lo, hi, 1.f, c, &e);
    expect(c[0] == (float) (big - 1) && c[1] == (float) (-big + 4) && c[2] == 5.f && e == 5.f, "far from the origin");
    mrh_plan::align_auto_pivot(lo2, hi2, 1.f, c, &e);
    expect(c[0] == (float) 2147483646ll && c[1] == (float) -2147483647ll && e == 2.f, "a 64-bit sum"); }
  { const int v[3] = {3, -3, 0};
    mrh_plan::align_auto_pivot(v, v, 0.1f, c, &e);
    expect(c[0] == 3.f * 0.1f && c[1] == -3.f * 0.1f && c[2] == 0.f && e == 0.1f, "a single sample: one voxel of extent"); }
  // tau = R c + t and back: exact for the identity, within binary64 rounding for a rotation
  double R[9], t[3] = {kT[0], kT[1], kT[2]}, tau[3], back[3];
  const float piv[3] = {0.1f, 0.2f, -0.05f};
  for (int i = 0; i < 9; i++) R[i] = (double) kR[i];
  mrh_plan::align_tau(R, piv, t, tau);
  mrh_plan::align_t(R, piv, tau, back);
  for (int i = 0; i < 3; i++) {
    const double row = ((R[3 * i] * (double) piv[0] + R[3 * i + 1] * (double) piv[1]) + R[3 * i + 2] * (double) piv[2]) + t[i];
    expect(tau[i] == row && std::fabs(back[i] - t[i]) < 1e-15 && (float) back[i] == kT[i], "tau and back", i);
  }
}

}  // namespace

int main() {
  defaults();
  refusals();
  precedence();
  sample_cap();
  pivots();
  printf("alignplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
