// remapplan_check.cpp — the argument and size plan of map-to-map fusion (mrh_plan::remap, remap_per_axis, remap_slots,
// remap_record_bytes; mrhash_amd/csrc/mrh_readerplan.h) on its own: a plain C++17 program that includes the header alone, for
// tests/test_remapplan.py (g++ -ffp-contract=off, ASan + UBSan).
//
// Checked: every refusal of include/mrhash_remap.h with its code and, where the C ABI's text is fixed, its message; the order
// null argument -> dst == src -> devices -> pending (either) -> sharded (either) -> reserved words -> min_weight -> finite pose ->
// rotation -> voxel sizes; the ratio limits on both sides; the kernels' arguments (pose as given, the binary64 inverse of R^T, the
// bound, w_min, the destination voxel size); the worst-case candidate counts at ratios 1/4, 1 and 4, re-derived here from the box
// of a source block; the overflow guards of the slot and record counts.
// stdout: one line per failure, then "remapplan_check: <n> failures".
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
const char* kWho = "mrh_fuse_map";
const mrh_remap_params kGood = {0.f, 0u, {0u, 0u}};

struct Call {
  mrh_remap_params p = kGood;
  const float* R = kR; const float* t = kT;
  bool have_out = true;
  float src_vs = 0.05f; int src_pending = 0, src_shards = 1;
  bool fuse = false, same_ctx = false, same_device = true;
  float dst_vs = 0.05f; int dst_pending = 0, dst_shards = 1;
  int run(mrh::RemapArgs* a, const char* who = kWho) const {
    return mrh_plan::remap(msg, who, &p, R, t, have_out, src_vs, src_pending, src_shards, fuse, same_ctx, same_device, dst_vs, dst_pending, dst_shards, a);
  }
};

void arguments() {
  mrh::RemapArgs a;
  Call c;
  expect(c.run(&a) == MRH_OK, "a resample call with every default");
  expect(!memcmp(a.R, kR, sizeof kR) && !memcmp(a.t, kT, sizeof kT), "the pose is carried as given");
  expect(a.vs_d == 0.05f && a.bound == 1048576.f * 0.05f && a.w_min == 1u && a.per_axis == 4, "vs_d, bound, w_min, per_axis", a.per_axis);
  // F = (R^T)^-1: F R^T = I to binary64 rounding, and F is R to binary32 rounding for a rotation
  double worst = 0.0, off = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += a.F[3 * i + k] * (double) kR[3 * j + k];  // (R^T)_kj = R_jk
      worst = std::fmax(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
      off = std::fmax(off, std::fabs(a.F[3 * i + j] - (double) kR[3 * i + j]));
    }
  expect(worst < 1e-14 && off < 1e-6, "F inverts R^T", (long long) (worst * 1e18), (long long) (off * 1e9));
  c.p.min_weight = 3u; c.p.dst_voxel_size = 0.1f;
  expect(c.run(&a) == MRH_OK && a.w_min == 3u && a.vs_d == 0.1f && a.per_axis == mrh_plan::remap_per_axis(0.1f / (double) 0.05f), "min_weight and dst_voxel_size", a.per_axis);
  c.p.min_weight = 255u;
  expect(c.run(&a) == MRH_OK && a.w_min == 255u, "min_weight 255 is accepted");
  Call f;
  f.fuse = true; f.dst_vs = 0.025f;
  expect(f.run(&a) == MRH_OK && a.vs_d == 0.025f, "a fuse call resamples at the destination's voxel size");
  f.p.dst_voxel_size = 0.025f;
  expect(f.run(&a) == MRH_OK && a.vs_d == 0.025f, "... which dst_voxel_size may repeat");
}

void refusals() {
  mrh::RemapArgs a;
  { expect_msg(mrh_plan::remap(msg, kWho, nullptr, kR, kT, true, 0.05f, 0, 1, false, false, true, 0.05f, 0, 1, &a), MRH_ERR_INVALID_ARG, "mrh_fuse_map: null argument"); }
  { Call c; c.R = nullptr; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_fuse_map: null argument"); }
  { Call c; c.t = nullptr; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_fuse_map: null argument"); }
  { Call c; c.have_out = false; expect_msg(c.run(&a, "mrh_resample_map"), MRH_ERR_INVALID_ARG, "mrh_resample_map: null argument"); }
  { Call c; c.fuse = true; c.same_ctx = true; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_fuse_map: the destination is the source"); }
  { Call c; c.fuse = true; c.same_device = false; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_fuse_map: the two contexts are on different devices"); }
  { Call c; c.same_ctx = true; c.same_device = false; expect(c.run(&a) == MRH_OK, "a resample call has no destination to compare with"); }
  { Call c; c.src_pending = 1; expect_msg(c.run(&a), MRH_ERR_STATE, "mrh_fuse_map: an exchange is pending (call mrh_integrate_resume)"); }
  { Call c; c.fuse = true; c.dst_pending = 1; expect_msg(c.run(&a), MRH_ERR_STATE, "mrh_fuse_map: an exchange is pending (call mrh_integrate_resume)"); }
  { Call c; c.dst_pending = 1; expect(c.run(&a) == MRH_OK, "the destination's state does not matter to a resample call"); }
  { Call c; c.src_shards = 2; expect_msg(c.run(&a), MRH_ERR_UNSUPPORTED, "mrh_fuse_map: sharded maps are not resampled (shard_count 2)"); }
  { Call c; c.fuse = true; c.dst_shards = 4; expect_msg(c.run(&a), MRH_ERR_UNSUPPORTED, "mrh_fuse_map: sharded maps take no resampled map (shard_count 4)"); }
  { Call c; c.p.reserved[0] = 1u; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_fuse_map: a reserved word is not 0"); }
  { Call c; c.p.reserved[1] = 0x80000000u; expect(c.run(&a) == MRH_ERR_INVALID_ARG, "the other reserved word too"); }
  { Call c; c.p.min_weight = 256u; expect_msg(c.run(&a), MRH_ERR_INVALID_ARG, "mrh_fuse_map: min_weight 256 (0 .. 255)"); }
  for (int i = 0; i < 12; i++)
    for (const float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()}) {
      float R[9], t[3];
      memcpy(R, kR, sizeof R); memcpy(t, kT, sizeof t);
      (i < 9 ? R[i] : t[i - 9]) = bad;
      Call c; c.R = R; c.t = t;
      expect(c.run(&a) == MRH_ERR_INVALID_ARG && !strcmp(msg, "mrh_fuse_map: pose is not finite"), "a pose that is not finite is refused", i);
    }
  { const float S[9] = {1.01f, 0, 0, 0, 1.01f, 0, 0, 0, 1.01f}; Call c; c.R = S; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not a rotation"), "a scaling is refused"); }
  { const float Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; Call c; c.R = Z; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not a rotation"), "a singular R is refused"); }
  { const float M[9] = {1, 0, 0, 0, 1, 0, 0, 0, -1}; Call c; c.R = M; expect(c.run(&a) == MRH_OK && a.F[8] == -1.0, "a reflection is orthonormal: accepted"); }
  { Call c; c.p.dst_voxel_size = -0.05f; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "dst_voxel_size"), "a negative voxel size"); }
  { Call c; c.p.dst_voxel_size = std::numeric_limits<float>::quiet_NaN(); expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "dst_voxel_size"), "a NaN voxel size"); }
  { Call c; c.fuse = true; c.p.dst_voxel_size = 0.06f; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "contradicts the destination's"), "dst_voxel_size against dst"); }
}

void ratios() {
  mrh::RemapArgs a;
  for (const float vs_d : {0.0125f, 0.02f, 0.05f, 0.1f, 0.2f}) {
    Call c; c.p.dst_voxel_size = vs_d;
    expect(c.run(&a) == MRH_OK && a.vs_d == vs_d, "ratios 1/4 .. 4 are accepted", (long long) (vs_d * 1e6f));
  }
  for (const float vs_d : {0.0124f, 0.2001f, 1.f, 1e-6f}) {
    Call c; c.p.dst_voxel_size = vs_d;
    expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the ratio must lie in [1/4, 4]"), "ratios outside are refused", (long long) (vs_d * 1e6f));
  }
  { Call c; c.fuse = true; c.dst_vs = 0.25f; expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "ratio"), "... between two contexts as well"); }
  { Call c; c.src_vs = 0.0625f; c.p.dst_voxel_size = 0.25f; expect(c.run(&a) == MRH_OK && a.per_axis == 3, "exactly 4", a.per_axis); }
  { Call c; c.src_vs = 0.0625f; c.p.dst_voxel_size = 0.015625f; expect(c.run(&a) == MRH_OK && a.per_axis == 12, "exactly 1/4", a.per_axis); }
}

// The box of one source block, in destination blocks, re-derived: side 8 source voxels (+ 2 beyond the shift limit), its
// axis-aligned bound at most sqrt(3) (1 + 2^-9) times wider, + 2 (1 destination voxel + 1/2 destination voxel + 1.75 source voxels)
// of margin; an interval of length L meets at most floor(L) + 2 cells
int per_axis_here(const double r) {
  const double side = 10.0 * std::sqrt(3.0) * (1.0 + std::ldexp(1.0, -9)) / r, margin = 1.0 + 0.5 + 1.75 / r;
  return (int) std::floor((side + 2.0 * margin) / 8.0) + 2;
}

void worst_cases() {
  expect(mrh_plan::remap_per_axis(0.25) == 12 && mrh_plan::remap_per_axis(1.0) == 4 && mrh_plan::remap_per_axis(4.0) == 3, "per-axis counts at 1/4, 1 and 4",
         mrh_plan::remap_per_axis(0.25), mrh_plan::remap_per_axis(1.0));
  for (double r = 0.25; r <= 4.0; r += 1.0 / 64.0) {
    const int n = mrh_plan::remap_per_axis(r);
    expect(n == per_axis_here(r) && n >= 3 && n <= 12, "per-axis count re-derived", n, (long long) (r * 64));
    if (r > 0.25) expect(n <= mrh_plan::remap_per_axis(r - 1.0 / 64.0), "monotone in the ratio", n);
  }
  uint64_t slots = 0, bytes = 0;
  expect(mrh_plan::remap_slots(msg, kWho, 14000, 4, &slots) == MRH_OK && slots == 14000ull * 64, "slots of a 14 k-block map at ratio 1", (long long) slots);
  expect(mrh_plan::remap_slots(msg, kWho, 1, 12, &slots) == MRH_OK && slots == 1728, "slots at ratio 1/4", (long long) slots);
  expect(mrh_plan::remap_slots(msg, kWho, 1, 3, &slots) == MRH_OK && slots == 27, "slots at ratio 4", (long long) slots);
  expect(mrh_plan::remap_slots(msg, kWho, 0, 4, &slots) == MRH_OK && slots == 0, "no source block, no slot");
  // 2^31 - 1 slots: the last count that fits, and the first that does not
  expect(mrh_plan::remap_slots(msg, kWho, 33554431, 4, &slots) == MRH_OK && slots == 33554431ull * 64, "33 554 431 blocks x 64 fit", (long long) slots);
  expect_msg(mrh_plan::remap_slots(msg, kWho, 33554432, 4, &slots), MRH_ERR_CAPACITY, "mrh_fuse_map: 33554432 source blocks with 64 candidate slots each (limit 2^31 - 1 slots)");
  expect(mrh_plan::remap_slots(msg, kWho, 1ull << 62, 12, &slots) == MRH_ERR_CAPACITY, "a product beyond 64 bits is refused, not wrapped");
  expect(mrh_plan::remap_slots(msg, kWho, 0xFFFFFFFFFFFFFFFFull, 3, &slots) == MRH_ERR_CAPACITY, "... whatever the count");
  expect(mrh_plan::remap_slots(msg, kWho, 10, 0, &slots) == MRH_ERR_CAPACITY && mrh_plan::remap_slots(msg, kWho, 10, 65, &slots) == MRH_ERR_CAPACITY, "a per-axis count outside 1 .. 64");
  expect(mrh_plan::remap_record_bytes(msg, kWho, 0x7FFFFFFFull, &bytes) == MRH_OK && bytes == 0x7FFFFFFFull * 6160ull, "2^31 - 1 records", (long long) bytes);
  expect_msg(mrh_plan::remap_record_bytes(msg, kWho, 0x80000000ull, &bytes), MRH_ERR_CAPACITY, "mrh_fuse_map: 2147483648 records in one call (limit 2^31 - 1)");
  expect(mrh_plan::remap_record_bytes(msg, kWho, 14000, &bytes) == MRH_OK && bytes == 86240000ull, "14 k records are 86 MB", (long long) bytes);
  expect(sizeof(mrh_block_record) == mrh_plan::kRemapRecordBytes && sizeof(mrh_remap_params) == 16 && sizeof(mrh_remap_info) == 40, "struct sizes");
}

void precedence() {
  mrh::RemapArgs a;
  const float nan = std::numeric_limits<float>::quiet_NaN(), Rn[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 1};
  Call c;  // wrong in every respect
  c.fuse = true; c.same_ctx = true; c.same_device = false; c.src_pending = 1; c.dst_pending = 1; c.src_shards = 2; c.dst_shards = 2;
  c.p.reserved[0] = 1u; c.p.min_weight = 999u; c.R = Rn; c.p.dst_voxel_size = 7.f;
  c.have_out = false;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "null argument"), "null argument first");
  c.have_out = true;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "the destination is the source"), "then dst == src");
  c.same_ctx = false;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "different devices"), "then the devices");
  c.same_device = true;
  expect(c.run(&a) == MRH_ERR_STATE, "then a pending exchange on the source");
  c.src_pending = 0;
  expect(c.run(&a) == MRH_ERR_UNSUPPORTED && strstr(msg, "are not resampled"), "then a sharded source");
  c.src_shards = 1;
  expect(c.run(&a) == MRH_ERR_STATE, "then a pending exchange on the destination");
  c.dst_pending = 0;
  expect(c.run(&a) == MRH_ERR_UNSUPPORTED && strstr(msg, "take no resampled map"), "then a sharded destination");
  c.dst_shards = 1;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "reserved word"), "then the reserved words");
  c.p.reserved[0] = 0u;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "min_weight 999"), "then min_weight");
  c.p.min_weight = 0u;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "not finite"), "then the pose");
  c.R = kR;
  expect(c.run(&a) == MRH_ERR_INVALID_ARG && strstr(msg, "contradicts"), "then the voxel size");
}

}  // namespace

int main() {
  arguments();
  refusals();
  ratios();
  worst_cases();
  precedence();
  printf("remapplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
