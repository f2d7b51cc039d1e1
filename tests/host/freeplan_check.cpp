// freeplan_check.cpp — the argument plans of the free-space layer (mrh_plan::freespace_create / _carve / _box / _segments,
// mrhash_amd/csrc/mrh_readerplan.h) on their own: a plain C++17 program that includes the header alone, for
// tests/test_freespaceplan.py (g++ -ffp-contract=off, ASan + UBSan).
//
// Checked: per plan the order of the refusals with each case's error code (null argument -> pending -> sharded -> no layer ->
// the limits in the order the header lists them), every limit on both sides of its edge, the defaults (half a cell, the
// context's weight), the sample count against a literal march, the word shape of a layer, the voxel box of a cell box and the
// refusal bound (float) (1 << 20) * vs; the messages the GPU tests compare mrh_last_error with, literally.
// stdout: one line per failure, then "freeplan_check: <n> failures".
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
const float kVs = 0.02f;
const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

uint32_t literal_count(const float lo, const float hi, const float step) {
  uint32_t k = 0;
  while (lo + (float) k * step <= hi) k++;
  return k;
}

// ---- mrh_freespace_create ----
const mrh_freespace_params kLayer = {{-20, -20, -20}, {40, 33, 65}, 3, 0u};
int create(const mrh_freespace_params& p, mrh::FreeLayer* L, const int pending = 0, const int shards = 1) {
  return mrh_plan::freespace_create(msg, "mrh_freespace_create", &p, pending, shards, L);
}

void check_create() {
  mrh::FreeLayer L;
  expect(create(kLayer, &L) == MRH_OK && L.ox == -20 && L.nx == 40 && L.ny == 33 && L.nz == 65 && L.shift == 3, "a layer is carried as given");
  expect(L.nbx == 10 && L.nby == 9 && L.n_words == 10u * 9u * 33u, "words are 4 x 4 x 2 bricks", L.n_words);
  mrh_freespace_params p = kLayer;
  // the order: every later fault is present as well
  p.reserved = 1u; p.cell_shift = 4; p.dims[0] = 0;
  expect_msg(mrh_plan::freespace_create(msg, "mrh_freespace_create", nullptr, 1, 2, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: null argument");
  expect_msg(create(p, &L, 1, 2), MRH_ERR_STATE, "mrh_freespace_create: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(create(p, &L, 0, 2), MRH_ERR_UNSUPPORTED, "mrh_freespace_create: sharded maps have no free-space layer (shard_count 2)");
  expect_msg(create(p, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: a reserved word is not 0");
  p.reserved = 0u;
  expect_msg(create(p, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: cell_shift 4 (0 .. 3)");
  p.cell_shift = -1;
  expect_msg(create(p, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: cell_shift -1 (0 .. 3)");
  p.cell_shift = 0;
  expect_msg(create(p, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: layer of 0 x 33 x 65 cells (1 .. 1024 per side)");
  p.dims[0] = 1025;
  expect(create(p, &L) == MRH_ERR_INVALID_ARG, "1025 cells per side are refused");
  // the edges: 1 and 1024 per side, 2^28 cells, the voxel span
  p = {{0, 0, 0}, {1, 1, 1}, 0, 0u};
  expect(create(p, &L) == MRH_OK && L.n_words == 1u, "one cell is one word");
  p = {{-512, -512, -128}, {1024, 1024, 256}, 0, 0u};
  expect(create(p, &L) == MRH_OK && L.n_words == 256u * 256u * 128u, "2^28 cells are accepted", L.n_words);
  p.dims[2] = 257;
  expect_msg(create(p, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: layer of 269484032 cells (limit 2^28)");
  p = {{-(1 << 20), 0, (1 << 20) - 8}, {8, 8, 8}, 3, 0u};
  expect(create(p, &L) == MRH_OK, "voxels -2^23 and 2^23 - 1 are the edges");
  p.origin[0] = -(1 << 20) - 1;
  expect_msg(create(p, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: axis 0 of the layer spans voxels -8388616 .. -8388553, outside [-2^23, 2^23)");
  p.origin[0] = 0; p.origin[2] = (1 << 20) - 7;
  expect_msg(create(p, &L), MRH_ERR_INVALID_ARG, "mrh_freespace_create: axis 2 of the layer spans voxels 8388552 .. 8388615, outside [-2^23, 2^23)");
  p = {{2147483647, 0, 0}, {1024, 1, 1}, 3, 0u};
  expect(create(p, &L) == MRH_ERR_INVALID_ARG, "an origin at INT32_MAX is refused without overflow");
}

// ---- the carves ----
const mrh_carve_params kCarve = {500.f, 480.f, 11.5f, 7.5f, 16, 24, 0.1f, 3.f, 0.f, 0.f, {0u, 0u}};
int carve(const mrh_carve_params& p, const bool depth_form, const uint64_t n, mrh::CarveArgs* a, const bool have_layer = true, const int pending = 0,
          const int shards = 1, const int shift = 3, const float* R = kR, const float* t = kT, const bool have_obs = true) {
  return mrh_plan::freespace_carve(msg, depth_form ? "mrh_freespace_carve_depth" : "mrh_freespace_carve_points", depth_form, &p, have_obs, n, R, t, have_layer, kVs,
                                   shift, pending, shards, a);
}

void check_carve() {
  mrh::CarveArgs a;
  expect(carve(kCarve, true, 0, &a) == MRH_OK && a.cam.rows == 16 && a.cam.cols == 24 && a.cam.ifx == 1.0f / 500.f && a.cam.ify == 1.0f / 480.f, "the depth form's camera");
  expect(a.cam.step == 0.5f * (kVs * 8.f) && a.margin == 0.f && a.bound == 1048576.f * kVs, "step 0 is half a cell, the bound (float) (1 << 20) * vs");
  expect(a.cam.n_samples == literal_count(0.1f, 3.f, 0.5f * (kVs * 8.f)), "the sample count is the literal march's", a.cam.n_samples);
  expect(!memcmp(a.cam.R, kR, sizeof kR) && !memcmp(a.cam.t, kT, sizeof kT), "the pose is carried as given");
  expect(carve(kCarve, true, 0, &a, true, 0, 1, 0) == MRH_OK && a.cam.step == 0.5f * (kVs * 1.f), "half a cell at s = 0");
  mrh_carve_params p = kCarve;
  p.rows = 0; p.fx = 0.f;  // the points form ignores fx .. cols
  expect(carve(p, false, 65, &a) == MRH_OK && a.n == 65u && a.cam.rows == 0 && a.cam.cols == 0 && a.cam.ifx == 0.f, "the points form ignores the camera", a.n);
  expect(carve(kCarve, false, 0, &a, true, 0, 1, 3, kR, kT, false) == MRH_OK && a.n == 0u, "an empty cloud needs no list");
  expect(carve(kCarve, false, MRH_FREESPACE_MAX_POINTS, &a) == MRH_OK && a.n == MRH_FREESPACE_MAX_POINTS, "2^24 points are accepted", a.n);
  for (const float step : {0.1f, 0.075f, 0.013f, 1.f, 7.f})
    for (const float lo : {0.f, 0.1f, 2.5f}) {
      p = kCarve; p.step = step; p.min_depth = lo;
      expect(carve(p, true, 0, &a) == MRH_OK && a.cam.n_samples == literal_count(lo, 3.f, step) && a.cam.step == step, "sample counts", a.cam.n_samples, literal_count(lo, 3.f, step));
    }
  p = kCarve; p.min_depth = 0.f; p.max_depth = 1048575.f; p.step = 1.f;
  expect(carve(p, true, 0, &a) == MRH_OK && a.cam.n_samples == (1u << 20), "2^20 samples are accepted", a.cam.n_samples);
  p.max_depth = 1048576.f;
  expect_msg(carve(p, true, 0, &a), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: more than 2^20 samples per ray (min_depth 0, max_depth 1.04858e+06, step 1)");

  // the order: every later fault is present as well
  p = kCarve;
  p.reserved[1] = 1u; p.rows = 0; p.fx = nan; p.min_depth = -1.f; p.margin = -1.f; p.step = -1.f;
  const float Rn[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 1};
  expect_msg(mrh_plan::freespace_carve(msg, "mrh_freespace_carve_depth", true, nullptr, true, 0, Rn, kT, false, kVs, 3, 1, 2, &a), MRH_ERR_INVALID_ARG,
             "mrh_freespace_carve_depth: null argument");
  expect_msg(carve(p, true, 0, &a, false, 1, 2, 3, Rn, kT, false), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: null argument");
  expect_msg(carve(p, true, 0, &a, false, 1, 2, 3, nullptr), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: null argument");
  expect_msg(carve(p, false, 1, &a, false, 1, 2, 3, Rn, kT, false), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_points: null argument");
  expect_msg(carve(p, false, (1ull << 24) + 1, &a, false, 1, 2, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_points: 16777217 points in one call (limit 2^24)");
  expect_msg(carve(p, true, 0, &a, false, 1, 2, 3, Rn), MRH_ERR_STATE, "mrh_freespace_carve_depth: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(carve(p, true, 0, &a, false, 0, 2, 3, Rn), MRH_ERR_UNSUPPORTED, "mrh_freespace_carve_depth: sharded maps have no free-space layer (shard_count 2)");
  expect_msg(carve(p, true, 0, &a, false, 0, 1, 3, Rn), MRH_ERR_STATE, "mrh_freespace_carve_depth: the context has no free-space layer (call mrh_freespace_create)");
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: a reserved word is not 0");
  p.reserved[1] = 0u;
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: image of 0 x 24 pixels (1 .. 4096 per side)");
  p.rows = 16;
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: bad intrinsics");
  p.fx = 500.f;
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: need 0 <= min_depth < max_depth (got -1, 3)");
  p.min_depth = 3.f;
  expect(carve(p, true, 0, &a, true, 0, 1, 3, Rn) == MRH_ERR_INVALID_ARG && strstr(msg, "need 0 <= min_depth < max_depth"), "min_depth == max_depth is refused");
  p.min_depth = 0.f; p.max_depth = inf;
  expect(carve(p, true, 0, &a, true, 0, 1, 3, Rn) == MRH_ERR_INVALID_ARG && strstr(msg, "need 0 <= min_depth < max_depth"), "an infinite max_depth is refused");
  p.max_depth = 3.f;  // min_depth == 0 is accepted: the next fault is the margin's
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: margin -1");
  p.margin = inf;
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: margin inf");
  p.margin = 0.05f;
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: the sample spacing must be > 0 (step -1)");
  p.step = 0.f;
  expect_msg(carve(p, true, 0, &a, true, 0, 1, 3, Rn), MRH_ERR_INVALID_ARG, "mrh_freespace_carve_depth: pose is not finite");
  expect(carve(p, true, 0, &a) == MRH_OK && a.margin == 0.05f && a.cam.min_depth == 0.f, "min_depth 0 and a margin are accepted");
}

// ---- the box ----
const mrh_freespace_box_params kBox = {{-21, -21, -21}, {42, 35, 67}, 0, 0.f, {0u, 0u}};
int box(const mrh_freespace_box_params& p, mrh::FreeBox* b, const bool have_layer = true, const int pending = 0, const int shards = 1, const int shift = 3,
        const bool have_out = true) {
  return mrh_plan::freespace_box(msg, "mrh_freespace_box", &p, have_out, have_layer, shift, 2, pending, shards, b);
}

void check_box() {
  mrh::FreeBox b;
  expect(box(kBox, &b) == MRH_OK && b.ox == -21 && b.nx == 42 && b.ny == 35 && b.nz == 67, "a box is carried as given");
  expect(b.vox.ox == -168 && b.vox.oy == -168 && b.vox.nx == 336 && b.vox.ny == 280 && b.vox.nz == 536, "the voxel box is the cell box << s", b.vox.ox, b.vox.nx);
  expect(b.vox.w_min == 2 && b.vox.band == 0.f, "min_weight 0 is the context's threshold, the band is passed on");
  mrh_freespace_box_params p = kBox;
  p.min_weight = 5; p.surface_band = 0.03f;
  expect(box(p, &b, true, 0, 1, 1) == MRH_OK && b.vox.w_min == 5 && b.vox.band == 0.03f && b.vox.ox == -42 && b.vox.nz == 134, "explicit gates, s = 1");
  p = kBox;
  p.reserved[0] = 1u; p.dims[1] = 513; p.surface_band = -1.f; p.min_weight = -1;
  expect_msg(mrh_plan::freespace_box(msg, "mrh_freespace_box", nullptr, true, false, 3, 2, 1, 2, &b), MRH_ERR_INVALID_ARG, "mrh_freespace_box: null argument");
  expect_msg(box(p, &b, false, 1, 2, 3, false), MRH_ERR_INVALID_ARG, "mrh_freespace_box: null argument");
  expect_msg(box(p, &b, false, 1, 2), MRH_ERR_STATE, "mrh_freespace_box: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(box(p, &b, false, 0, 2), MRH_ERR_UNSUPPORTED, "mrh_freespace_box: sharded maps have no free-space layer (shard_count 2)");
  expect_msg(box(p, &b, false), MRH_ERR_STATE, "mrh_freespace_box: the context has no free-space layer (call mrh_freespace_create)");
  expect_msg(box(p, &b), MRH_ERR_INVALID_ARG, "mrh_freespace_box: a reserved word is not 0");
  p.reserved[0] = 0u;
  expect_msg(box(p, &b), MRH_ERR_INVALID_ARG, "mrh_freespace_box: box of 42 x 513 x 67 cells (1 .. 512 per side)");
  p.dims[1] = 512;
  expect_msg(box(p, &b), MRH_ERR_INVALID_ARG, "mrh_freespace_box: surface_band -1");
  p.surface_band = nan;
  expect(box(p, &b) == MRH_ERR_INVALID_ARG && strstr(msg, "surface_band"), "a NaN band is refused");
  p.surface_band = 0.f;
  expect_msg(box(p, &b), MRH_ERR_INVALID_ARG, "mrh_freespace_box: min_weight -1");
  p.min_weight = 0;
  expect(box(p, &b) == MRH_OK, "512 cells per side are accepted");
  p.dims[1] = 0;
  expect(box(p, &b) == MRH_ERR_INVALID_ARG, "0 cells per side are refused");
  p = {{-(1 << 20), 0, (1 << 20) - 512}, {512, 1, 512}, 0, 0.f, {0u, 0u}};
  expect(box(p, &b) == MRH_OK && b.vox.ox == -(1 << 23) && b.vox.nz == 4096, "voxels -2^23 and 2^23 - 1 are the edges", b.vox.ox);
  p.origin[2]++;
  expect_msg(box(p, &b), MRH_ERR_INVALID_ARG, "mrh_freespace_box: axis 2 of the box spans voxels 8384520 .. 8388615, outside [-2^23, 2^23)");
  p.origin[2]--; p.origin[0]--;
  expect(box(p, &b) == MRH_ERR_INVALID_ARG && strstr(msg, "axis 0"), "one cell below -2^23 is refused");
}

// ---- the segments ----
int segs(const uint64_t n, const float step, mrh::SegArgs* a, const bool have_layer = true, const int pending = 0, const int shards = 1, const int shift = 3,
         const bool have_in = true, const bool have_out = true) {
  return mrh_plan::freespace_segments(msg, "mrh_freespace_segments", have_in, have_out, n, step, have_layer, kVs, shift, pending, shards, a);
}

void check_segments() {
  mrh::SegArgs a;
  expect(segs(65, 0.f, &a) == MRH_OK && a.n == 65u && a.step == 0.5f * (kVs * 8.f) && a.bound == 1048576.f * kVs, "step 0 is half a cell");
  expect(segs(1, 0.25f, &a, true, 0, 1, 1) == MRH_OK && a.step == 0.25f, "an explicit step");
  expect(segs(0, 0.f, &a, true, 0, 1, 3, false) == MRH_OK && a.n == 0u, "n = 0 needs no lists");
  expect(segs(MRH_FREESPACE_MAX_POINTS, 0.f, &a) == MRH_OK, "2^24 segments are accepted");
  expect_msg(segs((1ull << 24) + 1, -1.f, &a, false, 1, 2, 3, false), MRH_ERR_INVALID_ARG, "mrh_freespace_segments: null argument");
  expect_msg(segs((1ull << 24) + 1, -1.f, &a, false, 1, 2, 3, true, false), MRH_ERR_INVALID_ARG, "mrh_freespace_segments: null argument");
  expect_msg(segs((1ull << 24) + 1, -1.f, &a, false, 1, 2), MRH_ERR_STATE, "mrh_freespace_segments: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(segs((1ull << 24) + 1, -1.f, &a, false, 0, 2), MRH_ERR_UNSUPPORTED, "mrh_freespace_segments: sharded maps have no free-space layer (shard_count 2)");
  expect_msg(segs((1ull << 24) + 1, -1.f, &a, false), MRH_ERR_STATE, "mrh_freespace_segments: the context has no free-space layer (call mrh_freespace_create)");
  expect_msg(segs((1ull << 24) + 1, -1.f, &a), MRH_ERR_INVALID_ARG, "mrh_freespace_segments: 16777217 segments in one call (limit 2^24)");
  expect_msg(segs(1, -1.f, &a), MRH_ERR_INVALID_ARG, "mrh_freespace_segments: the sample spacing must be > 0 (step -1)");
  expect(segs(1, nan, &a) == MRH_ERR_INVALID_ARG && segs(1, inf, &a) == MRH_ERR_INVALID_ARG, "a step that is not finite is refused");
}

void check_layer_calls() {
  expect_msg(mrh_plan::freespace_layer(msg, "mrh_freespace_clear", false, 1, 2), MRH_ERR_STATE, "mrh_freespace_clear: an exchange is pending (call mrh_integrate_resume)");
  expect_msg(mrh_plan::freespace_layer(msg, "mrh_freespace_clear", false, 0, 2), MRH_ERR_UNSUPPORTED, "mrh_freespace_clear: sharded maps have no free-space layer (shard_count 2)");
  expect_msg(mrh_plan::freespace_layer(msg, "mrh_freespace_destroy", false, 0, 1), MRH_ERR_STATE,
             "mrh_freespace_destroy: the context has no free-space layer (call mrh_freespace_create)");
  expect(mrh_plan::freespace_layer(msg, "mrh_freespace_clear", true, 0, 1) == MRH_OK, "a layer is enough");
  for (const float vs : {0.05f, 0.0625f, 0.02f, 1e-3f})
    for (int s = 0; s <= 3; s++) expect(mrh_plan::freespace_half_cell(vs, s) == 0.5f * (vs * (float) (1 << s)), "half a cell", s);
}

}  // namespace

int main() {
  check_create();
  check_carve();
  check_box();
  check_segments();
  check_layer_calls();
  printf("freeplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
