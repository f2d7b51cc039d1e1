// gw_check.cpp — the pure host parts of the GeoWrapper facade (mrhash_amd/csrc/gw_pose.h, gw_chunks.h, gw_files.h) on their own: a
// plain C++17 program that includes the three headers and nothing else of the facade, for tests/test_gw_host.py (g++
// -ffp-contract=off, ASan + UBSan).
//
// Checked — pose: identity, a quarter turn about each axis by hand, a non-unit quaternion against Eigen's unnormalised formula
// evaluated here, and quat_from(split_pose(pose_from(t, q)).R) == +-q for one unit quaternion per branch of quat_from, w >= 0.
// chunks: worldToChunks rounds half away from zero; a chunk the transparent sphere test takes and the reference's refuses; add /
// gather / erase / blocks of the grid; the extraction plan (empty, one chunk, inside the first sphere, a walk with its centres
// counted by hand, radiusi == 1, axes that fit but a chunk outside the sphere).  files: vertex and face rows against an iostream
// restatement written here, the file byte-identical for 1, 2 and 7 workers, MRHGRID1 round trips and its two refusals, the two
// serializeData clouds and the seeds PLY against text written out by hand.
// stdout: one line per failure, "gw_check: compared <n> doubles", then "gw_check: <n> failures".
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <sstream>

#include "gw_chunks.h"
#include "gw_files.h"
#include "gw_pose.h"

namespace {

int failures = 0;

void expect(const bool ok, const char* what, const double a = 0, const double b = 0) {
  if (ok) return;
  failures++;
  printf("FAILED %s (%.9g, %.9g)\n", what, a, b);
}
void expect_text(const std::string& got, const std::string& want, const char* what) {
  if (got == want) return;
  failures++;
  printf("FAILED %s:\n--- got\n%s\n--- expected\n%s\n", what, got.c_str(), want.c_str());
}

// ---- pose ----------------------------------------------------------------------------------------------------------------

void expect_rotation(const std::array<float, 16>& T, const double (&R)[9], const double tol, const char* what) {
  const gw::PoseRt p = gw::split_pose(T);
  for (int i = 0; i < 9; i++) expect(std::fabs((double) p.R[i] - R[i]) <= tol, what, p.R[i], R[i]);
}

void pose() {
  const std::array<float, 3> t = {1.f, -2.f, 3.5f};
  const std::array<float, 16> I = gw::pose_from(t, {0.f, 0.f, 0.f, 1.f});
  const std::array<float, 16> want_I = {1, 0, 0, 1.f, 0, 1, 0, -2.f, 0, 0, 1, 3.5f, 0, 0, 0, 1};
  expect(I == want_I, "identity");
  const gw::PoseRt split = gw::split_pose(I);
  expect(split.t[0] == 1.f && split.t[1] == -2.f && split.t[2] == 3.5f, "split_pose: translation");

  const float h = std::sqrt(0.5f);
  expect_rotation(gw::pose_from(t, {h, 0.f, 0.f, h}), {1, 0, 0, 0, 0, -1, 0, 1, 0}, 1e-6, "quarter turn about x");
  expect_rotation(gw::pose_from(t, {0.f, h, 0.f, h}), {0, 0, 1, 0, 1, 0, -1, 0, 0}, 1e-6, "quarter turn about y");
  expect_rotation(gw::pose_from(t, {0.f, 0.f, h, h}), {0, -1, 0, 1, 0, 0, 0, 0, 1}, 1e-6, "quarter turn about z");

  // no normalisation: Eigen's formula on the quaternion as given, evaluated here in double
  const double x = 0.2, y = -0.4, z = 0.6, w = 1.5;
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                       2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
  expect_rotation(gw::pose_from(t, {(float) x, (float) y, (float) z, (float) w}), R, 2e-6, "non-unit quaternion, unnormalised formula");
  expect(R[0] < 0.0, "the non-unit case is no rotation", R[0]);  // 1 - 2 * 0.52 = -0.04; the normalised quaternion gives 0.608

  // one unit quaternion per branch of quat_from: trace > 0, then m00, m11, m22 largest; then the first with its sign flipped
  const double q[5][4] = {{0.1, 0.2, 0.3, 0.9}, {0.99, 0.05, 0.08, 0.05}, {0.05, 0.99, 0.08, 0.05}, {0.05, 0.08, 0.99, 0.05}, {-0.1, -0.2, -0.3, -0.9}};
  for (int k = 0; k < 5; k++) {
    const double n = std::sqrt(q[k][0] * q[k][0] + q[k][1] * q[k][1] + q[k][2] * q[k][2] + q[k][3] * q[k][3]);
    const std::array<float, 4> u = {(float) (q[k][0] / n), (float) (q[k][1] / n), (float) (q[k][2] / n), (float) (q[k][3] / n)};
    const gw::PoseRt p = gw::split_pose(gw::pose_from(t, u));
    const double tr = (double) p.R[0] + p.R[4] + p.R[8];
    const int branch = tr > 0.0 ? 0 : (p.R[0] > p.R[4] && p.R[0] > p.R[8]) ? 1 : p.R[4] > p.R[8] ? 2 : 3;
    expect(branch == (k == 4 ? 0 : k), "the quaternion reaches its branch of quat_from", branch, k);
    const std::array<float, 4> back = gw::quat_from(p.R);
    const double sign = u[3] < 0.f ? -1.0 : 1.0;
    for (int i = 0; i < 4; i++) expect(std::fabs((double) back[i] - sign * u[i]) <= 1e-6, "quat_from(R(q)) == +-q", back[i], sign * u[i]);
    expect(back[3] >= 0.f, "w >= 0", back[3]);
  }
}

// ---- chunks --------------------------------------------------------------------------------------------------------------

mrh_block_desc block_at(int x, int y, int z, int resolution = 0) { return mrh_block_desc{x, y, z, resolution}; }

void chunks() {
  for (const float ext : {1.f, 2.f}) {
    const gw::Chunk c = gw::worldToChunks({0.5f * ext, -0.5f * ext, 0.49f * ext}, ext);
    expect(c[0] == 1 && c[1] == -1 && c[2] == 0, "worldToChunks rounds half away from zero", c[0] * 100 + c[1] * 10 + c[2], ext);
    const gw::Chunk d = gw::worldToChunks({-0.49f * ext, 1.5f * ext, -2.5f * ext}, ext);
    expect(d[0] == 0 && d[1] == 2 && d[2] == -3, "worldToChunks, the other signs", d[0] * 100 + d[1] * 10 + d[2], ext);
  }
  // two chunks from the centre, radius 1.5, chunk radius sqrt(3) / 2 = 0.866: 2 <= 2.366 but 2 > |1.5 - 0.866|
  const gw::Vec3 origin = {0.f, 0.f, 0.f};
  expect(std::fabs(gw::chunkRadius(1.f) - 0.8660254f) < 1e-6f, "chunkRadius", gw::chunkRadius(1.f));
  expect(gw::chunkTouchesSphere({2, 0, 0}, origin, 1.5f, 1.f), "the transparent test takes the chunk");
  expect(!gw::chunkInSphereRef({2, 0, 0}, origin, 1.5f, 1.f), "the literal test refuses it");
  expect(gw::chunkInSphereRef({2, 0, 0}, origin, 3.f, 1.f) && !gw::chunkTouchesSphere({4, 0, 0}, origin, 1.5f, 1.f), "and the two other answers");

  // five blocks of 0.16 m (voxels of 0.02 m) in three chunks of 1 m: x = -10 -> -1.6 m -> chunk -2; 0 and 1 -> chunk 0; 4 -> 0.64 m -> chunk 1
  const mrh_block_desc descs[5] = {block_at(4, 0, 0), block_at(0, 0, 0), block_at(-10, 0, 0), block_at(1, 0, 0), block_at(-10, 1, 0)};
  std::vector<mrh_voxel> vox(5 * 512);
  for (size_t i = 0; i < vox.size(); i++) vox[i] = mrh_voxel{(float) (i / 512) + (float) (i % 512) / 1024.f, 0.f, {0, 0, 0}, (uint8_t) (i / 512 + 1)};
  gw::ChunkGrid grid;
  expect(grid.empty() && grid.blocks() == 0, "a new grid is empty");
  grid.add(descs, vox.data(), 5, 0.02f, 1.f);
  expect(grid.blocks() == 5 && grid.chunks().size() == 3, "add: five blocks in three chunks", (double) grid.blocks(), (double) grid.chunks().size());
  const gw::ChunkGrid::Gathered all = grid.gather([](const gw::Chunk&) { return true; });
  const int order[5] = {2, 4, 1, 3, 0};  // map order of the chunks, arrival order inside one
  expect(all.descs.size() == 5 && all.voxels.size() == 5 * 512 && all.taken.size() == 3, "gather(all): every block once", (double) all.descs.size());
  for (int k = 0; k < 5 && all.descs.size() == 5; k++) {
    expect(all.descs[k].x == descs[order[k]].x && all.descs[k].y == descs[order[k]].y, "gather(all): map order", k, all.descs[k].x);
    expect(all.voxels[k * 512 + 7].sdf == vox[order[k] * 512 + 7].sdf && all.voxels[k * 512 + 511].weight == order[k] + 1, "gather(all): the block's own voxels", k);
  }
  expect(all.taken.size() == 3 && all.taken[0] == gw::Chunk{-2, 0, 0} && all.taken[1] == gw::Chunk{0, 0, 0} && all.taken[2] == gw::Chunk{1, 0, 0}, "gather(all): the chunks");
  expect(grid.blocks() == 5, "gather without erase leaves the grid as it was (a failed import)", (double) grid.blocks());
  const gw::ChunkGrid::Gathered some = grid.gather([](const gw::Chunk& c) { return c[0] >= 0; });
  expect(some.descs.size() == 3 && some.taken.size() == 2, "gather(x >= 0)", (double) some.descs.size(), (double) some.taken.size());
  grid.erase(some.taken);
  expect(grid.blocks() == 2 && grid.chunks().size() == 1, "erase drops the gathered blocks", (double) grid.blocks());
  expect(grid.gather([](const gw::Chunk& c) { return c[0] >= 0; }).descs.empty(), "nothing is gathered twice");
  grid.clear();
  expect(grid.empty(), "clear");
}

int centres(const gw::MeshPlan& p) {
  int n = 0;
  p.forEachCenter([&](const gw::Vec3&) { n++; });
  return n;
}

void plan() {
  const gw::ChunkGrid none;
  const gw::MeshPlan e = gw::planExtract({}, none, 1, 1.f);
  expect(e.empty && e.radiusi == 10 && e.radius == 10.f, "plan: empty map", e.radiusi);

  const gw::MeshPlan one = gw::planExtract({{3, 4, 5}}, none, 1, 1.f);
  expect(!one.empty && one.lo == gw::Chunk{3, 4, 5} && one.hi == gw::Chunk{4, 5, 6}, "plan: one chunk, hi = lo + 1");
  expect(one.first_center == gw::Vec3{3.f, 4.f, 5.f} && one.in_first_sphere && centres(one) == 1, "plan: one chunk is one pass", centres(one));

  // inside the sphere of 10 - 0.866 around the first centre, and no axis longer than 10 chunks; chunks of 2 m
  gw::ChunkGrid host;  // one paged-out block at y = 50 * 0.16 = 8 m: chunk (0, 4, 0)
  const mrh_block_desc paged = block_at(0, 50, 0);
  const std::vector<mrh_voxel> paged_voxels(512);
  host.add(&paged, paged_voxels.data(), 1, 0.02f, 2.f);
  const gw::MeshPlan in = gw::planExtract({{0, 0, 0}, {3, 0, 0}}, host, 2, 1.f);
  expect(in.lo == gw::Chunk{0, 0, 0} && in.hi == gw::Chunk{3, 4, 1}, "plan: bounds over device and host chunks", in.hi[1], in.hi[2]);
  expect(in.in_first_sphere && centres(in) == 1 && in.ext == 2.f, "plan: a map inside the first sphere is one pass", centres(in));

  // 25 chunks along x, 12 along y: steps of 10 -> x = 0, 10, 20 and y = 0, 10, z = 0: six centres
  const gw::MeshPlan walk = gw::planExtract({{0, 0, 0}, {25, 0, 0}, {0, 12, 0}}, none, 1, 1.f);
  expect(!walk.in_first_sphere && walk.hi == gw::Chunk{25, 12, 1} && centres(walk) == 6, "plan: a long map is walked", centres(walk));
  gw::Vec3 last{};
  walk.forEachCenter([&](const gw::Vec3& c) { last = c; });
  expect(last == gw::Vec3{20.f, 10.f, 0.f}, "plan: the last centre", last[0], last[1]);

  const gw::MeshPlan near = gw::planExtract({{0, 0, 0}, {2, 0, 0}}, none, 1, 0.05f);
  expect(near.radiusi == 1 && std::fabs(near.radius - 0.5f) < 1e-6f && !near.in_first_sphere && centres(near) == 2, "plan: max_depth 0.05 -> radiusi 1", near.radiusi, centres(near));

  const gw::MeshPlan corner = gw::planExtract({{0, 0, 0}, {9, 9, 9}}, none, 1, 1.f);  // 15.6 chunks from the first centre
  expect(!corner.in_first_sphere && centres(corner) == 1, "plan: every axis fits but a chunk lies outside the sphere", centres(corner));
}

// ---- files ---------------------------------------------------------------------------------------------------------------

void mesh_rows() {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> V = {0.0, -0.0, 1e-5, 9.9999995e-5, 1e-4, 123456.5, 999999.5, 1e6, 1e-300, 4.9e-324, 1e300, inf, -inf,
                           std::numeric_limits<double>::quiet_NaN(), 0.1, 2.5, 1.0 / 3.0};
  std::mt19937_64 rng(20240607);
  std::uniform_real_distribution<float> uniform(-50.f, 50.f);
  for (int i = 0; i < 100000; i++) V.push_back((double) uniform(rng));
  const uint64_t nv = V.size() / 3;
  expect(V.size() == 100017 && V.size() % 3 == 0, "the inputs fill whole rows", (double) V.size());
  const double shades[5] = {0.0, 1.0, 127.9, 255.0, 255.9};
  std::vector<double> C(V.size());
  for (size_t i = 0; i < C.size(); i++) C[i] = shades[(i * 7 + i / 5) % 5];
  std::vector<int32_t> F = {0, 1, 2, INT32_MAX, INT32_MIN, -1};
  for (int i = 0; i < 2994; i++) F.push_back((int32_t) (rng() % (3 * nv)));
  const uint64_t nf = F.size() / 3;

  // value by value, then the file: what an ofstream prints
  uint64_t compared = 0, differing = 0;
  for (const double v : V) {
    char buf[32];
    std::ostringstream o;
    o << v;
    compared++;
    const std::string got(buf, gw::putDouble(buf, v));
    if (got != o.str()) { differing++; printf("FAILED double %.17g: to_chars \"%s\", ostream \"%s\"\n", v, got.c_str(), o.str().c_str()); }
  }
  failures += (int) differing;
  printf("gw_check: compared %llu doubles, %llu differ\n", (unsigned long long) compared, (unsigned long long) differing);
  std::ostringstream want;
  want << "ply\nformat ascii 1.0\nelement vertex " << nv << "\nproperty float x\nproperty float y\nproperty float z\n"
       << "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face " << nf << "\nproperty list uchar int vertex_indices\nend_header\n";
  for (uint64_t i = 0; i < nv; i++)
    want << V[i * 3] << " " << V[i * 3 + 1] << " " << V[i * 3 + 2] << " " << (int) (unsigned char) C[i * 3] << " " << (int) (unsigned char) C[i * 3 + 1] << " "
         << (int) (unsigned char) C[i * 3 + 2] << "\n";
  for (uint64_t i = 0; i < nf; i++) want << "3 " << F[i * 3] << " " << F[i * 3 + 1] << " " << F[i * 3 + 2] << "\n";
  for (const unsigned n_workers : {1u, 2u, 7u}) {
    std::ostringstream got;
    got << gw::meshPlyHeader(nv, nf);
    const std::vector<gw::PlyPiece> pieces = gw::formatMesh(V.data(), C.data(), F.data(), nv, nf, n_workers);
    expect(pieces.size() == 2 * n_workers, "two pieces per worker", (double) pieces.size());
    gw::writePieces(got, pieces);
    expect(got.str() == want.str(), "the mesh file equals the iostream restatement", n_workers, (double) got.str().size());
  }
  const std::vector<gw::PlyPiece> nothing = gw::formatMesh(nullptr, nullptr, nullptr, 0, 0, 3);
  expect(nothing.size() == 6 && nothing[0].len == 0 && nothing[5].len == 0, "an empty mesh has empty pieces");
}

void grid_file() {
  for (const uint64_t n : {(uint64_t) 0, (uint64_t) 3}) {
    std::vector<mrh_block_desc> descs;
    std::vector<mrh_voxel> vox(n * 512);
    for (uint64_t k = 0; k < n; k++) descs.push_back(block_at((int) k - 1, 7, -3, (int) (k & 1)));
    for (size_t i = 0; i < vox.size(); i++) vox[i] = mrh_voxel{(float) i * 0.5f, (float) i, {(uint8_t) i, 2, 3}, (uint8_t) (i % 251)};
    std::stringstream file;
    gw::writeGridHeader(file, n);
    for (uint64_t k = 0; k < n; k++) gw::writeGridBlock(file, descs[k], &vox[k * 512]);
    expect(file.str().size() == 16 + n * (16 + 512 * 12), "MRHGRID1: size", (double) file.str().size());
    std::vector<mrh_block_desc> d2;
    std::vector<mrh_voxel> v2;
    const uint64_t got = gw::readGrid(file, "x.bin", d2, v2);
    expect(got == n && d2.size() == (n ? n : 1) && v2.size() == (n ? n : 1) * 512, "MRHGRID1: count", (double) got);
    expect(n == 0 || (!std::memcmp(d2.data(), descs.data(), n * sizeof(mrh_block_desc)) && !std::memcmp(v2.data(), vox.data(), n * 512 * sizeof(mrh_voxel))), "MRHGRID1: round trip");
    if (n == 0) continue;
    std::vector<std::pair<std::string, std::string>> bad = {{"ply\nformat ascii 1.0\nelement vertex 100\n", "GeoWrapper::deserializeGrid | not a MRHGRID1 file: x.bin"},
                                                            {"MRHG", "GeoWrapper::deserializeGrid | not a MRHGRID1 file: x.bin"},
                                                            {file.str().substr(0, file.str().size() - 5), "GeoWrapper::deserializeGrid | truncated file: x.bin"},
                                                            {file.str().substr(0, 16), "GeoWrapper::deserializeGrid | truncated file: x.bin"}};
    for (const auto& b : bad) {
      std::istringstream in(b.first);
      std::string what = "(no exception)";
      try { gw::readGrid(in, "x.bin", d2, v2); } catch (const std::runtime_error& e) { what = e.what(); }
      expect_text(what, b.second, "MRHGRID1: refusal");
    }
  }
}

void data_files() {
  // voxels of 0.5 m.  A fine block at (1, 0, -1): origin (4, 0, -4); voxel 0 (weight 3, sdf 0.25) and voxel 9 = (1, 1, 0) -> (4.5, 0.5, -4)
  // (weight 5, sdf -0.5).  A coarse block at (0, 2, 0): origin (0, 8, 0), 4^3 voxels of 1 m; voxel 5 = (1, 1, 0) -> (1, 9, 0) (weight 7, sdf 1).
  // A third block without a weighted voxel gives no point.
  const mrh_block_desc descs[3] = {block_at(1, 0, -1), block_at(0, 2, 0, 1), block_at(5, 5, 5)};
  std::vector<mrh_voxel> vox(3 * 512, mrh_voxel{9.f, 0.f, {0, 0, 0}, 0});
  vox[0] = mrh_voxel{0.25f, 0.f, {0, 0, 0}, 3};
  vox[9] = mrh_voxel{-0.5f, 0.f, {0, 0, 0}, 5};
  vox[512 + 5] = mrh_voxel{1.f, 0.f, {0, 0, 0}, 7};
  vox[512 + 64] = mrh_voxel{1.f, 0.f, {0, 0, 0}, 200};  // beyond the 4^3 voxels of a coarse block: not read
  std::vector<gw::DataPoint> hash_pts, voxel_pts;
  gw::dataPoints(descs, vox.data(), 3, 0.5f, hash_pts, voxel_pts);
  const std::string head = "\nproperty float x\nproperty float y\nproperty float z\nproperty float red\nproperty float green\nproperty float blue\nproperty float weight\n";
  std::ostringstream h, v;
  gw::writeDataPoints(h, hash_pts, false);
  gw::writeDataPoints(v, voxel_pts, true);
  expect_text(h.str(), "ply\nformat ascii 1.0\nelement vertex 2" + head + "end_header\n4 0 -4 1 0 0 4\n0 8 0 0 1 0 7\n", "serializeData: hash points");
  expect_text(v.str(), "ply\nformat ascii 1.0\nelement vertex 3" + head + "property float sdf\nend_header\n4 0 -4 1 0 0 3 0.25\n4.5 0.5 -4 1 0 0 5 -0.5\n1 9 0 0 1 0 7 1\n",
              "serializeData: voxel points");

  const std::vector<mrh_splat_seed> seeds = {mrh_splat_seed{{1.f, 2.f, 3.f}, 0.5f, {255, 0, 7}, 0}, mrh_splat_seed{{-0.25f, 1e-5f, 1e6f}, 0.125f, {1, 2, 3}, 0}};
  std::ostringstream s;
  gw::writeSeeds(s, seeds);
  expect_text(s.str(), "ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nproperty float scale\n"
                       "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n1 2 3 0.5 255 0 7\n-0.25 1e-05 1e+06 0.125 1 2 3\n", "seeds PLY");
}

}  // namespace

int main() {
  pose();
  chunks();
  plan();
  mesh_rows();
  grid_file();
  data_files();
  printf("gw_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
