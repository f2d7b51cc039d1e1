// geowrapper.cpp — host facade over the C ABI; mirrors pygeowrapper::GeoWrapper (geowrapper.cpp:9-577 of the
// reference) for the setDepthImage / compute() / extractMesh() path.  Errors that the reference turns into
// print-and-exit (cuda_utils.cuh:9-17) are raised as std::runtime_error instead.
#include "geowrapper.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <chrono>
#include <stdexcept>
#include <thread>

#include "gw_files.h"

namespace pygeowrapper {

using gw::PoseRt;
using gw::pose_from;
using gw::split_pose;

template <typename T> T zeroed() { T v; std::memset(&v, 0, sizeof v); return v; }

void GeoWrapper::check(int rc, const char* what) const {
  if (rc != MRH_OK) throw std::runtime_error(std::string("GeoWrapper::") + what + " | " + mrh_last_error(ctx_));
}

GeoWrapper::GeoWrapper(float sdf_truncation, float sdf_truncation_scale, int integration_weight_sample, float virtual_voxel_size,
                       int n_frames_invalidate_voxels, int voxel_extents_scale, bool /*viewer_active*/, float marching_cubes_threshold,
                       uint8_t min_weight_threshold, float min_depth, float max_depth, const std::string& gs_optimization_param_path,
                       float sdf_var_threshold, float vertices_merging_threshold, bool projective_sdf) {
  set_.sdf_truncation = sdf_truncation; set_.sdf_truncation_scale = sdf_truncation_scale; set_.integration_weight_sample = integration_weight_sample;
  set_.virtual_voxel_size = virtual_voxel_size; set_.n_frames_invalidate_voxels = n_frames_invalidate_voxels; set_.voxel_extents_scale = voxel_extents_scale;
  set_.min_weight_threshold = min_weight_threshold; set_.sdf_var_threshold = sdf_var_threshold; set_.vertices_merging_threshold = vertices_merging_threshold;
  if (!gs_optimization_param_path.empty()) {
    // geowrapper.cpp:74-78 builds a GaussianContainer from this file.  Here only its initialisation half exists (the
    // per-frame splat seeds, mrh_splat_seeds); the optimiser / rasteriser stay out of scope, so of the JSON only the two
    // quad-tree keys are read (src/gs/gaussian.cu:49-50; defaults gaussian.cuh:28-29).
    std::ifstream js(gs_optimization_param_path);
    if (!js.is_open()) throw std::runtime_error("GeoWrapper::GeoWrapper | cannot open " + gs_optimization_param_path);
    const std::string text((std::istreambuf_iterator<char>(js)), std::istreambuf_iterator<char>());
    auto number_after = [&](const char* key, double fallback) {
      const size_t k = text.find(std::string("\"") + key + "\"");
      if (k == std::string::npos) return fallback;
      const size_t colon = text.find(':', k);
      if (colon == std::string::npos) return fallback;
      return std::strtod(text.c_str() + colon + 1, nullptr);
    };
    qtree_thresh_ = (float) number_after("qtree_thresh", 0.1);
    qtree_min_pixel_size_ = (int) number_after("qtree_min_pixel_size", 1.0);
    gs_enabled_ = true;
    std::cerr << "GeoWrapper::GeoWrapper | splat seeds only (quad-tree threshold " << qtree_thresh_ << ", min pixel size " << qtree_min_pixel_size_
              << "); Gaussian-splatting optimisation is outside this library's scope" << std::endl;
  }
  mrh_params p = zeroed<mrh_params>();
  p.abi_version = MRH_ABI_VERSION;
  p.sdf_truncation = sdf_truncation;
  p.sdf_truncation_scale = sdf_truncation_scale;
  p.integration_weight_sample = integration_weight_sample;
  p.integration_weight_max = set_.integration_weight_max;
  p.virtual_voxel_size = virtual_voxel_size;
  p.n_frames_invalidate_voxels = n_frames_invalidate_voxels;
  p.voxel_extents_scale = voxel_extents_scale;
  p.marching_cubes_threshold = marching_cubes_threshold;
  p.min_weight_threshold = min_weight_threshold;
  p.projective_sdf = projective_sdf ? 1 : 0;
  p.min_depth = min_depth;
  p.max_depth = max_depth;
  p.sdf_var_threshold = sdf_var_threshold;
  p.vertices_merging_threshold = vertices_merging_threshold;
  // capacities: 0 = the reference rule applied to the free HBM of the device (geowrapper.cpp:37-54);
  // MRHASH_NUM_SDF_BLOCKS / MRHASH_DEVICE override
  if (const char* e = std::getenv("MRHASH_NUM_SDF_BLOCKS")) p.num_sdf_blocks = std::strtoull(e, nullptr, 10);
  if (const char* e = std::getenv("MRHASH_DEVICE")) p.device_id = std::atoi(e);
  device_id_ = p.device_id;
  if (const char* e = std::getenv("MRHASH_STREAM")) streaming_enabled_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MRH_SYNC_COMPUTE")) sync_compute_ = std::atoi(e) != 0;
  p.shard_count = 1;
  int rc = mrh_create(&p, &ctx_);
  if (rc != MRH_OK) throw std::runtime_error(std::string("GeoWrapper::GeoWrapper | ") + mrh_last_error(nullptr));
  mrh_stats st;
  check(mrh_get_stats(ctx_, &st), "GeoWrapper");
  set_.num_sdf_blocks = (int) st.num_sdf_blocks;
  set_.hash_num_buckets = set_.num_sdf_blocks;  // geowrapper.cpp:50
  set_.max_num_sdf_block_integrate_from_global_hash = (int) (st.num_sdf_blocks / 7);  // 0.10 / 0.70 of the block budget, :53-54
  pose_ = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  camera_in_lidar_ = pose_;
}

GeoWrapper::~GeoWrapper() {
  mrh_destroy(ctx_);  // detaches from the communicator
  mrh_comm_destroy(comm_.comm);
}

// ---- multi-GPU: RCCL behind the C ABI (include/mrhash_comm.h) ------------------------------------------------------------
std::array<uint8_t, MRH_COMM_ID_BYTES> GeoWrapper::commUniqueId() {
  std::array<uint8_t, MRH_COMM_ID_BYTES> id;
  if (mrh_comm_unique_id(id.data()) != MRH_OK) throw std::runtime_error(std::string("GeoWrapper::commUniqueId | ") + mrh_comm_last_error(nullptr));
  return id;
}

void GeoWrapper::commInit(const std::array<uint8_t, MRH_COMM_ID_BYTES>& id, int rank, int world, int chunk_log2, bool tile_sharded) {
  if (comm_.comm) throw std::runtime_error("GeoWrapper::commInit | a communicator is already attached");
  if (mrh_comm_create(id.data(), rank, world, device_id_, &comm_.comm) != MRH_OK)
    throw std::runtime_error(std::string("GeoWrapper::commInit | ") + mrh_comm_last_error(nullptr));
  check(mrh_comm_attach(ctx_, comm_.comm), "commInit");
  comm_.rank = rank; comm_.world = world; comm_.chunk_log2 = chunk_log2; comm_.tile_sharded = tile_sharded;
  if (tile_sharded) check(mrh_set_sharding(ctx_, rank, world, chunk_log2), "commInit");
  streaming_enabled_ = false;  // a sharded map is sized per rank; the host chunk grid and the exchange steps do not mix
}

void GeoWrapper::mergeSubmaps() {
  if (!comm_.comm) throw std::runtime_error("GeoWrapper::mergeSubmaps | commInit has not been called");
  mrh_comm_merge_info info;
  check(mrh_comm_merge_submaps(ctx_, comm_.chunk_log2, &info), "mergeSubmaps");
  comm_.tile_sharded = true;
}

void GeoWrapper::setCurrPose(const std::array<float, 3>& t, const std::array<float, 4>& q) { pose_ = pose_from(t, q); }

void GeoWrapper::setCamera(float fx, float fy, float cx, float cy, int rows, int cols, float min_depth, float max_depth, int camera_model) {
  check(mrh_set_camera(ctx_, fx, fy, cx, cy, rows, cols, min_depth, max_depth, camera_model), "setCamera");
  cam_.set = true;
  cam_.model = camera_model; cam_.rows = rows; cam_.cols = cols;
  cam_.fx = fx; cam_.fy = fy; cam_.cx = cx; cam_.cy = cy; cam_.min_depth = min_depth; cam_.max_depth = max_depth;
  // Streaming radius.  The reference uses max_depth itself (geowrapper.cpp:138), which is the z-range of a pinhole frame,
  // not its reach: a voxel at z = max_depth in an image corner is farther from the camera centre than that, so blocks
  // still inside the frustum can be paged out and then re-created empty.  Here the radius is the true reach of a frame:
  // (max_depth + truncation) along the most oblique pixel ray, plus one block diagonal.
  const float trunc = set_.sdf_truncation + set_.sdf_truncation_scale * max_depth;
  float sec = 1.f;
  if (camera_model == MRH_CAMERA_PINHOLE && fx > 0.f && fy > 0.f) {
    const float ux = std::max(cx + 0.5f, (float) cols - cx) / fx, uy = std::max(cy + 0.5f, (float) rows - cy) / fy;
    sec = std::sqrt(1.f + ux * ux + uy * uy);
  }
  cam_.reach = (max_depth + trunc) * sec + 8.f * set_.virtual_voxel_size * std::sqrt(3.f);
}

// The reference copies the image into its own host buffer here and uploads it in compute() (geowrapper.cpp:300-321,
// :125-126).  Here the setter's copy IS the upload: mrh_upload_* copies into pinned staging (the numpy array is free on
// return, as with the reference) and starts the host-to-device copy on a second stream right away, under the previous
// frame's kernels; compute() only enqueues the frame.
void GeoWrapper::setDepthImage(const float* data, size_t rows, size_t cols) {
  check(mrh_upload_depth(ctx_, data, (int) rows, (int) cols), "setDepthImage");
  have_depth_ = true;
}

void GeoWrapper::setRGBImage(const uint8_t* data, size_t rows, size_t cols) {
  check(mrh_upload_rgb(ctx_, data, (int) rows, (int) cols), "setRGBImage");
  have_rgb_ = true;
}

void GeoWrapper::setPointCloud(const float* pts, size_t n, const float* normals_or_null, bool compute_normals) {
  point_cloud_.assign(pts, pts + 3 * n);
  if (normals_or_null) normals_.assign(normals_or_null, normals_or_null + 3 * n);
  else normals_.clear();
  estimate_normals_ = compute_normals && !normals_or_null;
  normals_on_device_ = false;
}

const std::vector<float>& GeoWrapper::normals() const {
  if (normals_on_device_) {
    const float* nxyz = nullptr;
    uint64_t n = 0;
    check(mrh_get_normals(ctx_, &nxyz, &n, nullptr), "getNormals");
    normals_.assign(nxyz, nxyz + 3 * n);
    normals_on_device_ = false;
  }
  return normals_;
}

// ---- streamer, host side: chunk grid (streamer.cuh:251-352, streamer.cpp:214-247, :292-331) ---------------------------
constexpr float kStreamThreshold = 0.15f;  // params.h:28 stream_threshold

GeoWrapper::Blocks GeoWrapper::dumpBlocks(const char* what, const bool with_voxels) {
  Blocks b;
  check(mrh_dump_blocks(ctx_, nullptr, nullptr, 0, &b.n), what);
  b.descs.resize(b.n ? b.n : 1);
  b.voxels.resize(with_voxels ? (b.n ? b.n : 1) * 512 : 1);
  check(mrh_dump_blocks(ctx_, b.descs.data(), with_voxels ? b.voxels.data() : nullptr, b.n, &b.n), what);
  return b;
}

void GeoWrapper::streamOutToGrid(const std::array<float, 3>& center, float radius) {
  uint64_t n = 0;
  check(mrh_stream_out(ctx_, center.data(), radius, nullptr, nullptr, 0, &n), "stream");
  if (n == 0) return;
  std::vector<mrh_block_desc> descs(n);
  std::vector<mrh_voxel> vox(n * 512);
  check(mrh_stream_out(ctx_, center.data(), radius, descs.data(), vox.data(), n, &n), "stream");
  grid_.add(descs.data(), vox.data(), n, set_.virtual_voxel_size, chunkExt());
}

// Streamer::streamInToGPU (streamer.cpp:292-331, :358-378): what was gathered from the host grid goes to the device and leaves the grid
void GeoWrapper::streamInGathered(const char* what, const gw::ChunkGrid::Gathered& g) {
  if (g.descs.empty()) return;
  // import first, forget the host copies only once the device holds them: a failed import (pool full) must not lose blocks
  check(mrh_import_blocks(ctx_, g.descs.data(), g.voxels.data(), g.descs.size()), what);
  grid_.erase(g.taken);  // "it lives on the device from now"
}

// Streamer::stream (streamer.cpp:333-354) with the two radii chosen so that paging is TRANSPARENT — a block is either on
// the device or in the host grid, and everything a frame can touch is on the device:
//   in : every chunk that touches the sphere of the frame's reach comes back (also called every frame by compute());
//   out: blocks farther than reach + 2 chunk radii leave — none of them lies in a chunk the next stream-in would take.
void GeoWrapper::stream(const std::array<float, 3>& camera_position, float radius) {
  streamOutToGrid(camera_position, radius + 2.f * gw::chunkRadius(chunkExt()) + 1e-3f);
  streamInSphere(camera_position, radius);
}

void GeoWrapper::streamInSphere(const std::array<float, 3>& center, float radius) {
  const float ext = chunkExt();
  streamInGathered("stream", grid_.gather([&](const gw::Chunk& c) { return gw::chunkTouchesSphere(c, center, radius, ext); }));
}

void GeoWrapper::compute() {
  if (streaming_enabled_) {
    const std::array<float, 3> cam = {pose_[3], pose_[7], pose_[11]};
    if (!grid_.empty()) streamInSphere(cam, cam_.reach);  // host-only test unless a paged-out chunk is within reach
    // geowrapper.cpp:137-138 reads the free count back every frame; here it is the newest level the device has reported
    // (a frame or two old, no stall): paging is transparent in this library, so the trigger frame does not matter
    int64_t free_fine = 0;
    check(mrh_peek_free_blocks(ctx_, &free_fine, nullptr, nullptr), "compute");
    if ((float) free_fine <= kStreamThreshold * (float) set_.num_sdf_blocks) stream(cam, cam_.reach);
  }
  const PoseRt at = split_pose(pose_);
  check(mrh_set_pose(ctx_, at.R, at.t), "compute");
  if (have_depth_ && have_rgb_) {  // geowrapper.cpp:140
    check(mrh_integrate(ctx_, set_.n_frames_invalidate_voxels), "compute");
    // The reference reports an exhausted pool / a full table from the device (printf, vds.cu:566-569) and carries on without
    // the affected blocks.  Same here, without a stall: the flags of a frame that finished a moment ago arrive with the
    // pool-level report; each is announced once.
    uint32_t flags = 0;
    if (sync_compute_) {
      // MRH_SYNC_COMPUTE=1 / _setSyncCompute(true): compute() as the reference's — blocking (geowrapper.cpp:118-148 ends in
      // cudaDeviceSynchronize), the frame's own capacity flags announced in this call, a device error thrown by it.
      const int rc = mrh_sync(ctx_);
      if (rc != MRH_OK && rc != MRH_ERR_CAPACITY && rc != MRH_ERR_OUT_OF_RANGE) check(rc, "compute");
      mrh_stats st;
      check(mrh_get_stats(ctx_, &st), "compute");
      flags = st.error_flags & ~flags_announced_;
      flags_announced_ |= st.error_flags;
      last_compute_flags_ = flags;
    }
    if (sync_compute_ ? flags != 0 : (mrh_peek_error_flags(ctx_, &flags) == MRH_OK && flags)) {
      if (flags & 1u) std::cerr << "GeoWrapper::compute | SDF block pool exhausted: blocks of recent frames were skipped" << std::endl;
      if (flags & 2u) std::cerr << "GeoWrapper::compute | hash table probe limit reached: blocks of recent frames were skipped" << std::endl;
      if (flags & 4u) std::cerr << "GeoWrapper::compute | block coordinates left the +-2^20 key range" << std::endl;
    }
    if (gs_enabled_) {  // geowrapper.cpp:142-143 runGS -> extractNodesQTree + checkNodes; Add_gaussians keeps what they emit
      const mrh_splat_seed* seeds = nullptr;
      uint64_t n = 0;
      check(mrh_splat_seeds(ctx_, qtree_thresh_, qtree_min_pixel_size_, &seeds, &n), "compute");
      seeds_.insert(seeds_.end(), seeds, seeds + n);
    }
  }
  if (!point_cloud_.empty()) {  // geowrapper.cpp:146-147: VoxelContainer::integrate(point_cloud, eigenvectors, weights, ...)
    // Normals passed along with the points (one per point) drive the normal-direction SDF when the wrapper was built with
    // projective_sdf = false (vds.cu:1248-1251, :1322-1326); with the projective SDF (every shipped configuration and
    // runner) the reference only normalises them and never uses them (vds.cu:1236), so they are simply not needed.
    // setPointCloud(points, compute_normals = true) has them estimated on the device from the uploaded points, one plane per
    // 0.4 m neighbourhood as the reference's MAD-tree leaves (geowrapper.cpp:377-403); the definition is DESIGN.md D12.
    if (!normals_.empty() && !estimate_normals_) check(mrh_upload_normals(ctx_, normals_.data(), normals_.size() / 3), "compute");
    check(mrh_upload_points(ctx_, point_cloud_.data(), point_cloud_.size() / 3), "compute");
    if (estimate_normals_) {
      check(mrh_estimate_normals(ctx_, nullptr, nullptr), "compute");
      normals_on_device_ = true;
    }
    check(mrh_integrate_points(ctx_, set_.n_frames_invalidate_voxels), "compute");
  }
}

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

void GeoWrapper::extractMesh(const std::string& filename) {
  const double t0 = now_ms();
  // the previous mesh goes first: if this extraction throws, the getters must not read buffers the library has already reused
  mesh_ = MeshView();

  if (comm_.comm && comm_.world > 1) {
    // sharded map: boundary blocks to every rank, every rank extracts what it owns, rank 0 merges the runs into the single-GPU
    // canonical order and post-processes; the halo goes again so that fusion can continue
    if (!comm_.tile_sharded) throw std::runtime_error("GeoWrapper::extractMesh | frame-sharded sub-maps: call mergeSubmaps() first");
    if (!grid_.empty()) throw std::runtime_error("GeoWrapper::extractMesh | a sharded map cannot have blocks on the host grid");
    std::cout << "GeoWrapper::extractMesh | extracting (rank " << comm_.rank << " of " << comm_.world << ")..." << std::endl;
    uint64_t taken = 0, nt_all = 0;
    check(mrh_comm_exchange_halo(ctx_, &taken), "extractMesh");
    check(mrh_comm_gather_mesh(ctx_, 0, &nt_all), "extractMesh");
    check(mrh_drop_blocks(ctx_, MRH_DROP_HALO, nullptr), "extractMesh");
    if (comm_.rank != 0) return;  // the mesh lives on rank 0
    std::cout << "MarchingCubesExtractor::extractIsoSurface | triangles extracted: " << nt_all << std::endl;
    writeMesh(filename, t0);
    return;
  }

  // geowrapper.cpp:150-190: one extraction over the resident map where the reference's chunk walk would have a single iteration
  // whose sphere holds the whole map (gw::planExtract) and the map fits the pool — taken without paging 6 KiB per block out and in
  // again (the only difference: the map stays on the device afterwards; the reference leaves it on the host); else the walk.
  const float ext = chunkExt();
  const Blocks dev = dumpBlocks("extractMesh", false);
  std::vector<gw::Chunk> dev_chunks(dev.n);
  for (uint64_t k = 0; k < dev.n; k++) dev_chunks[k] = gw::chunkOfBlock(dev.descs[k], set_.virtual_voxel_size, ext);
  const gw::MeshPlan plan = gw::planExtract(dev_chunks, grid_, set_.voxel_extents_scale, cam_.max_depth);
  uint64_t nt = 0;
  std::cout << "GeoWrapper::extractMesh | extracting..." << std::endl;
  bool one_pass = plan.empty || plan.in_first_sphere;
  if (one_pass && !grid_.empty()) {
    int64_t free_fine = 0;
    check(mrh_get_free_blocks(ctx_, &free_fine, nullptr), "extractMesh");
    one_pass = (int64_t) hostGridBlocks() <= free_fine;
  }
  if (one_pass) {
    streamInGathered("stream", grid_.gather([](const gw::Chunk&) { return true; }));  // whatever the streamer paged out takes part in the mesh
    check(mrh_extract_triangles(ctx_, nullptr, &nt), "extractMesh");                     // the soup itself stays on the device
  } else {
    const std::array<float, 3> origin = {0.f, 0.f, 0.f};
    streamOutToGrid(origin, -1.f);  // Streamer::streamAllOut (geowrapper.cpp:153)
    check(mrh_mesh_merge_begin(ctx_), "extractMesh");
    try {
      plan.forEachCenter([&](const gw::Vec3& center) {
        const gw::ChunkGrid::Gathered in = grid_.gather([&](const gw::Chunk& c) { return gw::chunkInSphereRef(c, center, plan.radius, ext); });
        if (in.descs.empty()) return;  // an empty sphere: no triangles, nothing to merge (:181)
        // refuse BEFORE touching anything when the sphere holds more blocks than the pool has free (the reference would run its heap
        // into the ground, silently)
        int64_t free_fine = 0;
        check(mrh_get_free_blocks(ctx_, &free_fine, nullptr), "extractMesh");
        if ((int64_t) in.descs.size() > free_fine)
          throw std::runtime_error("GeoWrapper::extractMesh | a sphere of radius " + std::to_string(plan.radius) + " m holds " + std::to_string(in.descs.size()) +
                                   " blocks, the pool has " + std::to_string(free_fine) + " free (num_sdf_blocks " + std::to_string(set_.num_sdf_blocks) +
                                   "): nothing was moved, the map is intact on the host grid");
        streamInGathered("extractMesh", in);
        uint64_t n_it = 0;
        check(mrh_extract_triangles(ctx_, nullptr, &n_it), "extractMesh");
        streamOutToGrid(origin, -1.f);  // streamAllOut (:186)
      });
    } catch (...) {
      uint64_t dummy = 0;
      (void) mrh_mesh_merge_end(ctx_, &dummy);
      try { streamOutToGrid(origin, -1.f); } catch (...) {}  // every block in exactly one place: the host grid
      throw;
    }
    check(mrh_mesh_merge_end(ctx_, &nt), "extractMesh");
  }
  std::cout << "MarchingCubesExtractor::extractIsoSurface | triangles extracted: " << nt << std::endl;
  writeMesh(filename, t0);
}

// the mesh of the last extraction out of the library, and the ASCII PLY of geowrapper.cpp:194-227 (gw_files.h)
void GeoWrapper::writeMesh(const std::string& filename, const double t0) {
  const bool dbg = std::getenv("MRH_DEBUG") != nullptr;
  check(mrh_extract_mesh(ctx_, &mesh_.v, &mesh_.nv, &mesh_.f, &mesh_.nf, &mesh_.c), "extractMesh");
  const double t1 = now_ms();
  mesh_.cached = false;  // getVertices / getFaces / getColors copy on first use (cacheMesh)
  const uint64_t nv = mesh_.nv, nf = mesh_.nf;
  std::ofstream ply(filename, std::ios::binary);
  if (!ply.is_open()) {
    std::cerr << "GeoWrapper::extractMesh | Failed to open file for writing: " << filename << std::endl;
    return;
  }
  ply << gw::meshPlyHeader(nv, nf);
  const unsigned n_workers = (unsigned) std::min<uint64_t>(std::max(1u, std::min(32u, std::thread::hardware_concurrency())), (nv + nf) / 65536 + 1);
  const double t2 = now_ms();
  const std::vector<gw::PlyPiece> pieces = gw::formatMesh(mesh_.v, mesh_.c, mesh_.f, nv, nf, n_workers);
  const double t3 = now_ms();
  gw::writePieces(ply, pieces);
  ply.close();
  if (dbg) std::cerr << "[geowrapper] extractMesh: library " << t1 - t0 << " ms, formatting " << t3 - t2
                     << ", writing " << now_ms() - t3 << std::endl;
  std::cout << "GeoWrapper::extractMesh | written " << nv << " vertices and " << nf << " faces to " << filename << std::endl;
}

void GeoWrapper::cacheMesh() const {
  if (mesh_.cached) return;
  mesh_.V.assign(mesh_.v, mesh_.v + mesh_.nv * 3);
  mesh_.C.assign(mesh_.c, mesh_.c + mesh_.nv * 3);
  mesh_.F.assign(mesh_.f, mesh_.f + mesh_.nf * 3);
  mesh_.cached = true;
}

void GeoWrapper::streamAllOut() {
  // The reference pages every block to the host chunk grid here (streamer.cpp:250-281) because its marching cubes
  // then walks the grid chunk by chunk.  With 288 GB of HBM the whole map is extracted in one pass instead
  // (extractMesh brings back whatever the streamer paged out), so this only drains the stream.
  check(mrh_sync(ctx_), "streamAllOut");
}

// intrinsics, image shape and depth range of the last setCamera into a zeroed parameter block (mrh_raycast_params, mrh_track_params):
// every other field is left at 0, its default
template <typename Params>
Params GeoWrapper::cameraParams() const {
  Params p = zeroed<Params>();
  p.fx = cam_.fx; p.fy = cam_.fy; p.cx = cam_.cx; p.cy = cam_.cy;
  p.rows = cam_.rows; p.cols = cam_.cols;
  p.min_depth = cam_.min_depth; p.max_depth = cam_.max_depth;
  return p;
}

// `method` needs the camera of a setCamera call, of the given model
void GeoWrapper::requireCamera(const char* method, const int model) const {
  const std::string who = std::string("GeoWrapper::") + method + " | ";
  if (!cam_.set) throw std::runtime_error(who + "setCamera has not been called");
  if (cam_.model != model)
    throw std::runtime_error(who + (model == MRH_CAMERA_PINHOLE ? "pinhole cameras only (the camera is spherical)" : "spherical cameras only (the camera is pinhole)"));
}

GeoWrapper::RaycastImages GeoWrapper::raycastPose(const std::array<float, 16>& pose) {
  requireCamera("raycast", MRH_CAMERA_PINHOLE);
  mrh_raycast_params p = cameraParams<mrh_raycast_params>();  // step 0: half the truncation
  p.outputs = MRH_RAYCAST_NORMALS | MRH_RAYCAST_COLORS;
  const PoseRt at = split_pose(pose);
  const float *depth = nullptr, *normals = nullptr;
  const uint8_t* rgb = nullptr;
  check(mrh_raycast(ctx_, &p, at.R, at.t, &depth, &normals, &rgb), "raycast");
  RaycastImages out;
  out.rows = p.rows; out.cols = p.cols;
  const size_t n = (size_t) p.rows * (size_t) p.cols;
  out.depth.assign(depth, depth + n);
  out.normals.assign(normals, normals + 3 * n);
  out.colors.assign(rgb, rgb + 3 * n);
  return out;
}

GeoWrapper::RaycastScan GeoWrapper::raycastScanPose(const std::array<float, 16>& pose) {
  requireCamera("raycastScan", MRH_CAMERA_SPHERICAL);
  mrh_raycast_params p = cameraParams<mrh_raycast_params>();  // step 0: half the truncation
  p.outputs = MRH_RAYCAST_NORMALS | MRH_RAYCAST_COLORS | MRH_RAYCAST_POINTS;
  const PoseRt at = split_pose(pose);
  const float *range = nullptr, *normals = nullptr, *points = nullptr;
  const uint8_t* rgb = nullptr;
  check(mrh_raycast_spherical(ctx_, &p, at.R, at.t, &range, &normals, &rgb, &points), "raycastScan");
  RaycastScan out;
  out.rows = p.rows; out.cols = p.cols;
  const size_t n = (size_t) p.rows * (size_t) p.cols;
  out.range.assign(range, range + n);
  out.normals.assign(normals, normals + 3 * n);
  out.colors.assign(rgb, rgb + 3 * n);
  out.points.assign(points, points + 3 * n);
  return out;
}

GeoWrapper::DistanceField GeoWrapper::distanceField(const std::array<float, 3>& lo, const std::array<float, 3>& hi, const float max_distance) {
  const double vs = (double) set_.virtual_voxel_size;
  mrh_esdf_params p = zeroed<mrh_esdf_params>();
  for (int a = 0; a < 3; a++) {
    if (!(hi[a] >= lo[a])) throw std::runtime_error("GeoWrapper::distanceField|hi < lo on axis " + std::to_string(a));
    const double first = std::floor((double) lo[a] / vs + 0.5), last = std::floor((double) hi[a] / vs + 0.5);
    if (!(last - first + 1.0 <= (double) MRH_ESDF_MAX_SIDE))
      throw std::runtime_error("GeoWrapper::distanceField|axis " + std::to_string(a) + " of the box spans more than " + std::to_string(MRH_ESDF_MAX_SIDE) + " voxels");
    if (!(std::fabs(first) < 2147483000.0)) throw std::runtime_error("GeoWrapper::distanceField|the box is out of range");
    p.origin[a] = (int32_t) first;
    p.dims[a] = (int32_t) (last - first + 1.0);
  }
  const double reach = std::ceil((double) max_distance / vs);
  if (!(reach >= 1.0 && reach <= (double) MRH_ESDF_MAX_REACH))
    throw std::runtime_error("GeoWrapper::distanceField|max_distance must be within (0, " + std::to_string(MRH_ESDF_MAX_REACH) + " voxels]");
  p.max_distance_voxels = (int32_t) reach;
  p.outputs = MRH_ESDF_STATE;
  const float* dist = nullptr;
  const uint8_t* state = nullptr;
  check(mrh_esdf(ctx_, &p, &dist, &state, nullptr), "distanceField");
  DistanceField out;
  const size_t n = (size_t) p.dims[0] * (size_t) p.dims[1] * (size_t) p.dims[2];
  for (int a = 0; a < 3; a++) { out.origin[a] = p.origin[a]; out.dims[a] = p.dims[a]; }
  out.dist.assign(dist, dist + n);
  out.state.assign(state, state + n);
  return out;
}

GeoWrapper::PointQuery GeoWrapper::queryPoints(const float* pts, const size_t n, const bool smooth, const bool sensor_frame) {
  mrh_query_params p = zeroed<mrh_query_params>();
  p.field = smooth ? MRH_QUERY_FIELD_SMOOTH : MRH_QUERY_FIELD_MAP;
  p.outputs = MRH_QUERY_GRADIENT | MRH_QUERY_COLOUR;
  const PoseRt at = split_pose(pose_);
  const float *dist = nullptr, *grad = nullptr;
  const uint8_t *rgbw = nullptr, *state = nullptr;
  check(mrh_query_points(ctx_, &p, pts, (uint64_t) n, sensor_frame ? at.R : nullptr, sensor_frame ? at.t : nullptr, &dist, &grad, &rgbw, &state), "queryPoints");
  PointQuery out;
  if (n) {
    out.dist.assign(dist, dist + n);
    out.grad.assign(grad, grad + 3 * n);
    out.rgbw.assign(rgbw, rgbw + 4 * n);
    out.state.assign(state, state + n);
  }
  return out;
}

GeoWrapper::RayCast GeoWrapper::castRays(const float* origins, const float* directions, const size_t n, const float max_range, const float min_range, const float step,
                                         const float* tmax, const bool sensor_frame, const bool normalize) {
  mrh_rays_params p = zeroed<mrh_rays_params>();
  p.min_range = min_range; p.max_range = max_range; p.step = step;
  p.outputs = MRH_RAYS_NORMALS | MRH_RAYS_COLORS | MRH_RAYS_COUNTS;
  std::vector<float> unit;
  if (normalize && n) {  // binary32, no contraction (the file is built with -ffp-contract=off): a zero direction becomes NaN, a bad ray
    unit.resize(3 * n);
    for (size_t i = 0; i < n; i++) {
      const float dx = directions[3 * i], dy = directions[3 * i + 1], dz = directions[3 * i + 2];
      const float len = std::sqrt((dx * dx + dy * dy) + dz * dz);
      unit[3 * i] = dx / len; unit[3 * i + 1] = dy / len; unit[3 * i + 2] = dz / len;
    }
    directions = unit.data();
  }
  const PoseRt at = split_pose(pose_);
  const float *range = nullptr, *normals = nullptr, *first = nullptr;
  const uint8_t *status = nullptr, *rgb = nullptr;
  const uint32_t* counts = nullptr;
  check(mrh_cast_rays(ctx_, &p, origins, directions, tmax, (uint64_t) n, sensor_frame ? at.R : nullptr, sensor_frame ? at.t : nullptr, &range, &status, &normals, &rgb,
                      &counts, &first), "castRays");
  RayCast out;
  if (n) {
    out.range.assign(range, range + n);
    out.status.assign(status, status + n);
    out.normals.assign(normals, normals + 3 * n);
    out.rgb.assign(rgb, rgb + 3 * n);
    out.counts.assign(counts, counts + 2 * n);
    out.first_unknown.assign(first, first + n);
  }
  return out;
}

mrh_remap_info GeoWrapper::fuseMap(GeoWrapper& other, const std::array<float, 3>& t, const std::array<float, 4>& q, const uint32_t min_weight) {
  mrh_remap_params p = zeroed<mrh_remap_params>();
  p.min_weight = min_weight;
  const PoseRt at = split_pose(pose_from(t, q));
  mrh_remap_info info = zeroed<mrh_remap_info>();
  check(mrh_fuse_map(ctx_, other.ctx_, &p, at.R, at.t, &info), "fuseMap");
  return info;
}

namespace {
// the tail of a pose fit: (R, t) as the C ABI returns them into the (t, q) of a TrackResult / AlignResult, as setCurrPose takes them
template <typename Result>
void fitted_pose(Result& out, const float R[9], const float t[3]) {
  out.t = {t[0], t[1], t[2]};
  out.q = gw::quat_from(R);
}
}  // namespace

// depth != nullptr: a depth image of the pinhole camera (D14); else the cloud pts [n * 3] against the spherical camera's render (D15)
GeoWrapper::TrackResult GeoWrapper::trackPose(const char* who, const float* depth, const float* pts, size_t n, const std::array<float, 16>& pose) {
  const mrh_track_params p = cameraParams<mrh_track_params>();  // step, dist_max, iterations, min_pixels: the defaults
  const PoseRt at = split_pose(pose);
  float out_R[9], out_t[3];
  TrackResult out;
  check(depth ? mrh_track_depth(ctx_, &p, depth, at.R, at.t, out_R, out_t, &out.info) : mrh_track_scan(ctx_, &p, pts, n, at.R, at.t, out_R, out_t, &out.info), who);
  fitted_pose(out, out_R, out_t);
  return out;
}

GeoWrapper::AlignResult GeoWrapper::alignMap(GeoWrapper& other, const std::array<float, 3>& t, const std::array<float, 4>& q, const int iterations, const uint32_t min_weight) {
  mrh_align_params p = zeroed<mrh_align_params>();
  p.iterations = iterations;
  p.min_weight = min_weight;
  const PoseRt at = split_pose(pose_from(t, q));
  float out_R[9], out_t[3];
  AlignResult out;
  std::memset(&out.info, 0, sizeof out.info);
  check(mrh_align_map(ctx_, other.ctx_, &p, at.R, at.t, out_R, out_t, &out.info), "alignMap");
  fitted_pose(out, out_R, out_t);
  return out;
}

GeoWrapper::TrackResult GeoWrapper::trackDepthPose(const float* depth, size_t rows, size_t cols, const std::array<float, 16>& pose) {
  requireCamera("trackDepthImage", MRH_CAMERA_PINHOLE);
  if (!depth || rows != (size_t) cam_.rows || cols != (size_t) cam_.cols)
    throw std::runtime_error("GeoWrapper::trackDepthImage | the depth image must have the camera's rows x cols");
  return trackPose("trackDepthImage", depth, nullptr, 0, pose);
}

GeoWrapper::TrackResult GeoWrapper::trackCloudPose(const float* pts, size_t n, const std::array<float, 16>& pose) {
  requireCamera("trackPointCloud", MRH_CAMERA_SPHERICAL);
  if (!pts && n) throw std::runtime_error("GeoWrapper::trackPointCloud | no points");
  return trackPose("trackPointCloud", nullptr, pts, n, pose);
}

// depth != nullptr: the depth form of D20 on an image of the pinhole camera; else the points form on the cloud pts [n * 3], which
// reads the depth limits of the last setCamera and nothing else of it
GeoWrapper::TrackResult GeoWrapper::trackSdfPose(const char* who, const float* depth, size_t rows, size_t cols, const float* pts, size_t n,
                                                 const std::array<float, 16>& pose) {
  const std::string at_who = std::string("GeoWrapper::") + who + " | ";
  if (depth) {
    requireCamera(who, MRH_CAMERA_PINHOLE);
    if (rows != (size_t) cam_.rows || cols != (size_t) cam_.cols) throw std::runtime_error(at_who + "the depth image must have the camera's rows x cols");
  } else {
    if (!cam_.set) throw std::runtime_error(at_who + "setCamera has not been called");
    if (!pts && n) throw std::runtime_error(at_who + "no points");
  }
  const mrh_sdftrack_params p = cameraParams<mrh_sdftrack_params>();  // band, iterations, min_pixels: the defaults
  const PoseRt at = split_pose(pose);
  float out_R[9], out_t[3];
  TrackResult out;
  std::memset(&out.info, 0, sizeof out.info);
  check(depth ? mrh_track_depth_sdf(ctx_, &p, depth, at.R, at.t, out_R, out_t, &out.info) : mrh_track_points_sdf(ctx_, &p, pts, n, at.R, at.t, out_R, out_t, &out.info), who);
  fitted_pose(out, out_R, out_t);
  return out;
}

void GeoWrapper::clearBuffers() {
  std::cout << "clearing buffers..." << std::endl;
  cacheMesh();  // the mesh of the last extractMesh outlives the map, as the reference's host matrices do
  check(mrh_reset(ctx_), "clearBuffers");
  flags_announced_ = last_compute_flags_ = 0;
  grid_.clear();  // Streamer::clearGrid (geowrapper.cpp:555)
}

void GeoWrapper::serializeData(const std::string& filename_hash, const std::string& filename_voxel) {
  const Blocks dev = dumpBlocks("serializeData", true);
  std::vector<gw::DataPoint> hash_pts, voxel_pts;
  gw::dataPoints(dev.descs.data(), dev.voxels.data(), dev.n, set_.virtual_voxel_size, hash_pts, voxel_pts);
  auto write = [](const std::string& fn, const std::vector<gw::DataPoint>& pts, bool with_sdf) {
    std::ofstream o(fn);
    if (!o.is_open()) { std::cerr << "GeoWrapper::serializeData | cannot open " << fn << std::endl; return; }
    gw::writeDataPoints(o, pts, with_sdf);
  };
  write(filename_hash, hash_pts, false);
  write(filename_voxel, voxel_pts, true);
  std::cout << "Streamer::serializeData | written " << hash_pts.size() << " hash points and " << voxel_pts.size() << " voxels to " << filename_hash
            << " and " << filename_voxel << std::endl;
}

void GeoWrapper::serializeGrid(const std::string& filename) {
  const Blocks dev = dumpBlocks("serializeGrid", true);
  std::ofstream o(filename, std::ios::binary);
  if (!o.is_open()) throw std::runtime_error("GeoWrapper::serializeGrid | cannot open " + filename);
  gw::writeGridHeader(o, dev.n + hostGridBlocks());  // device-resident blocks, then the streamer's host chunk grid
  for (uint64_t k = 0; k < dev.n; ++k) gw::writeGridBlock(o, dev.descs[k], &dev.voxels[k * 512]);
  for (const auto& kv : grid_.chunks())
    for (const gw::HostBlock& b : kv.second) gw::writeGridBlock(o, b.desc, b.voxels.data());
}

void GeoWrapper::deserializeGrid(const std::string& filename) {
  // inverse of serializeGrid: blocks are inserted (or overwritten) through mrh_import_blocks, the stream-in half of
  // the reference's streamer (Streamer::streamInToGPU, streamer.cpp:358-378) as far as a resident map needs it
  std::ifstream in(filename, std::ios::binary);
  if (!in.is_open()) throw std::runtime_error("GeoWrapper::deserializeGrid | cannot open " + filename);
  std::vector<mrh_block_desc> descs;
  std::vector<mrh_voxel> vox;
  const uint64_t n = gw::readGrid(in, filename, descs, vox);
  check(mrh_import_blocks(ctx_, descs.data(), vox.data(), n), "deserializeGrid");
}

void GeoWrapper::GSSavePointCloud(const std::string& folder) {
  if (!gs_enabled_) {
    std::cerr << "GeoWrapper::GSSavePointCloud | GS container not initialized" << std::endl;  // geowrapper.cpp:233-236
    return;
  }
  // the reference writes the optimised model (GaussianModel::Save_ply, src/gs/gaussian.cu:260-282) to
  // <folder>/point_cloud.ply; here the same file holds the seeds the model is initialised from
  const std::string mk = "mkdir -p '" + folder + "'";
  if (std::system(mk.c_str()) != 0) throw std::runtime_error("GeoWrapper::GSSavePointCloud | cannot create " + folder);
  std::ofstream ply(folder + "/point_cloud.ply");
  if (!ply.is_open()) throw std::runtime_error("GeoWrapper::GSSavePointCloud | cannot write " + folder + "/point_cloud.ply");
  gw::writeSeeds(ply, seeds_);
  std::cout << "GeoWrapper::GSSavePointCloud | written " << seeds_.size() << " splat seeds to " << folder << std::endl;
}

void GeoWrapper::GSFinalOpt() {  // geowrapper.cpp:241-244: no-op without a GS container
  if (gs_enabled_) throw std::runtime_error("GeoWrapper::GSFinalOpt | Gaussian-splatting optimisation is outside this library's scope");
}

}  // namespace pygeowrapper
