// geowrapper.h — C++ host facade with the reference's GeoWrapper surface (geowrapper.h:18-260 of
// rvp-group/mrhash), sitting on the C ABI of include/mrhash_hip.h.  No CUDA/HIP types appear here: the
// facade owns host-side copies of the inputs (the reference's setters copy too, geowrapper.cpp:246-321)
// and one opaque mrh_ctx.
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "mrhash_hip.h"
#include "mrhash_comm.h"
#include "mrhash_raycast.h"
#include "mrhash_esdf.h"
#include "mrhash_query.h"
#include "mrhash_rays.h"
#include "mrhash_remap.h"
#include "mrhash_align.h"
#include "mrhash_track.h"
#include "mrhash_sdftrack.h"
#include "mrhash_normals.h"

#include "gw_chunks.h"
#include "gw_pose.h"

namespace pygeowrapper {

class GeoWrapper {
public:
  // same 15 arguments, same order, same defaults as geowrapper.h:63-78 / pygeowrapper.cpp:14-29
  GeoWrapper(float sdf_truncation, float sdf_truncation_scale, int integration_weight_sample, float virtual_voxel_size,
             int n_frames_invalidate_voxels, int voxel_extents_scale, bool viewer_active, float marching_cubes_threshold,
             uint8_t min_weight_threshold, float min_depth, float max_depth, const std::string& gs_optimization_param_path = "",
             float sdf_var_threshold = 0.f, float vertices_merging_threshold = 0.f, bool projective_sdf = true);
  ~GeoWrapper();
  GeoWrapper(const GeoWrapper&) = delete;
  GeoWrapper& operator=(const GeoWrapper&) = delete;

  // getters / setters: like the reference they only touch the cached host copy (geowrapper.h:80-109)
  int getHashNumBuckets() const { return set_.hash_num_buckets; }  void setHashNumBuckets(int v) { set_.hash_num_buckets = v; }
  int getNumSdfBlocks() const { return set_.num_sdf_blocks; }  void setNumSdfBlocks(int v) { set_.num_sdf_blocks = v; }
  int getHashBucketSize() const { return set_.hash_bucket_size; }  void setHashBucketSize(int v) { set_.hash_bucket_size = v; }
  float getSdfTruncation() const { return set_.sdf_truncation; }  void setSdfTruncation(float v) { set_.sdf_truncation = v; }
  float getSdfTruncationScale() const { return set_.sdf_truncation_scale; }  void setSdfTruncationScale(float v) { set_.sdf_truncation_scale = v; }
  int getIntegrationWeightSample() const { return set_.integration_weight_sample; }  void setIntegrationWeightSample(int v) { set_.integration_weight_sample = v; }
  int getIntegrationWeightMax() const { return set_.integration_weight_max; }  void setIntegrationWeightMax(int v) { set_.integration_weight_max = v; }
  float getVirtualVoxelSize() const { return set_.virtual_voxel_size; }  void setVirtualVoxelSize(float v) { set_.virtual_voxel_size = v; }
  int getLinkedListSize() const { return set_.linked_list_size; }  void setLinkedListSize(int v) { set_.linked_list_size = v; }
  int getNFramesInvalidateVoxels() const { return set_.n_frames_invalidate_voxels; }  void setNFramesInvalidateVoxels(int v) { set_.n_frames_invalidate_voxels = v; }
  int getMaxNumSdfBlockIntegrateFromGlobalHash() const { return set_.max_num_sdf_block_integrate_from_global_hash; }  void setMaxNumSdfBlockIntegrateFromGlobalHash(int v) { set_.max_num_sdf_block_integrate_from_global_hash = v; }
  int getVoxelExtentsScale() const { return set_.voxel_extents_scale; }  void setVoxelExtentsScale(int v) { set_.voxel_extents_scale = v; }

  // translation <tx,ty,tz>, quaternion <qx,qy,qz,qw> (geowrapper.cpp:86-92)
  void setCurrPose(const std::array<float, 3>& t, const std::array<float, 4>& q);
  const std::array<float, 16>& getCurrPose() const { return pose_; }  // row-major 4x4
  void setCameraInLidar(const std::array<float, 16>& m) { camera_in_lidar_ = m; }
  void setCamera(float fx, float fy, float cx, float cy, int rows, int cols, float min_depth, float max_depth, int camera_model);

  // raw-pointer forms of the numpy setters; shape checks live in the binding (geowrapper.cpp:246-321)
  void setDepthImage(const float* data, size_t rows, size_t cols);
  void setRGBImage(const uint8_t* data, size_t rows, size_t cols);
  // normals_or_null: one per point, or none; compute_normals (without normals): compute() estimates them on the device
  // (mrh_estimate_normals), as the reference's MAD-tree does on the host (geowrapper.cpp:374-404)
  void setPointCloud(const float* pts, size_t n, const float* normals_or_null, bool compute_normals = false);
  const std::vector<float>& pointCloud() const { return point_cloud_; }
  // the normals given to setPointCloud, or, after a compute() that estimated them, those: read back on the first call only
  const std::vector<float>& normals() const;

  void compute();                                // geowrapper.cpp:118-148
  void extractMesh(const std::string& filename);  // geowrapper.cpp:150-230
  // V / F / C of the last extractMesh.  The library keeps them (until the next extraction); the copies the getters hand out are
  // made on first use — extractMesh itself formats the PLY straight from the library's buffers (83 MB of copies, a third
  // of the call, when nobody asks for the arrays).
  const std::vector<double>& vertices() const { cacheMesh(); return mesh_.V; }
  const std::vector<int32_t>& faces() const { cacheMesh(); return mesh_.F; }
  const std::vector<double>& colors() const { cacheMesh(); return mesh_.C; }

  void streamAllOut();
  // Streamer::stream (streamer.cpp:333-354): blocks farther than `radius` from `camera_position` leave the device for the
  // host chunk grid, chunks inside the sphere come back.  compute() calls it when the pool runs low (geowrapper.cpp:137-138).
  void stream(const std::array<float, 3>& camera_position, float radius);
  size_t hostGridBlocks() const { return grid_.blocks(); }  // blocks currently held by the host chunk grid
  void setSyncCompute(bool on) { sync_compute_ = on; }
  uint32_t lastComputeFlags() const { return last_compute_flags_; }  // sync mode: flags the last compute() raised (1 pool, 2 table, 4 key range)
  void clearBuffers();
  void serializeData(const std::string& filename_hash, const std::string& filename_voxel);
  void serializeGrid(const std::string& filename);
  void deserializeGrid(const std::string& filename);
  void GSSavePointCloud(const std::string& folder);
  void GSFinalOpt();
  const std::vector<mrh_splat_seed>& splatSeeds() const { return seeds_; }  // accumulated over compute() calls

  // ---- rendering (include/mrhash_raycast.h; no reference counterpart): the map seen by the camera of the last setCamera
  // (intrinsics, rows, cols, min and max depth), from the current pose (getCurrPose) or from (t, q) converted as setCurrPose
  // does.  depth [rows * cols] (camera z, metres), normals [rows * cols * 3] (world frame), colors [rows * cols * 3], row-major;
  // a pixel without a hit is 0 in all three.  A spherical camera throws std::runtime_error (raycastScan renders it).  Blocks paged out to the host
  // grid (stream(), streamAllOut()) are not on the device and are not rendered.
  struct RaycastImages {
    int rows = 0, cols = 0;
    std::vector<float> depth, normals;
    std::vector<uint8_t> colors;
  };
  RaycastImages raycast() { return raycastPose(pose_); }
  RaycastImages raycast(const std::array<float, 3>& t, const std::array<float, 4>& q) { return raycastPose(gw::pose_from(t, q)); }
  // The same for the spherical camera of the last setCamera (LiDAR scans, range images): range [rows * cols] (metres along the
  // ray) instead of depth, and the crossings as sensor-frame points [rows * cols * 3] — an organised scan of `cols` points per
  // row with (0, 0, 0) for a ray without a hit, which setPointCloud takes as it is.  A pinhole camera throws std::runtime_error.
  struct RaycastScan {
    int rows = 0, cols = 0;
    std::vector<float> range, normals, points;
    std::vector<uint8_t> colors;
  };
  RaycastScan raycastScan() { return raycastScanPose(pose_); }
  RaycastScan raycastScan(const std::array<float, 3>& t, const std::array<float, 4>& q) { return raycastScanPose(gw::pose_from(t, q)); }

  // ---- distance fields (include/mrhash_esdf.h; no reference counterpart): the Euclidean signed distance to the
  // nearest surface for every finest voxel of the world box [lo, hi] (metres), exact up to max_distance.  Per axis the box is
  // origin = floor(lo / vs + 0.5) .. floor(hi / vs + 0.5) in voxels (in double), the reach ceil(max_distance / vs) voxels.  Only
  // surface inside the box is seen: pad the box by max_distance.  dist [nx * ny * nz] metres and state [nx * ny * nz] (MRH_ESDF_*
  // bits), x fastest.  Throws std::runtime_error when hi < lo or a side exceeds MRH_ESDF_MAX_SIDE voxels.
  struct DistanceField {
    std::array<int32_t, 3> origin{}, dims{};
    std::vector<float> dist;
    std::vector<uint8_t> state;
  };
  DistanceField distanceField(const std::array<float, 3>& lo, const std::array<float, 3>& hi, float max_distance);

  // ---- point queries (include/mrhash_query.h; no reference counterpart): TSDF distance (metres), gradient, colour
  // and weight of the map at n points [n * 3].  smooth = false: the map's own field (the reference's trilinearInterpolation, what
  // the mesh and the render see: the mean of eight cells, piecewise constant inside a dual cell); smooth = true: the continuous
  // field with its analytic gradient, for planners and registration.  sensor_frame = false: world points; true: points in the
  // sensor frame at the pose of the last setCurrPose, (0, 0, 0) = no return (refused) — raycastScan's points as they are.
  // dist [n], grad [n * 3], rgbw [n * 4] = r, g, b, weight, state [n] (MRH_QUERY_* bits).
  struct PointQuery {
    std::vector<float> dist, grad;
    std::vector<uint8_t> rgbw, state;
  };
  PointQuery queryPoints(const float* pts, size_t n, bool smooth = false, bool sensor_frame = false);

  // ---- ray queries (include/mrhash_rays.h; no reference counterpart): n rays, each with its own origin [n * 3],
  // direction [n * 3] and, with tmax [n] (nullptr: none), its own end, cast through the map: samples at min_range + k * step
  // (step 0 = half the truncation) up to max_range.  normalize = true divides every direction here, on the host, in binary32:
  // len = sqrtf((dx * dx + dy * dy) + dz * dz), d / len per component — ranges are metres then; false: the directions as given,
  // ranges count multiples of them.  sensor_frame as in queryPoints.  Neighbouring rays share a wave: order them so that
  // neighbours are close in space.  range [n], status [n] (MRH_RAY_* bits; 0 = every sample was observed free space), normals
  // [n * 3], rgb [n * 3], counts [n * 2] = n_free, n_unknown, first_unknown [n].
  struct RayCast {
    std::vector<float> range, normals, first_unknown;
    std::vector<uint8_t> status, rgb;
    std::vector<uint32_t> counts;
  };
  RayCast castRays(const float* origins, const float* directions, size_t n, float max_range, float min_range = 0.f, float step = 0.f, const float* tmax = nullptr,
                   bool sensor_frame = false, bool normalize = true);

  // ---- map-to-map fusion (include/mrhash_remap.h; no reference counterpart): the map of `other`, whose frame lies
  // at the pose (t, q) — as setCurrPose takes it — in this map's world, resampled at this map's voxel size and merged into it
  // voxel by voxel (MRH_UNPACK_MERGE).  `other` is only read.  Blocks that either wrapper's host chunk grid has paged out take no
  // part: only `other`'s device map is resampled, and the records merge into this wrapper's device map.
  mrh_remap_info fuseMap(GeoWrapper& other, const std::array<float, 3>& t, const std::array<float, 4>& q, uint32_t min_weight = 0);

  // ---- map-to-map registration (include/mrhash_align.h; no reference counterpart): the pose of `other`'s frame in
  // this map's world, estimated from the two maps alone, started from (t, q) — as fuseMap takes it — with every parameter of
  // mrh_align_params at its default unless given.  Both wrappers are only read; blocks paged out to either host chunk grid take no
  // part.  Returns the pose as fuseMap takes it: alignMap -> fuseMap closes the loop.  info.status == MRH_ALIGN_LOST: (t, q) is the
  // pose from before the step that failed.
  struct AlignResult {
    std::array<float, 3> t;
    std::array<float, 4> q;  // qx, qy, qz, qw
    mrh_align_info info;
  };
  AlignResult alignMap(GeoWrapper& other, const std::array<float, 3>& t, const std::array<float, 4>& q, int iterations = 0, uint32_t min_weight = 0);

  // ---- tracking (include/mrhash_track.h; no reference counterpart): the pose of a depth image (rows x cols as
  // the camera of the last setCamera, metres) by point-to-plane ICP against the map, started from the current pose (setCurrPose)
  // or from (t, q).  Every parameter of mrh_track_params at its default.  Returns the pose as setCurrPose takes it; pose_ is left
  // alone — the SLAM loop is trackDepthImage -> setCurrPose -> setDepthImage -> compute.  info.status == MRH_TRACK_LOST: (t, q) is
  // the pose from before the step that failed.  A spherical camera throws std::runtime_error.
  struct TrackResult {
    std::array<float, 3> t;
    std::array<float, 4> q;  // qx, qy, qz, qw
    mrh_track_info info;
  };
  TrackResult trackDepthImage(const float* depth, size_t rows, size_t cols) { return trackDepthPose(depth, rows, cols, pose_); }
  TrackResult trackDepthImage(const float* depth, size_t rows, size_t cols, const std::array<float, 3>& t, const std::array<float, 4>& q) { return trackDepthPose(depth, rows, cols, gw::pose_from(t, q)); }
  // The same for a LiDAR scan: n sensor-frame points [n * 3], organised or not, (0, 0, 0) = no return, against one
  // spherical render of the map with the camera of the last setCamera(..., model = 1).  The loop is trackPointCloud -> setCurrPose
  // -> setPointCloud -> compute; the cloud given to setPointCloud is neither read nor replaced.  A pinhole camera throws
  // std::runtime_error.  The map must render the ground for the height to be observable: a truncation of 4 voxels does (D15).
  TrackResult trackPointCloud(const float* pts, size_t n) { return trackCloudPose(pts, n, pose_); }
  TrackResult trackPointCloud(const float* pts, size_t n, const std::array<float, 3>& t, const std::array<float, 4>& q) { return trackCloudPose(pts, n, gw::pose_from(t, q)); }
  // ---- render-free tracking (include/mrhash_sdftrack.h; no reference counterpart): the same two calls without the
  // render — the image's back-projected pixels, or the cloud's points, are registered against the map's own distance field.
  // Intrinsics and depth limits are those of the last setCamera; band, iterations and min_pixels at their defaults.  The depth
  // form needs a pinhole camera; the points form reads the depth limits only and accepts either camera model: no field of view,
  // no azimuth seam, and no ground that has to render.  A point further than the truncation from the surface gives no row.
  TrackResult trackDepthImageSDF(const float* depth, size_t rows, size_t cols) { return trackSdfPose("trackDepthImageSDF", depth, rows, cols, nullptr, 0, pose_); }
  TrackResult trackDepthImageSDF(const float* depth, size_t rows, size_t cols, const std::array<float, 3>& t, const std::array<float, 4>& q) { return trackSdfPose("trackDepthImageSDF", depth, rows, cols, nullptr, 0, gw::pose_from(t, q)); }
  TrackResult trackPointCloudSDF(const float* pts, size_t n) { return trackSdfPose("trackPointCloudSDF", nullptr, 0, 0, pts, n, pose_); }
  TrackResult trackPointCloudSDF(const float* pts, size_t n, const std::array<float, 3>& t, const std::array<float, 4>& q) { return trackSdfPose("trackPointCloudSDF", nullptr, 0, 0, pts, n, gw::pose_from(t, q)); }

  // ---- multi-GPU (include/mrhash_comm.h; no reference counterpart): one GeoWrapper per process / GPU.
  // commUniqueId() on one rank, the 128 bytes handed to the others by the launcher, then commInit on every rank.
  //   tile_sharded = true : the result-identical mode — every rank is given every frame, compute() fuses the tiles this rank
  //                         owns (starve frames reduce over the ranks inside the library), extractMesh() exchanges the boundary
  //                         blocks, gathers the per-rank extractions on rank 0 and writes the file there (other ranks: no file,
  //                         empty V / F / C).
  //   tile_sharded = false: frame sharding — every rank fuses its own frames into its own sub-map; mergeSubmaps() folds them
  //                         into one tile-sharded map, after which extractMesh() works as above.
  static std::array<uint8_t, MRH_COMM_ID_BYTES> commUniqueId();
  void commInit(const std::array<uint8_t, MRH_COMM_ID_BYTES>& id, int rank, int world, int chunk_log2 = 3, bool tile_sharded = true);
  void mergeSubmaps();
  int commRank() const { return comm_.rank; }
  int commWorld() const { return comm_.world; }

  mrh_ctx* ctx() { return ctx_; }

private:
  void check(int rc, const char* what) const;

  // ---- the reference's cached settings (geowrapper.h:80-109): host copies behind the getters and setters
  struct Settings {
    int hash_num_buckets = 0, num_sdf_blocks = 0, hash_bucket_size = 10, linked_list_size = 7, max_num_sdf_block_integrate_from_global_hash = 0;
    int integration_weight_sample, integration_weight_max = 255, n_frames_invalidate_voxels, voxel_extents_scale;
    float sdf_truncation, sdf_truncation_scale, virtual_voxel_size, sdf_var_threshold, vertices_merging_threshold;
    uint8_t min_weight_threshold;
  } set_;
  std::array<float, 16> pose_;
  std::array<float, 16> camera_in_lidar_;

  // ---- the camera of the last setCamera, for the renders and the tracking calls
  struct Camera {
    bool set = false;
    int model = MRH_CAMERA_PINHOLE, rows = 0, cols = 0;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f, min_depth = 0.f, max_depth = 0.f;
    float reach = 0.f;  // farthest distance from the camera centre at which a frame can touch a block
  } cam_;
  template <typename Params> Params cameraParams() const;    // intrinsics, shape and depth range of the last setCamera; the rest 0
  void requireCamera(const char* method, int model) const;   // throws unless setCamera was called with that camera model
  RaycastImages raycastPose(const std::array<float, 16>& pose);
  RaycastScan raycastScanPose(const std::array<float, 16>& pose);
  TrackResult trackDepthPose(const float* depth, size_t rows, size_t cols, const std::array<float, 16>& pose);
  TrackResult trackCloudPose(const float* pts, size_t n, const std::array<float, 16>& pose);
  TrackResult trackPose(const char* who, const float* depth, const float* pts, size_t n, const std::array<float, 16>& pose);
  TrackResult trackSdfPose(const char* who, const float* depth, size_t rows, size_t cols, const float* pts, size_t n, const std::array<float, 16>& pose);

  // ---- inputs of compute()
  bool have_depth_ = false, have_rgb_ = false;  // the images themselves live in the library (pinned staging + device slots)
  std::vector<float> point_cloud_;
  mutable std::vector<float> normals_;
  bool estimate_normals_ = false;           // setPointCloud(..., compute_normals = true): compute() estimates on the device
  mutable bool normals_on_device_ = false;  // ... and did: normals_ is filled by the first normals() after it
  bool sync_compute_ = false;               // MRH_SYNC_COMPUTE=1: compute() blocks and reports its own frame's flags (the reference's contract)
  uint32_t flags_announced_ = 0, last_compute_flags_ = 0;

  // ---- host side of the streamer (gw_chunks.h): the chunk grid of streamed-out blocks
  gw::ChunkGrid grid_;
  bool streaming_enabled_ = true;  // MRHASH_STREAM=0 turns the per-frame test off
  float chunkExt() const { return (float) set_.voxel_extents_scale; }  // chunk edge in metres (geowrapper.cpp:56)
  void streamOutToGrid(const std::array<float, 3>& center, float radius);
  void streamInGathered(const char* what, const gw::ChunkGrid::Gathered& g);  // gather -> import -> erase only after the import succeeded
  void streamInSphere(const std::array<float, 3>& center, float radius);      // every chunk that touches the sphere
  struct Blocks {
    std::vector<mrh_block_desc> descs;  // at least one element long, as voxels: data() is never null
    std::vector<mrh_voxel> voxels;
    uint64_t n = 0;
  };
  Blocks dumpBlocks(const char* what, bool with_voxels);  // the device-resident blocks (mrh_dump_blocks: count, then fill)

  // ---- the mesh of the last extractMesh: a view of the library's buffers (mrh_extract_mesh), copied on the first getter
  struct MeshView {
    std::vector<double> V, C;
    std::vector<int32_t> F;
    bool cached = true;
    const double *v = nullptr, *c = nullptr;
    const int32_t* f = nullptr;
    uint64_t nv = 0, nf = 0;
  };
  mutable MeshView mesh_;
  void cacheMesh() const;
  void writeMesh(const std::string& filename, double t0);

  // ---- 3DGS initialisation: on when a gs_optimization_param_path was given
  bool gs_enabled_ = false;
  float qtree_thresh_ = 0.1f;
  int qtree_min_pixel_size_ = 1;
  std::vector<mrh_splat_seed> seeds_;

  mrh_ctx* ctx_ = nullptr;
  int device_id_ = 0;
  struct Comm {
    mrh_comm* comm = nullptr;
    int rank = 0, world = 1, chunk_log2 = 3;
    bool tile_sharded = false;
  } comm_;
};

}  // namespace pygeowrapper
