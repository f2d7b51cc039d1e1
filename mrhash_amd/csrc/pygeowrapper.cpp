// pygeowrapper.cpp — pybind11 binding with the surface of the reference's nanobind module
// (pybind/pygeowrapper.cpp:12-84): module `pygeowrapper`, class `GeoWrapper`, same method names, argument
// names/order/defaults and error behaviour (RuntimeError on shape violations).  nanobind is not available in
// this image; pybind11 returns numpy arrays where the reference returns Eigen matrices.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <optional>
#include <vector>
#include <pybind11/stl.h>

#include "geowrapper.h"

namespace py = pybind11;
using pygeowrapper::GeoWrapper;

namespace {

using FloatArray = py::array_t<float, py::array::c_style | py::array::forcecast>;  // any array-like, converted to contiguous float32
using OptFloatArray = std::optional<FloatArray>;

[[noreturn]] void refuse(const char* who, const char* what) { throw std::runtime_error(std::string("GeoWrapper::") + who + "|" + what); }

std::array<float, 3> vec3(const FloatArray& a) { return {a.data()[0], a.data()[1], a.data()[2]}; }

// (t, q) = (<tx,ty,tz>, <qx,qy,qz,qw>) as setCurrPose takes them
struct Pose { std::array<float, 3> t; std::array<float, 4> q; };
Pose pose_arg(const char* who, const FloatArray& t, const FloatArray& q) {
  if (t.size() != 3 || q.size() != 4) refuse(who, "expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
  return {vec3(t), {q.data()[0], q.data()[1], q.data()[2], q.data()[3]}};
}
// ... both or neither: no pose = the current one
std::optional<Pose> pose_arg(const char* who, const OptFloatArray& t, const OptFloatArray& q) {
  if (t.has_value() != q.has_value()) refuse(who, "give both t and q, or neither");
  if (!t) return std::nullopt;
  return pose_arg(who, *t, *q);
}

// [n, 3], or flat with 3 n elements
bool is_xyz(const FloatArray& a) { return (a.ndim() == 2 && a.shape(1) == 3) || (a.ndim() == 1 && a.size() % 3 == 0); }

template <typename T> py::array_t<T> to_numpy(const T* data, size_t n, const std::vector<size_t>& shape) {
  py::array_t<T> a(shape);
  if (n) std::memcpy(a.mutable_data(), data, n * sizeof(T));
  return a;
}
template <typename T> py::array_t<T> to_numpy(const std::vector<T>& v, const std::vector<size_t>& shape) { return to_numpy(v.data(), v.size(), shape); }
template <typename T> py::array_t<T> rows_of(const std::vector<T>& v, size_t cols) { return to_numpy(v, {v.size() / cols, cols}); }
template <typename T, size_t N> py::array_t<T> to_numpy(const std::array<T, N>& a) { return to_numpy(a.data(), N, {N}); }
template <typename T, size_t N> py::array_t<T> to_numpy(const T (&a)[N]) { return to_numpy(a, N, {N}); }

py::dict track_info(const mrh_track_info& i) {
  py::dict d;
  d["status"] = i.status; d["iterations_done"] = i.iterations_done; d["pixels"] = i.pixels; d["rms"] = i.rms; d["sums"] = to_numpy(i.sums);
  return d;
}

py::dict align_info(const mrh_align_info& i) {
  py::dict d;
  d["status"] = i.status; d["iterations_done"] = i.iterations_done; d["source_blocks"] = i.source_blocks;
  d["samples"] = i.samples; d["accepted"] = i.accepted; d["rms"] = i.rms;
  d["pivot"] = to_numpy(i.pivot); d["extent"] = i.extent; d["sums"] = to_numpy(i.sums);
  return d;
}

py::dict fuse_info(const mrh_remap_info& i) {
  py::dict d;
  d["source_blocks"] = i.source_blocks; d["candidate_blocks"] = i.candidate_blocks; d["records"] = i.records;
  d["valid_voxels"] = i.valid_voxels; d["taken"] = i.taken;
  return d;
}

// (t [3], q [4] = qx,qy,qz,qw, info dict) of a tracking call
py::tuple track_tuple(const GeoWrapper::TrackResult& r) { return py::make_tuple(to_numpy(r.t), to_numpy(r.q), track_info(r.info)); }

}  // namespace

PYBIND11_MODULE(pygeowrapper, m) {
  m.doc() = "MI355X-native drop-in for mrhash.src.pygeowrapper (HIP kernels behind include/mrhash_hip.h)";
  py::class_<GeoWrapper>(m, "GeoWrapper")
    .def(py::init<float, float, int, float, int, int, bool, float, uint8_t, float, float, std::string, float, float, bool>(),
         py::arg("sdf_truncation"), py::arg("sdf_truncation_scale"), py::arg("integration_weight_sample"), py::arg("virtual_voxel_size"),
         py::arg("n_frames_invalidate_voxels"), py::arg("voxel_extents_scale"), py::arg("viewer_active"), py::arg("marching_cubes_threshold"),
         py::arg("min_weight_threshold"), py::arg("min_depth"), py::arg("max_depth"), py::arg("gs_optimization_param_path") = "",
         py::arg("sdf_var_threshold") = 0.f, py::arg("vertices_merging_threshold") = 0.f, py::arg("projective_sdf") = true)
    // the cached settings, then the other getters
    .def("getHashNumBuckets", &GeoWrapper::getHashNumBuckets).def("setHashNumBuckets", &GeoWrapper::setHashNumBuckets)
    .def("getNumSdfBlocks", &GeoWrapper::getNumSdfBlocks).def("setNumSdfBlocks", &GeoWrapper::setNumSdfBlocks)
    .def("getHashBucketSize", &GeoWrapper::getHashBucketSize).def("setHashBucketSize", &GeoWrapper::setHashBucketSize)
    .def("getSdfTruncation", &GeoWrapper::getSdfTruncation).def("setSdfTruncation", &GeoWrapper::setSdfTruncation)
    .def("getSdfTruncationScale", &GeoWrapper::getSdfTruncationScale).def("setSdfTruncationScale", &GeoWrapper::setSdfTruncationScale)
    .def("getIntegrationWeightSample", &GeoWrapper::getIntegrationWeightSample).def("setIntegrationWeightSample", &GeoWrapper::setIntegrationWeightSample)
    .def("getIntegrationWeightMax", &GeoWrapper::getIntegrationWeightMax).def("setIntegrationWeightMax", &GeoWrapper::setIntegrationWeightMax)
    .def("getVirtualVoxelSize", &GeoWrapper::getVirtualVoxelSize).def("setVirtualVoxelSize", &GeoWrapper::setVirtualVoxelSize)
    .def("getLinkedListSize", &GeoWrapper::getLinkedListSize).def("setLinkedListSize", &GeoWrapper::setLinkedListSize)
    .def("getNFramesInvalidateVoxels", &GeoWrapper::getNFramesInvalidateVoxels).def("setNFramesInvalidateVoxels", &GeoWrapper::setNFramesInvalidateVoxels)
    .def("getMaxNumSdfBlockIntegrateFromGlobalHash", &GeoWrapper::getMaxNumSdfBlockIntegrateFromGlobalHash).def("setMaxNumSdfBlockIntegrateFromGlobalHash", &GeoWrapper::setMaxNumSdfBlockIntegrateFromGlobalHash)
    .def("getVoxelExtentsScale", &GeoWrapper::getVoxelExtentsScale).def("setVoxelExtentsScale", &GeoWrapper::setVoxelExtentsScale)
    .def("getCurrPose", [](const GeoWrapper& g) { return to_numpy(g.getCurrPose().data(), 16, {4, 4}); })
    .def("getPointCloud", [](const GeoWrapper& g) { return rows_of(g.pointCloud(), 3); })
    .def("getNormals", [](const GeoWrapper& g) { return rows_of(g.normals(), 3); })
    .def("getVertices", [](const GeoWrapper& g) { return rows_of(g.vertices(), 3); })
    .def("getFaces", [](const GeoWrapper& g) { return rows_of(g.faces(), 3); })
    .def("getColors", [](const GeoWrapper& g) { return rows_of(g.colors(), 3); })
    // the other setters
    .def("setRGBImage", [](GeoWrapper& g, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
      // geowrapper.cpp:246-274 (the reference runner passes float32 RGB and relies on the implicit cast)
      if (a.ndim() != 3) refuse("setRGBImage", "input should be a 3D numpy array");
      if (a.shape(2) != 3) refuse("setRGBImage", "input should have 3 channels");
      g.setRGBImage(a.data(), (size_t) a.shape(0), (size_t) a.shape(1));
    })
    .def("setDepthImage", [](GeoWrapper& g, FloatArray a) {
      // geowrapper.cpp:300-321
      if (a.ndim() != 2) refuse("setDepthImage", "input should be a 2D numpy array");
      g.setDepthImage(a.data(), (size_t) a.shape(0), (size_t) a.shape(1));
    })
    .def("setPointCloud", [](GeoWrapper& g, FloatArray pts, bool compute_normals) {
      // geowrapper.cpp:345-405: [N, 3] points in the sensor frame (the runners pass points[:, :3]); copied
      if (pts.ndim() != 2) refuse("setPointCloud", "input should be a 2D numpy array");
      if (pts.shape(1) < 3) refuse("setPointCloud", "input should have at least 3 columns (x, y, z)");
      std::vector<float> xyz;  // the first three of more columns
      if (pts.shape(1) != 3) {
        xyz.resize((size_t) pts.shape(0) * 3);
        auto r = pts.unchecked<2>();
        for (py::ssize_t i = 0; i < pts.shape(0); i++) { xyz[3 * i] = r(i, 0); xyz[3 * i + 1] = r(i, 1); xyz[3 * i + 2] = r(i, 2); }
      }
      g.setPointCloud(pts.shape(1) == 3 ? pts.data() : xyz.data(), (size_t) pts.shape(0), nullptr, compute_normals);
    }, py::arg("input_point_cloud"), py::arg("compute_normals") = false)
    .def("setPointCloud", [](GeoWrapper& g, FloatArray pts, FloatArray normals) {
      // geowrapper.cpp:460-490
      if (pts.ndim() != 2) refuse("setPointCloud", "point cloud input should be a 2D numpy array");
      if (normals.ndim() != 2) refuse("setPointCloud", "normals input should be a 2D numpy array");
      if (pts.shape(0) != normals.shape(0)) refuse("setPointCloud", "point_cloud input and normals input should have the same number of points");
      g.setPointCloud(pts.data(), (size_t) pts.shape(0), normals.data());
    })
    .def("setCamera", &GeoWrapper::setCamera)
    .def("setCurrPose", [](GeoWrapper& g, FloatArray t, FloatArray q) {
      const Pose p = pose_arg("setCurrPose", t, q);
      g.setCurrPose(p.t, p.q);
    })
    .def("setCameraInLidar", [](GeoWrapper& g, FloatArray m4) {
      if (m4.size() != 16) refuse("setCameraInLidar", "expected a 4x4 matrix");
      std::array<float, 16> a;
      std::memcpy(a.data(), m4.data(), 16 * sizeof(float));
      g.setCameraInLidar(a);
    })
    .def("compute", &GeoWrapper::compute)
    .def("extractMesh", &GeoWrapper::extractMesh)
    .def("GSSavePointCloud", &GeoWrapper::GSSavePointCloud)
    .def("GSFinalOpt", &GeoWrapper::GSFinalOpt)
    .def("streamAllOut", &GeoWrapper::streamAllOut)
    // not part of the reference binding: lets tests drive and observe the streamer directly
    .def("_stream", [](GeoWrapper& g, FloatArray pos, float radius) {
      if (pos.size() != 3) refuse("_stream", "expected a 3-vector");
      g.stream(vec3(pos), radius);
    })
    .def("_hostGridBlocks", &GeoWrapper::hostGridBlocks)
    .def("_setSyncCompute", &GeoWrapper::setSyncCompute)
    .def("_lastComputeFlags", &GeoWrapper::lastComputeFlags)
    // multi-GPU (include/mrhash_comm.h, no reference counterpart): RCCL behind the C ABI, one GeoWrapper per rank
    .def_static("_commUniqueId", []() {
      const auto id = GeoWrapper::commUniqueId();
      return py::bytes((const char*) id.data(), id.size());
    })
    .def("_commInit", [](GeoWrapper& g, py::bytes id, int rank, int world, int chunk_log2, bool tile_sharded) {
      const std::string b = id;
      if (b.size() != MRH_COMM_ID_BYTES) refuse("_commInit", "the id has 128 bytes");
      std::array<uint8_t, MRH_COMM_ID_BYTES> a;
      std::memcpy(a.data(), b.data(), a.size());
      g.commInit(a, rank, world, chunk_log2, tile_sharded);
    }, py::arg("id"), py::arg("rank"), py::arg("world"), py::arg("chunk_log2") = 3, py::arg("tile_sharded") = true)
    .def("_mergeSubmaps", &GeoWrapper::mergeSubmaps)
    // splat seeds accumulated so far (what the reference hands to GaussianModel::Add_gaussians): (xyz, scale, rgb)
    .def("_splatSeeds", [](const GeoWrapper& g) {
      const auto& seeds = g.splatSeeds();
      std::vector<float> xyz(seeds.size() * 3), scale(seeds.size());
      std::vector<uint8_t> rgb(seeds.size() * 3);
      for (size_t i = 0; i < seeds.size(); i++) {
        for (int k = 0; k < 3; k++) { xyz[3 * i + k] = seeds[i].p[k]; rgb[3 * i + k] = seeds[i].rgb[k]; }
        scale[i] = seeds[i].scale;
      }
      return py::make_tuple(rows_of(xyz, 3), rows_of(scale, 1), rows_of(rgb, 3));
    })
    // not part of the reference binding: renders the map with the camera of the last setCamera from the current pose, or from
    // (t, q) = (<tx,ty,tz>, <qx,qy,qz,qw>); returns (depth [H, W] f32, normals [H, W, 3] f32 world frame, colors [H, W, 3] u8)
    .def("raycast", [](GeoWrapper& g, OptFloatArray t, OptFloatArray q) {
      const auto p = pose_arg("raycast", t, q);
      const GeoWrapper::RaycastImages im = p ? g.raycast(p->t, p->q) : g.raycast();
      const size_t H = (size_t) im.rows, W = (size_t) im.cols;
      return py::make_tuple(to_numpy(im.depth, {H, W}), to_numpy(im.normals, {H, W, 3}), to_numpy(im.colors, {H, W, 3}));
    }, py::arg("t") = py::none(), py::arg("q") = py::none())
    // ... and with the spherical camera of the last setCamera: (range [H, W] f32, normals [H, W, 3] f32 world frame, colors
    // [H, W, 3] u8, points [H * W, 3] f32 sensor frame — an organised scan, (0, 0, 0) where nothing was hit)
    .def("raycastScan", [](GeoWrapper& g, OptFloatArray t, OptFloatArray q) {
      const auto p = pose_arg("raycastScan", t, q);
      const GeoWrapper::RaycastScan im = p ? g.raycastScan(p->t, p->q) : g.raycastScan();
      const size_t H = (size_t) im.rows, W = (size_t) im.cols;
      return py::make_tuple(to_numpy(im.range, {H, W}), to_numpy(im.normals, {H, W, 3}), to_numpy(im.colors, {H, W, 3}), to_numpy(im.points, {H * W, 3}));
    }, py::arg("t") = py::none(), py::arg("q") = py::none())
    // not part of the reference binding: the Euclidean signed distance field of the world box [lo, hi] (metres), exact up to
    // max_distance; returns (dist [nz, ny, nx] f32 metres, state [nz, ny, nx] u8, origin (x, y, z) in voxels, dims (nx, ny, nz))
    .def("distanceField", [](GeoWrapper& g, FloatArray lo, FloatArray hi, float max_distance) {
      if (lo.size() != 3 || hi.size() != 3) refuse("distanceField", "expected two 3-vectors (lo, hi)");
      const GeoWrapper::DistanceField f = g.distanceField(vec3(lo), vec3(hi), max_distance);
      const std::vector<size_t> zyx = {(size_t) f.dims[2], (size_t) f.dims[1], (size_t) f.dims[0]};
      return py::make_tuple(to_numpy(f.dist, zyx), to_numpy(f.state, zyx), py::make_tuple(f.origin[0], f.origin[1], f.origin[2]),
                            py::make_tuple(f.dims[0], f.dims[1], f.dims[2]));
    }, py::arg("lo"), py::arg("hi"), py::arg("max_distance"))
    // not part of the reference binding: TSDF distance, gradient and colour of the map at points [n, 3] — world points, or with
    // sensor_frame = True points in the sensor frame at the pose of the last setCurrPose ((0, 0, 0) = no return, refused; what
    // raycastScan returns).  smooth = False: the map's own, piecewise-constant field; True: the continuous field.  Returns
    // (dist [n] f32, grad [n, 3] f32, rgbw [n, 4] u8 = r, g, b, weight, state [n] u8 of MRH_QUERY_* bits)
    .def("queryPoints", [](GeoWrapper& g, FloatArray points, bool smooth, bool sensor_frame) {
      if (!is_xyz(points)) refuse("queryPoints", "expected points of shape [n, 3]");
      const size_t n = (size_t) points.size() / 3;
      const GeoWrapper::PointQuery r = g.queryPoints(points.data(), n, smooth, sensor_frame);
      return py::make_tuple(to_numpy(r.dist, {n}), to_numpy(r.grad, {n, 3}), to_numpy(r.rgbw, {n, 4}), to_numpy(r.state, {n}));
    }, py::arg("points"), py::arg("smooth") = false, py::arg("sensor_frame") = false)
    // not part of the reference binding: rays cast through the map — origins [n, 3], directions [n, 3], tmax [n] or
    // None; world rays, or with sensor_frame = True rays in the sensor frame at the pose of the last setCurrPose.  normalize = True
    // divides each direction on the host in float32 by sqrt((dx * dx + dy * dy) + dz * dz).  Returns (range [n] f32, status [n] u8 of
    // MRH_RAY_* bits, normals [n, 3] f32, rgb [n, 3] u8, counts [n, 2] u32 = n_free, n_unknown, first_unknown [n] f32)
    .def("castRays", [](GeoWrapper& g, FloatArray origins, FloatArray directions, float max_range, float min_range, float step, py::object tmax,
                        bool sensor_frame, bool normalize) {
      if (!is_xyz(origins) || !is_xyz(directions) || origins.size() != directions.size()) refuse("castRays", "expected origins and directions of shape [n, 3]");
      const size_t n = (size_t) origins.size() / 3;
      FloatArray ends;
      if (!tmax.is_none()) {
        ends = FloatArray::ensure(tmax);
        if (!ends || (size_t) ends.size() != n) refuse("castRays", "expected tmax of shape [n]");
      }
      const GeoWrapper::RayCast r = g.castRays(origins.data(), directions.data(), n, max_range, min_range, step, tmax.is_none() ? nullptr : ends.data(), sensor_frame, normalize);
      return py::make_tuple(to_numpy(r.range, {n}), to_numpy(r.status, {n}), to_numpy(r.normals, {n, 3}), to_numpy(r.rgb, {n, 3}), to_numpy(r.counts, {n, 2}),
                            to_numpy(r.first_unknown, {n}));
    }, py::arg("origins"), py::arg("directions"), py::arg("max_range"), py::arg("min_range") = 0.f, py::arg("step") = 0.f, py::arg("tmax") = py::none(),
       py::arg("sensor_frame") = false, py::arg("normalize") = true)
    // not part of the reference binding: the map of `other`, whose frame lies at the pose (t, q) in this map's world, resampled at
    // this map's voxel size and merged into it.  Returns the counts of mrh_remap_info as a dict.  Blocks paged out to
    // either wrapper's host chunk grid take no part
    .def("fuseMap", [](GeoWrapper& g, GeoWrapper& other, FloatArray t, FloatArray q, uint32_t min_weight) {
      const Pose p = pose_arg("fuseMap", t, q);
      return fuse_info(g.fuseMap(other, p.t, p.q, min_weight));
    }, py::arg("other"), py::arg("t"), py::arg("q"), py::arg("min_weight") = 0)
    // not part of the reference binding: the pose of `other`'s frame in this map's world, estimated from the two maps alone (DESIGN.md
    // D19), started from (t, q) as fuseMap takes it.  Returns (t [3], q [4] = qx,qy,qz,qw, info dict): what fuseMap then takes
    .def("alignMap", [](GeoWrapper& g, GeoWrapper& other, FloatArray t, FloatArray q, int iterations, uint32_t min_weight) {
      const Pose p = pose_arg("alignMap", t, q);
      const GeoWrapper::AlignResult r = g.alignMap(other, p.t, p.q, iterations, min_weight);
      return py::make_tuple(to_numpy(r.t), to_numpy(r.q), align_info(r.info));
    }, py::arg("other"), py::arg("t"), py::arg("q"), py::arg("iterations") = 0, py::arg("min_weight") = 0)
    // not part of the reference binding: the pose of a depth image (2-D, the camera's rows x cols, metres) by ICP against the map,
    // started from the current pose or from (t, q); returns (t [3], q [4] = qx,qy,qz,qw, info dict) and leaves the current pose
    // alone — call setCurrPose(t, q) with the result before setDepthImage / compute
    .def("trackDepthImage", [](GeoWrapper& g, FloatArray depth, OptFloatArray t, OptFloatArray q) {
      if (depth.ndim() != 2) refuse("trackDepthImage", "input should be a 2D numpy array");
      const auto p = pose_arg("trackDepthImage", t, q);
      const size_t rows = (size_t) depth.shape(0), cols = (size_t) depth.shape(1);
      return track_tuple(p ? g.trackDepthImage(depth.data(), rows, cols, p->t, p->q) : g.trackDepthImage(depth.data(), rows, cols));
    }, py::arg("depth"), py::arg("t") = py::none(), py::arg("q") = py::none())
    // the same for a LiDAR scan ([N, 3] float32, sensor frame) under the spherical camera of setCamera(..., model = 1); the loop is
    // trackPointCloud -> setCurrPose -> setPointCloud -> compute
    .def("trackPointCloud", [](GeoWrapper& g, FloatArray pts, OptFloatArray t, OptFloatArray q) {
      if (pts.ndim() != 2 || pts.shape(1) != 3) refuse("trackPointCloud", "input should be a 2D numpy array with 3 columns");
      const auto p = pose_arg("trackPointCloud", t, q);
      const size_t n = (size_t) pts.shape(0);
      return track_tuple(p ? g.trackPointCloud(pts.data(), n, p->t, p->q) : g.trackPointCloud(pts.data(), n));
    }, py::arg("points"), py::arg("t") = py::none(), py::arg("q") = py::none())
    // not part of the reference binding: the two tracking calls without the render — the image's pixels, or the cloud's
    // points, against the map's own distance field; same arguments and result.  trackPointCloudSDF accepts either camera model
    .def("trackDepthImageSDF", [](GeoWrapper& g, FloatArray depth, OptFloatArray t, OptFloatArray q) {
      if (depth.ndim() != 2) refuse("trackDepthImageSDF", "input should be a 2D numpy array");
      const auto p = pose_arg("trackDepthImageSDF", t, q);
      const size_t rows = (size_t) depth.shape(0), cols = (size_t) depth.shape(1);
      return track_tuple(p ? g.trackDepthImageSDF(depth.data(), rows, cols, p->t, p->q) : g.trackDepthImageSDF(depth.data(), rows, cols));
    }, py::arg("depth"), py::arg("t") = py::none(), py::arg("q") = py::none())
    .def("trackPointCloudSDF", [](GeoWrapper& g, FloatArray pts, OptFloatArray t, OptFloatArray q) {
      if (pts.ndim() != 2 || pts.shape(1) != 3) refuse("trackPointCloudSDF", "input should be a 2D numpy array with 3 columns");
      const auto p = pose_arg("trackPointCloudSDF", t, q);
      const size_t n = (size_t) pts.shape(0);
      return track_tuple(p ? g.trackPointCloudSDF(pts.data(), n, p->t, p->q) : g.trackPointCloudSDF(pts.data(), n));
    }, py::arg("points"), py::arg("t") = py::none(), py::arg("q") = py::none())
    .def("clearBuffers", &GeoWrapper::clearBuffers)
    .def("serializeData", &GeoWrapper::serializeData, py::arg("filename_hash") = "./data/hash_points.ply",
         py::arg("filename_voxel") = "./data/voxel_points.ply")
    .def("serializeGrid", &GeoWrapper::serializeGrid, py::arg("filename") = "./data/grid.bin")
    .def("deserializeGrid", &GeoWrapper::deserializeGrid, py::arg("filename") = "./data/grid.bin");
}
