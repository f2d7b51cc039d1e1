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

template <typename T>
py::array_t<T> to_array(const std::vector<T>& v, size_t cols) {
  const size_t rows = cols ? v.size() / cols : 0;
  py::array_t<T> a({rows, cols});
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

// (t [3], q [4] = qx,qy,qz,qw, info dict) of a tracking call
py::tuple track_tuple(const GeoWrapper::TrackResult& r) {
  py::array_t<float> ot(3), oq(4);
  std::memcpy(ot.mutable_data(), r.t.data(), 3 * sizeof(float));
  std::memcpy(oq.mutable_data(), r.q.data(), 4 * sizeof(float));
  py::array_t<int64_t> sums(32);
  std::memcpy(sums.mutable_data(), r.info.sums, sizeof r.info.sums);
  py::dict info;
  info["status"] = r.info.status;
  info["iterations_done"] = r.info.iterations_done;
  info["pixels"] = r.info.pixels;
  info["rms"] = r.info.rms;
  info["sums"] = sums;
  return py::make_tuple(ot, oq, info);
}

}  // namespace

PYBIND11_MODULE(pygeowrapper, m) {
  m.doc() = "MI355X-native drop-in for mrhash.src.pygeowrapper (HIP kernels behind include/mrhash_hip.h)";
  py::class_<GeoWrapper>(m, "GeoWrapper")
    .def(py::init<float, float, int, float, int, int, bool, float, uint8_t, float, float, std::string, float, float, bool>(),
         py::arg("sdf_truncation"), py::arg("sdf_truncation_scale"), py::arg("integration_weight_sample"), py::arg("virtual_voxel_size"),
         py::arg("n_frames_invalidate_voxels"), py::arg("voxel_extents_scale"), py::arg("viewer_active"), py::arg("marching_cubes_threshold"),
         py::arg("min_weight_threshold"), py::arg("min_depth"), py::arg("max_depth"), py::arg("gs_optimization_param_path") = "",
         py::arg("sdf_var_threshold") = 0.f, py::arg("vertices_merging_threshold") = 0.f, py::arg("projective_sdf") = true)
    // getters
    .def("getHashNumBuckets", &GeoWrapper::getHashNumBuckets)
    .def("getNumSdfBlocks", &GeoWrapper::getNumSdfBlocks)
    .def("getHashBucketSize", &GeoWrapper::getHashBucketSize)
    .def("getSdfTruncation", &GeoWrapper::getSdfTruncation)
    .def("getSdfTruncationScale", &GeoWrapper::getSdfTruncationScale)
    .def("getIntegrationWeightSample", &GeoWrapper::getIntegrationWeightSample)
    .def("getIntegrationWeightMax", &GeoWrapper::getIntegrationWeightMax)
    .def("getVirtualVoxelSize", &GeoWrapper::getVirtualVoxelSize)
    .def("getLinkedListSize", &GeoWrapper::getLinkedListSize)
    .def("getNFramesInvalidateVoxels", &GeoWrapper::getNFramesInvalidateVoxels)
    .def("getMaxNumSdfBlockIntegrateFromGlobalHash", &GeoWrapper::getMaxNumSdfBlockIntegrateFromGlobalHash)
    .def("getVoxelExtentsScale", &GeoWrapper::getVoxelExtentsScale)
    .def("getCurrPose", [](const GeoWrapper& g) {
      py::array_t<float> a({4, 4});
      std::memcpy(a.mutable_data(), g.getCurrPose().data(), 16 * sizeof(float));
      return a;
    })
    .def("getPointCloud", [](const GeoWrapper& g) { return to_array<float>(g.pointCloud(), 3); })
    .def("getNormals", [](const GeoWrapper& g) { return to_array<float>(g.normals(), 3); })
    .def("getVertices", [](const GeoWrapper& g) { return to_array<double>(g.vertices(), 3); })
    .def("getFaces", [](const GeoWrapper& g) { return to_array<int32_t>(g.faces(), 3); })
    .def("getColors", [](const GeoWrapper& g) { return to_array<double>(g.colors(), 3); })
    // setters
    .def("setHashNumBuckets", &GeoWrapper::setHashNumBuckets)
    .def("setNumSdfBlocks", &GeoWrapper::setNumSdfBlocks)
    .def("setHashBucketSize", &GeoWrapper::setHashBucketSize)
    .def("setSdfTruncation", &GeoWrapper::setSdfTruncation)
    .def("setSdfTruncationScale", &GeoWrapper::setSdfTruncationScale)
    .def("setIntegrationWeightSample", &GeoWrapper::setIntegrationWeightSample)
    .def("setIntegrationWeightMax", &GeoWrapper::setIntegrationWeightMax)
    .def("setVirtualVoxelSize", &GeoWrapper::setVirtualVoxelSize)
    .def("setLinkedListSize", &GeoWrapper::setLinkedListSize)
    .def("setNFramesInvalidateVoxels", &GeoWrapper::setNFramesInvalidateVoxels)
    .def("setMaxNumSdfBlockIntegrateFromGlobalHash", &GeoWrapper::setMaxNumSdfBlockIntegrateFromGlobalHash)
    .def("setVoxelExtentsScale", &GeoWrapper::setVoxelExtentsScale)
    .def("setRGBImage", [](GeoWrapper& g, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
      // geowrapper.cpp:246-274 (the reference runner passes float32 RGB and relies on the implicit cast)
      if (a.ndim() != 3) throw std::runtime_error("GeoWrapper::setRGBImage|input should be a 3D numpy array");
      if (a.shape(2) != 3) throw std::runtime_error("GeoWrapper::setRGBImage|input should have 3 channels");
      g.setRGBImage(a.data(), (size_t) a.shape(0), (size_t) a.shape(1));
    })
    .def("setDepthImage", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> a) {
      // geowrapper.cpp:300-321
      if (a.ndim() != 2) throw std::runtime_error("GeoWrapper::setDepthImage|input should be a 2D numpy array");
      g.setDepthImage(a.data(), (size_t) a.shape(0), (size_t) a.shape(1));
    })
    .def("setPointCloud", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> pts, bool compute_normals) {
      // geowrapper.cpp:345-405: [N, 3] points in the sensor frame (the runners pass points[:, :3]); copied
      if (pts.ndim() != 2) throw std::runtime_error("GeoWrapper::setPointCloud|input should be a 2D numpy array");
      if (pts.shape(1) < 3) throw std::runtime_error("GeoWrapper::setPointCloud|input should have at least 3 columns (x, y, z)");
      if (pts.shape(1) == 3) {
        g.setPointCloud(pts.data(), (size_t) pts.shape(0), nullptr, compute_normals);
      } else {
        std::vector<float> xyz((size_t) pts.shape(0) * 3);
        auto r = pts.unchecked<2>();
        for (py::ssize_t i = 0; i < pts.shape(0); i++) { xyz[3 * i] = r(i, 0); xyz[3 * i + 1] = r(i, 1); xyz[3 * i + 2] = r(i, 2); }
        g.setPointCloud(xyz.data(), (size_t) pts.shape(0), nullptr, compute_normals);
      }
    }, py::arg("input_point_cloud"), py::arg("compute_normals") = false)
    .def("setPointCloud", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> pts,
                             py::array_t<float, py::array::c_style | py::array::forcecast> normals) {
      // geowrapper.cpp:460-490
      if (pts.ndim() != 2) throw std::runtime_error("GeoWrapper::setPointCloud|point cloud input should be a 2D numpy array");
      if (normals.ndim() != 2) throw std::runtime_error("GeoWrapper::setPointCloud|normals input should be a 2D numpy array");
      if (pts.shape(0) != normals.shape(0))
        throw std::runtime_error("GeoWrapper::setPointCloud|point_cloud input and normals input should have the same number of points");
      g.setPointCloud(pts.data(), (size_t) pts.shape(0), normals.data());
    })
    .def("setCamera", &GeoWrapper::setCamera)
    .def("setCurrPose", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> t,
                           py::array_t<float, py::array::c_style | py::array::forcecast> q) {
      if (t.size() != 3 || q.size() != 4) throw std::runtime_error("GeoWrapper::setCurrPose|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
      g.setCurrPose({t.data()[0], t.data()[1], t.data()[2]}, {q.data()[0], q.data()[1], q.data()[2], q.data()[3]});
    })
    .def("setCameraInLidar", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> m4) {
      if (m4.size() != 16) throw std::runtime_error("GeoWrapper::setCameraInLidar|expected a 4x4 matrix");
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
    .def("_stream", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> pos, float radius) {
      if (pos.size() != 3) throw std::runtime_error("GeoWrapper::_stream|expected a 3-vector");
      g.stream({pos.data()[0], pos.data()[1], pos.data()[2]}, radius);
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
      if (b.size() != MRH_COMM_ID_BYTES) throw std::runtime_error("GeoWrapper::_commInit|the id has 128 bytes");
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
      return py::make_tuple(to_array<float>(xyz, 3), to_array<float>(scale, 1), to_array<uint8_t>(rgb, 3));
    })
    // not part of the reference binding: renders the map with the camera of the last setCamera from the current pose, or from
    // (t, q) = (<tx,ty,tz>, <qx,qy,qz,qw>); returns (depth [H, W] f32, normals [H, W, 3] f32 world frame, colors [H, W, 3] u8)
    .def("raycast", [](GeoWrapper& g, std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                       std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> q) {
      if (t.has_value() != q.has_value()) throw std::runtime_error("GeoWrapper::raycast|give both t and q, or neither");
      GeoWrapper::RaycastImages im;
      if (t) {
        if (t->size() != 3 || q->size() != 4) throw std::runtime_error("GeoWrapper::raycast|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
        im = g.raycast({t->data()[0], t->data()[1], t->data()[2]}, {q->data()[0], q->data()[1], q->data()[2], q->data()[3]});
      } else {
        im = g.raycast();
      }
      const size_t H = (size_t) im.rows, W = (size_t) im.cols;
      py::array_t<float> depth({H, W});
      py::array_t<float> normals({H, W, (size_t) 3});
      py::array_t<uint8_t> colors({H, W, (size_t) 3});
      std::memcpy(depth.mutable_data(), im.depth.data(), im.depth.size() * sizeof(float));
      std::memcpy(normals.mutable_data(), im.normals.data(), im.normals.size() * sizeof(float));
      std::memcpy(colors.mutable_data(), im.colors.data(), im.colors.size());
      return py::make_tuple(depth, normals, colors);
    }, py::arg("t") = py::none(), py::arg("q") = py::none())
    // ... and with the spherical camera of the last setCamera: (range [H, W] f32, normals [H, W, 3] f32 world frame, colors
    // [H, W, 3] u8, points [H * W, 3] f32 sensor frame — an organised scan, (0, 0, 0) where nothing was hit)
    .def("raycastScan", [](GeoWrapper& g, std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                           std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> q) {
      if (t.has_value() != q.has_value()) throw std::runtime_error("GeoWrapper::raycastScan|give both t and q, or neither");
      GeoWrapper::RaycastScan im;
      if (t) {
        if (t->size() != 3 || q->size() != 4) throw std::runtime_error("GeoWrapper::raycastScan|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
        im = g.raycastScan({t->data()[0], t->data()[1], t->data()[2]}, {q->data()[0], q->data()[1], q->data()[2], q->data()[3]});
      } else {
        im = g.raycastScan();
      }
      const size_t H = (size_t) im.rows, W = (size_t) im.cols;
      py::array_t<float> range({H, W});
      py::array_t<float> normals({H, W, (size_t) 3});
      py::array_t<uint8_t> colors({H, W, (size_t) 3});
      py::array_t<float> points({H * W, (size_t) 3});
      std::memcpy(range.mutable_data(), im.range.data(), im.range.size() * sizeof(float));
      std::memcpy(normals.mutable_data(), im.normals.data(), im.normals.size() * sizeof(float));
      std::memcpy(colors.mutable_data(), im.colors.data(), im.colors.size());
      std::memcpy(points.mutable_data(), im.points.data(), im.points.size() * sizeof(float));
      return py::make_tuple(range, normals, colors, points);
    }, py::arg("t") = py::none(), py::arg("q") = py::none())
    // not part of the reference binding: the Euclidean signed distance field of the world box [lo, hi] (metres), exact up to
    // max_distance; returns (dist [nz, ny, nx] f32 metres, state [nz, ny, nx] u8, origin (x, y, z) in voxels, dims (nx, ny, nz))
    .def("distanceField", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> lo,
                             py::array_t<float, py::array::c_style | py::array::forcecast> hi, float max_distance) {
      if (lo.size() != 3 || hi.size() != 3) throw std::runtime_error("GeoWrapper::distanceField|expected two 3-vectors (lo, hi)");
      const GeoWrapper::DistanceField f = g.distanceField({lo.data()[0], lo.data()[1], lo.data()[2]}, {hi.data()[0], hi.data()[1], hi.data()[2]}, max_distance);
      const size_t nx = (size_t) f.dims[0], ny = (size_t) f.dims[1], nz = (size_t) f.dims[2];
      py::array_t<float> dist({nz, ny, nx});
      py::array_t<uint8_t> state({nz, ny, nx});
      std::memcpy(dist.mutable_data(), f.dist.data(), f.dist.size() * sizeof(float));
      std::memcpy(state.mutable_data(), f.state.data(), f.state.size());
      return py::make_tuple(dist, state, py::make_tuple(f.origin[0], f.origin[1], f.origin[2]), py::make_tuple(f.dims[0], f.dims[1], f.dims[2]));
    }, py::arg("lo"), py::arg("hi"), py::arg("max_distance"))
    // not part of the reference binding: TSDF distance, gradient and colour of the map at points [n, 3] — world points, or with
    // sensor_frame = True points in the sensor frame at the pose of the last setCurrPose ((0, 0, 0) = no return, refused; what
    // raycastScan returns).  smooth = False: the map's own, piecewise-constant field; True: the continuous field.  Returns
    // (dist [n] f32, grad [n, 3] f32, rgbw [n, 4] u8 = r, g, b, weight, state [n] u8 of MRH_QUERY_* bits)
    .def("queryPoints", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> points, bool smooth, bool sensor_frame) {
      if (!((points.ndim() == 2 && points.shape(1) == 3) || (points.ndim() == 1 && points.size() % 3 == 0)))
        throw std::runtime_error("GeoWrapper::queryPoints|expected points of shape [n, 3]");
      const size_t n = (size_t) points.size() / 3;
      const GeoWrapper::PointQuery r = g.queryPoints(points.data(), n, smooth, sensor_frame);
      py::array_t<float> dist({n});
      py::array_t<float> grad({n, (size_t) 3});
      py::array_t<uint8_t> rgbw({n, (size_t) 4});
      py::array_t<uint8_t> state({n});
      if (n) {
        std::memcpy(dist.mutable_data(), r.dist.data(), r.dist.size() * sizeof(float));
        std::memcpy(grad.mutable_data(), r.grad.data(), r.grad.size() * sizeof(float));
        std::memcpy(rgbw.mutable_data(), r.rgbw.data(), r.rgbw.size());
        std::memcpy(state.mutable_data(), r.state.data(), r.state.size());
      }
      return py::make_tuple(dist, grad, rgbw, state);
    }, py::arg("points"), py::arg("smooth") = false, py::arg("sensor_frame") = false)
    // not part of the reference binding: rays cast through the map — origins [n, 3], directions [n, 3], tmax [n] or
    // None; world rays, or with sensor_frame = True rays in the sensor frame at the pose of the last setCurrPose.  normalize = True
    // divides each direction on the host in float32 by sqrt((dx * dx + dy * dy) + dz * dz).  Returns (range [n] f32, status [n] u8 of
    // MRH_RAY_* bits, normals [n, 3] f32, rgb [n, 3] u8, counts [n, 2] u32 = n_free, n_unknown, first_unknown [n] f32)
    .def("castRays", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> origins,
                        py::array_t<float, py::array::c_style | py::array::forcecast> directions, float max_range, float min_range, float step, py::object tmax,
                        bool sensor_frame, bool normalize) {
      auto rays_of = [](const py::array_t<float, py::array::c_style | py::array::forcecast>& a) {
        return (a.ndim() == 2 && a.shape(1) == 3) || (a.ndim() == 1 && a.size() % 3 == 0);
      };
      if (!rays_of(origins) || !rays_of(directions) || origins.size() != directions.size())
        throw std::runtime_error("GeoWrapper::castRays|expected origins and directions of shape [n, 3]");
      const size_t n = (size_t) origins.size() / 3;
      py::array_t<float, py::array::c_style | py::array::forcecast> ends;
      if (!tmax.is_none()) {
        ends = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(tmax);
        if (!ends || (size_t) ends.size() != n) throw std::runtime_error("GeoWrapper::castRays|expected tmax of shape [n]");
      }
      const GeoWrapper::RayCast r = g.castRays(origins.data(), directions.data(), n, max_range, min_range, step, tmax.is_none() ? nullptr : ends.data(), sensor_frame, normalize);
      py::array_t<float> range({n});
      py::array_t<uint8_t> status({n});
      py::array_t<float> normals({n, (size_t) 3});
      py::array_t<uint8_t> rgb({n, (size_t) 3});
      py::array_t<uint32_t> counts({n, (size_t) 2});
      py::array_t<float> first({n});
      if (n) {
        std::memcpy(range.mutable_data(), r.range.data(), r.range.size() * sizeof(float));
        std::memcpy(status.mutable_data(), r.status.data(), r.status.size());
        std::memcpy(normals.mutable_data(), r.normals.data(), r.normals.size() * sizeof(float));
        std::memcpy(rgb.mutable_data(), r.rgb.data(), r.rgb.size());
        std::memcpy(counts.mutable_data(), r.counts.data(), r.counts.size() * sizeof(uint32_t));
        std::memcpy(first.mutable_data(), r.first_unknown.data(), r.first_unknown.size() * sizeof(float));
      }
      return py::make_tuple(range, status, normals, rgb, counts, first);
    }, py::arg("origins"), py::arg("directions"), py::arg("max_range"), py::arg("min_range") = 0.f, py::arg("step") = 0.f, py::arg("tmax") = py::none(),
       py::arg("sensor_frame") = false, py::arg("normalize") = true)
    // not part of the reference binding: the map of `other`, whose frame lies at the pose (t, q) in this map's world, resampled at
    // this map's voxel size and merged into it.  Returns the counts of mrh_remap_info as a dict.  Blocks paged out to
    // either wrapper's host chunk grid take no part
    .def("fuseMap", [](GeoWrapper& g, GeoWrapper& other, py::array_t<float, py::array::c_style | py::array::forcecast> t,
                       py::array_t<float, py::array::c_style | py::array::forcecast> q, uint32_t min_weight) {
      if (t.size() != 3 || q.size() != 4) throw std::runtime_error("GeoWrapper::fuseMap|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
      const mrh_remap_info r = g.fuseMap(other, {t.data()[0], t.data()[1], t.data()[2]}, {q.data()[0], q.data()[1], q.data()[2], q.data()[3]}, min_weight);
      py::dict d;
      d["source_blocks"] = r.source_blocks; d["candidate_blocks"] = r.candidate_blocks; d["records"] = r.records;
      d["valid_voxels"] = r.valid_voxels; d["taken"] = r.taken;
      return d;
    }, py::arg("other"), py::arg("t"), py::arg("q"), py::arg("min_weight") = 0)
    // not part of the reference binding: the pose of `other`'s frame in this map's world, estimated from the two maps alone (DESIGN.md
    // D19), started from (t, q) as fuseMap takes it.  Returns (t [3], q [4] = qx,qy,qz,qw, info dict): what fuseMap then takes
    .def("alignMap", [](GeoWrapper& g, GeoWrapper& other, py::array_t<float, py::array::c_style | py::array::forcecast> t,
                        py::array_t<float, py::array::c_style | py::array::forcecast> q, int iterations, uint32_t min_weight) {
      if (t.size() != 3 || q.size() != 4) throw std::runtime_error("GeoWrapper::alignMap|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
      const GeoWrapper::AlignResult r = g.alignMap(other, {t.data()[0], t.data()[1], t.data()[2]}, {q.data()[0], q.data()[1], q.data()[2], q.data()[3]}, iterations, min_weight);
      py::array_t<float> ot(3), oq(4), pivot(3);
      std::memcpy(ot.mutable_data(), r.t.data(), 3 * sizeof(float));
      std::memcpy(oq.mutable_data(), r.q.data(), 4 * sizeof(float));
      std::memcpy(pivot.mutable_data(), r.info.pivot, sizeof r.info.pivot);
      py::array_t<int64_t> sums(32);
      std::memcpy(sums.mutable_data(), r.info.sums, sizeof r.info.sums);
      py::dict info;
      info["status"] = r.info.status; info["iterations_done"] = r.info.iterations_done; info["source_blocks"] = r.info.source_blocks;
      info["samples"] = r.info.samples; info["accepted"] = r.info.accepted; info["rms"] = r.info.rms;
      info["pivot"] = pivot; info["extent"] = r.info.extent; info["sums"] = sums;
      return py::make_tuple(ot, oq, info);
    }, py::arg("other"), py::arg("t"), py::arg("q"), py::arg("iterations") = 0, py::arg("min_weight") = 0)
    // not part of the reference binding: the pose of a depth image (2-D, the camera's rows x cols, metres) by ICP against the map,
    // started from the current pose or from (t, q); returns (t [3], q [4] = qx,qy,qz,qw, info dict) and leaves the current pose
    // alone — call setCurrPose(t, q) with the result before setDepthImage / compute
    .def("trackDepthImage", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> depth,
                               std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                               std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> q) {
      if (depth.ndim() != 2) throw std::runtime_error("GeoWrapper::trackDepthImage|input should be a 2D numpy array");
      if (t.has_value() != q.has_value()) throw std::runtime_error("GeoWrapper::trackDepthImage|give both t and q, or neither");
      GeoWrapper::TrackResult r;
      if (t) {
        if (t->size() != 3 || q->size() != 4) throw std::runtime_error("GeoWrapper::trackDepthImage|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
        r = g.trackDepthImage(depth.data(), (size_t) depth.shape(0), (size_t) depth.shape(1), {t->data()[0], t->data()[1], t->data()[2]},
                              {q->data()[0], q->data()[1], q->data()[2], q->data()[3]});
      } else {
        r = g.trackDepthImage(depth.data(), (size_t) depth.shape(0), (size_t) depth.shape(1));
      }
      return track_tuple(r);
    }, py::arg("depth"), py::arg("t") = py::none(), py::arg("q") = py::none())
    // the same for a LiDAR scan ([N, 3] float32, sensor frame) under the spherical camera of setCamera(..., model = 1); the loop is
    // trackPointCloud -> setCurrPose -> setPointCloud -> compute
    .def("trackPointCloud", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> pts,
                               std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                               std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> q) {
      if (pts.ndim() != 2 || pts.shape(1) != 3) throw std::runtime_error("GeoWrapper::trackPointCloud|input should be a 2D numpy array with 3 columns");
      if (t.has_value() != q.has_value()) throw std::runtime_error("GeoWrapper::trackPointCloud|give both t and q, or neither");
      if (!t) return track_tuple(g.trackPointCloud(pts.data(), (size_t) pts.shape(0)));
      if (t->size() != 3 || q->size() != 4) throw std::runtime_error("GeoWrapper::trackPointCloud|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
      return track_tuple(g.trackPointCloud(pts.data(), (size_t) pts.shape(0), {t->data()[0], t->data()[1], t->data()[2]},
                                           {q->data()[0], q->data()[1], q->data()[2], q->data()[3]}));
    }, py::arg("points"), py::arg("t") = py::none(), py::arg("q") = py::none())
    // not part of the reference binding: the two tracking calls without the render — the image's pixels, or the cloud's
    // points, against the map's own distance field; same arguments and result.  trackPointCloudSDF accepts either camera model
    .def("trackDepthImageSDF", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> depth,
                                  std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                                  std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> q) {
      if (depth.ndim() != 2) throw std::runtime_error("GeoWrapper::trackDepthImageSDF|input should be a 2D numpy array");
      if (t.has_value() != q.has_value()) throw std::runtime_error("GeoWrapper::trackDepthImageSDF|give both t and q, or neither");
      if (!t) return track_tuple(g.trackDepthImageSDF(depth.data(), (size_t) depth.shape(0), (size_t) depth.shape(1)));
      if (t->size() != 3 || q->size() != 4) throw std::runtime_error("GeoWrapper::trackDepthImageSDF|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
      return track_tuple(g.trackDepthImageSDF(depth.data(), (size_t) depth.shape(0), (size_t) depth.shape(1), {t->data()[0], t->data()[1], t->data()[2]},
                                              {q->data()[0], q->data()[1], q->data()[2], q->data()[3]}));
    }, py::arg("depth"), py::arg("t") = py::none(), py::arg("q") = py::none())
    .def("trackPointCloudSDF", [](GeoWrapper& g, py::array_t<float, py::array::c_style | py::array::forcecast> pts,
                                  std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                                  std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> q) {
      if (pts.ndim() != 2 || pts.shape(1) != 3) throw std::runtime_error("GeoWrapper::trackPointCloudSDF|input should be a 2D numpy array with 3 columns");
      if (t.has_value() != q.has_value()) throw std::runtime_error("GeoWrapper::trackPointCloudSDF|give both t and q, or neither");
      if (!t) return track_tuple(g.trackPointCloudSDF(pts.data(), (size_t) pts.shape(0)));
      if (t->size() != 3 || q->size() != 4) throw std::runtime_error("GeoWrapper::trackPointCloudSDF|expected a 3-vector and a 4-vector (qx,qy,qz,qw)");
      return track_tuple(g.trackPointCloudSDF(pts.data(), (size_t) pts.shape(0), {t->data()[0], t->data()[1], t->data()[2]},
                                              {q->data()[0], q->data()[1], q->data()[2], q->data()[3]}));
    }, py::arg("points"), py::arg("t") = py::none(), py::arg("q") = py::none())
    .def("clearBuffers", &GeoWrapper::clearBuffers)
    .def("serializeData", &GeoWrapper::serializeData, py::arg("filename_hash") = "./data/hash_points.ply",
         py::arg("filename_voxel") = "./data/voxel_points.ply")
    .def("serializeGrid", &GeoWrapper::serializeGrid, py::arg("filename") = "./data/grid.bin")
    .def("deserializeGrid", &GeoWrapper::deserializeGrid, py::arg("filename") = "./data/grid.bin");
}
