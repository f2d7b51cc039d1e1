// gw_files.h — the files the GeoWrapper facade writes and reads, on streams and buffers: the mesh PLY of extractMesh, the two
// point clouds of serializeData, the MRHGRID1 file of serializeGrid / deserializeGrid and the seeds PLY of GSSavePointCloud.
// Pure host code over the types of include/mrhash_hip.h: no context, no C-ABI call; checked by tests/host/gw_check.cpp.
#pragma once

#include <charconv>
#include <cstdint>
#include <cstring>
#include <istream>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "mrhash_hip.h"

namespace gw {

// ---- the mesh: ASCII PLY, same header and value formatting as geowrapper.cpp:194-227.  The reference streams every number
// through an ofstream (`<<` on a double is printf's %g with precision 6); std::to_chars(general, 6) is defined to produce the
// same characters, so the rows are formatted in parallel pieces and written in order: byte-identical file, a fraction of the
// 0.9 s the iostream loop takes for a million triangles.
inline std::string meshPlyHeader(uint64_t nv, uint64_t nf) {
  return "ply\nformat ascii 1.0\nelement vertex " + std::to_string(nv) + "\nproperty float x\nproperty float y\nproperty float z\n" +
         "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face " + std::to_string(nf) +
         "\nproperty list uchar int vertex_indices\nend_header\n";
}

constexpr size_t kVertexRowMax = 64;  // 3 x <= 13 chars + 3 x <= 3 chars + separators
constexpr size_t kFaceRowMax = 40;    // "3" + 3 x (space + <= 11 chars) + newline

inline char* putDouble(char* p, double v) { return std::to_chars(p, p + 32, v, std::chars_format::general, 6).ptr; }
inline char* putInt(char* p, int v) { return std::to_chars(p, p + 16, v).ptr; }

// rows [lo, hi) of V [nv * 3] with the colours C [nv * 3] into p (room for kVertexRowMax per row); returns the end
inline char* formatVertices(const double* V, const double* C, uint64_t lo, uint64_t hi, char* p) {
  for (uint64_t i = lo; i < hi; ++i) {
    for (int a = 0; a < 3; a++) { p = putDouble(p, V[i * 3 + a]); *p++ = ' '; }
    for (int a = 0; a < 3; a++) { p = putInt(p, (int) (unsigned char) (C[i * 3 + a])); *p++ = a == 2 ? '\n' : ' '; }
  }
  return p;
}

// rows [lo, hi) of F [nf * 3] into p (room for kFaceRowMax per row); returns the end
inline char* formatFaces(const int32_t* F, uint64_t lo, uint64_t hi, char* p) {
  for (uint64_t i = lo; i < hi; ++i) {
    *p++ = '3';
    for (int a = 0; a < 3; a++) { *p++ = ' '; p = putInt(p, F[i * 3 + a]); }
    *p++ = '\n';
  }
  return p;
}

struct PlyPiece { std::unique_ptr<char[]> buf; size_t len = 0; };

// the body of the file in 2 * n_workers pieces, to be written in this order: the vertex rows split n_workers ways, then the face
// rows; one thread per worker (none for one worker)
inline std::vector<PlyPiece> formatMesh(const double* V, const double* C, const int32_t* F, uint64_t nv, uint64_t nf, unsigned n_workers) {
  std::vector<PlyPiece> pieces(2 * (size_t) n_workers);
  auto format_piece = [&](unsigned k) {
    const uint64_t vlo = nv * k / n_workers, vhi = nv * (k + 1) / n_workers, flo = nf * k / n_workers, fhi = nf * (k + 1) / n_workers;
    PlyPiece &v = pieces[k], &f = pieces[n_workers + k];
    v.buf.reset(new char[(vhi - vlo) * kVertexRowMax + 1]);
    v.len = (size_t) (formatVertices(V, C, vlo, vhi, v.buf.get()) - v.buf.get());
    f.buf.reset(new char[(fhi - flo) * kFaceRowMax + 1]);
    f.len = (size_t) (formatFaces(F, flo, fhi, f.buf.get()) - f.buf.get());
  };
  std::vector<std::thread> workers;
  for (unsigned k = 1; k < n_workers; k++) workers.emplace_back(format_piece, k);
  format_piece(0);
  for (std::thread& w : workers) w.join();
  return pieces;
}

inline void writePieces(std::ostream& o, const std::vector<PlyPiece>& pieces) {
  for (const PlyPiece& c : pieces) o.write(c.buf.get(), (std::streamsize) c.len);
}

// ---- serializeData: PLY point clouds of block origins and weighted voxels (streamer.cpp:104-160): x y z r g b weight [sdf]
struct DataPoint { float x, y, z, r, g, b, w, s; };

// appends one hash point per block with a weighted voxel (its mean weight) and one voxel point per weighted voxel
inline void dataPoints(const mrh_block_desc* descs, const mrh_voxel* vox, uint64_t n, float voxel_size, std::vector<DataPoint>& hash_pts,
                       std::vector<DataPoint>& voxel_pts) {
  for (uint64_t k = 0; k < n; ++k) {
    const mrh_block_desc& d = descs[k];
    const float bx = (float) (d.x * 8) * voxel_size, by = (float) (d.y * 8) * voxel_size, bz = (float) (d.z * 8) * voxel_size;
    const int side = 8 >> d.resolution, sf = 1 << d.resolution;
    float wsum = 0.f;
    unsigned valid = 0;
    for (int l = 0; l < side * side * side; ++l) {
      const mrh_voxel& v = vox[k * 512 + l];
      if (v.weight == 0) continue;
      const int lx = (l % side) * sf, ly = ((l % (side * side)) / side) * sf, lz = (l / (side * side)) * sf;
      voxel_pts.push_back({bx + lx * voxel_size, by + ly * voxel_size, bz + lz * voxel_size,
                           d.resolution == 0 ? 1.f : 0.f, d.resolution == 1 ? 1.f : 0.f, 0.f, (float) v.weight, v.sdf});
      wsum += (float) v.weight;
      valid++;
    }
    if (valid) hash_pts.push_back({bx, by, bz, d.resolution == 0 ? 1.f : 0.f, d.resolution == 1 ? 1.f : 0.f, 0.f, wsum / (float) valid, 0.f});
  }
}

inline void writeDataPoints(std::ostream& o, const std::vector<DataPoint>& pts, bool with_sdf) {
  o << "ply\nformat ascii 1.0\nelement vertex " << pts.size() << "\nproperty float x\nproperty float y\nproperty float z\n"
    << "property float red\nproperty float green\nproperty float blue\nproperty float weight\n" << (with_sdf ? "property float sdf\n" : "") << "end_header\n";
  for (const DataPoint& p : pts) {
    o << p.x << " " << p.y << " " << p.z << " " << p.r << " " << p.g << " " << p.b << " " << p.w;
    if (with_sdf) o << " " << p.s;
    o << "\n";
  }
}

// ---- serializeGrid: a flat documented format instead of cista (serializer.h:16-77): "MRHGRID1" u64 n, then n x {mrh_block_desc,
// 512 x mrh_voxel}
inline void writeGridHeader(std::ostream& o, uint64_t total) { o.write("MRHGRID1", 8); o.write((const char*) &total, 8); }
inline void writeGridBlock(std::ostream& o, const mrh_block_desc& desc, const mrh_voxel* voxels) {
  o.write((const char*) &desc, sizeof(mrh_block_desc));
  o.write((const char*) voxels, 512 * sizeof(mrh_voxel));
}

// the blocks of a MRHGRID1 stream: descs [n] and vox [n * 512], both at least one block long; returns n.  `filename` is for the texts
inline uint64_t readGrid(std::istream& in, const std::string& filename, std::vector<mrh_block_desc>& descs, std::vector<mrh_voxel>& vox) {
  char magic[8];
  uint64_t n = 0;
  in.read(magic, 8);
  in.read((char*) &n, 8);
  if (!in || std::memcmp(magic, "MRHGRID1", 8) != 0) throw std::runtime_error("GeoWrapper::deserializeGrid | not a MRHGRID1 file: " + filename);
  descs.resize(n ? n : 1);
  vox.resize((n ? n : 1) * 512);
  for (uint64_t k = 0; k < n; ++k) {
    in.read((char*) &descs[k], sizeof(mrh_block_desc));
    in.read((char*) &vox[k * 512], 512 * sizeof(mrh_voxel));
  }
  if (!in) throw std::runtime_error("GeoWrapper::deserializeGrid | truncated file: " + filename);
  return n;
}

// ---- GSSavePointCloud: the reference writes the optimised model (GaussianModel::Save_ply, src/gs/gaussian.cu:260-282); here the
// same file holds the seeds the model is initialised from
inline void writeSeeds(std::ostream& ply, const std::vector<mrh_splat_seed>& seeds) {
  ply << "ply\nformat ascii 1.0\nelement vertex " << seeds.size()
      << "\nproperty float x\nproperty float y\nproperty float z\nproperty float scale\n"
         "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
  for (const mrh_splat_seed& s : seeds)
    ply << s.p[0] << " " << s.p[1] << " " << s.p[2] << " " << s.scale << " " << (int) s.rgb[0] << " " << (int) s.rgb[1] << " " << (int) s.rgb[2] << "\n";
}

}  // namespace gw
