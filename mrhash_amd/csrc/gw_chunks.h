// gw_chunks.h — host side of the streamer (streamer.cuh:40-80, :251-352, streamer.cpp:214-247, :292-331): the chunk grid of
// streamed-out blocks, its chunk arithmetic, and the geometry by which extractMesh chooses between one extraction and the
// reference's walk over the grid.  Pure host code over the block types of include/mrhash_hip.h: no context, no C-ABI call;
// checked by tests/host/gw_check.cpp.  `ext` is the chunk edge in metres, (float) voxel_extents_scale (geowrapper.cpp:56).
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "mrhash_hip.h"

namespace gw {

using Chunk = std::array<int, 3>;
using Vec3 = std::array<float, 3>;

// Streamer::worldToChunks: p / ext rounded half away from zero
inline Chunk worldToChunks(const Vec3& pw, float ext) {
  Chunk c;
  for (int a = 0; a < 3; a++) {
    const float p = pw[a] / ext;
    const float s = (float) ((0.f < p) - (p < 0.f));
    c[a] = (int) (p + s * 0.5f);
  }
  return c;
}

// the chunk of a block, from its origin in metres
inline Chunk chunkOfBlock(const mrh_block_desc& d, float voxel_size, float ext) {
  const float bs = 8.f * voxel_size;
  return worldToChunks({(float) d.x * bs, (float) d.y * bs, (float) d.z * bs}, ext);
}

inline float chunkRadius(float ext) { return std::sqrt(3.f * ext * ext) / 2.0f; }  // voxel_extents_.norm() / 2 (streamer.cuh:315-317)

inline float chunkDistance(const Chunk& chunk, const Vec3& center, float ext) {
  const float dx = chunk[0] * ext - center[0], dy = chunk[1] * ext - center[1], dz = chunk[2] * ext - center[2];
  return std::sqrt(dx * dx + dy * dy + dz * dz);
}

// any part of the chunk within `radius` of `center`?  (The reference's isChunkInSphere, streamer.cuh:345-352, asks for
// the WHOLE chunk to be inside, which leaves blocks the next frame can touch on the host; see GeoWrapper::stream.)
inline bool chunkTouchesSphere(const Chunk& chunk, const Vec3& center, float radius, float ext) {
  return chunkDistance(chunk, center, ext) <= radius + chunkRadius(ext);
}

// Streamer::isChunkInSphere (streamer.cuh:345-352), literally: the chunk CENTRE within |radius - chunk radius| of the sphere
// centre.  Used by the chunk loop of extractMesh only (stream() pages with its own, transparent radii).
inline bool chunkInSphereRef(const Chunk& chunk, const Vec3& center, float radius, float ext) {
  return chunkDistance(chunk, center, ext) <= std::fabs(radius - chunkRadius(ext));
}

struct HostBlock {
  mrh_block_desc desc;
  std::vector<mrh_voxel> voxels;  // 512, reference layout
};

class ChunkGrid {
public:
  // what gather() hands to mrh_import_blocks, and the chunks it came from
  struct Gathered { std::vector<mrh_block_desc> descs; std::vector<mrh_voxel> voxels; std::vector<Chunk> taken; };

  // Streamer::integrateInChunkGrid: n blocks (descs [n], voxels [n * 512]) into the chunks of their origins
  void add(const mrh_block_desc* descs, const mrh_voxel* voxels, uint64_t n, float voxel_size, float ext) {
    for (uint64_t k = 0; k < n; k++)
      chunks_[chunkOfBlock(descs[k], voxel_size, ext)].push_back({descs[k], std::vector<mrh_voxel>(voxels + k * 512, voxels + (k + 1) * 512)});
  }
  // copies of every block of the chunks that `take(chunk)` accepts, in map order; the grid itself is left alone
  template <typename Take>
  Gathered gather(Take take) const {
    Gathered g;
    for (const auto& kv : chunks_) {
      if (!take(kv.first)) continue;
      for (const HostBlock& b : kv.second) {
        g.descs.push_back(b.desc);
        g.voxels.insert(g.voxels.end(), b.voxels.begin(), b.voxels.end());
      }
      g.taken.push_back(kv.first);
    }
    return g;
  }
  void erase(const std::vector<Chunk>& taken) { for (const Chunk& k : taken) chunks_.erase(k); }
  size_t blocks() const {
    size_t n = 0;
    for (const auto& kv : chunks_) n += kv.second.size();
    return n;
  }
  bool empty() const { return chunks_.empty(); }
  void clear() { chunks_.clear(); }
  const std::map<Chunk, std::vector<HostBlock>>& chunks() const { return chunks_; }

private:
  std::map<Chunk, std::vector<HostBlock>> chunks_;
};

// The geometry of GeoWrapper::extractMesh (geowrapper.cpp:150-190).  The reference pages EVERYTHING out, then walks the chunk grid
// in steps of int(10 * max depth) chunks: stream in the sphere of radius 10 * max depth around the step's chunk, marching cubes,
// merge into the running mesh, page everything out again.  Whenever that loop has a single iteration whose sphere holds the
// whole map (in_first_sphere), its triangles are those of ONE extraction over the resident map; whether the map also fits the
// pool is the caller's to ask.
struct MeshPlan {
  bool empty = true;    // no block on the device and none on the host grid
  Chunk lo{}, hi{};     // Streamer::computeBounds over what WOULD be on the host after streamAllOut; lo == hi -> hi + 1
  float radius = 0.f;   // params.h:35 radius_scale_chunk
  int radiusi = 1;      // (int) radius == 0 would never advance the reference's loops
  Vec3 first_center{};  // Streamer::chunkToWorld(lo)
  bool in_first_sphere = false;
  float ext = 1.f;

  template <typename Visit>
  void forEachCenter(Visit visit) const {  // the centres of the reference's loops, in its order (Streamer::chunkToWorld)
    for (int x = lo[0]; x < hi[0]; x += radiusi)
      for (int y = lo[1]; y < hi[1]; y += radiusi)
        for (int z = lo[2]; z < hi[2]; z += radiusi) visit(Vec3{(float) x * ext, (float) y * ext, (float) z * ext});
  }
};

inline MeshPlan planExtract(const std::vector<Chunk>& device_chunks, const ChunkGrid& grid, int voxel_extents_scale, float max_depth) {
  MeshPlan p;
  p.ext = (float) voxel_extents_scale;
  p.radius = 10.0f * max_depth;
  p.radiusi = std::max(1, (int) p.radius);
  p.empty = device_chunks.empty() && grid.empty();
  if (p.empty) return p;
  p.lo = {INT32_MAX, INT32_MAX, INT32_MAX};
  p.hi = {INT32_MIN, INT32_MIN, INT32_MIN};
  auto widen = [&](const Chunk& c) { for (int a = 0; a < 3; a++) { p.lo[a] = std::min(p.lo[a], c[a]); p.hi[a] = std::max(p.hi[a], c[a]); } };
  for (const Chunk& c : device_chunks) widen(c);
  for (const auto& kv : grid.chunks()) widen(kv.first);
  for (int a = 0; a < 3; a++) if (p.lo[a] == p.hi[a]) p.hi[a] += 1;  // geowrapper.cpp:165-173
  p.first_center = {(float) p.lo[0] * p.ext, (float) p.lo[1] * p.ext, (float) p.lo[2] * p.ext};
  auto inside = [&](const Chunk& c) { return chunkInSphereRef(c, p.first_center, p.radius, p.ext); };
  p.in_first_sphere = std::all_of(device_chunks.begin(), device_chunks.end(), inside) &&
                      std::all_of(grid.chunks().begin(), grid.chunks().end(), [&](const auto& kv) { return inside(kv.first); });
  for (int a = 0; a < 3; a++) p.in_first_sphere = p.in_first_sphere && (p.lo[a] + p.radiusi >= p.hi[a]);
  return p;
}

}  // namespace gw
