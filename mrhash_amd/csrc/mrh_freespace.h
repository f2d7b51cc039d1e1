// mrh_freespace.h — the free-space layer (include/mrhash_freespace.h): a dense bit grid over a box of
// cells, carved by the rays of depth frames and scans (k_freespace_carve), read as the state of a box of cells with its frontier
// (k_freespace_classify, k_freespace_frontier) and along segments (k_freespace_segments).
//
// The reference has no such structure; the definition is this project's D22.  What the kernels share with the other readers is
// used as it is: the ray of a pixel, z_k and P(z) are the render's (mrh_raycast.h: ray_dir_sensor, ray_z, ray_point), the
// per-ray sample count of a segment is the ray queries' (mrh_rays.h: ray_count_samples), world -> voxel is world_to_voxel
// (mrh_device.h), and a voxel's observed / site bits are the distance field's (mrh_esdf.h: esdf_brick, esdf_brick_voxel).
//
// WORDS.  One u32 is a 4 x 4 x 2 brick of cells, bit = (x & 3) | (y & 3) << 2 | (z & 1) << 4, bricks x fastest (FreeLayer,
// mrh_readerplan.h).  A ray with any direction stays in one word for about three cells — six samples at the default half-cell
// spacing — where a word of 32 cells along x would hold 64 samples of a ray along x and one or two of a ray along y or z; and
// the 64 rays of a wave's 8 x 8 pixel tile, a pencil a few cells wide, meet the same few words at the same depth.
//
// k_freespace_carve: one lane per ray.  The lane ORs the bits of consecutive samples that fall into one word into a mask in a
// register; when the word changes (and after the last sample) it loads the word with a plain load and issues one atomicOr — the
// vector global atomic without return — only when the mask holds a bit the word lacks.  Bits are never cleared while carves run,
// so a stale load can only cost an atomic that was not needed, never lose a bit.  No LDS, no barrier.
#pragma once

#include "mrh_esdf.h"
#include "mrh_rays.h"
#include "mrh_readerplan.h"  // FreeLayer, CarveArgs, FreeBox, SegArgs

namespace mrh {

constexpr int kFreeLanes = 256;
constexpr u32 kFreeNoWord = 0xFFFFFFFFu;
enum FreeCell : int { FREE_CELL_BAD = 0, FREE_CELL_OUTSIDE = 1, FREE_CELL_INSIDE = 2 };
enum FreeState : u32 { FREE_FREE = 1u, FREE_OBSERVED = 2u, FREE_OCCUPIED = 4u, FREE_FRONTIER = 8u };

// the word and the bit of the layer cell (x, y, z), layer coordinates; FREE_CELL_OUTSIDE when the cell is not in the box
__device__ __forceinline__ FreeCell free_word_of(const FreeLayer& L, const int x, const int y, const int z, u32& word, u32& bit) {
  if ((u32) x >= (u32) L.nx || (u32) y >= (u32) L.ny || (u32) z >= (u32) L.nz) return FREE_CELL_OUTSIDE;
  word = ((u32) (z >> 1) * (u32) L.nby + (u32) (y >> 2)) * (u32) L.nbx + (u32) (x >> 2);  // < L.n_words
  bit = 1u << ((x & 3) | ((y & 3) << 2) | ((z & 1) << 4));
  return FREE_CELL_INSIDE;
}

// The sample P of a carve or a segment: FREE_CELL_BAD unless |P_a| < bound on every axis (a NaN fails; nothing has been converted
// to an integer yet), else the cell world_to_voxel(vs, P) >> s and its word
__device__ __forceinline__ FreeCell free_sample(const FreeLayer& L, const float vs, const float bound, const f3 P, u32& word, u32& bit) {
  if (!(fabsf(P.x) < bound && fabsf(P.y) < bound && fabsf(P.z) < bound)) return FREE_CELL_BAD;
  const i3 v = world_to_voxel(vs, P);  // |v| <= 2^20 + 1, |origin| <= 2^23: no overflow
  return free_word_of(L, (v.x >> L.shift) - L.ox, (v.y >> L.shift) - L.oy, (v.z >> L.shift) - L.oz, word, bit);
}

// the merged mask of one word: a plain load first, the atomic only for a bit the word lacks
__device__ __forceinline__ void free_flush(u32* words, const u32 word, const u32 mask) {
  if (word == kFreeNoWord) return;
  if ((words[word] & mask) != mask) atomicOr(words + word, mask);
}

// PIXELS: obs is a depth image of a.cam.rows x a.cam.cols, walked in the render's 8 x 8 tiles per wave (grid: 16 x 16 tiles);
// else obs holds a.n sensor-frame points, 64 consecutive points per wave
template <bool PIXELS>
__global__ __launch_bounds__(kFreeLanes) void k_freespace_carve(const float vs, const FreeLayer L, u32* words, const CarveArgs a, const float* __restrict__ obs) {
  const RayCam& rc = a.cam;
  float end;
  f3 ds;
  if (PIXELS) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * kRenderTile + (wave & 1) * 8 + (lane & 7);
    const int r = blockIdx.y * kRenderTile + (wave >> 1) * 8 + (lane >> 3);
    if (r >= rc.rows || c >= rc.cols) return;
    const float D = obs[(size_t) r * (size_t) rc.cols + (size_t) c];
    if (!(D > rc.min_depth)) return;  // NaN, or D <= min_depth
    end = D > rc.max_depth ? rc.max_depth : D - a.margin;
    ds = ray_dir_sensor<false>(rc, r, c);
  } else {
    const size_t i = (size_t) blockIdx.x * kFreeLanes + threadIdx.x;
    if (i >= (size_t) a.n) return;
    const float x = obs[3 * i + 0], y = obs[3 * i + 1], z = obs[3 * i + 2];
    const float rho = sqrtf((x * x + y * y) + z * z);
    if (!(fabsf(rho) < INFINITY) || rho <= rc.min_depth) return;  // NaN, +inf, the missing return
    end = fminf(rho, rc.max_depth) - a.margin;
    ds = mk3(x / rho, y / rho, z / rho);
  }
  // d_w = R d with every row summed left to right, as the render
  const f3 d = mk3(rc.R[0] * ds.x + rc.R[1] * ds.y + rc.R[2] * ds.z, rc.R[3] * ds.x + rc.R[4] * ds.y + rc.R[5] * ds.z,
                   rc.R[6] * ds.x + rc.R[7] * ds.y + rc.R[8] * ds.z);
  const RayLine rl = ray_line(rc);
  u32 cur = kFreeNoWord, mask = 0;
  for (u32 k = 0; k < rc.n_samples; ++k) {
    const float z = ray_z(rl, k);
    if (!(z <= end)) break;  // z_k is monotone in k: no later sample is in
    u32 word, bit;
    if (free_sample(L, vs, a.bound, ray_point(rl, d, z), word, bit) != FREE_CELL_INSIDE) continue;
    if (word != cur) {
      free_flush(words, cur, mask);
      cur = word;
      mask = 0;
    }
    mask |= bit;
  }
  free_flush(words, cur, mask);
}

// One lane per segment.  Reads the layer alone; plain stores of the outputs (counts may be nullptr)
__global__ __launch_bounds__(kFreeLanes) void k_freespace_segments(const float vs, const FreeLayer L, const u32* __restrict__ words, const SegArgs a,
                                                                   const float* __restrict__ pa, const float* __restrict__ pb, uint8_t* __restrict__ status,
                                                                   u32* __restrict__ counts) {
  const size_t i = (size_t) blockIdx.x * kFreeLanes + threadIdx.x;
  if (i >= (size_t) a.n) return;
  const f3 A = mk3(pa[3 * i + 0], pa[3 * i + 1], pa[3 * i + 2]);
  const f3 B = mk3(pb[3 * i + 0], pb[3 * i + 1], pb[3 * i + 2]);
  bool bad = !(fabsf(A.x) < INFINITY && fabsf(A.y) < INFINITY && fabsf(A.z) < INFINITY && fabsf(B.x) < INFINITY && fabsf(B.y) < INFINITY && fabsf(B.z) < INFINITY);
  u32 n = 0, n_free = 0;
  if (!bad) {
    const f3 e = mk3(B.x - A.x, B.y - A.y, B.z - A.z);
    const float len = sqrtf((e.x * e.x + e.y * e.y) + e.z * e.z);  // +inf when the difference overflows: too many samples below
    const f3 d = len == 0.f ? mk3(0.f, 0.f, 0.f) : mk3(e.x / len, e.y / len, e.z / len);
    const RayLine rl = RayLine{A, 0.f, a.step, MRH_FREESPACE_MAX_SAMPLES + 1u};  // z_k = 0 + k * step = k * step
    n = ray_count_samples(rl, MRH_FREESPACE_MAX_SAMPLES + 1u, len);
    bad = n > MRH_FREESPACE_MAX_SAMPLES;
    u32 cur = kFreeNoWord, w = 0;
    for (u32 k = 0; k < n && !bad; ++k) {
      u32 word, bit;
      const FreeCell fc = free_sample(L, vs, a.bound, ray_point(rl, d, ray_z(rl, k)), word, bit);
      if (fc == FREE_CELL_BAD) bad = true;
      if (fc != FREE_CELL_INSIDE) continue;
      if (word != cur) {
        cur = word;
        w = words[word];
      }
      n_free += (w & bit) ? 1u : 0u;
    }
  }
  status[i] = (uint8_t) (bad ? MRH_FREE_SEG_BAD : n_free == n ? 0u : MRH_FREE_SEG_UNKNOWN);
  if (counts) {
    counts[2 * i + 0] = bad ? 0u : n;
    counts[2 * i + 1] = bad ? 0u : n_free;
  }
}

__device__ __forceinline__ size_t free_box_cell(const FreeBox& bx, const int i, const int j, const int k) {
  return ((size_t) k * (size_t) bx.ny + (size_t) j) * (size_t) bx.nx + (size_t) i;
}

// FREE | OBSERVED | OCCUPIED of box cell (i, j, k) from the two ORs over its voxels and the layer's bit
__device__ __forceinline__ void free_store_cell(const FreeLayer& L, const u32* __restrict__ words, const FreeBox& bx, const int i, const int j, const int k,
                                                const bool observed, const bool site, uint8_t* __restrict__ state) {
  u32 st = (observed ? (u32) FREE_OBSERVED : 0u) | (site ? (u32) FREE_OCCUPIED : 0u);
  u32 word, bit;
  if (free_word_of(L, bx.ox + i - L.ox, bx.oy + j - L.oy, bx.oz + k - L.oz, word, bit) == FREE_CELL_INSIDE && (words[word] & bit)) st |= FREE_FREE;
  state[free_box_cell(bx, i, j, k)] = (uint8_t) st;
}

// One workgroup per 8^3 brick of voxel space the box touches (grid: bricks per axis; a cell never straddles a brick), two voxels
// per lane through k_esdf_classify's brick.  The lanes take the brick's voxels cell by cell: voxel index = cell << 3s | position
// in the cell, so the 2^(3s) voxels of a cell are 2^(3s) consecutive lanes of one wave for s <= 2 and their OR is a piece of a
// wave ballot; for s = 3 the brick is one cell and the eight ballots meet in LDS, the workgroup-wide OR.  No atomics, the map and
// the layer are only read.
__global__ __launch_bounds__(256) void k_freespace_classify(const Map m, const Tab t, const FreeLayer L, const u32* __restrict__ words, const FreeBox bx,
                                                            uint8_t* __restrict__ state) {
  __shared__ u32 s_val;
  __shared__ u32 s_or[4];
  const EsdfBox& vb = bx.vox;
  const EsdfBrick br = esdf_brick(m, t, mki3((vb.ox >> 3) + (int) blockIdx.x, (vb.oy >> 3) + (int) blockIdx.y, (vb.oz >> 3) + (int) blockIdx.z), &s_val);
  const int s = L.shift, side_bits = 3 - s;                 // a brick has 2^side_bits cells per side
  const int in_mask = (1 << s) - 1, cell_mask = (1 << side_bits) - 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 both = 0;  // s == 3: this wave's OR over both halves
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int idx = (int) threadIdx.x + 256 * h;
    const int within = idx & ((1 << (3 * s)) - 1), cell = idx >> (3 * s);
    const int lx = ((cell & cell_mask) << s) | (within & in_mask);
    const int ly = (((cell >> side_bits) & cell_mask) << s) | ((within >> s) & in_mask);
    const int lz = ((cell >> (2 * side_bits)) << s) | (within >> (2 * s));
    const int vi = br.v0.x + lx - vb.ox, vj = br.v0.y + ly - vb.oy, vk = br.v0.z + lz - vb.oz;
    const bool in_box = (u32) vi < (u32) vb.nx && (u32) vj < (u32) vb.ny && (u32) vk < (u32) vb.nz;  // the same for every voxel of a cell
    float sdf;
    const u32 st = in_box ? esdf_brick_voxel(m, t, vb, br, lx, ly, lz, sdf) : 0u;
    const u64 obs = __ballot((st & ESDF_OBSERVED) != 0), site = __ballot((st & ESDF_SITE) != 0);
    if (s < 3) {
      const int g = 1 << (3 * s);  // 1, 8 or 64 lanes per cell
      const u64 gm = (g == 64 ? ~0ull : ((1ull << g) - 1)) << (lane & ~(g - 1));
      if (in_box && (lane & (g - 1)) == 0) free_store_cell(L, words, bx, vi >> s, vj >> s, vk >> s, (obs & gm) != 0, (site & gm) != 0, state);
    } else {
      both |= (obs ? (u32) FREE_OBSERVED : 0u) | (site ? (u32) FREE_OCCUPIED : 0u);
    }
  }
  if (s == 3) {  // uniform; the brick is one cell of the box
    if (lane == 0) s_or[wave] = both;
    __syncthreads();
    if (threadIdx.x == 0) {
      const u32 all = (s_or[0] | s_or[1]) | (s_or[2] | s_or[3]);
      free_store_cell(L, words, bx, (br.v0.x - vb.ox) >> 3, (br.v0.y - vb.oy) >> 3, (br.v0.z - vb.oz) >> 3, (all & FREE_OBSERVED) != 0, (all & FREE_OCCUPIED) != 0, state);
    }
  }
}

// The 6-stencil: one lane per cell of the box, `in` the classified bytes, `out` another buffer.  FRONTIER: FREE and not OCCUPIED
// with a face neighbour inside the box that is neither FREE nor OBSERVED
__global__ __launch_bounds__(kFreeLanes) void k_freespace_frontier(const FreeBox bx, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  const size_t cell = (size_t) blockIdx.x * kFreeLanes + threadIdx.x;
  const size_t sx = (size_t) bx.nx, sxy = sx * (size_t) bx.ny;
  if (cell >= sxy * (size_t) bx.nz) return;
  const int i = (int) (cell % sx), j = (int) ((cell / sx) % (size_t) bx.ny), k = (int) (cell / sxy);
  u32 st = in[cell];
  if ((st & FREE_FREE) && !(st & FREE_OCCUPIED)) {
    const u32 known = FREE_FREE | FREE_OBSERVED;
    bool open = false;
    if (i > 0) open = open || !(in[cell - 1] & known);
    if (i + 1 < bx.nx) open = open || !(in[cell + 1] & known);
    if (j > 0) open = open || !(in[cell - sx] & known);
    if (j + 1 < bx.ny) open = open || !(in[cell + sx] & known);
    if (k > 0) open = open || !(in[cell - sxy] & known);
    if (k + 1 < bx.nz) open = open || !(in[cell + sxy] & known);
    if (open) st |= FREE_FRONTIER;
  }
  out[cell] = (uint8_t) st;
}

}  // namespace mrh
