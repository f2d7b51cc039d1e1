// mrh_esdf.h — the Euclidean signed distance field of a box of the map (include/mrhash_esdf.h): for every
// finest-resolution cell of the box the exact distance, capped at a reach R, to the nearest surface cell ("site") of the box.
//
// The reference has no distance field; the definition is this project's D16.  What it reads of the map is getVoxel
// (vds.cu:163-205) through mrh_mc.h:get_voxel_i, the lookup mrh_get_voxel answers with.
//
// Four launches: k_esdf_classify reads the map once (state byte per cell, a site's own sdf into `dist`), k_esdf_rows finds
// every cell's nearest site along x from wave ballots, k_esdf_columns_y and k_esdf_columns_z add the other two axes of the
// separable squared distance through LDS-staged columns; the z pass finishes the cell.  Squared distances are u32 integers
// (at most 3 * 511^2), cell indices size_t; no atomics, no float sums, plain stores.  The result does not depend on the
// launch shape: every cell's value is a minimum over a fixed set of integers and one correctly rounded square root.
#pragma once

#include "mrh_mc.h"
#include "mrh_readerplan.h"  // EsdfBox

namespace mrh {

constexpr int kEsdfMaxSide = 512;              // MRH_ESDF_MAX_SIDE
constexpr u32 kEsdfNone16 = 0xFFFFu;           // x pass: no site within reach on this row
constexpr u32 kEsdfInf = 0x40000000u;          // column passes: no site so far; kEsdfInf + 511^2 does not wrap
constexpr u32 kEsdfFar = 0xFFFFFFFFu;          // d2 of a `far` cell
constexpr int kEsdfTile = 32;                  // columns (adjacent in x) a workgroup of the column passes owns
constexpr int kEsdfColumnLanes = 8;            // lanes that share one column (256 / kEsdfTile)
enum EsdfState : u32 { ESDF_OBSERVED = 1u, ESDF_SITE = 2u, ESDF_INSIDE = 4u, ESDF_FAR = 8u };

__device__ __forceinline__ size_t esdf_cell(const EsdfBox& bx, const int i, const int j, const int k) {
  return ((size_t) k * (size_t) bx.ny + (size_t) j) * (size_t) bx.nx + (size_t) i;
}

// D16 classification of one voxel sample
__device__ __forceinline__ u32 esdf_classify(const Map& m, const EsdfBox& bx, const bool found, const int res, const float sdf, const u32 rgbw) {
  if (!found || (int) (rgbw >> 24) < bx.w_min) return 0u;
  const float band = bx.band > 0.f ? bx.band : m.vs * (float) (1 << res);
  u32 st = ESDF_OBSERVED;
  if (fabsf(sdf) <= band) st |= ESDF_SITE;  // false for a NaN
  if (sdf < 0.f) st |= ESDF_INSIDE;
  return st;
}

// One 8^3 brick of voxel space as a workgroup of 256 lanes reads it (k_esdf_classify here, k_freespace_classify in
// mrh_freespace.h).  Where voxel -> block is the arithmetic shift for the whole brick, the brick IS one map block: it is resolved
// once and its planes are read directly (a coarse block's 64 voxels each answer for the 2^3 cells they cover); elsewhere every
// voxel takes get_voxel_i.
struct EsdfBrick {
  i3 v0;        // the brick's first voxel
  bool direct;  // uniform
  u32 val;      // direct: the block's table value (kNbAbsent: no block)
  Neigh nb;
};
// brick b, by the whole workgroup: s_val is one word of LDS, and the call holds a barrier when the brick is direct (uniform)
__device__ __forceinline__ EsdfBrick esdf_brick(const Map& m, const Tab& t, const i3 b, u32* s_val) {
  EsdfBrick br;
  br.v0 = mki3(b.x * kBlockSide, b.y * kBlockSide, b.z * kBlockSide);
  const i3 v0 = br.v0;
  // |coordinate| of every cell of the brick is at most this (|v0| <= 2^23 + 8: no overflow)
  const int amax = max(max(max(abs(v0.x), abs(v0.x + kBlockSide - 1)), max(abs(v0.y), abs(v0.y + kBlockSide - 1))), max(abs(v0.z), abs(v0.z + kBlockSide - 1)));
  br.direct = amax < m.block_shift_limit;  // uniform
  br.nb = neigh_none();
  br.nb.shift_limit = m.block_shift_limit;
  if (br.direct) {
    if (threadIdx.x == 0) *s_val = block_val(t, br.nb, b);
    __syncthreads();
  }
  br.val = br.direct ? *s_val : kNbAbsent;
  return br;
}
// the D16 state of the brick's voxel (lx, ly, lz) under bx's two gates, and its sdf
__device__ __forceinline__ u32 esdf_brick_voxel(const Map& m, const Tab& t, const EsdfBox& bx, const EsdfBrick& br, const int lx, const int ly, const int lz,
                                                float& sdf) {
  sdf = 0.f;
  u32 rgbw = 0;
  int res = 0;
  bool found = false;
  if (br.direct) {
    if (br.val != kNbAbsent) {
      found = true;
      res = (br.val & kValCoarseBit) ? 1 : 0;
      const VoxPtr vp = vox_ptr(t, br.val);
      const int idx = res ? (lz >> 1) * 16 + (ly >> 1) * 4 + (lx >> 1) : lz * 64 + ly * 8 + lx;
      sdf = vp.sdf[idx];
      rgbw = vp.rgbw[idx];
    }
  } else {
    const VoxSample s = get_voxel_i(m, t, br.nb, mki3(br.v0.x + lx, br.v0.y + ly, br.v0.z + lz));
    found = s.found; res = s.res; sdf = s.sdf; rgbw = s.rgbw;
  }
  return esdf_classify(m, bx, found, res, sdf, rgbw);
}

// One workgroup per 8^3 brick of voxel space the box touches (grid: bricks per axis), two cells per lane
__global__ __launch_bounds__(256) void k_esdf_classify(const Map m, const Tab t, const EsdfBox bx, uint8_t* __restrict__ state,
                                                       float* __restrict__ dist) {
  __shared__ u32 s_val;
  const EsdfBrick br = esdf_brick(m, t, mki3((bx.ox >> 3) + (int) blockIdx.x, (bx.oy >> 3) + (int) blockIdx.y, (bx.oz >> 3) + (int) blockIdx.z), &s_val);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int li = (int) threadIdx.x + 256 * h;
    const int lx = li & 7, ly = (li >> 3) & 7, lz = li >> 6;
    const int i = br.v0.x + lx - bx.ox, j = br.v0.y + ly - bx.oy, k = br.v0.z + lz - bx.oz;
    if ((u32) i >= (u32) bx.nx || (u32) j >= (u32) bx.ny || (u32) k >= (u32) bx.nz) continue;
    float sdf;
    const u32 st = esdf_brick_voxel(m, t, bx, br, lx, ly, lz, sdf);
    const size_t cell = esdf_cell(bx, i, j, k);
    state[cell] = (uint8_t) st;
    if (st & ESDF_SITE) dist[cell] = sdf;
  }
}

// One wave per x-row (four rows per workgroup).  The row's site bits are eight wave ballots (uniform 64-bit words); a lane owns
// the cells lane, lane + 64, ... and takes the nearest set bit at or below and at or above each of them.  out: |dx| as u16,
// kEsdfNone16 where no site of the row lies within the reach.
__global__ __launch_bounds__(256) void k_esdf_rows(const EsdfBox bx, const uint8_t* __restrict__ state, uint16_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const size_t rows = (size_t) bx.ny * (size_t) bx.nz;
  const size_t row = (size_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // the whole wave; the kernel has no barrier
  const uint8_t* __restrict__ st = state + row * (size_t) bx.nx;
  uint16_t* __restrict__ o = out + row * (size_t) bx.nx;
  u64 words[kEsdfMaxSide / 64];
#pragma unroll
  for (int c = 0; c < kEsdfMaxSide / 64; ++c) {
    const int i = c * 64 + lane;
    words[c] = __ballot(i < bx.nx && (st[i < bx.nx ? i : 0] & ESDF_SITE) != 0);
  }
  const u64 le = ~0ull >> (63 - lane), ge = ~0ull << lane;  // bits at or below / at or above the lane's
#pragma unroll
  for (int c = 0; c < kEsdfMaxSide / 64; ++c) {
    const int i = c * 64 + lane;
    if (c * 64 >= bx.nx) break;  // uniform
    int left = -1, right = -1;
#pragma unroll
    for (int w = c; w >= 0; --w) {
      const u64 x = w == c ? words[w] & le : words[w];
      if (left < 0 && x) left = w * 64 + 63 - __clzll((long long) x);
    }
#pragma unroll
    for (int w = c; w < kEsdfMaxSide / 64; ++w) {
      const u64 x = w == c ? words[w] & ge : words[w];
      if (right < 0 && x) right = w * 64 + __ffsll((unsigned long long) x) - 1;
    }
    u32 d = kEsdfNone16;
    if (left >= 0) d = (u32) (i - left);
    if (right >= 0) d = min(d, (u32) (right - i));
    if (d > bx.reach) d = kEsdfNone16;  // |dx| <= 511 < kEsdfNone16
    if (i < bx.nx) o[i] = (uint16_t) d;
  }
}

// min over the column's cells c within the reach of in[c] + (y - c)^2, expanding outward from y; s: the staged tile,
// [cell of the column][kEsdfTile].  The walk ends where (y - c)^2 alone reaches the best so far: nothing further out can win.
// LDS: a 32-lane half of the wave is one column group (one row, 32 adjacent words, 32 banks), and ds_read_b32 serves the two
// halves separately, so the reads are conflict-free (SQ_LDS_BANK_CONFLICT = 0, profiles/esdf/lds_counters.txt).
__device__ __forceinline__ u32 esdf_column_min(const u32* __restrict__ s, const int len, const int y, const int cx, const u32 reach) {
  u32 best = s[y * kEsdfTile + cx];
  const int dmax = (int) min(reach, (u32) (len - 1));
  for (int d = 1; d <= dmax; ++d) {
    const u32 dd = (u32) (d * d);
    if (dd >= best) break;
    if (y - d >= 0) best = min(best, s[(y - d) * kEsdfTile + cx] + dd);
    if (y + d < len) best = min(best, s[(y + d) * kEsdfTile + cx] + dd);
  }
  return best < kEsdfInf ? best : kEsdfInf;
}

// The y pass: grid (x tiles, nz).  A workgroup stages kEsdfTile columns of ny squared x distances (dynamic LDS:
// kEsdfTile * ny words, at most 64 KiB) and writes min over j' of dx^2 + (j - j')^2; kEsdfInf: none within reach.
__global__ __launch_bounds__(256) void k_esdf_columns_y(const EsdfBox bx, const uint16_t* __restrict__ in, u32* __restrict__ out) {
  extern __shared__ u32 s_col[];
  const int cx = threadIdx.x & (kEsdfTile - 1), g = threadIdx.x / kEsdfTile;
  const int i = (int) blockIdx.x * kEsdfTile + cx, k = (int) blockIdx.y;
  for (int j = g; j < bx.ny; j += kEsdfColumnLanes) {
    u32 v = kEsdfInf;
    if (i < bx.nx) {
      const u32 d = in[esdf_cell(bx, i, j, k)];
      if (d != kEsdfNone16) v = d * d;
    }
    s_col[j * kEsdfTile + cx] = v;
  }
  __syncthreads();
  if (i >= bx.nx) return;
  for (int j = g; j < bx.ny; j += kEsdfColumnLanes) out[esdf_cell(bx, i, j, k)] = esdf_column_min(s_col, bx.ny, j, cx, bx.reach);
}

// The z pass: grid (x tiles, ny), columns of nz staged the same way, and the cell is finished — the reach test, the square root,
// the sign, the far bit.  A site keeps the sdf k_esdf_classify wrote into dist (its d2 is 0 and it is never far).
// out_state / out_d2 may be nullptr (not wanted); out_state may be `state` itself.
__global__ __launch_bounds__(256) void k_esdf_columns_z(const Map m, const EsdfBox bx, const u32* __restrict__ in, const uint8_t* state,
                                                        float* __restrict__ dist, uint8_t* out_state, u32* __restrict__ out_d2) {
  extern __shared__ u32 s_col[];
  const int cx = threadIdx.x & (kEsdfTile - 1), g = threadIdx.x / kEsdfTile;
  const int i = (int) blockIdx.x * kEsdfTile + cx, j = (int) blockIdx.y;
  for (int k = g; k < bx.nz; k += kEsdfColumnLanes) s_col[k * kEsdfTile + cx] = i < bx.nx ? in[esdf_cell(bx, i, j, k)] : kEsdfInf;
  __syncthreads();
  if (i >= bx.nx) return;
  const u32 r2 = bx.reach * bx.reach;  // <= 4095^2
  for (int k = g; k < bx.nz; k += kEsdfColumnLanes) {
    const u32 d2 = esdf_column_min(s_col, bx.nz, k, cx, bx.reach);
    const bool far = d2 > r2;  // kEsdfInf > 4095^2: "no site" is far
    const size_t cell = esdf_cell(bx, i, j, k);
    const u32 st = state[cell];
    if (!(st & ESDF_SITE)) {
      const float mag = m.vs * (far ? (float) bx.reach : sqrtf((float) d2));
      dist[cell] = (st & ESDF_INSIDE) ? -mag : mag;
    }
    if (out_state) out_state[cell] = (uint8_t) (st | (far ? (u32) ESDF_FAR : 0u));
    if (out_d2) out_d2[cell] = far ? kEsdfFar : d2;
  }
}

}  // namespace mrh
