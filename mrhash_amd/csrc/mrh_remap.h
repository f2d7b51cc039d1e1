// mrh_remap.h — map-to-map fusion: a map resampled under a rigid pose onto another lattice, as block records
// (include/mrhash_remap.h).
//
// The reference ships no such call; the definition is this project's D18.  The samples are D17's SMOOTH field (smooth_field,
// mrh_query.h) and getVoxel (vds.cu:163-205) on the source map, used as they stand.
//
// Stages, all read-only on the map, no atomic decides the order or the set of the records:
//   k_remap_candidates   one lane per live source block: the packed keys of the destination blocks its transformed cube can
//                        meet, into the lane's own per_axis^3 slots (unused slots hold kKeyEmpty, which sorts last)
//   radix sort (mrh_sort.h), k_remap_mark_first, the chained scan (k_tile_sums_u64 / k_tile_scan_u64), k_remap_compact
//                        the distinct candidate keys in key order == (x, y, z) order, the order of mrh_pack_blocks
//   k_remap_flags        one 512-lane workgroup per candidate: validity only (the rgbw plane, no interpolation) -> mark and the
//                        count of valid voxels; scan and k_remap_compact again: the kept blocks
//   k_remap_sample       one 512-lane workgroup per kept block, one lane per voxel, 12 bytes per lane straight into the record
// Both 512-lane kernels transform the block's eight corner voxels once; when their source blocks span at most 3 per axis the 27
// table values go to LDS and reach the lookups through Neigh::vals / Neigh::base, else every sample goes through the table.
// block_val answers the same either way, so both forms give the same bits.
#pragma once

#include "mrh_query.h"
#include "mrh_sort.h"

namespace mrh {

constexpr int kRemapLanes = 512;  // one lane per voxel of a destination block

// P of voxel `v` (storage index lz * 64 + ly * 8 + lx) of destination block b; false: outside the range rule (D18)
__device__ __forceinline__ bool remap_point(const RemapArgs& a, const i3 b, const int v, f3& P) {
  const f3 W = voxel_to_world(a.vs_d, mki3(b.x * kBlockSide + (v & 7), b.y * kBlockSide + ((v >> 3) & 7), b.z * kBlockSide + (v >> 6)));
  const float dx = W.x - a.t[0], dy = W.y - a.t[1], dz = W.z - a.t[2];
  P = mk3((a.R[0] * dx + a.R[3] * dy) + a.R[6] * dz, (a.R[1] * dx + a.R[4] * dy) + a.R[7] * dz, (a.R[2] * dx + a.R[5] * dy) + a.R[8] * dz);
  return fabsf(P.x) < a.bound && fabsf(P.y) < a.bound && fabsf(P.z) < a.bound;  // NaN and Inf fail; before any conversion
}

// getVoxel(P) (get_voxel_f's lookup) with what a record keeps of it: sum_squared and r, g, b, weight.  False: not found
template <bool SUMSQ>
__device__ __forceinline__ bool remap_nearest(const Map& m, const Tab& t, const Neigh& nb, const f3 P, u32& sumsq_bits, u32& rgbw) {
  const i3 v = world_to_voxel(m.vs, P);
  const u32 val = block_val(t, nb, query_block_of(m, v));
  if (val == kNbAbsent) return false;
  const VoxPtr vp = vox_ptr(t, val);
  const u32 li = voxel_local_index(v, (val & kValCoarseBit) ? 1 : 0);
  if (SUMSQ) sumsq_bits = __float_as_uint(vp.sumsq[li]);
  rgbw = vp.rgbw[li];
  return true;
}

// Workgroup-uniform: the Neigh of destination block b.  Lanes 0 .. 7 transform the block's corner voxels; when all eight are in
// range and their source blocks span at most 3 per axis, lanes 0 .. 26 resolve that 3^3 into s_vals.  Two barriers
__device__ __forceinline__ Neigh remap_neigh(const Map& m, const Tab& t, const RemapArgs& a, const i3 b, u32* s_vals, int* s_corner) {
  Neigh nb = neigh_none();
  nb.shift_limit = m.block_shift_limit;
  if (threadIdx.x < 8) {
    const int k = (int) threadIdx.x;
    f3 P;
    const bool ok = remap_point(a, b, ((k & 1) ? 7 : 0) + ((k & 2) ? 56 : 0) + ((k & 4) ? 448 : 0), P);
    const i3 cb = ok ? query_block_of(m, world_to_voxel(m.vs, P)) : mki3(0, 0, 0);
    s_corner[4 * k + 0] = cb.x; s_corner[4 * k + 1] = cb.y; s_corner[4 * k + 2] = cb.z; s_corner[4 * k + 3] = ok ? 1 : 0;
  }
  __syncthreads();
  i3 lo = mki3(s_corner[0], s_corner[1], s_corner[2]), hi = lo;
  bool fits = true;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    fits = fits && s_corner[4 * k + 3] != 0;
    lo.x = min(lo.x, s_corner[4 * k + 0]); hi.x = max(hi.x, s_corner[4 * k + 0]);
    lo.y = min(lo.y, s_corner[4 * k + 1]); hi.y = max(hi.y, s_corner[4 * k + 1]);
    lo.z = min(lo.z, s_corner[4 * k + 2]); hi.z = max(hi.z, s_corner[4 * k + 2]);
  }
  // in range, |block| <= 2^17 + 1: neither the differences nor lo + 2 can wrap
  fits = fits && hi.x - lo.x <= 2 && hi.y - lo.y <= 2 && hi.z - lo.z <= 2;
  if (fits) {
    const i3 base = mki3(lo.x + 1, lo.y + 1, lo.z + 1);
    if (threadIdx.x < 27) {
      const int k = (int) threadIdx.x;
      s_vals[k] = block_val(t, nb, mki3(base.x + (k % 3 - 1), base.y + ((k / 3) % 3 - 1), base.z + (k / 9 - 1)));  // nb.vals is still null: the table
    }
    nb.vals = s_vals;
    nb.base = base;
  }
  __syncthreads();
  return nb;
}

// One lane per live source block (Tab::compact[0, n_src), the kSelAll selection): the packed keys of the destination blocks
// that can hold a valid voxel whose corner (0, 0, 0) lies in this block, into slots [i * per_axis^3, (i + 1) * per_axis^3).
// In binary64: the block's cube [8 b, 8 b + 8] vs_s — grown by one voxel beyond the shift limit, where voxel -> block may
// assign a face voxel to the neighbour — through W = F P + t, its axis-aligned bound grown by one destination voxel and by the
// rounding allowance of the sample kernels' binary32 arithmetic, then clipped to the packed-key range.  The
// counts per axis are clamped to per_axis, which the plan sized the slots by (never reached for a pose the plan accepts).
__global__ __launch_bounds__(256) void k_remap_candidates(const Map m, const Tab t, const RemapArgs a, const u32 n_src, u64* __restrict__ keys) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_src) return;
  const int pa = a.per_axis;
  u64* mine = keys + (size_t) i * (size_t) (pa * pa * pa);
  const int4 ent = t.compact[i];
  const double vs_s = (double) m.vs, vs_d = (double) a.vs_d;
  const int bc[3] = {ent.x, ent.y, ent.z};
  int reach = 0;
  for (int k = 0; k < 3; k++) reach = max(reach, max(abs(bc[k] * kBlockSide), abs(bc[k] * kBlockSide + kBlockSide)));
  const int grow = reach >= m.block_shift_limit ? 1 : 0;
  double c[2][3], Mp = 0.0;
  for (int k = 0; k < 3; k++) {
    c[0][k] = (double) (bc[k] * kBlockSide - grow) * vs_s;
    c[1][k] = (double) (bc[k] * kBlockSide + kBlockSide + grow) * vs_s;
    Mp = fmax(Mp, fmax(fabs(c[0][k]), fabs(c[1][k])));
  }
  double lo[3], hi[3], Mw = 0.0;
  for (int corner = 0; corner < 8; corner++) {
    const double px = c[corner & 1][0], py = c[(corner >> 1) & 1][1], pz = c[(corner >> 2) & 1][2];
    for (int k = 0; k < 3; k++) {
      const double w = (a.F[3 * k] * px + a.F[3 * k + 1] * py + a.F[3 * k + 2] * pz) + (double) a.t[k];
      lo[k] = corner ? fmin(lo[k], w) : w;
      hi[k] = corner ? fmax(hi[k], w) : w;
      Mw = fmax(Mw, fabs(w));
    }
  }
  // one destination voxel + the rounding allowance: 2^-24 |W| for W = (float) v * vs_d, at most vs_d / 2 inside the key range,
  // and 27 * 2^-24 |P| for the rest of the chain, at most 1.75 vs_s inside the range rule
  const double margin = vs_d + fmin(Mw * (1.01 / 16777216.0), 0.5 * vs_d) + fmin(Mp * (27.0 / 16777216.0), 1.75 * vs_s);
  int b0[3], nb[3];
  bool any = true;
  for (int k = 0; k < 3; k++) {
    const double edge = (double) kKeyBias;
    const double first = fmax(floor(floor((lo[k] - margin) / vs_d) / 8.0), -edge);
    const double last = fmin(floor(ceil((hi[k] + margin) / vs_d) / 8.0), edge - 1.0);
    any = any && first <= last;  // false as well when a bound is NaN
    b0[k] = any ? (int) first : 0;
    nb[k] = any ? min((int) (last - first) + 1, pa) : 0;
  }
  int slot = 0;
  if (any)
    for (int x = 0; x < nb[0]; x++)
      for (int y = 0; y < nb[1]; y++)
        for (int z = 0; z < nb[2]; z++) {
          u64 key = kKeyEmpty;
          pack_key(mki3(b0[0] + x, b0[1] + y, b0[2] + z), key);  // inside the range by the clip above
          mine[slot++] = key;
        }
  for (; slot < pa * pa * pa; slot++) mine[slot] = kKeyEmpty;
}

// marks[i] = 1 for the first of each run of equal keys of the sorted list, 0 for its repeats and for the unused slots
__global__ __launch_bounds__(256) void k_remap_mark_first(const u64* __restrict__ keys, const u32 n, u64* __restrict__ marks) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const u64 k = keys[i];
  marks[i] = (k != kKeyEmpty && (i == 0 || keys[i - 1] != k)) ? 1ull : 0ull;
}

// the marked keys to their positions (the exclusive scan of the marks): order kept
__global__ __launch_bounds__(256) void k_remap_compact(const u64* __restrict__ keys, const u64* __restrict__ marks, const u64* __restrict__ pos, const u32 n,
                                                        u64* __restrict__ out) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i < n && marks[i]) out[pos[i]] = keys[i];
}

// What a lane needs to know of its voxel before it samples: P in range, nearest found with weight >= w_min
template <bool SUMSQ>
__device__ __forceinline__ bool remap_voxel(const Map& m, const Tab& t, const Neigh& nb, const RemapArgs& a, const i3 b, f3& P, float& h, u32& sumsq_bits, u32& rgbw) {
  if (!remap_point(a, b, (int) threadIdx.x, P)) return false;
  h = get_voxel_size_f(m, t, nb, P);
  return remap_nearest<SUMSQ>(m, t, nb, P, sumsq_bits, rgbw) && (rgbw >> 24) >= a.w_min;
}

// One workgroup per candidate block (grid-stride): marks[e] = the block has a valid voxel; valid_total += its valid voxels (a
// sum of integers: the order of the additions does not show)
__global__ __launch_bounds__(kRemapLanes) void k_remap_flags(const Map m, const Tab t, const RemapArgs a, const u64* __restrict__ cand, const u32 n,
                                                            u64* __restrict__ marks, u64* __restrict__ valid_total) {
  __shared__ u32 s_vals[27];
  __shared__ int s_corner[32];
  for (u32 e = blockIdx.x; e < n; e += gridDim.x) {
    const i3 b = unpack_key(cand[e]);
    const Neigh nb = remap_neigh(m, t, a, b, s_vals, s_corner);
    f3 P;
    float h;
    u32 ss, rgbw;
    const bool ok = remap_voxel<false>(m, t, nb, a, b, P, h, ss, rgbw) && smooth_valid(m, t, nb, P, h);
    const int cnt = __syncthreads_count(ok ? 1 : 0);  // also: every lane is done with s_vals before the next block's corners
    if (threadIdx.x == 0) {
      marks[e] = cnt ? 1ull : 0ull;
      if (cnt) atomicAdd((unsigned long long*) valid_total, (unsigned long long) cnt);
    }
  }
}

// One workgroup per kept block (grid-stride), one lane per voxel: the record of block kept[e] at records + e * 6160
__global__ __launch_bounds__(kRemapLanes) void k_remap_sample(const Map m, const Tab t, const RemapArgs a, const u64* __restrict__ kept, const u32 n,
                                                             char* __restrict__ records) {
  __shared__ u32 s_vals[27];
  __shared__ int s_corner[32];
  for (u32 e = blockIdx.x; e < n; e += gridDim.x) {
    const i3 b = unpack_key(kept[e]);
    const Neigh nb = remap_neigh(m, t, a, b, s_vals, s_corner);
    char* rec = records + (size_t) e * sizeof(mrh_block_record);
    if (threadIdx.x == 0) *(int4*) rec = make_int4(b.x, b.y, b.z, 0);
    f3 P;
    float h, dist = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    u32 ss = 0, rgbw = 0;
    const bool ok = remap_voxel<true>(m, t, nb, a, b, P, h, ss, rgbw) && smooth_field(m, t, nb, P, h, false, dist, gx, gy, gz);
    u32* out = (u32*) (rec + sizeof(mrh_block_desc) + (size_t) threadIdx.x * sizeof(mrh_voxel));
    out[0] = ok ? __float_as_uint(dist) : 0u;
    out[1] = ok ? ss : 0u;
    out[2] = ok ? rgbw : 0u;
    __syncthreads();  // every lane is done with s_vals before the next block's corners
  }
}
static_assert(sizeof(mrh_block_record) == 6160 && sizeof(mrh_block_desc) == 16 && sizeof(mrh_voxel) == 12, "the record layout k_pack_records writes");

}  // namespace mrh
