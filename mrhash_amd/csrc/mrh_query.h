// mrh_query.h — point queries: distance, gradient and colour of the map at a list of positions (include/mrhash_query.h;
// DESIGN.md §4.12 and D17).
//
// Reference: trilinearInterpolation (vds.cu:260-338), getVoxelSize (vds.cu:236-240) and getVoxel (vds.cu:163-205) through
// mrh_mc.h's trilinear, get_voxel_size_f and get_voxel_f, used here as they stand.  The reference ships no query; the two
// fields, the refusal rule and the outputs are this project's definition D17.
//
// Layout: one lane per point, 256-lane workgroups, read-only on the map: no atomics, plain loads and stores, every loop
// bounded.  k_query<SMOOTH, POSED>: SMOOTH picks the field, POSED the sensor-to-world transform of the input.  For the MAP
// field each lane resolves the 27 blocks around its point's block once, into its own slice of LDS, and hands the slice to
// trilinear / get_voxel_f through Neigh::vals / Neigh::base.  block_val answers from the slice inside the 3^3 and through the
// table outside it, and a slice entry IS block_val's table answer for that block, so the result is bit for bit that of the
// literal form — every sample through the table (neigh_none, as k_raycast does): about 57 dependent lookups per query against
// 27 independent ones.  The literal form was built, measured slower and dropped.
#pragma once

#include "mrh_mc.h"
#include "mrh_readerplan.h"  // QueryArgs

namespace mrh {

constexpr int kQueryLanes = 256;
constexpr int kQuerySlice = 27;  // words per lane: an odd stride, so the lanes of a wave that read the same index hit distinct banks

// voxel -> block as get_voxel_i converts it: the shift below the limit (mrh_device.h), else the reference's float detour
__device__ __forceinline__ i3 query_block_of(const Map& m, const i3 v) {
  const int ax = v.x < 0 ? -v.x : v.x, ay = v.y < 0 ? -v.y : v.y, az = v.z < 0 ? -v.z : v.z;
  return (u32) (ax | ay | az) < (u32) m.block_shift_limit ? mki3(v.x >> 3, v.y >> 3, v.z >> 3) : voxel_to_block(v, m.vs);
}

// The SMOOTH field's corner at world position `pos`: get_voxel_f, except that a corner in the block `b0` of corner (0, 0, 0)
// reuses that block's table value `val0` (first: this IS corner (0, 0, 0), which resolves them).  False: not found, or weight 0.
// SDF = false: the weight alone is read (the validity pass of mrh_remap.h), `sdf` is left as it is
template <bool SDF>
__device__ __forceinline__ bool query_corner(const Map& m, const Tab& t, const Neigh& nb, const f3 pos, const bool first, i3& b0, u32& val0, float& sdf) {
  const i3 v = world_to_voxel(m.vs, pos);
  const i3 b = query_block_of(m, v);
  u32 val;
  if (first) {
    val = block_val(t, nb, b);
    b0 = b; val0 = val;
  } else {
    val = (b.x == b0.x && b.y == b0.y && b.z == b0.z) ? val0 : block_val(t, nb, b);
  }
  if (val == kNbAbsent) return false;
  const VoxPtr vp = vox_ptr(t, val);
  const u32 li = voxel_local_index(v, (val & kValCoarseBit) ? 1 : 0);
  if (SDF) sdf = vp.sdf[li];
  return (vp.rgbw[li] >> 24) != 0;
}

__device__ __forceinline__ float query_lerp(const float a, const float b, const float w) { return a + w * (b - a); }

// The SMOOTH field of D17 at P, h = the local voxel size at P: the eight corners ((f_x + i) h, (f_y + j) h, (f_z + k) h) through
// query_corner.  False (dist and the gradient untouched) unless all eight are found with weight > 0; the gradient is evaluated
// when want_grad.  k_query and k_remap_sample (mrh_remap.h) both call it
__device__ __forceinline__ bool smooth_field(const Map& m, const Tab& t, const Neigh& nb, const f3 P, const float h, const bool want_grad, float& dist, float& gx,
                                             float& gy, float& gz) {
  const float ux = P.x / h, uy = P.y / h, uz = P.z / h;
  const float fx = floorf(ux), fy = floorf(uy), fz = floorf(uz);
  const float wx = ux - fx, wy = uy - fy, wz = uz - fz;
  float sv[8];
  i3 b0 = mki3(0, 0, 0);
  u32 val0 = kNbAbsent;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const f3 pos = mk3((fx + (float) (c & 1)) * h, (fy + (float) ((c >> 1) & 1)) * h, (fz + (float) ((c >> 2) & 1)) * h);
    sv[c] = 0.f;
    ok = ok && query_corner<true>(m, t, nb, pos, c == 0, b0, val0, sv[c]);
  }
  if (!ok) return false;
  // along x for the four (j, k), then y, then z
  const float c00 = query_lerp(sv[0], sv[1], wx), c10 = query_lerp(sv[2], sv[3], wx), c01 = query_lerp(sv[4], sv[5], wx), c11 = query_lerp(sv[6], sv[7], wx);
  const float c0 = query_lerp(c00, c10, wy), c1 = query_lerp(c01, c11, wy);
  dist = query_lerp(c0, c1, wz);
  if (want_grad) {
    gx = query_lerp(query_lerp(sv[1] - sv[0], sv[3] - sv[2], wy), query_lerp(sv[5] - sv[4], sv[7] - sv[6], wy), wz) / h;
    gy = query_lerp(c10 - c00, c11 - c01, wz) / h;
    gz = (c1 - c0) / h;
  }
  return true;
}

// smooth_field's validity alone: all eight corners found with weight > 0 (the rgbw plane only, no interpolation)
__device__ __forceinline__ bool smooth_valid(const Map& m, const Tab& t, const Neigh& nb, const f3 P, const float h) {
  const float fx = floorf(P.x / h), fy = floorf(P.y / h), fz = floorf(P.z / h);
  i3 b0 = mki3(0, 0, 0);
  u32 val0 = kNbAbsent;
  float unused = 0.f;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const f3 pos = mk3((fx + (float) (c & 1)) * h, (fy + (float) ((c >> 1) & 1)) * h, (fz + (float) ((c >> 2) & 1)) * h);
    ok = ok && query_corner<false>(m, t, nb, pos, c == 0, b0, val0, unused);
  }
  return ok;
}

template <bool SMOOTH, bool POSED>
__global__ __launch_bounds__(kQueryLanes) void k_query(const Map m, const Tab t, const QueryArgs q, const float* __restrict__ xyz, float* __restrict__ out_dist,
                                                        float* __restrict__ out_grad, uint8_t* __restrict__ out_rgbw, uint8_t* __restrict__ out_state) {
  const size_t i = (size_t) blockIdx.x * kQueryLanes + threadIdx.x;
  if (i >= (size_t) q.n) return;  // the partial last workgroup; no barrier below: the LDS slices are lane-private
  const float x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  f3 P = mk3(x, y, z);
  bool refused = false;
  if (POSED) {
    refused = x == 0.f && y == 0.f && z == 0.f;  // a missing return (+-0 in every component)
    P = mk3(((q.R[0] * x + q.R[1] * y) + q.R[2] * z) + q.t[0], ((q.R[3] * x + q.R[4] * y) + q.R[5] * z) + q.t[1],
            ((q.R[6] * x + q.R[7] * y) + q.R[8] * z) + q.t[2]);
  }
  refused = refused || !(fabsf(P.x) < q.bound && fabsf(P.y) < q.bound && fabsf(P.z) < q.bound);  // NaN and Inf fail; before any conversion

  float dist = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  u32 rgbw = 0, state = MRH_QUERY_REFUSED;
  if (!refused) {
    Neigh nb = neigh_none();
    nb.shift_limit = m.block_shift_limit;
    if constexpr (!SMOOTH) {
      __shared__ u32 s_vals[kQueryLanes * kQuerySlice];
      u32* mine = s_vals + threadIdx.x * kQuerySlice;
      const i3 b0 = query_block_of(m, world_to_voxel(m.vs, P));  // |b0| <= 2^17 + 1 under the bound: b0 +- 1 cannot wrap
      const Neigh none = nb;
#pragma unroll 1
      for (int k = 0; k < kQuerySlice; ++k) mine[k] = block_val(t, none, mki3(b0.x + (k % 3 - 1), b0.y + ((k / 3) % 3 - 1), b0.z + (k / 9 - 1)));
      nb.vals = mine;
      nb.base = b0;
    }
    const float h = get_voxel_size_f(m, t, nb, P);
    const VoxSample s = get_voxel_f(m, t, nb, P);
    state = (s.found ? MRH_QUERY_BLOCK : 0u) | (h > m.vs ? MRH_QUERY_COARSE : 0u);
    if (out_rgbw && s.found) rgbw = s.rgbw;
    if (!SMOOTH) {
      if (trilinear(m, t, nb, P, dist)) {
        state |= MRH_QUERY_DIST;
        if (out_grad) {  // central difference over one voxel of the local size, the offset points as in k_raycast's normal
          bool ok = true;
#pragma unroll 1
          for (int a = 0; a < 3 && ok; ++a) {
            f3 pp = P, pm = P;
            if (a == 0) { pp.x = P.x + h; pm.x = P.x - h; }
            else if (a == 1) { pp.y = P.y + h; pm.y = P.y - h; }
            else { pp.z = P.z + h; pm.z = P.z - h; }
            float dp, dm;
            ok = trilinear(m, t, nb, pp, dp) && trilinear(m, t, nb, pm, dm);
            const float g = ok ? (dp - dm) / (h + h) : 0.f;
            if (a == 0) gx = g;
            else if (a == 1) gy = g;
            else gz = g;
          }
          if (ok) state |= MRH_QUERY_GRAD;
          else { gx = 0.f; gy = 0.f; gz = 0.f; }
        }
      } else {
        dist = 0.f;
      }
    } else if (smooth_field(m, t, nb, P, h, out_grad != nullptr, dist, gx, gy, gz)) {
      state |= MRH_QUERY_DIST;
      if (out_grad) state |= MRH_QUERY_GRAD;
    }
  }
  out_dist[i] = dist;
  out_state[i] = (uint8_t) state;
  if (out_grad) {
    out_grad[3 * i + 0] = gx;
    out_grad[3 * i + 1] = gy;
    out_grad[3 * i + 2] = gz;
  }
  if (out_rgbw) {
    out_rgbw[4 * i + 0] = (uint8_t) (rgbw & 0xFF);
    out_rgbw[4 * i + 1] = (uint8_t) ((rgbw >> 8) & 0xFF);
    out_rgbw[4 * i + 2] = (uint8_t) ((rgbw >> 16) & 0xFF);
    out_rgbw[4 * i + 3] = (uint8_t) (rgbw >> 24);
  }
}

}  // namespace mrh
