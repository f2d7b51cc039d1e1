// mrh_raycast.h — rendering the map from a pinhole or a spherical camera: depth (pinhole) or range (spherical), world-frame
// normal and colour of the first zero crossing of the TSDF along every pixel ray, and for the spherical camera the crossing as a
// sensor-frame point: an organised scan (include/mrhash_raycast.h).
//
// Reference: findIntersectionBisection (vds.cu:348-383) with n_iteration_bisection = 3 (params.h:26), trilinearInterpolation
// (vds.cu:260-338, restated by mrh_mc.h:trilinear, which is used here as it is), getVoxelSize (vds.cu:236-240), getVoxel
// (vds.cu:163-205), inverseProjection (camera.cuh:88) and normalize (cuda_math.cuh:1075-1078).  The reference ships no kernel
// that marches a ray; the march, the hit rule and the outputs are this project's definition D11.
//
// Layout: one lane per pixel, a wave64 renders an 8 x 8 tile (its rays share blocks and table slots), a workgroup of four
// waves a 16 x 16 tile.  Read-only on the map: no atomics, plain stores of the images.  k_raycast<false> is the pinhole
// render, k_raycast<true> the spherical one: they differ in the ray's direction and in the points image, nothing else.
#pragma once

#include "mrh_mc.h"
#include "mrh_readerplan.h"  // RayCam

namespace mrh {

constexpr int kRenderTile = 16;                 // pixels per side of a workgroup's tile
constexpr int kRayBisections = 3;               // n_iteration_bisection (params.h:26)
constexpr float kRaySkipReachVoxels = 65000.f;  // rays that stay within this many voxels of the origin may jump (see ray_skip_absent)

// What the march helpers below take of a ray besides its direction: where it starts and how it is sampled.  The renders build it
// from the camera (one origin for the image: uniform values), k_cast_rays (mrh_rays.h) per lane, with the ray's own origin and
// its own number of samples
struct RayLine {
  f3 o;             // origin, world frame
  float z0, step;   // z_k = z0 + k * step
  u32 n_samples;    // samples of THIS ray: a jump never runs past n_samples - 1
};
__device__ __forceinline__ RayLine ray_line(const RayCam& rc) { return RayLine{mk3(rc.t[0], rc.t[1], rc.t[2]), rc.min_depth, rc.step, rc.n_samples}; }

// z_k, computed afresh for every k (never accumulated)
__device__ __forceinline__ float ray_z(const RayLine& rl, const u32 k) { return rl.z0 + (float) k * rl.step; }
// P(z) = o + z d_w (vds.cu:368: world_cam_pos + c * world_dir)
__device__ __forceinline__ f3 ray_point(const RayLine& rl, const f3 d, const float z) {
  return mk3(rl.o.x + z * d.x, rl.o.y + z * d.y, rl.o.z + z * d.z);
}

// Sample k lies in the ABSENT block b.  Returns the next sample that has to be looked at: k + 1, or one past the last sample
// that provably lies in b as well (every sample in between is invalid by rule 3, so jumping over it changes no bit).
//
// Rounding argument (the caller guarantees that every position of the ray, the block's corners included, is within
// kRaySkipReachVoxels < 2^16 voxels of the origin, and that every voxel of b converts to its block by the arithmetic shift):
// the box is b's world extent shrunk by 0.25 voxel per side, lo = (8 b - 0.25) vs, hi = (8 b + 7.25) vs (8 b +- 0.25 is
// exact in binary32 here; the product rounds once).  A sample is skipped only when its computed z satisfies
// z_in <= z_k' <= z_out for the computed slab interval of every axis (z_k' is monotone in k', so testing the first and the last
// skipped sample covers all of them).  For an axis with d > 0, z_k' <= RN(RN(hi - t) / d) gives t + z d <= hi + |hi - t| 2^-23,
// and RN(t + RN(z d)) adds at most 2^-24 (|z d| + |P|); likewise at lo and for d < 0; d == 0 leaves the coordinate at t,
// which must lie inside [lo, hi].  With every magnitude below 2^17 voxels these are at most 5 * 2^17 * 2^-24 < 0.04 voxel;
// worldPointToVirtualVoxelPos (P / vs, +- 0.5, + 1e-5, floor / ceil) adds three more roundings of at most 2^-7 voxel and the
// 1e-5 epsilon.  So P / vs stays within 0.07 voxel of [8 b - 0.25, 8 b + 7.25], rounds to a voxel in [8 b, 8 b + 7] per axis,
// and that voxel's block is b (shift).  Samples before the ray enters the shrunk box (z_k < z_in: the current sample sits in
// the quarter-voxel rim) are not jumped; they get the literal test like every other sample that is not skipped.
__device__ __forceinline__ u32 ray_skip_absent(const RayLine& rl, const f3 d, const float vs, const i3 b, const u32 k, const float z) {
  const float ob[3] = {rl.o.x, rl.o.y, rl.o.z};
  const float db[3] = {d.x, d.y, d.z};
  const int bb[3] = {b.x, b.y, b.z};
  float z_in = -INFINITY, z_out = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = ((float) (bb[a] * kBlockSide) - 0.25f) * vs;
    const float hi = ((float) (bb[a] * kBlockSide + (kBlockSide - 1)) + 0.25f) * vs;
    if (db[a] > 0.f) {
      z_in = fmaxf(z_in, (lo - ob[a]) / db[a]);
      z_out = fminf(z_out, (hi - ob[a]) / db[a]);
    } else if (db[a] < 0.f) {
      z_in = fmaxf(z_in, (hi - ob[a]) / db[a]);
      z_out = fminf(z_out, (lo - ob[a]) / db[a]);
    } else if (!(ob[a] >= lo && ob[a] <= hi)) {
      return k + 1;
    }
  }
  if (!(z >= z_in)) return k + 1;  // the current sample is in the rim (or NaN): no jump
  const float kf = floorf((z_out - rl.z0) / rl.step);
  if (!(kf >= (float) (k + 1))) return k + 1;
  u32 last = kf >= (float) (rl.n_samples - 1) ? rl.n_samples - 1 : (u32) kf;
  if (!(ray_z(rl, last) <= z_out)) {  // kf may be one too high; z_k itself decides
    last--;
    if (last <= k || !(ray_z(rl, last) <= z_out)) return k + 1;
  }
  return last + 1;
}

// findIntersectionBisection (vds.cu:348-383): a = z_{k-1} (D > 0), b = z_k (D <= 0).  False: a trilinear inside the
// refinement failed and the crossing is rejected.
__device__ __forceinline__ bool ray_refine(const Map& m, const Tab& t, const Neigh& nb, const RayLine& rl, const f3 d, float a, float ad, float b,
                                           float bd, float& out) {
  float c = a;
#pragma unroll 1
  for (int i = 0; i < kRayBisections; ++i) {
    c = a + (ad / (ad - bd)) * (b - a);
    float cd;
    if (!trilinear(m, t, nb, ray_point(rl, d, c), cd)) return false;
    if (ad * cd > 0.f) {
      a = c; ad = cd;
    } else {
      b = c; bd = cd;
    }
  }
  out = c;
  return true;
}

// The sensor-frame direction of pixel (r, c).  Pinhole: camera.cuh:88 with d = 1.  Spherical: camera.cuh:91-99 with d = 1, the
// expressions of inverse_projection_m (mrh_device.h) — azimuth from the column, elevation from the row, sine and cosine through
// mrh_sincosf (the host has checked that every pixel's angle is in its domain).
template <bool SPH>
__device__ __forceinline__ f3 ray_dir_sensor(const RayCam& rc, const int r, const int c) {
  const float u = rc.ifx * (((float) c - rc.cx) - 0.5f);
  const float v = rc.ify * (((float) r - rc.cy) - 0.5f);
  if (!SPH) return mk3(u, v, 1.f);
  float s0, c0, s1, c1;
  mrh_sincosf(u, &s0, &c0);
  mrh_sincosf(v, &s1, &c1);
  return mk3(c0 * c1, s0 * c1, s1);
}

// out_depth: camera z of the crossing (pinhole) or the range along the ray (spherical).  out_points (spherical only): the
// crossing in the sensor frame, range * d_c = inverse_projection_m(r, c, range); a miss is (0, 0, 0), a missing return.
template <bool SPH>
__global__ __launch_bounds__(256) void k_raycast(const Map m, const Tab t, const RayCam rc, float* __restrict__ out_depth,
                                                 float* __restrict__ out_normals, uint8_t* __restrict__ out_rgb, float* __restrict__ out_points) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * kRenderTile + (wave & 1) * 8 + (lane & 7);
  const int r = blockIdx.y * kRenderTile + (wave >> 1) * 8 + (lane >> 3);
  if (r >= rc.rows || c >= rc.cols) return;
  // d_w = R d_c with every row summed left to right (cuda_algebra.cuh:71-75)
  f3 d;
  {
    const f3 dc = ray_dir_sensor<SPH>(rc, r, c);
    d = mk3(rc.R[0] * dc.x + rc.R[1] * dc.y + rc.R[2] * dc.z, rc.R[3] * dc.x + rc.R[4] * dc.y + rc.R[5] * dc.z,
            rc.R[6] * dc.x + rc.R[7] * dc.y + rc.R[8] * dc.z);
  }
  Neigh nb = neigh_none();  // no workgroup neighbourhood: every block through the table
  nb.shift_limit = m.block_shift_limit;
  // empty-space skipping is allowed when every position of this ray stays within kRaySkipReachVoxels of the origin
  // (ray_skip_absent's rounding argument); the margin to 2^16 covers the rounding of this estimate and the block corners
  const float reach = fmaxf(fmaxf(fabsf(rc.t[0]), fabsf(rc.t[1])), fabsf(rc.t[2])) + rc.max_depth * fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
  const bool may_skip = reach < kRaySkipReachVoxels * m.vs;
  const RayLine rl = ray_line(rc);

  // the march: the lane remembers the last block it probed (position, present or absent)
  bool cached = false, present = false;
  i3 cb = mki3(0, 0, 0);
  bool prev_valid = false;
  float prev_d = 0.f, prev_z = 0.f;
  bool hit = false;
  float depth = 0.f;
  for (u32 k = 0; k < rc.n_samples;) {
    const float z = ray_z(rl, k);
    const f3 P = ray_point(rl, d, z);
    const i3 v = world_to_voxel(m.vs, P);
    const int ax = v.x < 0 ? -v.x : v.x, ay = v.y < 0 ? -v.y : v.y, az = v.z < 0 ? -v.z : v.z;
    const bool shift = (u32) (ax | ay | az) < (u32) m.block_shift_limit;  // voxel -> block is the shift below the limit (mrh_device.h)
    const i3 b = shift ? mki3(v.x >> 3, v.y >> 3, v.z >> 3) : voxel_to_block(v, m.vs);
    if (!cached || b.x != cb.x || b.y != cb.y || b.z != cb.z) {
      cb = b;
      cached = true;
      present = block_val(t, nb, b) != kNbAbsent;  // a key outside the packed range, or one without storage, is absent
    }
    if (!present) {  // rule 3: invalid
      prev_valid = false;
      const int m0 = b.x * kBlockSide, m1 = b.y * kBlockSide, m2 = b.z * kBlockSide;
      const int bmax = max(max(max(abs(m0), abs(m0 + kBlockSide - 1)), max(abs(m1), abs(m1 + kBlockSide - 1))), max(abs(m2), abs(m2 + kBlockSide - 1)));
      k = (may_skip && bmax < m.block_shift_limit) ? ray_skip_absent(rl, d, m.vs, b, k, z) : k + 1;
      continue;
    }
    float D;
    const bool ok = trilinear(m, t, nb, P, D);
    if (ok && prev_valid && prev_d > 0.f && D <= 0.f && ray_refine(m, t, nb, rl, d, prev_z, prev_d, z, D, depth)) {
      hit = true;
      break;
    }
    prev_valid = ok;
    prev_d = D;
    prev_z = z;
    ++k;
  }

  float n[3] = {0.f, 0.f, 0.f};
  u32 rgbw = 0;
  if (hit) {
    const f3 P = ray_point(rl, d, depth);
    if (out_normals) {  // central difference over one voxel of the local size, normalised as cuda_math.cuh:1075-1078
      const float h = get_voxel_size_f(m, t, nb, P);
      float g[3];
      bool ok = true;
#pragma unroll 1
      for (int a = 0; a < 3 && ok; ++a) {
        f3 pp = P, pm = P;
        if (a == 0) { pp.x = P.x + h; pm.x = P.x - h; }
        else if (a == 1) { pp.y = P.y + h; pm.y = P.y - h; }
        else { pp.z = P.z + h; pm.z = P.z - h; }
        float dp, dm;
        ok = trilinear(m, t, nb, pp, dp) && trilinear(m, t, nb, pm, dm);
        g[a] = ok ? dp - dm : 0.f;
      }
      if (ok) {
        const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        if (len != 0.f) {
          const float inv = 1.f / len;
          n[0] = g[0] * inv; n[1] = g[1] * inv; n[2] = g[2] * inv;
        }
      }
    }
    if (out_rgb) {
      const VoxSample s = get_voxel_f(m, t, nb, P);
      if (s.found) rgbw = s.rgbw;
    }
  }
  const size_t pix = (size_t) r * (size_t) rc.cols + (size_t) c;
  if (out_depth) out_depth[pix] = depth;
  if (out_normals) {
    out_normals[3 * pix + 0] = n[0];
    out_normals[3 * pix + 1] = n[1];
    out_normals[3 * pix + 2] = n[2];
  }
  if (out_rgb) {
    out_rgb[3 * pix + 0] = (uint8_t) (rgbw & 0xFF);
    out_rgb[3 * pix + 1] = (uint8_t) ((rgbw >> 8) & 0xFF);
    out_rgb[3 * pix + 2] = (uint8_t) ((rgbw >> 16) & 0xFF);
  }
  if (SPH && out_points) {  // d_c again rather than three registers held across the march: the same operations, the same bits
    const f3 dc = ray_dir_sensor<SPH>(rc, r, c);
    out_points[3 * pix + 0] = hit ? depth * dc.x : 0.f;  // a miss is +0 in every component, whatever the sign of d_c
    out_points[3 * pix + 1] = hit ? depth * dc.y : 0.f;
    out_points[3 * pix + 2] = hit ? depth * dc.z : 0.f;
  }
}

}  // namespace mrh
