// mrh_rays.h — ray queries: a list of arbitrary rays cast through the map, each with its own origin, direction and end; per ray the
// refined range, normal and colour of the first zero crossing as the renders find it, and what the ray crossed on its way: how many
// samples were observed free space, how many were unknown, where the first unknown one lies, and whether it ran behind a surface
// (include/mrhash_rays.h).
//
// The march, the hit rule, the refinement, the normal and the colour are k_raycast's (mrh_raycast.h, D11) through the same device
// functions — trilinear, block_val, get_voxel_f, get_voxel_size_f (mrh_mc.h), ray_refine and the absent-block jump ray_skip_absent
// (mrh_raycast.h) — used as they are.  What differs from the render:
//   origin      per lane: the jump and its reach gate take the lane's o_w, the reach estimate the ray's own end
//   the jump    counts as unknown: n_unknown += next - k, first_unknown is the sample the jump started from; it is clamped to
//               the ray's own number of samples (RayLine::n_samples), not the batch's
//   bad rays    leave before any float -> int conversion and before the march
//
// Layout: one lane per ray, 256-lane workgroups; a wave64 takes 64 CONSECUTIVE rays of the caller's order, so the caller's order
// decides how coherent a wave's blocks and table slots are (the render's 8 x 8 tiles are one good order).  Nothing is sorted or
// reordered here.  Read-only on the map: no atomics, no LDS, no barrier, plain stores of the outputs; a ray's outputs depend on
// no other lane.  The last workgroup may be partial.
#pragma once

#include "mrh_raycast.h"
#include "mrh_readerplan.h"  // RaysArgs

namespace mrh {

constexpr int kRaysLanes = 256;

// samples of a ray that ends at `end`: the k < n with z_k <= end.  z_k is monotone in k (two monotone roundings), so the count is
// found by bisection on k with z_k itself, as the host counts the batch's samples (mrh_plan::ray_sample_count)
__device__ __forceinline__ u32 ray_count_samples(const RayLine& rl, const u32 n, const float end) {
  if (!(ray_z(rl, 0) <= end)) return 0;       // also a NaN end, which a bad ray never brings here
  if (ray_z(rl, n - 1) <= end) return n;
  u32 lo = 0, hi = n - 1;                     // z(lo) <= end < z(hi)
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (ray_z(rl, mid) <= end) lo = mid;
    else hi = mid;
  }
  return hi;
}

__global__ __launch_bounds__(kRaysLanes) void k_cast_rays(const Map m, const Tab t, const RaysArgs a, const float* __restrict__ origins,
                                                          const float* __restrict__ dirs, const float* __restrict__ tmax, float* __restrict__ out_range,
                                                          uint8_t* __restrict__ out_status, float* __restrict__ out_normals, uint8_t* __restrict__ out_rgb,
                                                          u32* __restrict__ out_counts, float* __restrict__ out_first) {
  const size_t i = (size_t) blockIdx.x * kRaysLanes + threadIdx.x;
  if (i >= (size_t) a.n) return;  // the partial last workgroup; no barrier below
  f3 o = mk3(origins[3 * i + 0], origins[3 * i + 1], origins[3 * i + 2]);
  f3 d = mk3(dirs[3 * i + 0], dirs[3 * i + 1], dirs[3 * i + 2]);
  if (a.posed) {  // every row summed left to right, the translation last
    const f3 os = o, ds = d;
    o = mk3(((a.R[0] * os.x + a.R[1] * os.y) + a.R[2] * os.z) + a.t[0], ((a.R[3] * os.x + a.R[4] * os.y) + a.R[5] * os.z) + a.t[1],
            ((a.R[6] * os.x + a.R[7] * os.y) + a.R[8] * os.z) + a.t[2]);
    d = mk3((a.R[0] * ds.x + a.R[1] * ds.y) + a.R[2] * ds.z, (a.R[3] * ds.x + a.R[4] * ds.y) + a.R[5] * ds.z, (a.R[6] * ds.x + a.R[7] * ds.y) + a.R[8] * ds.z);
  }
  float end = a.max_range;
  bool bad = false;
  if (tmax) {
    const float tm = tmax[i];
    bad = tm != tm;
    end = fminf(tm, a.max_range);
  }
  // NaN and +-Inf fail every comparison below; nothing has been converted to an integer yet
  bad = bad || !(fabsf(o.x) < a.bound && fabsf(o.y) < a.bound && fabsf(o.z) < a.bound);
  bad = bad || !(fabsf(d.x) < INFINITY && fabsf(d.y) < INFINITY && fabsf(d.z) < INFINITY);
  bad = bad || (d.x == 0.f && d.y == 0.f && d.z == 0.f);

  bool hit = false, inside = false, have_unknown = false;
  float range = 0.f, first_unknown = 0.f;
  u32 n_free = 0, n_unknown = 0;
  float n[3] = {0.f, 0.f, 0.f};
  u32 rgbw = 0;
  if (!bad) {
    RayLine rl = RayLine{o, a.min_range, a.step, a.n_samples};
    rl.n_samples = ray_count_samples(rl, a.n_samples, end);  // the ray's own: the march and the jump stop there
    Neigh nb = neigh_none();  // no workgroup neighbourhood: every block through the table
    nb.shift_limit = m.block_shift_limit;
    // k_raycast's gate with the lane's origin and the ray's own end (ray_skip_absent's rounding argument)
    const float reach = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)) + end * fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
    const bool may_skip = reach < kRaySkipReachVoxels * m.vs;

    bool cached = false, present = false;
    i3 cb = mki3(0, 0, 0);
    bool prev_valid = false;
    float prev_d = 0.f, prev_z = 0.f;
    for (u32 k = 0; k < rl.n_samples;) {
      const float z = ray_z(rl, k);
      const f3 P = ray_point(rl, d, z);
      const i3 v = world_to_voxel(m.vs, P);
      const int ax = v.x < 0 ? -v.x : v.x, ay = v.y < 0 ? -v.y : v.y, az = v.z < 0 ? -v.z : v.z;
      const bool shift = (u32) (ax | ay | az) < (u32) m.block_shift_limit;
      const i3 b = shift ? mki3(v.x >> 3, v.y >> 3, v.z >> 3) : voxel_to_block(v, m.vs);
      if (!cached || b.x != cb.x || b.y != cb.y || b.z != cb.z) {
        cb = b;
        cached = true;
        present = block_val(t, nb, b) != kNbAbsent;
      }
      if (!present) {  // rule 3: invalid, and every sample a jump passes over with it
        prev_valid = false;
        const int m0 = b.x * kBlockSide, m1 = b.y * kBlockSide, m2 = b.z * kBlockSide;
        const int bmax = max(max(max(abs(m0), abs(m0 + kBlockSide - 1)), max(abs(m1), abs(m1 + kBlockSide - 1))), max(abs(m2), abs(m2 + kBlockSide - 1)));
        const u32 next = (may_skip && bmax < m.block_shift_limit) ? ray_skip_absent(rl, d, m.vs, b, k, z) : k + 1;  // <= rl.n_samples
        if (!have_unknown) { have_unknown = true; first_unknown = z; }
        n_unknown += next - k;
        k = next;
        continue;
      }
      float D;
      const bool ok = trilinear(m, t, nb, P, D);
      if (ok && prev_valid && prev_d > 0.f && D <= 0.f && ray_refine(m, t, nb, rl, d, prev_z, prev_d, z, D, range)) {
        hit = true;  // k = K_i: this sample is not counted
        break;
      }
      if (!ok) {
        if (!have_unknown) { have_unknown = true; first_unknown = z; }
        n_unknown++;
      } else if (D > 0.f) {
        n_free++;
      } else {
        inside = true;
      }
      prev_valid = ok;
      prev_d = D;
      prev_z = z;
      ++k;
    }

    if (hit) {
      const f3 P = ray_point(rl, d, range);
      if (out_normals) {  // k_raycast's: central difference over one voxel of the local size
        const float h = get_voxel_size_f(m, t, nb, P);
        float g[3];
        bool ok = true;
#pragma unroll 1
        for (int c = 0; c < 3 && ok; ++c) {
          f3 pp = P, pm = P;
          if (c == 0) { pp.x = P.x + h; pm.x = P.x - h; }
          else if (c == 1) { pp.y = P.y + h; pm.y = P.y - h; }
          else { pp.z = P.z + h; pm.z = P.z - h; }
          float dp, dm;
          ok = trilinear(m, t, nb, pp, dp) && trilinear(m, t, nb, pm, dm);
          g[c] = ok ? dp - dm : 0.f;
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
  }
  out_range[i] = range;
  out_status[i] = (uint8_t) (bad ? MRH_RAY_BAD : (hit ? MRH_RAY_HIT : 0u) | (n_unknown ? MRH_RAY_UNKNOWN : 0u) | (inside ? MRH_RAY_INSIDE : 0u));
  if (out_normals) {
    out_normals[3 * i + 0] = n[0];
    out_normals[3 * i + 1] = n[1];
    out_normals[3 * i + 2] = n[2];
  }
  if (out_rgb) {
    out_rgb[3 * i + 0] = (uint8_t) (rgbw & 0xFF);
    out_rgb[3 * i + 1] = (uint8_t) ((rgbw >> 8) & 0xFF);
    out_rgb[3 * i + 2] = (uint8_t) ((rgbw >> 16) & 0xFF);
  }
  if (out_counts) {
    out_counts[2 * i + 0] = n_free;
    out_counts[2 * i + 1] = n_unknown;
  }
  if (out_first) out_first[i] = first_unknown;
}

}  // namespace mrh
