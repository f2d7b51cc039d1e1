// mrh_align.h — map-to-map registration: the linearisation of SDF-to-SDF alignment between two maps (include/mrhash_align.h;
// DESIGN.md §4.14 and D19, which is normative; tests/align_ref.py restates it).  The reference has no registration: the
// definition is this project's.  The destination's field is D17's SMOOTH field with its analytic gradient (smooth_field,
// mrh_query.h), the fixed-point step, the sums and their reduction the tracker's (track_fix, track_reduce_store, k_track_finish,
// mrh_track.h), the loop, the solve and the pose update the host's (mrh_tracksolve.h); all are used as they stand.
//
// k_align_gather<EMIT>   one 512-lane workgroup per live source block (Tab::compact[0, n_src), the kSelAll selection; grid-stride),
//                        one lane per stored voxel (a coarse block uses 64): the pose-independent gates of D19.  EMIT = false
//                        counts the accepted cells of the block and takes their integer box; the chained scan
//                        (k_tile_sums_u64 / k_tile_scan_u64, mrh_sort.h) turns the counts into positions; EMIT = true applies
//                        the same gates again and writes the block's samples, ballot-compacted, as 16-byte (P.x, P.y, P.z, s)
//                        records from its position on.  No atomics: the list is in source-block order, voxel order inside a
//                        block, and the sums do not depend on it anyway.
// k_align_box            one workgroup: the blocks' boxes into one, for the automatic pivot and extent
// k_align_linearise      one lane per sample, 256-lane workgroups, one 16-byte load per lane; steps 1-7 of D19 in registers
//                        (binary32, no FMA contraction), then track_reduce_store into the partial slab.  Neighbouring lanes hold
//                        neighbouring voxels of one source block, so their gathers meet in a few destination blocks.
// All of them only read the maps: plain vector loads and stores, every loop bounded.
//
// Bounds of the sums, at most 2^26 samples: |J~| < 2^15, so |J~ J~| < 2^30 and the 21 sums stay below 2^56; |e~| <= 2^18 (|e| <=
// dist_max <= 1), |J~ e~| < 2^33, the 6 sums below 2^59; e~^2 <= 2^36, its sum below 2^62.  All fit a signed 64-bit word.
#pragma once

#include <climits>

#include "mrh_query.h"
#include "mrh_readerplan.h"  // AlignGather, AlignLin
#include "mrh_track.h"

namespace mrh {

constexpr int kAlignGatherLanes = 512;  // one lane per voxel of a fine block
constexpr int kAlignLanes = 256;        // four wave64s: what track_reduce_store reduces

// the cell of lane `v` of the block `ent` (compact entry): accepted under the pose-independent gates?  vox: its integer voxel
// coordinate 8 b + k l, smp: (P, s)
__device__ __forceinline__ bool align_cell(const Tab& t, const AlignGather& g, const int4 ent, const int v, i3& vox, float4& smp) {
  const u32 val = (u32) ent.w;
  const bool coarse = (val & kValCoarseBit) != 0;
  if (v >= (coarse ? kCoarseVoxels : kBlockSide * kBlockSide * kBlockSide)) return false;
  const int bits = coarse ? 2 : 3, k = coarse ? 2 : 1, mask = (1 << bits) - 1;  // the dense index of voxel_local_index
  vox = mki3(ent.x * kBlockSide + k * (v & mask), ent.y * kBlockSide + k * ((v >> bits) & mask), ent.z * kBlockSide + k * (v >> (2 * bits)));
  const VoxPtr vp = vox_ptr(t, val);
  const float s = vp.sdf[v];
  const u32 w = vp.rgbw[v] >> 24;
  const f3 P = voxel_to_world(g.vs_s, vox);
  smp = make_float4(P.x, P.y, P.z, s);
  bool ok = w >= g.w_min && fabsf(s) < g.band;  // a NaN fails
  if (g.crop) ok = ok && fabsf(P.x - g.c[0]) <= g.extent && fabsf(P.y - g.c[1]) <= g.extent && fabsf(P.z - g.c[2]) <= g.extent;
  return ok;
}

// EMIT = false: counts[e] = accepted cells of block e, boxes[2 e], boxes[2 e + 1] = (lo, hi) of their voxel coordinates (INT_MAX,
// INT_MIN when there is none).  EMIT = true: the samples of block e to samples[pos[e] ..), nothing at or beyond `cap`
template <bool EMIT>
__global__ __launch_bounds__(kAlignGatherLanes) void k_align_gather(const Tab t, const AlignGather g, const u32 n_src, u64* __restrict__ counts,
                                                                    int4* __restrict__ boxes, const u64* __restrict__ pos, float4* __restrict__ samples,
                                                                    const u64 cap) {
  constexpr int kWaves = kAlignGatherLanes / 64;
  __shared__ int s_part[kWaves][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u32 e = blockIdx.x; e < n_src; e += gridDim.x) {
    i3 vox = mki3(0, 0, 0);
    float4 smp = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool ok = align_cell(t, g, t.compact[e], (int) threadIdx.x, vox, smp);
    const u64 ballot = __ballot(ok);
    if (EMIT) {
      if (lane == 0) s_part[wave][0] = __popcll(ballot);
      __syncthreads();
      u64 at = pos[e];
      for (int w = 0; w < wave; ++w) at += (u64) s_part[w][0];
      at += (u64) __popcll(ballot & lanemask_lt());
      if (ok && at < cap) samples[at] = smp;
    } else {
      int lo[3] = {ok ? vox.x : INT_MAX, ok ? vox.y : INT_MAX, ok ? vox.z : INT_MAX};
      int hi[3] = {ok ? vox.x : INT_MIN, ok ? vox.y : INT_MIN, ok ? vox.z : INT_MIN};
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          lo[a] = min(lo[a], __shfl_xor(lo[a], off));
          hi[a] = max(hi[a], __shfl_xor(hi[a], off));
        }
      if (lane == 0) {
        s_part[wave][0] = __popcll(ballot);
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_part[wave][1 + a] = lo[a]; s_part[wave][4 + a] = hi[a]; }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        int r[7] = {0, INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
        for (int w = 0; w < kWaves; ++w) {
          r[0] += s_part[w][0];
          for (int a = 0; a < 3; ++a) { r[1 + a] = min(r[1 + a], s_part[w][1 + a]); r[4 + a] = max(r[4 + a], s_part[w][4 + a]); }
        }
        counts[e] = (u64) r[0];
        boxes[2 * (size_t) e] = make_int4(r[1], r[2], r[3], 0);
        boxes[2 * (size_t) e + 1] = make_int4(r[4], r[5], r[6], 0);
      }
    }
    __syncthreads();  // every lane is done with s_part before the next block
  }
}

// one workgroup of 1024: out[0] = lo, out[1] = hi over the n blocks' boxes (the sentinels of empty blocks are neutral)
__global__ __launch_bounds__(1024) void k_align_box(const int4* __restrict__ boxes, const u32 n, int4* __restrict__ out) {
  __shared__ int s_part[16][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int r[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
  for (u32 e = threadIdx.x; e < n; e += 1024u) {
    const int4 lo = boxes[2 * (size_t) e], hi = boxes[2 * (size_t) e + 1];
    r[0] = min(r[0], lo.x); r[1] = min(r[1], lo.y); r[2] = min(r[2], lo.z);
    r[3] = max(r[3], hi.x); r[4] = max(r[4], hi.y); r[5] = max(r[5], hi.z);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r[a] = min(r[a], __shfl_xor(r[a], off));
      r[3 + a] = max(r[3 + a], __shfl_xor(r[3 + a], off));
    }
  if (lane == 0)
#pragma unroll
    for (int a = 0; a < 6; ++a) s_part[wave][a] = r[a];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w)
      for (int a = 0; a < 3; ++a) { r[a] = min(r[a], s_part[w][a]); r[3 + a] = max(r[3 + a], s_part[w][3 + a]); }
    out[0] = make_int4(r[0], r[1], r[2], 0);
    out[1] = make_int4(r[3], r[4], r[5], 0);
  }
}

// steps 1-7 of D19 for one sample (P, s) against the destination map (m, t).  False: rejected.
__device__ __forceinline__ bool align_sample(const Map& m, const Tab& t, const AlignLin& k, const float4 smp, int J[6], int& e_fix) {
  const f3 a = track_rows(k.R, smp.x - k.c[0], smp.y - k.c[1], smp.z - k.c[2]);
  const f3 W = mk3(a.x + k.tau[0], a.y + k.tau[1], a.z + k.tau[2]);
  if (!(fabsf(W.x) < k.bound && fabsf(W.y) < k.bound && fabsf(W.z) < k.bound)) return false;  // NaN and Inf fail; before any conversion
  Neigh nb = neigh_none();
  nb.shift_limit = m.block_shift_limit;
  const float h = get_voxel_size_f(m, t, nb, W);
  float d = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  if (!smooth_field(m, t, nb, W, h, true, d, gx, gy, gz)) return false;
  if (!(fabsf(d) < k.band)) return false;
  const float e = smp.w - d;
  if (!(fabsf(e) <= k.dist_max)) return false;
  const float Jf[6] = {(a.y * gz - a.z * gy) * k.s_a, (a.z * gx - a.x * gz) * k.s_a, (a.x * gy - a.y * gx) * k.s_a,
                       gx * mrh_track::kJOne, gy * mrh_track::kJOne, gz * mrh_track::kJOne};
  return track_fix(Jf, e, J, e_fix);
}

// one lane per sample, a 1-D grid of ceil(n / 256) workgroups, each of which writes one row of the partial slab
__global__ __launch_bounds__(kAlignLanes) void k_align_linearise(const Map m, const Tab t, const AlignLin k, const float4* __restrict__ samples,
                                                                 i64* __restrict__ slab) {
  const u32 i = blockIdx.x * (u32) kAlignLanes + threadIdx.x;
  int J[6] = {0, 0, 0, 0, 0, 0}, e = 0;
  bool ok = i < k.n;
  if (ok) ok = align_sample(m, t, k, samples[i], J, e);
  track_reduce_store(J, e, ok, slab);
}

}  // namespace mrh
