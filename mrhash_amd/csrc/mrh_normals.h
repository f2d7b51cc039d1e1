// mrh_normals.h — one surface normal per point of a LiDAR scan, estimated on the device (include/mrhash_normals.h; DESIGN.md
// §4.6 and D12).
//
// Reference: GeoWrapper::setPointCloud with compute_normals (geowrapper.cpp:374-404) takes the smallest eigenvector of a
// MAD-tree leaf (mad_tree.cpp) of at most b_max = 0.4 m and turns it towards the sensor.  What is kept from it is its nature — one
// plane per small neighbourhood, shared by the points in it, oriented per point —, its leaf size and its orientation rule; the
// neighbourhood (a cell of side rho and the 26 around it), the arithmetic and the gate are this project's definition D12,
// restated in numpy by tests/normals_ref.py.
//
// Four launches per scan, nothing else: k_normals_accumulate (a lane per point: cell key, local coordinate, ten exact integer
// sums per cell in an open-address table of the feature's own), k_normals_solve (64 occupied cells a workgroup: 16 lanes gather
// the 27 cells around each, then a lane per cell: fp64 covariance, Jacobi, gate), k_normals_assign (a lane per point: orient or
// fall back, 12 bytes out, the counts per workgroup) and k_normals_sweep (the occupied slots only: the table is left empty for the
// next scan, so no scan pays for clearing slots it never touched; the counts of the scan).  Integer sums are order-independent,
// everything after them is a function of the sums: the result does not depend on the order of the points or on which lane wins
// a slot.
#pragma once

#include "mrh_device.h"
#include "mrh_readerplan.h"  // NrmPar

namespace mrh {

constexpr u64 kNrmEmpty = ~0ull;             // a free slot of the cell table (a key has 63 bits)
constexpr u32 kNrmMissing = 0xFFFFFFFFu;     // NrmTab::pt_slot of a missing return
constexpr u32 kNrmFallback = 0xFFFFFFFEu;    // ... of a point outside the key range
constexpr int kNrmSums = 10;                 // n, sum u (3), upper triangle of sum u u^T (xx xy xz yy yz zz)
constexpr int kNrmSweeps = 8;                // cyclic Jacobi sweeps (D12 step 6)
constexpr int kNrmCellBias = 1 << 20;        // a cell coordinate c, |c| < 2^20, is stored as c + 2^20 in 21 bits
enum NrmCounter { NC_ESTIMATED = 0, NC_FALLBACK = 1, NC_MISSING = 2, NC_CELLS = 3, NC_N = 4 };

struct NrmTab {
  u64* keys;      // [mask + 1]  packed cell coordinate, kNrmEmpty = free
  u64* sums;      // [mask + 1][kNrmSums]
  float4* cell;   // [mask + 1]  {cell normal, 1 = estimated / 0 = fallback}: written by k_normals_solve for every occupied slot
  u32* list;      // the occupied slots, in the order they were claimed
  u32* pt_slot;   // per point: its cell's slot, kNrmMissing or kNrmFallback
  u32* partial;   // per workgroup of k_normals_assign: its estimated / fallback / missing points
  u64* ctr;       // NC_N counters of THIS scan
  u64* ctr_next;  // ... of the next one: zeroed by k_normals_sweep
  u32 mask;
};

__device__ __forceinline__ u32 nrm_hash(const u64 key, const u32 mask) {
  u64 k = key;
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33;
  return (u32) k & mask;
}

// D12 step 1: ||p|| as step 8 computes it; a point is a return iff that is a positive finite number
__device__ __forceinline__ float nrm_range(const float x, const float y, const float z) { return sqrtf(x * x + y * y + z * z); }

// D12 step 2.  false: a cell coordinate outside +-2^20 (the point takes the fallback)
__device__ __forceinline__ bool nrm_cell_of(const float rho, const float p[3], u64* key, u32 u[3]) {
  u64 k = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float s = p[a] / rho;
    const float c = floorf(s);
    if (!(fabsf(c) < 1048576.f)) return false;
    const int ui = (int) floorf((s - c) * 1024.f);
    u[a] = (u32) (ui < 1023 ? ui : 1023);
    k |= (u64) ((int) c + kNrmCellBias) << (21 * a);
  }
  *key = k;
  return true;
}

// FOLD: runs of consecutive lanes with one key are summed inside the wave, and the run's first lane alone goes to memory — the
// neighbours of an organised scan share cells (up to several hundred points each), so most of a wave's 640 atomics would hit a
// handful of addresses.  FOLD = false (MRH_NORMALS_FOLD=0) is the plain variant: every point adds its own ten sums.
template <bool FOLD>
__global__ __launch_bounds__(256) void k_normals_accumulate(const NrmTab t, const NrmPar par, const float* __restrict__ xyz, const u32 n) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  const u32 lane = threadIdx.x & 63u;
  u64 key = kNrmEmpty;
  u32 u[3] = {0, 0, 0};
  u32 slot = kNrmMissing;
  if (i < n) {
    const float p[3] = {xyz[3 * (size_t) i], xyz[3 * (size_t) i + 1], xyz[3 * (size_t) i + 2]};
    const float r = nrm_range(p[0], p[1], p[2]);
    if (r > 0.f && r < INFINITY) {
      slot = kNrmFallback;
      if (!nrm_cell_of(par.rho, p, &key, u)) key = kNrmEmpty;
    }
  }
  const bool valid = key != kNrmEmpty;
  u32 v[9] = {u[0], u[1], u[2], u[0] * u[0], u[0] * u[1], u[0] * u[2], u[1] * u[1], u[1] * u[2], u[2] * u[2]};
  u32 cnt = 1;
  bool head = valid;  // this lane takes its (run's) sums to memory
  u32 start = lane;
  if (FOLD) {
    const u32 klo = (u32) key, khi = (u32) (key >> 32);
    const u32 plo = __shfl_up(klo, 1), phi = __shfl_up(khi, 1);
    const bool first = lane == 0 || plo != klo || phi != khi;
    const u64 firsts = __ballot(first);
    const u64 above = lane == 63 ? 0ull : firsts >> (lane + 1);
    const u32 end = above ? lane + (u32) __ffsll((long long) above) - 1u : 63u;      // last lane of this lane's run
    start = 63u - (u32) __clzll((long long) (firsts & (~0ull >> (63u - lane))));      // ... and its first (bit 0 is always set)
    // a 64-lane sum of values below 2^20 fits 32 bits
#pragma unroll
    for (u32 step = 1; step < 64; step <<= 1) {
      const bool take = lane + step <= end;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const u32 o = __shfl_down(v[k], step);
        if (take) v[k] += o;
      }
    }
    cnt = end - lane + 1;
    head = valid && first;
  }
  bool claimed = false;
  if (head) {
    u32 s = nrm_hash(key, t.mask);
    bool found = false;
    for (u32 it = 0; it <= t.mask; ++it) {  // the table is at most half full: ends at the key or at a free slot
      u64 cur = *(volatile const u64*) &t.keys[s];
      if (cur == kNrmEmpty) {
        cur = atomicCAS(&t.keys[s], kNrmEmpty, key);
        if (cur == kNrmEmpty) { claimed = true; found = true; break; }
      }
      if (cur == key) { found = true; break; }
      s = (s + 1) & t.mask;
    }
    if (found) {
      slot = s;
      u64* const q = t.sums + (size_t) s * kNrmSums;
      atomicAdd(&q[0], (u64) cnt);
#pragma unroll
      for (int k = 0; k < 9; ++k) atomicAdd(&q[1 + k], (u64) v[k]);
    }
  }
  if (FOLD) {
    const u32 hs = __shfl(slot, start);  // the run's slot (or kNrmFallback if its first lane found none)
    if (valid) slot = hs;
  }
  // the slots claimed by this workgroup join the list of occupied cells: one counter update per workgroup (every update of that
  // one address takes its turn in the L2: one per wave was 2 048 turns a scan)
  __shared__ u32 s_claims[4], s_base;
  const u32 wave = threadIdx.x >> 6;
  const u64 cm = __ballot(claimed);
  if (lane == 0) s_claims[wave] = (u32) __popcll(cm);
  __syncthreads();
  if (threadIdx.x == 0) {
    const u32 total = s_claims[0] + s_claims[1] + s_claims[2] + s_claims[3];
    s_base = total ? (u32) atomicAdd(&t.ctr[NC_CELLS], (u64) total) : 0u;
  }
  __syncthreads();
  if (claimed) {
    u32 at = s_base + (u32) __popcll(cm & ((1ull << lane) - 1ull));
    for (u32 w = 0; w < wave; ++w) at += s_claims[w];
    t.list[at] = slot;
  }
  if (i < n) t.pt_slot[i] = slot;
}

// One Jacobi rotation of the symmetric A on the pair (P, Q), R the third index; V collects the rotations (D12 step 6)
template <int P, int Q, int R>
__device__ __forceinline__ void nrm_rotate(double A[3][3], double V[3][3]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0);
  const double s = tt * c;
  A[P][P] = A[P][P] - tt * apq;
  A[Q][Q] = A[Q][Q] + tt * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
}

// A workgroup takes kNrmSolveCells occupied cells at a time.  Gather: 16 lanes per cell, two neighbours each at most — a table
// probe and 80 bytes of sums, shifted into the cell's coordinate — summed over the 16 lanes in exact integers.  Solve: the
// workgroup's first wave, a cell per lane: covariance, Jacobi, gate.  The Jacobi is one dependent chain of some 8 000 binary64
// instructions (24 rotations of three divisions and two square roots each), 17 us whatever else happens, so the kernel is laid
// out for ONE such chain per scan: 64 cells a workgroup, hence a full wave in the chain and few enough workgroups (321 for the
// 20 521 cells of a 128 x 1024 scan) to be resident all at once.
constexpr int kNrmSolveCells = 64;

// the sum of v over 16 neighbouring lanes, in every one of them
__device__ __forceinline__ long long nrm_sum16(long long v) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const u32 lo = __shfl_xor((u32) (u64) v, off, 16), hi = __shfl_xor((u32) ((u64) v >> 32), off, 16);
    v += (long long) ((u64) hi << 32 | lo);
  }
  return v;
}

__global__ __launch_bounds__(1024) void k_normals_solve(const NrmTab t, const NrmPar par) {
  __shared__ long long s_sum[kNrmSolveCells][kNrmSums];
  const u32 ncells = (u32) t.ctr[NC_CELLS];
  const u32 group = threadIdx.x >> 4, sub = threadIdx.x & 15u;
  for (u32 base = blockIdx.x * kNrmSolveCells; base < ncells; base += gridDim.x * kNrmSolveCells) {  // uniform over the workgroup
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0, a9 = 0;  // N, S (3), Q (xx xy xz yy yz zz): named, so that they stay in registers
    const u32 j = base + group;
    if (j < ncells) {
      const u64 key = t.keys[t.list[j]];
      for (u32 nb = sub; nb < 27u; nb += 16u) {
        const int dx = (int) (nb % 3u) - 1, dy = (int) (nb / 3u % 3u) - 1, dz = (int) (nb / 9u) - 1;
        const int x = (int) (key & 0x1FFFFFu) + dx, y = (int) ((key >> 21) & 0x1FFFFFu) + dy, z = (int) ((key >> 42) & 0x1FFFFFu) + dz;
        if ((u32) x >= (1u << 21) || (u32) y >= (1u << 21) || (u32) z >= (1u << 21)) continue;  // no point can have such a cell
        const u64 nk = (u64) x | (u64) y << 21 | (u64) z << 42;
        u32 s = nrm_hash(nk, t.mask);
        bool found = false;
        for (u32 it = 0; it <= t.mask; ++it) {
          const u64 cur = t.keys[s];
          if (cur == nk) { found = true; break; }
          if (cur == kNrmEmpty) break;
          s = (s + 1) & t.mask;
        }
        if (!found) continue;
        const long long* const q = (const long long*) (t.sums + (size_t) s * kNrmSums);
        const long long m = q[0], sx = q[1], sy = q[2], sz = q[3];
        const long long ax = 1024 * dx, ay = 1024 * dy, az = 1024 * dz;  // u' = u + a: the neighbour's points in this cell's coordinate
        a0 += m;
        a1 += sx + m * ax; a2 += sy + m * ay; a3 += sz + m * az;
        a4 += q[4] + 2 * sx * ax + m * ax * ax;
        a5 += q[5] + sx * ay + ax * sy + m * ax * ay;
        a6 += q[6] + sx * az + ax * sz + m * ax * az;
        a7 += q[7] + 2 * sy * ay + m * ay * ay;
        a8 += q[8] + sy * az + ay * sz + m * ay * az;
        a9 += q[9] + 2 * sz * az + m * az * az;
      }
    }
    a0 = nrm_sum16(a0); a1 = nrm_sum16(a1); a2 = nrm_sum16(a2); a3 = nrm_sum16(a3); a4 = nrm_sum16(a4);
    a5 = nrm_sum16(a5); a6 = nrm_sum16(a6); a7 = nrm_sum16(a7); a8 = nrm_sum16(a8); a9 = nrm_sum16(a9);
    if (sub == 0) {
      long long* const o = s_sum[group];
      o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = a4; o[5] = a5; o[6] = a6; o[7] = a7; o[8] = a8; o[9] = a9;
    }
    __syncthreads();
    if (threadIdx.x < (u32) kNrmSolveCells && base + threadIdx.x < ncells) {
      const long long* const c = s_sum[threadIdx.x];
      const long long N = c[0];
      // covariance x N^2 from exact integers, then one division per entry (D12 step 5): a coordinate that all points share gives
      // a row of exact zeros, since N Q_ij and S_i S_j are then roundings of one and the same integer
      const double Nd = (double) N, NN = Nd * Nd;
      const double Sd[3] = {(double) c[1], (double) c[2], (double) c[3]};
      double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
      A[0][0] = (Nd * (double) c[4] - Sd[0] * Sd[0]) / NN;
      A[0][1] = A[1][0] = (Nd * (double) c[5] - Sd[0] * Sd[1]) / NN;
      A[0][2] = A[2][0] = (Nd * (double) c[6] - Sd[0] * Sd[2]) / NN;
      A[1][1] = (Nd * (double) c[7] - Sd[1] * Sd[1]) / NN;
      A[1][2] = A[2][1] = (Nd * (double) c[8] - Sd[1] * Sd[2]) / NN;
      A[2][2] = (Nd * (double) c[9] - Sd[2] * Sd[2]) / NN;
      for (int sweep = 0; sweep < kNrmSweeps; ++sweep) {
        nrm_rotate<0, 1, 2>(A, V);
        nrm_rotate<0, 2, 1>(A, V);
        nrm_rotate<1, 2, 0>(A, V);
      }
      // ascending by (value, index): the smallest eigenvalue l0 with its vector, l1 the value of the middle one.  Selected with
      // constant indices only: one index computed at run time would move A and V from registers to scratch memory
      double l0 = A[0][0], nx = V[0][0], ny = V[1][0], nz = V[2][0];
      int i0 = 0;
      if (A[1][1] < l0) { l0 = A[1][1]; nx = V[0][1]; ny = V[1][1]; nz = V[2][1]; i0 = 1; }
      if (A[2][2] < l0) { l0 = A[2][2]; nx = V[0][2]; ny = V[1][2]; nz = V[2][2]; i0 = 2; }
      const double la = i0 == 0 ? A[1][1] : A[0][0], lb = i0 == 2 ? A[1][1] : A[2][2];
      const double l1 = la < lb ? la : lb;
      const bool est = N >= (long long) par.min_points && l1 >= par.min_l1 && l0 <= par.max_flat * l1;
      t.cell[t.list[base + threadIdx.x]] = make_float4((float) nx, (float) ny, (float) nz, est ? 1.f : 0.f);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_normals_assign(const NrmTab t, const float* __restrict__ xyz, const u32 n, float* __restrict__ out) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  int kind = -1;  // NC_ESTIMATED / NC_FALLBACK / NC_MISSING
  if (i < n) {
    const u32 slot = t.pt_slot[i];
    const float x = xyz[3 * (size_t) i], y = xyz[3 * (size_t) i + 1], z = xyz[3 * (size_t) i + 2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    kind = NC_MISSING;
    if (slot != kNrmMissing) {
      float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
      if (slot != kNrmFallback) c = t.cell[slot];
      if (c.w != 0.f) {
        kind = NC_ESTIMATED;
        const bool away = c.x * x + c.y * y + c.z * z > 0.f;
        nx = away ? -c.x : c.x; ny = away ? -c.y : c.y; nz = away ? -c.z : c.z;
      } else {
        kind = NC_FALLBACK;  // the reversed beam
        const float r = nrm_range(x, y, z);
        nx = -(x / r); ny = -(y / r); nz = -(z / r);
      }
    }
    out[3 * (size_t) i] = nx; out[3 * (size_t) i + 1] = ny; out[3 * (size_t) i + 2] = nz;
  }
  // the three counts of this workgroup; k_normals_sweep adds the workgroups up (6 144 updates of three addresses, one per wave
  // and count, took their turns in the L2 for 33 of this kernel's 39 us)
  __shared__ u32 s_count[3];
  if (threadIdx.x < 3) s_count[threadIdx.x] = 0;
  __syncthreads();
  const u32 lane = threadIdx.x & 63u;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const u64 m = __ballot(kind == k);
    if (m && lane == 0) atomicAdd(&s_count[k], (u32) __popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < 3) t.partial[3 * blockIdx.x + threadIdx.x] = s_count[threadIdx.x];
}

// Leaves the table as the next scan expects it: the occupied slots free, their sums zero, the next scan's counters zero.  This
// scan's counters stay (mrh_normals_info is read from them); its first workgroup completes them.
__global__ __launch_bounds__(256) void k_normals_sweep(const NrmTab t, const u32 assign_wgs) {
  const u32 ncells = (u32) t.ctr[NC_CELLS];
  // a lane per 8-byte word, so that the ten words of a cell are written by ten neighbouring lanes
  const u64 words = (u64) ncells * kNrmSums;
  for (u64 e = (u64) blockIdx.x * 256u + threadIdx.x; e < words; e += (u64) gridDim.x * 256u) {
    const u32 slot = t.list[(u32) (e / kNrmSums)], k = (u32) (e % kNrmSums);
    t.sums[(size_t) slot * kNrmSums + k] = 0;
    if (k == 0) t.keys[slot] = kNrmEmpty;
  }
  if (blockIdx.x == 0) {  // ... and the per-point counts of this scan: the sum of k_normals_assign's workgroups
    __shared__ u32 s_count[3];
    if (threadIdx.x < 3) s_count[threadIdx.x] = 0;
    __syncthreads();
    u32 a[3] = {0, 0, 0};
    for (u32 b = threadIdx.x; b < assign_wgs; b += 256u) { a[0] += t.partial[3 * b]; a[1] += t.partial[3 * b + 1]; a[2] += t.partial[3 * b + 2]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&s_count[k], a[k]);
    __syncthreads();
    if (threadIdx.x < 3) t.ctr[threadIdx.x] = s_count[threadIdx.x];
    if (threadIdx.x < NC_N) t.ctr_next[threadIdx.x] = 0;
  }
}

}  // namespace mrh
