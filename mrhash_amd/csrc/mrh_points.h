// mrh_points.h — the host side of LiDAR scans behind the C ABI: the cloud and its layout (mrh_upload_points, mrh_set_points_device,
// mrh_upload_normals, mrh_set_scan_layout / mrh_detect_scan_layout) and mrh_integrate_points, a driver over named stages that
// takes a scan through one of two record paths — the voxel buckets (kernels in mrh_scan.h) or, where their scratch does not fit,
// the voxel ids need 64-bit keys, a beam is too long or MRH_LIDAR_BUCKETS=0 says so, the sorted records (kernels in mrh_lidar.h,
// the sort in mrh_sort.h).  At the end, the normals of a scan: mrh_estimate_normals[_device] and mrh_get_normals (kernels in
// mrh_normals.h, the argument plan in mrh_readerplan.h).  The state is mrh_ctx::lidar, the normals' scratch and counts mrh_ctx::nrm.
// Included by mrh_capi.hip, same translation unit: it needs the context's internals (mrh_ctx, HIP_TRY, fail, dev_alloc, pinned_alloc,
// regrow / regrow_all / regrow_pinned, ensure_device, ensure_ready, launch_compact_all, mark_frame and, from mrh_frame.h,
// frame_upkeep, refill_coarse, plan_begin, starve_and_tail).
#pragma once

namespace {

// Is this cloud an organised scan — rows of L points each, row-major, neighbours in the array neighbours in direction both along a
// row and from one row to the next?  A few dozen point pairs decide: the candidate L (a power of two that leaves a multiple of 16
// rows) whose points i and i + L lie closest in direction, if that and the step to i + 1 are within a few degrees.  Only a hint
// for the order in which k_scan_walk takes the beams (mrh_scan.h: Scan::patch_log2): a wrong answer costs time, never a bit.
int detect_scan_row_len(const float* xyz, const uint64_t n) {
  if (n < 4096 || n % 256) return 0;
  auto cos_between = [&](uint64_t a, uint64_t b, double* out) {
    const float *p = xyz + 3 * a, *q = xyz + 3 * b;
    const double pp = (double) p[0] * p[0] + (double) p[1] * p[1] + (double) p[2] * p[2], qq = (double) q[0] * q[0] + (double) q[1] * q[1] + (double) q[2] * q[2];
    if (!(pp > 0.0) || !(qq > 0.0)) return false;  // a missing return
    *out = ((double) p[0] * q[0] + (double) p[1] * q[1] + (double) p[2] * q[2]) / std::sqrt(pp * qq);
    return true;
  };
  constexpr int kSamples = 96;
  const double cos_limit = 0.99756;  // 4 degrees (a 16-beam sensor's rows are 2-3 degrees apart)
  int best = 0;
  double best_cos = cos_limit;
  for (uint64_t L = 16; L <= 8192 && L * 16 <= n; L <<= 1) {
    if (n % L || (n / L) % 16) continue;
    double sum_row = 0.0, sum_next = 0.0;
    int ok = 0;
    for (int k = 0; k < kSamples; k++) {
      const uint64_t i = (uint64_t) ((double) k * (double) (n - L - 2) / kSamples);
      double a, b;
      if ((i % L) + 1 < L && cos_between(i, i + 1, &a) && cos_between(i, i + L, &b)) { sum_next += a; sum_row += b; ok++; }
    }
    if (ok < kSamples / 4) continue;
    if (sum_next / ok > cos_limit && sum_row / ok > best_cos) { best_cos = sum_row / ok; best = (int) L; }
  }
  return best;
}

// what the three calls that hand over a cloud or its normals reject
int cloud_checks(mrh_ctx* c, const char* who, const float* xyz, const uint64_t n) {
  const int rc = ensure_ready(c, who);
  if (rc) return rc;
  if (n && !xyz) return fail(c, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  return MRH_OK;
}

// n x 3 floats of the host into the context's own grow-only buffer `d`; blocking.  `num` says how many of them are valid: none
// from the moment the buffer may change until the copy has landed.
int upload_xyz(mrh_ctx* c, const float* xyz, const uint64_t n, float*& d, size_t& cap, size_t& num) {
  num = 0;
  const int rc = regrow(c, d, cap, (size_t) n, (size_t) n * 3 * sizeof(float));
  if (rc) return rc;
  if (n) HIP_TRY(c, hipMemcpyAsync(d, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's buffer is free on return (GeoWrapper::setPointCloud copies)
  num = n;
  return MRH_OK;
}

}  // namespace

extern "C" {

int mrh_detect_scan_layout(const float* xyz, uint64_t n) { return xyz ? detect_scan_row_len(xyz, n) : 0; }

int mrh_set_scan_layout(mrh_ctx* c, int row_len) {
  if (!c) return MRH_ERR_INVALID_ARG;
  c->lidar.layout_hint = row_len;
  c->lidar.row_len = row_len > 0 ? row_len : 0;
  c->lidar.detect_n = 0;
  return MRH_OK;
}

int mrh_upload_points(mrh_ctx* c, const float* xyz, uint64_t n) {
  int rc = cloud_checks(c, "mrh_upload_points", xyz, n);
  if (rc) return rc;
  auto& L = c->lidar;
  L.d_points_cur = nullptr;  // the buffer it may point to is about to be released
  rc = upload_xyz(c, xyz, n, L.d_points, L.points_cap, L.num_points);
  if (rc) return rc;
  L.d_points_cur = L.d_points;
  L.have_cloud = true;
  if (L.layout_hint > 0) L.row_len = L.layout_hint;
  else if (L.layout_hint == 0 && n) {
    if (n != L.detect_n || ++L.detect_age >= 64) {
      L.detect_len = detect_scan_row_len(xyz, n);
      L.detect_n = n;
      L.detect_age = 0;
    }
    L.row_len = L.detect_len;
  } else L.row_len = 0;
  return MRH_OK;
}

int mrh_set_points_device(mrh_ctx* c, const float* d_xyz, uint64_t n) {
  const int rc = cloud_checks(c, "mrh_set_points_device", d_xyz, n);
  if (rc) return rc;
  c->lidar.d_points_cur = d_xyz;
  c->lidar.num_points = n;
  c->lidar.have_cloud = true;
  c->lidar.row_len = c->lidar.layout_hint > 0 ? c->lidar.layout_hint : 0;  // a cloud in device memory is not looked at: mrh_set_scan_layout says how it is laid out
  return MRH_OK;
}

int mrh_upload_normals(mrh_ctx* c, const float* nxyz, uint64_t n) {
  const int rc = cloud_checks(c, "mrh_upload_normals", nxyz, n);
  if (!rc) { c->nrm.info = {}; c->nrm.info_pending = false; }  // these normals were not estimated here (mrh_get_normals)
  return rc ? rc : upload_xyz(c, nxyz, n, c->lidar.d_normals, c->lidar.normals_cap, c->lidar.num_normals);
}

}  // extern "C"

namespace {

// ---- the stages of mrh_integrate_points, in the order the driver runs them ---------------------------------------------------------

// what the call rejects before it touches the device
int points_checks(mrh_ctx* c) {
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_integrate_points: an exchange is pending (call mrh_integrate_resume)");
  if (c->halo_upper) return fail(c, MRH_ERR_STATE, "mrh_integrate_points: halo blocks of other shards are present (call mrh_drop_blocks(MRH_DROP_HALO) after the extraction)");
  if (!c->has_camera) return fail(c, MRH_ERR_STATE, "mrh_integrate_points: set_camera has not been called");
  const uint64_t n = c->lidar.num_points;
  if (!c->p.projective_sdf && c->lidar.num_normals != n)
    return fail(c, MRH_ERR_STATE, "mrh_integrate_points: the normal-direction SDF needs one normal per point (mrh_upload_normals)");
  if (n >= (1ull << 24)) return fail(c, MRH_ERR_CAPACITY, "mrh_integrate_points: %llu points in one scan (limit 2^24 - 1)", (unsigned long long) n);
  return MRH_OK;
}

// An organised scan is taken in 2-D patches of beams (mrh_lidar.h: BeamOrder); its row length: mrh_set_scan_layout, the look at a
// host cloud (mrh_upload_points), or the spherical camera's columns if it has one pixel per point
BeamOrder beam_order(const mrh_ctx* c, const uint64_t n) {
  BeamOrder order;
  order.patch_log2 = 8; order.patches_per_row = 1; order.row_len = 256;
  const auto& L = c->lidar;
  const Cam& k = c->cam;
  const int want = L.patch_log2;
  const uint64_t row_len = L.row_len > 0 ? (uint64_t) L.row_len : (L.layout_hint == 0 && (uint64_t) k.rows * (uint64_t) k.cols == n ? (uint64_t) k.cols : 0);
  if (want < 8 && row_len > 0 && n % row_len == 0 && row_len % (1u << want) == 0 && (n / row_len) % (256u >> want) == 0) {
    order.patch_log2 = (u32) want; order.patches_per_row = (u32) (row_len >> want); order.row_len = (u32) row_len;
  }
  return order;
}

// Everything about one scan that the host can work out before a record exists
struct ScanPlan {
  const float* pts; const float* normals;  // normals: nullptr under the projective SDF
  u32 np, grid;                            // points, walk workgroups of 256
  BeamOrder order;
  uint64_t slots, rec_bound;               // voxels a beam can cross, and the records of the scan that bounds
  int coarse_bit;                          // bits of a voxel id of this pool; coarse units carry one more
  bool wide;                               // ... beyond 32: the sorted path with 64-bit keys
  bool buckets;                            // the voxel buckets take the scan (else the sorted records)
  size_t walk_lds;                         // the buckets' walk kernel: dynamic LDS
  int ord_shift, narrow;                   // ... Scan::ord_shift (5 on variance-adaptive maps), Scan::narrow (8-byte records)
};

void launch_alloc3d(mrh_ctx* c, const ScanPlan& p) {
  const u32 stamp = (u32) ((c->frames + 1) & 0x3FFFFFFFu);
  k_alloc3d<<<p.grid, 256, 0, c->stream>>>(c->cam, c->map, c->tab, c->fast, p.pts, p.normals, p.np, stamp, p.order);
}

int bits_for(const uint64_t max_value) { int b = 1; while (b < 63 && (max_value >> b)) b++; return b; }

// Host arithmetic only.  integrate3D (vds.cu:1215-1410): records of every (point, voxel).  Their buffers are sized by a bound the
// host can compute (a beam crosses at most `slots` voxels), so no pass that writes records needs a count from the host first.
int plan_scan(mrh_ctx* c, ScanPlan* p) {
  const Cam& k = c->cam;
  const Map& m = c->map;
  const uint64_t n = p->np;
  // slots: the voxel-level DDA walks from voxel(p_min) to voxel(p_max), |p_max - p_min| <= 2 tr, tr <= trunc + scale *
  // integration distance: at most sum_axis(|end - start|) + 1 steps <= (2 tr / vs) * sqrt(3) + 3, plus the roundings
  const double tr_max = (double) m.trunc + (double) m.trunc_scale * (double) k.max_int_dist;
  p->slots = std::min<uint64_t>(kMaxDdaIter, (uint64_t) std::floor(2.0 * tr_max / (double) m.vs * 1.7320508) + 10);
  p->rec_bound = n * p->slots;
  if (p->rec_bound >= 0xFFFFFFF0ull) return fail(c, MRH_ERR_CAPACITY, "mrh_integrate_points: %llu points x %llu voxels per beam exceed 2^32 records per scan", (unsigned long long) n, (unsigned long long) p->slots);
  // key width from the pool capacity: voxel id < cap * 512, one more bit for coarse units
  p->coarse_bit = bits_for((uint64_t) c->num_blocks * 512 - 1);
  p->wide = p->coarse_bit + (c->tab.multi_res ? 1 : 0) > 32;
  // voxel buckets (mrh_scan.h) unless the map's voxel ids, the beam length or the memory say otherwise: then the sorted records
  p->buckets = c->lidar.use_buckets && c->lidar.buckets_scratch >= 0 && !p->wide && (uint64_t) c->num_blocks * 512 < 0x7FFFFE00ull &&
               p->slots <= (uint64_t) kScanMaxSlots;
  p->walk_lds = (size_t) (2 * p->slots * 256 + 2 * kScanSetSize) * sizeof(u32);
  p->ord_shift = c->tab.multi_res ? 5 : 0;
  p->narrow = (n << p->ord_shift) <= (1ull << 23) && !getenv("MRH_SCAN_WIDE_RECORDS") ? 1 : 0;  // MRH_SCAN_WIDE_RECORDS=1: tests
  return MRH_OK;
}

// Scratch and buffers of the voxel-bucket scans (mrh_scan.h).  0: ready, 1: not on this context (the sorted path takes over), < 0: error.
int scan_prepare(mrh_ctx* c, const ScanPlan& p) {
  hipStream_t s = c->stream;
  auto& L = c->lidar;
  Scan& sc = L.buckets;
  if (L.buckets_scratch == 0) {
    const size_t nb = (size_t) c->num_blocks;
    bool ok = dev_alloc(c, sc.vcnt, nb * 512 * sizeof(u32)) == hipSuccess;
    ok = ok && dev_alloc(c, sc.bstamp, nb * sizeof(u32)) == hipSuccess;
    ok = ok && dev_alloc(c, L.d_buckets_ctr, 2 * SC_N * sizeof(u32)) == hipSuccess;
    if (!ok) {  // one counter per voxel slot does not fit next to this map
      (void) hipGetLastError();
      (void) dev_free(c, sc.vcnt); (void) dev_free(c, sc.bstamp); (void) dev_free(c, L.d_buckets_ctr);
      L.buckets_scratch = -1;
      return 1;
    }
    HIP_TRY(c, hipMemsetAsync(sc.vcnt, 0, nb * 512 * sizeof(u32), s));
    HIP_TRY(c, hipMemsetAsync(sc.bstamp, 0, nb * sizeof(u32), s));
    HIP_TRY(c, hipMemsetAsync(L.d_buckets_ctr, 0, 2 * SC_N * sizeof(u32), s));
    L.buckets_scratch = 1;
    L.buckets_dirty = false;
  }
  if (L.buckets_dirty) {  // a scan that failed half way leaves counters behind
    HIP_TRY(c, hipMemsetAsync(sc.vcnt, 0, (size_t) c->num_blocks * 512 * sizeof(u32), s));
    HIP_TRY(c, hipMemsetAsync(L.d_buckets_ctr, 0, 2 * SC_N * sizeof(u32), s));
    L.buckets_dirty = false;
  }
  if (p.rec_bound > L.buckets_rec_cap) {
    const size_t cap = (size_t) p.rec_bound;
    // chunks: one per touched block + one per kScanChunkWeight of weight (a record weighs at least 32: <= records / 256, taken as
    // records / 128) + two per run beyond kScanLongRun (the run's own chunk and the cut behind it: <= 2 * records / 65)
    const size_t chunk_cap = std::min<size_t>(c->num_blocks, cap) + cap / 128 + 2 * cap / (kScanLongRun + 1) + 64;
    const int rc = regrow_all(c, L.buckets_rec_cap, cap, {{sc.st_meta, cap * sizeof(uint2)}, {sc.st_sdf, cap * sizeof(float)}, {sc.st_grp, cap * sizeof(uint2)},
                                                           {sc.rec, cap * sizeof(uint4)}, {sc.chunks, chunk_cap * sizeof(uint4)}});
    if (rc) return rc;
    sc.rec_cap = (u32) std::min<size_t>(cap, 0xFFFFFFF0ull);
    sc.chunk_cap = (u32) std::min<size_t>(chunk_cap, 0xFFFFFFF0ull);
  }
  const int rc = regrow(c, sc.wgdesc, L.buckets_wg_cap, (size_t) p.grid, p.grid * sizeof(uint2));
  if (rc) return rc;
  if (p.walk_lds > 65536 && p.walk_lds > L.buckets_lds_set) {
    HIP_TRY(c, hipFuncSetAttribute((const void*) k_scan_walk, hipFuncAttributeMaxDynamicSharedMemorySize, (int) p.walk_lds));
    L.buckets_lds_set = p.walk_lds;
  }
  return 0;
}

// The buffers of the path that takes the scan; turns the plan to the sorted path when the buckets' scratch does not fit here
int scan_buffers(mrh_ctx* c, ScanPlan* p) {
  if (p->buckets) {
    const int rc = scan_prepare(c, *p);
    if (rc < 0) return rc;
    p->buckets = rc == 0;
    if (p->buckets) return MRH_OK;
  }
  auto& L = c->lidar;
  const size_t key_bytes = p->wide ? 8 : 4;
  if (p->rec_bound > L.rec_cap || key_bytes > L.rec_key_bytes) {  // two (key, sdf) buffers under one capacity and one key width
    const size_t cap = std::max<size_t>(p->rec_bound, L.rec_cap), kb = std::max(key_bytes, L.rec_key_bytes);
    L.rec_key_bytes = 0;
    const int rc = regrow_all(c, L.rec_cap, cap, {{L.d_rec_keys[0], cap * kb}, {L.d_rec_vals[0], cap * sizeof(float)},
                                                  {L.d_rec_keys[1], cap * kb}, {L.d_rec_vals[1], cap * sizeof(float)}});
    if (rc) return rc;
    L.rec_key_bytes = kb;
  }
  if (p->np > L.pt_cap) {  // counts per point, one total per count workgroup
    const int rc = regrow_all(c, L.pt_cap, p->np, {{L.d_pt_counts, p->np * sizeof(u32)}, {L.d_pt_offsets, (p->np / 256 + 2) * sizeof(u32)}});
    if (rc) return rc;
  }
  if (!L.h_sorted_report) {
    HIP_TRY(c, pinned_alloc(c, L.h_sorted_report, 4 * sizeof(u32)));
    memset(L.h_sorted_report, 0, 4 * sizeof(u32));
  }
  return MRH_OK;
}

// The scan through the voxel buckets: walk (count per voxel), offsets, place, apply
int scan_buckets(mrh_ctx* c, const ScanPlan& p) {
  hipStream_t s = c->stream;
  const Tab& t = c->tab;
  auto& L = c->lidar;
  Scan sc = L.buckets;
  sc.seq = ++L.buckets_seq;
  if (sc.seq >= 0x80000000u) {  // a block's stamp is seq * 2 + coarse in 32 bits: the sequence restarts at 1 with clean stamps
    HIP_TRY(c, hipMemsetAsync(sc.bstamp, 0, (size_t) c->num_blocks * sizeof(u32), s));
    // ... and with both counter sets at zero: the restart breaks the alternation that lets a scan zero the next one's set
    HIP_TRY(c, hipMemsetAsync(L.d_buckets_ctr, 0, 2 * SC_N * sizeof(u32), s));
    sc.seq = L.buckets_seq = 1;
  }
  sc.ctr = L.d_buckets_ctr + (sc.seq & 1u) * SC_N;
  sc.ctr_next = L.d_buckets_ctr + ((sc.seq + 1u) & 1u) * SC_N;
  sc.ord_shift = p.ord_shift;
  sc.narrow = p.narrow;
  sc.order = p.order;
  k_scan_walk<<<p.grid, 256, p.walk_lds, s>>>(c->cam, c->map, t, p.pts, p.normals, p.np, sc, (int) p.slots);
  // the touched blocks are found by their stamps inside k_scan_offsets, windows of kScanWindow blocks; 512 workgroups walk the
  // windows (2 048 of these 1 024-thread workgroups took 9 us to DISPATCH for ~1 us of work each, tools/trace_scan.py)
  k_scan_offsets<<<std::min<u32>(512u, (u32) ((c->num_blocks + kScanWindow - 1) / kScanWindow)), 1024, 0, s>>>(t, sc, t.multi_res ? (u32) c->num_blocks : 0u);
  k_scan_place<<<p.grid, 256, 0, s>>>(sc, (int) p.slots);
  k_scan_apply<<<1536, 256, 0, s>>>(c->map, t, sc, p.np << sc.ord_shift, c->profile);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// stable radix sort of the scan's (voxel id, sdf) records on key bits [0, end_bit): the padding key (all ones) ends up last,
// equal ids keep their point-major order (mrh_sort.h)
// *out_buf = which of the two buffer pairs holds the sorted records
template <typename K>
int lidar_sort(mrh_ctx* c, K* k0, K* k1, float* v0, float* v1, const size_t n, const int end_bit, int* out_buf) {
  const u32 ntiles = (u32) ((n + kSortTile - 1) / kSortTile);
  const u32 total = 256u * ntiles;
  if (n > 0xFFFFFFFFull - kSortTile || (uint64_t) 256u * ntiles > kSortScanMax)  // records and histogram entries are indexed in 32 bits
    return fail(c, MRH_ERR_CAPACITY, "mrh_integrate_points: %zu records in one scan through the sorted path (limit 2^32 - %d)", n, kSortTile + 1);
  // the scan-sized sort of mrh_sort.h: per 8-bit digit a tile histogram, a one-workgroup scan, a stable scatter
  auto& L = c->lidar;
  if ((size_t) total * sizeof(u32) + 1024 > L.sort_tmp_bytes) {  // grown to twice what is asked for
    const size_t bytes = (size_t) total * sizeof(u32) * 2 + 1024;
    const int rc = regrow_all(c, L.sort_tmp_bytes, bytes, {{L.d_sort_tmp, bytes}});
    if (rc) return rc;
  }
  K* const ks[2] = {k0, k1};
  float* const vs[2] = {v0, v1};
  *out_buf = radix_sort_pairs<K, float>(c->stream, ks, vs, nullptr, n, end_bit, (u32*) L.d_sort_tmp, (u32*) L.d_sort_tmp + 256);  // [0, 256): the digit totals
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// The scan through sorted records, keys of type K: records of every (point, voxel) in point-major order -> stable sort by voxel ->
// fold.  The emit pass needs nothing from the host and runs WHILE the host picks up the scan's one report (record count,
// high-water mark: they size the sort): count -> scan -> report -> emit are enqueued together, the sort and the fold follow the report.
template <typename K>
int scan_sorted(mrh_ctx* c, const ScanPlan& p) {
  hipStream_t s = c->stream;
  const Cam& k = c->cam;
  const Map& m = c->map;
  const Tab& t = c->tab;
  auto& L = c->lidar;
  // the one host round trip of a scan: the emit pass derives its offsets from the per-workgroup totals itself, and its LAST
  // workgroup, which knows the grand total before its walk starts, writes {high-water mark, records} and a sequence mark into
  // pinned memory: the host reads it and enqueues the sort while the emit pass runs
  ScanState ss;
  ss.wg_totals = L.d_pt_offsets; ss.host_rec = L.h_sorted_report; ss.seq = ++L.sorted_seq;
  const u32 seq = ss.seq;
  k_points_walk<false, u32><<<p.grid, 256, 0, s>>>(k, m, t, p.pts, p.normals, p.np, L.d_pt_counts, ss, (u32*) nullptr, nullptr, p.coarse_bit, 0u);
  k_points_walk<true, K><<<p.grid, 256, 0, s>>>(k, m, t, p.pts, p.normals, p.np, L.d_pt_counts, ss, (K*) L.d_rec_keys[0], L.d_rec_vals[0], p.coarse_bit, (u32) std::min<uint64_t>(L.rec_cap, 0xFFFFFFFFull));
  HIP_TRY(c, hipGetLastError());
  {
    volatile u32* mark = L.h_sorted_report + 3;
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    while (*mark != seq) {
      MRH_CPU_RELAX();
      if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;  // long scan or a fault
    }
    if (*mark != seq) HIP_TRY(c, hipStreamSynchronize(s));  // reports a device error if that is why the mark never came
    if (*mark != seq) return fail(c, MRH_ERR_DEVICE, "mrh_integrate_points: the scan report did not arrive");
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  const int hwm = (int) L.h_sorted_report[0];
  const uint64_t n_rec = (uint64_t) L.h_sorted_report[1];
  if (n_rec > p.rec_bound) return fail(c, MRH_ERR_DEVICE, "mrh_integrate_points: %llu records exceed the bound of %llu", (unsigned long long) n_rec, (unsigned long long) p.rec_bound);
  if (n_rec == 0) return MRH_OK;
  // the sort only looks at the bits a voxel id of THIS map can have (the high-water mark of the pool); it is stable, and the
  // records were emitted in point order: every voxel's run ends up in ascending point index (D6)
  const int end_bit = t.multi_res ? p.coarse_bit + 1 : bits_for((uint64_t) (hwm > 0 ? hwm : 1) * 512 - 1);
  const u32 agrid = (u32) ((n_rec + kApplyChunk - 1) / kApplyChunk);
  int sb = 1;
  const int rc = lidar_sort(c, (K*) L.d_rec_keys[0], (K*) L.d_rec_keys[1], L.d_rec_vals[0], L.d_rec_vals[1], (size_t) n_rec, end_bit, &sb);
  if (rc) return rc;
  k_points_apply<K><<<agrid, 256, 0, s>>>(m, t, (const K*) L.d_rec_keys[sb], L.d_rec_vals[sb], (u32) n_rec, p.coarse_bit, c->profile);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

int run_scan(mrh_ctx* c, const ScanPlan& p) {
  if (p.buckets) return scan_buckets(c, p);
  return p.wide ? scan_sorted<u64>(c, p) : scan_sorted<u32>(c, p);
}

// checkVarSDF -> reallocBlocks -> flatAndReduceHashTable(); reintegrate3D then launches integrate3DKernel again (vds.cu:1561-1580):
// the driver runs the whole scan a second time, into fine and coarse blocks alike
int realloc_pass(mrh_ctx* c) {
  hipStream_t s = c->stream;
  const int rc = launch_compact_all(c);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_NREALLOC], 0, 2 * sizeof(int), s));  // NREALLOC, NREINT
  k_check_var<<<2048, 64, 0, s>>>(c->map, c->tab, c->d_realloc);
  k_realloc<<<64, 256, 0, s>>>(c->tab, c->d_realloc, c->d_reint);
  return MRH_OK;
}

}  // namespace

extern "C" {

// VoxelContainer::integrate(point_cloud, ...) voxel_data_structures.cpp:112-135
int mrh_integrate_points(mrh_ctx* c, int n_frames_invalidate) {
  int rc = ensure_ready(c, "mrh_integrate_points");
  if (rc) return rc;
  rc = points_checks(c);
  if (rc) return rc;
  rc = frame_upkeep(c);
  if (rc) return rc;
  FramePlan& plan = c->plan;
  plan_begin(c, plan, FRAME_GENERAL, n_frames_invalidate);  // GC (and the starve step) of a scan run through the general kernels on the list of ALL live blocks
  if (c->tab.multi_res) { c->mr_summaries_valid = false; c->mr_next_general = true; c->refill_flag_valid = false; }
  if (c->lidar.num_points > 0) {
    if (c->tab.multi_res) refill_coarse(c);
    ScanPlan p;
    p.pts = c->lidar.d_points_cur;
    p.normals = c->p.projective_sdf ? nullptr : c->lidar.d_normals;
    p.np = (u32) c->lidar.num_points;
    p.grid = (p.np + 255) / 256;
    p.order = beam_order(c, p.np);
    launch_alloc3d(c, p);  // before anything below can refuse the scan or drain the stream: the allocation runs while the host sizes buffers
    rc = plan_scan(c, &p);
    if (rc) return rc;
    rc = scan_buffers(c, &p);
    if (rc) return rc;
    rc = run_scan(c, p);
    if (rc) return rc;
    if (c->tab.multi_res && c->frames > 0) {
      rc = realloc_pass(c);
      if (rc) return rc;
      rc = run_scan(c, p);
      if (rc) return rc;
    }
  }
  if (plan.max_num_frames > 0) {  // flatAndReduceHashTable() without a camera: every live block (voxel_data_structures.cpp:121, :126)
    rc = launch_compact_all(c);
    if (rc) return rc;
  }
  rc = starve_and_tail(c, plan);  // garbageCollect(camera, max_num_frames); counts the frame
  if (rc < 0) return rc;
  HIP_TRY(c, hipGetLastError());
  if (c->peek_enabled) {
    const int mrc = mark_frame(c);  // pool-level report for mrh_peek_free_blocks
    if (mrc) return mrc;
  }
  return rc;
}

}  // extern "C"

// ---- scan normals (include/mrhash_normals.h; kernels in mrh_normals.h): they act on the cloud above.  State: mrh_ctx::nrm -------------
namespace {

// the parameter block with its defaults filled in, as the kernels take it (mrh_readerplan.h)
int normals_args(mrh_ctx* c, const char* who, const mrh_normals_params* p, const uint64_t n, NrmPar* out) {
  char msg[mrh_plan::kMsgBytes];
  const int rc = mrh_plan::normals(msg, who, p, n, c->p.virtual_voxel_size, out);
  return rc ? fail(c, rc, "%s", msg) : MRH_OK;
}

// scratch for n points: grown to the next power of two, born clean
int normals_scratch(mrh_ctx* c, const uint64_t n) {
  auto& N = c->nrm;
  hipStream_t s = c->stream;
  if (!N.d_ctr) {
    HIP_TRY(c, dev_alloc(c, N.d_ctr, 2 * NC_N * sizeof(u64)));
    HIP_TRY(c, hipMemsetAsync(N.d_ctr, 0, 2 * NC_N * sizeof(u64), s));
  }
  if (n > N.cap) {
    const size_t cap = (size_t) next_pow2(std::max<uint64_t>(n, 512)), slots = 2 * cap;
    NrmTab& t = N.tab;
    const int rc = regrow_all(c, N.cap, cap, {{t.keys, slots * sizeof(u64)}, {t.sums, slots * kNrmSums * sizeof(u64)}, {t.cell, slots * sizeof(float4)},
                                              {t.list, cap * sizeof(u32)}, {t.pt_slot, cap * sizeof(u32)}, {t.partial, (cap / 256 + 1) * 3 * sizeof(u32)}});
    if (rc) return rc;
    t.mask = (u32) (slots - 1);
    N.dirty = true;
  }
  if (N.dirty) {
    const size_t slots = (size_t) N.tab.mask + 1;
    HIP_TRY(c, hipMemsetAsync(N.tab.keys, 0xFF, slots * sizeof(u64), s));
    HIP_TRY(c, hipMemsetAsync(N.tab.sums, 0, slots * kNrmSums * sizeof(u64), s));
    HIP_TRY(c, hipMemsetAsync(N.d_ctr, 0, 2 * NC_N * sizeof(u64), s));
    N.dirty = false;
  }
  return MRH_OK;
}

// The four launches of one scan, n > 0.  *out_ctr: this scan's counters on the device, valid until the scan after the next
int launch_normals(mrh_ctx* c, const NrmPar& par, const float* d_xyz, const uint64_t n, float* d_nxyz, const u64** out_ctr) {
  int rc = normals_scratch(c, n);
  if (rc) return rc;
  auto& N = c->nrm;
  hipStream_t s = c->stream;
  NrmTab t = N.tab;
  const u32 set = ++N.seq & 1u;
  t.ctr = N.d_ctr + set * NC_N;
  t.ctr_next = N.d_ctr + (set ^ 1u) * NC_N;
  const u32 np = (u32) n, grid = (np + 255u) / 256u;
  N.dirty = true;
  if (N.fold) k_normals_accumulate<true><<<grid, 256, 0, s>>>(t, par, d_xyz, np);
  else k_normals_accumulate<false><<<grid, 256, 0, s>>>(t, par, d_xyz, np);
  k_normals_solve<<<std::min<u32>(1024u, (np + kNrmSolveCells - 1) / kNrmSolveCells), 1024, 0, s>>>(t, par);
  k_normals_assign<<<grid, 256, 0, s>>>(t, d_xyz, np, d_nxyz);
  k_normals_sweep<<<std::min<u32>(1024u, grid), 256, 0, s>>>(t, grid);
  HIP_TRY(c, hipGetLastError());
  N.dirty = false;
  *out_ctr = t.ctr;
  return MRH_OK;
}

// the counters of the last mrh_estimate_normals have landed in pinned memory (the caller synchronised): into Normals::info
void normals_fold_info(mrh_ctx* c) {
  auto& N = c->nrm;
  if (!N.info_pending) return;
  N.info.estimated = N.h_ctr[NC_ESTIMATED]; N.info.fallback = N.h_ctr[NC_FALLBACK];
  N.info.missing = N.h_ctr[NC_MISSING]; N.info.cells = N.h_ctr[NC_CELLS];
  N.info_pending = false;
}

}  // namespace

extern "C" {

int mrh_estimate_normals_device(mrh_ctx* c, const mrh_normals_params* p, const float* d_xyz, uint64_t n, float* d_nxyz) {
  int rc = ensure_device(c, "mrh_estimate_normals_device");
  if (rc) return rc;
  if (n && (!d_xyz || !d_nxyz)) return fail(c, MRH_ERR_INVALID_ARG, "mrh_estimate_normals_device: null argument");
  NrmPar par;
  rc = normals_args(c, "mrh_estimate_normals_device", p, n, &par);
  if (rc || n == 0) return rc;
  const u64* ctr;
  return launch_normals(c, par, d_xyz, n, d_nxyz, &ctr);
}

int mrh_estimate_normals(mrh_ctx* c, const mrh_normals_params* p, mrh_normals_info* out_info) {
  int rc = ensure_device(c, "mrh_estimate_normals");
  if (rc) return rc;
  auto& L = c->lidar;
  auto& N = c->nrm;
  if (!L.have_cloud) return fail(c, MRH_ERR_STATE, "mrh_estimate_normals: no current scan (mrh_upload_points / mrh_set_points_device)");
  const uint64_t n = L.num_points;
  NrmPar par;
  rc = normals_args(c, "mrh_estimate_normals", p, n, &par);
  if (rc) return rc;
  if (!N.h_ctr) {
    HIP_TRY(c, pinned_alloc(c, N.h_ctr, NC_N * sizeof(u64)));
    memset(N.h_ctr, 0, NC_N * sizeof(u64));
  }
  L.num_normals = 0;  // none valid from the moment the buffer may change
  rc = regrow(c, L.d_normals, L.normals_cap, (size_t) n, (size_t) n * 3 * sizeof(float));
  if (rc) return rc;
  N.info = {};
  N.info.points = n;
  N.info_pending = false;
  if (n) {
    const u64* ctr;
    rc = launch_normals(c, par, L.d_points_cur, n, L.d_normals, &ctr);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(N.h_ctr, ctr, NC_N * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    N.info_pending = true;
  }
  L.num_normals = n;
  if (out_info) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    normals_fold_info(c);
    *out_info = N.info;
  }
  return MRH_OK;
}

int mrh_get_normals(mrh_ctx* c, const float** out_nxyz, uint64_t* out_n, mrh_normals_info* out_info) {
  int rc = ensure_device(c, "mrh_get_normals");
  if (rc) return rc;
  if (!out_nxyz || !out_n) return fail(c, MRH_ERR_INVALID_ARG, "mrh_get_normals: null argument");
  auto& L = c->lidar;
  auto& N = c->nrm;
  const size_t n = L.num_normals;
  if ((rc = regrow_pinned(c, N.h_out, N.h_out_cap, n, n * 3 * sizeof(float)))) return rc;
  if (n) HIP_TRY(c, hipMemcpyAsync(N.h_out, L.d_normals, n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  normals_fold_info(c);
  *out_nxyz = N.h_out;
  *out_n = n;
  if (out_info) *out_info = N.info;
  return MRH_OK;
}

}  // extern "C"
