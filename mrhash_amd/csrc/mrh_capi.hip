// mrh_capi.hip — implementation of the C ABI (include/mrhash_hip.h) on top of the gfx950 kernels.
//
// Host side of the thin HIP layer: enqueues the per-frame kernel chain with no host round trip, and only synchronises in the
// calls that hand data back.  Here: the helpers every entry point shares, the entry points, the splat, raycast, distance-field, tracking and normals glue.
// The context and its lifetime: mrh_context.h; the copy pool: mrh_hostcopy.h; uploads, frame marks, peeks: mrh_upload.h; the
// host side of a depth frame: mrh_frame.h; extraction, scans, block I/O, RCCL: mrh_extract.h, mrh_points.h, mrh_blocks.h,
// mrh_comm.h.  One translation unit.
// There is NO CPU fallback in this file: without a HIP device mrh_create fails with MRH_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <sys/mman.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/mrhash_hip.h"
#include "../../include/mrhash_comm.h"
#include "../../include/mrhash_raycast.h"
#include "../../include/mrhash_esdf.h"
#include "../../include/mrhash_track.h"
#include "../../include/mrhash_normals.h"
#include "mrh_kernels.h"
#include "mrh_mc.h"
#include "mrh_raycast.h"
#include "mrh_esdf.h"
#include "mrh_track.h"
#include "mrh_normals.h"
#include "mrh_fast.h"
#include "mrh_pipe.h"
#include "mrh_fast2.h"
#include "mrh_mesh.h"
#include "mrh_lidar.h"
#include "mrh_scan.h"
#include "mrh_sort.h"
#include "mrh_splat.h"

using namespace mrh;

#include "mrh_context.h"
#include "mrh_hostcopy.h"
#include "mrh_upload.h"

namespace {

int drain_events(mrh_ctx* c) {
  for (auto& e : c->ev_pending) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e.a, e.b));
    c->sum_ms += ms;
    c->last_ms = ms;
    c->n_ms++;
    c->ev_pool.push_back(e);
  }
  c->ev_pending.clear();
  for (auto& e : c->ev_pending_front) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e.a, e.b));
    c->sum_front_ms += ms;
    c->n_front_ms++;
    c->ev_pool.push_back(e);
  }
  c->ev_pending_front.clear();
  return MRH_OK;
}

int check_device_flags(mrh_ctx* c, u32 flags) {
  // the flags are already cleared on the device (take_device_flags): whatever else is reported first, a scan that left its
  // bounds has left counters behind, and the next scan must start from zero
  if (flags & ERR_SCAN) c->lidar.buckets_dirty = true;
  if (flags & ERR_RANGE) return fail(c, MRH_ERR_OUT_OF_RANGE, "a block coordinate left the packed-key range of +-2^20 blocks");
  if (flags & ERR_POOL) return fail(c, MRH_ERR_CAPACITY, "SDF block pool exhausted (num_sdf_blocks = %llu)", (unsigned long long) c->num_blocks);
  if (flags & ERR_TABLE) return fail(c, MRH_ERR_CAPACITY, "hash table probe limit reached (hash_slots = %llu)", (unsigned long long) c->slots);
  if (flags & ERR_TRI) return fail(c, MRH_ERR_CAPACITY, "triangle buffer full (max_triangles = %llu)", (unsigned long long) c->max_triangles);
  if (flags & ERR_SCAN) return fail(c, MRH_ERR_DEVICE, "a LiDAR scan left its bounds (voxels per beam, touched blocks or chunks): the map is not usable");
  return MRH_OK;
}

// Device error flags are taken off the device and cleared there in one stream-ordered step (nothing else runs on the
// stream in between), so a flag is reported for the call that raised it and not for every later one.
int take_device_flags(mrh_ctx* c, u32* out) {
  u32 flags = 0;
  HIP_TRY(c, hipMemcpyAsync(&flags, &c->tab.ctr[CTR_ERROR], sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (flags) HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_ERROR], 0, sizeof(u32), c->stream));
  if (flags & ERR_POOL) c->table_dirty = true;  // keys without storage exist (publish_without_storage): census + rebuild before the next frame,
                                                // so that the positions can be allocated again as soon as the pool has room (vds.cu:566-569 retries every frame)
  c->flags_seen |= flags;
  *out = flags;
  return MRH_OK;
}

int ensure_device(mrh_ctx* c, const char* who) {
  if (!c) return MRH_ERR_INVALID_ARG;
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(c, MRH_ERR_DEVICE, "%s: hipSetDevice failed: %s", who, hipGetErrorString(e));
  return MRH_OK;
}
// every entry point except the per-frame ones (setters, mrh_integrate, the non-blocking peeks): behind the pipelined frames issued
// so far, the zombies nobody wanted leave the table, so that whatever the call reads, changes or waits for is exactly the map two
// serial launches per frame would have left
int ensure_ready(mrh_ctx* c, const char* who) {
  int rc = ensure_device(c, who);
  if (rc) return rc;
  rc = flush_deferred(c);  // a host-fed frame that mrh_integrate kept back runs before anything else looks at the map
  if (rc < 0) return rc;
  main_stream_changed_map(c);  // whatever this call does to the map, the front stream must see it before its next launch
  c->ps.flushed_since_frame = true;
  return strict_point(c);
}

// The scalars an extraction reads back land in one pinned block, h_mc (a copy into a stack variable is staged by the runtime):
// k_mc_scan_total's {triangle total, corner-record demand | bit 63: a block found no room}, the post-process's {vertices, faces},
// each copied as a pair, and compact_all's block count (an int).
enum HMcSlot { HMC_TRIANGLES = 0, HMC_RECORDS = 1, HMC_VERTICES = 2, HMC_FACES = 3, HMC_COMPACT = 4, HMC_SLOTS = 8 };
int ensure_h_mc(mrh_ctx* c) {
  if (c->h_mc) return MRH_OK;
  HIP_TRY(c, pinned_alloc(c, c->h_mc, HMC_SLOTS * sizeof(u64)));
  memset(c->h_mc, 0, HMC_SLOTS * sizeof(u64));
  return MRH_OK;
}

// flatAndReduceHashTable() without a camera: every live block onto the compact list (no frustum filter); enqueue only
int launch_compact_all(mrh_ctx* c) {
  HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_COMPACT], 0, sizeof(int), c->stream));
  k_compact<<<512, 256, 0, c->stream>>>(c->cam, c->map, c->tab, 0);
  return MRH_OK;
}

// compacts every live block and returns the count; blocking
int compact_all(mrh_ctx* c, int* out_n) {
  hipStream_t s = c->stream;
  int rc = launch_compact_all(c);
  if (rc) return rc;
  rc = ensure_h_mc(c);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->h_mc + HMC_COMPACT, &c->tab.ctr[CTR_COMPACT], sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  *out_n = *(const int*) (c->h_mc + HMC_COMPACT);
  return MRH_OK;
}

// grow-only scratch `slot` of at least `bytes` (contents undefined); the previous buffer is released only after the stream drained
int arena_get(mrh_ctx* c, const int slot, const size_t bytes, void** out) {
  if (bytes > c->arena_cap[slot]) {
    if (slot == 1) c->mesh_clean_words = 0;  // new memory: the post-process's tables are not the empty ones it left behind
    const int rc = regrow(c, c->arena[slot], c->arena_cap[slot], bytes + bytes / 4, bytes + bytes / 4);
    if (rc) return rc;
  }
  *out = c->arena[slot];
  return MRH_OK;
}

// Arena `slot` handed out by `lay(MeshScratch&)`, the one list of the buffers that live in it: `lay` runs once on no memory to
// learn the size the arena needs and again on the real base, so the size asked for and the pointers handed out cannot disagree.
template <typename Layout>
int arena_layout(mrh_ctx* c, const int slot, MeshScratch* m, Layout&& lay) {
  MeshScratch dry;
  lay(dry);
  m->bytes = dry.used;
  const int rc = arena_get(c, slot, m->bytes, &m->base);
  if (rc) return rc;
  m->used = 0;
  lay(*m);
  if (m->used > m->bytes) return fail(c, MRH_ERR_STATE, "scratch arena %d: the layout took %zu of %zu bytes", slot, m->used, m->bytes);
  return MRH_OK;
}

}  // namespace

#include "mrh_frame.h"
#include "mrh_extract.h"
#include "mrh_points.h"
#include "mrh_blocks.h"
#include "mrh_xplan.h"
#include "mrh_comm.h"

extern "C" {

#define MRH_STR2(x) #x
#define MRH_STR(x) MRH_STR2(x)
const char* mrh_version(void) { return "mrhash_hip abi" MRH_STR(MRH_ABI_VERSION) " gfx950 hand-written-hip"; }
#ifdef MRH_MC_TRACE
// tuning builds only (tools/trace_mc.sh): read (and optionally clear) the phase accumulators of k_mc
int mrh_debug_mc_trace(uint32_t* out, int clear) {  // out: 2 x 65536 x 8 words
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(d_mc_trace), sizeof(d_mc_trace)) != hipSuccess) return MRH_ERR_DEVICE;
  if (clear) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(d_mc_trace)) != hipSuccess || hipMemset(p, 0, sizeof(d_mc_trace)) != hipSuccess) return MRH_ERR_DEVICE;
  }
  return MRH_OK;
}
#endif

#ifdef MRH_SCAN_TRACE
// tuning builds only (tools/trace_scan.sh): read (and optionally clear) the phase stamps of the scan kernels
int mrh_debug_scan_trace(unsigned long long* out, int clear) {  // out: 4 x kScanTraceWgs x 8 words
  if (hipDeviceSynchronize() != hipSuccess) return MRH_ERR_DEVICE;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(d_scan_trace), sizeof(d_scan_trace)) != hipSuccess) return MRH_ERR_DEVICE;
  if (clear) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(d_scan_trace)) != hipSuccess || hipMemset(p, 0, sizeof(d_scan_trace)) != hipSuccess) return MRH_ERR_DEVICE;
  }
  return MRH_OK;
}
#endif

const char* mrh_last_error(const mrh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int mrh_create(const mrh_params* p, mrh_ctx** out) {
  if (!p || !out) return fail(nullptr, MRH_ERR_INVALID_ARG, "mrh_create: null argument");
  int rc = create_checks(p);
  if (rc) return rc;
  mrh_ctx* c = new mrh_ctx();
  if (!(rc = size_map(c, p)) && !(rc = alloc_map(c)) && !(rc = probe_arithmetic(c))) {
    read_switches(c);
    rc = init_buffers(c);
  }
  if (rc) {  // the one failure path: whatever the stages allocated is in the ledger
    g_create_err = "mrh_create: " + c->err;
    free_all(c);
    delete c;
    (void) hipGetLastError();  // reported above: the next context's launch checks must not find it
    return rc;
  }
  // identity pose; camera must be set by the caller (geowrapper.cpp:80 installs a 1x1 placeholder)
  const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const float z[3] = {0, 0, 0};
  mrh_set_pose(c, I, z);
  c->cam.min_depth = p->min_depth;
  c->cam.max_depth = p->max_depth;
  *out = c;
  return MRH_OK;
}

int mrh_destroy(mrh_ctx* c) {
  if (!c) return MRH_OK;
  if (getenv("MRH_DEBUG") && c->dbg_lazy_frames)
    fprintf(stderr, "[mrhash_hip] pipelined frames %llu: host waited %.1f us per frame for the ring, spent %.1f us per frame in the launch calls, %llu cross-stream waits\n",
            (unsigned long long) c->dbg_lazy_frames, c->dbg_spin_us / c->dbg_lazy_frames, c->dbg_api_us / c->dbg_lazy_frames, (unsigned long long) c->dbg_waits);
  if (getenv("MRH_DEBUG") && c->lidar.d_buckets_ctr && c->lidar.buckets_seq) {  // the last scan's counters (mrh_scan.h)
    u32 h[2 * SC_N] = {0};
    (void) hipStreamSynchronize(c->stream);
    (void) hipMemcpy(h, c->lidar.d_buckets_ctr, sizeof(h), hipMemcpyDeviceToHost);
    const u32* k = h + (c->lidar.buckets_seq & 1u) * SC_N;
    fprintf(stderr, "[mrhash_hip] last scan: %u records, %u chunks + %u runs beyond a wave\n", k[SC_PLACED], k[SC_CHUNKS], k[SC_BIG]);
  }
#ifdef MRH_TRACE
  if (const char* path = getenv("MRH_TRACE_FILE")) {  // tuning builds: phase timestamps of the last k_back launch
    if (c->fast.trace) {
      hipDeviceSynchronize();
      const size_t n = std::min<size_t>(c->num_blocks, 40960) * 8;
      std::vector<u64> h(n);
      hipMemcpy(h.data(), c->fast.trace, n * sizeof(u64), hipMemcpyDeviceToHost);
      if (FILE* fp = fopen(path, "wb")) { fwrite(h.data(), sizeof(u64), n, fp); fclose(fp); }
    }
  }
#endif
  if (c->deferred.on) { (void) hipSetDevice(c->device); (void) flush_deferred(c); }  // the frame mrh_integrate accepted last
  widen_quiesce();  // the result arrays are about to be unmapped
  if (getenv("MRH_DEBUG") || getenv("MRH_WIDEN_REPORT"))
    fprintf(stderr, "[mrhash_hip] widening: %llu chunks redone by the calling thread (their helper had not finished 40 us after the chunk landed)\n", (unsigned long long) widen_redone());
  free_all(c);
  delete c;
  return MRH_OK;
}

int mrh_reset(mrh_ctx* c) {
  int rc = ensure_ready(c, "mrh_reset");
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  rc = drain_events(c);
  if (rc) return rc;
  return init_buffers(c);
}

int mrh_set_camera(mrh_ctx* c, float fx, float fy, float cx, float cy, int rows, int cols, float min_depth, float max_depth, int model) {
  if (!c) return MRH_ERR_INVALID_ARG;
  if (rows <= 0 || cols <= 0 || (model != MRH_CAMERA_PINHOLE && model != MRH_CAMERA_SPHERICAL))
    return fail(c, MRH_ERR_INVALID_ARG, "mrh_set_camera: bad rows/cols/model");
  if (c->deferred.on) {  // a frame kept back by mrh_integrate was issued under the old camera
    const int frc = ensure_device(c, "mrh_set_camera");
    if (frc) return frc;
    const int drc = flush_deferred(c);
    if (drc < 0) return drc;
  }
  Cam& k = c->cam;
  // camera.cuh:19-34
  k.fx = fx; k.fy = fy; k.ifx = 1.f / fx; k.ify = 1.f / fy; k.cx = cx; k.cy = cy;
  k.rows = rows; k.cols = cols;
  k.row_thr = (int) ((float) (unsigned) rows * 0.5f);
  k.col_thr = (int) ((float) (unsigned) cols * 0.5f);
  k.min_depth = min_depth; k.max_depth = max_depth;
  k.max_int_dist = max_depth;  // geowrapper.cpp:111 setIntegrationDistance(max_depth)
  c->spherical = model == MRH_CAMERA_SPHERICAL;
  k.model = c->spherical ? 1 : 0;
  c->has_camera = true;
  return MRH_OK;
}

int mrh_set_pose(mrh_ctx* c, const float R[9], const float t[3]) {
  if (!c || !R || !t) return MRH_ERR_INVALID_ARG;
  Cam& k = c->cam;
  memcpy(k.R, R, 36);
  memcpy(k.t, t, 12);
  // cuda_algebra.cuh:45-57, 137-143 (the reference recomputes this per thread on the device)
  k.Ri[0] = R[0]; k.Ri[1] = R[3]; k.Ri[2] = R[6];
  k.Ri[3] = R[1]; k.Ri[4] = R[4]; k.Ri[5] = R[7];
  k.Ri[6] = R[2]; k.Ri[7] = R[5]; k.Ri[8] = R[8];
  // evaluated with separate products and sums (no FMA): this TU is built with -ffp-contract=off
  const float x = k.Ri[0] * t[0] + k.Ri[1] * t[1] + k.Ri[2] * t[2];
  const float y = k.Ri[3] * t[0] + k.Ri[4] * t[1] + k.Ri[5] * t[2];
  const float z = k.Ri[6] * t[0] + k.Ri[7] * t[1] + k.Ri[8] * t[2];
  k.ti[0] = -x; k.ti[1] = -y; k.ti[2] = -z;
  return MRH_OK;
}

namespace {

// ---- 3DGS splat seeds: GaussianContainer::extractNodesQTree + checkNodes (gaussian_data_structures.cpp:48-68, .cu:58-84), see mrh_splat.h
int seeds_checks(mrh_ctx* c, const float qtree_thresh, const int qtree_min_pixel_size, const mrh_splat_seed** out, uint64_t* out_n) {
  if (!out || !out_n) return fail(c, MRH_ERR_INVALID_ARG, "mrh_splat_seeds: null argument");
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_splat_seeds: an exchange is pending (call mrh_integrate_resume)");
  if (!c->has_camera) return fail(c, MRH_ERR_STATE, "mrh_splat_seeds: set_camera has not been called");
  if (c->spherical) return fail(c, MRH_ERR_UNSUPPORTED, "mrh_splat_seeds: pinhole camera only");
  if (qtree_min_pixel_size < 0 || qtree_thresh != qtree_thresh) return fail(c, MRH_ERR_INVALID_ARG, "mrh_splat_seeds: bad quad-tree parameter");
  if (!c->d_depth || !c->d_rgb) return fail(c, MRH_ERR_STATE, "mrh_splat_seeds: no depth / colour image");
  const Cam& k = c->cam;
  if (c->depth_rows != k.rows || c->depth_cols != k.cols || c->rgb_rows != k.rows || c->rgb_cols != k.cols)
    return fail(c, MRH_ERR_INVALID_ARG, "mrh_splat_seeds: image shape differs from the camera");
  if ((uint64_t) k.rows * (uint64_t) k.cols > (1ull << 22)) return fail(c, MRH_ERR_CAPACITY, "mrh_splat_seeds: image above 2^22 pixels");
  return MRH_OK;
}
// The buffers of a tree of qt.total potential nodes.  The seven device buffers sized by the node count and d_qt_misc are one
// regrow_all under qt_cap, reallocated whenever the count differs, not only when it grows.  A failed allocation leaves no device
// buffer and capacity 0, so the next call allocates again whatever its image shape; the last call's leaves go with d_qt_leaves.
// The pinned seeds only grow (regrow_pinned; they used to shrink with the tree): k_qt_scatter is told their capacity.
int qtree_buffers(mrh_ctx* c, const QTree& qt) {
  const size_t n = qt.total, seeds = std::min<size_t>(n, (size_t) 1 << 20);  // seeds <= leaves <= 1 000 000 (mrh_splat_seeds checks)
  int rc = MRH_OK;
  if (n != c->qt_cap) {
    c->qt_n_leaves = 0;
    c->qt_leaves_on_host = true;
    c->qt_leaves.clear();
    rc = regrow_all(c, c->qt_cap, n, {{c->d_qt_sums, n * sizeof(QSum)}, {c->d_qt_flags, n * sizeof(u32)}, {c->d_qt_unc, n * sizeof(u32)}, {c->d_qt_marks, n * sizeof(u64)},
                                      {c->d_qt_pos, (n + (n + kChainTile - 1) / kChainTile + 1) * sizeof(u64)},  // + the tile sums of the marks' scan
                                      {c->d_qt_parked, n * sizeof(mrh_splat_seed)}, {c->d_qt_leaves, n * sizeof(mrh_qtree_leaf)}, {c->d_qt_misc, 2 * sizeof(u64)}});
  }
  if (!rc) rc = regrow_pinned(c, c->h_qt_seeds, c->qt_seed_cap, seeds, seeds * sizeof(mrh_splat_seed));
  if (rc) return rc;
  if (!c->h_qt_out) HIP_TRY(c, pinned_alloc(c, c->h_qt_out, 2 * sizeof(u64)));
  return MRH_OK;
}
int launch_qtree(mrh_ctx* c, const QTree& qt, const float qtree_thresh) {
  hipStream_t s = c->stream;
  const u32 grid = (qt.total + 255) / 256;
  u32* unc_count = (u32*) (c->d_qt_misc + 1);
  // exact statistics of every potential node, four tree levels per launch
  int L = qt.D, T = L < 4 ? L : 4;
  k_qt_sums_bottom<<<1u << (2 * (L - T)), 256, 0, s>>>(qt, c->d_rgb, c->d_qt_sums, T, c->d_qt_misc);
  for (L -= T; L > 0; L -= T) {
    T = L < 4 ? L : 4;
    k_qt_sums_up<<<1u << (2 * (L - T)), 256, 0, s>>>(qt, c->d_qt_sums, L, T);
  }
  // exclusive scan of the marks (mrh_sort.h): the tile sums (parked behind the positions) are cleared by k_qt_decide and added up by
  // k_qt_emit's workgroups, then every tile scans on its own
  const u32 tiles = (u32) ((qt.total + kChainTile - 1) / kChainTile);
  static_assert(kChainTile % 256 == 0, "a workgroup of k_qt_emit lies inside one scan tile");
  k_qt_decide<<<grid, 256, 0, s>>>(qt, qtree_thresh, c->d_qt_sums, c->qt_literal, c->d_qt_flags, c->d_qt_unc, unc_count, c->d_qt_pos + qt.total, tiles);
  k_qt_literal<<<512, 256, 0, s>>>(qt, c->d_rgb, qtree_thresh, c->d_qt_unc, unc_count, c->d_qt_flags);
  k_qt_emit<<<grid, 256, 0, s>>>(qt, c->cam, c->map, c->tab, c->d_depth, c->d_rgb, c->d_qt_flags, c->d_qt_marks, c->d_qt_parked, c->d_qt_pos + qt.total);
  k_tile_scan_u64<<<tiles, 1024, 0, s>>>(c->d_qt_marks, (u32) qt.total, c->d_qt_pos + qt.total, c->d_qt_pos);
  k_qt_scatter<<<grid, 256, 0, s>>>(qt, c->d_qt_marks, c->d_qt_pos, c->d_qt_parked, c->d_qt_leaves, c->h_qt_seeds, (u32) c->qt_seed_cap, c->d_qt_misc, c->h_qt_out);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

}  // namespace

int mrh_upload_depth(mrh_ctx* c, const float* depth, int rows, int cols) {
  int rc = ensure_device(c, "mrh_upload_depth");
  if (rc) return rc;
  if (!depth || rows <= 0 || cols <= 0) return fail(c, MRH_ERR_INVALID_ARG, "mrh_upload_depth: bad argument");
  const void* dev = nullptr;
  rc = upload_image(c, c->up_depth, depth, (size_t) rows * cols * sizeof(float), &dev);
  if (rc) return rc;
  c->d_depth = (const float*) dev;
  c->depth_rows = rows; c->depth_cols = cols;
  return MRH_OK;
}

int mrh_upload_rgb(mrh_ctx* c, const uint8_t* rgb, int rows, int cols) {
  int rc = ensure_device(c, "mrh_upload_rgb");
  if (rc) return rc;
  if (!rgb || rows <= 0 || cols <= 0) return fail(c, MRH_ERR_INVALID_ARG, "mrh_upload_rgb: bad argument");
  const void* dev = nullptr;
  rc = upload_image(c, c->up_rgb, rgb, (size_t) rows * cols * 3, &dev);
  if (rc) return rc;
  c->d_rgb = (const uint8_t*) dev;
  c->rgb_rows = rows; c->rgb_cols = cols;
  return MRH_OK;
}

int mrh_set_depth_device(mrh_ctx* c, const float* d_depth, int rows, int cols) {
  if (!c || !d_depth || rows <= 0 || cols <= 0) return fail(c, MRH_ERR_INVALID_ARG, "mrh_set_depth_device: bad argument");
  if (c->deferred.on) { (void) hipSetDevice(c->device); const int drc = flush_deferred(c); if (drc < 0) return drc; }
  c->d_depth = d_depth; c->depth_rows = rows; c->depth_cols = cols;
  c->up_depth.cur = -1;
  return MRH_OK;
}

int mrh_set_rgb_device(mrh_ctx* c, const uint8_t* d_rgb, int rows, int cols) {
  if (!c || !d_rgb || rows <= 0 || cols <= 0) return fail(c, MRH_ERR_INVALID_ARG, "mrh_set_rgb_device: bad argument");
  if (c->deferred.on) { (void) hipSetDevice(c->device); const int drc = flush_deferred(c); if (drc < 0) return drc; }
  c->d_rgb = d_rgb; c->rgb_rows = rows; c->rgb_cols = cols;
  c->up_rgb.cur = -1;
  return MRH_OK;
}

// voxel_data_structures.cpp:90-110 VoxelContainer::integrate, as one sync-free kernel chain (mrh_frame.h)
int mrh_integrate(mrh_ctx* c, int n_frames_invalidate) {
  int rc = ensure_device(c, "mrh_integrate");
  if (rc) return rc;
  rc = flush_deferred(c);  // the frame of the previous call: its images have landed meanwhile
  if (rc < 0) return rc;
  if (frame_is_deferrable(c)) return defer_frame(c, n_frames_invalidate);
  rc = run_frame(c, n_frames_invalidate);
  if (rc == MRH_OK) prewarm_maybe(c);
  return rc;
}

int mrh_integrate_resume(mrh_ctx* c) {
  const int rc = ensure_ready(c, "mrh_integrate_resume");
  return rc ? rc : resume_frame(c);
}

int mrh_exchange_buffer(mrh_ctx* c, void** out_ptr, uint64_t* out_n, int* out_is_device) {
  if (!c || !out_ptr || !out_n) return MRH_ERR_INVALID_ARG;
  if (c->pending == 0) return fail(c, MRH_ERR_STATE, "mrh_exchange_buffer: no exchange is pending");
  const size_t npix = (size_t) c->cam.rows * c->cam.cols;
  *out_ptr = c->pending == 1 ? (void*) c->d_zbuf : (void*) (c->d_zbuf + npix);
  *out_n = npix;
  if (out_is_device) *out_is_device = 1;
  return MRH_OK;
}

int mrh_sync(mrh_ctx* c) {
  int rc = ensure_ready(c, "mrh_sync");
  if (rc) return rc;
  u32 flags = 0;
  rc = take_device_flags(c, &flags);
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  rc = drain_events(c);
  if (rc) return rc;
  flags |= c->flags_deferred;
  c->flags_deferred = 0;
  c->flags_peeked = 0;
  return check_device_flags(c, flags);
}

int mrh_splat_seeds(mrh_ctx* c, float qtree_thresh, int qtree_min_pixel_size, const mrh_splat_seed** out, uint64_t* out_n) {
  int rc = ensure_ready(c, "mrh_splat_seeds");
  if (rc) return rc;
  if ((rc = seeds_checks(c, qtree_thresh, qtree_min_pixel_size, out, out_n))) return rc;
  // depth of the potential tree: the first level whose largest rectangle (the bottom-right chain of ceil halves) can no longer
  // split (quad_tree.cu:133-149)
  QTree qt = {c->cam.cols, c->cam.rows, 0, qtree_min_pixel_size, 0};
  for (int w = qt.W, h = qt.H; qt.D < kQtMaxDepth && !(w / 2 <= qt.min_px || h / 2 <= qt.min_px); qt.D++) { w -= w / 2; h -= h / 2; }
  qt.total = qt_level_offset(qt.D + 1);
  if ((rc = qtree_buffers(c, qt))) return rc;
  if ((rc = send_uploads(c, c->stream))) return rc;
  if ((rc = launch_qtree(c, qt, qtree_thresh))) return rc;
  if ((rc = mark_frame(c))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the last launch wrote totals and seeds into pinned memory
  const u64 h_misc[2] = {((volatile u64*) c->h_qt_out)[0], ((volatile u64*) c->h_qt_out)[1]};
  const uint64_t n_leaves = h_misc[0] & 0xFFFFFFFFull, n_seeds = h_misc[0] >> 32;
  c->qt_last_literal = (uint32_t) h_misc[1];
  if (n_leaves > 1000000ull) return fail(c, MRH_ERR_CAPACITY, "mrh_splat_seeds: %llu leaves, above the reference's capacity of 1000000 (params.h:20-23)", (unsigned long long) n_leaves);
  // the leaves (tens of thousands per frame) stay on the device until mrh_get_qtree_leaves asks: the fusion loop only takes the seeds
  c->qt_n_leaves = n_leaves;
  c->qt_leaves_on_host = n_leaves == 0;
  c->qt_leaves.clear();
  if (getenv("MRH_DEBUG")) {
    fprintf(stderr, "[mrh] splat seeds: %u potential nodes, %u literal evaluations, %llu leaves, %llu seeds\n", qt.total,
            c->qt_last_literal, (unsigned long long) n_leaves, (unsigned long long) n_seeds);
  }
  *out_n = n_seeds;
  *out = c->h_qt_seeds;
  return MRH_OK;
}

int mrh_get_qtree_leaves(mrh_ctx* c, const mrh_qtree_leaf** out, uint64_t* out_n) {
  if (!c || !out || !out_n) return MRH_ERR_INVALID_ARG;
  if (!c->qt_leaves_on_host) {
    c->qt_leaves.resize(c->qt_n_leaves);
    HIP_TRY(c, hipMemcpyAsync(c->qt_leaves.data(), c->d_qt_leaves, c->qt_n_leaves * sizeof(mrh_qtree_leaf), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->qt_leaves_on_host = true;
  }
  *out = c->qt_leaves.data();
  *out_n = c->qt_leaves.size();
  return MRH_OK;
}

int mrh_get_free_blocks(mrh_ctx* c, int64_t* out_free_fine, int64_t* out_free_coarse) {
  int rc = ensure_ready(c, "mrh_get_free_blocks");
  if (rc) return rc;
  int h[2] = {0, 0};  // CTR_HEAP_FINE, CTR_HEAP_COARSE are adjacent: stack tops, free count = top + 1
  HIP_TRY(c, hipMemcpyAsync(h, &c->tab.ctr[CTR_HEAP_FINE], 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out_free_fine) *out_free_fine = (int64_t) h[0] + 1;
  if (out_free_coarse) *out_free_coarse = (int64_t) h[1] + 1;
  return MRH_OK;
}

int mrh_peek_free_blocks(mrh_ctx* c, int64_t* out_free_fine, int64_t* out_free_coarse, uint64_t* out_frames_behind) {
  int rc = ensure_device(c, "mrh_peek_free_blocks");
  if (rc) return rc;
  if ((rc = enable_peeks(c))) return rc;  // a first call finds no report below: answered the blocking way
  uint64_t seq = 0, back = 0;
  if ((rc = newest_report(c, "mrh_peek_free_blocks", &seq, &back)) < 0) return rc;
  if (rc) {
    if (out_free_fine) *out_free_fine = (int64_t) c->h_peek[8 * (seq % 8)] + 1;
    if (out_free_coarse) *out_free_coarse = (int64_t) c->h_peek[8 * (seq % 8) + 1] + 1;
    // a host-fed frame that mrh_integrate has kept back (flush_deferred) has no sequence number yet: it counts as one more frame behind
    if (out_frames_behind) *out_frames_behind = back - 1 + (c->deferred.on ? 1 : 0);
    return MRH_OK;
  }
  if (out_frames_behind) *out_frames_behind = 0;
  return mrh_get_free_blocks(c, out_free_fine, out_free_coarse);  // blocking: runs a kept-back frame first (ensure_ready)
}

int mrh_peek_error_flags(mrh_ctx* c, uint32_t* out_new_flags) {
  int rc = ensure_device(c, "mrh_peek_error_flags");
  if (rc) return rc;
  if (!out_new_flags) return MRH_ERR_INVALID_ARG;
  *out_new_flags = 0;
  if (!c->peek_enabled) return enable_peeks(c);
  uint64_t seq = 0, back = 0;
  if ((rc = newest_report(c, "mrh_peek_error_flags", &seq, &back)) <= 0) return rc;
  const u32 flags = (u32) c->h_peek[8 * (seq % 8) + CTR_ERROR];
  *out_new_flags = flags & ~c->flags_peeked;
  if (*out_new_flags & ERR_POOL) c->table_dirty = true;  // as in take_device_flags: drop the keys without storage before the next frame
  c->flags_peeked = flags;  // the device clears its flags only in mrh_sync: what is set now has been reported
  return MRH_OK;
}

int mrh_set_profile(mrh_ctx* c, int enabled) {
  int rc = ensure_ready(c, "mrh_set_profile");
  if (rc) return rc;
  c->profile = enabled ? 1 : 0;
  return MRH_OK;
}

int mrh_get_stats(mrh_ctx* c, mrh_stats* out) {
  int rc = ensure_ready(c, "mrh_get_stats");
  if (rc) return rc;
  if (!out) return MRH_ERR_INVALID_ARG;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_LIVE_FINE], 0, 2 * sizeof(int), s));
  HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_MAXPROBE], 0, 2 * sizeof(int), s));  // CTR_MAXPROBE, CTR_TOMBS_NOW
  k_count_live<<<256, 256, 0, s>>>(c->tab);
  k_table_census<<<(int) std::min<uint64_t>(2048, (c->slots + 255) / 256), 256, 0, s>>>(c->tab, (size_t) c->slots);
  int h_ctr[CTR_COUNT];
  u64 h_prof[PROF_COUNT];
  const bool fastp = !c->tab.multi_res;
  std::vector<u64> partials(fastp ? (size_t) 32768 * 4 : (size_t) c->integrate_grid);
  HIP_TRY(c, hipMemcpyAsync(h_ctr, c->tab.ctr, sizeof h_ctr, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(h_prof, c->tab.prof, sizeof h_prof, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(partials.data(), fastp ? c->d_cnt_partials : c->d_upd_partials, partials.size() * sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  rc = drain_events(c);
  if (rc) return rc;
  u64 total_upd = h_prof[PROF_UPDATED];  // LiDAR scans (k_points_apply); the image paths count through the partials
  for (u64 v : partials) total_upd += v;
  memset(out, 0, sizeof *out);
  out->frames_integrated = c->frames;
  out->num_sdf_blocks = c->num_blocks;
  out->occupied_fine = (uint64_t) h_ctr[CTR_LIVE_FINE];
  out->occupied_coarse = (uint64_t) h_ctr[CTR_LIVE_COARSE];
  out->free_fine = (int64_t) h_ctr[CTR_HEAP_FINE] + 1;
  out->free_coarse = (int64_t) h_ctr[CTR_HEAP_COARSE] + 1;
  out->last_compact_blocks = (uint64_t) h_ctr[CTR_COMPACT] + (fastp ? (uint64_t) h_ctr[CTR_CULLED] + (uint64_t) h_ctr[CTR_FREED_EARLY] : 0);
  if (fastp && c->ps.h_levels && out->last_compact_blocks >= (uint64_t) h_ctr[CTR_ZSKIP]) out->last_compact_blocks -= (uint64_t) h_ctr[CTR_ZSKIP];  // list entries that were unwanted zombies
  out->total_updated_voxels = total_upd;
  out->last_updated_voxels = total_upd - c->prev_total_updated;
  out->last_inserted_blocks = h_prof[PROF_INSERTED] - c->prev_inserted;
  out->last_freed_blocks = h_prof[PROF_FREED] - c->prev_freed;
  c->prev_total_updated = total_upd;
  c->prev_inserted = h_prof[PROF_INSERTED];
  c->prev_freed = h_prof[PROF_FREED];
  out->total_compact_blocks = h_prof[PROF_COMPACT];
  out->last_triangles = c->last_triangles;
  out->last_integrate_kernel_ms = c->last_ms;
  out->sum_integrate_kernel_ms = c->sum_ms;
  out->n_integrate_kernel = c->n_ms;
  out->error_flags = (u32) h_ctr[CTR_ERROR] | c->flags_seen;
  out->hash_slots = c->slots;
  out->tombstones = (uint64_t) h_ctr[CTR_TOMBS_NOW];
  out->max_probe_length = (u32) h_ctr[CTR_MAXPROBE];
  out->rehash_count = (u32) h_ctr[CTR_NREHASH];
  out->last_mc_count_ms = c->last_mc_count_ms;
  out->last_mc_emit_ms = c->last_mc_emit_ms;
  out->last_mc_blocks = c->last_mc_blocks;
  out->sum_front_kernel_ms = c->sum_front_ms;
  out->n_front_kernel = c->n_front_ms;
  HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_TOMBS_NOW], 0, sizeof(int), s));  // the census accumulator belongs to maintain_table
  return MRH_OK;
}

int mrh_selftest_division(mrh_ctx* c, uint64_t samples, uint64_t seed, uint64_t* out_mismatches) {
  int rc = ensure_ready(c, "mrh_selftest_division");
  if (rc) return rc;
  if (!out_mismatches) return MRH_ERR_INVALID_ARG;
  DevBuf<u64> d;
  HIP_TRY(c, d.alloc(1));
  HIP_TRY(c, hipMemsetAsync(d, 0, sizeof(u64), c->stream));
  const u32 threads = 1024 * 256;
  const u32 iters = (u32) ((samples + threads - 1) / threads);
  k_selftest_division<<<1024, 256, 0, c->stream>>>(seed, iters, d);
  u64 h = 0;
  HIP_TRY(c, hipMemcpyAsync(&h, d, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *out_mismatches = h;
  return MRH_OK;
}

}  // extern "C"

// ---- raycasting (include/mrhash_raycast.h, mrh_raycast.h) ------------------------------------------------------------------
namespace {
float ray_z_host(const float min_depth, const float step, const uint32_t k) { return min_depth + (float) k * step; }  // = ray_z

// the arguments every entry point shares, checked before the map is touched; fills the kernel's camera.  model: MRH_CAMERA_*
int raycast_args(mrh_ctx* c, const char* who, const int model, const mrh_raycast_params* p, const float* R, const float* t, RayCam* rc) {
  if (!p || !R || !t) return fail(c, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (c->pending) return fail(c, MRH_ERR_STATE, "%s: an exchange is pending (call mrh_integrate_resume)", who);
  if (c->map.shard_count > 1) return fail(c, MRH_ERR_UNSUPPORTED, "%s: sharded maps are not rendered (shard_count %d)", who, c->map.shard_count);
  if (p->rows < 1 || p->rows > MRH_RAYCAST_MAX_SIDE || p->cols < 1 || p->cols > MRH_RAYCAST_MAX_SIDE)
    return fail(c, MRH_ERR_INVALID_ARG, "%s: image of %d x %d pixels (1 .. %d per side)", who, p->rows, p->cols, MRH_RAYCAST_MAX_SIDE);
  if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || p->fx == 0.f || p->fy == 0.f || !std::isfinite(p->cx) || !std::isfinite(p->cy))
    return fail(c, MRH_ERR_INVALID_ARG, "%s: bad intrinsics", who);
  if (!(p->min_depth > 0.f) || !(p->max_depth > p->min_depth) || !std::isfinite(p->max_depth))
    return fail(c, MRH_ERR_INVALID_ARG, "%s: need 0 < min_depth < max_depth (got %g, %g)", who, (double) p->min_depth, (double) p->max_depth);
  const uint32_t known = MRH_RAYCAST_NORMALS | MRH_RAYCAST_COLORS | (model == MRH_CAMERA_SPHERICAL ? MRH_RAYCAST_POINTS : 0u);
  if (p->outputs & ~known) return fail(c, MRH_ERR_INVALID_ARG, "%s: unknown output bits 0x%x", who, p->outputs);
  const float step = p->step == 0.f ? 0.5f * c->p.sdf_truncation : p->step;
  if (!(step > 0.f) || !std::isfinite(step)) return fail(c, MRH_ERR_INVALID_ARG, "%s: the sample spacing must be > 0 (step %g)", who, (double) step);
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(R[i])) return fail(c, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(t[i])) return fail(c, MRH_ERR_INVALID_ARG, "%s: pose is not finite", who);
  // samples z_k <= max_depth: z_k is monotone in k (two monotone roundings), so the count is found by bisection on k
  if (ray_z_host(p->min_depth, step, MRH_RAYCAST_MAX_SAMPLES) <= p->max_depth)
    return fail(c, MRH_ERR_INVALID_ARG, "%s: more than 2^20 samples per ray (min_depth %g, max_depth %g, step %g)", who, (double) p->min_depth,
                (double) p->max_depth, (double) step);
  uint32_t lo = 0, hi = MRH_RAYCAST_MAX_SAMPLES;  // z(lo) <= max_depth < z(hi)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ray_z_host(p->min_depth, step, mid) <= p->max_depth) lo = mid;
    else hi = mid;
  }
  rc->ifx = 1.0f / p->fx;
  rc->ify = 1.0f / p->fy;
  rc->cx = p->cx; rc->cy = p->cy;
  rc->rows = p->rows; rc->cols = p->cols;
  if (model == MRH_CAMERA_SPHERICAL) {
    // every pixel's azimuth and elevation within the range mrh_sincosf is specified on: the kernel's expressions (ray_dir_sensor)
    // at the corner pixels — they are monotone in the column and in the row, so the corners bound every pixel
    const float az0 = rc->ifx * (((float) 0 - rc->cx) - 0.5f), az1 = rc->ifx * (((float) (rc->cols - 1) - rc->cx) - 0.5f);
    const float el0 = rc->ify * (((float) 0 - rc->cy) - 0.5f), el1 = rc->ify * (((float) (rc->rows - 1) - rc->cy) - 0.5f);
    const float worst = std::fmax(std::fmax(std::fabs(az0), std::fabs(az1)), std::fmax(std::fabs(el0), std::fabs(el1)));
    if (!(worst <= MRH_SM_SINCOS_MAX))
      return fail(c, MRH_ERR_INVALID_ARG, "%s: a pixel's azimuth or elevation reaches %g rad (sine and cosine are specified up to %g)", who,
                  (double) worst, (double) MRH_SM_SINCOS_MAX);
  }
  rc->min_depth = p->min_depth; rc->max_depth = p->max_depth; rc->step = step;
  rc->n_samples = hi;
  for (int i = 0; i < 9; i++) rc->R[i] = R[i];
  for (int i = 0; i < 3; i++) rc->t[i] = t[i];
  return MRH_OK;
}

// the four images, device pointers (nullptr = not wanted); `points` exists for the spherical model only
struct RayOut {
  float* depth; float* normals; uint8_t* rgb; float* points;
};

void launch_raycast(mrh_ctx* c, const int model, const RayCam& rc, const RayOut& o) {
  const dim3 grid((unsigned) ((rc.cols + kRenderTile - 1) / kRenderTile), (unsigned) ((rc.rows + kRenderTile - 1) / kRenderTile));
  if (model == MRH_CAMERA_SPHERICAL) k_raycast<true><<<grid, kRenderTile * kRenderTile, 0, c->stream>>>(c->map, c->tab, rc, o.depth, o.normals, o.rgb, o.points);
  else k_raycast<false><<<grid, kRenderTile * kRenderTile, 0, c->stream>>>(c->map, c->tab, rc, o.depth, o.normals, o.rgb, nullptr);
}

// c->d_ray / c->h_ray per pixel: [depth f32 | normals 3 x f32 | points 3 x f32 | rgb 3 x u8], each image contiguous
constexpr size_t kRayPixelBytes = sizeof(float) * 7 + 3;
constexpr size_t ray_off_normals(const size_t npix) { return npix * sizeof(float); }
constexpr size_t ray_off_points(const size_t npix) { return npix * sizeof(float) * 4; }
constexpr size_t ray_off_rgb(const size_t npix) { return npix * sizeof(float) * 7; }

// mrh_raycast / mrh_raycast_spherical: the render into the context's own images and their pinned copy (blocks)
int raycast_host(mrh_ctx* c, const char* who, const int model, const mrh_raycast_params* p, const float* R, const float* t, const float** out_depth,
                 const float** out_normals, const uint8_t** out_rgb, const float** out_points) {
  if (!c) return MRH_ERR_INVALID_ARG;
  RayCam rc;
  int rc_ = raycast_args(c, who, model, p, R, t, &rc);
  if (rc_) return rc_;
  rc_ = ensure_ready(c, who);
  if (rc_) return rc_;
  const size_t npix = (size_t) rc.rows * (size_t) rc.cols;
  const size_t bytes = npix * kRayPixelBytes;
  rc_ = regrow(c, c->d_ray, c->ray_cap, npix, bytes, false);  // the previous raycast has finished (it blocked): nothing reads the old buffers
  if (rc_) return rc_;
  if ((rc_ = regrow_pinned(c, c->h_ray, c->h_ray_cap, npix, bytes))) return rc_;
  const bool want_n = out_normals && (p->outputs & MRH_RAYCAST_NORMALS), want_c = out_rgb && (p->outputs & MRH_RAYCAST_COLORS);
  const bool want_p = out_points && (p->outputs & MRH_RAYCAST_POINTS);
  const RayOut d = {(float*) c->d_ray, (float*) (c->d_ray + ray_off_normals(npix)), (uint8_t*) (c->d_ray + ray_off_rgb(npix)),
                    (float*) (c->d_ray + ray_off_points(npix))};
  launch_raycast(c, model, rc, RayOut{out_depth ? d.depth : nullptr, want_n ? d.normals : nullptr, want_c ? d.rgb : nullptr, want_p ? d.points : nullptr});
  HIP_TRY(c, hipGetLastError());
  if (out_depth) HIP_TRY(c, hipMemcpyAsync(c->h_ray, d.depth, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (want_n) HIP_TRY(c, hipMemcpyAsync(c->h_ray + ray_off_normals(npix), d.normals, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (want_c) HIP_TRY(c, hipMemcpyAsync(c->h_ray + ray_off_rgb(npix), d.rgb, npix * 3, hipMemcpyDeviceToHost, c->stream));
  if (want_p) HIP_TRY(c, hipMemcpyAsync(c->h_ray + ray_off_points(npix), d.points, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out_depth) *out_depth = (const float*) c->h_ray;
  if (out_normals) *out_normals = want_n ? (const float*) (c->h_ray + ray_off_normals(npix)) : nullptr;
  if (out_rgb) *out_rgb = want_c ? (const uint8_t*) (c->h_ray + ray_off_rgb(npix)) : nullptr;
  if (out_points) *out_points = want_p ? (const float*) (c->h_ray + ray_off_points(npix)) : nullptr;
  return MRH_OK;
}

// mrh_raycast_device / mrh_raycast_spherical_device: the render into the caller's device buffers (enqueues)
int raycast_device(mrh_ctx* c, const char* who, const int model, const mrh_raycast_params* p, const float* R, const float* t, const RayOut& o) {
  if (!c) return MRH_ERR_INVALID_ARG;
  RayCam rc;
  int rc_ = raycast_args(c, who, model, p, R, t, &rc);
  if (rc_) return rc_;
  rc_ = ensure_ready(c, who);
  if (rc_) return rc_;
  launch_raycast(c, model, rc, RayOut{o.depth, (p->outputs & MRH_RAYCAST_NORMALS) ? o.normals : nullptr, (p->outputs & MRH_RAYCAST_COLORS) ? o.rgb : nullptr,
                                      (p->outputs & MRH_RAYCAST_POINTS) ? o.points : nullptr});
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
}  // namespace

extern "C" {

int mrh_raycast(mrh_ctx* c, const mrh_raycast_params* p, const float R_row_major[9], const float t[3], const float** out_depth,
                const float** out_normals, const uint8_t** out_rgb) {
  return raycast_host(c, "mrh_raycast", MRH_CAMERA_PINHOLE, p, R_row_major, t, out_depth, out_normals, out_rgb, nullptr);
}

int mrh_raycast_device(mrh_ctx* c, const mrh_raycast_params* p, const float R_row_major[9], const float t[3], float* d_depth, float* d_normals,
                       uint8_t* d_rgb) {
  return raycast_device(c, "mrh_raycast_device", MRH_CAMERA_PINHOLE, p, R_row_major, t, RayOut{d_depth, d_normals, d_rgb, nullptr});
}

int mrh_raycast_spherical(mrh_ctx* c, const mrh_raycast_params* p, const float R_row_major[9], const float t[3], const float** out_range,
                          const float** out_normals, const uint8_t** out_rgb, const float** out_points) {
  return raycast_host(c, "mrh_raycast_spherical", MRH_CAMERA_SPHERICAL, p, R_row_major, t, out_range, out_normals, out_rgb, out_points);
}

int mrh_raycast_spherical_device(mrh_ctx* c, const mrh_raycast_params* p, const float R_row_major[9], const float t[3], float* d_range,
                                 float* d_normals, uint8_t* d_rgb, float* d_points) {
  return raycast_device(c, "mrh_raycast_spherical_device", MRH_CAMERA_SPHERICAL, p, R_row_major, t, RayOut{d_range, d_normals, d_rgb, d_points});
}

}  // extern "C"

// ---- distance fields (include/mrhash_esdf.h, mrh_esdf.h) ---------------------------------------------------------------------
namespace {

// the arguments both entry points share, checked before the map is touched; fills the kernels' box
int esdf_args(mrh_ctx* c, const char* who, const mrh_esdf_params* p, EsdfBox* bx) {
  if (!p) return fail(c, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (c->pending) return fail(c, MRH_ERR_STATE, "%s: an exchange is pending (call mrh_integrate_resume)", who);
  if (c->map.shard_count > 1) return fail(c, MRH_ERR_UNSUPPORTED, "%s: sharded maps have no distance field (shard_count %d)", who, c->map.shard_count);
  for (int a = 0; a < 3; a++) {
    if (p->dims[a] < 1 || p->dims[a] > MRH_ESDF_MAX_SIDE)
      return fail(c, MRH_ERR_INVALID_ARG, "%s: box of %d x %d x %d cells (1 .. %d per side)", who, p->dims[0], p->dims[1], p->dims[2], MRH_ESDF_MAX_SIDE);
    const int64_t lo = p->origin[a], hi = lo + p->dims[a] - 1;
    if (lo < -(1ll << 23) || hi >= (1ll << 23))
      return fail(c, MRH_ERR_INVALID_ARG, "%s: axis %d of the box spans voxels %lld .. %lld, outside [-2^23, 2^23)", who, a, (long long) lo, (long long) hi);
  }
  if (p->max_distance_voxels < 1 || p->max_distance_voxels > MRH_ESDF_MAX_REACH)
    return fail(c, MRH_ERR_INVALID_ARG, "%s: max_distance_voxels %d (1 .. %d)", who, p->max_distance_voxels, MRH_ESDF_MAX_REACH);
  if (!std::isfinite(p->surface_band) || p->surface_band < 0.f) return fail(c, MRH_ERR_INVALID_ARG, "%s: surface_band %g", who, (double) p->surface_band);
  if (p->min_weight < 0) return fail(c, MRH_ERR_INVALID_ARG, "%s: min_weight %d", who, p->min_weight);
  if (p->outputs & ~(MRH_ESDF_STATE | MRH_ESDF_SQUARED)) return fail(c, MRH_ERR_INVALID_ARG, "%s: unknown output bits 0x%x", who, p->outputs);
  bx->ox = p->origin[0]; bx->oy = p->origin[1]; bx->oz = p->origin[2];
  bx->nx = p->dims[0]; bx->ny = p->dims[1]; bx->nz = p->dims[2];
  bx->reach = (u32) p->max_distance_voxels;
  bx->w_min = std::max(1, p->min_weight ? p->min_weight : c->map.min_weight_threshold);
  bx->band = p->surface_band;
  return MRH_OK;
}

// the scratch of a box of n cells, before its pointers are handed to launch_esdf
int esdf_scratch(mrh_ctx* c, const size_t n) {
  mrh_ctx::Esdf& e = c->esdf;
  if (n <= e.cap) return MRH_OK;  // an earlier mrh_esdf_device may still read the old scratch: regrow_all drains the stream
  return regrow_all(c, e.cap, n, {{e.d_state, n}, {e.d_row, n * sizeof(uint16_t)}, {e.d_plane, n * sizeof(u32)}});
}

// the four launches on the scratch esdf_scratch has sized; out_state (which may be the scratch's own state plane) and out_d2 may be nullptr
int launch_esdf(mrh_ctx* c, const EsdfBox& bx, float* dist, uint8_t* out_state, u32* out_d2) {
  mrh_ctx::Esdf& e = c->esdf;
  hipStream_t s = c->stream;
  const auto bricks = [](const int o, const int len) { return (unsigned) (((o + len - 1) >> 3) - (o >> 3) + 1); };
  const unsigned tiles = (unsigned) ((bx.nx + kEsdfTile - 1) / kEsdfTile);
  k_esdf_classify<<<dim3(bricks(bx.ox, bx.nx), bricks(bx.oy, bx.ny), bricks(bx.oz, bx.nz)), 256, 0, s>>>(c->map, c->tab, bx, e.d_state, dist);
  k_esdf_rows<<<(unsigned) (((size_t) bx.ny * (size_t) bx.nz + 3) / 4), 256, 0, s>>>(bx, e.d_state, e.d_row);
  k_esdf_columns_y<<<dim3(tiles, (unsigned) bx.nz), 256, (size_t) kEsdfTile * (size_t) bx.ny * sizeof(u32), s>>>(bx, e.d_row, e.d_plane);
  k_esdf_columns_z<<<dim3(tiles, (unsigned) bx.ny), 256, (size_t) kEsdfTile * (size_t) bx.nz * sizeof(u32), s>>>(c->map, bx, e.d_plane, e.d_state, dist, out_state, out_d2);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
static_assert((size_t) kEsdfTile * MRH_ESDF_MAX_SIDE * sizeof(u32) <= 65536, "a staged column tile fits the default dynamic LDS limit");
static_assert(kEsdfMaxSide == MRH_ESDF_MAX_SIDE && kEsdfTile * kEsdfColumnLanes == 256, "mrh_esdf.h and mrhash_esdf.h agree");

}  // namespace

extern "C" {

int mrh_esdf(mrh_ctx* c, const mrh_esdf_params* p, const float** out_dist, const uint8_t** out_state, const uint32_t** out_d2) {
  if (!c) return MRH_ERR_INVALID_ARG;
  EsdfBox bx;
  int rc = esdf_args(c, "mrh_esdf", p, &bx);
  if (rc) return rc;
  if ((rc = ensure_ready(c, "mrh_esdf"))) return rc;
  const size_t n = (size_t) bx.nx * (size_t) bx.ny * (size_t) bx.nz;
  mrh_ctx::Esdf& e = c->esdf;
  // results per cell: device dist f32 and d2 u32; pinned [dist f32 | d2 u32 | state u8], each plane contiguous
  if (n > e.out_cap && (rc = regrow_all(c, e.out_cap, n, {{e.d_dist, n * sizeof(float)}, {e.d_d2, n * sizeof(u32)}}))) return rc;
  if ((rc = regrow_pinned(c, e.h_out, e.h_cap, n, n * 9))) return rc;
  if ((rc = esdf_scratch(c, n))) return rc;
  const bool want_s = out_state && (p->outputs & MRH_ESDF_STATE), want_q = out_d2 && (p->outputs & MRH_ESDF_SQUARED);
  if ((rc = launch_esdf(c, bx, e.d_dist, want_s ? e.d_state : nullptr, want_q ? e.d_d2 : nullptr))) return rc;
  char* h_dist = e.h_out; char* h_d2 = e.h_out + n * 4; char* h_state = e.h_out + n * 8;
  if (out_dist) HIP_TRY(c, hipMemcpyAsync(h_dist, e.d_dist, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (want_q) HIP_TRY(c, hipMemcpyAsync(h_d2, e.d_d2, n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  if (want_s) HIP_TRY(c, hipMemcpyAsync(h_state, e.d_state, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out_dist) *out_dist = (const float*) h_dist;
  if (out_state) *out_state = want_s ? (const uint8_t*) h_state : nullptr;
  if (out_d2) *out_d2 = want_q ? (const uint32_t*) h_d2 : nullptr;
  return MRH_OK;
}

int mrh_esdf_device(mrh_ctx* c, const mrh_esdf_params* p, float* d_dist, uint8_t* d_state, uint32_t* d_d2) {
  if (!c) return MRH_ERR_INVALID_ARG;
  EsdfBox bx;
  int rc = esdf_args(c, "mrh_esdf_device", p, &bx);
  if (rc) return rc;
  if (!d_dist) return fail(c, MRH_ERR_INVALID_ARG, "mrh_esdf_device: d_dist is null");
  if ((rc = ensure_ready(c, "mrh_esdf_device"))) return rc;
  if ((rc = esdf_scratch(c, (size_t) bx.nx * (size_t) bx.ny * (size_t) bx.nz))) return rc;
  return launch_esdf(c, bx, d_dist, (p->outputs & MRH_ESDF_STATE) ? d_state : nullptr, (p->outputs & MRH_ESDF_SQUARED) ? (u32*) d_d2 : nullptr);
}

}  // extern "C"

// ---- tracking (include/mrhash_track.h, mrh_track.h, mrh_tracksolve.h) ---------------------------------------------------------
namespace {

// what is tracked: a pinhole depth image of the model's rows x cols (D14) or a cloud of n sensor-frame points against the
// spherical render (D15); on the host (staged through pinned memory) or on the device
struct TrackObs {
  int model;  // MRH_CAMERA_*: the camera model of the model render, and with it the linearisation
  const float* host; const float* dev;
  size_t n;   // points (spherical); a depth image has rows * cols pixels
};

// mrh_track_depth / mrh_track_scan and their device variants: one render of the model through the raycast's own argument check and
// launch, then per iteration the linearisation kernel, k_track_finish, the 256-byte read-back from pinned memory, and solve +
// update on the host (blocks)
int track_run(mrh_ctx* c, const char* who, const mrh_track_params* p, const TrackObs& obs, const float* R0, const float* t0, float* out_R, float* out_t,
              mrh_track_info* out_info) {
  if (!c) return MRH_ERR_INVALID_ARG;
  const bool scan = obs.model == MRH_CAMERA_SPHERICAL;
  if (!p || (!(obs.host || obs.dev) && !(scan && obs.n == 0)) || !out_R || !out_t) return fail(c, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (scan && obs.n > ((size_t) 1 << 24)) return fail(c, MRH_ERR_INVALID_ARG, "%s: %zu points in one scan (limit 2^24)", who, obs.n);
  const mrh_raycast_params rp = {p->fx, p->fy, p->cx, p->cy, p->rows, p->cols, p->min_depth, p->max_depth, p->step,
                                 MRH_RAYCAST_NORMALS | (scan ? MRH_RAYCAST_POINTS : 0u)};
  RayCam rc;
  int rc_ = raycast_args(c, who, obs.model, &rp, R0, t0, &rc);
  if (rc_) return rc_;
  const float dist_max = p->dist_max == 0.f ? std::fmin(2.f * c->p.sdf_truncation, 1.f) : p->dist_max;
  if (!(dist_max > 0.f && dist_max <= 1.f)) return fail(c, MRH_ERR_INVALID_ARG, "%s: the gate must lie in (0, 1] m (dist_max %g)", who, (double) dist_max);
  if (p->iterations < 0 || p->iterations > MRH_TRACK_MAX_ITERATIONS)
    return fail(c, MRH_ERR_INVALID_ARG, "%s: %d iterations (1 .. %d, 0 = 10)", who, p->iterations, MRH_TRACK_MAX_ITERATIONS);
  const int iterations = p->iterations ? p->iterations : 10;
  const uint32_t min_pixels = p->min_pixels ? p->min_pixels : 64u;
  rc_ = ensure_ready(c, who);
  if (rc_) return rc_;
  // the previous call blocked: nothing reads the old buffers
  const size_t npix = (size_t) rc.rows * (size_t) rc.cols;
  const size_t n_obs = scan ? obs.n : npix;  // lanes of a linearisation
  const dim3 grid = scan ? dim3((unsigned) ((n_obs + 255) / 256))
                         : dim3((unsigned) ((rc.cols + kRenderTile - 1) / kRenderTile), (unsigned) ((rc.rows + kRenderTile - 1) / kRenderTile));
  const size_t n_rows = (size_t) grid.x * grid.y;
  double R[9], t[3];
  for (int i = 0; i < 9; i++) R[i] = (double) R0[i];
  for (int i = 0; i < 3; i++) t[i] = (double) t0[i];
  int64_t sums[mrh_track::kSumWords] = {};
  int status = MRH_TRACK_OK, done = 0;
  if (n_obs == 0) status = MRH_TRACK_LOST;  // an empty scan: nothing is rendered or launched
  else {
    if ((rc_ = regrow(c, c->trk.d_img, c->trk.cap, npix, npix * 5 * sizeof(float), false))) return rc_;
    if ((rc_ = regrow(c, c->trk.d_slab, c->trk.slab_cap, n_rows, n_rows * mrh_track::kSumWords * sizeof(i64), false))) return rc_;
    if (!c->trk.h_sums) HIP_TRY(c, pinned_alloc(c, c->trk.h_sums, mrh_track::kSumWords * sizeof(i64)));
    if (scan && (rc_ = regrow(c, c->trk.d_mp, c->trk.mp_cap, npix, npix * 3 * sizeof(float), false))) return rc_;
    float* d_md = (float*) c->trk.d_img;  // the model's depth (range), then its normals
    float* d_mn = d_md + npix;
    const float* d_obs = obs.dev;
    if (!d_obs && scan) {
      const size_t bytes = n_obs * 3 * sizeof(float);
      if ((rc_ = regrow_pinned(c, c->trk.h_cloud, c->trk.h_cloud_cap, n_obs, bytes))) return rc_;
      if ((rc_ = regrow(c, c->trk.d_cloud, c->trk.cloud_cap, n_obs, bytes, false))) return rc_;
      memcpy(c->trk.h_cloud, obs.host, bytes);
      HIP_TRY(c, hipMemcpyAsync(c->trk.d_cloud, c->trk.h_cloud, bytes, hipMemcpyHostToDevice, c->stream));
      d_obs = c->trk.d_cloud;
    } else if (!d_obs) {
      if ((rc_ = regrow_pinned(c, c->trk.h_depth, c->trk.h_cap, npix, npix * sizeof(float)))) return rc_;
      memcpy(c->trk.h_depth, obs.host, npix * sizeof(float));
      HIP_TRY(c, hipMemcpyAsync(d_md + 4 * npix, c->trk.h_depth, npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
      d_obs = d_md + 4 * npix;
    }
    launch_raycast(c, obs.model, rc, RayOut{d_md, d_mn, nullptr, scan ? c->trk.d_mp : nullptr});
    HIP_TRY(c, hipGetLastError());

    TrackLin k;
    k.fx = p->fx; k.fy = p->fy; k.cx = p->cx; k.cy = p->cy; k.ifx = rc.ifx; k.ify = rc.ify;
    k.rows = rc.rows; k.cols = rc.cols;
    k.min_depth = rc.min_depth; k.max_depth = rc.max_depth;
    k.dmax2 = dist_max * dist_max;
    k.s_a = mrh_track::angle_scale(rc.max_depth);
    for (int i = 0; i < 9; i++) k.Rr[i] = R0[i];
    for (int i = 0; i < 3; i++) k.tr[i] = t0[i];
    for (int it = 0; it < iterations; it++) {
      for (int i = 0; i < 9; i++) k.R[i] = (float) R[i];
      for (int i = 0; i < 3; i++) k.t[i] = (float) t[i];
      if (scan) k_track_scan_linearise<<<grid, 256, 0, c->stream>>>(k, d_obs, (unsigned) n_obs, d_md, d_mn, c->trk.d_mp, c->trk.d_slab);
      else k_track_linearise<<<grid, kRenderTile * kRenderTile, 0, c->stream>>>(k, d_obs, d_md, d_mn, c->trk.d_slab);
      k_track_finish<<<1, 1024, 0, c->stream>>>(c->trk.d_slab, (int) n_rows, c->trk.h_sums);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // the last launch wrote the sums into pinned memory
      for (int i = 0; i < mrh_track::kSumWords; i++) sums[i] = (int64_t) ((volatile long long*) c->trk.h_sums)[i];
      double xi[6];
      if (!mrh_track::solve(sums, k.s_a, min_pixels, xi)) {
        status = MRH_TRACK_LOST;
        break;
      }
      mrh_track::update(R, t, xi);
      done++;
    }
  }
  for (int i = 0; i < 9; i++) out_R[i] = (float) R[i];
  for (int i = 0; i < 3; i++) out_t[i] = (float) t[i];
  if (out_info) {
    out_info->status = status;
    out_info->iterations_done = done;
    out_info->pixels = (uint64_t) sums[mrh_track::kSumN];
    out_info->rms = mrh_track::rms(sums);
    for (int i = 0; i < mrh_track::kSumWords; i++) out_info->sums[i] = sums[i];
  }
  return MRH_OK;
}

}  // namespace

extern "C" {

int mrh_track_depth(mrh_ctx* c, const mrh_track_params* p, const float* depth_host, const float R_init[9], const float t_init[3], float out_R[9],
                    float out_t[3], mrh_track_info* out_info) {
  return track_run(c, "mrh_track_depth", p, TrackObs{MRH_CAMERA_PINHOLE, depth_host, nullptr, 0}, R_init, t_init, out_R, out_t, out_info);
}

int mrh_track_depth_device(mrh_ctx* c, const mrh_track_params* p, const float* d_depth, const float R_init[9], const float t_init[3], float out_R[9],
                           float out_t[3], mrh_track_info* out_info) {
  return track_run(c, "mrh_track_depth_device", p, TrackObs{MRH_CAMERA_PINHOLE, nullptr, d_depth, 0}, R_init, t_init, out_R, out_t, out_info);
}

int mrh_track_scan(mrh_ctx* c, const mrh_track_params* p, const float* points_host, size_t n, const float R_init[9], const float t_init[3], float out_R[9],
                   float out_t[3], mrh_track_info* out_info) {
  return track_run(c, "mrh_track_scan", p, TrackObs{MRH_CAMERA_SPHERICAL, points_host, nullptr, n}, R_init, t_init, out_R, out_t, out_info);
}

int mrh_track_scan_device(mrh_ctx* c, const mrh_track_params* p, const float* d_points, size_t n, const float R_init[9], const float t_init[3],
                          float out_R[9], float out_t[3], mrh_track_info* out_info) {
  return track_run(c, "mrh_track_scan_device", p, TrackObs{MRH_CAMERA_SPHERICAL, nullptr, d_points, n}, R_init, t_init, out_R, out_t, out_info);
}

}  // extern "C"

// ---- normal estimation (include/mrhash_normals.h, mrh_normals.h) ------------------------------------------------------------
namespace {

// the parameter block with its defaults filled in, as the kernels take it
int normals_args(mrh_ctx* c, const char* who, const mrh_normals_params* p, const uint64_t n, NrmPar* out) {
  mrh_normals_params q = {0.f, 0u, 0.f, 0.f};
  if (p) q = *p;
  auto bad = [](float v) { return !(v >= 0.f) || !std::isfinite(v); };
  if (bad(q.radius) || bad(q.min_spread) || bad(q.max_flatness) || q.max_flatness >= 1.f)
    return fail(c, MRH_ERR_INVALID_ARG, "%s: bad parameter (radius %g, min_spread %g, max_flatness %g)", who, (double) q.radius, (double) q.min_spread, (double) q.max_flatness);
  if (n >= (1ull << 24)) return fail(c, MRH_ERR_CAPACITY, "%s: %llu points in one scan (limit 2^24 - 1)", who, (unsigned long long) n);
  out->rho = q.radius == 0.f ? 2.0f * c->p.virtual_voxel_size : q.radius;
  if (!(out->rho > 0.f) || !std::isfinite(out->rho)) return fail(c, MRH_ERR_INVALID_ARG, "%s: the cell side must be > 0 (radius %g)", who, (double) out->rho);
  out->min_points = q.min_points == 0u ? 5u : q.min_points;
  const double spread = 1024.0 * (q.min_spread == 0.f ? 0.0625 : (double) q.min_spread);
  out->min_l1 = spread * spread;
  out->max_flat = q.max_flatness == 0.f ? 0.0625 : (double) q.max_flatness;
  return MRH_OK;
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
