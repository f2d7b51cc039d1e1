// mrh_capi.hip — implementation of the C ABI (include/mrhash_hip.h) on top of the gfx950 kernels.
//
// Host side of the thin HIP layer: enqueues the per-frame kernel chain with no host round trip, and only synchronises in the
// calls that hand data back.  Here: the helpers every entry point shares; lifetime, camera, pose and uploads; mrh_integrate and
// mrh_integrate_resume, sync and stats; the free-block calls, the peeks and the self-test.
// The context and its lifetime: mrh_context.h; the copy pool: mrh_hostcopy.h; uploads, frame marks, peeks: mrh_upload.h; the
// host side of a depth frame: mrh_frame.h; extraction, scans and their normals, block I/O, splat seeding, RCCL: mrh_extract.h,
// mrh_points.h, mrh_blocks.h, mrh_seeds.h, mrh_comm.h; raycast, distance fields, tracking (rendered and render-free), point and ray queries,
// map-to-map fusion and registration: mrh_readers.h, their argument plans:
// mrh_readerplan.h.  One translation unit.
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
#include "../../include/mrhash_query.h"
#include "../../include/mrhash_rays.h"
#include "../../include/mrhash_freespace.h"
#include "../../include/mrhash_track.h"
#include "../../include/mrhash_align.h"
#include "../../include/mrhash_sdftrack.h"
#include "../../include/mrhash_normals.h"
#include "mrh_kernels.h"
#include "mrh_mc.h"
#include "mrh_raycast.h"
#include "mrh_esdf.h"
#include "mrh_query.h"
#include "mrh_rays.h"
#include "mrh_freespace.h"
#include "mrh_remap.h"
#include "mrh_track.h"
#include "mrh_align.h"
#include "mrh_sdftrack.h"
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
#include "mrh_seeds.h"
#include "mrh_readerplan.h"
#include "mrh_readers.h"
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
  if (c->free.on) HIP_TRY(c, hipMemsetAsync(c->free.d_words, 0, (size_t) c->free.L.n_words * sizeof(u32), c->stream));  // the bits go, the box stays
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
