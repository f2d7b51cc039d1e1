// mrh_capi.hip — implementation of the C ABI (include/mrhash_hip.h) on top of the gfx950 kernels.
//
// Host side of the thin HIP layer: enqueues the per-frame kernel chain with no host round trip, and only synchronises in the
// calls that hand data back.  Here: the helpers every entry point shares, the entry points, the integrate paths, the splat, raycast
// and normals glue.  The context and its lifetime: mrh_context.h; the copy pool: mrh_hostcopy.h; uploads, frame marks, peeks:
// mrh_upload.h; extraction, scans, block I/O, RCCL: mrh_extract.h, mrh_points.h, mrh_blocks.h, mrh_comm.h.  One translation unit.
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
#include "../../include/mrhash_normals.h"
#include "mrh_kernels.h"
#include "mrh_mc.h"
#include "mrh_raycast.h"
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

// Table upkeep between two frames (mrh_kernels.h): census of the tombstones every `census_period` frames or after a bulk
// change, rebuild decided on the device.  Four short launches, no host round trip.
int maintain_table(mrh_ctx* c, bool force_census) {
  if (c->pending || c->census_period < 0) return MRH_OK;
  if (!force_census && !c->table_dirty && c->frames_since_census < (uint64_t) c->census_period) return MRH_OK;
  hipStream_t s = c->stream;
  const Tab& t = c->tab;
  const int grid = (int) std::min<uint64_t>(2048, (c->slots + 255) / 256);
  k_table_census<<<grid, 256, 0, s>>>(t, (size_t) c->slots);
  k_rehash_decide<<<1, 1, 0, s>>>(t, (u32) (c->slots / 4), c->census_force);
  k_rehash_clear<<<grid, 256, 0, s>>>(t, (size_t) c->slots);
  k_rehash_insert<<<1024, 256, 0, s>>>(t);
  c->frames_since_census = 0;
  c->table_dirty = false;
  HIP_TRY(c, hipGetLastError());
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
  if (c->stream_front) c->front_needs_sync = true;  // whatever this call does to the map, the front stream must see it before its next launch
  c->flushed_since_frame = true;
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

// What every frame — images or a scan — does to the table before its kernels: the upkeep rebuilds from the descriptors, so the
// zombies of the pipelined frames leave first
int frame_upkeep(mrh_ctx* c) {
  if (c->zombies_possible && c->census_period >= 0 && (c->table_dirty || c->frames_since_census >= (uint64_t) c->census_period)) {
    const int rc = strict_point(c);
    if (rc) return rc;
  }
  const int rc = maintain_table(c, false);
  if (rc) return rc;
  c->frames_since_census++;
  return MRH_OK;
}

// coarse free-list refill of a multi-resolution map, decided on the device (vds.cu:885-891, :1048-1054)
void refill_coarse(mrh_ctx* c) {
  k_refill_decide<<<1, 64, 0, c->stream>>>(c->tab, c->low_blocks_to_allocate, c->d_flag);
  k_refill<<<(c->low_blocks_to_allocate + 255) / 256, 256, 0, c->stream>>>(c->tab, c->low_blocks_to_allocate, c->d_flag);
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

int ensure_zbuf(mrh_ctx* c, size_t npix) { return regrow(c, c->d_zbuf, c->zbuf_n, npix, 2 * npix * sizeof(u64)); }

// A starve frame of a single-resolution, unsharded map on the two-launch path: behind the frame's k_back<FREE = false>, the two
// min-passes and the tail (pass 2 + summaries + garbage collection + the other z-buffer pair cleared) — three launches on the main
// stream, nothing of the pipeline flushed.  lz: 2 = a pipelined frame (collected blocks become zombies), 0 = a serial frame.
int launch_starve_fused(mrh_ctx* c, const Cam& k, const Fast& f, const Lists& L, const int set, const float thr, const u32 stamp, const int lz) {
  const size_t npix = (size_t) k.rows * k.cols;
  hipStream_t s = c->stream;
  if (c->zfused_n < npix) {
    c->zfused_clean[0] = c->zfused_clean[1] = false;
    const int rc = regrow(c, c->d_zfused, c->zfused_n, npix, 4 * npix * sizeof(u64));
    if (rc) return rc;
  }
  if (c->zfused_clean_npix != npix) c->zfused_clean[0] = c->zfused_clean[1] = false;  // the camera changed size since the pairs were cleared
  c->zfused_clean_npix = npix;
  const int p = c->zfused_next, q = p ^ 1;
  u64* z0 = c->d_zfused + (size_t) p * 2 * c->zfused_n;
  u64* z1 = z0 + npix;
  u64* other = c->d_zfused + (size_t) q * 2 * c->zfused_n;
  // "empty" = INT64_MAX: above every key (depth bits of a finite positive float < 0x7F800000)
  if (!c->zfused_clean[p]) k_fill_u64<<<256, 256, 0, s>>>(z0, 2 * npix, 0x7FFFFFFFFFFFFFFFull);
  c->zfused_clean[p] = false;
  const int grid = 2048;  // x 4 waves, one block each per round
  if (k.model) {
    k_starve_z<0, true><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L.vis, set, z0, z1);
    k_starve_z<1, true><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L.vis, set, z0, z1);
    if (lz == 2) k_starve_tail<2, true><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L, set, thr, stamp, z0, z1, other, 2 * npix);
    else k_starve_tail<0, true><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L, set, thr, stamp, z0, z1, other, 2 * npix);
  } else {
    k_starve_z<0, false><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L.vis, set, z0, z1);
    k_starve_z<1, false><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L.vis, set, z0, z1);
    if (lz == 2) k_starve_tail<2, false><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L, set, thr, stamp, z0, z1, other, 2 * npix);
    else k_starve_tail<0, false><<<grid, 256, 0, s>>>(k, c->map, c->tab, f, L, set, thr, stamp, z0, z1, other, 2 * npix);
  }
  HIP_TRY(c, hipGetLastError());
  c->zfused_clean[q] = true;
  c->zfused_next = q;
  c->n_starve_fused++;
  return MRH_OK;
}
// may this frame's starve step take the three fused launches?  (tile-sharded maps reduce the z-buffers over the ranks between the
// passes, multi-resolution and general frames walk lists of another kind: they keep k_starve<0,1,2>)
bool starve_fused_ok(const mrh_ctx* c) { return c->starve_fused && c->p.shard_count <= 1 && !c->tab.multi_res && !c->frame_general; }

// one of the three starve passes over the current compact (fast path: visible) list
int launch_starve(mrh_ctx* c, int pass) {
  const Cam& k = c->cam;
  const size_t npix = (size_t) k.rows * k.cols;
  hipStream_t s = c->stream;
  if (pass == 0) {
    int rc = ensure_zbuf(c, npix);
    if (rc) return rc;
    // "empty" = INT64_MAX: above every key (depth bits of a finite positive float < 0x7F800000) in both the
    // unsigned and the signed reading, so shards can be min-reduced as int64
    k_fill_u64<<<256, 256, 0, s>>>(c->d_zbuf, 2 * npix, 0x7FFFFFFFFFFFFFFFull);
    k_starve<0><<<c->integrate_grid, 512, 0, s>>>(k, c->map, c->tab, c->d_zbuf, c->d_zbuf + npix);
  } else if (pass == 1) {
    k_starve<1><<<c->integrate_grid, 512, 0, s>>>(k, c->map, c->tab, c->d_zbuf, c->d_zbuf + npix);
  } else {
    k_starve<2><<<c->integrate_grid, 512, 0, s>>>(k, c->map, c->tab, c->d_zbuf, c->d_zbuf + npix);
  }
  return MRH_OK;
}

// everything of a frame that follows the starve step
int frame_tail(mrh_ctx* c, bool starved, int max_num_frames) {
  hipStream_t s = c->stream;
  const Cam& k = c->cam;
  const Map& m = c->map;
  const Tab& t = c->tab;
  const float thr = m.trunc + m.trunc_scale * k.max_depth;  // getTruncation(camera.maxDepth(), ...), vds.cu:1720
  if (c->frame_general) {  // garbageCollectIdentify + garbageCollectFree over the compact list (vds.cu:1674-1713, :1827-1844)
    if (max_num_frames > 0) {
      k_gc_identify<<<c->integrate_grid, 512, 0, s>>>(t, thr, c->d_decision);
      if (c->profile) k_gc_free<true><<<256, 256, 0, s>>>(t, c->d_decision);
      else k_gc_free<false><<<256, 256, 0, s>>>(t, c->d_decision);
    }
    if (!t.multi_res) c->fast_summaries_stale = true;  // the general kernels do not maintain the fast path's GC summaries
  } else if (!t.multi_res) {
    if (starved) k_summarize_visible<<<1024, 256, 0, s>>>(t, c->fast);  // weights changed: the GC summaries follow the payload
    if (max_num_frames > 0 && !c->frame_gc_inline) {
      const Lists L = {t.compact, c->fast.bbox, c->d_cfree, c->d_zmin, (u32) c->num_blocks};
      k_free_lists<<<256, 256, 0, s>>>(t, c->fast, L, c->frame_parity, thr);
    }
  }
  c->frames++;
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// starve (voxel_data_structures.cpp:139) + the rest of the frame; sharded contexts stop for the host's min-reduction
int starve_and_tail(mrh_ctx* c, int max_num_frames) {
  const bool starve = max_num_frames > 0 && c->frames > 0 && c->frames % (uint64_t) max_num_frames == 0;
  if (starve) {
    int rc = launch_starve(c, 0);
    if (rc) return rc;
    if (c->p.shard_count > 1 && c->comm) {
      // a communicator is attached: the two min-reductions over the shards run on this stream, between the passes —
      // ncclAllReduce(int64, MIN) over xGMI, no host synchronisation, the frame stays one enqueue
      const size_t npix = (size_t) c->cam.rows * c->cam.cols;
      rc = comm_allreduce_zbuf(c, c->d_zbuf, npix);
      if (rc) return rc;
      if ((rc = launch_starve(c, 1))) return rc;
      rc = comm_allreduce_zbuf(c, c->d_zbuf + npix, npix);
      if (rc) return rc;
      if ((rc = launch_starve(c, 2))) return rc;
      return frame_tail(c, starve, max_num_frames);
    }
    if (c->p.shard_count > 1) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      c->pending = 1;
      c->pending_max_frames = max_num_frames;
      return MRH_PENDING_EXCHANGE;
    }
    if ((rc = launch_starve(c, 1))) return rc;
    if ((rc = launch_starve(c, 2))) return rc;
  }
  return frame_tail(c, starve, max_num_frames);
}

}  // namespace

#include "mrh_extract.h"
#include "mrh_points.h"
#include "mrh_blocks.h"
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

// voxel_data_structures.cpp:90-110 VoxelContainer::integrate, as one sync-free kernel chain
static int integrate_frame(mrh_ctx* c, int n_frames_invalidate);

static int integrate_checks(mrh_ctx* c);
static void prewarm_maybe(mrh_ctx* c);
int mrh_integrate(mrh_ctx* c, int n_frames_invalidate) {
  int rc = ensure_device(c, "mrh_integrate");
  if (rc) return rc;
  rc = flush_deferred(c);  // the frame of the previous call: its images have landed meanwhile
  if (rc < 0) return rc;
  // is this a frame of host images whose transfers are still on their way?
  const bool up_d = c->up_depth.cur >= 0 && c->d_depth == c->up_depth.s[c->up_depth.cur].d && !c->up_depth.waited[0] && !c->up_depth.waited[1];
  const bool up_c = c->up_rgb.cur >= 0 && c->d_rgb == c->up_rgb.s[c->up_rgb.cur].d && !c->up_rgb.waited[0] && !c->up_rgb.waited[1];
  if (c->defer_uploads && (up_d || up_c) && c->p.shard_count <= 1 && !c->comm && !c->profile) {
    rc = integrate_checks(c);  // what can be wrong with the call is reported by the call
    if (rc) return rc;
    mrh_ctx::DeferredFrame& d = c->deferred;
    d.on = true;
    d.n_inval = n_frames_invalidate;
    d.cam = c->cam;
    d.d_depth = c->d_depth; d.d_rgb = c->d_rgb;
    d.depth_rows = c->depth_rows; d.depth_cols = c->depth_cols; d.rgb_rows = c->rgb_rows; d.rgb_cols = c->rgb_cols;
    const UpRing* rings[2] = {&c->up_depth, &c->up_rgb};
    for (int i = 0; i < 2; i++) d.ring[i] = {rings[i]->cur, rings[i]->last_copy, {rings[i]->waited[0], rings[i]->waited[1]}};
    return MRH_OK;
  }
  rc = integrate_frame(c, n_frames_invalidate);
  if (rc < 0) return rc;
  const int mrc = mark_frame(c);
  if (!mrc && rc == MRH_OK) prewarm_maybe(c);
  return mrc ? mrc : rc;
}

extern "C++" {
namespace {
// runs the frame mrh_integrate kept back, with the inputs it was issued under; the context's current inputs (the next frame's
// pose and images may have arrived meanwhile) are put back afterwards
int flush_deferred(mrh_ctx* c) {
  mrh_ctx::DeferredFrame& d = c->deferred;
  if (!d.on) return MRH_OK;
  d.on = false;
  UpRing* rings[2] = {&c->up_depth, &c->up_rgb};
  mrh_ctx::DeferredFrame now;
  now.cam = c->cam;
  now.d_depth = c->d_depth; now.d_rgb = c->d_rgb;
  now.depth_rows = c->depth_rows; now.depth_cols = c->depth_cols; now.rgb_rows = c->rgb_rows; now.rgb_cols = c->rgb_cols;
  for (int i = 0; i < 2; i++) now.ring[i] = {rings[i]->cur, rings[i]->last_copy, {rings[i]->waited[0], rings[i]->waited[1]}};
  c->cam = d.cam;
  c->d_depth = d.d_depth; c->d_rgb = d.d_rgb;
  c->depth_rows = d.depth_rows; c->depth_cols = d.depth_cols; c->rgb_rows = d.rgb_rows; c->rgb_cols = d.rgb_cols;
  for (int i = 0; i < 2; i++) { rings[i]->cur = d.ring[i].cur; rings[i]->last_copy = d.ring[i].last_copy; rings[i]->waited[0] = d.ring[i].waited[0]; rings[i]->waited[1] = d.ring[i].waited[1]; }
  int rc = integrate_frame(c, d.n_inval);
  if (rc >= 0) {
    const int mrc = mark_frame(c);
    if (mrc) rc = mrc;
  }
  c->cam = now.cam;
  c->d_depth = now.d_depth; c->d_rgb = now.d_rgb;
  c->depth_rows = now.depth_rows; c->depth_cols = now.depth_cols; c->rgb_rows = now.rgb_rows; c->rgb_cols = now.rgb_cols;
  for (int i = 0; i < 2; i++) {
    rings[i]->cur = now.ring[i].cur;
    if (now.ring[i].last_copy != d.ring[i].last_copy) {  // a newer image of this kind has arrived: its transfer has not been waited for
      rings[i]->last_copy = now.ring[i].last_copy;
      rings[i]->waited[0] = now.ring[i].waited[0]; rings[i]->waited[1] = now.ring[i].waited[1];
    }  // else: the same transfer, and what the frame has waited for stays waited for
  }
  return rc;
}

int take_event_pair(mrh_ctx* c, EvPair& e) {
  if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); return MRH_OK; }
  if (c->ev_pending.size() >= 4096) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int r = drain_events(c);
    if (r) return r;
    e = c->ev_pool.back(); c->ev_pool.pop_back();
    return MRH_OK;
  }
  HIP_TRY(c, event_new(c, e.a, true)); HIP_TRY(c, event_new(c, e.b, true));
  return MRH_OK;
}

// the lists of ring slot i; slot 0's are the context's own (serial frames, the starve passes, frame_tail)
Lists ring_lists(const mrh_ctx* c, const int i) {
  if (i == 0) return Lists{c->tab.compact, c->fast.bbox, c->d_cfree, c->d_zmin, (u32) c->num_blocks};
  return Lists{c->ring_vis[i], c->ring_bbox[i], c->ring_cfree[i], c->ring_zmin[i], (u32) c->num_blocks};
}

// k_back's and k_front's arguments, in the kernels' parameter order (mrh_fast2.h)
struct BackArgs {
  Cam c; Map m; Tab t; Fast f; Lists L;
  int set, zero_set;
  float thr;
  const float* depth_raw; const uint8_t* rgb_raw; u32* deferred;  // the fused multi-resolution frame's re-integration
  u32 want_stamp; int seq;
};
struct FrontArgs {
  Cam c; Map m; Tab t; Fast f; Lists L;
  const float* depth; const uint8_t* rgb;
  int tiles_x, n_tiles; u32 stamp; int set, gc_on; float thr;
  int n_refill, low_blocks_to_allocate; const int* refill_flag;  // the fused multi-resolution frame's coarse-list refill
};

// Profile mode (`ev` given): the event pair is attached to the launch itself (hipExtLaunchKernelGGL), so it holds the kernel's own
// begin / end timestamps — the duration rocprofv3 reports — instead of a hipEventRecord bracket, which adds the dispatch latency of
// a dependent launch (~3.5 us here) to every sample.
template <bool FREE, bool PROFILE, bool MULTI, bool SAFEDIV, int LZ, bool SPH>
void back_as(const int grid, hipStream_t s, const EvPair* ev, const BackArgs& a) {
  const size_t lds = (size_t) 4 * kTileMaxPx * sizeof(uint2);  // one tile per wave
  if (ev) hipExtLaunchKernelGGL((k_back<FREE, PROFILE, MULTI, SAFEDIV, LZ, SPH>), dim3(grid), dim3(256), (uint32_t) lds, s, ev->a, ev->b, 0u,
                                a.c, a.m, a.t, a.f, a.L, a.set, a.zero_set, a.thr, a.depth_raw, a.rgb_raw, a.deferred, a.want_stamp, a.seq);
  else k_back<FREE, PROFILE, MULTI, SAFEDIV, LZ, SPH><<<grid, 256, lds, s>>>(a.c, a.m, a.t, a.f, a.L, a.set, a.zero_set, a.thr, a.depth_raw, a.rgb_raw,
                                                                             a.deferred, a.want_stamp, a.seq);
}
template <bool FREE, bool PROFILE, int LZ>
void back_single_res(const bool safe_div, const bool sph, const int grid, hipStream_t s, const EvPair* ev, const BackArgs& a) {
  if (safe_div && sph) back_as<FREE, PROFILE, false, true, LZ, true>(grid, s, ev, a);
  else if (safe_div) back_as<FREE, PROFILE, false, true, LZ, false>(grid, s, ev, a);
  else if (sph) back_as<FREE, PROFILE, false, false, LZ, true>(grid, s, ev, a);
  else back_as<FREE, PROFILE, false, false, LZ, false>(grid, s, ev, a);
}
// The one launch site of k_back.  The runtime flags, in the kernel's template order, pick one of the instantiations the library
// builds: single-resolution frames FREE x SAFEDIV x LZ (0: serial, 2: pipelined) x SPH, with the roofline counters (PROFILE) on
// the profile launches of the frames that collect inline — a starve frame's profile launch carries its event pair only —; the
// fused multi-resolution frame FREE, MULTI x SAFEDIV (never profiled, pipelined or spherical).
void launch_back(const bool free_, const bool multi, const bool safe_div, const int lz, const bool sph, const int grid, hipStream_t s, const EvPair* ev,
                 const BackArgs& a) {
  if (multi) {
    if (safe_div) back_as<true, false, true, true, 0, false>(grid, s, ev, a);
    else back_as<true, false, true, false, 0, false>(grid, s, ev, a);
  } else if (lz == 2) {
    if (free_ && ev) back_single_res<true, true, 2>(safe_div, sph, grid, s, ev, a);
    else if (free_) back_single_res<true, false, 2>(safe_div, sph, grid, s, ev, a);
    else back_single_res<false, false, 2>(safe_div, sph, grid, s, ev, a);
  } else {
    if (free_ && ev) back_single_res<true, true, 0>(safe_div, sph, grid, s, ev, a);
    else if (free_) back_single_res<true, false, 0>(safe_div, sph, grid, s, ev, a);
    else back_single_res<false, false, 0>(safe_div, sph, grid, s, ev, a);
  }
}

template <bool PROFILE, bool MULTI, bool LAZY, bool SPH>
void front_as(const int grid, hipStream_t s, const EvPair* ev, const FrontArgs& a) {
  if (ev) hipExtLaunchKernelGGL((k_front<PROFILE, MULTI, LAZY, SPH>), dim3(grid), dim3(256), 0, s, ev->a, ev->b, 0u, a.c, a.m, a.t, a.f, a.L, a.depth, a.rgb,
                                a.tiles_x, a.n_tiles, a.stamp, a.set, a.gc_on, a.thr, a.n_refill, a.low_blocks_to_allocate, a.refill_flag);
  else k_front<PROFILE, MULTI, LAZY, SPH><<<grid, 256, 0, s>>>(a.c, a.m, a.t, a.f, a.L, a.depth, a.rgb, a.tiles_x, a.n_tiles, a.stamp, a.set, a.gc_on, a.thr,
                                                               a.n_refill, a.low_blocks_to_allocate, a.refill_flag);
}
template <bool PROFILE>
void front_single_res(const bool lazy, const bool sph, const int grid, hipStream_t s, const EvPair* ev, const FrontArgs& a) {
  if (lazy && sph) front_as<PROFILE, false, true, true>(grid, s, ev, a);
  else if (lazy) front_as<PROFILE, false, true, false>(grid, s, ev, a);
  else if (sph) front_as<PROFILE, false, false, true>(grid, s, ev, a);
  else front_as<PROFILE, false, false, false>(grid, s, ev, a);
}
// The one launch site of k_front: single-resolution frames PROFILE (= a profile launch, `ev` given) x LAZY x SPH, the fused
// multi-resolution frame MULTI alone.
void launch_front(const bool multi, const bool lazy, const bool sph, const int grid, hipStream_t s, const EvPair* ev, const FrontArgs& a) {
  if (multi) front_as<false, true, false, false>(grid, s, nullptr, a);
  else if (ev) front_single_res<true>(lazy, sph, grid, s, ev, a);
  else front_single_res<false>(lazy, sph, grid, s, nullptr, a);
}

// the integration of the oldest pending pipelined frame, behind its front half
int launch_pending(mrh_ctx* c, const bool count_skips = false) {
  if (!c->npend) return MRH_OK;
  const mrh_ctx::PendingBack pb = c->pendq[0];  // the oldest
  for (int i = 1; i < c->npend; i++) c->pendq[i - 1] = c->pendq[i];
  c->npend--;
  hipStream_t s = c->stream;
  const hipError_t q = c->pipe_always_wait ? hipErrorNotReady : hipEventQuery(c->ev_front[pb.ring]);
  if (q == hipErrorNotReady) {
    (void) hipGetLastError();
    HIP_TRY(c, hipStreamWaitEvent(s, c->ev_front[pb.ring], 0));
    c->dbg_waits++;
  } else if (q != hipSuccess) {
    return fail(c, MRH_ERR_DEVICE, "mrh_integrate: front half of a pipelined frame: %s", hipGetErrorString(q));
  }
  const Map& m = c->map;
  const Tab& t = c->tab;
  if (count_skips) HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_ZSKIP], 0, sizeof(int), s));  // mrh_get_stats: M of the last frame, exactly
  if (pb.profile)  // U and M of the frame (device-side counters of the roofline numerator): after its front half, before its integration
    k_count_updates<<<c->fused_grid, 256, 0, s>>>(pb.cam, m, t, pb.f, c->d_cnt_partials, CTR_SET0 + 4 * pb.set, pb.L.vis, pb.L.cfree, pb.stamp, pb.count_zombies ? 1 : 0);
  launch_back(pb.free_, false, pb.safe_div, 2, pb.sph, c->pipe_grid, s, pb.profile ? &pb.ev : nullptr,
              {pb.cam, m, t, pb.f, pb.L, pb.set, pb.zero_set, pb.thr, nullptr, nullptr, nullptr, pb.stamp, pb.seq});
  if (pb.profile) c->ev_pending.push_back(pb.ev);
  if (pb.free_) c->zombies_possible = true;
  if (pb.starve) {
    const int src = launch_starve_fused(c, pb.cam, pb.f, pb.L, pb.set, pb.thr, pb.stamp, 2);
    if (src) return src;
    c->zombies_possible = true;
  }
  HIP_TRY(c, hipGetLastError());
  // the frame's pool report (mark_frame left it to this launch): behind its integration
  return pb.report_seq && c->peek_enabled ? post_report(c, pb.report_seq, s) : MRH_OK;
}

// Behind the pipelined frames issued so far (their integrations are all on the main stream, each behind its front half), the
// zombies nobody wanted leave the table: k_reclaim runs alone on the main stream — the front stream is idle once the last
// integration has started, and nothing is enqueued on it before the host has seen the main stream drain (front_needs_sync).
int strict_point(mrh_ctx* c) {
  while (c->npend) {
    const int rc = launch_pending(c, c->npend == 1);
    if (rc) return rc;
  }
  if (!c->zombies_possible) return MRH_OK;
  k_reclaim<<<64, 256, 0, c->stream>>>(c->tab, c->fast);
  k_reclaim_done<<<1, 1, 0, c->stream>>>(c->tab);
  // the pool report of the newest mark now understates the free list by the zombies that have just left: written again behind the
  // reclaim, so that a peek after mrh_sync (or after any other flush) reads the level the flush left (with the reclaim period at 64
  // frames the difference is no longer a handful of blocks)
  if (c->peek_enabled && c->frame_seq > 1) {
    const uint64_t seq = c->frame_seq - 1;
    if (c->peek_seq[seq % 8] == seq && c->peek_done[seq % 8]) {
      if (const int rc = post_report(c, seq, c->stream)) return rc;
    }
  }
  c->zombies_possible = false;
  c->lazy_run = 0;
  c->front_needs_sync = true;
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// the pipelining state (mrh_ctx::pipe)
int ensure_pipe_state(mrh_ctx* c) {
  if (c->stream_front) return MRH_OK;
  const size_t cap = c->num_blocks;
  // the stream comes last: it is what says "the state exists", and a step that failed is taken again by the next call
  // (hipEventDisableSystemFence on these events — they order two streams of one device — was measured in round 5: no difference)
  for (hipEvent_t& e : c->ev_front) if (!e) HIP_TRY(c, event_new(c, e, false));
  for (int i = 1; i < kPipeRing; i++) {
    if (!c->ring_vis[i]) HIP_TRY(c, dev_alloc(c, c->ring_vis[i], cap * sizeof(int4)));
    if (!c->ring_bbox[i]) HIP_TRY(c, dev_alloc(c, c->ring_bbox[i], cap * sizeof(int4)));
    if (!c->ring_cfree[i]) HIP_TRY(c, dev_alloc(c, c->ring_cfree[i], cap * sizeof(int4)));
    if (!c->ring_zmin[i]) HIP_TRY(c, dev_alloc(c, c->ring_zmin[i], cap * sizeof(float)));
  }
  if (!c->fast.zlist) HIP_TRY(c, dev_alloc(c, c->fast.zlist, cap * sizeof(int4)));
  if (!c->want_ring) HIP_TRY(c, dev_alloc(c, c->want_ring, (size_t) kPipeRing * c->slots * sizeof(u32)));
  HIP_TRY(c, hipMemsetAsync(c->want_ring, 0, (size_t) kPipeRing * c->slots * sizeof(u32), c->stream));  // stamps start at 1
  if (!c->h_levels) HIP_TRY(c, pinned_alloc(c, c->h_levels, 4 * sizeof(int)));
  // (a high-priority front stream, a ring of eight and integrations deferred by two calls were measured: no difference)
  HIP_TRY(c, hipStreamCreateWithFlags(&c->stream_front, hipStreamNonBlocking));
  c->h_levels[0] = (int) c->num_blocks - 1; c->h_levels[1] = 0; c->h_levels[2] = -1;
  c->tab.h_levels = c->h_levels;
  c->front_needs_sync = true;  // the memset above
  return MRH_OK;
}

// Fast::dcx of the two-launch frames, grow-only: one image per ring slot with the pipelining state, slot 0's alone without it
int ensure_frame_dcx(mrh_ctx* c, const size_t npix) {
  if (c->pipe_npix >= npix) return MRH_OK;
  {
    const int rc = strict_point(c);  // the pending integrations read the buffers that are about to go
    if (rc) return rc;
  }
  if (c->stream_front) HIP_TRY(c, hipStreamSynchronize(c->stream_front));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint2*& d : c->pipe_dcx) HIP_TRY(c, dev_free(c, d));
  c->pipe_npix = 0;
  const int n = c->stream_front ? kPipeRing : 1;
  for (int i = 0; i < n; i++) HIP_TRY(c, dev_alloc(c, c->pipe_dcx[i], npix * sizeof(uint2)));
  c->pipe_npix = npix;
  return MRH_OK;
}

// room in the pool, as the last integration launch reported it (a few frames old: the margins are generous).  Pipelining state only.
bool pool_roomy(const mrh_ctx* c) {
  const int64_t free_known = (int64_t) ((volatile int*) c->h_levels)[0] + 1, zombies_known = ((volatile int*) c->h_levels)[1];
  return free_known >= (int64_t) (c->num_blocks / 4) && zombies_known <= (int64_t) (c->num_blocks / 8);
}

// One frame of a single-resolution map (pinhole or spherical camera):
//   pipelined: front stream: k_front<LAZY> (+ event) | main stream: wait for that event, k_back<LZ = 2>.  The front stream never
//              waits for the main one, so this frame's front half runs next to the integration of the frame(s) before it;
//              the host only holds back when it is kPipeRing - 1 frames ahead of the integration that has started.
//   serial:    [k_reclaim] -> k_front -> k_back (-> the starve passes), all on the main stream, no zombies anywhere.
// A serial frame comes with MRH_PIPE=0, after anything else touched the map, every `pipe_period` frames (the reclaim bounds the
// zombies), on starve frames that cannot stay in the pipeline, and while the pool is short of room: zombies hold their pool slots
// until the reclaim, so a pool that is nearly full is fused serially — the reference's accounting, exactly.
int integrate_single_res_frame(mrh_ctx* c, const int max_num_frames, const bool starve_now) {
  int rc = MRH_OK;
  hipStream_t s = c->stream;
  const Cam& k = c->cam;
  const Map& m = c->map;
  const Tab& t = c->tab;
  const size_t npix = (size_t) k.rows * k.cols;
  if (c->pipe) {
    rc = ensure_pipe_state(c);
    if (rc) return rc;
  }
  rc = ensure_frame_dcx(c, npix);
  if (rc) return rc;
  if (c->fast_summaries_stale) {  // a LiDAR scan (general kernels) ran since: rebuild the GC summaries once
    rc = strict_point(c);
    if (rc) return rc;
    k_summarize_all<<<2048, 256, 0, s>>>(t, c->fast);
    c->fast_summaries_stale = false;
    c->front_needs_sync = true;
  }
  const int tiles_x = (k.cols + kRayTile - 1) / kRayTile, tiles_y = (k.rows + kRayTile - 1) / kRayTile;
  const int n_tiles = tiles_x * tiles_y;
  // a caller that synchronises (or asks for statistics, a mesh, ...) after EVERY frame gains nothing from the pipeline and would pay
  // for its flush each time: three frames in a row that found the pipeline flushed switch to serial frames, the first frame that
  // follows another frame directly switches back
  c->sync_streak = c->flushed_since_frame ? c->sync_streak + 1 : 0;
  c->flushed_since_frame = false;
  // images that come from the host (mrh_upload_*) make the frame loop host- and link-bound (staging copy + 2.15 MB over PCIe: ~60 us
  // per frame at 640x480 against ~40 us of GPU work): nothing to gain from overlapping kernels, and the second stream's events
  // only add to the host's bill (measured: 77 us per frame pipelined, 64 serial) — such frames are fused serially unless
  // MRH_PIPE_UPLOADS=1 says otherwise (the test-suite sets it, so that its upload-fed streams exercise the pipeline)
  const bool resident_inputs = c->up_depth.cur < 0 && c->up_rgb.cur < 0;
  // a starve frame stays a frame of the pipeline when its starve step can take the fused launches (round 6; before: every starve
  // frame flushed the pipeline, ran serially and left a host synchronisation in front of the next pipelined frame)
  const bool starve_in_pipe = starve_now && starve_fused_ok(c) && !c->starve_serial;
  const bool lazy = c->pipe && (!starve_now || starve_in_pipe) && pool_roomy(c) && c->lazy_run < c->pipe_period && c->sync_streak < 3 &&
                    (resident_inputs || c->pipe_uploads);
  if (!lazy) {
    rc = strict_point(c);
    if (rc) return rc;
  }
  rc = send_uploads(c, lazy ? c->stream_front : s);  // the raw images are read by the front half
  if (rc) return rc;
  const int seq = (int) (c->pipe_seq & 0x3FFFFFFF);
  const int ring = lazy ? (int) (c->pipe_seq % kPipeRing) : 0;  // a serial frame runs behind everything on the main stream: any slot
  c->pipe_seq++;                                                // is free for it, and the starve passes walk slot 0's lists
  const int set = (int) (c->fast_frames % kListSets), zero_set = (set + kListSets - 1) % kListSets;
  c->frame_parity = set;
  c->fast_frames++;
  c->fast.dcx = c->pipe_dcx[ring];
  c->fast.want = c->want_ring + (size_t) ring * c->slots;  // (no want stamps without the pipelining state: nullptr)
  const Fast f = c->fast;
  const u32 stamp = (u32) ((c->frames + 1) & 0x3FFFFFFFu);
  const float gc_thr = m.trunc + m.trunc_scale * k.max_depth;  // getTruncation(camera.maxDepth(), ...), vds.cu:1720
  const bool safe_div = m.half_vs_two_steps || m.wsum_two_steps;  // the short divisions failed their check at mrh_create
  const bool sph = c->spherical;
  // GC runs inside k_back unless this is a starve frame (the starve step changes weights after the integrate pass)
  c->frame_gc_inline = max_num_frames > 0 && !starve_now;
  const Lists L = ring_lists(c, ring);
  EvPair ev = {nullptr, nullptr}, evf = {nullptr, nullptr};
  if (c->profile) {
    rc = take_event_pair(c, evf);
    if (rc) return rc;
    rc = take_event_pair(c, ev);
    if (rc) return rc;
  }
  const FrontArgs front = {k, m, t, f, L, c->d_depth, c->d_rgb, tiles_x, n_tiles, stamp, set, max_num_frames > 0 ? 1 : 0, gc_thr, 0, 0, nullptr};
  if (lazy) {
    if (c->front_needs_sync) {  // the main stream erased keys / pushed the free list (reclaim, a serial frame, any other entry
      HIP_TRY(c, hipStreamSynchronize(s));  // point) after the front stream last looked: the front half must see all of it
      c->front_needs_sync = false;
      c->pipe_base = c->pipe_seq - 1;
    }
    // ring slot `ring` was last used by frame seq - kPipeRing; its integration is complete once the one after it has started,
    // and that one has also cleared the list-counter set this frame appends to
    {
      const int64_t need = (int64_t) seq - kPipeRing + 2;
      if (need > (int64_t) c->pipe_base) {
        const auto t0 = std::chrono::steady_clock::now();
        while ((int64_t) ((volatile int*) c->h_levels)[2] < need) {
          MRH_CPU_RELAX();
          if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) return fail(c, MRH_ERR_DEVICE, "mrh_integrate: the integration of frame %lld never started", (long long) need);
        }
        c->dbg_spin_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      }
    }
    c->dbg_lazy_frames++;
    const auto t_api = std::chrono::steady_clock::now();
    launch_front(false, true, sph, n_tiles + c->sweep_wgs, c->stream_front, c->profile ? &evf : nullptr, front);
    HIP_TRY(c, hipEventRecord(c->ev_front[ring], c->stream_front));
    if (c->profile) c->ev_pending_front.push_back(evf);
    // the integration of the PREVIOUS pipelined frame goes out now (its front half ran a frame ago: usually no wait), this
    // frame's is left for the next call
    const bool zombies_before = c->zombies_possible;
    while (c->npend >= c->pipe_defer) {
      rc = launch_pending(c);
      if (rc) return rc;
    }
    mrh_ctx::PendingBack& pb = c->pendq[c->npend++];
    pb.on = true;
    pb.cam = k; pb.f = f; pb.L = L;
    pb.set = set; pb.zero_set = zero_set; pb.ring = ring; pb.seq = seq; pb.stamp = stamp; pb.thr = gc_thr;
    pb.free_ = c->frame_gc_inline; pb.profile = c->profile != 0; pb.safe_div = safe_div; pb.sph = sph;
    pb.count_zombies = zombies_before || c->zombies_possible || c->frame_gc_inline;
    pb.starve = starve_now;
    pb.ev = ev;
    pb.report_seq = 0;
    c->last_frame_lazy = true;
    c->lazy_run++;
    c->frames++;  // frame_tail's bookkeeping; nothing else of it applies (GC runs inside the integration)
    c->dbg_api_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_api).count();
    HIP_TRY(c, hipGetLastError());
    return MRH_OK;
  }
  // ---- serial frame, all on the main stream (strict_point above has flushed and reclaimed)
  c->last_frame_lazy = false;
  launch_front(false, false, sph, n_tiles + c->sweep_wgs, s, c->profile ? &evf : nullptr, front);
  if (c->profile) {
    c->ev_pending_front.push_back(evf);
    k_count_updates<<<c->fused_grid, 256, 0, s>>>(k, m, t, f, c->d_cnt_partials, CTR_SET0 + 4 * set, L.vis, L.cfree, stamp, 0);
  }
  launch_back(c->frame_gc_inline, false, safe_div, 0, sph, c->fused_grid, s, c->profile ? &ev : nullptr,
              {k, m, t, f, L, set, zero_set, gc_thr, nullptr, nullptr, nullptr, stamp, seq});
  c->front_needs_sync = true;  // direct frees on the main stream
  if (c->profile) c->ev_pending.push_back(ev);
  if (starve_now && starve_fused_ok(c)) {
    rc = launch_starve_fused(c, k, f, L, set, gc_thr, stamp, 0);
    if (rc) return rc;
    c->frames++;  // frame_tail's bookkeeping: the summaries and the garbage collection ran inside the tail launch
    return MRH_OK;
  }
  return starve_and_tail(c, max_num_frames);
}

// One fused frame of a multi-resolution map, on the main stream: k_front<MULTI> (with the coarse-list refill, vds.cu:885-891),
// k_back<MULTI> (GC inline, the re-integration of what checkVarSDF reallocated), k_mr_tail.
int integrate_fused_mr_frame(mrh_ctx* c, const int max_num_frames) {
  hipStream_t s = c->stream;
  const Cam& k = c->cam;
  const Map& m = c->map;
  const Tab& t = c->tab;
  int rc = ensure_frame_dcx(c, (size_t) k.rows * k.cols);
  if (rc) return rc;
  c->fast.dcx = c->pipe_dcx[0];
  const Fast& f = c->fast;
  const int parity = (int) (c->fast_frames % kListSets), zero_set = (parity + kListSets - 1) % kListSets;  // the frame's list-counter set, and the one to clear
  c->frame_parity = parity;
  c->fast_frames++;
  const u32 stamp = (u32) ((c->frames + 1) & 0x3FFFFFFFu);
  const float gc_thr = m.trunc + m.trunc_scale * k.max_depth;  // getTruncation(camera.maxDepth(), ...), vds.cu:1720
  const Lists L = ring_lists(c, 0);
  const bool safe_div = m.half_vs_two_steps || m.wsum_two_steps;  // the short divisions failed their check at mrh_create
  const int tiles_x = (k.cols + kRayTile - 1) / kRayTile, tiles_y = (k.rows + kRayTile - 1) / kRayTile;
  const int n_tiles = tiles_x * tiles_y;
  if (!c->mr_summaries_valid) {
    k_summarize_all<<<2048, 256, 0, s>>>(t, f);
    c->mr_summaries_valid = true;
  }
  c->frame_gc_inline = true;
  // the coarse-list refill rides in k_front; its test was taken by the previous frame's k_mr_tail unless something else touched
  // the coarse list since (general frames, import, stream-out, reset)
  if (!c->refill_flag_valid) k_refill_decide<<<1, 64, 0, s>>>(t, c->low_blocks_to_allocate, c->d_flag);
  const int n_refill = (c->low_blocks_to_allocate + 255) / 256;
  launch_front(true, false, false, n_tiles + c->sweep_wgs_mr + n_refill, s, nullptr,
               {k, m, t, f, L, c->d_depth, c->d_rgb, tiles_x, n_tiles, stamp, parity, 1, gc_thr, n_refill, c->low_blocks_to_allocate, c->d_flag});
  launch_back(true, true, safe_div, 0, false, c->fused_grid, s, nullptr,
              {k, m, t, f, L, parity, zero_set, gc_thr, c->d_depth, c->d_rgb, (u32*) c->d_reint, 0u, 0});
  k_mr_tail<<<1, 256, 0, s>>>(t, (const u32*) c->d_reint, c->low_blocks_to_allocate, c->d_flag);
  rc = starve_and_tail(c, max_num_frames);
  c->refill_flag_valid = rc == MRH_OK;
  return rc;
}

// One frame of a multi-resolution map through the general kernels (mrh_kernels.h), on the main stream.
int integrate_general_frame(mrh_ctx* c, const int max_num_frames) {
  hipStream_t s = c->stream;
  const Cam& k = c->cam;
  const Map& m = c->map;
  const Tab& t = c->tab;
  refill_coarse(c);
  // the image every kernel below reads as "depth": the raw image (pinhole: cloud z == depth, cleaned on the fly) or, for
  // the spherical model, getDepth(cloud) computed once per frame
  const float* depth_img = c->d_depth;
  if (c->spherical) {
    const size_t npix = (size_t) k.rows * k.cols;
    const int rc = regrow(c, c->d_cloud, c->cloud_n, npix, npix * sizeof(float));
    if (rc) return rc;
    k_cloud_depth<<<(int) ((npix + 255) / 256), 256, 0, s>>>(k, c->d_depth, c->d_cloud);
    depth_img = c->d_cloud;
  }
  const dim3 tiles((k.cols + kTile - 1) / kTile, (k.rows + kTile - 1) / kTile);
  if (c->profile) k_alloc<true><<<tiles, dim3(kTile, kTile), 0, s>>>(k, m, t, depth_img);
  else k_alloc<false><<<tiles, dim3(kTile, kTile), 0, s>>>(k, m, t, depth_img);
  k_compact<<<512, 256, 0, s>>>(k, m, t, 1);

  if (c->profile) {
    EvPair ev;
    const int rc = take_event_pair(c, ev);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(ev.a, s));
    k_integrate<true><<<c->integrate_grid, 512, 0, s>>>(k, m, t, depth_img, c->d_rgb, c->d_upd_partials);
    HIP_TRY(c, hipEventRecord(ev.b, s));
    c->ev_pending.push_back(ev);
  } else {
    k_integrate<false><<<c->integrate_grid, 512, 0, s>>>(k, m, t, depth_img, c->d_rgb, c->d_upd_partials);
  }

  if (c->frames > 0) {
    // checkVarSDF -> reallocBlocks -> flatAndReduceHashTable(camera) -> reintegrateDepthMap
    HIP_TRY(c, hipMemsetAsync(&t.ctr[CTR_NREALLOC], 0, 2 * sizeof(int), s));  // NREALLOC, NREINT
    k_check_var<<<2048, 64, 0, s>>>(m, t, c->d_realloc);
    k_realloc<<<64, 256, 0, s>>>(t, c->d_realloc, c->d_reint);
    k_compact<<<512, 256, 0, s>>>(k, m, t, 1);
    k_reintegrate<<<1024, 64, 0, s>>>(k, m, t, depth_img, c->d_rgb, c->d_reint);
  }

  return starve_and_tail(c, max_num_frames);
}

}  // namespace
}  // extern "C++"

// what mrh_integrate rejects before it touches the device
static int integrate_checks(mrh_ctx* c) {
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_integrate: an exchange is pending (call mrh_integrate_resume)");
  if (c->halo_upper) return fail(c, MRH_ERR_STATE, "mrh_integrate: halo blocks of other shards are present (call mrh_drop_blocks(MRH_DROP_HALO) after the extraction)");
  if (!c->has_camera) return fail(c, MRH_ERR_STATE, "mrh_integrate: set_camera has not been called");
  if (c->comm && c->p.shard_count > 1) {  // the starve all-reduce runs over the communicator's ranks: they must be this map's shards
    int cr = 0, cw = 1;
    // MRH_COMM_ALLOW_SHARD_MISMATCH=1 is a test hook for one-GPU boxes (a one-rank group reducing the buffer of one of two shards)
    if (!comm_matches_sharding(c, &cr, &cw) && !getenv("MRH_COMM_ALLOW_SHARD_MISMATCH"))
      return fail(c, MRH_ERR_STATE, "mrh_integrate: the context is shard %d of %d, the attached communicator rank %d of %d", c->p.shard_rank, c->p.shard_count, cr, cw);
  }
  if (!c->d_depth || !c->d_rgb) return fail(c, MRH_ERR_STATE, "mrh_integrate: depth and rgb images are required");
  const Cam& k = c->cam;
  if (c->depth_rows != k.rows || c->depth_cols != k.cols || c->rgb_rows != k.rows || c->rgb_cols != k.cols)
    return fail(c, MRH_ERR_INVALID_ARG, "mrh_integrate: image shape does not match the camera");
  return MRH_OK;
}

// see mrh_ctx::prewarm_on
static void prewarm_maybe(mrh_ctx* c) {
  if (!c->prewarm_on || c->prewarm_done || c->frames != 3 || c->n_extractions || c->f64_link || c->mesh_on_host || c->pending) return;
  c->prewarm_done = true;
  int lev = 0;
  if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&lev, &c->tab.ctr[CTR_HEAP_FINE], sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
    (void) hipGetLastError();
    return;
  }
  const uint64_t live = (uint64_t) std::max<int64_t>((int64_t) c->num_blocks - ((int64_t) lev + 1), 0);  // fine slots in use (coarse units live in fine slots)
  const uint64_t nv = live * 64;
  if (nv < 65536) return;  // a mesh this small costs its first extraction next to nothing
  try {
    const size_t nf = (size_t) (nv + nv / 4);  // faces: a little above the vertices (closed surfaces: twice; what is seen of a room: ~1.1 x)
    size_mesh_staging(c, (size_t) nv, nf);
    if (c->stage_ctl.data()) memset(c->stage_ctl.data(), 0, c->stage_ctl.cap * sizeof(u32));  // no epoch, no flag of an earlier life
    c->V.reserve_unpinned((size_t) nv * 3); c->C.reserve_unpinned((size_t) nv * 3);  // never pinned: mapped and faulted in
    c->V32.clear(); c->C32.clear(); c->F.clear(); c->V.clear(); c->C.clear();  // capacity, not content: the getters still answer "no mesh"
  } catch (...) {
    // no memory for it: the first extraction sizes its buffers itself, as it always did
  }
  (void) hipGetLastError();
}

static int integrate_frame(mrh_ctx* c, int n_frames_invalidate) {
  int rc = integrate_checks(c);
  if (rc) return rc;
  const Cam& k = c->cam;
  const int max_num_frames = n_frames_invalidate < 0 ? c->p.n_frames_invalidate_voxels : n_frames_invalidate;
  hipStream_t s = c->stream;
  const Tab& t = c->tab;
  rc = frame_upkeep(c);
  if (rc) return rc;

  // Multi-resolution maps take the same two launches when that is exact: the fused kernel checks the variance of a
  // fine block right after updating it, which covers every block the reference's checkVarSDF can newly decide on —
  // EXCEPT blocks that changed without being checked (frame 0 is never checked, voxel_data_structures.cpp:99; the starve
  // step decrements weights after the check; imported blocks) and are then outside the image on the next frame.  Those
  // frames, and the starve frames themselves, go through the general kernels.
  const bool starve_now = max_num_frames > 0 && c->frames > 0 && c->frames % (uint64_t) max_num_frames == 0;
  c->frame_fused_mr = t.multi_res && c->mr_fused && !c->profile && max_num_frames > 0 && !starve_now && !c->mr_next_general &&
                      c->frames >= 2 && !c->spherical;
  c->frame_general = t.multi_res && !c->frame_fused_mr;  // (a frame of a single-resolution map always takes the two launches)
  if (t.multi_res && !c->frame_fused_mr) {
    c->mr_summaries_valid = false;
    c->mr_next_general = starve_now || c->frames == 0;
    c->refill_flag_valid = false;
  }
  if (max_num_frames > 0 && starve_fused_ok(c) && c->zfused_n < (size_t) k.rows * k.cols) {
    // the z-buffers of the starve frames, both pairs empty, while the context is still allocating (not inside its first starve frame)
    const size_t npix = (size_t) k.rows * k.cols;
    c->zfused_clean[0] = c->zfused_clean[1] = false;
    rc = regrow(c, c->d_zfused, c->zfused_n, npix, 4 * npix * sizeof(u64));
    if (rc) return rc;
    k_fill_u64<<<512, 256, 0, s>>>(c->d_zfused, 4 * npix, 0x7FFFFFFFFFFFFFFFull);
    c->zfused_clean[0] = c->zfused_clean[1] = true;
    c->zfused_clean_npix = npix;
  }
  // the frame's kind: the two launches of a single-resolution map (pipelined or serial), a fused or a general multi-resolution frame
  if (!t.multi_res) return integrate_single_res_frame(c, max_num_frames, starve_now);
  rc = send_uploads(c, s);  // the frame's kernels read the images on the main stream
  if (rc) return rc;
  return c->frame_fused_mr ? integrate_fused_mr_frame(c, max_num_frames) : integrate_general_frame(c, max_num_frames);
}

int mrh_integrate_resume(mrh_ctx* c) {
  int rc = ensure_ready(c, "mrh_integrate_resume");
  if (rc) return rc;
  if (c->pending == 1) {
    launch_starve(c, 1);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->pending = 2;
    return MRH_PENDING_EXCHANGE;
  }
  if (c->pending == 2) {
    launch_starve(c, 2);
    c->pending = 0;
    rc = frame_tail(c, true, c->pending_max_frames);
    if (rc < 0) return rc;
    const int mrc = mark_frame(c);  // the tail's kernels read the frame's images too
    return mrc ? mrc : rc;
  }
  return fail(c, MRH_ERR_STATE, "mrh_integrate_resume: no exchange is pending");
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
  if (fastp && c->h_levels && out->last_compact_blocks >= (uint64_t) h_ctr[CTR_ZSKIP]) out->last_compact_blocks -= (uint64_t) h_ctr[CTR_ZSKIP];  // list entries that were unwanted zombies
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

// the arguments both entry points share, checked before the map is touched; fills the kernel's camera
int raycast_args(mrh_ctx* c, const char* who, const mrh_raycast_params* p, const float* R, const float* t, RayCam* rc) {
  if (!p || !R || !t) return fail(c, MRH_ERR_INVALID_ARG, "%s: null argument", who);
  if (c->pending) return fail(c, MRH_ERR_STATE, "%s: an exchange is pending (call mrh_integrate_resume)", who);
  if (c->map.shard_count > 1) return fail(c, MRH_ERR_UNSUPPORTED, "%s: sharded maps are not rendered (shard_count %d)", who, c->map.shard_count);
  if (p->rows < 1 || p->rows > MRH_RAYCAST_MAX_SIDE || p->cols < 1 || p->cols > MRH_RAYCAST_MAX_SIDE)
    return fail(c, MRH_ERR_INVALID_ARG, "%s: image of %d x %d pixels (1 .. %d per side)", who, p->rows, p->cols, MRH_RAYCAST_MAX_SIDE);
  if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || p->fx == 0.f || p->fy == 0.f || !std::isfinite(p->cx) || !std::isfinite(p->cy))
    return fail(c, MRH_ERR_INVALID_ARG, "%s: bad intrinsics", who);
  if (!(p->min_depth > 0.f) || !(p->max_depth > p->min_depth) || !std::isfinite(p->max_depth))
    return fail(c, MRH_ERR_INVALID_ARG, "%s: need 0 < min_depth < max_depth (got %g, %g)", who, (double) p->min_depth, (double) p->max_depth);
  if (p->outputs & ~(MRH_RAYCAST_NORMALS | MRH_RAYCAST_COLORS)) return fail(c, MRH_ERR_INVALID_ARG, "%s: unknown output bits 0x%x", who, p->outputs);
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
  rc->min_depth = p->min_depth; rc->max_depth = p->max_depth; rc->step = step;
  rc->n_samples = hi;
  for (int i = 0; i < 9; i++) rc->R[i] = R[i];
  for (int i = 0; i < 3; i++) rc->t[i] = t[i];
  return MRH_OK;
}

void launch_raycast(mrh_ctx* c, const RayCam& rc, float* depth, float* normals, uint8_t* rgb) {
  const dim3 grid((unsigned) ((rc.cols + kRenderTile - 1) / kRenderTile), (unsigned) ((rc.rows + kRenderTile - 1) / kRenderTile));
  k_raycast<<<grid, kRenderTile * kRenderTile, 0, c->stream>>>(c->map, c->tab, rc, depth, normals, rgb);
}
}  // namespace

extern "C" {

int mrh_raycast(mrh_ctx* c, const mrh_raycast_params* p, const float R_row_major[9], const float t[3], const float** out_depth,
                const float** out_normals, const uint8_t** out_rgb) {
  if (!c) return MRH_ERR_INVALID_ARG;
  RayCam rc;
  int rc_ = raycast_args(c, "mrh_raycast", p, R_row_major, t, &rc);
  if (rc_) return rc_;
  rc_ = ensure_ready(c, "mrh_raycast");
  if (rc_) return rc_;
  const size_t npix = (size_t) rc.rows * (size_t) rc.cols;
  const size_t bytes = npix * (sizeof(float) * 4 + 3);
  rc_ = regrow(c, c->d_ray, c->ray_cap, npix, bytes, false);  // the previous raycast has finished (it blocked): nothing reads the old buffers
  if (rc_) return rc_;
  if ((rc_ = regrow_pinned(c, c->h_ray, c->h_ray_cap, npix, bytes))) return rc_;
  const bool want_n = out_normals && (p->outputs & MRH_RAYCAST_NORMALS), want_c = out_rgb && (p->outputs & MRH_RAYCAST_COLORS);
  float* d_depth = (float*) c->d_ray;
  float* d_normals = (float*) (c->d_ray + npix * sizeof(float));
  uint8_t* d_rgb = (uint8_t*) (c->d_ray + npix * sizeof(float) * 4);
  launch_raycast(c, rc, out_depth ? d_depth : nullptr, want_n ? d_normals : nullptr, want_c ? d_rgb : nullptr);
  HIP_TRY(c, hipGetLastError());
  if (out_depth) HIP_TRY(c, hipMemcpyAsync(c->h_ray, d_depth, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (want_n) HIP_TRY(c, hipMemcpyAsync(c->h_ray + npix * sizeof(float), d_normals, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (want_c) HIP_TRY(c, hipMemcpyAsync(c->h_ray + npix * sizeof(float) * 4, d_rgb, npix * 3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out_depth) *out_depth = (const float*) c->h_ray;
  if (out_normals) *out_normals = want_n ? (const float*) (c->h_ray + npix * sizeof(float)) : nullptr;
  if (out_rgb) *out_rgb = want_c ? (const uint8_t*) (c->h_ray + npix * sizeof(float) * 4) : nullptr;
  return MRH_OK;
}

int mrh_raycast_device(mrh_ctx* c, const mrh_raycast_params* p, const float R_row_major[9], const float t[3], float* d_depth, float* d_normals,
                       uint8_t* d_rgb) {
  if (!c) return MRH_ERR_INVALID_ARG;
  RayCam rc;
  int rc_ = raycast_args(c, "mrh_raycast_device", p, R_row_major, t, &rc);
  if (rc_) return rc_;
  rc_ = ensure_ready(c, "mrh_raycast_device");
  if (rc_) return rc_;
  launch_raycast(c, rc, d_depth, (p->outputs & MRH_RAYCAST_NORMALS) ? d_normals : nullptr, (p->outputs & MRH_RAYCAST_COLORS) ? d_rgb : nullptr);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
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
