// mrh_capi.hip — implementation of the C ABI (include/mrhash_hip.h) on top of the gfx950 kernels.
//
// Host side of the thin HIP layer: owns the device buffers, enqueues the per-frame kernel chain on one
// stream with no host round trip, and only synchronises in the calls that hand data back.
// There is NO CPU fallback in this file: without a HIP device mrh_create fails with MRH_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <sys/mman.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#define MRH_CPU_RELAX() _mm_pause()
#else
#define MRH_CPU_RELAX() ((void) 0)  // host code as the device pass sees it
#endif

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

constexpr int kPipeRing = 6;  // = mrh::kListSets: frames in flight + 2

namespace {

thread_local std::string g_create_err;

struct EvPair {
  hipEvent_t a, b;
};

struct UpSlot {
  void* h = nullptr;            // pinned staging
  void* d = nullptr;            // device image
  size_t cap = 0;
  hipEvent_t copied = nullptr;  // H2D out of `h` done (copy stream)
  bool copied_rec = false;
  uint64_t last_seq = 0;        // newest frame_done mark of a frame that read `d` (0: none)
};
struct UpRing {
  UpSlot s[3];
  int cur = -1;                 // slot holding the current image; -1: none, or a caller's device pointer
  hipStream_t stream = nullptr; // this ring's copy stream
  hipEvent_t last_copy = nullptr;  // newest copy event of this ring
  bool waited[2] = {false, false}; // ... has been waited for by {main, front} stream
};

// Host result buffer of the blocking calls (triangle soup, V / F / C): grow-only, never zero-filled, PINNED.
// A device-to-host copy into pageable memory is pinned and unpinned by the runtime around every call, page by page: with
// transparent huge pages behind the buffer that is cheap (tools/micro/d2h_paths.hip: 128 MB in 2.4 ms), with 4 KiB pages it
// doubles the copy (30 MB of V / F / C: 0.57 -> 1.5 ms) — and which of the two a malloc'ed buffer gets depends on what the
// process freed before (glibc raises its mmap threshold after the first large free; the next buffer then comes from the heap,
// where MADV_HUGEPAGE does nothing for pages that already exist).  Pinned once, the copy runs at link speed every time, and a
// kernel can write the buffer (k_copy_out).  The pinned memory is an anonymous 2 MiB-aligned mapping advised to huge pages,
// touched, and registered (hipHostRegister): 1.5 ms for 36 MB where hipHostMalloc takes 5-9 ms (tools/micro/pinned_alloc_cost.hip)
// — what a context's FIRST extraction pays.  If the registration is refused the mapping stays as a pageable buffer (dev == nullptr:
// copies go through hipMemcpyAsync).
template <typename T>
struct HostVec {
  T* p = nullptr;    // host pointer
  T* dev = nullptr;  // the same memory as the device sees it (nullptr: not registered)
  bool pin = true;   // false: a plain huge-page mapping the device never touches (V / C doubles, filled by the host's widening)
  size_t n = 0, cap = 0;
  size_t span = 0, head = 0;  // the mapping: its size and the bytes between its base and p
  HostVec() = default;
  HostVec(const HostVec&) = delete;
  HostVec& operator=(const HostVec&) = delete;
  ~HostVec() { release(); }
  void release() {
    if (!p) return;
    if (dev) (void) hipHostUnregister((void*) p);
    (void) munmap((void*) ((char*) p - head), span);
    p = nullptr; dev = nullptr; cap = 0; span = 0; head = 0;
  }
  T* data() { return p; }
  const T* data() const { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  void clear() { n = 0; }
  const T& operator[](size_t i) const { return p[i]; }
  bool pin_pending = false;  // mapped and faulted in by reserve_unpinned, not registered yet: the next resize_discard registers it
  // the mapping alone: mmap + huge-page advice + first touch.  No HIP call — safe on a helper thread next to a frame loop (a
  // hipHostRegister on another thread holds the runtime's lock for its whole 1-2 ms: round 6 measured the frame loop at a quarter
  // of its rate with the registration on a helper thread)
  void map_(const size_t count, const bool touch) {
    release();
    const size_t want = count + count / 8;  // head room: a map that grows a little keeps its buffer
    const size_t bytes = ((want * sizeof(T) + (2u << 20) - 1) >> 21) << 21;
    const size_t sp = bytes + (2u << 20);
    void* m = mmap(nullptr, sp, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) throw std::bad_alloc();
    // the whole span is kept (the unaligned head stays untouched, i.e. unbacked): one munmap releases it
    char* aligned = (char*) (((uintptr_t) m + (2u << 20) - 1) & ~(uintptr_t) ((2u << 20) - 1));
    (void) madvise(aligned, bytes, MADV_HUGEPAGE);
    // fault the pages in (as huge pages) before they are pinned; a buffer the device never sees is faulted in by whoever
    // writes it first — the widening threads, side by side (47 MB of V / C at the driver's workload: zeroing them here, on one
    // thread, was most of a context's first extraction) — unless the prewarm asks for it
    if (touch) for (size_t o = 0; o < bytes; o += 4096) ((volatile char*) aligned)[o] = 0;
    span = sp;
    head = (size_t) (aligned - (char*) m);
    p = (T*) aligned;
    dev = nullptr;
    cap = bytes / sizeof(T);
  }
  void register_() {
    pin_pending = false;
    void* d = nullptr;
    const size_t bytes = cap * sizeof(T);
    if (hipHostRegister((void*) p, bytes, hipHostRegisterDefault) == hipSuccess && hipHostGetDevicePointer(&d, (void*) p, 0) == hipSuccess && d) {
      dev = (T*) d;
    } else {
      (void) hipGetLastError();
      (void) hipHostUnregister((void*) p);
      (void) hipGetLastError();
      dev = nullptr;
    }
  }
  // capacity for `count` elements, faulted in, registration left to the first resize_discard (helper thread: no HIP call)
  void reserve_unpinned(const size_t count) {
    if (count <= cap) return;
    map_(count, true);
    pin_pending = pin;
    n = 0;
  }
  // contents are NOT preserved when the buffer grows
  void resize_discard(size_t count) {
    if (count > cap) {
      map_(count, pin);
      pin_pending = false;
      if (pin) register_();
    } else if (pin_pending) {
      register_();
    }
    n = count;
  }
  void assign(const T* a, const T* b) {
    resize_discard((size_t) (b - a));
    if (n) memcpy(p, a, n * sizeof(T));
  }
};

}  // namespace

struct mrh_ctx {
  mrh_params p;
  int device = 0;
  hipStream_t stream = nullptr;
  Cam cam;
  Map map;
  Tab tab;
  bool has_camera = false;
  bool spherical = false;
  // images.  Host uploads (mrh_upload_depth / _rgb) go through a ring of three slots per image kind — pinned staging +
  // device buffer — on a second stream, so the copy of frame N+1 overlaps the kernels of frame N; the frame's kernels
  // wait for the newest copy event, a slot is rewritten only after the last frame that read it (frame_done event).
  UpRing up_depth, up_rgb;
  // A frame of host images is LAUNCHED one mrh_integrate late (round 5): by then its two transfers have completed and the frame's
  // kernels need no cross-stream wait — a wait that is enqueued while its event is still pending costs the waiting stream ~6 us
  // of idle time, and a host-fed frame had two of them in front of its 41 us of kernels.  mrh_integrate checks what it can,
  // keeps {pose, image pointers, ring state} and returns; the next mrh_integrate — or whichever other entry point needs the map
  // (ensure_ready) — runs the frame first, with those inputs swapped in.  MRH_DEFER_UPLOADS=0 launches at once.
  struct DeferredFrame {
    bool on = false;
    int n_inval = 0;
    Cam cam;
    const float* d_depth = nullptr; const uint8_t* d_rgb = nullptr;
    int depth_rows = 0, depth_cols = 0, rgb_rows = 0, rgb_cols = 0;
    struct Ring { int cur; hipEvent_t last_copy; bool waited[2]; } ring[2];
  } deferred;
  int defer_uploads = 1;
  bool copy_ready = false;             // copy stream and frame marks exist
  hipEvent_t frame_done[8] = {};       // recorded behind the kernels that READ a frame's ring slots (front stream for a pipelined frame): slot reuse
  hipEvent_t peek_done[8] = {};        // recorded on the main stream behind the k_report of a mark: what the non-blocking peeks query
  uint64_t frame_seq = 1;
  // pool level for the host without a read-back stall (mrh_peek_free_blocks): a 2-int D2H per frame into pinned memory
  int* h_peek = nullptr;               // [8][8] pinned: ctr[0 .. 4] = free-list levels ... error flags per report
  // grow-only device scratch of the extraction (0: block list / counts / per-voxel counts, 1: mesh post-process, 2: V / C / F):
  // a mesh of a million triangles needs ~400 MB of temporaries, and hipMalloc + hipFree of those cost more than the kernels
  void* arena[3] = {nullptr, nullptr, nullptr};
  size_t arena_cap[3] = {0, 0, 0};
  uint64_t peek_seq[8] = {};
  bool peek_enabled = false;
  const float* d_depth = nullptr;
  const uint8_t* d_rgb = nullptr;
  int depth_rows = 0, depth_cols = 0, rgb_rows = 0, rgb_cols = 0;
  // scratch
  u32* d_decision = nullptr;
  u64* d_zbuf = nullptr;  // 2 * npix
  size_t zbuf_n = 0;
  // starve frames on the two-launch path (mrh_fast2.h: k_starve_z / k_starve_tail): two PAIRS of z-buffers, the tail launch of
  // one starve frame puts the other pair back to "empty" for the next
  u64* d_zfused = nullptr;  // 2 pairs x 2 x npix
  size_t zfused_n = 0;
  bool zfused_clean[2] = {false, false};
  size_t zfused_clean_npix = 0;  // the image size the clean pairs were cleared for (a pair holds zbuf0 | zbuf1 at THAT size)
  int zfused_next = 0;
  bool starve_fused = true;  // MRH_STARVE_FUSED=0: the eight launches of rounds 1-5 (k_starve<0,1,2>, k_summarize_visible, k_free_lists)
  bool starve_serial = false;  // MRH_STARVE_SERIAL=1: starve frames leave the pipeline (and keep the three fused launches)
  uint64_t n_starve_fused = 0;
  int4* d_realloc = nullptr;
  int4* d_reint = nullptr;
  int* d_flag = nullptr;
  u64* d_upd_partials = nullptr;
  u32* d_misc = nullptr;  // 4 words for k_get_voxel
  float* d_rcp_w = nullptr;  // Fast::rcp_w
  Fast fast;              // fast path buffers
  // ---- pipelined frames (integrate_single_res_frame; MRH_PIPE=0: every frame serial, the two launches on the main stream) ----
  // The front half of a frame (k_front<..., LAZY>) is launched on `stream_front`, its integration (k_back<..., LZ = 2>) on the
  // main stream behind one event; the front stream never waits for the main one, so the front half of frame g + 1 runs next to
  // the integration of frame g.  Up to kPipeRing - 1 frames are in flight, each with its own {depth, colour} image, lists,
  // list-counter set and want stamps.  Everything that is not a pipelined frame meets the map only after k_reclaim.
  int pipe = 1;
  int pipe_grid = 1024;                     // workgroups of a pipelined integration: ONE resident generation (4 per CU x 256 CUs).  With 2048 the
                                            // second generation competes with the front half's workgroups for the slots the first one frees: 37.3 against
                                            // 34.8 us per frame (MRH_PIPE_GRID; the serial launch keeps 2048)
  int pipe_uploads = 0;                     // MRH_PIPE_UPLOADS=1: pipeline frames whose images came through mrh_upload_* too
  int pipe_period = 64;                     // the reclaim (and one serial frame) every so many pipelined frames; MRH_PIPE_PERIOD.  (32 until
                                            // round 6: a period boundary costs the pipeline ~60 us, the zombies it bounds are also bounded by the
                                            // pool test below (zombies <= pool / 8); 64 — the census period — gave +4 % at 100 steps, 128 no more)
  bool pipe_always_wait = false;            // MRH_PIPE_ALWAYS_WAIT=1: a pipelined integration always carries its wait packet (A/B)
  // the pipelining state (ensure_pipe_state: a context with `pipe` set, at its first single-resolution frame) — the front stream,
  // its events, ring slots 1 .. kPipeRing - 1, the want stamps, h_levels and Fast::zlist
  hipStream_t stream_front = nullptr;
  hipEvent_t ev_front[kPipeRing] = {};
  uint2* pipe_dcx[kPipeRing] = {};          // {cleaned depth, packed colour} of a frame (written by k_front), per ring slot; without the pipelining
  size_t pipe_npix = 0;                     // state [0] alone, which every serial frame uses (ensure_frame_dcx)
  int4* ring_vis[kPipeRing] = {}; int4* ring_bbox[kPipeRing] = {}; int4* ring_cfree[kPipeRing] = {}; float* ring_zmin[kPipeRing] = {};  // [0]: unused (ring_lists)
  u32* want_ring = nullptr;                 // kPipeRing x slots stamps
  int* h_levels = nullptr;                  // pinned {fine free-list level, zombies, sequence number of the last integration that started}
  uint64_t pipe_seq = 0;                    // single-resolution frames issued (pipelined or not)
  uint64_t pipe_base = 0;                   // every frame below this sequence number is known complete (host synchronised)
  int lazy_run = 0;                         // pipelined frames since the last reclaim
  bool zombies_possible = false;
  bool last_frame_lazy = false;
  bool flushed_since_frame = false;          // an entry point other than the per-frame ones ran since the last frame
  int sync_streak = 0;
  bool front_needs_sync = false;            // the main stream changed the table / free list behind the front stream's back
  // the integration of the newest pipelined frame is enqueued by the NEXT mrh_integrate (or by whichever other entry point comes
  // first): by then its front half has usually finished, the host sees that (hipEventQuery) and the main stream needs no
  // cross-stream wait in front of the launch — such a wait costs ~6 us of idle main stream per frame on this runtime
  struct PendingBack {
    bool on = false;
    Cam cam;
    Fast f;
    Lists L;
    int set = 0, zero_set = 0, ring = 0, seq = 0;
    u32 stamp = 0;
    float thr = 0.f;
    bool free_ = false, profile = false, safe_div = false, count_zombies = false, sph = false;
    bool starve = false;  // a starve frame: behind the integration (which collects nothing) the three fused starve launches
    EvPair ev = {nullptr, nullptr};
    uint64_t report_seq = 0;  // frame mark whose pool report was written before this integration ran (refreshed behind it)
  };
  static constexpr int kPendMax = 3;
  PendingBack pendq[kPendMax];            // oldest first
  int npend = 0;
  int pipe_defer = 1;                     // integrations kept back (MRH_PIPE_DEFER, 1 .. kPendMax - 1): the older a front half, the surer it has finished
  uint64_t dbg_waits = 0;
  double dbg_spin_us = 0, dbg_api_us = 0; uint64_t dbg_lazy_frames = 0;  // MRH_DEBUG: where the host's time in a pipelined frame goes
  int4* d_cfree = nullptr;
  float* d_cloud = nullptr; size_t cloud_n = 0;  // spherical camera: getDepth(cloud) image of the current frame (k_cloud_depth)
  bool frame_general = false;       // this frame ran through the general kernels (mrh_kernels.h): GC by k_gc_identify / k_gc_free
  bool fast_summaries_stale = false;  // single-resolution map: a general frame left Fast::summary behind
  // LiDAR scans (mrh_points.h).  Nothing here is touched by mrh_reset: the counters are zero between scans, buckets_dirty covers a failed one
  struct Lidar {
    // ---- the cloud of the next scan
    float* d_points = nullptr;        // owned copy (mrh_upload_points) ...
    const float* d_points_cur = nullptr;  // ... or the caller's device pointer (mrh_set_points_device)
    size_t points_cap = 0, num_points = 0;
    float* d_normals = nullptr; size_t normals_cap = 0, num_normals = 0;  // one normal per point (mrh_upload_normals, mrh_estimate_normals)
    bool have_cloud = false;          // a scan has been handed over (mrh_upload_points / mrh_set_points_device), n = 0 included
    int layout_hint = 0;    // mrh_set_scan_layout / MRH_SCAN_ROW_LEN: > 0 points per row of the caller's organised scans, 0 find out (host clouds), < 0 none
    int row_len = 0;        // ... of the CURRENT cloud (0: not organised, or not known)
    uint64_t detect_n = 0;  // the look at a host cloud is repeated when the cloud's size changes and every 64th upload (a sensor keeps its layout;
    int detect_len = 0, detect_age = 0;  // the look itself costs the calling thread ~20 us of cache misses, more than the order wins per scan)
    int patch_log2 = 4;     // MRH_SCAN_PATCH_LOG2: columns (log2) of the beam patch a walk workgroup takes from an organised scan; 8 = 256 consecutive points
    // ---- the sorted path (mrh_lidar.h): per-point counts, two (key, sdf) record buffers, the sort's scratch
    u32* d_pt_counts = nullptr; u32* d_pt_offsets = nullptr; size_t pt_cap = 0;
    u32* h_sorted_report = nullptr;   // pinned {hwm, last offset, last count, sequence}: the one report of a sorted scan
    u32 sorted_seq = 0;
    void* d_rec_keys[2] = {nullptr, nullptr}; float* d_rec_vals[2] = {nullptr, nullptr}; size_t rec_cap = 0, rec_key_bytes = 0;
    void* d_sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
    // ---- the voxel buckets (mrh_scan.h): per-voxel counters + block stamps (allocated with the first scan), stash, placed records, chunks
    Scan buckets = {};
    int use_buckets = 1;           // MRH_LIDAR_BUCKETS=0: scans through the sorted records of mrh_lidar.h (cross-check)
    int buckets_scratch = 0;       // the counters and stamps — 0: not tried yet, 1: allocated, -1: do not fit / not applicable (sorted path)
    bool buckets_dirty = false;    // a scan failed half way: the counters are cleared before the next one
    size_t buckets_rec_cap = 0, buckets_wg_cap = 0;
    u32* d_buckets_ctr = nullptr;  // two sets of SC_N counters: a scan zeroes the next one's
    u32 buckets_seq = 0;
    size_t buckets_lds_set = 0;
  } lidar;
  // 3DGS splat seeds (mrh_splat.h): sized for one (image shape, min pixel size)
  size_t qt_cap = 0;  // potential nodes the device buffers below hold (regrow_all); it replaces the QTree once recorded here
  QSum* d_qt_sums = nullptr; u32* d_qt_flags = nullptr; u32* d_qt_unc = nullptr; u64* d_qt_marks = nullptr; u64* d_qt_pos = nullptr;
  mrh_splat_seed* d_qt_parked = nullptr; mrh_qtree_leaf* d_qt_leaves = nullptr;
  // what the caller takes from a seeding call is written by its last launch straight into pinned host memory (a few hundred to a few
  // thousand 20-byte seeds and two counters): one synchronisation, no transfer calls (they were two pageable read-backs, each behind
  // a synchronisation of its own: ~35 of the call's 135 us)
  mrh_splat_seed* h_qt_seeds = nullptr; size_t qt_seed_cap = 0;
  u64* h_qt_out = nullptr;   // [0] totals (leaves | seeds << 32), [1] literal evaluations
  u64* d_qt_misc = nullptr;  // [0] totals (leaves | seeds << 32), [1] uncertain-node counter (low word)
  int qt_literal = 0;        // MRH_QTREE_LITERAL=1: every node error through the reference's summation order (cross-check)
  uint32_t qt_last_literal = 0;
  std::vector<mrh_qtree_leaf> qt_leaves;
  uint64_t qt_n_leaves = 0;            // leaves of the last mrh_splat_seeds, still on the device (d_qt_leaves) until someone asks
  bool qt_leaves_on_host = true;
  int mr_fused = 1;          // MRH_MR_FUSED=0: multi-resolution maps always through the general kernels (mrh_kernels.h)
  bool mr_next_general = true;    // the next multi-resolution frame must take the general path (frame 0 / after a starve frame / after an import)
  bool mr_summaries_valid = false;  // fast.summary / summary_c describe every live block (the general kernels do not maintain them)
  bool frame_fused_mr = false;
  bool refill_flag_valid = false;  // d_flag holds the refill test for the next fused frame (taken by k_mr_tail)
  int mesh_on_host = 0;      // MRH_MESH_HOST=1: mesh post-process with the host restatement instead of mrh_mesh.h
  float* d_zmin = nullptr;   // per visible-list entry (Lists::zmin)
  uint64_t fast_frames = 0;  // fast-path frames issued: parity selects the list-counter set
  int frame_parity = 0;
  u64* d_cnt_partials = nullptr;
  int fused_grid = 2048;  // x 4 waves
  int sweep_wgs_mr = 1024; // the same for multi-resolution maps (9x the descriptors); MRH_SWEEP_WGS_MR
  int sweep_wgs = 128;    // descriptor-sweep workgroups appended to the allocation launch (k_front)
  bool frame_gc_inline = false;
  int integrate_grid = 1024;
  int low_blocks_to_allocate = 0;
  uint64_t num_blocks = 0, slots = 0, max_triangles = 0;
  uint64_t frames = 0;
  int pending = 0;           // sharded starve frames: 1 after pass 0, 2 after pass 1
  int pending_max_frames = 0;
  // mesh (host)
  HostVec<mrh_triangle> tris;   // host copy of the soup: only when the caller of mrh_extract_triangles asks for it
  std::vector<mrh_block_desc> tri_blocks;
  std::vector<uint32_t> tri_counts;
  // ... of the last extraction, still on the device (arena slot 0) until mrh_get_triangle_blocks asks
  int tri_dev_n = 0;
  const int4* d_tri_sorted = nullptr;
  const u32* d_tri_counts = nullptr;
  u64* h_mc = nullptr;  // pinned: triangle total of the extraction in flight
  hipEvent_t ev_mc_total = nullptr;  // ... has landed
  u32* d_mc_recs = nullptr; size_t mc_rec_cap = 0;  // corner records of the count pass (mrh_mc.h McRecords), grow-only
  uint64_t mc_rec_fallbacks = 0;                    // extractions whose records did not fit (emitted by k_mc<emit> instead)
  HostVec<double> V, C;
  HostVec<int32_t> F;
  // V and C cross the link in fp32 (k_stage_out) and are widened by the host while the rest is still on its way (widen_from_staging)
  HostVec<float> V32, C32;     // pinned staging
  HostVec<u32> stage_ctl;      // pinned: [0..5] {vertices, faces, epoch} as three u64, [16..] one flag word per 64 KiB chunk of V32, then of C32
  u32 stage_epoch = 0;
  void* mesh_clean_base = nullptr;  // arena slot 1 as the last extraction left it: the first mesh_clean_words words are 0xFFFFFFFF
  size_t mesh_clean_words = 0;
  // The host side of a context's FIRST extraction — four pinned mappings (mmap + first touch + hipHostRegister: ~0.9 ms for the
  // 20 MB of a 0.5 M-triangle mesh) and the 24 MB of doubles the caller sees — used to be paid inside that call, after a
  // synchronisation that told it the sizes: 2.8 ms where every later extraction takes 0.85, and a one-shot extractMesh (what
  // every runner of the reference does) only ever makes the first.  A context that fuses frames will be asked for its mesh: at
  // the end of its THIRD mrh_integrate — a context is still allocating and warming up there — those buffers are sized from the
  // live blocks (64 vertices a block: twice what the rooms of the benchmarks yield, so a map that keeps growing still fits).
  // The first extraction then finds its staging ready and runs like any other; if the estimate was short, it grows the
  // buffers as before.  Done in the calling thread, once: a helper thread was built first (round 6) and slowed the frame loop
  // by 8 % for as long as it was faulting pages in, at whichever frame it was started.  MRH_PREWARM=0 switches it off.
  bool prewarm_on = true, prewarm_done = false;
  uint64_t n_extractions = 0;
  bool f64_link = false;       // MRH_MESH_F64_LINK=1: V / C widened on the device and copied as doubles (the round-3 path; A/B, tests)
  // profiling
  int profile = 0;
  std::vector<EvPair> ev_pool;
  std::vector<EvPair> ev_pending;
  std::vector<EvPair> ev_pending_front;  // the allocation launch (k_front) of profiled fast-path frames
  float sum_ms = 0.f, last_ms = 0.f;
  uint64_t n_ms = 0;
  float sum_front_ms = 0.f;
  uint64_t n_front_ms = 0;
  uint64_t prev_total_updated = 0, prev_inserted = 0, prev_freed = 0, total_compact = 0;
  uint64_t last_triangles = 0;
  // hash-table upkeep (mrh_kernels.h: k_table_census / k_rehash_*)
  int census_period = 64;          // frames between two censuses; MRH_REHASH_PERIOD
  int census_force = 0;            // MRH_REHASH_FORCE=1: every census rebuilds (tests)
  uint64_t frames_since_census = 0;
  bool table_dirty = false;        // bulk erase / insert since the last census (stream-out, import, drop): census before the next frame
  // device error flags: `flags_seen` = union of everything taken off the device since create / reset (stats),
  // `flags_deferred` = taken but not yet returned to the caller by mrh_sync, `flags_peeked` = already returned by a peek
  u32 flags_seen = 0, flags_deferred = 0, flags_peeked = 0;
  // multi-GPU block exchange
  char* d_pack = nullptr; size_t pack_cap = 0;      // mrh_pack_blocks result (records)
  mrh_triangle* d_soup = nullptr; size_t soup_cap = 0, soup_n = 0;  // triangle soup of the last extraction / run merge (mrh_get_triangles_device)
  int4* d_halo = nullptr; size_t halo_cap = 0, halo_upper = 0;  // blocks brought in by MRH_UNPACK_HALO (upper bound of the device count)
  u32* d_taken = nullptr;
  // marching cubes timing (mrh_stats)
  hipEvent_t mc_ev[4] = {};
  float last_mc_count_ms = 0.f, last_mc_emit_ms = 0.f;
  uint64_t last_mc_blocks = 0;
  // MeshExtractor::merge_mesh_ (mrh_mesh_merge_begin / _end): the soups of the extractions in between, back to back
  bool merge_on = false;
  mrh_triangle* d_acc = nullptr; size_t acc_cap = 0, acc_n = 0;
  // RCCL (mrh_comm.h): the communicator this context is attached to, exchange buffers, phase clocks
  mrh_comm* comm = nullptr;
  char* d_xsend = nullptr; size_t xsend_cap = 0;
  char* d_xrecv = nullptr; size_t xrecv_cap = 0;
  hipEvent_t comm_ev[5] = {};
  mrh_comm_phases comm_phases = {};
  std::vector<EvPair> comm_ev_pool, comm_ev_pending;
  // raycasting (mrh_raycast.h): the images of mrh_raycast, grow-only — device [depth f32 | normals 3 x f32 | rgb 3 x u8] per
  // pixel and the pinned host copy the caller reads
  char* d_ray = nullptr; size_t ray_cap = 0;  // pixels
  char* h_ray = nullptr; size_t h_ray_cap = 0;
  // normal estimation (mrh_normals.h): the cell table (2 slots per point of `cap`), the list of occupied slots and the slot of
  // every point, grow-only; two sets of counters, a scan's last launch zeroes the next one's
  struct Normals {
    NrmTab tab = {};
    size_t cap = 0;                // points the scratch holds
    u64* d_ctr = nullptr;          // [2][NC_N]
    u32 seq = 0;
    bool dirty = false;            // a call failed between its first and its last launch: table and counters are cleared first
    int fold = 1;                  // MRH_NORMALS_FOLD=0: k_normals_accumulate<false> (A/B, tests)
    u64* h_ctr = nullptr;          // pinned [NC_N]: the counters of the last mrh_estimate_normals, copied behind its kernels
    mrh_normals_info info = {};    // ... as the caller sees them; `points` = 0 and info_pending = false: none
    bool info_pending = false;     // h_ctr has not been folded into `info` yet
    float* h_out = nullptr; size_t h_out_cap = 0;  // pinned: what mrh_get_normals hands out
  } nrm;
  std::string err;
};

static int comm_allreduce_zbuf(mrh_ctx* c, mrh::u64* buf, size_t n);  // mrh_comm.h
static void comm_release(mrh_ctx* c);
static bool comm_matches_sharding(const mrh_ctx* c, int* comm_rank, int* comm_world);

namespace {

int fail(mrh_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  else g_create_err = buf;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                                   \
  do {                                                                                                       \
    hipError_t e__ = (expr);                                                                                 \
    if (e__ != hipSuccess) return fail(ctx, MRH_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

// device scratch that is released on every path out of a function (error returns included)
template <typename T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void) hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc((void**) &p, n * sizeof(T)); }
  operator T*() const { return p; }
};

// Grow-only device buffers of the context whose contents are NOT kept.  The old buffers are released before the new ones are
// allocated (the peak is one buffer, not two), behind a drained stream unless the caller knows that nothing reads them
// (sync = false), and `cap` is zero for as long as a pointer is null: an allocation that fails leaves "no buffer, capacity 0",
// never a recorded capacity over a null pointer.  `members` grow together under the one capacity: all of them, or none.
// Sizing — what is compared, head room, what else a grow resets — is the call site's.
struct GrowMember {
  void** p; size_t bytes;
  template <typename T> GrowMember(T*& q, size_t b) : p((void**) &q), bytes(b) {}
};
int regrow_all(mrh_ctx* c, size_t& cap, const size_t cap_new, std::initializer_list<GrowMember> members, const bool sync = true) {
  cap = 0;
  if (sync) HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (const GrowMember& m : members) {
    if (*m.p) HIP_TRY(c, hipFree(*m.p));
    *m.p = nullptr;
  }
  for (const GrowMember& m : members) {
    const hipError_t e = hipMalloc(m.p, m.bytes);
    if (e == hipSuccess) continue;
    for (const GrowMember& f : members) { if (*f.p) (void) hipFree(*f.p); *f.p = nullptr; }
    return fail(c, MRH_ERR_DEVICE, "hipMalloc of %zu bytes failed: %s", m.bytes, hipGetErrorString(e));
  }
  cap = cap_new;
  return MRH_OK;
}
// one buffer of `bytes` bytes recorded as `cap_new`, if `cap_new` does not fit in `cap`
template <typename T>
int regrow(mrh_ctx* c, T*& p, size_t& cap, const size_t cap_new, const size_t bytes, const bool sync = true) {
  return cap_new <= cap ? MRH_OK : regrow_all(c, cap, cap_new, {{p, bytes}}, sync);
}
// ... whose first `keep_bytes` ARE kept (halo list, merge accumulator, exchange buffers): the new buffer first, the copy on the
// context's stream, the old one released behind the drained stream; any step that fails leaves buffer and capacity as they were
template <typename T>
int regrow_keep(mrh_ctx* c, T*& p, size_t& cap, const size_t cap_new, const size_t bytes_new, const size_t keep_bytes) {
  if (cap_new <= cap) return MRH_OK;
  DevBuf<T> grown;  // released on an error return
  HIP_TRY(c, hipMalloc((void**) &grown.p, bytes_new));
  if (p && keep_bytes) HIP_TRY(c, hipMemcpyAsync(grown.p, p, keep_bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::swap(p, grown.p);  // the old buffer goes with `grown`
  cap = cap_new;
  return MRH_OK;
}
// ... and a pinned host buffer the caller reads results from (the call that filled it blocked: no synchronisation), contents not kept
template <typename T>
int regrow_pinned(mrh_ctx* c, T*& p, size_t& cap, const size_t cap_new, const size_t bytes) {
  if (cap_new <= cap) return MRH_OK;
  cap = 0;
  if (p) { (void) hipHostFree(p); p = nullptr; }
  HIP_TRY(c, hipHostMalloc((void**) &p, bytes, hipHostMallocDefault));
  cap = cap_new;
  return MRH_OK;
}

uint64_t next_pow2(uint64_t v) {
  uint64_t r = 1;
  while (r < v) r <<= 1;
  return r;
}

void free_all(mrh_ctx* c) {
  if (!c) return;
  (void) hipSetDevice(c->device);
  for (UpRing* r : {&c->up_depth, &c->up_rgb})
    if (r->stream) { (void) hipStreamSynchronize(r->stream); (void) hipStreamDestroy(r->stream); }
  if (c->stream_front) (void) hipStreamSynchronize(c->stream_front);
  if (c->stream) (void) hipStreamSynchronize(c->stream);
  auto F = [](void* p) { if (p) (void) hipFree(p); };
  F(c->want_ring); F(c->fast.zlist);
  for (int i = 0; i < kPipeRing; i++) { F(c->pipe_dcx[i]); if (i) { F(c->ring_vis[i]); F(c->ring_bbox[i]); F(c->ring_cfree[i]); F(c->ring_zmin[i]); } if (c->ev_front[i]) (void) hipEventDestroy(c->ev_front[i]); }
  if (c->h_levels) (void) hipHostFree(c->h_levels);
  if (c->stream_front) { (void) hipStreamSynchronize(c->stream_front); (void) hipStreamDestroy(c->stream_front); }
  F(c->tab.keys); F(c->tab.vals); F(c->tab.heap_fine); F(c->tab.heap_coarse); F(c->tab.desc_fine); F(c->tab.desc_coarse);
  F(c->tab.pool); F(c->tab.compact); F(c->tab.ctr); F(c->tab.prof);
  for (UpRing* r : {&c->up_depth, &c->up_rgb})
    for (UpSlot& u : r->s) {
      if (u.h) (void) hipHostFree(u.h);
      F(u.d);
      if (u.copied) (void) hipEventDestroy(u.copied);
    }
  for (hipEvent_t e : c->frame_done) if (e) (void) hipEventDestroy(e);
  for (hipEvent_t e : c->peek_done) if (e) (void) hipEventDestroy(e);
  if (c->h_peek) (void) hipHostFree(c->h_peek);
  if (c->h_mc) (void) hipHostFree(c->h_mc);
  if (c->lidar.h_sorted_report) (void) hipHostFree(c->lidar.h_sorted_report);
  for (void* a : c->arena) if (a) (void) hipFree(a);
  F(c->d_decision); F(c->d_zbuf); F(c->d_zfused); F(c->d_realloc); F(c->d_reint); F(c->d_flag);
  F(c->d_upd_partials); F(c->d_misc); F(c->d_rcp_w); F(c->d_cfree); F(c->d_zmin); F(c->lidar.d_points); F(c->lidar.d_pt_counts); F(c->lidar.d_pt_offsets); F(c->lidar.d_rec_keys[0]); F(c->lidar.d_rec_keys[1]); F(c->lidar.d_rec_vals[0]); F(c->lidar.d_rec_vals[1]); F(c->lidar.d_sort_tmp); F(c->lidar.buckets.vcnt); F(c->lidar.buckets.bstamp); F(c->lidar.buckets.st_meta); F(c->lidar.buckets.st_sdf); F(c->lidar.buckets.st_grp); F(c->lidar.buckets.wgdesc); F(c->lidar.buckets.rec); F(c->lidar.buckets.chunks); F(c->lidar.d_buckets_ctr); F(c->fast.summary); F(c->fast.summary_c); F(c->fast.bbox); F(c->d_cnt_partials);
  F(c->d_pack); F(c->d_halo); F(c->d_taken); F(c->d_cloud); F(c->lidar.d_normals); F(c->d_soup); F(c->d_mc_recs);
  for (hipEvent_t e : c->mc_ev) if (e) (void) hipEventDestroy(e);
  if (c->ev_mc_total) (void) hipEventDestroy(c->ev_mc_total);
  comm_release(c);
  F(c->d_xsend); F(c->d_xrecv); F(c->d_acc);
  for (hipEvent_t e : c->comm_ev) if (e) (void) hipEventDestroy(e);
  for (auto& e : c->comm_ev_pool) { (void) hipEventDestroy(e.a); (void) hipEventDestroy(e.b); }
  for (auto& e : c->comm_ev_pending) { (void) hipEventDestroy(e.a); (void) hipEventDestroy(e.b); }
  F(c->d_qt_sums); F(c->d_qt_flags); F(c->d_qt_unc); F(c->d_qt_marks); F(c->d_qt_pos); F(c->d_qt_parked); F(c->d_qt_leaves); F(c->d_qt_misc);
  F(c->d_ray);
  if (c->h_ray) (void) hipHostFree(c->h_ray);
  F(c->nrm.tab.keys); F(c->nrm.tab.sums); F(c->nrm.tab.cell); F(c->nrm.tab.list); F(c->nrm.tab.pt_slot); F(c->nrm.tab.partial); F(c->nrm.d_ctr);
  if (c->nrm.h_ctr) (void) hipHostFree(c->nrm.h_ctr);
  if (c->nrm.h_out) (void) hipHostFree(c->nrm.h_out);
  if (c->h_qt_seeds) (void) hipHostFree(c->h_qt_seeds);
  if (c->h_qt_out) (void) hipHostFree(c->h_qt_out);
  for (int i = 0; i < c->npend; i++) if (c->pendq[i].profile) c->ev_pool.push_back(c->pendq[i].ev);
  c->npend = 0;
  for (auto& e : c->ev_pool) { (void) hipEventDestroy(e.a); (void) hipEventDestroy(e.b); }
  for (auto& e : c->ev_pending) { (void) hipEventDestroy(e.a); (void) hipEventDestroy(e.b); }
  for (auto& e : c->ev_pending_front) { (void) hipEventDestroy(e.a); (void) hipEventDestroy(e.b); }
  if (c->stream) (void) hipStreamDestroy(c->stream);
}

// (re)initialises every device structure to the empty map (voxel_data_structures.cpp:58-87 + ctor counters)
int init_buffers(mrh_ctx* c) {
  hipStream_t s = c->stream;
  c->mr_next_general = true;
  c->refill_flag_valid = false;
  c->mr_summaries_valid = false;
  c->fast_frames = 0;
  if (c->stream_front) HIP_TRY(c, hipStreamSynchronize(c->stream_front));
  for (int i = 0; i < c->npend; i++) if (c->pendq[i].profile) c->ev_pool.push_back(c->pendq[i].ev);
  c->npend = 0;  // a reset map has nothing left to integrate
  c->pipe_seq = 0;
  c->pipe_base = 0;
  c->lazy_run = 0;
  c->zombies_possible = false;
  c->front_needs_sync = false;
  if (c->h_levels) { c->h_levels[0] = (int) c->num_blocks - 1; c->h_levels[1] = 0; c->h_levels[2] = -1; }
  if (c->want_ring) HIP_TRY(c, hipMemsetAsync(c->want_ring, 0, (size_t) kPipeRing * c->slots * sizeof(u32), s));
  const Tab& t = c->tab;
  k_init_table<<<1024, 256, 0, s>>>(t.keys, c->slots);
  k_init_heap<<<1024, 256, 0, s>>>(t.heap_fine, (u32) c->num_blocks, getenv("MRH_DEBUG_HEAP_DESCENDING") ? 1 : 0);
  HIP_TRY(c, hipMemsetAsync(t.vals, 0, c->slots * sizeof(u32), s));
  HIP_TRY(c, hipMemsetAsync(t.desc_fine, 0, c->num_blocks * sizeof(int4), s));
  if (t.multi_res) HIP_TRY(c, hipMemsetAsync(t.desc_coarse, 0, c->num_blocks * 8 * sizeof(int4), s));
  HIP_TRY(c, hipMemsetAsync(t.pool, 0, c->num_blocks * (size_t) kFineBytes, s));
  int h_ctr[CTR_COUNT];
  memset(h_ctr, 0, sizeof h_ctr);
  h_ctr[CTR_HEAP_FINE] = (int) c->num_blocks - 1;  // voxel_data_structures.cuh:91-92
  h_ctr[CTR_HEAP_COARSE] = -1;                     // :94-95
  HIP_TRY(c, hipMemcpyAsync(t.ctr, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(t.prof, 0, PROF_COUNT * sizeof(u64), s));
  HIP_TRY(c, hipMemsetAsync(c->d_upd_partials, 0, (size_t) c->integrate_grid * sizeof(u64), s));
  HIP_TRY(c, hipMemsetAsync(c->d_cnt_partials, 0, (size_t) 32768 * 4 * sizeof(u64), s));
  HIP_TRY(c, hipStreamSynchronize(s));
  c->frames = 0;
  c->frames_since_census = 0;
  c->table_dirty = false;
  c->flags_seen = c->flags_deferred = c->flags_peeked = 0;
  c->halo_upper = 0;
  c->prev_total_updated = c->prev_inserted = c->prev_freed = c->total_compact = 0;
  c->sum_ms = c->last_ms = 0.f;
  c->n_ms = 0;
  c->sum_front_ms = 0.f;
  c->n_front_ms = 0;
  c->tris.clear(); c->V.clear(); c->C.clear(); c->F.clear();
  c->last_triangles = 0;
  return MRH_OK;
}

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
int strict_point(mrh_ctx* c);
// every entry point except the per-frame ones (setters, mrh_integrate, the non-blocking peeks): behind the pipelined frames issued
// so far, the zombies nobody wanted leave the table, so that whatever the call reads, changes or waits for is exactly the map two
// serial launches per frame would have left
int flush_deferred(mrh_ctx* c);
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
  HIP_TRY(c, hipHostMalloc((void**) &c->h_mc, HMC_SLOTS * sizeof(u64), hipHostMallocDefault));
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
  if (p->abi_version != MRH_ABI_VERSION) return fail(nullptr, MRH_ERR_INVALID_ARG, "mrh_create: abi_version mismatch");
  if (!(p->virtual_voxel_size > 0.f)) return fail(nullptr, MRH_ERR_INVALID_ARG, "mrh_create: virtual_voxel_size must be > 0");
  if (!(p->sdf_truncation >= 0.f) || !(p->sdf_truncation_scale >= 0.f))
    return fail(nullptr, MRH_ERR_INVALID_ARG, "mrh_create: sdf_truncation and sdf_truncation_scale must be >= 0");
  if (p->voxel_extents_scale != 0 && p->voxel_extents_scale != 1)
    return fail(nullptr, MRH_ERR_UNSUPPORTED, "mrh_create: voxel_extents_scale != 1 is incoherent in the reference (vhu.cuh:90-92 vs 138-140)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MRH_ERR_NO_DEVICE, "mrh_create: no HIP device visible");
  if (p->device_id < 0 || p->device_id >= ndev) return fail(nullptr, MRH_ERR_INVALID_ARG, "mrh_create: device_id %d out of range (%d devices)", p->device_id, ndev);
  if (p->shard_count > 1 && (p->shard_rank < 0 || p->shard_rank >= p->shard_count))
    return fail(nullptr, MRH_ERR_INVALID_ARG, "mrh_create: shard_rank out of range");

  mrh_ctx* c = new mrh_ctx();
  c->p = *p;
  if (c->p.integration_weight_max == 0) c->p.integration_weight_max = 255;
  if (c->p.voxel_extents_scale == 0) c->p.voxel_extents_scale = 1;
  if (c->p.shard_count < 1) c->p.shard_count = 1;
  c->device = p->device_id;
  memset(&c->tab, 0, sizeof c->tab);
  memset(&c->cam, 0, sizeof c->cam);
#define CREATE_TRY(expr)                                                                                         \
  do {                                                                                                           \
    hipError_t e__ = (expr);                                                                                     \
    if (e__ != hipSuccess) {                                                                                     \
      fail(nullptr, MRH_ERR_DEVICE, "mrh_create: %s failed: %s", #expr, hipGetErrorString(e__));                 \
      free_all(c);                                                                                               \
      delete c;                                                                                                  \
      return MRH_ERR_DEVICE;                                                                                     \
    }                                                                                                            \
  } while (0)
  CREATE_TRY(hipSetDevice(c->device));
  CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));

  // capacities: geowrapper.cpp:37-54 when not given explicitly
  size_t free_b = 0, total_b = 0;
  CREATE_TRY(hipMemGetInfo(&free_b, &total_b));
  const double to_alloc = (double) free_b * 0.70;  // SDFBlocks_ratio
  c->num_blocks = p->num_sdf_blocks ? p->num_sdf_blocks : (uint64_t) ((to_alloc * 0.70) / (12.0 * 512.0));
  if (c->num_blocks >= (1ull << 28)) c->num_blocks = (1ull << 28) - 1;  // 31-bit coarse unit ids
  c->max_triangles = p->max_triangles ? p->max_triangles : (uint64_t) ((to_alloc * 0.25) / 72.0);
  c->slots = next_pow2(p->hash_slots ? p->hash_slots : 4 * c->num_blocks);
  if (c->slots < 1024) c->slots = 1024;
  c->low_blocks_to_allocate = (int) ((float) c->num_blocks * 0.1f);  // voxel_data_structures.cuh:57-61

  Tab& t = c->tab;
  t.slot_mask = (u32) (c->slots - 1);
  t.max_probe = 512;
  t.cap_blocks = (u32) c->num_blocks;
  t.multi_res = p->sdf_var_threshold > 0.f ? 1u : 0u;
  CREATE_TRY(hipMalloc((void**) &t.keys, c->slots * sizeof(u64)));
  CREATE_TRY(hipMalloc((void**) &t.vals, c->slots * sizeof(u32)));
  CREATE_TRY(hipMalloc((void**) &t.heap_fine, (c->num_blocks + 1) * sizeof(u32)));
  CREATE_TRY(hipMalloc((void**) &t.desc_fine, c->num_blocks * sizeof(int4)));
  if (t.multi_res) {
    CREATE_TRY(hipMalloc((void**) &t.heap_coarse, (c->num_blocks * 8 + 9) * sizeof(u32)));
    CREATE_TRY(hipMalloc((void**) &t.desc_coarse, c->num_blocks * 8 * sizeof(int4)));
    CREATE_TRY(hipMalloc((void**) &c->d_realloc, c->num_blocks * sizeof(int4)));
    CREATE_TRY(hipMalloc((void**) &c->d_reint, c->num_blocks * sizeof(int4)));
  }
  CREATE_TRY(hipMalloc((void**) &t.pool, c->num_blocks * (size_t) kFineBytes));
  CREATE_TRY(hipMalloc((void**) &t.compact, c->num_blocks * (t.multi_res ? 9 : 1) * sizeof(int4)));
  CREATE_TRY(hipMalloc((void**) &c->d_decision, c->num_blocks * (t.multi_res ? 9 : 1) * sizeof(u32)));
  CREATE_TRY(hipMalloc((void**) &t.ctr, CTR_COUNT * sizeof(int)));
  CREATE_TRY(hipMalloc((void**) &t.prof, PROF_COUNT * sizeof(u64)));
  CREATE_TRY(hipMalloc((void**) &c->d_flag, sizeof(int)));
  CREATE_TRY(hipMalloc((void**) &c->d_misc, 4 * sizeof(u32)));
  CREATE_TRY(hipMalloc((void**) &c->d_upd_partials, (size_t) c->integrate_grid * sizeof(u64)));
  CREATE_TRY(hipMalloc((void**) &c->d_cnt_partials, (size_t) 32768 * 4 * sizeof(u64)));  // max MRH_FUSED_GRID
  memset(&c->fast, 0, sizeof c->fast);
  CREATE_TRY(hipMalloc((void**) &c->fast.summary, c->num_blocks * sizeof(uint2)));
  c->fast.zlist_cap = (u32) c->num_blocks;
  if (const char* g = getenv("MRH_ZLIST_CAP")) { const int v = atoi(g); if (v > 0 && (uint64_t) v < c->num_blocks) c->fast.zlist_cap = (u32) v; }
  const size_t list_cap = c->num_blocks * (t.multi_res ? 9 : 1);  // visible / free lists may hold coarse units, too
  CREATE_TRY(hipMalloc((void**) &c->fast.bbox, list_cap * sizeof(int4)));
  if (t.multi_res) CREATE_TRY(hipMalloc((void**) &c->fast.summary_c, c->num_blocks * 8 * sizeof(uint2)));
#ifdef MRH_TRACE
  CREATE_TRY(hipMalloc((void**) &c->fast.trace, c->num_blocks * 8 * sizeof(u64)));
  CREATE_TRY(hipMemset(c->fast.trace, 0, c->num_blocks * 8 * sizeof(u64)));
#endif
  CREATE_TRY(hipMalloc((void**) &c->d_cfree, list_cap * sizeof(int4)));
  CREATE_TRY(hipMalloc((void**) &c->d_zmin, list_cap * sizeof(float)));
#undef CREATE_TRY

  Map& m = c->map;
  m.vs = p->virtual_voxel_size;
  m.trunc = p->sdf_truncation;
  m.trunc_scale = p->sdf_truncation_scale;
  m.var_threshold = p->sdf_var_threshold;
  m.mc_threshold = p->marching_cubes_threshold;
  m.weight_sample = p->integration_weight_sample & 0xFF;
  m.weight_max = c->p.integration_weight_max & 0xFF;
  m.min_weight_threshold = p->min_weight_threshold;
  m.shard_rank = c->p.shard_rank;
  m.shard_count = c->p.shard_count;
  m.shard_chunk_log2 = (p->shard_chunk_log2 > 0 && p->shard_chunk_log2 < 16) ? p->shard_chunk_log2 : 3;
  {  // where is voxel -> block an arithmetic shift?  (mrh_device.h: world_to_block_fast)
    const u32 init = 1u << 23;
    u32 first_bad = 0;
    if (hipMemcpy(c->d_misc, &init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) first_bad = 1;
    k_block_shift_limit<<<(1 << 23) / 256, 256, 0, c->stream>>>(m.vs, c->d_misc);
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&first_bad, c->d_misc, sizeof first_bad, hipMemcpyDeviceToHost) != hipSuccess) first_bad = 1;
    int lim = 1;
    while ((u32) (lim << 1) <= first_bad && lim < (1 << 22)) lim <<= 1;  // largest power of two <= first mismatch
    m.block_shift_limit = first_bad <= 1 ? 0 : lim;
    if (getenv("MRH_DEBUG")) fprintf(stderr, "[mrhash_hip] voxel->block is a shift for |v| < %d (first mismatch at %u, voxel size %g)\n", m.block_shift_limit, first_bad, (double) m.vs);
  }

  {  // correctly rounded reciprocals for the short divisions of the running mean (mrh_device.h: div_cr)
    auto rn_reciprocal = [](float b) {  // fp64 quotient, then the nearest of the three neighbouring floats (b * c is exact in fp64)
      const float c0 = (float) (1.0 / (double) b);
      float best = c0;
      double err = std::fabs(1.0 - (double) c0 * (double) b);
      for (float t : {std::nextafter(c0, 0.f), std::nextafter(c0, INFINITY)}) {
        const double e = std::fabs(1.0 - (double) t * (double) b);
        if (e < err) { err = e; best = t; }
      }
      return best;
    };
    // weight sums: the kernels use v_rcp_f32 + one Newton step; for the integers 1 .. 510 that must be RN(1 / w)
    std::vector<float> dev(kRcpWeightEntries, 0.f);
    bool ok = hipMalloc((void**) &c->d_rcp_w, dev.size() * sizeof(float)) == hipSuccess;
    if (ok) {
      k_rcp_weights<<<(kRcpWeightEntries + 255) / 256, 256, 0, c->stream>>>(c->d_rcp_w);
      ok = hipStreamSynchronize(c->stream) == hipSuccess && hipMemcpy(dev.data(), c->d_rcp_w, dev.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    }
    int w_bad = ok ? 0 : 1;
    for (int w = 1; ok && w <= 510; w++) w_bad += dev[w] != rn_reciprocal((float) w);
    m.wsum_two_steps = w_bad ? 1 : 0;
    const float half_vs = m.vs / 2;
    m.r_half_vs = rn_reciprocal(half_vs);
    u32 bad = 1;
    if (hipMemset(c->d_misc, 0, sizeof(u32)) == hipSuccess) {
      k_check_div_cr<<<4096, 256, 0, c->stream>>>(half_vs, m.r_half_vs, c->d_misc);
      if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&bad, c->d_misc, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess) bad = 1;
    }
    m.half_vs_two_steps = bad ? 1 : 0;
    if (const char* g = getenv("MRH_SAFE_DIV")) { if (atoi(g)) m.half_vs_two_steps = 1; }  // force the fallback instantiation (tests)
    if (getenv("MRH_DEBUG")) fprintf(stderr, "[mrhash_hip] division by vs / 2 with one residual step: %u mismatches over the working range -> %s; refined reciprocals of the weight sums: %d not correctly rounded\n", bad, bad ? "two steps" : "one step", w_bad);
  }

  if (const char* g = getenv("MRH_FUSED_GRID")) {  // tuning knob: workgroups (x4 waves) of the fused integrate kernel
    const int v = atoi(g);
    if (v > 0 && v <= 32768) c->fused_grid = v;
  }
  if (const char* g = getenv("MRH_DEFER_UPLOADS")) c->defer_uploads = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_PIPE")) c->pipe = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_STARVE_FUSED")) c->starve_fused = atoi(g) != 0;
  c->starve_serial = getenv("MRH_STARVE_SERIAL") != nullptr;
  c->pipe_always_wait = getenv("MRH_PIPE_ALWAYS_WAIT") != nullptr;
  if (const char* g = getenv("MRH_PREWARM")) c->prewarm_on = atoi(g) != 0;
  if (const char* g = getenv("MRH_PIPE_GRID")) { const int v = atoi(g); if (v > 0 && v <= 32768) c->pipe_grid = v; }
  if (const char* g = getenv("MRH_PIPE_DEFER")) { const int v = atoi(g); if (v >= 1 && v < mrh_ctx::kPendMax) c->pipe_defer = v; }
  if (const char* g = getenv("MRH_PIPE_UPLOADS")) c->pipe_uploads = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_PIPE_PERIOD")) { const int v = atoi(g); if (v > 0) c->pipe_period = v; }
  if (const char* g = getenv("MRH_SWEEP_WGS")) { const int v = atoi(g); if (v > 0 && v <= 4096) c->sweep_wgs = v; }
  if (const char* g = getenv("MRH_MESH_HOST")) c->mesh_on_host = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_MESH_F64_LINK")) c->f64_link = atoi(g) != 0;
  c->V.pin = c->C.pin = c->f64_link;  // fp32 link: the doubles are written by the host only
  if (const char* g = getenv("MRH_QTREE_LITERAL")) c->qt_literal = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_MR_FUSED")) c->mr_fused = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_SCAN_ROW_LEN")) c->lidar.layout_hint = atoi(g);
  if (const char* g = getenv("MRH_SCAN_PATCH_LOG2")) { const int v = atoi(g); if (v >= 0 && v <= 8) c->lidar.patch_log2 = v; }
  if (const char* g = getenv("MRH_LIDAR_BUCKETS")) c->lidar.use_buckets = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_NORMALS_FOLD")) c->nrm.fold = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_SCAN_SEQ_START")) c->lidar.buckets_seq = (u32) strtoul(g, nullptr, 0);  // tests: scans next to the wrap of the block stamps
  if (const char* g = getenv("MRH_REHASH_PERIOD")) { const int v = atoi(g); if (v > 0) c->census_period = v; }
  if (const char* g = getenv("MRH_REHASH_FORCE")) c->census_force = atoi(g) ? 1 : 0;
  if (const char* g = getenv("MRH_REHASH_OFF")) { if (atoi(g)) c->census_period = -1; }  // no upkeep at all (tests: shows what it prevents)
  if (const char* g = getenv("MRH_SWEEP_WGS_MR")) { const int v = atoi(g); if (v > 0 && v <= 4096) c->sweep_wgs_mr = v; }
  int rc = init_buffers(c);
  if (rc != MRH_OK) {
    g_create_err = c->err;
    free_all(c);
    delete c;
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

// Host copy into pinned staging with non-temporal stores: the destination is read next by the DMA engine, not by this
// core, so write-allocating it through the cache only costs bandwidth (tools/micro/staging_copy.hip: 1.2 MB in 28.5 us
// vs 40.9 us with memcpy, cold pageable source).
#if !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2"))) void copy_streaming_avx2(void* dst, const void* src, size_t n) {
  const __m256i* s = (const __m256i*) src;
  __m256i* d = (__m256i*) dst;  // pinned allocations are page-aligned
  const size_t v = n / 32;
  for (size_t i = 0; i < v; i++) _mm256_stream_si256(d + i, _mm256_loadu_si256(s + i));
  _mm_sfence();
  if (n & 31) memcpy((char*) dst + v * 32, (const char*) src + v * 32, n & 31);
}
// floats -> doubles with non-temporal stores (the doubles are read by the caller later, not by this core)
__attribute__((target("avx2"))) void widen_floats_avx2(double* dst, const float* src, size_t n) {
  const size_t v = n / 8;
  for (size_t i = 0; i < v; i++) {
    const __m256 f = _mm256_loadu_ps(src + i * 8);
    _mm256_stream_pd(dst + i * 8, _mm256_cvtps_pd(_mm256_castps256_ps128(f)));
    _mm256_stream_pd(dst + i * 8 + 4, _mm256_cvtps_pd(_mm256_extractf128_ps(f, 1)));
  }
  _mm_sfence();
  for (size_t i = v * 8; i < n; i++) dst[i] = (double) src[i];
}
void widen_floats(double* dst, const float* src, size_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2 && ((uintptr_t) dst & 31) == 0) widen_floats_avx2(dst, src, n);
  else for (size_t i = 0; i < n; i++) dst[i] = (double) src[i];
}
void copy_chunk(void* dst, const void* src, size_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2 && n >= (64u << 10) && ((uintptr_t) dst & 31) == 0) copy_streaming_avx2(dst, src, n);
  else memcpy(dst, src, n);
}

// The setter's copy of a 640x480 frame (1.2 MB depth + 0.9 MB colour) is what bounds the host-input path: one core moves
// it at ~28 GB/s with streaming stores, 75 us per frame against 45 us of GPU work.  A small pool of helper threads shares
// every copy (128 KiB chunks handed out by an atomic counter; the calling thread works too).  The helpers spin for a short
// while after a job, so that in a frame loop the next upload finds them awake, and sleep on a condition variable
// otherwise.  One pool per process, started by the first large upload, MRH_COPY_THREADS=0 turns it off.
struct CopyPool {
  static constexpr size_t kChunk = 128u << 10;
  struct Job {
    std::atomic<char*> dst{nullptr}; std::atomic<const char*> src{nullptr}; std::atomic<size_t> bytes{0}, nchunks{0};
    // widening jobs (widen_from_staging): two parts of `bytes` bytes of floats each, chunk i < nchunks / 2 belongs to part 0;
    // a chunk is taken up when its flag word equals `epoch` (flags == nullptr: at once)
    std::atomic<int> widen{0};
    std::atomic<char*> dst2{nullptr}; std::atomic<const char*> src2{nullptr};
    std::atomic<const volatile uint32_t*> flags{nullptr}, flags2{nullptr};
    std::atomic<uint32_t> epoch{0};
  };
  static constexpr size_t kWidenChunk = 64u << 10;  // = kStageChunk: bytes of floats per flag
  static constexpr size_t kMaxStates = 1u << 16;    // chunks of one widening job that carry a state (beyond: the job waits for every helper)
  std::atomic<int> abort_widen{0};
  std::atomic<int64_t> spin_until_ns{0};  // helpers do not go to sleep before this time (widen_prewake)
  static int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  std::mutex m;
  std::condition_variable cv;
  std::vector<std::thread> threads;
  std::atomic<uint64_t> generation{0};  // bumped once per job, after the job's tickets are out
  // Chunk tickets carry the job they belong to: (generation << 32) | next chunk.  A helper that saw generation g and was
  // descheduled can only ever claim a chunk of job g, and only while job g is unfinished (an unclaimed chunk of g exists):
  // it can neither consume a ticket of a later job nor count a chunk into its `done`.  The descriptor of job g lives in
  // jobs[g & 1], which is rewritten only by job g + 2, i.e. after g and g + 1 have both completed.
  std::atomic<uint64_t> ticket{0};
  std::atomic<size_t> done{0};
  std::atomic<int> sleepers{0};
  // A WIDENING job does not wait for its helpers (round 5): every chunk has a state {0 not done, 2 done}, and when the tickets
  // have run out the submitting thread REDOES whatever is not done after a short grace — the bytes are the same whoever writes
  // them ((double) (float) of pinned staging that nothing rewrites meanwhile) —, so a helper that claimed a chunk and then lost
  // its core costs the call one chunk of work instead of the scheduler's time slice (tools/stress_extract.py: tail of hundreds of
  // ms with the host oversubscribed).  Such a straggler may still be reading the staging and writing the doubles after the call
  // has returned: `inflight` counts the helpers between "about to claim" and "finished", and whoever is about to rewrite the
  // staging, release or regrow the arrays, or publish another job waits for it to reach zero first (quiesce()).
  // Upload jobs (copy()) keep waiting for every chunk: their source is the CALLER's buffer, which is free on return.
  std::atomic<int> inflight{0};
  std::unique_ptr<std::atomic<uint8_t>[]> state{new std::atomic<uint8_t>[kMaxStates]};
  std::atomic<uint64_t> redone{0};  // chunks the submitting thread redid (MRH_DEBUG / tools/stress_extract.py)
  Job jobs[2];
  bool started = false;

  void quiesce() {
    while (inflight.load(std::memory_order_seq_cst) != 0) MRH_CPU_RELAX();
  }
  // claims the next chunk of job g; false: none left (or the tickets belong to another job)
  bool claim(const uint64_t g, const Job& j, size_t& i) {
    uint64_t cur = ticket.load(std::memory_order_acquire);
    for (;;) {
      if ((cur >> 32) != (g & 0xFFFFFFFFull)) return false;  // another job's tickets: not ours to take
      i = (size_t) (cur & 0xFFFFFFFFull);
      if (i >= j.nchunks.load(std::memory_order_relaxed)) return false;
      if (ticket.compare_exchange_weak(cur, cur + 1, std::memory_order_acq_rel, std::memory_order_acquire)) return true;
    }
  }
  void work(const uint64_t g) {  // helpers
    Job& j = jobs[g & 1];
    for (;;) {
      inflight.fetch_add(1, std::memory_order_seq_cst);  // BEFORE the claim: a submitter that sees zero knows nobody holds a chunk
      size_t i;
      if (!claim(g, j, i)) { inflight.fetch_sub(1, std::memory_order_seq_cst); break; }
      // chunk i of job g is ours: nobody rewrites the descriptor before `inflight` is back at zero
      if (j.widen.load(std::memory_order_relaxed)) {
        if (widen_chunk(j, i, nullptr, nullptr) && i < kMaxStates) state[i].store(2, std::memory_order_release);
      } else {
        const size_t off = i * kChunk, len = std::min(kChunk, j.bytes.load(std::memory_order_relaxed) - off);
        copy_chunk(j.dst.load(std::memory_order_relaxed) + off, j.src.load(std::memory_order_relaxed) + off, len);
      }
      done.fetch_add(1, std::memory_order_acq_rel);
      inflight.fetch_sub(1, std::memory_order_seq_cst);
    }
  }
  // has the flag of chunk i of a widening job arrived?
  static bool chunk_landed(const Job& j, const size_t i) {
    const size_t half = j.nchunks.load(std::memory_order_relaxed) / 2;
    const volatile uint32_t* fl = i >= half ? j.flags2.load(std::memory_order_relaxed) : j.flags.load(std::memory_order_relaxed);
    return !fl || fl[i >= half ? i - half : i] == j.epoch.load(std::memory_order_relaxed);
  }
  // one chunk of a widening job; the submitting thread passes `drained` and gives up (abort_widen) when the stream has run dry
  // without the chunk's flag.  false: not widened (given up)
  bool widen_chunk(Job& j, const size_t i, bool (*drained)(void*), void* arg) {
    const size_t half = j.nchunks.load(std::memory_order_relaxed) / 2;
    const int part = i >= half ? 1 : 0;
    const size_t lc = i - (part ? half : 0);
    const volatile uint32_t* fl = part ? j.flags2.load(std::memory_order_relaxed) : j.flags.load(std::memory_order_relaxed);
    if (fl) {
      const uint32_t epoch = j.epoch.load(std::memory_order_relaxed);
      for (uint32_t spins = 1; fl[lc] != epoch; spins++) {
        if (abort_widen.load(std::memory_order_relaxed)) return false;
        MRH_CPU_RELAX();
        if (drained && (spins & 1023u) == 0 && drained(arg)) {
          // the stream has run dry: everything the launch wrote is visible, or about to be — only a flag that stays away is an error
          const int64_t t = now_ns();
          while (fl[lc] != epoch && now_ns() - t < 200000000) MRH_CPU_RELAX();
          if (fl[lc] == epoch) break;
          abort_widen.store(1, std::memory_order_relaxed);
          return false;
        }
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    const size_t bytes = j.bytes.load(std::memory_order_relaxed);
    const size_t off = lc * kWidenChunk, len = std::min(kWidenChunk, bytes - off);
    const float* src = (const float*) ((part ? j.src2.load(std::memory_order_relaxed) : j.src.load(std::memory_order_relaxed)) + off);
    double* dst = (double*) ((part ? j.dst2.load(std::memory_order_relaxed) : j.dst.load(std::memory_order_relaxed)) + 2 * off);
    widen_floats(dst, src, len / sizeof(float));
    return true;
  }
  // both parts of a widening job through the pool (the calling thread works too); false: gave up on a flag
  bool widen(double* const dst[2], const float* const src[2], const volatile uint32_t* const flags[2], const uint32_t epoch, const size_t nfloat,
             bool (*drained)(void*), void* arg) {
    if (!started) start();
    const size_t bytes = nfloat * sizeof(float);
    const size_t per = (bytes + kWidenChunk - 1) / kWidenChunk, nc = 2 * per;
    if (nc == 0) return true;
    quiesce();  // a straggler of the previous widening job still reads its descriptor
    abort_widen.store(0, std::memory_order_relaxed);
    const uint64_t g = generation.load(std::memory_order_relaxed) + 1;  // one submitter at a time (g_copy_mutex)
    Job& j = jobs[g & 1];
    j.dst.store((char*) dst[0], std::memory_order_relaxed); j.src.store((const char*) src[0], std::memory_order_relaxed);
    j.dst2.store((char*) dst[1], std::memory_order_relaxed); j.src2.store((const char*) src[1], std::memory_order_relaxed);
    j.flags.store(flags[0], std::memory_order_relaxed); j.flags2.store(flags[1], std::memory_order_relaxed);
    j.epoch.store(epoch, std::memory_order_relaxed);
    j.bytes.store(bytes, std::memory_order_relaxed); j.nchunks.store(nc, std::memory_order_relaxed);
    j.widen.store(1, std::memory_order_relaxed);
    const bool stateful = nc <= kMaxStates;
    for (size_t i = 0; i < std::min(nc, kMaxStates); i++) state[i].store(0, std::memory_order_relaxed);
    done.store(0, std::memory_order_relaxed);
    ticket.store((g & 0xFFFFFFFFull) << 32, std::memory_order_release);
    generation.store(g, std::memory_order_release);
    if (sleepers.load(std::memory_order_acquire) > 0) { std::lock_guard<std::mutex> lk(m); cv.notify_all(); }
    {  // work(g) with the stream check in the flag wait
      size_t i;
      while (claim(g, j, i)) {
        if (widen_chunk(j, i, drained, arg) && i < kMaxStates) state[i].store(2, std::memory_order_release);
        done.fetch_add(1, std::memory_order_acq_rel);
      }
    }
    if (stateful) {
      // The tickets are out; at most one chunk per helper is still under way.  In chunk order: wait for it while it can still be
      // on its way (the flag has not arrived, or arrived less than a grace of 40 us ago — a chunk is ~10 us of work), then redo it.
      for (size_t i = 0; i < nc && !abort_widen.load(std::memory_order_relaxed); i++) {
        int64_t landed_at = 0;
        uint32_t spins = 0;
        while (state[i].load(std::memory_order_acquire) != 2) {
          if (abort_widen.load(std::memory_order_relaxed)) break;
          if (!chunk_landed(j, i)) {  // nobody can have widened it yet: the wait is for the device (with the stream check)
            if (drained && (++spins & 1023u) == 0 && drained(arg)) {
              const int64_t t = now_ns();
              while (!chunk_landed(j, i) && now_ns() - t < 200000000) MRH_CPU_RELAX();
              if (!chunk_landed(j, i)) { abort_widen.store(1, std::memory_order_relaxed); break; }
            }
            MRH_CPU_RELAX();
            continue;
          }
          const int64_t now = now_ns();
          if (!landed_at) landed_at = now;
          if (now - landed_at > 40000) {  // its helper lost its core (or is slow): the same bytes, written here
            if (widen_chunk(j, i, drained, arg)) { state[i].store(2, std::memory_order_release); redone.fetch_add(1, std::memory_order_relaxed); }
            break;
          }
          MRH_CPU_RELAX();
        }
      }
    } else {
      while (done.load(std::memory_order_acquire) < nc && !abort_widen.load(std::memory_order_relaxed)) MRH_CPU_RELAX();
    }
    // (the descriptor keeps `widen` set: a straggler reads it after this call has returned; the next job rewrites it behind quiesce())
    return abort_widen.load(std::memory_order_relaxed) == 0;
  }
  // wake the helpers now and keep them spinning for a millisecond: a widening job is on its way
  void prewake() {
    if (!started) start();
    spin_until_ns.store(now_ns() + 1500000, std::memory_order_relaxed);
    if (sleepers.load(std::memory_order_acquire) > 0) {
      quiesce();
      const uint64_t g = generation.load(std::memory_order_relaxed) + 1;  // an empty job: nothing to claim
      Job& j = jobs[g & 1];
      j.widen.store(0, std::memory_order_relaxed);
      j.bytes.store(0, std::memory_order_relaxed); j.nchunks.store(0, std::memory_order_relaxed);
      done.store(0, std::memory_order_relaxed);
      ticket.store((g & 0xFFFFFFFFull) << 32, std::memory_order_release);
      generation.store(g, std::memory_order_release);
      std::lock_guard<std::mutex> lk(m); cv.notify_all();
    }
  }
  void helper() {
    uint64_t seen = generation.load(std::memory_order_acquire);
    for (;;) {
      // wait for the next job: spin ~100 us (a frame loop submits every 40-100 us), then sleep
      const auto t0 = std::chrono::steady_clock::now();
      uint64_t g;
      int spins = 0;
      while ((g = generation.load(std::memory_order_acquire)) == seen) {
        MRH_CPU_RELAX();
        if ((++spins & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(150) &&
            now_ns() > spin_until_ns.load(std::memory_order_relaxed)) {
          std::unique_lock<std::mutex> lk(m);
          sleepers.fetch_add(1);
          cv.wait(lk, [&] { return generation.load(std::memory_order_acquire) != seen; });
          sleepers.fetch_sub(1);
        }
      }
      seen = g;
      work(g);
    }
  }
  void start() {
    started = true;
    int n = 3;
    if (const char* e = getenv("MRH_COPY_THREADS")) n = atoi(e);
    const int hw = (int) std::thread::hardware_concurrency();
    if (hw > 0 && n > hw - 1) n = hw - 1;
    for (int i = 0; i < n; i++) {
      threads.emplace_back([this] { helper(); });
      threads.back().detach();  // they sleep on the condition variable when idle; the pool lives as long as the process
    }
  }
  void copy(void* d, const void* s_, size_t n) {
    if (!started) start();
    if (threads.empty() || n < 4 * kChunk) { copy_chunk(d, s_, n); return; }
    quiesce();  // a straggler of a widening job still reads that job's descriptor
    const size_t nc = (n + kChunk - 1) / kChunk;
    const uint64_t g = generation.load(std::memory_order_relaxed) + 1;  // one submitter at a time (g_copy_mutex)
    Job& j = jobs[g & 1];
    j.dst.store((char*) d, std::memory_order_relaxed); j.src.store((const char*) s_, std::memory_order_relaxed);
    j.bytes.store(n, std::memory_order_relaxed); j.nchunks.store(nc, std::memory_order_relaxed);
    j.widen.store(0, std::memory_order_relaxed);
    done.store(0, std::memory_order_relaxed);  // no ticket of an earlier job is outstanding: they all completed before their copy() returned
    ticket.store((g & 0xFFFFFFFFull) << 32, std::memory_order_release);
    generation.store(g, std::memory_order_release);
    if (sleepers.load(std::memory_order_acquire) > 0) { std::lock_guard<std::mutex> lk(m); cv.notify_all(); }
    size_t i;
    while (claim(g, j, i)) {
      const size_t off = i * kChunk, len = std::min(kChunk, n - off);
      copy_chunk((char*) d + off, (const char*) s_ + off, len);
      done.fetch_add(1, std::memory_order_acq_rel);
    }
    while (done.load(std::memory_order_acquire) < nc) MRH_CPU_RELAX();  // the source is the caller's: nobody may still read it on return
  }
};
CopyPool* copy_pool() {
  static CopyPool* pool = new CopyPool();  // never destroyed: detached helpers may still be parked on it at exit
  return pool;
}
std::mutex g_copy_mutex;  // one job at a time (contexts on different host threads share the pool)
void copy_to_staging(void* dst, const void* src, size_t n) {
  std::lock_guard<std::mutex> lk(g_copy_mutex);
  copy_pool()->copy(dst, src, n);
}
bool widen_from_staging(double* const dst[2], const float* const src[2], const volatile u32* const flags[2], u32 epoch, size_t nfloat,
                        bool (*drained)(void*), void* arg) {
  std::lock_guard<std::mutex> lk(g_copy_mutex);
  return copy_pool()->widen(dst, src, flags, epoch, nfloat, drained, arg);
}
void widen_prewake() {
  std::lock_guard<std::mutex> lk(g_copy_mutex);
  copy_pool()->prewake();
}
// no helper is still reading a staging buffer or writing a result array of an earlier widening job (CopyPool: `inflight`)
void widen_quiesce() {
  std::lock_guard<std::mutex> lk(g_copy_mutex);
  copy_pool()->quiesce();
}
uint64_t widen_redone() { return copy_pool()->redone.load(std::memory_order_relaxed); }
#else
void copy_to_staging(void* dst, const void* src, size_t n);
bool widen_from_staging(double* const dst[2], const float* const src[2], const volatile u32* const flags[2], u32 epoch, size_t nfloat,
                        bool (*drained)(void*), void* arg) { return false; }
void widen_prewake() {}
void widen_quiesce() {}
uint64_t widen_redone() { return 0; }
#endif

// one host image into the next slot of its ring: wait until the slot is free, copy into pinned staging (the caller's
// buffer is free on return), enqueue the H2D on the copy stream
int upload_image(mrh_ctx* c, UpRing& ring, const void* src, const size_t bytes, const void** out_dev) {
  if (!c->copy_ready) {
    // One copy stream per image kind: the depth and the colour image of a frame then move through two SDMA engines side by
    // side (64 us per frame instead of 77 on one stream).  A copy kernel pulling the pinned buffer over PCIe is faster on its
    // own (48 GB/s against 25-30, tools/micro/h2d_paths.hip) but finds no wave slots while k_back fills every SIMD's
    // registers, neither with stream priority nor with CU masks (tools/micro/cu_mask_overlap.hip: a masked stream costs the
    // big kernel 14 %): measured at 73-75 us per frame inside the library, and dropped.
    for (UpRing* r : {&c->up_depth, &c->up_rgb}) HIP_TRY(c, hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : c->frame_done) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->copy_ready = true;
  }
  const int next = (ring.cur + 1) % 3;
  // a frame that mrh_integrate kept back (flush_deferred) has not marked its slots yet: before the ring comes round to one of them, it runs
  if (c->deferred.on && next == c->deferred.ring[&ring == &c->up_rgb ? 1 : 0].cur) {
    const int frc = flush_deferred(c);
    if (frc < 0) return frc;
  }
  UpSlot& u = ring.s[next];
  if (u.last_seq) HIP_TRY(c, hipEventSynchronize(c->frame_done[u.last_seq % 8]));  // this mark or a later one of the same stream
  if (u.copied_rec) HIP_TRY(c, hipEventSynchronize(u.copied));
  if (bytes > u.cap) {
    if (u.h) HIP_TRY(c, hipHostFree(u.h));
    if (u.d) HIP_TRY(c, hipFree(u.d));
    u.h = u.d = nullptr; u.cap = 0;
    HIP_TRY(c, hipHostMalloc(&u.h, bytes, hipHostMallocDefault));
    HIP_TRY(c, hipMalloc(&u.d, bytes));
    u.cap = bytes;
    if (!u.copied) HIP_TRY(c, hipEventCreateWithFlags(&u.copied, hipEventDisableTiming));
  }
  copy_to_staging(u.h, src, bytes);
  // (Round 5 measured the two runtime calls below on a thread of their own, so that the caller is back in its code ~10 us earlier:
  // uploads alone 56 -> 43 us per frame, but a FRAME stays at 62-64 us — mrh_integrate then waits for that thread to have
  // recorded the event before it can enqueue the stream wait, and the chain staging -> copy call -> stream wait -> launches is
  // on the caller's critical path whoever makes the calls.  Removed again; profiles/r05/README.md.)
  HIP_TRY(c, hipMemcpyAsync(u.d, u.h, bytes, hipMemcpyHostToDevice, ring.stream));
  HIP_TRY(c, hipEventRecord(u.copied, ring.stream));
  u.copied_rec = true;
  u.last_seq = 0;
  ring.last_copy = u.copied;  // a ring's copies are ordered on its stream: the newest event covers the earlier ones
  ring.waited[0] = ring.waited[1] = false;
  ring.cur = next;
  *out_dev = u.d;
  return MRH_OK;
}

// before kernels that read the images: `reader` — the stream those kernels are launched on: the front stream for a pipelined
// frame (its integration reads the cleaned copy the front half wrote), the main stream otherwise — waits for the newest uploads
int send_uploads(mrh_ctx* c, hipStream_t reader) {
  const int w = (reader == c->stream) ? 0 : 1;
  for (UpRing* r : {&c->up_depth, &c->up_rgb})
    if (r->last_copy && !r->waited[w]) {
      // a transfer the host already sees complete needs no wait packet (a kernel launched from here on reads what it wrote)
      const hipError_t q = hipEventQuery(r->last_copy);
      if (q == hipErrorNotReady) {
        (void) hipGetLastError();
        HIP_TRY(c, hipStreamWaitEvent(reader, r->last_copy, 0));
      } else if (q != hipSuccess) {
        return fail(c, MRH_ERR_DEVICE, "image transfer: %s", hipGetErrorString(q));
      }
      r->waited[w] = true;
    }
  return MRH_OK;
}

// ---- the non-blocking peeks (mrh_peek_free_blocks, mrh_peek_error_flags): h_peek, eight reports, one per frame mark ----
// the first peek of a context: reports start with the next frame
int enable_peeks(mrh_ctx* c) {
  if (c->peek_enabled) return MRH_OK;
  HIP_TRY(c, hipHostMalloc((void**) &c->h_peek, 64 * sizeof(int), hipHostMallocDefault));
  memset(c->h_peek, 0, 64 * sizeof(int));
  c->peek_enabled = true;
  return MRH_OK;
}
// the newest of the last eight marks whose report has landed: 1 and {*seq, *back: marks behind the newest, 1 = none}, 0 if none has, or an error
int newest_report(mrh_ctx* c, const char* who, uint64_t* seq_out, uint64_t* back_out) {
  for (uint64_t back = 1; back <= 8 && back < c->frame_seq; back++) {
    const uint64_t seq = c->frame_seq - back;
    if (c->peek_seq[seq % 8] != seq) continue;
    const hipError_t q = hipEventQuery(c->peek_done[seq % 8]);
    if (q == hipErrorNotReady) continue;
    if (q != hipSuccess) return fail(c, MRH_ERR_DEVICE, "%s: %s", who, hipGetErrorString(q));
    if (c->peek_seq[seq % 8] != seq) continue;
    *seq_out = seq; *back_out = back;
    return 1;
  }
  return 0;
}
// the pool report of mark `seq` (ctr[0 .. 4]: free-list levels ... error flags) into its slot of h_peek, behind whatever is on
// `s`; from here on the mark exists for the peeks (newest_report).  A mark that is posted again refreshes its report.
int post_report(mrh_ctx* c, const uint64_t seq, hipStream_t s) {
  k_report<<<1, 64, 0, s>>>(&c->tab.ctr[CTR_HEAP_FINE], c->h_peek + 8 * (seq % 8));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->peek_done[seq % 8], s));
  c->peek_seq[seq % 8] = seq;
  return MRH_OK;
}

// after the kernels of a frame (or of a seeding call) are enqueued: mark the ring slots they read, report the pool level
int mark_frame(mrh_ctx* c) {
  UpSlot* used[2] = {nullptr, nullptr};
  if (c->up_depth.cur >= 0 && c->d_depth == c->up_depth.s[c->up_depth.cur].d) used[0] = &c->up_depth.s[c->up_depth.cur];
  if (c->up_rgb.cur >= 0 && c->d_rgb == c->up_rgb.s[c->up_rgb.cur].d) used[1] = &c->up_rgb.s[c->up_rgb.cur];
  if (!used[0] && !used[1] && !c->peek_enabled) return MRH_OK;
  const uint64_t seq = c->frame_seq++;
  if (!c->frame_done[0])
    for (hipEvent_t& e : c->frame_done) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const bool lazy = c->last_frame_lazy && c->npend;  // the frame's integration is not enqueued yet (launch_pending)
  if (c->peek_enabled) {
    if (!c->peek_done[0])
      for (hipEvent_t& e : c->peek_done) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (lazy) {
      // The report of a pipelined frame is written behind its integration, by launch_pending; until then the mark does not
      // exist for the peeks (they fall back to an older one and say how many frames behind it is).  A report launched here would
      // sit behind the integration of an EARLIER frame only, and an event on the front stream says nothing about it at all.
      c->peek_seq[seq % 8] = 0;
      c->pendq[c->npend - 1].report_seq = seq;
    } else if (const int rc = post_report(c, seq, c->stream)) {
      return rc;
    }
  }
  if (used[0] || used[1]) {
    // the raw images of a pipelined frame are read by its front half, on the front stream (its integration reads the cleaned copy)
    HIP_TRY(c, hipEventRecord(c->frame_done[seq % 8], lazy ? c->stream_front : c->stream));
    for (UpSlot* u : used) if (u) u->last_seq = seq;
  }
  return MRH_OK;
}

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
  if (!c->h_qt_out) HIP_TRY(c, hipHostMalloc((void**) &c->h_qt_out, 2 * sizeof(u64), hipHostMallocDefault));
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
}  // namespace
}  // extern "C++"

extern "C++" {
namespace {

int take_event_pair(mrh_ctx* c, EvPair& e) {
  if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); return MRH_OK; }
  if (c->ev_pending.size() >= 4096) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int r = drain_events(c);
    if (r) return r;
    e = c->ev_pool.back(); c->ev_pool.pop_back();
    return MRH_OK;
  }
  HIP_TRY(c, hipEventCreate(&e.a)); HIP_TRY(c, hipEventCreate(&e.b));
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
  // (a high-priority front stream, a ring of eight and integrations deferred by two calls were measured: no difference)
  HIP_TRY(c, hipStreamCreateWithFlags(&c->stream_front, hipStreamNonBlocking));
  // (hipEventDisableSystemFence on these events — they order two streams of one device — was measured in round 5: no difference)
  for (hipEvent_t& e : c->ev_front) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (int i = 1; i < kPipeRing; i++) {
    HIP_TRY(c, hipMalloc((void**) &c->ring_vis[i], cap * sizeof(int4)));
    HIP_TRY(c, hipMalloc((void**) &c->ring_bbox[i], cap * sizeof(int4)));
    HIP_TRY(c, hipMalloc((void**) &c->ring_cfree[i], cap * sizeof(int4)));
    HIP_TRY(c, hipMalloc((void**) &c->ring_zmin[i], cap * sizeof(float)));
  }
  HIP_TRY(c, hipMalloc((void**) &c->fast.zlist, cap * sizeof(int4)));
  HIP_TRY(c, hipMalloc((void**) &c->want_ring, (size_t) kPipeRing * c->slots * sizeof(u32)));
  HIP_TRY(c, hipMemsetAsync(c->want_ring, 0, (size_t) kPipeRing * c->slots * sizeof(u32), c->stream));  // stamps start at 1
  if (!c->h_levels) HIP_TRY(c, hipHostMalloc((void**) &c->h_levels, 4 * sizeof(int), hipHostMallocDefault));
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
  for (uint2*& d : c->pipe_dcx) { if (d) HIP_TRY(c, hipFree(d)); d = nullptr; }
  c->pipe_npix = 0;
  const int n = c->stream_front ? kPipeRing : 1;
  for (int i = 0; i < n; i++) HIP_TRY(c, hipMalloc((void**) &c->pipe_dcx[i], npix * sizeof(uint2)));
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

}  // extern "C"

#include "mrh_points.h"

extern "C" {

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

}  // extern "C"

#include "mrh_blocks.h"

extern "C" {

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
extern "C++" {
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
}  // extern "C++"

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
extern "C++" {
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
    HIP_TRY(c, hipMalloc((void**) &N.d_ctr, 2 * NC_N * sizeof(u64)));
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
}  // extern "C++"

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
    HIP_TRY(c, hipHostMalloc((void**) &N.h_ctr, NC_N * sizeof(u64), hipHostMallocDefault));
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

#include "mrh_comm.h"
