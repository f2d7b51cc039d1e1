// mrh_context.h — the context (mrh_ctx) and its lifetime: what it holds, how it reports errors, what it owns (the ledger behind
// dev_alloc / pinned_alloc / event_new), mrh_create's stages and free_all.  Included by mrh_capi.hip after the kernel headers and
// before every host-path header (mrh_upload.h, mrh_extract.h, mrh_points.h, mrh_blocks.h, mrh_seeds.h, mrh_readers.h, mrh_comm.h).  DESIGN.md 4.8.
#pragma once

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

// What a depth frame was issued under: the camera with its pose, the two images, and where each upload ring stood.  One function
// reads it out of the context and one puts it back (mrh_frame.h: read_inputs, apply_inputs).
struct FrameInputs {
  Cam cam;
  const float* d_depth; const uint8_t* d_rgb;
  int depth_rows, depth_cols, rgb_rows, rgb_cols;
  struct Ring { int cur; hipEvent_t last_copy; bool waited[2]; } ring[2];  // up_depth, up_rgb
};
// A frame of host images is LAUNCHED one mrh_integrate late (round 5): by then its two transfers have completed and the frame's
// kernels need no cross-stream wait — a wait that is enqueued while its event is still pending costs the waiting stream ~6 us
// of idle time, and a host-fed frame had two of them in front of its 41 us of kernels.  mrh_integrate checks what it can,
// keeps the inputs and returns; the next mrh_integrate — or whichever other entry point needs the map (ensure_ready) — runs the
// frame first, with those inputs swapped in (mrh_frame.h: flush_deferred).  MRH_DEFER_UPLOADS=0 launches at once.
struct DeferredFrame {
  bool on = false;
  int n_inval = 0;
  FrameInputs in;
};

// Every decision about one frame, each computed once (mrh_frame.h: plan_begin, plan_frame, the pipelined-or-serial choice in
// integrate_single_res_frame, take_slots) and read by whatever launches for the frame; the context keeps the last one.
enum FrameKind {
  FRAME_SERIAL,     // the two launches of a single-resolution map on the main stream
  FRAME_PIPELINED,  // ... its front half on the front stream, its integration held back (PendingBack)
  FRAME_FUSED_MR,   // the two launches of a multi-resolution map
  FRAME_GENERAL,    // the general kernels (mrh_kernels.h): multi-resolution frames that cannot be fused, LiDAR scans; GC by k_gc_identify / k_gc_free
};
struct FramePlan {
  FrameKind kind = FRAME_SERIAL;
  int max_num_frames = 0;       // n_frames_invalidate_voxels of this frame; > 0: garbage collection on
  bool starve_now = false;      // the frame ends with the starve step
  bool starve_fused = false;    // a starve step of this frame takes k_starve_z / k_starve_tail (else k_starve<0,1,2>) ...
  bool starve_in_pipe = false;  // ... and this frame's does, without leaving the pipeline
  bool gc_inline = false;       // k_back collects (FREE); else frame_tail or the starve tail does
  bool safe_div = false, sph = false;
  float gc_thr = 0.f;           // the GC threshold
  int set = 0, zero_set = 0;    // the frame's list-counter set, and the one its integration clears
  int ring = 0, seq = 0;        // ring slot (0: a serial frame) and sequence number among the single-resolution frames
  u32 stamp = 0;
  int tiles_x = 0, n_tiles = 0; // ray tiles of k_front
};
// the integration of the newest pipelined frame is enqueued by the NEXT mrh_integrate (or by whichever other entry point comes
// first): by then its front half has usually finished, the host sees that (hipEventQuery) and the main stream needs no
// cross-stream wait in front of the launch — such a wait costs ~6 us of idle main stream per frame on this runtime.
// The plan, and what only a held-back integration needs: what its front half was launched with, a profile launch's event pair
// (null: none), the frame mark whose pool report was left to this launch (0: none), k_count_updates' zombie flag.
struct PendingBack {
  FramePlan plan;
  Cam cam; Fast f; Lists L;
  EvPair ev;
  uint64_t report_seq;
  bool count_zombies;
};

// ---- pipelined frames (mrh_frame.h; MRH_PIPE=0: every frame serial, the two launches on the main stream) ----
// The front half of a frame (k_front<..., LAZY>) is launched on `stream_front`, its integration (k_back<..., LZ = 2>) on the
// main stream behind one event; the front stream never waits for the main one, so the front half of frame g + 1 runs next to
// the integration of frame g.  Up to kPipeRing - 1 frames are in flight, each with its own {depth, colour} image, lists,
// list-counter set and want stamps.  Two invariants order the streams, each enforced in one place (mrh_frame.h):
//   (a) after the main stream has changed keys or the free list (a reclaim, a serial frame, a table rebuild, any other entry point),
//       the next front half is launched only after the host has seen the main stream drain: main_stream_changed_map raises
//       front_needs_sync, resync_front — in front of k_front<LAZY> — synchronises and lowers it;
//   (b) anything that is not a pipelined frame meets the map only behind strict_point: the pending integrations launched, the zombies
//       reclaimed.  In particular the table is rebuilt only with no frame in flight (frame_upkeep).
struct PipeState {
  // created by ensure_pipe_state (a context with `pipe` set, at its first single-resolution frame) and kept for the context's life:
  // the front stream, its events, ring slots 1 .. kPipeRing - 1, the want stamps, h_levels (and Fast::zlist)
  hipStream_t stream_front = nullptr;
  hipEvent_t ev_front[kPipeRing] = {};
  int4* ring_vis[kPipeRing] = {}; int4* ring_bbox[kPipeRing] = {}; int4* ring_cfree[kPipeRing] = {}; float* ring_zmin[kPipeRing] = {};  // [0]: unused (ring_lists)
  u32* want_ring = nullptr;        // kPipeRing x slots stamps
  int* h_levels = nullptr;         // pinned {fine free-list level, zombies, sequence number of the last integration that started}
  uint2* dcx[kPipeRing] = {};      // {cleaned depth, packed colour} of a frame (written by k_front), per ring slot; without the pipelining
  size_t npix = 0;                 // state [0] alone, which every serial frame uses (ensure_frame_dcx)
  // what describes the MAP's frames: cleared by reset_pipe_counters (mrh_reset: an empty map has no frame in flight, no zombies, and
  // its list-counter sets and sequence numbers start over)
  uint64_t fast_frames = 0;        // two-launch frames issued: selects the list-counter set
  uint64_t seq = 0;                // single-resolution frames issued (pipelined or not)
  uint64_t base = 0;               // every frame below this sequence number is known complete (host synchronised)
  int lazy_run = 0;                // pipelined frames since the last reclaim
  bool zombies_possible = false;
  bool front_needs_sync = false;   // invariant (a)
  static constexpr int kPendMax = 3;
  PendingBack pendq[kPendMax];     // oldest first
  int npend = 0;
  // what describes the CALLER's pattern and the scratch: survives a reset.  A caller that synchronised after each of the last frames
  // still does (flushed_since_frame is raised by the reset's own ensure_ready anyway), last_frame_lazy is written by every frame
  // before mark_frame reads it, and the z-buffer pairs are scratch that is as clean or dirty as before.
  bool last_frame_lazy = false;
  bool flushed_since_frame = false;  // an entry point other than the per-frame ones ran since the last frame
  int sync_streak = 0;               // frames in a row that found the pipeline flushed
  // starve frames on the two-launch path (mrh_fast2.h: k_starve_z / k_starve_tail): two PAIRS of z-buffers, the tail launch of
  // one starve frame puts the other pair back to "empty" for the next
  u64* d_zfused = nullptr;  // 2 pairs x 2 x npix
  size_t zfused_n = 0;
  bool zfused_clean[2] = {false, false};
  size_t zfused_clean_npix = 0;  // the image size the clean pairs were cleared for (a pair holds zbuf0 | zbuf1 at THAT size)
  int zfused_next = 0;
};

}  // namespace

struct mrh_ctx {
  mrh_params p;
  int device = 0;
  hipStream_t stream = nullptr;
  // everything dev_alloc / pinned_alloc / event_new handed out and nobody has freed yet: what free_all releases
  struct Owned { std::vector<void*> dev, pinned; std::vector<hipEvent_t> events; } owned;
  Cam cam;
  Map map;
  Tab tab;
  bool has_camera = false;
  bool spherical = false;
  // images.  Host uploads (mrh_upload_depth / _rgb) go through a ring of three slots per image kind — pinned staging +
  // device buffer — on a second stream, so the copy of frame N+1 overlaps the kernels of frame N; the frame's kernels
  // wait for the newest copy event, a slot is rewritten only after the last frame that read it (frame_done event).
  UpRing up_depth, up_rgb;
  DeferredFrame deferred;
  int defer_uploads = 1;            // MRH_DEFER_UPLOADS=0: a host-fed frame is launched by the mrh_integrate that issues it
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
  // the pipeline's switches; its state is `ps`
  int pipe = 1;
  int pipe_grid = 1024;                     // workgroups of a pipelined integration: ONE resident generation (4 per CU x 256 CUs).  With 2048 the
                                            // second generation competes with the front half's workgroups for the slots the first one frees: 37.3 against
                                            // 34.8 us per frame (MRH_PIPE_GRID; the serial launch keeps 2048)
  int pipe_uploads = 0;                     // MRH_PIPE_UPLOADS=1: pipeline frames whose images came through mrh_upload_* too
  int pipe_period = 64;                     // the reclaim (and one serial frame) every so many pipelined frames; MRH_PIPE_PERIOD.  (32 until
                                            // round 6: a period boundary costs the pipeline ~60 us, the zombies it bounds are also bounded by the
                                            // pool test below (zombies <= pool / 8); 64 — the census period — gave +4 % at 100 steps, 128 no more)
  bool pipe_always_wait = false;            // MRH_PIPE_ALWAYS_WAIT=1: a pipelined integration always carries its wait packet (A/B)
  int pipe_defer = 1;                     // integrations kept back (MRH_PIPE_DEFER, 1 .. PipeState::kPendMax - 1): the older a front half, the surer it has finished
  PipeState ps;
  FramePlan plan;  // the last frame's (a sharded starve frame's until mrh_integrate_resume has run its tail)
  uint64_t dbg_waits = 0;
  double dbg_spin_us = 0, dbg_api_us = 0; uint64_t dbg_lazy_frames = 0;  // MRH_DEBUG: where the host's time in a pipelined frame goes
  int4* d_cfree = nullptr;
  float* d_cloud = nullptr; size_t cloud_n = 0;  // spherical camera: getDepth(cloud) image of the current frame (k_cloud_depth)
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
  // 3DGS splat seeds (mrh_seeds.h, kernels in mrh_splat.h): sized for one (image shape, min pixel size)
  struct Seeds {
    size_t cap = 0;  // potential nodes the device buffers below hold (regrow_all); it replaces the QTree once recorded here
    QSum* d_sums = nullptr; u32* d_flags = nullptr; u32* d_unc = nullptr; u64* d_marks = nullptr; u64* d_pos = nullptr;
    mrh_splat_seed* d_parked = nullptr; mrh_qtree_leaf* d_leaves = nullptr;
    // what the caller takes from a seeding call is written by its last launch straight into pinned host memory (a few hundred to a few
    // thousand 20-byte seeds and two counters): one synchronisation, no transfer calls (they were two pageable read-backs, each behind
    // a synchronisation of its own: ~35 of the call's 135 us)
    mrh_splat_seed* h_seeds = nullptr; size_t seed_cap = 0;
    u64* h_out = nullptr;   // [0] totals (leaves | seeds << 32), [1] literal evaluations
    u64* d_misc = nullptr;  // [0] totals (leaves | seeds << 32), [1] uncertain-node counter (low word)
    int literal = 0;        // MRH_QTREE_LITERAL=1: every node error through the reference's summation order (cross-check)
    uint32_t last_literal = 0;
    std::vector<mrh_qtree_leaf> leaves;
    uint64_t n_leaves = 0;            // leaves of the last mrh_splat_seeds, still on the device (d_leaves) until someone asks
    bool leaves_on_host = true;
  } qt;
  int mr_fused = 1;          // MRH_MR_FUSED=0: multi-resolution maps always through the general kernels (mrh_kernels.h)
  bool mr_next_general = true;    // the next multi-resolution frame must take the general path (frame 0 / after a starve frame / after an import)
  bool mr_summaries_valid = false;  // fast.summary / summary_c describe every live block (the general kernels do not maintain them)
  bool refill_flag_valid = false;  // d_flag holds the refill test for the next fused frame (taken by k_mr_tail)
  int mesh_on_host = 0;      // MRH_MESH_HOST=1: mesh post-process with the host restatement instead of mrh_mesh.h
  float* d_zmin = nullptr;   // per visible-list entry (Lists::zmin)
  u64* d_cnt_partials = nullptr;
  int fused_grid = 2048;  // x 4 waves
  int sweep_wgs_mr = 1024; // the same for multi-resolution maps (9x the descriptors); MRH_SWEEP_WGS_MR
  int sweep_wgs = 128;    // descriptor-sweep workgroups appended to the allocation launch (k_front)
  int integrate_grid = 1024;
  int low_blocks_to_allocate = 0;
  uint64_t num_blocks = 0, slots = 0, max_triangles = 0;
  uint64_t frames = 0;
  int heap_descending = 0;   // MRH_DEBUG_HEAP_DESCENDING: the fine free list starts in descending order (tests)
  int pending = 0;           // sharded starve frames: 1 after pass 0, 2 after pass 1
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
  // raycasting (mrh_readers.h, kernels in mrh_raycast.h): the images of mrh_raycast and mrh_raycast_spherical, grow-only — device
  // [depth f32 | normals 3 x f32 | points 3 x f32 | rgb 3 x u8] per pixel and the pinned host copy the caller reads
  struct Ray {
    char* d_img = nullptr; size_t cap = 0;  // pixels
    char* h_img = nullptr; size_t h_cap = 0;
  } ray;
  // distance fields (mrh_readers.h, kernels in mrh_esdf.h), grow-only, in cells — scratch of every call: the state byte, the x pass's |dx| (u16: at most 511)
  // and the y pass's u32 plane; results of mrh_esdf: dist and d2 on the device and the pinned [dist f32 | d2 u32 | state u8] the caller reads
  struct Esdf {
    uint8_t* d_state = nullptr; uint16_t* d_row = nullptr; u32* d_plane = nullptr; size_t cap = 0;
    float* d_dist = nullptr; u32* d_d2 = nullptr; size_t out_cap = 0;
    char* h_out = nullptr; size_t h_cap = 0;
  } esdf;
  // point queries (mrh_readers.h, kernels in mrh_query.h), grow-only, in points — the results of mrh_query_points on the device and
  // in the pinned copy the caller reads, both [dist f32 | grad 3 x f32 | rgbw 4 x u8 | state u8], each plane contiguous
  struct Query {
    char* d_out = nullptr; size_t cap = 0;
    char* h_out = nullptr; size_t h_cap = 0;
  } query;
  // ray queries (mrh_readers.h, kernel in mrh_rays.h), grow-only, in rays — the results of mrh_cast_rays on the device and in the
  // pinned copy the caller reads, both [range f32 | normals 3 x f32 | counts 2 x u32 | first_unknown f32 | rgb 3 x u8 | status u8],
  // each plane contiguous.  The rays themselves come through `stage`
  struct Rays {
    char* d_out = nullptr; size_t cap = 0;
    char* h_out = nullptr; size_t h_cap = 0;
  } rays;
  // the free-space layer (mrh_readers.h, kernels in mrh_freespace.h): `on` and the box once mrh_freespace_create has run, the
  // words (capacity in words, grow-only; `L.n_words` of them are the layer).  Scratch and results of mrh_freespace_box, grow-only,
  // in cells: the classified bytes, the finished bytes, their pinned copy.  Results of mrh_freespace_segments, grow-only, in
  // segments: [counts 2 x u32 | status u8] on the device and pinned.  The carves' and the segments' host input comes through `stage`
  struct Free {
    bool on = false;
    mrh::FreeLayer L = {};
    u32* d_words = nullptr; size_t cap = 0;
    uint8_t* d_cls = nullptr; size_t cls_cap = 0;
    uint8_t* d_state = nullptr; size_t state_cap = 0;
    uint8_t* h_state = nullptr; size_t h_cap = 0;
    char* d_seg = nullptr; size_t seg_cap = 0;
    char* h_seg = nullptr; size_t h_seg_cap = 0;
  } free;
  // map-to-map fusion (mrh_readers.h, kernels in mrh_remap.h), grow-only — per candidate slot the two (key, value) pairs of the
  // sort, the marks and positions of the scans, with them the sort's histogram and the scans' tile sums; one counter (valid
  // voxels); the records of the last call (bytes)
  struct Remap {
    u64* d_keys[2] = {nullptr, nullptr}; u32* d_vals[2] = {nullptr, nullptr};
    u64* d_marks = nullptr; u64* d_pos = nullptr; u64* d_sums = nullptr; u32* d_sort = nullptr; size_t cap = 0;  // slots
    u64* d_count = nullptr;
    char* d_rec = nullptr; size_t rec_cap = 0;
  } remap;
  // map-to-map registration (mrh_readers.h, kernels in mrh_align.h), grow-only — as the source of a call: per live block the
  // count of its samples, their position (the scan), the tile sums of the scan and the block's integer box (lo, hi); the sample
  // list, 16 bytes each; pinned {lo, hi} of the whole list.  As the destination it uses `fit` alone
  struct Align {
    u64* d_counts = nullptr; u64* d_pos = nullptr; u64* d_sums = nullptr; int4* d_boxes = nullptr; size_t cap = 0;  // blocks
    float4* d_samples = nullptr; size_t smp_cap = 0;   // samples
    int4* h_box = nullptr;                             // {lo, hi} of the accepted voxel coordinates
  } align;
  // tracking (mrh_readers.h, kernels in mrh_track.h), grow-only — device [model depth or range f32 | model normals 3 x f32] per
  // pixel and, for scans (D15), the model's points image
  struct Track { char* d_img = nullptr; size_t cap = 0; float* d_mp = nullptr; size_t mp_cap = 0; } trk;  // both in pixels
  // what every pose fit reduces through (mrh_readers.h: linearise_sums) — tracking, and registration with this context as the
  // destination: the partial slab, one row of 32 words per workgroup of a linearisation (grow-only, in rows), and the pinned 32
  // sums k_track_finish leaves for the host.  One per context is enough: its users run on this context's stream and block
  struct Fit { long long* d_slab = nullptr; size_t slab_cap = 0; long long* h_sums = nullptr; } fit;
  // host input staged onto the device (mrh_readers.h: stage_obs), one pair of buffers, pinned and device, grow-only, in floats.
  // Its users: the depth image of mrh_track_depth, the cloud of mrh_track_scan, the points of mrh_query_points, the rays of
  // mrh_cast_rays, and the images, clouds and segments of the free-space calls.  Each
  // overwrites what the last one left, which is safe because every user blocks before it returns: nothing reads the pair then
  struct Stage { float* h = nullptr; size_t h_cap = 0; float* d = nullptr; size_t d_cap = 0; } stage;
  int* d_keep = nullptr;  // the frame path's CTR_COMPACT while a reader borrows the compact list (mrh_blocks.h: borrow_live_blocks)
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

// the calls that close a cycle between this header, mrh_upload.h, mrh_frame.h, mrh_comm.h (the next three: integrate_checks, in
// mrh_frame.h, sits above mrh_comm.h) and mrh_capi.hip, declared once
static int comm_allreduce_zbuf(mrh_ctx* c, mrh::u64* buf, size_t n);
static void comm_release(mrh_ctx* c);
static bool comm_matches_sharding(const mrh_ctx* c, int* comm_rank, int* comm_world);
namespace {
int strict_point(mrh_ctx* c);  // mrh_frame.h
int flush_deferred(mrh_ctx* c);
// PipeState's invariant (a): the main stream has changed keys or the free list, or is about to (every caller sits in front of the
// launches it speaks for), while the front stream is not looking.  Without a front stream the flag is raised for nobody.
void main_stream_changed_map(mrh_ctx* c) { c->ps.front_needs_sync = true; }

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

// ---- what the context owns: dev_alloc, dev_free, pinned_alloc, pinned_free, event_new alone create or release device memory, pinned
// memory or events for a context, and return the runtime's own error.  A free forgets the pointer and nulls it (on regrow only: linear search).
template <typename T> hipError_t own(std::vector<void*>& ledger, T*& p, const hipError_t e) {
  if (e != hipSuccess) p = nullptr; else ledger.push_back((void*) p);
  return e;
}
template <typename T> hipError_t disown(std::vector<void*>& ledger, T*& p, hipError_t (*release)(void*)) {
  const auto it = std::find(ledger.begin(), ledger.end(), (void*) p);
  const hipError_t e = !p ? hipSuccess : it == ledger.end() ? hipErrorInvalidValue : release((void*) p);
  if (it != ledger.end()) { *it = ledger.back(); ledger.pop_back(); }
  p = nullptr;
  return e;
}
template <typename T> hipError_t dev_alloc(mrh_ctx* c, T*& p, const size_t bytes) { return own(c->owned.dev, p, hipMalloc((void**) &p, bytes)); }
template <typename T> hipError_t dev_free(mrh_ctx* c, T*& p) { return disown(c->owned.dev, p, hipFree); }
template <typename T> hipError_t pinned_alloc(mrh_ctx* c, T*& p, const size_t bytes) { return own(c->owned.pinned, p, hipHostMalloc((void**) &p, bytes, hipHostMallocDefault)); }
template <typename T> hipError_t pinned_free(mrh_ctx* c, T*& p) { return disown(c->owned.pinned, p, hipHostFree); }
hipError_t event_new(mrh_ctx* c, hipEvent_t& ev, const bool timing) {  // timing = false: it only orders streams (hipEventDisableTiming)
  const hipError_t e = timing ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) ev = nullptr; else c->owned.events.push_back(ev);
  return e;
}

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
  for (const GrowMember& m : members) HIP_TRY(c, dev_free(c, *m.p));
  for (const GrowMember& m : members) {
    const hipError_t e = dev_alloc(c, *m.p, m.bytes);
    if (e == hipSuccess) continue;
    for (const GrowMember& f : members) (void) dev_free(c, *f.p);
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
  T* grown = nullptr;
  HIP_TRY(c, dev_alloc(c, grown, bytes_new));
  struct Drop { mrh_ctx* c; T*& p; ~Drop() { (void) dev_free(c, p); } } drop{c, grown};  // on every way out: the new buffer if a step fails, else the old one
  if (p && keep_bytes) HIP_TRY(c, hipMemcpyAsync(grown, p, keep_bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::swap(p, grown); cap = cap_new;
  return MRH_OK;
}
// ... and a pinned host buffer the caller reads results from (the call that filled it blocked: no synchronisation), contents not kept
template <typename T>
int regrow_pinned(mrh_ctx* c, T*& p, size_t& cap, const size_t cap_new, const size_t bytes) {
  if (cap_new <= cap) return MRH_OK;
  cap = 0;
  (void) pinned_free(c, p);
  HIP_TRY(c, pinned_alloc(c, p, bytes));
  cap = cap_new;
  return MRH_OK;
}

uint64_t next_pow2(uint64_t v) {
  uint64_t r = 1;
  while (r < v) r <<= 1;
  return r;
}

// A fixed sequence, whatever the context allocated: the streams drain, the communicator lets go, the ledger is released, the
// streams go last.  Also the one failure path of mrh_create: a context that got half way is released like any other.
void free_all(mrh_ctx* c) {
  if (!c) return;
  (void) hipSetDevice(c->device);
  hipStream_t* streams[4] = {&c->up_depth.stream, &c->up_rgb.stream, &c->ps.stream_front, &c->stream};
  for (hipStream_t* s : streams) if (*s) (void) hipStreamSynchronize(*s);
  comm_release(c);
  for (hipEvent_t e : c->owned.events) (void) hipEventDestroy(e);
  for (void* p : c->owned.pinned) (void) hipHostFree(p);
  for (void* p : c->owned.dev) (void) hipFree(p);
  c->owned = {};
  for (hipStream_t* s : streams) if (*s) { (void) hipStreamDestroy(*s); *s = nullptr; }
}

// what of PipeState describes the map's frames (see there): a reset map has nothing left to integrate
void reset_pipe_counters(mrh_ctx* c) {
  PipeState& ps = c->ps;
  for (int i = 0; i < ps.npend; i++) if (ps.pendq[i].ev.a) c->ev_pool.push_back(ps.pendq[i].ev);
  ps.npend = 0;
  ps.fast_frames = 0;
  ps.seq = ps.base = 0;
  ps.lazy_run = 0;
  ps.zombies_possible = false;
  ps.front_needs_sync = false;
}

// (re)initialises every device structure to the empty map (voxel_data_structures.cpp:58-87 + ctor counters)
int init_buffers(mrh_ctx* c) {
  hipStream_t s = c->stream;
  c->mr_next_general = true;
  c->refill_flag_valid = false;
  c->mr_summaries_valid = false;
  if (c->ps.stream_front) HIP_TRY(c, hipStreamSynchronize(c->ps.stream_front));
  reset_pipe_counters(c);
  if (c->ps.h_levels) { c->ps.h_levels[0] = (int) c->num_blocks - 1; c->ps.h_levels[1] = 0; c->ps.h_levels[2] = -1; }
  if (c->ps.want_ring) HIP_TRY(c, hipMemsetAsync(c->ps.want_ring, 0, (size_t) kPipeRing * c->slots * sizeof(u32), s));
  const Tab& t = c->tab;
  k_init_table<<<1024, 256, 0, s>>>(t.keys, c->slots);
  k_init_heap<<<1024, 256, 0, s>>>(t.heap_fine, (u32) c->num_blocks, c->heap_descending);
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

// ---- mrh_create in stages (each returns an error code through HIP_TRY; mrh_create releases a context that got half way) ----
// what mrh_create rejects before a context exists
int create_checks(const mrh_params* p) {
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
  return MRH_OK;
}

// parameter defaults, the main stream, the capacities (geowrapper.cpp:37-54 when not given explicitly), the Tab / Map fields
int size_map(mrh_ctx* c, const mrh_params* p) {
  c->p = *p;
  if (c->p.integration_weight_max == 0) c->p.integration_weight_max = 255;
  if (c->p.voxel_extents_scale == 0) c->p.voxel_extents_scale = 1;
  if (c->p.shard_count < 1) c->p.shard_count = 1;
  c->device = p->device_id;
  memset(&c->tab, 0, sizeof c->tab); memset(&c->cam, 0, sizeof c->cam); memset(&c->fast, 0, sizeof c->fast);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  size_t free_b = 0, total_b = 0;
  HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
  const double to_alloc = (double) free_b * 0.70;  // SDFBlocks_ratio
  c->num_blocks = p->num_sdf_blocks ? p->num_sdf_blocks : (uint64_t) ((to_alloc * 0.70) / (12.0 * 512.0));
  if (c->num_blocks >= (1ull << 28)) c->num_blocks = (1ull << 28) - 1;  // 31-bit coarse unit ids
  c->max_triangles = p->max_triangles ? p->max_triangles : (uint64_t) ((to_alloc * 0.25) / 72.0);
  c->slots = std::max<uint64_t>(1024, next_pow2(p->hash_slots ? p->hash_slots : 4 * c->num_blocks));
  c->low_blocks_to_allocate = (int) ((float) c->num_blocks * 0.1f);  // voxel_data_structures.cuh:57-61
  c->fast.zlist_cap = (u32) c->num_blocks;
  Tab& t = c->tab;
  t.slot_mask = (u32) (c->slots - 1); t.max_probe = 512; t.cap_blocks = (u32) c->num_blocks;
  t.multi_res = p->sdf_var_threshold > 0.f ? 1u : 0u;
  Map& m = c->map;
  m.vs = p->virtual_voxel_size; m.trunc = p->sdf_truncation; m.trunc_scale = p->sdf_truncation_scale;
  m.var_threshold = p->sdf_var_threshold; m.mc_threshold = p->marching_cubes_threshold; m.min_weight_threshold = p->min_weight_threshold;
  m.weight_sample = p->integration_weight_sample & 0xFF; m.weight_max = c->p.integration_weight_max & 0xFF;
  m.shard_rank = c->p.shard_rank; m.shard_count = c->p.shard_count;
  m.shard_chunk_log2 = (p->shard_chunk_log2 > 0 && p->shard_chunk_log2 < 16) ? p->shard_chunk_log2 : 3;
  return MRH_OK;
}

// the buffers every context has from the start (everything else is allocated by the path that first needs it)
int alloc_map(mrh_ctx* c) {
  Tab& t = c->tab;
  const size_t nb = c->num_blocks, list_cap = nb * (t.multi_res ? 9 : 1);  // visible / free lists may hold coarse units, too
  HIP_TRY(c, dev_alloc(c, t.keys, c->slots * sizeof(u64)));                HIP_TRY(c, dev_alloc(c, t.vals, c->slots * sizeof(u32)));
  HIP_TRY(c, dev_alloc(c, t.heap_fine, (nb + 1) * sizeof(u32)));           HIP_TRY(c, dev_alloc(c, t.desc_fine, nb * sizeof(int4)));
  if (t.multi_res) {
    HIP_TRY(c, dev_alloc(c, t.heap_coarse, (nb * 8 + 9) * sizeof(u32)));   HIP_TRY(c, dev_alloc(c, t.desc_coarse, nb * 8 * sizeof(int4)));
    HIP_TRY(c, dev_alloc(c, c->d_realloc, nb * sizeof(int4)));             HIP_TRY(c, dev_alloc(c, c->d_reint, nb * sizeof(int4)));
    HIP_TRY(c, dev_alloc(c, c->fast.summary_c, nb * 8 * sizeof(uint2)));
  }
  HIP_TRY(c, dev_alloc(c, t.pool, nb * (size_t) kFineBytes));
  HIP_TRY(c, dev_alloc(c, t.compact, list_cap * sizeof(int4)));            HIP_TRY(c, dev_alloc(c, c->d_decision, list_cap * sizeof(u32)));
  HIP_TRY(c, dev_alloc(c, t.ctr, CTR_COUNT * sizeof(int)));                HIP_TRY(c, dev_alloc(c, t.prof, PROF_COUNT * sizeof(u64)));
  HIP_TRY(c, dev_alloc(c, c->d_flag, sizeof(int)));                        HIP_TRY(c, dev_alloc(c, c->d_misc, 4 * sizeof(u32)));
  HIP_TRY(c, dev_alloc(c, c->d_upd_partials, (size_t) c->integrate_grid * sizeof(u64)));
  HIP_TRY(c, dev_alloc(c, c->d_cnt_partials, (size_t) 32768 * 4 * sizeof(u64)));  // max MRH_FUSED_GRID
  HIP_TRY(c, dev_alloc(c, c->fast.summary, nb * sizeof(uint2)));           HIP_TRY(c, dev_alloc(c, c->fast.bbox, list_cap * sizeof(int4)));
#ifdef MRH_TRACE
  HIP_TRY(c, dev_alloc(c, c->fast.trace, nb * 8 * sizeof(u64)));
  HIP_TRY(c, hipMemset(c->fast.trace, 0, nb * 8 * sizeof(u64)));
#endif
  HIP_TRY(c, dev_alloc(c, c->d_cfree, list_cap * sizeof(int4)));           HIP_TRY(c, dev_alloc(c, c->d_zmin, list_cap * sizeof(float)));
  return MRH_OK;
}

// Two self-checks of the arithmetic on this device.  A check that cannot run counts as failed: the kernels then take the
// instantiation that does not rely on it.
int probe_arithmetic(mrh_ctx* c) {
  Map& m = c->map;
  const bool dbg = getenv("MRH_DEBUG") != nullptr;
  // where is voxel -> block an arithmetic shift?  (mrh_device.h: world_to_block_fast)
  const u32 init = 1u << 23;
  u32 first_bad = 0;
  if (hipMemcpy(c->d_misc, &init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) first_bad = 1;
  k_block_shift_limit<<<(1 << 23) / 256, 256, 0, c->stream>>>(m.vs, c->d_misc);
  if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&first_bad, c->d_misc, sizeof first_bad, hipMemcpyDeviceToHost) != hipSuccess) first_bad = 1;
  int lim = 1;
  while ((u32) (lim << 1) <= first_bad && lim < (1 << 22)) lim <<= 1;  // largest power of two <= first mismatch
  m.block_shift_limit = first_bad <= 1 ? 0 : lim;
  if (dbg) fprintf(stderr, "[mrhash_hip] voxel->block is a shift for |v| < %d (first mismatch at %u, voxel size %g)\n", m.block_shift_limit, first_bad, (double) m.vs);
  // correctly rounded reciprocals for the short divisions of the running mean (mrh_device.h: div_cr)
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
  bool ok = dev_alloc(c, c->d_rcp_w, dev.size() * sizeof(float)) == hipSuccess;  // its table is this check's alone: without it, two steps
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
  if (dbg) fprintf(stderr, "[mrhash_hip] division by vs / 2 with one residual step: %u mismatches over the working range -> %s; refined reciprocals of the weight sums: %d not correctly rounded\n", bad, bad ? "two steps" : "one step", w_bad);
  return MRH_OK;
}

// The three ways a create-time switch is read.  A switch that is not set, or set outside what it accepts, leaves the default.
template <typename T> void env_onoff(const char* name, T& v) { if (const char* g = getenv(name)) v = atoi(g) ? 1 : 0; }  // NAME=0 off, any other integer on
inline bool env_present(const char* name) { return getenv(name) != nullptr; }  // whatever it is set to
template <typename T> void env_int(const char* name, const int64_t lo, const int64_t hi, T& v) {  // an integer in [lo, hi]
  if (const char* g = getenv(name)) { const int x = atoi(g); if (x >= lo && x <= hi) v = (T) x; }
}

// The single place the switches that hold for a context's life are read (per-call ones are read where they act).  What a switch
// does is written beside the member it sets.
void read_switches(mrh_ctx* c) {
  constexpr int64_t kIntMax = 0x7FFFFFFF;
  env_int("MRH_FUSED_GRID", 1, 32768, c->fused_grid);  // tuning knob: workgroups (x4 waves) of the fused integrate kernel
  env_onoff("MRH_DEFER_UPLOADS", c->defer_uploads);
  env_onoff("MRH_PIPE", c->pipe);
  env_onoff("MRH_STARVE_FUSED", c->starve_fused);
  c->starve_serial = env_present("MRH_STARVE_SERIAL");
  c->pipe_always_wait = env_present("MRH_PIPE_ALWAYS_WAIT");
  env_int("MRH_PIPE_GRID", 1, 32768, c->pipe_grid);
  env_int("MRH_PIPE_DEFER", 1, PipeState::kPendMax - 1, c->pipe_defer);
  env_onoff("MRH_PIPE_UPLOADS", c->pipe_uploads);
  env_int("MRH_PIPE_PERIOD", 1, kIntMax, c->pipe_period);
  env_int("MRH_SWEEP_WGS", 1, 4096, c->sweep_wgs);
  env_int("MRH_SWEEP_WGS_MR", 1, 4096, c->sweep_wgs_mr);
  env_onoff("MRH_MR_FUSED", c->mr_fused);
  env_int("MRH_ZLIST_CAP", 1, (int64_t) c->num_blocks - 1, c->fast.zlist_cap);  // Fast::zlist_cap below the pool size (tests)
  int safe_div = 0, rehash_off = 0;
  env_onoff("MRH_SAFE_DIV", safe_div);  // =1: force the fallback instantiation of the short divisions (tests)
  if (safe_div) c->map.half_vs_two_steps = 1;
  c->heap_descending = env_present("MRH_DEBUG_HEAP_DESCENDING") ? 1 : 0;
  env_onoff("MRH_PREWARM", c->prewarm_on);
  env_onoff("MRH_MESH_HOST", c->mesh_on_host);
  env_onoff("MRH_MESH_F64_LINK", c->f64_link);
  c->V.pin = c->C.pin = c->f64_link;  // fp32 link: the doubles are written by the host only
  env_onoff("MRH_QTREE_LITERAL", c->qt.literal);
  env_int("MRH_SCAN_ROW_LEN", -kIntMax - 1, kIntMax, c->lidar.layout_hint);
  env_int("MRH_SCAN_PATCH_LOG2", 0, 8, c->lidar.patch_log2);
  env_onoff("MRH_LIDAR_BUCKETS", c->lidar.use_buckets);
  env_onoff("MRH_NORMALS_FOLD", c->nrm.fold);
  if (const char* g = getenv("MRH_SCAN_SEQ_START")) c->lidar.buckets_seq = (u32) strtoul(g, nullptr, 0);  // tests: scans next to the wrap of the block stamps
  env_int("MRH_REHASH_PERIOD", 1, kIntMax, c->census_period);
  env_onoff("MRH_REHASH_FORCE", c->census_force);
  env_onoff("MRH_REHASH_OFF", rehash_off);  // =1: no upkeep at all (tests: shows what it prevents)
  if (rehash_off) c->census_period = -1;
}

}  // namespace
