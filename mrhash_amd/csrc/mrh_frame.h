// mrh_frame.h — the host side of a depth frame (voxel_data_structures.cpp:90-110 VoxelContainer::integrate, as one sync-free kernel
// chain): the inputs a frame is issued under and their deferral (FrameInputs), the table upkeep in front of a frame, the plan that
// holds every per-frame decision (FramePlan, mrh_context.h), the launch sites of k_front / k_back / the starve kernels, the
// pipeline (launch_pending, strict_point, mrh_ctx::ps) and the three frame paths.  Needs mrh_context.h, mrh_upload.h and the
// shared helpers at the top of mrh_capi.hip; mrh_points.h uses frame_upkeep, refill_coarse, plan_begin and starve_and_tail.
#pragma once
namespace {

// ---- the two cross-stream invariants of PipeState (mrh_context.h), each enforced in one place ----
// (a) main_stream_changed_map (mrh_context.h) says that the main stream has changed keys or the free list while the front stream
// was not looking; the next front half is launched only after the host has seen the main stream drain:
int resync_front(mrh_ctx* c) {
  PipeState& ps = c->ps;
  if (!ps.front_needs_sync) return MRH_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ps.front_needs_sync = false;
  ps.base = ps.seq - 1;  // (the frame that is being issued has taken its sequence number)
  return MRH_OK;
}
// (b) is strict_point, below.

// ---- a frame's inputs: read out of the context, put back ----
FrameInputs read_inputs(const mrh_ctx* c) {
  FrameInputs in;
  in.cam = c->cam;
  in.d_depth = c->d_depth; in.d_rgb = c->d_rgb;
  in.depth_rows = c->depth_rows; in.depth_cols = c->depth_cols; in.rgb_rows = c->rgb_rows; in.rgb_cols = c->rgb_cols;
  const UpRing* rings[2] = {&c->up_depth, &c->up_rgb};
  for (int i = 0; i < 2; i++) in.ring[i] = {rings[i]->cur, rings[i]->last_copy, {rings[i]->waited[0], rings[i]->waited[1]}};
  return in;
}
void apply_inputs(mrh_ctx* c, const FrameInputs& in) {
  c->cam = in.cam;
  c->d_depth = in.d_depth; c->d_rgb = in.d_rgb;
  c->depth_rows = in.depth_rows; c->depth_cols = in.depth_cols; c->rgb_rows = in.rgb_rows; c->rgb_cols = in.rgb_cols;
  UpRing* rings[2] = {&c->up_depth, &c->up_rgb};
  for (int i = 0; i < 2; i++) {
    rings[i]->cur = in.ring[i].cur; rings[i]->last_copy = in.ring[i].last_copy;
    rings[i]->waited[0] = in.ring[i].waited[0]; rings[i]->waited[1] = in.ring[i].waited[1];
  }
}

// ---- table upkeep in front of a frame ----
// Table upkeep between two frames (mrh_kernels.h): census of the tombstones every `census_period` frames or after a bulk
// change, rebuild decided on the device.  Four short launches, no host round trip.
bool census_due(const mrh_ctx* c) { return c->census_period >= 0 && (c->table_dirty || c->frames_since_census >= (uint64_t) c->census_period); }
int maintain_table(mrh_ctx* c) {
  if (c->pending || !census_due(c)) return MRH_OK;
  hipStream_t s = c->stream;
  const Tab& t = c->tab;
  const int grid = (int) std::min<uint64_t>(2048, (c->slots + 255) / 256);
  main_stream_changed_map(c);  // a rebuild moves keys
  k_table_census<<<grid, 256, 0, s>>>(t, (size_t) c->slots);
  k_rehash_decide<<<1, 1, 0, s>>>(t, (u32) (c->slots / 4), c->census_force);
  k_rehash_clear<<<grid, 256, 0, s>>>(t, (size_t) c->slots);
  k_rehash_insert<<<1024, 256, 0, s>>>(t);
  c->frames_since_census = 0;
  c->table_dirty = false;
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// What every frame — images or a scan — does to the table before its kernels.  The table is rebuilt only with no frame in flight:
// the upkeep rebuilds from the descriptors, so the pending integrations run and the zombies of the pipelined frames leave first.
int frame_upkeep(mrh_ctx* c) {
  if (census_due(c) && (c->ps.npend > 0 || c->ps.zombies_possible)) {
    const int rc = strict_point(c);
    if (rc) return rc;
  }
  const int rc = maintain_table(c);
  if (rc) return rc;
  c->frames_since_census++;
  return MRH_OK;
}

// coarse free-list refill of a multi-resolution map, decided on the device (vds.cu:885-891, :1048-1054)
void refill_coarse(mrh_ctx* c) {
  k_refill_decide<<<1, 64, 0, c->stream>>>(c->tab, c->low_blocks_to_allocate, c->d_flag);
  k_refill<<<(c->low_blocks_to_allocate + 255) / 256, 256, 0, c->stream>>>(c->tab, c->low_blocks_to_allocate, c->d_flag);
}

// ---- the plan ----
// What a plan holds for every frame, images or a scan (mrh_points.h plans its general frame with this alone)
void plan_begin(const mrh_ctx* c, FramePlan& p, const FrameKind kind, const int n_frames_invalidate) {
  p = FramePlan{};
  p.kind = kind;
  p.max_num_frames = n_frames_invalidate < 0 ? c->p.n_frames_invalidate_voxels : n_frames_invalidate;
  p.starve_now = p.max_num_frames > 0 && c->frames > 0 && c->frames % (uint64_t) p.max_num_frames == 0;  // voxel_data_structures.cpp:139
  p.gc_thr = c->map.trunc + c->map.trunc_scale * c->cam.max_depth;  // getTruncation(camera.maxDepth(), ...), vds.cu:1720
}

// ... and for a depth frame, up to the choice between a pipelined and a serial frame (integrate_single_res_frame) and the slots
// (take_slots).  Multi-resolution maps take the two launches when that is exact: the fused kernel checks the variance of a
// fine block right after updating it, which covers every block the reference's checkVarSDF can newly decide on —
// EXCEPT blocks that changed without being checked (frame 0 is never checked, voxel_data_structures.cpp:99; the starve
// step decrements weights after the check; imported blocks) and are then outside the image on the next frame.  Those
// frames, and the starve frames themselves, go through the general kernels.
void plan_frame(const mrh_ctx* c, FramePlan& p, const int n_frames_invalidate) {
  plan_begin(c, p, FRAME_SERIAL, n_frames_invalidate);  // (a frame of a single-resolution map always takes the two launches)
  const Cam& k = c->cam;
  if (c->tab.multi_res) {
    const bool fused = c->mr_fused && !c->profile && p.max_num_frames > 0 && !p.starve_now && !c->mr_next_general && c->frames >= 2 && !c->spherical;
    p.kind = fused ? FRAME_FUSED_MR : FRAME_GENERAL;
  }
  // may the starve step take the three fused launches?  (tile-sharded maps reduce the z-buffers over the ranks between the passes,
  // multi-resolution and general frames walk lists of another kind: they keep k_starve<0,1,2>)
  p.starve_fused = c->starve_fused && c->p.shard_count <= 1 && p.kind == FRAME_SERIAL;
  // a starve frame stays a frame of the pipeline when its starve step can take the fused launches (round 6; before: every starve
  // frame flushed the pipeline, ran serially and left a host synchronisation in front of the next pipelined frame)
  p.starve_in_pipe = p.starve_now && p.starve_fused && !c->starve_serial;
  // GC runs inside k_back unless this is a starve frame (the starve step changes weights after the integrate pass)
  p.gc_inline = p.kind == FRAME_FUSED_MR || (p.kind == FRAME_SERIAL && p.max_num_frames > 0 && !p.starve_now);
  p.safe_div = c->map.half_vs_two_steps || c->map.wsum_two_steps;  // the short divisions failed their check at mrh_create
  p.sph = c->spherical;
  p.tiles_x = (k.cols + kRayTile - 1) / kRayTile;
  p.n_tiles = p.tiles_x * ((k.rows + kRayTile - 1) / kRayTile);
}

// the counters advance: the frame's sequence number and ring slot (two-launch frames of a single-resolution map), its list-counter
// set with the one to clear, its stamp
void take_slots(mrh_ctx* c, FramePlan& p) {
  PipeState& ps = c->ps;
  if (p.kind != FRAME_FUSED_MR) {
    p.seq = (int) (ps.seq & 0x3FFFFFFF);
    p.ring = p.kind == FRAME_PIPELINED ? (int) (ps.seq % kPipeRing) : 0;  // a serial frame runs behind everything on the main stream: any slot
    ps.seq++;                                                             // is free for it, and the starve passes walk slot 0's lists
  }
  p.set = (int) (ps.fast_frames % kListSets);
  p.zero_set = (p.set + kListSets - 1) % kListSets;
  ps.fast_frames++;
  p.stamp = (u32) ((c->frames + 1) & 0x3FFFFFFFu);
}

// ---- launch sites ----
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
  const PipeState& ps = c->ps;
  return Lists{ps.ring_vis[i], ps.ring_bbox[i], ps.ring_cfree[i], ps.ring_zmin[i], (u32) c->num_blocks};
}

// k_back's and k_front's arguments, in the kernels' parameter order (mrh_fast2.h), each built from a plan and the {camera, fast-path
// buffers, lists} the frame was issued with
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
BackArgs back_args(const mrh_ctx* c, const FramePlan& p, const Cam& k, const Fast& f, const Lists& L) {
  if (p.kind == FRAME_FUSED_MR) return {k, c->map, c->tab, f, L, p.set, p.zero_set, p.gc_thr, c->d_depth, c->d_rgb, (u32*) c->d_reint, 0u, 0};
  return {k, c->map, c->tab, f, L, p.set, p.zero_set, p.gc_thr, nullptr, nullptr, nullptr, p.stamp, p.seq};
}
int refill_wgs(const mrh_ctx* c) { return (c->low_blocks_to_allocate + 255) / 256; }
FrontArgs front_args(const mrh_ctx* c, const FramePlan& p, const Cam& k, const Fast& f, const Lists& L) {
  const int gc_on = p.max_num_frames > 0 ? 1 : 0;
  if (p.kind == FRAME_FUSED_MR)
    return {k, c->map, c->tab, f, L, c->d_depth, c->d_rgb, p.tiles_x, p.n_tiles, p.stamp, p.set, gc_on, p.gc_thr, refill_wgs(c), c->low_blocks_to_allocate, c->d_flag};
  return {k, c->map, c->tab, f, L, c->d_depth, c->d_rgb, p.tiles_x, p.n_tiles, p.stamp, p.set, gc_on, p.gc_thr, 0, 0, nullptr};
}

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
// The one launch site of k_back.  The plan's flags, in the kernel's template order, pick one of the instantiations the library
// builds: single-resolution frames FREE (= gc_inline) x SAFEDIV x LZ (0: serial, 2: pipelined) x SPH, with the roofline counters
// (PROFILE) on the profile launches of the frames that collect inline — a starve frame's profile launch carries its event pair
// only —; the fused multi-resolution frame FREE, MULTI x SAFEDIV (never profiled, pipelined or spherical).
void launch_back(const FramePlan& p, const int grid, hipStream_t s, const EvPair* ev, const BackArgs& a) {
  if (p.kind == FRAME_FUSED_MR) {
    if (p.safe_div) back_as<true, false, true, true, 0, false>(grid, s, ev, a);
    else back_as<true, false, true, false, 0, false>(grid, s, ev, a);
  } else if (p.kind == FRAME_PIPELINED) {
    if (p.gc_inline && ev) back_single_res<true, true, 2>(p.safe_div, p.sph, grid, s, ev, a);
    else if (p.gc_inline) back_single_res<true, false, 2>(p.safe_div, p.sph, grid, s, ev, a);
    else back_single_res<false, false, 2>(p.safe_div, p.sph, grid, s, ev, a);
  } else {
    if (p.gc_inline && ev) back_single_res<true, true, 0>(p.safe_div, p.sph, grid, s, ev, a);
    else if (p.gc_inline) back_single_res<true, false, 0>(p.safe_div, p.sph, grid, s, ev, a);
    else back_single_res<false, false, 0>(p.safe_div, p.sph, grid, s, ev, a);
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
// The one launch site of k_front: single-resolution frames PROFILE (= a profile launch, `ev` given) x LAZY (a pipelined frame) x
// SPH, the fused multi-resolution frame MULTI alone.
void launch_front(const FramePlan& p, const int grid, hipStream_t s, const EvPair* ev, const FrontArgs& a) {
  if (p.kind == FRAME_FUSED_MR) front_as<false, true, false, false>(grid, s, nullptr, a);
  else if (ev) front_single_res<true>(p.kind == FRAME_PIPELINED, p.sph, grid, s, ev, a);
  else front_single_res<false>(p.kind == FRAME_PIPELINED, p.sph, grid, s, nullptr, a);
}

// ---- the starve step and the rest of a frame ----
int ensure_zbuf(mrh_ctx* c, size_t npix) { return regrow(c, c->d_zbuf, c->zbuf_n, npix, 2 * npix * sizeof(u64)); }

// the z-buffers of the fused starve launches: two pairs of 2 x npix keys; new memory holds no "empty" pair
int ensure_zfused(mrh_ctx* c, const size_t npix) {
  PipeState& ps = c->ps;
  if (ps.zfused_n >= npix) return MRH_OK;
  ps.zfused_clean[0] = ps.zfused_clean[1] = false;
  return regrow(c, ps.d_zfused, ps.zfused_n, npix, 4 * npix * sizeof(u64));
}

// The one launch site of k_starve_z and k_starve_tail, LZ: 2 = a pipelined frame (collected blocks become zombies), 0 = a serial one
template <bool SPH, int LZ>
void starve_fused_as(hipStream_t s, const Cam& k, const Map& m, const Tab& t, const Fast& f, const Lists& L, const FramePlan& p, u64* z0, u64* z1, u64* other,
                     const size_t npix) {
  const int grid = 2048;  // x 4 waves, one block each per round
  k_starve_z<0, SPH><<<grid, 256, 0, s>>>(k, m, t, f, L.vis, p.set, z0, z1);
  k_starve_z<1, SPH><<<grid, 256, 0, s>>>(k, m, t, f, L.vis, p.set, z0, z1);
  k_starve_tail<LZ, SPH><<<grid, 256, 0, s>>>(k, m, t, f, L, p.set, p.gc_thr, p.stamp, z0, z1, other, 2 * npix);
}
// A starve frame of a single-resolution, unsharded map on the two-launch path: behind the frame's k_back<FREE = false>, the two
// min-passes and the tail (pass 2 + summaries + garbage collection + the other z-buffer pair cleared) — three launches on the main
// stream, nothing of the pipeline flushed.
int launch_starve_fused(mrh_ctx* c, const FramePlan& p, const Cam& k, const Fast& f, const Lists& L) {
  PipeState& ps = c->ps;
  const size_t npix = (size_t) k.rows * k.cols;
  hipStream_t s = c->stream;
  const int rc = ensure_zfused(c, npix);
  if (rc) return rc;
  if (ps.zfused_clean_npix != npix) ps.zfused_clean[0] = ps.zfused_clean[1] = false;  // the camera changed size since the pairs were cleared
  ps.zfused_clean_npix = npix;
  const int pair = ps.zfused_next, q = pair ^ 1;
  u64* z0 = ps.d_zfused + (size_t) pair * 2 * ps.zfused_n;
  u64* z1 = z0 + npix;
  u64* other = ps.d_zfused + (size_t) q * 2 * ps.zfused_n;
  // "empty" = INT64_MAX: above every key (depth bits of a finite positive float < 0x7F800000)
  if (!ps.zfused_clean[pair]) k_fill_u64<<<256, 256, 0, s>>>(z0, 2 * npix, 0x7FFFFFFFFFFFFFFFull);
  ps.zfused_clean[pair] = false;
  const bool lazy = p.kind == FRAME_PIPELINED;
  if (k.model && lazy) starve_fused_as<true, 2>(s, k, c->map, c->tab, f, L, p, z0, z1, other, npix);
  else if (k.model) starve_fused_as<true, 0>(s, k, c->map, c->tab, f, L, p, z0, z1, other, npix);
  else if (lazy) starve_fused_as<false, 2>(s, k, c->map, c->tab, f, L, p, z0, z1, other, npix);
  else starve_fused_as<false, 0>(s, k, c->map, c->tab, f, L, p, z0, z1, other, npix);
  HIP_TRY(c, hipGetLastError());
  ps.zfused_clean[q] = true;
  ps.zfused_next = q;
  c->n_starve_fused++;
  return MRH_OK;
}

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
int frame_tail(mrh_ctx* c, const FramePlan& p) {
  hipStream_t s = c->stream;
  const Tab& t = c->tab;
  if (p.kind == FRAME_GENERAL) {  // garbageCollectIdentify + garbageCollectFree over the compact list (vds.cu:1674-1713, :1827-1844)
    if (p.max_num_frames > 0) {
      k_gc_identify<<<c->integrate_grid, 512, 0, s>>>(t, p.gc_thr, c->d_decision);
      if (c->profile) k_gc_free<true><<<256, 256, 0, s>>>(t, c->d_decision);
      else k_gc_free<false><<<256, 256, 0, s>>>(t, c->d_decision);
    }
    if (!t.multi_res) c->fast_summaries_stale = true;  // the general kernels do not maintain the fast path's GC summaries
  } else if (!t.multi_res) {
    if (p.starve_now) k_summarize_visible<<<1024, 256, 0, s>>>(t, c->fast);  // weights changed: the GC summaries follow the payload
    if (p.max_num_frames > 0 && !p.gc_inline) k_free_lists<<<256, 256, 0, s>>>(t, c->fast, ring_lists(c, 0), p.set, p.gc_thr);
  }
  c->frames++;
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// starve (voxel_data_structures.cpp:139) + the rest of the frame; sharded contexts stop for the host's min-reduction (resume_frame)
int starve_and_tail(mrh_ctx* c, const FramePlan& p) {
  if (p.starve_now) {
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
      return frame_tail(c, p);
    }
    if (c->p.shard_count > 1) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      c->pending = 1;  // c->plan is this frame's until resume_frame has run its tail
      return MRH_PENDING_EXCHANGE;
    }
    if ((rc = launch_starve(c, 1))) return rc;
    if ((rc = launch_starve(c, 2))) return rc;
  }
  return frame_tail(c, p);
}

// mrh_integrate_resume: the host has reduced a z-buffer over the shards
int resume_frame(mrh_ctx* c) {
  if (c->pending == 1) {
    launch_starve(c, 1);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->pending = 2;
    return MRH_PENDING_EXCHANGE;
  }
  if (c->pending == 2) {
    launch_starve(c, 2);
    c->pending = 0;
    const int rc = frame_tail(c, c->plan);
    if (rc < 0) return rc;
    const int mrc = mark_frame(c);  // the tail's kernels read the frame's images too
    return mrc ? mrc : rc;
  }
  return fail(c, MRH_ERR_STATE, "mrh_integrate_resume: no exchange is pending");
}

// ---- the pipeline ----
// the integration of the oldest pending pipelined frame, behind its front half
int launch_pending(mrh_ctx* c, const bool count_skips = false) {
  PipeState& ps = c->ps;
  if (!ps.npend) return MRH_OK;
  const PendingBack pb = ps.pendq[0];  // the oldest
  for (int i = 1; i < ps.npend; i++) ps.pendq[i - 1] = ps.pendq[i];
  ps.npend--;
  const FramePlan& p = pb.plan;
  hipStream_t s = c->stream;
  const hipError_t q = c->pipe_always_wait ? hipErrorNotReady : hipEventQuery(ps.ev_front[p.ring]);
  if (q == hipErrorNotReady) {
    (void) hipGetLastError();
    HIP_TRY(c, hipStreamWaitEvent(s, ps.ev_front[p.ring], 0));
    c->dbg_waits++;
  } else if (q != hipSuccess) {
    return fail(c, MRH_ERR_DEVICE, "mrh_integrate: front half of a pipelined frame: %s", hipGetErrorString(q));
  }
  const bool profiled = pb.ev.a != nullptr;  // the frame was issued in profile mode: it holds an event pair
  if (count_skips) HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_ZSKIP], 0, sizeof(int), s));  // mrh_get_stats: M of the last frame, exactly
  if (profiled)  // U and M of the frame (device-side counters of the roofline numerator): after its front half, before its integration
    k_count_updates<<<c->fused_grid, 256, 0, s>>>(pb.cam, c->map, c->tab, pb.f, c->d_cnt_partials, CTR_SET0 + 4 * p.set, pb.L.vis, pb.L.cfree, p.stamp,
                                                  pb.count_zombies ? 1 : 0);
  launch_back(p, c->pipe_grid, s, profiled ? &pb.ev : nullptr, back_args(c, p, pb.cam, pb.f, pb.L));
  if (profiled) c->ev_pending.push_back(pb.ev);
  if (p.gc_inline) ps.zombies_possible = true;
  if (p.starve_now) {  // behind the integration (which collects nothing) the three fused starve launches
    const int src = launch_starve_fused(c, p, pb.cam, pb.f, pb.L);
    if (src) return src;
    ps.zombies_possible = true;
  }
  HIP_TRY(c, hipGetLastError());
  // the frame's pool report (mark_frame left it to this launch): behind its integration
  return pb.report_seq && c->peek_enabled ? post_report(c, pb.report_seq, s) : MRH_OK;
}

// Invariant (b): anything that is not a pipelined frame meets the map only behind this.  Behind the pipelined frames issued so far
// (their integrations are all on the main stream, each behind its front half), the zombies nobody wanted leave the table:
// k_reclaim runs alone on the main stream — the front stream is idle once the last integration has started, and nothing is
// enqueued on it before the host has seen the main stream drain (invariant (a)).
int strict_point(mrh_ctx* c) {
  PipeState& ps = c->ps;
  while (ps.npend) {
    const int rc = launch_pending(c, ps.npend == 1);
    if (rc) return rc;
  }
  if (!ps.zombies_possible) return MRH_OK;
  main_stream_changed_map(c);
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
  ps.zombies_possible = false;
  ps.lazy_run = 0;
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// what mrh_ctx::PipeState holds for as long as the context lives, created at the first single-resolution frame of a context with `pipe` set
int ensure_pipe_state(mrh_ctx* c) {
  PipeState& ps = c->ps;
  if (ps.stream_front) return MRH_OK;
  const size_t cap = c->num_blocks;
  // the stream comes last: it is what says "the state exists", and a step that failed is taken again by the next call
  // (hipEventDisableSystemFence on these events — they order two streams of one device — was measured in round 5: no difference)
  for (hipEvent_t& e : ps.ev_front) if (!e) HIP_TRY(c, event_new(c, e, false));
  for (int i = 1; i < kPipeRing; i++) {
    if (!ps.ring_vis[i]) HIP_TRY(c, dev_alloc(c, ps.ring_vis[i], cap * sizeof(int4)));
    if (!ps.ring_bbox[i]) HIP_TRY(c, dev_alloc(c, ps.ring_bbox[i], cap * sizeof(int4)));
    if (!ps.ring_cfree[i]) HIP_TRY(c, dev_alloc(c, ps.ring_cfree[i], cap * sizeof(int4)));
    if (!ps.ring_zmin[i]) HIP_TRY(c, dev_alloc(c, ps.ring_zmin[i], cap * sizeof(float)));
  }
  if (!c->fast.zlist) HIP_TRY(c, dev_alloc(c, c->fast.zlist, cap * sizeof(int4)));
  if (!ps.want_ring) HIP_TRY(c, dev_alloc(c, ps.want_ring, (size_t) kPipeRing * c->slots * sizeof(u32)));
  main_stream_changed_map(c);  // (the memset below: the front stream reads the stamps)
  HIP_TRY(c, hipMemsetAsync(ps.want_ring, 0, (size_t) kPipeRing * c->slots * sizeof(u32), c->stream));  // stamps start at 1
  if (!ps.h_levels) HIP_TRY(c, pinned_alloc(c, ps.h_levels, 4 * sizeof(int)));
  // (a high-priority front stream, a ring of eight and integrations deferred by two calls were measured: no difference)
  HIP_TRY(c, hipStreamCreateWithFlags(&ps.stream_front, hipStreamNonBlocking));
  ps.h_levels[0] = (int) c->num_blocks - 1; ps.h_levels[1] = 0; ps.h_levels[2] = -1;
  c->tab.h_levels = ps.h_levels;
  return MRH_OK;
}

// Fast::dcx of the two-launch frames, grow-only: one image per ring slot with the pipelining state, slot 0's alone without it
int ensure_frame_dcx(mrh_ctx* c, const size_t npix) {
  PipeState& ps = c->ps;
  if (ps.npix >= npix) return MRH_OK;
  {
    const int rc = strict_point(c);  // the pending integrations read the buffers that are about to go
    if (rc) return rc;
  }
  if (ps.stream_front) HIP_TRY(c, hipStreamSynchronize(ps.stream_front));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint2*& d : ps.dcx) HIP_TRY(c, dev_free(c, d));
  ps.npix = 0;
  const int n = ps.stream_front ? kPipeRing : 1;
  for (int i = 0; i < n; i++) HIP_TRY(c, dev_alloc(c, ps.dcx[i], npix * sizeof(uint2)));
  ps.npix = npix;
  return MRH_OK;
}

// room in the pool, as the last integration launch reported it (a few frames old: the margins are generous).  Pipelining state only.
bool pool_roomy(const mrh_ctx* c) {
  const volatile int* lev = c->ps.h_levels;
  const int64_t free_known = (int64_t) lev[0] + 1, zombies_known = lev[1];
  return free_known >= (int64_t) (c->num_blocks / 4) && zombies_known <= (int64_t) (c->num_blocks / 8);
}

// ring slot p.ring was last used by frame seq - kPipeRing; its integration is complete once the one after it has started, and
// that one has also cleared the list-counter set this frame appends to: the host holds back until then
int wait_for_ring_slot(mrh_ctx* c, const FramePlan& p) {
  const int64_t need = (int64_t) p.seq - kPipeRing + 2;
  if (need <= (int64_t) c->ps.base) return MRH_OK;
  const auto t0 = std::chrono::steady_clock::now();
  while ((int64_t) ((volatile int*) c->ps.h_levels)[2] < need) {
    MRH_CPU_RELAX();
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) return fail(c, MRH_ERR_DEVICE, "mrh_integrate: the integration of frame %lld never started", (long long) need);
  }
  c->dbg_spin_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  return MRH_OK;
}

// ---- the three frame paths ----
// One frame of a single-resolution map (pinhole or spherical camera):
//   pipelined: front stream: k_front<LAZY> (+ event) | main stream: wait for that event, k_back<LZ = 2>.  The front stream never
//              waits for the main one, so this frame's front half runs next to the integration of the frame(s) before it;
//              the host only holds back when it is kPipeRing - 1 frames ahead of the integration that has started.
//   serial:    [k_reclaim] -> k_front -> k_back (-> the starve passes), all on the main stream, no zombies anywhere.
// A serial frame comes with MRH_PIPE=0, after anything else touched the map, every `pipe_period` frames (the reclaim bounds the
// zombies), on starve frames that cannot stay in the pipeline, and while the pool is short of room: zombies hold their pool slots
// until the reclaim, so a pool that is nearly full is fused serially — the reference's accounting, exactly.
// Three more terms: a caller that synchronises (or asks for statistics, a mesh, ...) after EVERY frame gains nothing from the
// pipeline and would pay for its flush each time: three frames in a row that found the pipeline flushed (sync_streak) switch to
// serial frames, the first frame that follows another frame directly switches back.  And images that come from the host
// (mrh_upload_*) make the frame loop host- and link-bound (staging copy + 2.15 MB over PCIe: ~60 us per frame at 640x480 against
// ~40 us of GPU work): nothing to gain from overlapping kernels, and the second stream's events only add to the host's bill
// (measured: 77 us per frame pipelined, 64 serial) — such frames are fused serially unless MRH_PIPE_UPLOADS=1 says otherwise (the
// test-suite sets it, so that its upload-fed streams exercise the pipeline).
bool frame_may_pipeline(const mrh_ctx* c, const FramePlan& p) {
  const bool resident_inputs = c->up_depth.cur < 0 && c->up_rgb.cur < 0;
  return c->pipe && (!p.starve_now || p.starve_in_pipe) && pool_roomy(c) && c->ps.lazy_run < c->pipe_period && c->ps.sync_streak < 3 &&
         (resident_inputs || c->pipe_uploads);
}
int integrate_single_res_frame(mrh_ctx* c, FramePlan& p) {
  PipeState& ps = c->ps;
  int rc = MRH_OK;
  hipStream_t s = c->stream;
  const Cam& k = c->cam;
  if (c->pipe) {
    rc = ensure_pipe_state(c);
    if (rc) return rc;
  }
  rc = ensure_frame_dcx(c, (size_t) k.rows * k.cols);
  if (rc) return rc;
  if (c->fast_summaries_stale) {  // a LiDAR scan (general kernels) ran since: rebuild the GC summaries once
    rc = strict_point(c);
    if (rc) return rc;
    main_stream_changed_map(c);
    k_summarize_all<<<2048, 256, 0, s>>>(c->tab, c->fast);
    c->fast_summaries_stale = false;
  }
  ps.sync_streak = ps.flushed_since_frame ? ps.sync_streak + 1 : 0;
  ps.flushed_since_frame = false;
  const bool lazy = frame_may_pipeline(c, p);
  if (lazy) p.kind = FRAME_PIPELINED;
  else if ((rc = strict_point(c))) return rc;
  rc = send_uploads(c, lazy ? ps.stream_front : s);  // the raw images are read by the front half
  if (rc) return rc;
  take_slots(c, p);
  c->fast.dcx = ps.dcx[p.ring];
  c->fast.want = ps.want_ring + (size_t) p.ring * c->slots;  // (no want stamps without the pipelining state: nullptr)
  const Fast f = c->fast;
  const Lists L = ring_lists(c, p.ring);
  EvPair ev = {nullptr, nullptr}, evf = {nullptr, nullptr};
  if (c->profile) {
    rc = take_event_pair(c, evf);
    if (rc) return rc;
    rc = take_event_pair(c, ev);
    if (rc) return rc;
  }
  const FrontArgs front = front_args(c, p, k, f, L);
  ps.last_frame_lazy = lazy;
  if (lazy) {
    rc = resync_front(c);
    if (rc) return rc;
    rc = wait_for_ring_slot(c, p);
    if (rc) return rc;
    c->dbg_lazy_frames++;
    const auto t_api = std::chrono::steady_clock::now();
    launch_front(p, p.n_tiles + c->sweep_wgs, ps.stream_front, c->profile ? &evf : nullptr, front);
    HIP_TRY(c, hipEventRecord(ps.ev_front[p.ring], ps.stream_front));
    if (c->profile) c->ev_pending_front.push_back(evf);
    // the integration of the PREVIOUS pipelined frame goes out now (its front half ran a frame ago: usually no wait), this
    // frame's is left for the next call
    const bool zombies_before = ps.zombies_possible;
    while (ps.npend >= c->pipe_defer) {
      rc = launch_pending(c);
      if (rc) return rc;
    }
    PendingBack& pb = ps.pendq[ps.npend++];  // (written in place: a frame copies its camera and buffers once)
    pb.plan = p; pb.cam = k; pb.f = f; pb.L = L;
    pb.ev = ev;
    pb.report_seq = 0;
    pb.count_zombies = zombies_before || ps.zombies_possible || p.gc_inline;
    ps.lazy_run++;
    c->frames++;  // frame_tail's bookkeeping; nothing else of it applies (GC runs inside the integration)
    c->dbg_api_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_api).count();
    HIP_TRY(c, hipGetLastError());
    return MRH_OK;
  }
  // ---- serial frame, all on the main stream (strict_point above has flushed and reclaimed)
  main_stream_changed_map(c);  // direct frees on the main stream
  launch_front(p, p.n_tiles + c->sweep_wgs, s, c->profile ? &evf : nullptr, front);
  if (c->profile) {
    c->ev_pending_front.push_back(evf);
    k_count_updates<<<c->fused_grid, 256, 0, s>>>(k, c->map, c->tab, f, c->d_cnt_partials, CTR_SET0 + 4 * p.set, L.vis, L.cfree, p.stamp, 0);
  }
  launch_back(p, c->fused_grid, s, c->profile ? &ev : nullptr, back_args(c, p, k, f, L));
  if (c->profile) c->ev_pending.push_back(ev);
  if (p.starve_now && p.starve_fused) {
    rc = launch_starve_fused(c, p, k, f, L);
    if (rc) return rc;
    c->frames++;  // frame_tail's bookkeeping: the summaries and the garbage collection ran inside the tail launch
    return MRH_OK;
  }
  return starve_and_tail(c, p);
}

// One fused frame of a multi-resolution map, on the main stream: k_front<MULTI> (with the coarse-list refill, vds.cu:885-891),
// k_back<MULTI> (GC inline, the re-integration of what checkVarSDF reallocated), k_mr_tail.
int integrate_fused_mr_frame(mrh_ctx* c, FramePlan& p) {
  hipStream_t s = c->stream;
  const Cam& k = c->cam;
  const Tab& t = c->tab;
  int rc = ensure_frame_dcx(c, (size_t) k.rows * k.cols);
  if (rc) return rc;
  c->fast.dcx = c->ps.dcx[0];
  const Fast& f = c->fast;
  take_slots(c, p);
  const Lists L = ring_lists(c, 0);
  if (!c->mr_summaries_valid) {
    k_summarize_all<<<2048, 256, 0, s>>>(t, f);
    c->mr_summaries_valid = true;
  }
  // the coarse-list refill rides in k_front; its test was taken by the previous frame's k_mr_tail unless something else touched
  // the coarse list since (general frames, import, stream-out, reset)
  if (!c->refill_flag_valid) k_refill_decide<<<1, 64, 0, s>>>(t, c->low_blocks_to_allocate, c->d_flag);
  launch_front(p, p.n_tiles + c->sweep_wgs_mr + refill_wgs(c), s, nullptr, front_args(c, p, k, f, L));
  launch_back(p, c->fused_grid, s, nullptr, back_args(c, p, k, f, L));
  k_mr_tail<<<1, 256, 0, s>>>(t, (const u32*) c->d_reint, c->low_blocks_to_allocate, c->d_flag);
  rc = starve_and_tail(c, p);
  c->refill_flag_valid = rc == MRH_OK;
  return rc;
}

// One frame of a multi-resolution map through the general kernels (mrh_kernels.h), on the main stream.
int integrate_general_frame(mrh_ctx* c, const FramePlan& p) {
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

  return starve_and_tail(c, p);
}

// ---- a frame, from the checks to its mark ----
// what mrh_integrate rejects before it touches the device
int integrate_checks(mrh_ctx* c) {
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

// checks, upkeep, the plan, and the path of the frame's kind: the two launches of a single-resolution map (pipelined or serial), a
// fused or a general multi-resolution frame
int integrate_frame(mrh_ctx* c, const int n_frames_invalidate) {
  int rc = integrate_checks(c);
  if (rc) return rc;
  rc = frame_upkeep(c);
  if (rc) return rc;
  FramePlan& p = c->plan;
  plan_frame(c, p, n_frames_invalidate);
  if (p.kind == FRAME_GENERAL) {
    c->mr_summaries_valid = false;
    c->mr_next_general = p.starve_now || c->frames == 0;
    c->refill_flag_valid = false;
  }
  const size_t npix = (size_t) c->cam.rows * c->cam.cols;
  if (p.max_num_frames > 0 && p.starve_fused && c->ps.zfused_n < npix) {
    // the z-buffers of the starve frames, both pairs empty, while the context is still allocating (not inside its first starve frame)
    rc = ensure_zfused(c, npix);
    if (rc) return rc;
    k_fill_u64<<<512, 256, 0, c->stream>>>(c->ps.d_zfused, 4 * npix, 0x7FFFFFFFFFFFFFFFull);
    c->ps.zfused_clean[0] = c->ps.zfused_clean[1] = true;
    c->ps.zfused_clean_npix = npix;
  }
  if (p.kind == FRAME_SERIAL) return integrate_single_res_frame(c, p);
  rc = send_uploads(c, c->stream);  // the frame's kernels read the images on the main stream
  if (rc) return rc;
  return p.kind == FRAME_FUSED_MR ? integrate_fused_mr_frame(c, p) : integrate_general_frame(c, p);
}

// a frame and its mark (upload-ring slots, pool report)
int run_frame(mrh_ctx* c, const int n_frames_invalidate) {
  const int rc = integrate_frame(c, n_frames_invalidate);
  if (rc < 0) return rc;
  const int mrc = mark_frame(c);
  return mrc ? mrc : rc;
}

// ---- host-fed frames are launched one mrh_integrate late (mrh_ctx::DeferredFrame) ----
// is this a frame of host images whose transfers are still on their way, on a context that may keep it back?
bool frame_is_deferrable(const mrh_ctx* c) {
  const bool up_d = c->up_depth.cur >= 0 && c->d_depth == c->up_depth.s[c->up_depth.cur].d && !c->up_depth.waited[0] && !c->up_depth.waited[1];
  const bool up_c = c->up_rgb.cur >= 0 && c->d_rgb == c->up_rgb.s[c->up_rgb.cur].d && !c->up_rgb.waited[0] && !c->up_rgb.waited[1];
  return c->defer_uploads && (up_d || up_c) && c->p.shard_count <= 1 && !c->comm && !c->profile;
}
int defer_frame(mrh_ctx* c, const int n_frames_invalidate) {
  const int rc = integrate_checks(c);  // what can be wrong with the call is reported by the call
  if (rc) return rc;
  c->deferred = {true, n_frames_invalidate, read_inputs(c)};
  return MRH_OK;
}
// runs the frame mrh_integrate kept back, with the inputs it was issued under; the context's current inputs (the next frame's
// pose and images may have arrived meanwhile) are put back afterwards
int flush_deferred(mrh_ctx* c) {
  DeferredFrame& d = c->deferred;
  if (!d.on) return MRH_OK;
  d.on = false;
  FrameInputs now = read_inputs(c);
  apply_inputs(c, d.in);
  const int rc = run_frame(c, d.n_inval);
  // A ring whose last_copy moved while the frame was held has a newer image of its kind, whose transfer nobody has waited for: it
  // keeps the newer transfer's marks.  Otherwise it is the same transfer, and what the frame has waited for stays waited for.
  const UpRing* rings[2] = {&c->up_depth, &c->up_rgb};
  for (int i = 0; i < 2; i++)
    if (now.ring[i].last_copy == d.in.ring[i].last_copy) { now.ring[i].waited[0] = rings[i]->waited[0]; now.ring[i].waited[1] = rings[i]->waited[1]; }
  apply_inputs(c, now);
  return rc;
}

}  // namespace
