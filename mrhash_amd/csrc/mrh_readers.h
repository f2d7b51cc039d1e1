// mrh_readers.h — the host side of the features that only read the map, behind the C ABI: raycasting (mrh_raycast[_spherical]
// [_device], kernels in mrh_raycast.h), distance fields (mrh_esdf[_device], mrh_esdf.h), tracking (mrh_track_depth / _scan
// [_device], mrh_track.h), render-free tracking (mrh_track_depth_sdf / _points_sdf[_device], mrh_sdftrack.h), point queries
// (mrh_query_points[_device], mrh_query.h), ray queries (mrh_cast_rays[_device], mrh_rays.h), the free-space layer (mrh_freespace_*,
// mrh_freespace.h; its carves and segments do not read the map and come in through free_enter), map-to-map fusion (mrh_resample_map /
// mrh_fuse_map, mrh_remap.h; the merge itself is mrh_blocks.h's unpack_records) and map-to-map registration (mrh_align_map,
// mrh_align.h).  What they share is here once: the way in (reader_enter: null context, the feature's argument plan from
// mrh_readerplan.h, ensure_ready; pair_enter and source_rc for the calls on two contexts), the way the blocking calls hand their
// result planes out of pinned memory (read_planes), the scan of u64 counts with its total (scan_total), host input through the one
// staging pair (stage_obs) and the two pose fits' reduction (linearise_sums) under the loop, the solve, the update and the
// report of mrh_tracksolve.h; the live-block list of the readers that walk the whole map is mrh_blocks.h's borrow_live_blocks.
// The state is mrh_ctx::ray, ::esdf, ::trk, ::query, ::rays, ::free, ::remap, ::align, ::fit and ::stage.  Included by mrh_capi.hip, same translation
// unit: it needs the context's internals (mrh_ctx, HIP_TRY, fail, regrow / regrow_all / regrow_pinned, pinned_alloc, ensure_ready).
#pragma once

namespace {

// Every reader's way in, in the order the C ABI documents: a null context, then what plan(msg) — the feature's
// argument plan — refuses, before the map is touched; then ensure_ready
template <typename PlanFn>
int reader_enter(mrh_ctx* c, const char* who, PlanFn&& plan) {
  if (!c) return MRH_ERR_INVALID_ARG;
  char msg[mrh_plan::kMsgBytes];
  const int rc = plan(msg);
  return rc ? fail(c, rc, "%s", msg) : ensure_ready(c, who);
}

// A failure of the source half of a call on two contexts, reported on dst with src's message; rc = 0 passes through
int source_rc(mrh_ctx* dst, const mrh_ctx* src, const char* who, const int rc) {
  return rc ? fail(dst, rc, "%s (source): %s", who, src->err.c_str()) : rc;
}
// The way in of the calls on two contexts (mrh_fuse_map, mrh_align_map), in the documented order: a null argument (reported on
// dst when there is one), what plan(msg) refuses, ensure_ready(dst), ensure_ready(src).  Every error is dst's
template <typename PlanFn>
int pair_enter(mrh_ctx* dst, mrh_ctx* src, const char* who, PlanFn&& plan) {
  if (!dst || !src) return dst ? fail(dst, MRH_ERR_INVALID_ARG, "%s: null argument", who) : MRH_ERR_INVALID_ARG;
  char msg[mrh_plan::kMsgBytes];
  if (const int rc = plan(msg)) return fail(dst, rc, "%s", msg);
  if (const int rc = ensure_ready(dst, who)) return rc;
  return source_rc(dst, src, who, ensure_ready(src, who));
}

// Exclusive scan of in[0, n), n >= 1, into pos (tile sums in `sums`: one word per kChainTile entries), and its total
// pos[n - 1] + in[n - 1].  One synchronisation: whatever the caller launched before it has finished too (blocks)
int scan_total(mrh_ctx* c, const u64* in, const u32 n, u64* sums, u64* pos, uint64_t* total) {
  hipStream_t s = c->stream;
  const u32 tiles = (n + kChainTile - 1) / kChainTile;
  k_tile_sums_u64<<<tiles, 1024, 0, s>>>(in, n, sums);
  k_tile_scan_u64<<<tiles, 1024, 0, s>>>(in, n, sums, pos);
  u64 last[2] = {0, 0};  // the position and the input word of the last entry
  HIP_TRY(c, hipMemcpyAsync(&last[0], pos + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(&last[1], in + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  *total = last[0] + last[1];
  return MRH_OK;
}

// One result plane of a blocking reader: where it lies in the pinned result, its size, where the kernels leave it, and whether
// the caller takes it
struct Plane {
  size_t off, bytes;
  void* dev;
  bool wanted;
  const void* host = nullptr;                               // read_planes: what the caller is handed (nullptr: not wanted)
  void* device() const { return wanted ? dev : nullptr; }   // what the launch is handed
};
// the wanted planes into the pinned result `h`, one synchronisation (blocks)
template <size_t N>
int read_planes(mrh_ctx* c, char* h, Plane (&planes)[N]) {
  for (Plane& p : planes)
    if (p.wanted) HIP_TRY(c, hipMemcpyAsync(h + p.off, p.dev, p.bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (Plane& p : planes) p.host = p.wanted ? h + p.off : nullptr;
  return MRH_OK;
}

// ---- raycasting (include/mrhash_raycast.h) -----------------------------------------------------------------------------------

// the four images, device pointers (nullptr = not wanted); `points` exists for the spherical model only
struct RayOut {
  float* depth; float* normals; uint8_t* rgb; float* points;
};

int raycast_enter(mrh_ctx* c, const char* who, const int model, const mrh_raycast_params* p, const float* R, const float* t, RayCam* rc) {
  return reader_enter(c, who, [&](char* msg) { return mrh_plan::raycast(msg, who, model, p, R, t, c->p.sdf_truncation, c->pending, c->map.shard_count, rc); });
}

int launch_raycast(mrh_ctx* c, const int model, const RayCam& rc, const RayOut& o) {
  const dim3 grid((unsigned) ((rc.cols + kRenderTile - 1) / kRenderTile), (unsigned) ((rc.rows + kRenderTile - 1) / kRenderTile));
  if (model == MRH_CAMERA_SPHERICAL) k_raycast<true><<<grid, kRenderTile * kRenderTile, 0, c->stream>>>(c->map, c->tab, rc, o.depth, o.normals, o.rgb, o.points);
  else k_raycast<false><<<grid, kRenderTile * kRenderTile, 0, c->stream>>>(c->map, c->tab, rc, o.depth, o.normals, o.rgb, nullptr);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// mrh_raycast / mrh_raycast_spherical: the render into the context's own images and their pinned copy (blocks)
int raycast_host(mrh_ctx* c, const char* who, const int model, const mrh_raycast_params* p, const float* R, const float* t, const float** out_depth,
                 const float** out_normals, const uint8_t** out_rgb, const float** out_points) {
  RayCam rc;
  int e = raycast_enter(c, who, model, p, R, t, &rc);
  if (e) return e;
  mrh_ctx::Ray& r = c->ray;
  // per pixel [depth f32 | normals 3 x f32 | points 3 x f32 | rgb 3 x u8], each image contiguous, on the device as in the pinned copy
  const size_t npix = (size_t) rc.rows * (size_t) rc.cols, f = sizeof(float), bytes = npix * (7 * f + 3);
  if ((e = regrow(c, r.d_img, r.cap, npix, bytes, false))) return e;  // the previous raycast has finished (it blocked): nothing reads the old buffers
  if ((e = regrow_pinned(c, r.h_img, r.h_cap, npix, bytes))) return e;
  auto image = [&](const size_t off, const size_t size, const bool wanted) { return Plane{off, size, r.d_img + off, wanted}; };
  enum { DEPTH, NORMALS, RGB, POINTS };
  Plane im[4] = {image(0, npix * f, out_depth != nullptr), image(npix * f, npix * 3 * f, out_normals && (p->outputs & MRH_RAYCAST_NORMALS)),
                 image(npix * 7 * f, npix * 3, out_rgb && (p->outputs & MRH_RAYCAST_COLORS)),
                 image(npix * 4 * f, npix * 3 * f, out_points && (p->outputs & MRH_RAYCAST_POINTS))};
  if ((e = launch_raycast(c, model, rc, RayOut{(float*) im[DEPTH].device(), (float*) im[NORMALS].device(), (uint8_t*) im[RGB].device(), (float*) im[POINTS].device()})))
    return e;
  if ((e = read_planes(c, r.h_img, im))) return e;
  if (out_depth) *out_depth = (const float*) im[DEPTH].host;
  if (out_normals) *out_normals = (const float*) im[NORMALS].host;
  if (out_rgb) *out_rgb = (const uint8_t*) im[RGB].host;
  if (out_points) *out_points = (const float*) im[POINTS].host;
  return MRH_OK;
}

// mrh_raycast_device / mrh_raycast_spherical_device: the render into the caller's device buffers (enqueues)
int raycast_device(mrh_ctx* c, const char* who, const int model, const mrh_raycast_params* p, const float* R, const float* t, const RayOut& o) {
  RayCam rc;
  const int e = raycast_enter(c, who, model, p, R, t, &rc);
  if (e) return e;
  return launch_raycast(c, model, rc, RayOut{o.depth, (p->outputs & MRH_RAYCAST_NORMALS) ? o.normals : nullptr, (p->outputs & MRH_RAYCAST_COLORS) ? o.rgb : nullptr,
                                             (p->outputs & MRH_RAYCAST_POINTS) ? o.points : nullptr});
}

// ---- distance fields (include/mrhash_esdf.h) -----------------------------------------------------------------------------------

// have_dist: mrh_esdf_device was given its one required output (mrh_esdf has none: true)
int esdf_enter(mrh_ctx* c, const char* who, const mrh_esdf_params* p, const bool have_dist, EsdfBox* bx) {
  return reader_enter(c, who, [&](char* msg) {
    const int e = mrh_plan::esdf(msg, who, p, c->map.min_weight_threshold, c->pending, c->map.shard_count, bx);
    return e || have_dist ? e : mrh_plan::refuse(msg, MRH_ERR_INVALID_ARG, "%s: d_dist is null", who);
  });
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

// ---- tracking (include/mrhash_track.h) -----------------------------------------------------------------------------------------

// what is tracked: a pinhole depth image of the model's rows x cols (D14) or a cloud of n sensor-frame points against the
// spherical render (D15); on the host (staged through pinned memory) or on the device
struct TrackObs {
  int model;  // MRH_CAMERA_*: the camera model of the model render, and with it the linearisation
  const float* host; const float* dev;
  size_t n;   // points (spherical); a depth image has rows * cols pixels
};

// Host input of n floats — a depth image, a cloud or query points — through the context's one staging pair onto the device
// (mrh_ctx::Stage: every user blocks before it returns, so the pair is free when the next one fills it)
int stage_obs(mrh_ctx* c, const float* host, const size_t n, const float** d_obs) {
  mrh_ctx::Stage& S = c->stage;
  int e = regrow_pinned(c, S.h, S.h_cap, n, n * sizeof(float));
  if (!e) e = regrow(c, S.d, S.d_cap, n, n * sizeof(float), false);
  if (e) return e;
  memcpy(S.h, host, n * sizeof(float));
  HIP_TRY(c, hipMemcpyAsync(S.d, S.h, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  *d_obs = S.d;
  return MRH_OK;
}

static_assert(MRH_TRACK_OK == mrh_track::kFitOk && MRH_TRACK_LOST == mrh_track::kFitLost && MRH_ALIGN_OK == mrh_track::kFitOk &&
              MRH_ALIGN_LOST == mrh_track::kFitLost, "one pair of status values serves tracking and registration (mrh_track::fit_run)");
// What both fits' callables end in, one linearisation into the 32 sums: launch(slab) starts the kernel whose n_rows workgroups write
// one row of the context's partial slab each (grown without a drain: its last user blocked), k_track_finish adds the rows into
// pinned memory, the host reads the 256 bytes.  Blocks
template <typename Launch>
int linearise_sums(mrh_ctx* c, const size_t n_rows, Launch&& launch, int64_t sums[mrh_track::kSumWords]) {
  mrh_ctx::Fit& F = c->fit;
  if (const int e = regrow(c, F.d_slab, F.slab_cap, n_rows, n_rows * mrh_track::kSumWords * sizeof(i64), false)) return e;
  if (!F.h_sums) HIP_TRY(c, pinned_alloc(c, F.h_sums, mrh_track::kSumWords * sizeof(i64)));
  launch(F.d_slab);
  k_track_finish<<<1, 1024, 0, c->stream>>>(F.d_slab, (int) n_rows, F.h_sums);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the last launch wrote the sums into pinned memory
  for (int i = 0; i < mrh_track::kSumWords; i++) sums[i] = (int64_t) ((volatile long long*) F.h_sums)[i];
  return MRH_OK;
}
static_assert(((uint64_t) MRH_ALIGN_MAX_SAMPLES + kAlignLanes - 1) / kAlignLanes <= 0x7FFFFFFFull, "the slab's rows fit k_track_finish's int");

// mrh_track_depth / mrh_track_scan and their device variants, a driver over the stages: plan (mrh_readerplan.h), buffers, the
// observation onto the device, one render of the model through the raycast's own launch, the loop with the linearisation kernel
// of the camera model as its callable, the report (blocks)
int track_run(mrh_ctx* c, const char* who, const mrh_track_params* p, const TrackObs& obs, const float* R0, const float* t0, float* out_R, float* out_t,
              mrh_track_info* out_info) {
  mrh_plan::Track plan;
  int e = reader_enter(c, who, [&](char* msg) {
    return mrh_plan::track(msg, who, obs.model, p, obs.host || obs.dev, obs.n, out_R && out_t, R0, t0, c->p.sdf_truncation, c->pending, c->map.shard_count, &plan);
  });
  if (e) return e;
  const RayCam& rc = plan.cam;
  const bool scan = obs.model == MRH_CAMERA_SPHERICAL;
  const size_t npix = (size_t) rc.rows * (size_t) rc.cols, n_obs = scan ? obs.n : npix;  // the model's pixels, the lanes of a linearisation
  const dim3 grid = scan ? dim3((unsigned) ((n_obs + 255) / 256))
                         : dim3((unsigned) ((rc.cols + kRenderTile - 1) / kRenderTile), (unsigned) ((rc.rows + kRenderTile - 1) / kRenderTile));
  const size_t n_rows = (size_t) grid.x * grid.y;  // its workgroups: one row of the partial slab each
  mrh_track::Fit f(R0, t0);  // an empty scan is lost: nothing is rendered or launched
  if (n_obs) {
    mrh_ctx::Track& T = c->trk;  // the previous call blocked: nothing reads the old buffers
    if ((e = regrow(c, T.d_img, T.cap, npix, npix * 4 * sizeof(float), false))) return e;
    if (scan && (e = regrow(c, T.d_mp, T.mp_cap, npix, npix * 3 * sizeof(float), false))) return e;
    float *d_md = (float*) T.d_img, *d_mn = d_md + npix;  // the model's depth (range), then its normals
    const float* d_obs = obs.dev;
    if (!d_obs && (e = stage_obs(c, obs.host, scan ? 3 * n_obs : npix, &d_obs))) return e;
    if ((e = launch_raycast(c, obs.model, rc, RayOut{d_md, d_mn, nullptr, scan ? T.d_mp : nullptr}))) return e;
    TrackLin k;
    k.fx = p->fx; k.fy = p->fy; k.cx = p->cx; k.cy = p->cy; k.ifx = rc.ifx; k.ify = rc.ify;
    k.rows = rc.rows; k.cols = rc.cols; k.min_depth = rc.min_depth; k.max_depth = rc.max_depth;
    k.dmax2 = plan.dist_max * plan.dist_max; k.s_a = mrh_track::angle_scale(rc.max_depth);
    for (int i = 0; i < 9; i++) k.Rr[i] = R0[i];
    for (int i = 0; i < 3; i++) k.tr[i] = t0[i];
    e = mrh_track::fit_run(f, plan.iterations, k.s_a, plan.min_pixels, [&](const float* R, const float* t, int64_t* sums) {
      for (int i = 0; i < 9; i++) k.R[i] = R[i];
      for (int i = 0; i < 3; i++) k.t[i] = t[i];
      return linearise_sums(c, n_rows, [&](i64* slab) {
        if (scan) k_track_scan_linearise<<<grid, 256, 0, c->stream>>>(k, d_obs, (unsigned) n_obs, d_md, d_mn, T.d_mp, slab);
        else k_track_linearise<<<grid, kRenderTile * kRenderTile, 0, c->stream>>>(k, d_obs, d_md, d_mn, slab);
      }, sums);
    });
    if (e < 0) return e;
  }
  mrh_track::fit_report(f, out_R, out_t, out_info, &mrh_track_info::pixels);
  return MRH_OK;
}

// mrh_track_depth_sdf / mrh_track_points_sdf and their device variants (include/mrhash_sdftrack.h, D20), beside track_run: plan,
// the observation onto the device, the loop with the linearisation kernel of the form as its callable, the report (blocks).  No
// render and no model buffers: the slab and the pinned sums are the context's (mrh_ctx::fit), the staging pair mrh_ctx::stage.
// depth_form: host / dev is a depth image of the plan's rows x cols, else a cloud of n points
int sdftrack_run(mrh_ctx* c, const char* who, const bool depth_form, const mrh_sdftrack_params* p, const float* host, const float* dev, const size_t n,
                 const float* R0, const float* t0, float* out_R, float* out_t, mrh_track_info* out_info) {
  mrh_plan::Sdftrack plan;
  int e = reader_enter(c, who, [&](char* msg) {
    return mrh_plan::sdftrack(msg, who, depth_form, p, host || dev, n, out_R && out_t, R0, t0, c->p.sdf_truncation, c->pending, c->map.shard_count, &plan);
  });
  if (e) return e;
  const size_t n_obs = depth_form ? (size_t) plan.rows * (size_t) plan.cols : n;  // the lanes of a linearisation
  const dim3 grid = depth_form ? dim3((unsigned) ((plan.cols + kRenderTile - 1) / kRenderTile), (unsigned) ((plan.rows + kRenderTile - 1) / kRenderTile))
                               : dim3((unsigned) ((n_obs + kSdfTrackLanes - 1) / kSdfTrackLanes));
  const size_t n_rows = (size_t) grid.x * grid.y;  // its workgroups: one row of the partial slab each
  mrh_track::Fit f(R0, t0);  // an empty cloud is lost: nothing is launched
  if (n_obs) {
    const float* d_obs = dev;
    if (!d_obs && (e = stage_obs(c, host, depth_form ? n_obs : 3 * n_obs, &d_obs))) return e;
    SdfTrackLin k;
    k.ifx = plan.ifx; k.ify = plan.ify; k.cx = plan.cx; k.cy = plan.cy;
    k.rows = plan.rows; k.cols = plan.cols; k.n = depth_form ? 0u : (uint32_t) n_obs;
    k.min_depth = plan.min_depth; k.max_depth = plan.max_depth; k.band = plan.band;
    k.s_a = mrh_track::angle_scale(plan.max_depth);
    k.bound = (float) (1 << 20) * c->map.vs;
    e = mrh_track::fit_run(f, plan.iterations, k.s_a, plan.min_pixels, [&](const float* R, const float* t, int64_t* sums) {
      for (int i = 0; i < 9; i++) k.R[i] = R[i];
      for (int i = 0; i < 3; i++) k.t[i] = t[i];
      return linearise_sums(c, n_rows, [&](i64* slab) {
        if (depth_form) k_sdftrack_depth_linearise<<<grid, kSdfTrackLanes, 0, c->stream>>>(c->map, c->tab, k, d_obs, slab);
        else k_sdftrack_points_linearise<<<grid, kSdfTrackLanes, 0, c->stream>>>(c->map, c->tab, k, d_obs, slab);
      }, sums);
    });
    if (e < 0) return e;
  }
  mrh_track::fit_report(f, out_R, out_t, out_info, &mrh_track_info::pixels);
  return MRH_OK;
}
static_assert(kSdfTrackLanes == kRenderTile * kRenderTile, "the depth form's tile is one workgroup of track_reduce_store");
static_assert((size_t) MRH_RAYCAST_MAX_SIDE * MRH_RAYCAST_MAX_SIDE <= (size_t) MRH_SDFTRACK_MAX_POINTS, "an image has no more samples than a cloud may: the sums' bounds");

// ---- point queries (include/mrhash_query.h) ------------------------------------------------------------------------------------

// the four outputs, device pointers (dist and state always; grad / rgbw nullptr = not produced)
struct QueryOut {
  float* dist; float* grad; uint8_t* rgbw; uint8_t* state;
};

// have_points / have_out: the point list and the required outputs were given (mrh_plan::query)
int query_enter(mrh_ctx* c, const char* who, const mrh_query_params* p, const bool have_points, const bool have_out, const uint64_t n, const float* R,
                const float* t, QueryArgs* q) {
  return reader_enter(c, who, [&](char* msg) { return mrh_plan::query(msg, who, p, have_points, have_out, n, R, t, c->p.virtual_voxel_size, c->pending, c->map.shard_count, q); });
}

// one launch for q.n >= 1 points; o.grad / o.rgbw are already nullptr where they are not wanted
int launch_query(mrh_ctx* c, const QueryArgs& q, const float* d_xyz, const QueryOut& o) {
  const unsigned grid = (unsigned) (((size_t) q.n + kQueryLanes - 1) / kQueryLanes);
  if (q.smooth && q.posed) k_query<true, true><<<grid, kQueryLanes, 0, c->stream>>>(c->map, c->tab, q, d_xyz, o.dist, o.grad, o.rgbw, o.state);
  else if (q.smooth) k_query<true, false><<<grid, kQueryLanes, 0, c->stream>>>(c->map, c->tab, q, d_xyz, o.dist, o.grad, o.rgbw, o.state);
  else if (q.posed) k_query<false, true><<<grid, kQueryLanes, 0, c->stream>>>(c->map, c->tab, q, d_xyz, o.dist, o.grad, o.rgbw, o.state);
  else k_query<false, false><<<grid, kQueryLanes, 0, c->stream>>>(c->map, c->tab, q, d_xyz, o.dist, o.grad, o.rgbw, o.state);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
static_assert((size_t) kQueryLanes * kQuerySlice * sizeof(u32) <= 65536, "the lane-private slices fit the static LDS limit");

// ---- ray queries (include/mrhash_rays.h) ---------------------------------------------------------------------------------------

// the rays of one call, device pointers (tmax nullptr: every ray ends at max_range)
struct RaysIn {
  const float* origins; const float* dirs; const float* tmax;
};
// the six outputs, device pointers (range and status always; the others nullptr = not produced)
struct RaysOut {
  float* range; uint8_t* status; float* normals; uint8_t* rgb; u32* counts; float* first_unknown;
};

// have_rays / have_out: origins and directions, and the required outputs, were given (mrh_plan::rays)
int rays_enter(mrh_ctx* c, const char* who, const mrh_rays_params* p, const bool have_rays, const bool have_out, const uint64_t n, const float* R, const float* t,
               RaysArgs* a) {
  return reader_enter(c, who, [&](char* msg) {
    return mrh_plan::rays(msg, who, p, have_rays, have_out, n, R, t, c->p.sdf_truncation, c->p.virtual_voxel_size, c->pending, c->map.shard_count, a);
  });
}

// one launch for a.n >= 1 rays; the optional outputs are already nullptr where they are not wanted
int launch_rays(mrh_ctx* c, const RaysArgs& a, const RaysIn& in, const RaysOut& o) {
  const unsigned grid = (unsigned) (((size_t) a.n + kRaysLanes - 1) / kRaysLanes);
  k_cast_rays<<<grid, kRaysLanes, 0, c->stream>>>(c->map, c->tab, a, in.origins, in.dirs, in.tmax, o.range, o.status, o.normals, o.rgb, o.counts, o.first_unknown);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// Host rays through the context's one staging pair (stage_obs's, see mrh_ctx::Stage): [origins 3n | directions 3n | tmax n] floats
int stage_rays(mrh_ctx* c, const float* origins, const float* dirs, const float* tmax, const size_t n, RaysIn* in) {
  mrh_ctx::Stage& S = c->stage;
  const size_t floats = (tmax ? 7 : 6) * n;
  int e = regrow_pinned(c, S.h, S.h_cap, floats, floats * sizeof(float));
  if (!e) e = regrow(c, S.d, S.d_cap, floats, floats * sizeof(float), false);
  if (e) return e;
  memcpy(S.h, origins, 3 * n * sizeof(float));
  memcpy(S.h + 3 * n, dirs, 3 * n * sizeof(float));
  if (tmax) memcpy(S.h + 6 * n, tmax, n * sizeof(float));
  HIP_TRY(c, hipMemcpyAsync(S.d, S.h, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
  *in = RaysIn{S.d, S.d + 3 * n, tmax ? S.d + 6 * n : nullptr};
  return MRH_OK;
}

// ---- the free-space layer (include/mrhash_freespace.h) -------------------------------------------------------------------------

// The way in of the calls that neither read nor change the map — create, clear, destroy, the carves, the segments: a null context,
// what plan(msg) refuses, the device.  No ensure_ready: a frame mrh_integrate kept back stays kept back and pipelined frames stay
// in flight (D22).  That is safe because these calls touch mrh_ctx::free and mrh_ctx::stage alone, which the frame path never
// does, and enqueue on the context's stream, where they are ordered with the readers of the layer
template <typename PlanFn>
int free_enter(mrh_ctx* c, const char* who, PlanFn&& plan) {
  if (!c) return MRH_ERR_INVALID_ARG;
  char msg[mrh_plan::kMsgBytes];
  const int rc = plan(msg);
  return rc ? fail(c, rc, "%s", msg) : ensure_device(c, who);
}

int free_layer_enter(mrh_ctx* c, const char* who) {
  return free_enter(c, who, [&](char* msg) { return mrh_plan::freespace_layer(msg, who, c->free.on, c->pending, c->map.shard_count); });
}

// the four carves: plan, host input through the staging pair, one launch; the host forms block
int carve_run(mrh_ctx* c, const char* who, const bool depth_form, const mrh_carve_params* p, const float* host, const float* dev, const uint64_t n, const float* R,
              const float* t) {
  CarveArgs a;
  int rc = free_enter(c, who, [&](char* msg) {
    return mrh_plan::freespace_carve(msg, who, depth_form, p, host || dev, n, R, t, c->free.on, c->map.vs, c->free.L.shift, c->pending, c->map.shard_count, &a);
  });
  if (rc) return rc;
  const size_t n_obs = depth_form ? (size_t) a.cam.rows * (size_t) a.cam.cols : (size_t) n;
  if (n_obs == 0) return MRH_OK;
  const mrh_ctx::Free& F = c->free;
  const float* d_obs = dev;
  if (!d_obs && (rc = stage_obs(c, host, depth_form ? n_obs : 3 * n_obs, &d_obs))) return rc;
  if (depth_form) {
    const dim3 grid((unsigned) ((a.cam.cols + kRenderTile - 1) / kRenderTile), (unsigned) ((a.cam.rows + kRenderTile - 1) / kRenderTile));
    k_freespace_carve<true><<<grid, kFreeLanes, 0, c->stream>>>(c->map.vs, F.L, F.d_words, a, d_obs);
  } else {
    k_freespace_carve<false><<<(unsigned) ((n_obs + kFreeLanes - 1) / kFreeLanes), kFreeLanes, 0, c->stream>>>(c->map.vs, F.L, F.d_words, a, d_obs);
  }
  HIP_TRY(c, hipGetLastError());
  if (!dev) HIP_TRY(c, hipStreamSynchronize(c->stream));  // the staging pair is free again
  return MRH_OK;
}
static_assert(kFreeLanes == kRenderTile * kRenderTile, "the depth form's workgroup is one 16 x 16 tile");

// have_out: the required output was given (mrh_freespace_box hands out its own: true).  Reads the map: enters like every reader
int freebox_enter(mrh_ctx* c, const char* who, const mrh_freespace_box_params* p, const bool have_out, FreeBox* bx) {
  return reader_enter(c, who, [&](char* msg) {
    return mrh_plan::freespace_box(msg, who, p, have_out, c->free.on, c->free.L.shift, c->map.min_weight_threshold, c->pending, c->map.shard_count, bx);
  });
}

// the two launches: the classified bytes into the context's scratch, the finished bytes into `out`
int launch_freebox(mrh_ctx* c, const FreeBox& bx, uint8_t* out) {
  mrh_ctx::Free& F = c->free;
  const size_t n = (size_t) bx.nx * (size_t) bx.ny * (size_t) bx.nz;
  if (const int rc = regrow(c, F.d_cls, F.cls_cap, n, n)) return rc;  // an earlier mrh_freespace_box_device may still read the old scratch: the stream drains
  const auto bricks = [](const int o, const int len) { return (unsigned) (((o + len - 1) >> 3) - (o >> 3) + 1); };
  const EsdfBox& v = bx.vox;
  k_freespace_classify<<<dim3(bricks(v.ox, v.nx), bricks(v.oy, v.ny), bricks(v.oz, v.nz)), 256, 0, c->stream>>>(c->map, c->tab, F.L, F.d_words, bx, F.d_cls);
  k_freespace_frontier<<<(unsigned) ((n + kFreeLanes - 1) / kFreeLanes), kFreeLanes, 0, c->stream>>>(bx, F.d_cls, out);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
static_assert(MRH_FREESPACE_BOX_MAX_SIDE + 1 <= 65535, "the bricks of a box (at most one per cell, plus one) fit a grid dimension");

int segments_enter(mrh_ctx* c, const char* who, const bool have_in, const bool have_out, const uint64_t n, const float step, SegArgs* a) {
  return free_enter(c, who, [&](char* msg) {
    return mrh_plan::freespace_segments(msg, who, have_in, have_out, n, step, c->free.on, c->map.vs, c->free.L.shift, c->pending, c->map.shard_count, a);
  });
}

// one launch for a.n >= 1 segments; counts may be nullptr
int launch_segments(mrh_ctx* c, const SegArgs& a, const float* d_a, const float* d_b, uint8_t* status, u32* counts) {
  const mrh_ctx::Free& F = c->free;
  k_freespace_segments<<<(unsigned) (((size_t) a.n + kFreeLanes - 1) / kFreeLanes), kFreeLanes, 0, c->stream>>>(c->map.vs, F.L, F.d_words, a, d_a, d_b, status, counts);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// ---- map-to-map fusion (include/mrhash_remap.h) --------------------------------------------------------------------------------

// the argument plan of both calls (mrh_plan::remap); dst: the destination of mrh_fuse_map, nullptr for mrh_resample_map
int remap_plan(char* msg, const char* who, mrh_ctx* src, mrh_ctx* dst, const mrh_remap_params* p, const float* R, const float* t, const bool have_out, RemapArgs* a) {
  const bool fuse = dst != nullptr;
  return mrh_plan::remap(msg, who, p, R, t, have_out, src->p.virtual_voxel_size, src->pending, src->map.shard_count, fuse, dst == src,
                         fuse && dst->device == src->device, fuse ? dst->p.virtual_voxel_size : 0.f, fuse ? dst->pending : 0, fuse ? dst->map.shard_count : 1, a);
}

// exclusive scan of marks[0, n) into R.d_pos, *count = how many are marked (blocks); the marked keys of `keys` in order to `out` (enqueued)
int remap_keep_marked(mrh_ctx* c, const u64* keys, const u32 n, u64* out, uint64_t* count) {
  mrh_ctx::Remap& R = c->remap;
  if (const int rc = scan_total(c, R.d_marks, n, R.d_sums, R.d_pos, count)) return rc;
  k_remap_compact<<<(n + 255) / 256, 256, 0, c->stream>>>(keys, R.d_marks, R.d_pos, n, out);  // behind the read-back: what follows on the stream reads `out`
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// The resampling behind ensure_ready(src): candidates, sort, distinct keys, flags, kept keys, sample; the records in
// src->remap.d_rec.  Blocks.  The live blocks come from borrow_live_blocks (mrh_blocks.h).  info->taken is left alone
int remap_run(mrh_ctx* c, const char* who, const RemapArgs& a, const mrh_block_record** out_records, uint64_t* out_n, mrh_remap_info* info) {
  mrh_ctx::Remap& R = c->remap;
  hipStream_t s = c->stream;
  *out_records = nullptr;
  *out_n = 0;
  info->source_blocks = info->candidate_blocks = info->records = info->valid_voxels = 0;
  if (!R.d_count) HIP_TRY(c, dev_alloc(c, R.d_count, sizeof(u64)));
  HIP_TRY(c, hipMemsetAsync(R.d_count, 0, sizeof(u64), s));
  int n_src = 0, rc = borrow_live_blocks(c, &n_src);
  if (rc) return rc;
  info->source_blocks = (uint64_t) n_src;
  if (n_src == 0) return MRH_OK;
  char msg[mrh_plan::kMsgBytes];
  uint64_t slots = 0;
  if ((rc = mrh_plan::remap_slots(msg, who, (uint64_t) n_src, a.per_axis, &slots))) return fail(c, rc, "%s", msg);
  const size_t n = (size_t) slots;
  if (n > R.cap) {  // the previous call blocked: nothing reads the old buffers
    const size_t cap = n + n / 4, st = (cap + kSortTile - 1) / kSortTile, ct = (cap + kChainTile - 1) / kChainTile;
    if ((rc = regrow_all(c, R.cap, cap, {{R.d_keys[0], cap * sizeof(u64)}, {R.d_keys[1], cap * sizeof(u64)}, {R.d_vals[0], cap * sizeof(u32)}, {R.d_vals[1], cap * sizeof(u32)},
                                         {R.d_marks, cap * sizeof(u64)}, {R.d_pos, cap * sizeof(u64)}, {R.d_sums, ct * sizeof(u64)}, {R.d_sort, (256 + 256 * st) * sizeof(u32)}}, false)))
      return rc;
    HIP_TRY(c, hipMemsetAsync(R.d_vals[0], 0, cap * sizeof(u32), s));  // the sort carries values along; nothing reads them
  }
  k_remap_candidates<<<((u32) n_src + 255) / 256, 256, 0, s>>>(c->map, c->tab, a, (u32) n_src, R.d_keys[0]);
  const int at = radix_sort_pairs<u64, u32>(s, R.d_keys, R.d_vals, nullptr, n, 64, R.d_sort, R.d_sort + 256);  // kKeyEmpty uses every bit
  k_remap_mark_first<<<((u32) n + 255) / 256, 256, 0, s>>>(R.d_keys[at], (u32) n, R.d_marks);
  uint64_t n_cand = 0, n_rec = 0;
  if ((rc = remap_keep_marked(c, R.d_keys[at], (u32) n, R.d_keys[at ^ 1], &n_cand))) return rc;
  info->candidate_blocks = n_cand;
  if (n_cand == 0) return MRH_OK;
  const u64* cand = R.d_keys[at ^ 1];
  k_remap_flags<<<(unsigned) std::min<uint64_t>(n_cand, 8192), kRemapLanes, 0, s>>>(c->map, c->tab, a, cand, (u32) n_cand, R.d_marks, R.d_count);
  if ((rc = remap_keep_marked(c, cand, (u32) n_cand, R.d_keys[at], &n_rec))) return rc;
  u64 valid = 0;
  HIP_TRY(c, hipMemcpyAsync(&valid, R.d_count, sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  info->records = n_rec;
  info->valid_voxels = valid;
  if (n_rec == 0) return MRH_OK;
  uint64_t bytes = 0;
  if ((rc = mrh_plan::remap_record_bytes(msg, who, n_rec, &bytes))) return fail(c, rc, "%s", msg);
  const size_t room = (size_t) (bytes + bytes / 4);  // the previous call blocked: nothing reads the old buffer
  if (bytes > R.rec_cap && (rc = regrow(c, R.d_rec, R.rec_cap, room, room, false))) return rc;
  k_remap_sample<<<(unsigned) std::min<uint64_t>(n_rec, 8192), kRemapLanes, 0, s>>>(c->map, c->tab, a, R.d_keys[at], (u32) n_rec, R.d_rec);
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  *out_records = (const mrh_block_record*) R.d_rec;
  *out_n = n_rec;
  return MRH_OK;
}

// ---- map-to-map registration (include/mrhash_align.h) ----------------------------------------------------------------------------

// The source half behind ensure_ready(src): the live blocks (borrow_live_blocks, mrh_blocks.h), count, box, scan, emit; the
// samples in src->align.d_samples.  Fills the automatic pivot and extent into `plan`.  Blocks: src's stream is drained when it
// returns.  Errors are reported on src
int align_gather(mrh_ctx* c, const char* who, mrh_plan::Align& plan, uint64_t* n_blocks, uint64_t* n_samples) {
  mrh_ctx::Align& A = c->align;
  hipStream_t s = c->stream;
  *n_blocks = *n_samples = 0;
  if (!A.h_box) HIP_TRY(c, pinned_alloc(c, A.h_box, 2 * sizeof(int4)));
  int n_src = 0, rc = borrow_live_blocks(c, &n_src);
  if (rc) return rc;
  *n_blocks = (uint64_t) n_src;
  if (n_src == 0) return MRH_OK;
  const u32 n = (u32) n_src, grid = std::min<u32>(n, 8192u);
  if ((size_t) n > A.cap) {  // the previous call blocked: nothing reads the old buffers
    const size_t cap = (size_t) n + n / 4, ct = (cap + kChainTile - 1) / kChainTile;
    if ((rc = regrow_all(c, A.cap, cap, {{A.d_counts, cap * sizeof(u64)}, {A.d_pos, cap * sizeof(u64)}, {A.d_sums, ct * sizeof(u64)}, {A.d_boxes, cap * 2 * sizeof(int4)}}, false)))
      return rc;
  }
  AlignGather g;
  g.vs_s = c->map.vs; g.band = plan.band; g.w_min = plan.w_min; g.crop = plan.crop; g.extent = plan.extent;
  for (int i = 0; i < 3; i++) g.c[i] = plan.pivot[i];
  k_align_gather<false><<<grid, kAlignGatherLanes, 0, s>>>(c->tab, g, n, A.d_counts, A.d_boxes, nullptr, nullptr, 0);
  k_align_box<<<1, 1024, 0, s>>>(A.d_boxes, n, A.h_box);  // into pinned memory: scan_total's synchronisation covers it
  uint64_t total = 0;
  if ((rc = scan_total(c, A.d_counts, n, A.d_sums, A.d_pos, &total))) return rc;
  char msg[mrh_plan::kMsgBytes];
  uint64_t bytes = 0;
  if ((rc = mrh_plan::align_sample_bytes(msg, who, total, &bytes))) return fail(c, rc, "%s", msg);
  *n_samples = total;
  if (total == 0) return MRH_OK;
  if (!plan.crop) {
    const volatile int4* hb = A.h_box;
    const int lo[3] = {hb[0].x, hb[0].y, hb[0].z}, hi[3] = {hb[1].x, hb[1].y, hb[1].z};
    mrh_plan::align_auto_pivot(lo, hi, c->map.vs, plan.pivot, &plan.extent);
  }
  const size_t room = (size_t) (total + total / 4);  // the previous call blocked: nothing reads the old buffer
  if ((size_t) total > A.smp_cap && (rc = regrow(c, A.d_samples, A.smp_cap, room, room * sizeof(float4), false))) return rc;
  k_align_gather<true><<<grid, kAlignGatherLanes, 0, s>>>(c->tab, g, n, nullptr, nullptr, A.d_pos, A.d_samples, (u64) total);
  HIP_TRY(c, hipStreamSynchronize(s));
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

int mrh_esdf(mrh_ctx* c, const mrh_esdf_params* p, const float** out_dist, const uint8_t** out_state, const uint32_t** out_d2) {
  EsdfBox bx;
  int rc = esdf_enter(c, "mrh_esdf", p, true, &bx);
  if (rc) return rc;
  const size_t n = (size_t) bx.nx * (size_t) bx.ny * (size_t) bx.nz;
  mrh_ctx::Esdf& e = c->esdf;
  // results per cell: device dist f32 and d2 u32; pinned [dist f32 | d2 u32 | state u8], each plane contiguous
  if (n > e.out_cap && (rc = regrow_all(c, e.out_cap, n, {{e.d_dist, n * sizeof(float)}, {e.d_d2, n * sizeof(u32)}}))) return rc;
  if ((rc = regrow_pinned(c, e.h_out, e.h_cap, n, n * 9))) return rc;
  if ((rc = esdf_scratch(c, n))) return rc;
  enum { DIST, D2, STATE };
  Plane pl[3] = {{0, n * sizeof(float), e.d_dist, out_dist != nullptr}, {n * 4, n * sizeof(u32), e.d_d2, out_d2 && (p->outputs & MRH_ESDF_SQUARED)},
                 {n * 8, n, e.d_state, out_state && (p->outputs & MRH_ESDF_STATE)}};
  if ((rc = launch_esdf(c, bx, e.d_dist, (uint8_t*) pl[STATE].device(), (u32*) pl[D2].device()))) return rc;
  if ((rc = read_planes(c, e.h_out, pl))) return rc;
  if (out_dist) *out_dist = (const float*) pl[DIST].host;
  if (out_state) *out_state = (const uint8_t*) pl[STATE].host;
  if (out_d2) *out_d2 = (const uint32_t*) pl[D2].host;
  return MRH_OK;
}

int mrh_esdf_device(mrh_ctx* c, const mrh_esdf_params* p, float* d_dist, uint8_t* d_state, uint32_t* d_d2) {
  EsdfBox bx;
  int rc = esdf_enter(c, "mrh_esdf_device", p, d_dist != nullptr, &bx);
  if (rc) return rc;
  if ((rc = esdf_scratch(c, (size_t) bx.nx * (size_t) bx.ny * (size_t) bx.nz))) return rc;
  return launch_esdf(c, bx, d_dist, (p->outputs & MRH_ESDF_STATE) ? d_state : nullptr, (p->outputs & MRH_ESDF_SQUARED) ? (u32*) d_d2 : nullptr);
}

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

int mrh_track_depth_sdf(mrh_ctx* c, const mrh_sdftrack_params* p, const float* depth_host, const float R_init[9], const float t_init[3], float out_R[9],
                        float out_t[3], mrh_track_info* out_info) {
  return sdftrack_run(c, "mrh_track_depth_sdf", true, p, depth_host, nullptr, 0, R_init, t_init, out_R, out_t, out_info);
}

int mrh_track_depth_sdf_device(mrh_ctx* c, const mrh_sdftrack_params* p, const float* d_depth, const float R_init[9], const float t_init[3], float out_R[9],
                               float out_t[3], mrh_track_info* out_info) {
  return sdftrack_run(c, "mrh_track_depth_sdf_device", true, p, nullptr, d_depth, 0, R_init, t_init, out_R, out_t, out_info);
}

int mrh_track_points_sdf(mrh_ctx* c, const mrh_sdftrack_params* p, const float* points_host, size_t n, const float R_init[9], const float t_init[3],
                         float out_R[9], float out_t[3], mrh_track_info* out_info) {
  return sdftrack_run(c, "mrh_track_points_sdf", false, p, points_host, nullptr, n, R_init, t_init, out_R, out_t, out_info);
}

int mrh_track_points_sdf_device(mrh_ctx* c, const mrh_sdftrack_params* p, const float* d_points, size_t n, const float R_init[9], const float t_init[3],
                                float out_R[9], float out_t[3], mrh_track_info* out_info) {
  return sdftrack_run(c, "mrh_track_points_sdf_device", false, p, nullptr, d_points, n, R_init, t_init, out_R, out_t, out_info);
}

int mrh_query_points(mrh_ctx* c, const mrh_query_params* p, const float* xyz_host, uint64_t n, const float R_row_major[9], const float t[3],
                     const float** out_dist, const float** out_grad, const uint8_t** out_rgbw, const uint8_t** out_state) {
  QueryArgs q;
  int rc = query_enter(c, "mrh_query_points", p, xyz_host != nullptr, true, n, R_row_major, t, &q);
  if (rc) return rc;
  if (out_dist) *out_dist = nullptr;
  if (out_grad) *out_grad = nullptr;
  if (out_rgbw) *out_rgbw = nullptr;
  if (out_state) *out_state = nullptr;
  if (n == 0) return MRH_OK;
  mrh_ctx::Query& Q = c->query;
  // per point [dist f32 | grad 3 x f32 | rgbw 4 x u8 | state u8], each plane contiguous, on the device as in the pinned copy
  const size_t np = (size_t) n, f = sizeof(float), bytes = np * (4 * f + 4 + 1);
  if ((rc = regrow(c, Q.d_out, Q.cap, np, bytes, false))) return rc;  // the previous mrh_query_points has finished (it blocked): nothing reads the old buffer
  if ((rc = regrow_pinned(c, Q.h_out, Q.h_cap, np, bytes))) return rc;
  const float* d_xyz = nullptr;
  if ((rc = stage_obs(c, xyz_host, 3 * np, &d_xyz))) return rc;
  auto plane = [&](const size_t off, const size_t size, const bool wanted) { return Plane{off, size, Q.d_out + off, wanted}; };
  enum { DIST, GRAD, RGBW, STATE };
  Plane pl[4] = {plane(0, np * f, out_dist != nullptr), plane(np * f, np * 3 * f, out_grad && (p->outputs & MRH_QUERY_GRADIENT)),
                 plane(np * 4 * f, np * 4, out_rgbw && (p->outputs & MRH_QUERY_COLOUR)), plane(np * 4 * f + np * 4, np, out_state != nullptr)};
  // dist and state are always computed, the gradient whenever its bit is set: a NULL out-pointer only saves the copy
  const QueryOut o = {(float*) pl[DIST].dev, (p->outputs & MRH_QUERY_GRADIENT) ? (float*) pl[GRAD].dev : nullptr, (uint8_t*) pl[RGBW].device(), (uint8_t*) pl[STATE].dev};
  if ((rc = launch_query(c, q, d_xyz, o))) return rc;
  if ((rc = read_planes(c, Q.h_out, pl))) return rc;
  if (out_dist) *out_dist = (const float*) pl[DIST].host;
  if (out_grad) *out_grad = (const float*) pl[GRAD].host;
  if (out_rgbw) *out_rgbw = (const uint8_t*) pl[RGBW].host;
  if (out_state) *out_state = (const uint8_t*) pl[STATE].host;
  return MRH_OK;
}

int mrh_query_points_device(mrh_ctx* c, const mrh_query_params* p, const float* d_xyz, uint64_t n, const float R_row_major[9], const float t[3],
                            float* d_dist, float* d_grad, uint8_t* d_rgbw, uint8_t* d_state) {
  QueryArgs q;
  const int rc = query_enter(c, "mrh_query_points_device", p, d_xyz != nullptr, d_dist && d_state, n, R_row_major, t, &q);
  if (rc || n == 0) return rc;
  return launch_query(c, q, d_xyz, QueryOut{d_dist, (p->outputs & MRH_QUERY_GRADIENT) ? d_grad : nullptr, (p->outputs & MRH_QUERY_COLOUR) ? d_rgbw : nullptr, d_state});
}

int mrh_cast_rays(mrh_ctx* c, const mrh_rays_params* p, const float* origins_host, const float* dirs_host, const float* tmax_host, uint64_t n,
                  const float R_row_major[9], const float t[3], const float** out_range, const uint8_t** out_status, const float** out_normals,
                  const uint8_t** out_rgb, const uint32_t** out_counts, const float** out_first_unknown) {
  RaysArgs a;
  int rc = rays_enter(c, "mrh_cast_rays", p, origins_host && dirs_host, true, n, R_row_major, t, &a);
  if (rc) return rc;
  if (out_range) *out_range = nullptr;
  if (out_status) *out_status = nullptr;
  if (out_normals) *out_normals = nullptr;
  if (out_rgb) *out_rgb = nullptr;
  if (out_counts) *out_counts = nullptr;
  if (out_first_unknown) *out_first_unknown = nullptr;
  if (n == 0) return MRH_OK;
  mrh_ctx::Rays& Y = c->rays;
  // per ray [range f32 | normals 3 x f32 | counts 2 x u32 | first_unknown f32 | rgb 3 x u8 | status u8], each plane contiguous, on the
  // device as in the pinned copy
  const size_t nr = (size_t) n, f = sizeof(float), bytes = nr * (7 * f + 3 + 1);
  if ((rc = regrow(c, Y.d_out, Y.cap, nr, bytes, false))) return rc;  // the previous mrh_cast_rays has finished (it blocked): nothing reads the old buffer
  if ((rc = regrow_pinned(c, Y.h_out, Y.h_cap, nr, bytes))) return rc;
  RaysIn in;
  if ((rc = stage_rays(c, origins_host, dirs_host, tmax_host, nr, &in))) return rc;
  auto plane = [&](const size_t off, const size_t size, const bool wanted) { return Plane{off, size, Y.d_out + off, wanted}; };
  const bool counts = (p->outputs & MRH_RAYS_COUNTS) != 0;
  enum { RANGE, NORMALS, COUNTS, FIRST, RGB, STATUS };
  Plane pl[6] = {plane(0, nr * f, out_range != nullptr), plane(nr * f, nr * 3 * f, out_normals && (p->outputs & MRH_RAYS_NORMALS)),
                 plane(nr * 4 * f, nr * 2 * f, out_counts && counts), plane(nr * 6 * f, nr * f, out_first_unknown && counts),
                 plane(nr * 7 * f, nr * 3, out_rgb && (p->outputs & MRH_RAYS_COLORS)), plane(nr * 7 * f + nr * 3, nr, out_status != nullptr)};
  // range and status are always computed: a NULL out-pointer only saves the copy
  const RaysOut o = {(float*) pl[RANGE].dev, (uint8_t*) pl[STATUS].dev, (float*) pl[NORMALS].device(), (uint8_t*) pl[RGB].device(), (u32*) pl[COUNTS].device(),
                     (float*) pl[FIRST].device()};
  if ((rc = launch_rays(c, a, in, o))) return rc;
  if ((rc = read_planes(c, Y.h_out, pl))) return rc;
  if (out_range) *out_range = (const float*) pl[RANGE].host;
  if (out_status) *out_status = (const uint8_t*) pl[STATUS].host;
  if (out_normals) *out_normals = (const float*) pl[NORMALS].host;
  if (out_rgb) *out_rgb = (const uint8_t*) pl[RGB].host;
  if (out_counts) *out_counts = (const uint32_t*) pl[COUNTS].host;
  if (out_first_unknown) *out_first_unknown = (const float*) pl[FIRST].host;
  return MRH_OK;
}

int mrh_cast_rays_device(mrh_ctx* c, const mrh_rays_params* p, const float* d_origins, const float* d_dirs, const float* d_tmax, uint64_t n,
                         const float R_row_major[9], const float t[3], float* d_range, uint8_t* d_status, float* d_normals, uint8_t* d_rgb,
                         uint32_t* d_counts, float* d_first_unknown) {
  RaysArgs a;
  const int rc = rays_enter(c, "mrh_cast_rays_device", p, d_origins && d_dirs, d_range && d_status, n, R_row_major, t, &a);
  if (rc || n == 0) return rc;
  const bool counts = (p->outputs & MRH_RAYS_COUNTS) != 0;
  return launch_rays(c, a, RaysIn{d_origins, d_dirs, d_tmax},
                     RaysOut{d_range, d_status, (p->outputs & MRH_RAYS_NORMALS) ? d_normals : nullptr, (p->outputs & MRH_RAYS_COLORS) ? d_rgb : nullptr,
                             counts ? (u32*) d_counts : nullptr, counts ? d_first_unknown : nullptr});
}

int mrh_freespace_create(mrh_ctx* c, const mrh_freespace_params* p) {
  const char* who = "mrh_freespace_create";
  FreeLayer L;
  int rc = free_enter(c, who, [&](char* msg) { return mrh_plan::freespace_create(msg, who, p, c->pending, c->map.shard_count, &L); });
  if (rc) return rc;
  mrh_ctx::Free& F = c->free;
  F.on = false;
  const size_t words = L.n_words;
  if ((rc = regrow(c, F.d_words, F.cap, words, words * sizeof(u32)))) return rc;  // a carve in flight writes the old words: the stream drains
  HIP_TRY(c, hipMemsetAsync(F.d_words, 0, words * sizeof(u32), c->stream));       // behind whatever still uses the old layer
  F.L = L;
  F.on = true;
  return MRH_OK;
}

int mrh_freespace_clear(mrh_ctx* c) {
  const int rc = free_layer_enter(c, "mrh_freespace_clear");
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(c->free.d_words, 0, (size_t) c->free.L.n_words * sizeof(u32), c->stream));
  return MRH_OK;
}

int mrh_freespace_destroy(mrh_ctx* c) {
  const int rc = free_layer_enter(c, "mrh_freespace_destroy");
  if (rc) return rc;
  mrh_ctx::Free& F = c->free;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // nothing uses the words any more
  F.on = false;
  F.cap = 0;
  HIP_TRY(c, dev_free(c, F.d_words));
  return MRH_OK;
}

int mrh_freespace_carve_depth(mrh_ctx* c, const mrh_carve_params* p, const float* depth_host, const float R_row_major[9], const float t[3]) {
  return carve_run(c, "mrh_freespace_carve_depth", true, p, depth_host, nullptr, 0, R_row_major, t);
}

int mrh_freespace_carve_depth_device(mrh_ctx* c, const mrh_carve_params* p, const float* d_depth, const float R_row_major[9], const float t[3]) {
  return carve_run(c, "mrh_freespace_carve_depth_device", true, p, nullptr, d_depth, 0, R_row_major, t);
}

int mrh_freespace_carve_points(mrh_ctx* c, const mrh_carve_params* p, const float* points_host, uint64_t n, const float R_row_major[9], const float t[3]) {
  return carve_run(c, "mrh_freespace_carve_points", false, p, points_host, nullptr, n, R_row_major, t);
}

int mrh_freespace_carve_points_device(mrh_ctx* c, const mrh_carve_params* p, const float* d_points, uint64_t n, const float R_row_major[9], const float t[3]) {
  return carve_run(c, "mrh_freespace_carve_points_device", false, p, nullptr, d_points, n, R_row_major, t);
}

int mrh_freespace_box(mrh_ctx* c, const mrh_freespace_box_params* p, const uint8_t** out_state) {
  FreeBox bx;
  int rc = freebox_enter(c, "mrh_freespace_box", p, out_state != nullptr, &bx);
  if (rc) return rc;
  mrh_ctx::Free& F = c->free;
  const size_t n = (size_t) bx.nx * (size_t) bx.ny * (size_t) bx.nz;
  if ((rc = regrow(c, F.d_state, F.state_cap, n, n, false))) return rc;  // the previous mrh_freespace_box has finished (it blocked)
  if ((rc = regrow_pinned(c, F.h_state, F.h_cap, n, n))) return rc;
  if ((rc = launch_freebox(c, bx, F.d_state))) return rc;
  Plane pl[1] = {{0, n, F.d_state, true}};
  if ((rc = read_planes(c, (char*) F.h_state, pl))) return rc;
  *out_state = (const uint8_t*) pl[0].host;
  return MRH_OK;
}

int mrh_freespace_box_device(mrh_ctx* c, const mrh_freespace_box_params* p, uint8_t* d_state) {
  FreeBox bx;
  const int rc = freebox_enter(c, "mrh_freespace_box_device", p, d_state != nullptr, &bx);
  return rc ? rc : launch_freebox(c, bx, d_state);
}

int mrh_freespace_segments(mrh_ctx* c, const float* a_host, const float* b_host, uint64_t n, float step, const uint8_t** out_status, const uint32_t** out_counts) {
  SegArgs a;
  int rc = segments_enter(c, "mrh_freespace_segments", a_host && b_host, true, n, step, &a);
  if (rc) return rc;
  if (out_status) *out_status = nullptr;
  if (out_counts) *out_counts = nullptr;
  if (n == 0) return MRH_OK;
  mrh_ctx::Free& F = c->free;
  // per segment [counts 2 x u32 | status u8], each plane contiguous, on the device as in the pinned copy
  const size_t ns = (size_t) n, bytes = ns * (2 * sizeof(u32) + 1);
  if ((rc = regrow(c, F.d_seg, F.seg_cap, ns, bytes, false))) return rc;  // the previous mrh_freespace_segments has finished (it blocked)
  if ((rc = regrow_pinned(c, F.h_seg, F.h_seg_cap, ns, bytes))) return rc;
  RaysIn in;  // the two endpoint lists through the staging pair, as the ray queries stage origins and directions
  if ((rc = stage_rays(c, a_host, b_host, nullptr, ns, &in))) return rc;
  enum { COUNTS, STATUS };
  Plane pl[2] = {{0, ns * 2 * sizeof(u32), F.d_seg, out_counts != nullptr}, {ns * 2 * sizeof(u32), ns, F.d_seg + ns * 2 * sizeof(u32), out_status != nullptr}};
  if ((rc = launch_segments(c, a, in.origins, in.dirs, (uint8_t*) pl[STATUS].dev, (u32*) pl[COUNTS].device()))) return rc;
  if ((rc = read_planes(c, F.h_seg, pl))) return rc;  // blocks also when nothing is wanted: the staging pair is free again
  if (out_status) *out_status = (const uint8_t*) pl[STATUS].host;
  if (out_counts) *out_counts = (const uint32_t*) pl[COUNTS].host;
  return MRH_OK;
}

int mrh_freespace_segments_device(mrh_ctx* c, const float* d_a, const float* d_b, uint64_t n, float step, uint8_t* d_status, uint32_t* d_counts) {
  SegArgs a;
  const int rc = segments_enter(c, "mrh_freespace_segments_device", d_a && d_b, d_status != nullptr, n, step, &a);
  if (rc || n == 0) return rc;
  return launch_segments(c, a, d_a, d_b, d_status, (u32*) d_counts);
}

int mrh_resample_map(mrh_ctx* src, const mrh_remap_params* p, const float R_row_major[9], const float t[3], const mrh_block_record** out_records, uint64_t* out_n,
                     mrh_remap_info* out_info) {
  const char* who = "mrh_resample_map";
  RemapArgs a;
  int rc = reader_enter(src, who, [&](char* msg) { return remap_plan(msg, who, src, nullptr, p, R_row_major, t, out_records && out_n, &a); });
  if (rc) return rc;
  mrh_remap_info info = {};
  rc = remap_run(src, who, a, out_records, out_n, &info);
  if (out_info) *out_info = info;
  return rc;
}

int mrh_fuse_map(mrh_ctx* dst, mrh_ctx* src, const mrh_remap_params* p, const float R_row_major[9], const float t[3], mrh_remap_info* out_info) {
  const char* who = "mrh_fuse_map";
  RemapArgs a;
  int rc = pair_enter(dst, src, who, [&](char* msg) { return remap_plan(msg, who, src, dst, p, R_row_major, t, true, &a); });
  if (rc) return rc;
  mrh_remap_info info = {};
  const mrh_block_record* records = nullptr;
  uint64_t n = 0;
  rc = source_rc(dst, src, who, remap_run(src, who, a, &records, &n, &info));  // it blocks: src's stream is drained before dst's stream reads the records
  if (!rc && n) rc = unpack_records(dst, MRH_UNPACK_MERGE, records, n, 1, &info.taken);
  if (out_info) *out_info = info;
  return rc;
}

int mrh_align_map(mrh_ctx* dst, mrh_ctx* src, const mrh_align_params* p, const float R_init[9], const float t_init[3], float out_R[9], float out_t[3],
                  mrh_align_info* out_info) {
  const char* who = "mrh_align_map";
  mrh_plan::Align plan;
  int rc = pair_enter(dst, src, who, [&](char* msg) {
    return mrh_plan::align(msg, who, p, R_init, t_init, out_R && out_t, dst == src, dst->device == src->device, src->p.sdf_truncation, src->pending,
                           src->map.shard_count, dst->p.sdf_truncation, dst->pending, dst->map.shard_count, &plan);
  });
  if (rc) return rc;
  uint64_t n_blocks = 0, n_samples = 0;
  // align_gather blocks: src's stream is drained before dst's stream reads the samples
  if ((rc = source_rc(dst, src, who, align_gather(src, who, plan, &n_blocks, &n_samples)))) return rc;
  mrh_track::Fit f(R_init, t_init);  // an empty sample list is lost: nothing is launched on dst
  if (n_samples) {
    const size_t n_rows = (size_t) ((n_samples + kAlignLanes - 1) / kAlignLanes);  // the destination half: on dst's stream with dst's Map / Tab
    AlignLin k;
    for (int i = 0; i < 3; i++) k.c[i] = plan.pivot[i];
    k.band = plan.band; k.dist_max = plan.dist_max; k.s_a = mrh_track::angle_scale(plan.extent);
    k.bound = (float) (1 << 20) * dst->map.vs; k.n = (uint32_t) n_samples;
    mrh_plan::align_tau(f.R, plan.pivot, f.t, f.t);  // the loop's translation is tau, about the pivot (element by element: in place)
    rc = mrh_track::fit_run(f, plan.iterations, k.s_a, plan.min_samples, [&](const float* R, const float* tau, int64_t* sums) {
      for (int i = 0; i < 9; i++) k.R[i] = R[i];
      for (int i = 0; i < 3; i++) k.tau[i] = tau[i];
      return linearise_sums(dst, n_rows, [&](i64* slab) {
        k_align_linearise<<<(unsigned) n_rows, kAlignLanes, 0, dst->stream>>>(dst->map, dst->tab, k, src->align.d_samples, slab);
      }, sums);
    });
    if (rc < 0) return rc;
    mrh_plan::align_t(f.R, plan.pivot, f.t, f.t);
  }
  mrh_track::fit_report(f, out_R, out_t, out_info, &mrh_align_info::accepted);
  if (out_info) {
    out_info->source_blocks = n_blocks;
    out_info->samples = n_samples;
    for (int i = 0; i < 3; i++) out_info->pivot[i] = plan.pivot[i];
    out_info->extent = plan.extent;
  }
  return MRH_OK;
}

}  // extern "C"
