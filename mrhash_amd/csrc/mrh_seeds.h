// mrh_seeds.h — the host side of 3DGS splat seeding behind the C ABI: mrh_splat_seeds, a driver over named stages (checks, the
// tree's shape, buffers, the launches, the read-back of totals and seeds from pinned memory), and mrh_get_qtree_leaves.
// GaussianContainer::extractNodesQTree + checkNodes (gaussian_data_structures.cpp:48-68, .cu:58-84); the kernels are in mrh_splat.h
// and mrh_sort.h.  The state is mrh_ctx::qt.  Included by mrh_capi.hip, same translation unit: it needs the context's internals
// (mrh_ctx, HIP_TRY, fail, regrow_all, regrow_pinned, pinned_alloc, ensure_ready and, from mrh_upload.h, send_uploads and mark_frame).
#pragma once

namespace {

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
// The buffers of a tree of qt.total potential nodes.  The seven device buffers sized by the node count and d_misc are one
// regrow_all under Seeds::cap, reallocated whenever the count differs, not only when it grows.  A failed allocation leaves no device
// buffer and capacity 0, so the next call allocates again whatever its image shape; the last call's leaves go with d_leaves.
// The pinned seeds only grow (regrow_pinned; they used to shrink with the tree): k_qt_scatter is told their capacity.
int qtree_buffers(mrh_ctx* c, const QTree& qt) {
  mrh_ctx::Seeds& S = c->qt;
  const size_t n = qt.total, seeds = std::min<size_t>(n, (size_t) 1 << 20);  // seeds <= leaves <= 1 000 000 (mrh_splat_seeds checks)
  int rc = MRH_OK;
  if (n != S.cap) {
    S.n_leaves = 0;
    S.leaves_on_host = true;
    S.leaves.clear();
    rc = regrow_all(c, S.cap, n, {{S.d_sums, n * sizeof(QSum)}, {S.d_flags, n * sizeof(u32)}, {S.d_unc, n * sizeof(u32)}, {S.d_marks, n * sizeof(u64)},
                                  {S.d_pos, (n + (n + kChainTile - 1) / kChainTile + 1) * sizeof(u64)},  // + the tile sums of the marks' scan
                                  {S.d_parked, n * sizeof(mrh_splat_seed)}, {S.d_leaves, n * sizeof(mrh_qtree_leaf)}, {S.d_misc, 2 * sizeof(u64)}});
  }
  if (!rc) rc = regrow_pinned(c, S.h_seeds, S.seed_cap, seeds, seeds * sizeof(mrh_splat_seed));
  if (rc) return rc;
  if (!S.h_out) HIP_TRY(c, pinned_alloc(c, S.h_out, 2 * sizeof(u64)));
  return MRH_OK;
}
int launch_qtree(mrh_ctx* c, const QTree& qt, const float qtree_thresh) {
  const mrh_ctx::Seeds& S = c->qt;
  hipStream_t s = c->stream;
  const u32 grid = (qt.total + 255) / 256;
  u32* unc_count = (u32*) (S.d_misc + 1);
  // exact statistics of every potential node, four tree levels per launch
  int L = qt.D, T = L < 4 ? L : 4;
  k_qt_sums_bottom<<<1u << (2 * (L - T)), 256, 0, s>>>(qt, c->d_rgb, S.d_sums, T, S.d_misc);
  for (L -= T; L > 0; L -= T) {
    T = L < 4 ? L : 4;
    k_qt_sums_up<<<1u << (2 * (L - T)), 256, 0, s>>>(qt, S.d_sums, L, T);
  }
  // exclusive scan of the marks (mrh_sort.h): the tile sums (parked behind the positions) are cleared by k_qt_decide and added up by
  // k_qt_emit's workgroups, then every tile scans on its own
  const u32 tiles = (u32) ((qt.total + kChainTile - 1) / kChainTile);
  static_assert(kChainTile % 256 == 0, "a workgroup of k_qt_emit lies inside one scan tile");
  k_qt_decide<<<grid, 256, 0, s>>>(qt, qtree_thresh, S.d_sums, S.literal, S.d_flags, S.d_unc, unc_count, S.d_pos + qt.total, tiles);
  k_qt_literal<<<512, 256, 0, s>>>(qt, c->d_rgb, qtree_thresh, S.d_unc, unc_count, S.d_flags);
  k_qt_emit<<<grid, 256, 0, s>>>(qt, c->cam, c->map, c->tab, c->d_depth, c->d_rgb, S.d_flags, S.d_marks, S.d_parked, S.d_pos + qt.total);
  k_tile_scan_u64<<<tiles, 1024, 0, s>>>(S.d_marks, (u32) qt.total, S.d_pos + qt.total, S.d_pos);
  k_qt_scatter<<<grid, 256, 0, s>>>(qt, S.d_marks, S.d_pos, S.d_parked, S.d_leaves, S.h_seeds, (u32) S.seed_cap, S.d_misc, S.h_out);
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

}  // namespace

extern "C" {

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
  mrh_ctx::Seeds& S = c->qt;
  const u64 h_misc[2] = {((volatile u64*) S.h_out)[0], ((volatile u64*) S.h_out)[1]};
  const uint64_t n_leaves = h_misc[0] & 0xFFFFFFFFull, n_seeds = h_misc[0] >> 32;
  S.last_literal = (uint32_t) h_misc[1];
  if (n_leaves > 1000000ull) return fail(c, MRH_ERR_CAPACITY, "mrh_splat_seeds: %llu leaves, above the reference's capacity of 1000000 (params.h:20-23)", (unsigned long long) n_leaves);
  // the leaves (tens of thousands per frame) stay on the device until mrh_get_qtree_leaves asks: the fusion loop only takes the seeds
  S.n_leaves = n_leaves;
  S.leaves_on_host = n_leaves == 0;
  S.leaves.clear();
  if (getenv("MRH_DEBUG")) {
    fprintf(stderr, "[mrh] splat seeds: %u potential nodes, %u literal evaluations, %llu leaves, %llu seeds\n", qt.total,
            S.last_literal, (unsigned long long) n_leaves, (unsigned long long) n_seeds);
  }
  *out_n = n_seeds;
  *out = S.h_seeds;
  return MRH_OK;
}

int mrh_get_qtree_leaves(mrh_ctx* c, const mrh_qtree_leaf** out, uint64_t* out_n) {
  if (!c || !out || !out_n) return MRH_ERR_INVALID_ARG;
  mrh_ctx::Seeds& S = c->qt;
  if (!S.leaves_on_host) {
    S.leaves.resize(S.n_leaves);
    HIP_TRY(c, hipMemcpyAsync(S.leaves.data(), S.d_leaves, S.n_leaves * sizeof(mrh_qtree_leaf), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    S.leaves_on_host = true;
  }
  *out = S.leaves.data();
  *out_n = S.leaves.size();
  return MRH_OK;
}

}  // extern "C"
