// mrh_blocks.h — the host side of block I/O behind the C ABI (streamer, dump, get_voxel, the multi-GPU pack / unpack / drop), each
// entry point a driver over named stages.  dump_compact, free_compact_launch, import_pipe, pack_selected and unpack_records are the
// one launch site of their kernels (mrh_comm.h packs through pack_selected, mrh_fuse_map merges through unpack_records; a reader of the whole map, mrh_readers.h, gets its blocks from borrow_live_blocks).  Included by mrh_capi.hip, same translation unit: it needs mrh_ctx's internals.
#pragma once

namespace {

// flags raised by earlier frames are set aside (mrh_sync reports them) so that a call which checks its own outcome on the
// device — import, unpack — answers for itself only
int set_aside_flags(mrh_ctx* c) {
  u32 flags = 0;
  const int rc = take_device_flags(c, &flags);
  if (!rc) c->flags_deferred |= flags;
  return rc;
}
// Host flags after blocks came or went behind the frame paths' back (import, unpack, drop).  NOT mrh_stream_out: what it leaves is
// the payload the frames wrote, so it only sets table_dirty and drops the refill test — a multi-resolution map stays on the fused path.
void map_changed_in_bulk(mrh_ctx* c) {
  c->mr_next_general = true;  // payload that has not been through a variance check
  c->refill_flag_valid = false;
  c->mr_summaries_valid = false;
  c->table_dirty = true;
}

// room on the coarse free list for `need` coarse blocks, in allocateMemoryLow's portions (vds.cu:860-871: k_refill): an import or a
// merge into a context whose frames have not refilled the list yet (vds.cu:885-891 does it at the start of a frame).  Blocks.
int ensure_coarse_units(mrh_ctx* c, const uint64_t need) {
  if (!c->tab.multi_res || need == 0) return MRH_OK;
  hipStream_t s = c->stream;
  int lev[2] = {0, 0};  // CTR_HEAP_FINE, CTR_HEAP_COARSE are adjacent: stack tops, free count = top + 1
  HIP_TRY(c, hipMemcpyAsync(lev, &c->tab.ctr[CTR_HEAP_FINE], 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  int64_t fine_free = (int64_t) lev[0] + 1, coarse_free = (int64_t) lev[1] + 1;
  while (coarse_free < (int64_t) need && c->low_blocks_to_allocate > 0 && fine_free > (int64_t) c->low_blocks_to_allocate) {
    HIP_TRY(c, hipMemsetAsync(c->d_flag, 0xFF, sizeof(int), s));  // any non-zero flag: refill
    k_refill<<<(c->low_blocks_to_allocate + 255) / 256, 256, 0, s>>>(c->tab, c->low_blocks_to_allocate, c->d_flag);
    fine_free -= c->low_blocks_to_allocate;
    coarse_free += 8 * (int64_t) c->low_blocks_to_allocate;
  }
  c->refill_flag_valid = false;
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
// live blocks matching a predicate -> Tab::compact[0, n)
int select_blocks(mrh_ctx* c, int sel_mode, int rank_arg, int* out_n) {
  HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_COMPACT], 0, sizeof(int), c->stream));
  k_select_blocks<<<512, 256, 0, c->stream>>>(c->map, c->tab, sel_mode, rank_arg);
  HIP_TRY(c, hipMemcpyAsync(out_n, &c->tab.ctr[CTR_COMPACT], sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
// Every live block -> Tab::compact[0, n) for a reader of the whole map (mrh_resample_map / mrh_fuse_map, mrh_align_map): the
// kSelAll selection borrows the frame path's compact list, and its counter — what mrh_stats reports of the last frame — is put
// back.  Tab::compact[0, n) itself stays for the reader's kernels: the reader blocks, so nothing else runs on the stream.  Blocks
int borrow_live_blocks(mrh_ctx* c, int* out_n) {
  if (!c->d_keep) HIP_TRY(c, dev_alloc(c, c->d_keep, sizeof(int)));
  HIP_TRY(c, hipMemcpyAsync(c->d_keep, &c->tab.ctr[CTR_COMPACT], sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  const int rc = select_blocks(c, kSelAll, 0, out_n);
  HIP_TRY(c, hipMemcpyAsync(&c->tab.ctr[CTR_COMPACT], c->d_keep, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  return rc;
}

// Tab::compact[0, n) -> the caller's descs (and voxels, if asked for), 8 192 blocks (48 MiB of voxels) per round trip; blocking
int dump_compact(mrh_ctx* c, const int n, mrh_block_desc* descs, mrh_voxel* voxels) {
  const int chunk = 8192;
  DevBuf<int4> d_descs;
  DevBuf<char> d_vox;
  HIP_TRY(c, d_descs.alloc((size_t) chunk));
  HIP_TRY(c, d_vox.alloc((size_t) chunk * kFineBytes));
  for (int first = 0; first < n; first += chunk) {
    const int cnt = (n - first) < chunk ? (n - first) : chunk;
    k_dump<<<cnt < 2048 ? cnt : 2048, 512, 0, c->stream>>>(c->tab, first, cnt, d_descs, d_vox);
    HIP_TRY(c, hipMemcpyAsync(&descs[first], d_descs, (size_t) cnt * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    if (voxels) HIP_TRY(c, hipMemcpyAsync(&voxels[(size_t) first * 512], d_vox, (size_t) cnt * kFineBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
// frees Tab::compact[0, n), n > 0 (garbageCollectFree's kernel with every decision set); blocking.  Which host flags the erase
// resets is the caller's: mrh_stream_out and mrh_drop_blocks differ there (map_changed_in_bulk).
int free_compact_launch(mrh_ctx* c, const int n) {
  HIP_TRY(c, hipMemcpyAsync(&c->tab.ctr[CTR_COMPACT], &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
  k_fill_u32<<<256, 256, 0, c->stream>>>(c->d_decision, (size_t) n, 1u);
  k_gc_free<false><<<256, 256, 0, c->stream>>>(c->tab, c->d_decision);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}

// The streamer's selection among the n blocks of Tab::compact: at `radius` or more from `center` (radius < 0: all), in position
// order if `sorted`.  A handful of flops per live block: done on the host copy of the list, which the canonical order needs anyway.
int select_far_blocks(mrh_ctx* c, const int n, const float center[3], const float radius, const bool sorted, std::vector<int4>* sel) {
  std::vector<int4> list((size_t) n);
  HIP_TRY(c, hipMemcpy(list.data(), c->tab.compact, (size_t) n * sizeof(int4), hipMemcpyDeviceToHost));
  const float vs = c->map.vs;
  sel->reserve((size_t) n);
  for (const int4& e : list) {
    const float px = (float) (e.x * kBlockSide) * vs, py = (float) (e.y * kBlockSide) * vs, pz = (float) (e.z * kBlockSide) * vs;
    const float dx = px - center[0], dy = py - center[1], dz = pz - center[2];
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (radius >= 0.f && !(d >= radius)) continue;
    sel->push_back(e);
  }
  if (sorted) std::sort(sel->begin(), sel->end(), [](const int4& a, const int4& b) { return std::tie(a.x, a.y, a.z) < std::tie(b.x, b.y, b.z); });
  return MRH_OK;
}

// n blocks of the caller's (pageable: the runtime stages it) memory into the map.  Two staging buffers, the copies on their own
// stream: the host-to-device copy of chunk i + 1 runs under the insert kernel of chunk i; one synchronisation at the end
int import_pipe(mrh_ctx* c, const mrh_block_desc* descs, const mrh_voxel* voxels, const uint64_t n) {
  const uint64_t chunk = 4096;  // 24 MiB of voxels
  struct Pipe {
    hipStream_t copy = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    ~Pipe() {
      if (copy) { (void) hipStreamSynchronize(copy); (void) hipStreamDestroy(copy); }
      for (hipEvent_t e : copied) if (e) (void) hipEventDestroy(e);
      for (hipEvent_t e : done) if (e) (void) hipEventDestroy(e);
    }
  } pipe;
  DevBuf<int4> d_descs[2];
  DevBuf<char> d_vox[2];
  const int nbuf = n > chunk ? 2 : 1;
  HIP_TRY(c, hipStreamCreateWithFlags(&pipe.copy, hipStreamNonBlocking));
  for (int b = 0; b < nbuf; b++) {
    HIP_TRY(c, d_descs[b].alloc(chunk));
    HIP_TRY(c, d_vox[b].alloc(chunk * (size_t) kFineBytes));
    HIP_TRY(c, hipEventCreateWithFlags(&pipe.copied[b], hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&pipe.done[b], hipEventDisableTiming));
  }
  uint64_t it = 0;
  for (uint64_t first = 0; first < n; first += chunk, it++) {
    const uint64_t cnt = (n - first) < chunk ? (n - first) : chunk;
    const int b = (int) (it & 1);
    if (it >= 2) HIP_TRY(c, hipStreamWaitEvent(pipe.copy, pipe.done[b], 0));  // the kernel that read this buffer two chunks ago
    HIP_TRY(c, hipMemcpyAsync(d_descs[b], &descs[first], cnt * sizeof(int4), hipMemcpyHostToDevice, pipe.copy));
    HIP_TRY(c, hipMemcpyAsync(d_vox[b], &voxels[first * 512], cnt * (size_t) kFineBytes, hipMemcpyHostToDevice, pipe.copy));
    HIP_TRY(c, hipEventRecord(pipe.copied[b], pipe.copy));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, pipe.copied[b], 0));
    k_import<kImportPlain><<<(int) (cnt < 2048 ? cnt : 2048), 512, 0, c->stream>>>(c->map, c->tab, c->fast.summary, (int) cnt, (const char*) (int4*) d_descs[b], sizeof(int4),
                                                                                   (const char*) d_vox[b], (size_t) kFineBytes, nullptr, nullptr);
    HIP_TRY(c, hipEventRecord(pipe.done[b], c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return MRH_OK;
}
// the n selected blocks of Tab::compact as records at `dst` (device memory); enqueue only
void pack_selected(mrh_ctx* c, const int n, char* dst) {
  if (n) k_pack_records<<<n < 4096 ? n : 4096, 512, 0, c->stream>>>(c->tab, 0, n, dst);
}
// mrh_unpack_blocks behind its argument checks, and mrh_fuse_map (mrh_readers.h) with the records it has just resampled: n >= 1
// records (device memory iff is_device_memory) through k_import in `mode`; the one launch site of both forms.  Blocks
int unpack_records(mrh_ctx* c, const int mode, const mrh_block_record* records, const uint64_t n, const int is_device_memory, uint64_t* out_taken) {
  int rc;
  if ((rc = set_aside_flags(c))) return rc;
  hipStream_t s = c->stream;
  DevBuf<char> staged;  // host records (tests over gloo) are read from one staged copy
  const char* d_rec = (const char*) records;
  if (!is_device_memory) {
    HIP_TRY(c, staged.alloc((size_t) n * sizeof(mrh_block_record)));
    HIP_TRY(c, hipMemcpyAsync(staged, records, (size_t) n * sizeof(mrh_block_record), hipMemcpyHostToDevice, s));
    d_rec = staged;
  }
  if (!c->d_taken) HIP_TRY(c, dev_alloc(c, c->d_taken, sizeof(u32)));
  HIP_TRY(c, hipMemsetAsync(c->d_taken, 0, sizeof(u32), s));
  const size_t room = c->halo_upper + n, cap = room + room / 2;  // the halo list takes every record of the call behind its entries
  if (mode == MRH_UNPACK_HALO && room > c->halo_cap) {
    if ((rc = regrow_keep(c, c->d_halo, c->halo_cap, cap, cap * sizeof(int4), c->halo_upper * sizeof(int4)))) return rc;
  }
  map_changed_in_bulk(c);
  DevBuf<u32> released;  // a merge into a variance-adaptive map: the fine slots that make way for coarse records ...
  if (mode == MRH_UNPACK_MERGE && c->tab.multi_res) {  // ... and room on the coarse free list for every coarse record of the call
    HIP_TRY(c, released.alloc((size_t) n + 1));
    HIP_TRY(c, hipMemsetAsync(released, 0, sizeof(u32), s));
    k_count_coarse_records<<<64, 256, 0, s>>>(d_rec, sizeof(mrh_block_record), (int) n, c->d_taken);  // d_taken doubles as the counter
    u32 need = 0;
    HIP_TRY(c, hipMemcpyAsync(&need, c->d_taken, sizeof(u32), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemsetAsync(c->d_taken, 0, sizeof(u32), s));
    if ((rc = ensure_coarse_units(c, need))) return rc;
  }
  const int grid = (int) (n < 4096 ? n : 4096);
  const size_t stride = sizeof(mrh_block_record);
  if (mode == MRH_UNPACK_HALO) {
    k_import<kImportHalo><<<grid, 512, 0, s>>>(c->map, c->tab, c->fast.summary, (int) n, d_rec, stride, d_rec + sizeof(mrh_block_desc), stride, c->d_halo, c->d_taken);
    c->halo_upper += n;
  } else {
    k_import<kImportMerge><<<grid, 512, 0, s>>>(c->map, c->tab, c->fast.summary, (int) n, d_rec, stride, d_rec + sizeof(mrh_block_desc), stride, nullptr, c->d_taken,
                                                (u32*) released);
    if (released.p) k_release_fine<<<1, 256, 0, s>>>(c->tab, released);
  }
  u32 taken = 0;
  HIP_TRY(c, hipMemcpyAsync(&taken, c->d_taken, sizeof(u32), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  if (out_taken) *out_taken = taken;
  u32 flags = 0;  // what this call raised itself is its own result
  rc = take_device_flags(c, &flags);
  return rc ? rc : check_device_flags(c, flags);
}
}  // namespace

extern "C" {

// Streamer, device half (streamer.cu:11-160): select by distance from the camera, copy out, free.
int mrh_stream_out(mrh_ctx* c, const float center[3], float radius, mrh_block_desc* descs, mrh_voxel* voxels, uint64_t capacity,
                   uint64_t* out_n) {
  int rc = ensure_ready(c, "mrh_stream_out");
  if (rc) return rc;
  if (!out_n || !center) return MRH_ERR_INVALID_ARG;
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_stream_out: an exchange is pending (call mrh_integrate_resume)");
  c->refill_flag_valid = false;  // freed coarse units change the level the next frame's refill test must see
  int n = 0;
  if ((rc = compact_all(c, &n))) return rc;
  *out_n = 0;
  if (n == 0) return MRH_OK;
  std::vector<int4> sel;
  if ((rc = select_far_blocks(c, n, center, radius, descs != nullptr, &sel))) return rc;
  *out_n = sel.size();
  if (!descs || sel.empty()) return MRH_OK;
  if (sel.size() > capacity) return fail(c, MRH_ERR_CAPACITY, "mrh_stream_out: capacity %llu < %zu blocks to stream out", (unsigned long long) capacity, sel.size());
  const int ns = (int) sel.size();
  HIP_TRY(c, hipMemcpy(c->tab.compact, sel.data(), (size_t) ns * sizeof(int4), hipMemcpyHostToDevice));  // the selection replaces the list
  if ((rc = dump_compact(c, ns, descs, voxels))) return rc;
  rc = free_compact_launch(c, ns);
  c->table_dirty = true;  // a bulk erase: census (and, if due, rebuild) before the next frame.  Nothing else: see map_changed_in_bulk
  return rc;
}

int mrh_dump_blocks(mrh_ctx* c, mrh_block_desc* descs, mrh_voxel* voxels, uint64_t capacity, uint64_t* out_n) {
  int rc = ensure_ready(c, "mrh_dump_blocks");
  if (rc) return rc;
  if (!out_n) return MRH_ERR_INVALID_ARG;
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_dump_blocks: an exchange is pending (call mrh_integrate_resume)");  // the starve passes still need Tab::compact
  int n = 0;
  if ((rc = compact_all(c, &n))) return rc;
  *out_n = (uint64_t) n;
  if (!descs) return MRH_OK;
  if ((uint64_t) n > capacity) return fail(c, MRH_ERR_CAPACITY, "mrh_dump_blocks: capacity %llu < %d live blocks", (unsigned long long) capacity, n);
  return dump_compact(c, n, descs, voxels);
}

int mrh_get_voxel(mrh_ctx* c, int32_t vx, int32_t vy, int32_t vz, mrh_voxel* out, int* out_found) {
  int rc = ensure_ready(c, "mrh_get_voxel");
  if (rc) return rc;
  if (!out) return MRH_ERR_INVALID_ARG;
  k_get_voxel<<<1, 1, 0, c->stream>>>(c->map, c->tab, vx, vy, vz, c->d_misc);
  u32 h[4];
  HIP_TRY(c, hipMemcpyAsync(h, c->d_misc, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(&out->sdf, &h[0], 4);
  memcpy(&out->sum_squared, &h[1], 4);
  out->rgb[0] = h[2] & 0xFF; out->rgb[1] = (h[2] >> 8) & 0xFF; out->rgb[2] = (h[2] >> 16) & 0xFF;
  out->weight = (uint8_t) (h[2] >> 24);
  if (out_found) *out_found = (int) h[3];
  return MRH_OK;
}

int mrh_import_blocks(mrh_ctx* c, const mrh_block_desc* descs, const mrh_voxel* voxels, uint64_t n) {
  int rc = ensure_ready(c, "mrh_import_blocks");
  if (rc) return rc;
  if (n == 0) return MRH_OK;
  if (!descs || !voxels) return fail(c, MRH_ERR_INVALID_ARG, "mrh_import_blocks: null argument");
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_import_blocks: an exchange is pending (call mrh_integrate_resume)");
  if ((rc = set_aside_flags(c))) return rc;
  if (c->tab.multi_res) {  // room on the coarse free list for every coarse block of the call
    uint64_t need = 0;
    for (uint64_t k = 0; k < n; k++) need += descs[k].resolution != 0;
    if ((rc = ensure_coarse_units(c, need))) return rc;
  }
  map_changed_in_bulk(c);
  if ((rc = import_pipe(c, descs, voxels, n))) return rc;
  u32 flags = 0;  // what this call raised itself is its own result
  rc = take_device_flags(c, &flags);
  return rc ? rc : check_device_flags(c, flags);
}

// ---- multi-GPU block exchange (include/mrhash_hip.h) -----------------------------------------------------------------

int mrh_set_sharding(mrh_ctx* c, int shard_rank, int shard_count, int shard_chunk_log2) {
  if (!c) return MRH_ERR_INVALID_ARG;
  if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return fail(c, MRH_ERR_INVALID_ARG, "mrh_set_sharding: rank %d of %d", shard_rank, shard_count);
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_set_sharding: an exchange is pending (call mrh_integrate_resume)");
  const int rc = ensure_ready(c, "mrh_set_sharding");  // the last pipelined frame is integrated under the ownership it was allocated with
  if (rc) return rc;
  c->p.shard_rank = shard_rank; c->p.shard_count = shard_count; c->p.shard_chunk_log2 = shard_chunk_log2;
  c->map.shard_rank = shard_rank;
  c->map.shard_count = shard_count;
  c->map.shard_chunk_log2 = (shard_chunk_log2 > 0 && shard_chunk_log2 < 16) ? shard_chunk_log2 : 3;
  return MRH_OK;
}

int mrh_pack_blocks(mrh_ctx* c, int mode, int rank_arg, const mrh_block_record** out_records, uint64_t* out_n, int* out_is_device_memory) {
  int rc = ensure_ready(c, "mrh_pack_blocks");
  if (rc) return rc;
  if (!out_records || !out_n) return MRH_ERR_INVALID_ARG;
  if (mode != MRH_PACK_HALO && mode != MRH_PACK_OWNER) return fail(c, MRH_ERR_INVALID_ARG, "mrh_pack_blocks: bad mode %d", mode);
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_pack_blocks: an exchange is pending (call mrh_integrate_resume)");
  int n = 0;
  if ((rc = select_blocks(c, mode == MRH_PACK_HALO ? kSelHalo : kSelOwner, rank_arg, &n))) return rc;
  if (out_is_device_memory) *out_is_device_memory = 1;
  *out_n = (uint64_t) n;
  *out_records = nullptr;
  if (n == 0) return MRH_OK;
  const size_t bytes = (size_t) n * sizeof(mrh_block_record);
  // select_blocks blocked: nothing reads the old buffer
  if (bytes > c->pack_cap && (rc = regrow(c, c->d_pack, c->pack_cap, bytes + bytes / 4, bytes + bytes / 4, false))) return rc;
  pack_selected(c, n, c->d_pack);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  *out_records = (const mrh_block_record*) c->d_pack;
  return MRH_OK;
}

int mrh_unpack_blocks(mrh_ctx* c, int mode, const mrh_block_record* records, uint64_t n, int is_device_memory, uint64_t* out_taken) {
  int rc = ensure_ready(c, "mrh_unpack_blocks");
  if (rc) return rc;
  if (out_taken) *out_taken = 0;
  if (mode != MRH_UNPACK_HALO && mode != MRH_UNPACK_MERGE) return fail(c, MRH_ERR_INVALID_ARG, "mrh_unpack_blocks: bad mode %d", mode);
  if (n == 0) return MRH_OK;
  if (!records) return fail(c, MRH_ERR_INVALID_ARG, "mrh_unpack_blocks: null argument");
  if (n > 0x7FFFFFFFull) return fail(c, MRH_ERR_CAPACITY, "mrh_unpack_blocks: %llu records in one call", (unsigned long long) n);
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_unpack_blocks: an exchange is pending (call mrh_integrate_resume)");
  return unpack_records(c, mode, records, n, is_device_memory, out_taken);
}

int mrh_drop_blocks(mrh_ctx* c, int mode, uint64_t* out_dropped) {
  int rc = ensure_ready(c, "mrh_drop_blocks");
  if (rc) return rc;
  if (out_dropped) *out_dropped = 0;
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_drop_blocks: an exchange is pending (call mrh_integrate_resume)");
  if (mode != MRH_DROP_HALO && mode != MRH_DROP_FOREIGN && mode != MRH_DROP_ALL) return fail(c, MRH_ERR_INVALID_ARG, "mrh_drop_blocks: bad mode %d", mode);
  int n = 0;
  if (mode == MRH_DROP_HALO) {  // the halo list -> Tab::compact[0, n)
    HIP_TRY(c, hipMemcpyAsync(&n, &c->tab.ctr[CTR_HALO], sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(c->tab.compact, c->d_halo, (size_t) n * sizeof(int4), hipMemcpyDeviceToDevice, c->stream));
  } else if ((rc = select_blocks(c, mode == MRH_DROP_FOREIGN ? kSelForeign : kSelAll, 0, &n))) return rc;
  HIP_TRY(c, hipMemsetAsync(&c->tab.ctr[CTR_HALO], 0, sizeof(int), c->stream));  // halo blocks are foreign: they go with the rest
  c->halo_upper = 0;
  if (n > 0) {
    if ((rc = free_compact_launch(c, n))) return rc;
    map_changed_in_bulk(c);
  }
  if (out_dropped) *out_dropped = (uint64_t) n;
  return MRH_OK;
}

}  // extern "C"
