// mrh_upload.h — host images on their way to the device, and what a frame leaves behind for the host: the two upload rings
// (upload_image, send_uploads), the frame marks that free a ring slot for reuse (mark_frame) and the pool reports behind the
// non-blocking peeks (enable_peeks, newest_report, post_report).  Needs mrh_context.h and mrh_hostcopy.h.
#pragma once
namespace {

// one host image into the next slot of its ring: wait until the slot is free, copy into pinned staging (the caller's
// buffer is free on return), enqueue the H2D on the copy stream
int upload_image(mrh_ctx* c, UpRing& ring, const void* src, const size_t bytes, const void** out_dev) {
  // One copy stream per image kind: the depth and the colour image of a frame then move through two SDMA engines side by
  // side (64 us per frame instead of 77 on one stream).  A copy kernel pulling the pinned buffer over PCIe is faster on its
  // own (48 GB/s against 25-30, tools/micro/h2d_paths.hip) but finds no wave slots while k_back fills every SIMD's
  // registers, neither with stream priority nor with CU masks (tools/micro/cu_mask_overlap.hip: a masked stream costs the
  // big kernel 14 %): measured at 73-75 us per frame inside the library, and dropped.
  if (!ring.stream) HIP_TRY(c, hipStreamCreateWithFlags(&ring.stream, hipStreamNonBlocking));
  const int next = (ring.cur + 1) % 3;
  // a frame that mrh_integrate kept back (flush_deferred) has not marked its slots yet: before the ring comes round to one of them, it runs
  if (c->deferred.on && next == c->deferred.in.ring[&ring == &c->up_rgb ? 1 : 0].cur) {
    const int frc = flush_deferred(c);
    if (frc < 0) return frc;
  }
  UpSlot& u = ring.s[next];
  if (u.last_seq) HIP_TRY(c, hipEventSynchronize(c->frame_done[u.last_seq % 8]));  // this mark or a later one of the same stream
  if (u.copied_rec) HIP_TRY(c, hipEventSynchronize(u.copied));
  if (bytes > u.cap) {
    u.cap = 0;
    HIP_TRY(c, pinned_free(c, u.h));
    HIP_TRY(c, dev_free(c, u.d));
    HIP_TRY(c, pinned_alloc(c, u.h, bytes));
    HIP_TRY(c, dev_alloc(c, u.d, bytes));
    if (!u.copied) HIP_TRY(c, event_new(c, u.copied, false));
    u.cap = bytes;
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
  HIP_TRY(c, pinned_alloc(c, c->h_peek, 64 * sizeof(int)));
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
  if (!c->frame_done[7])  // created in order: the last one says that all exist
    for (hipEvent_t& e : c->frame_done) if (!e) HIP_TRY(c, event_new(c, e, false));
  const bool lazy = c->ps.last_frame_lazy && c->ps.npend;  // the frame's integration is not enqueued yet (launch_pending)
  if (c->peek_enabled) {
    if (!c->peek_done[7])
      for (hipEvent_t& e : c->peek_done) if (!e) HIP_TRY(c, event_new(c, e, false));
    if (lazy) {
      // The report of a pipelined frame is written behind its integration, by launch_pending; until then the mark does not
      // exist for the peeks (they fall back to an older one and say how many frames behind it is).  A report launched here would
      // sit behind the integration of an EARLIER frame only, and an event on the front stream says nothing about it at all.
      c->peek_seq[seq % 8] = 0;
      c->ps.pendq[c->ps.npend - 1].report_seq = seq;
    } else if (const int rc = post_report(c, seq, c->stream)) {
      return rc;
    }
  }
  if (used[0] || used[1]) {
    // the raw images of a pipelined frame are read by its front half, on the front stream (its integration reads the cleaned copy)
    HIP_TRY(c, hipEventRecord(c->frame_done[seq % 8], lazy ? c->ps.stream_front : c->stream));
    for (UpSlot* u : used) if (u) u->last_seq = seq;
  }
  return MRH_OK;
}
}  // namespace
