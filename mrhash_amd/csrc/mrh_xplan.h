// mrh_xplan.h — who sends how many bytes from where, and who receives them where, in the three multi-GPU exchanges of mrh_comm.h.
// Plain host C++17, no HIP or RCCL header, nothing of the library's namespace: tests/host/xplan_check.cpp compiles it alone, builds
// the plan of every rank of a 1 .. 8-rank group on the CPU and delivers the parts with memcpy (ncclSend / ncclRecv have no time
// limit: a send without its receive is a hang, a size mismatch is corruption).
//
// Every rank builds its plan from the SAME agreed counts, so what one plans to send is what its peer plans to receive.  A stream is
// one kind of data with a send side and a receive area of its own (halo and merge: the block records; gather: 0 the block metadata,
// 1 the triangles).  Offsets are bytes from the base of that side.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

struct XPart { int peer; bool send; int stream; uint64_t off, bytes; };  // one ncclSend / ncclRecv
struct XSeg { uint64_t off, bytes; };

enum XOwn {        // the rank's own part:
  kOwnAbsent,      //   has no room in the receive areas and is not consumed (halo; a gather's non-root)
  kOwnInPlace,     //   has no room there, the consumer reads it from the send side at own_sent[0] (merge)
  kOwnCopied,      //   has room there, no part carries it: the caller copies own_sent[s] to seg[s][rank] on the device (gather's root)
  kOwnLooped,      //   has room there and travels as parts of the plan, from this rank to itself (the self-loop)
};

struct XPlan {
  std::vector<XPart> parts;  // in the order they are issued: RCCL matches the sends and receives of a pair in that order
  // seg[s][src]: what this rank consumes from source src, and where in stream s's receive area.  An own part without room there
  // keeps its size and a zero-width place (kOwnInPlace reads it elsewhere, kOwnAbsent does not read it)
  std::vector<XSeg> seg[2];
  uint64_t area[2] = {0, 0};        // where each stream's receive area begins in the receive buffer
  uint64_t area_bytes[2] = {0, 0};  // and how much of it the segments with room fill
  uint64_t recv_bytes = 0;          // room the receive buffer needs
  XOwn own = kOwnAbsent;
  XSeg own_sent[2] = {{0, 0}, {0, 0}};  // the own part on the send side
  uint64_t bytes_out = 0, bytes_in = 0;       // PhaseClock::finish: what crosses a link (with the self-loop, the halo's bytes_in counts the own part too)
  uint64_t sent = 0, received = 0, kept = 0;  // merge, in records: to other ranks, from other ranks, the own part
};

// The one protocol behind the three exchanges.  bytes(s, src, dst): what src ships to dst in stream s, from the agreed counts;
// at(s, dst): where this rank's part for dst lies on its send side.  Per peer, in rank order: its sends, then its receives; the
// sources' segments lie in rank order in each receive area, the own one with room there only if `own` says so.
template <class Bytes, class At>
XPlan xplan_build(const int world, const int rank, const bool self, const int streams, const XOwn own, Bytes bytes, At at) {
  XPlan p;
  p.own = own;
  // A zero-size part is neither sent nor received: both sides decide that here, from the same agreed number, and nowhere else.
  auto part = [&](const int peer, const bool send, const int s, const uint64_t off, const uint64_t n) {
    if (n) p.parts.push_back({peer, send, s, off, n});
  };
  for (int s = 0; s < streams; s++) {
    // the gather's triangle area starts on a 256-byte boundary behind the metadata: the run merge reads it with 16-byte loads
    // (k_permute_runs), and the metadata's end is only 4-byte aligned
    if (s) p.area[s] = (p.area[s - 1] + p.area_bytes[s - 1] + 255) & ~(uint64_t) 255;
    for (int src = 0; src < world; src++) {
      p.seg[s].push_back({p.area_bytes[s], bytes(s, src, rank)});
      if (src != rank || own == kOwnLooped || own == kOwnCopied) p.area_bytes[s] += bytes(s, src, rank);
    }
    p.recv_bytes = p.area[s] + p.area_bytes[s];
    p.own_sent[s] = {at(s, rank), bytes(s, rank, rank)};
  }
  for (int r = 0; r < world; r++) {
    if (r == rank && !self) continue;
    for (int s = 0; s < streams; s++) part(r, true, s, at(s, r), bytes(s, rank, r));
    for (int s = 0; s < streams; s++) part(r, false, s, p.seg[s][r].off, p.seg[s][r].bytes);
    if (r != rank)
      for (int s = 0; s < streams; s++) { p.bytes_out += bytes(s, rank, r); p.bytes_in += bytes(s, r, rank); }
  }
  return p;
}

// halo: every rank sends ALL its records (counts[rank] of `rec` bytes, at the base of its send side) to every other rank
inline XPlan xplan_halo(const int world, const int rank, const bool self, const uint64_t* counts, const uint64_t rec) {
  XPlan p = xplan_build(world, rank, self, 1, self ? kOwnLooped : kOwnAbsent, [&](int, int src, int) { return counts[src] * rec; },
                        [](int, int) { return (uint64_t) 0; });
  if (self) p.bytes_in += p.own_sent[0].bytes;  // what the exchange has always reported: everything that arrived
  return p;
}

// merge: matrix[src * world + dest] records go from src to dest; a rank's send side holds its row, the parts in destination order
inline XPlan xplan_merge(const int world, const int rank, const bool self, const uint64_t* matrix, const uint64_t rec) {
  std::vector<uint64_t> row_off((size_t) world, 0);
  for (int r = 1; r < world; r++) row_off[r] = row_off[r - 1] + matrix[(size_t) rank * world + r - 1] * rec;
  XPlan p = xplan_build(world, rank, self, 1, self ? kOwnLooped : kOwnInPlace, [&](int, int src, int dst) { return matrix[(size_t) src * world + dst] * rec; },
                        [&](int, int dst) { return row_off[dst]; });
  p.sent = p.bytes_out / rec; p.received = p.bytes_in / rec; p.kept = p.own_sent[0].bytes / rec;
  return p;
}

// gather: counts[2 * r + s] units of unit[s] bytes go from rank r to root in stream s; a rank's send sides hold just its own part
inline XPlan xplan_gather(const int world, const int rank, const bool self, const int root, const uint64_t* counts, const uint64_t unit[2]) {
  return xplan_build(world, rank, self, 2, rank != root ? kOwnAbsent : self ? kOwnLooped : kOwnCopied,
                     [&](int s, int src, int dst) { return dst == root ? counts[2 * (size_t) src + s] * unit[s] : (uint64_t) 0; },
                     [](int, int) { return (uint64_t) 0; });
}

}  // namespace
