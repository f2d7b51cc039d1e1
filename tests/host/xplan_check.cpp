// Stand-alone check of mrhash_amd/csrc/mrh_xplan.h — who sends what to whom in the halo exchange, the sub-map merge and the mesh
// gather — on any CPU: no GPU, no HIP, no RCCL.  tests/test_xplan.py builds it with AddressSanitizer + UBSan and expects exit status 0.
//
// For every world size 1 .. 8, with and without the self-loop, for each exchange (the gather with every rank as root) and a set of
// count patterns it builds the plan of EVERY rank and plays the group through: the sends of a to b against the receives of b from a,
// in order, as RCCL matches them, each delivered with memcpy between per-rank byte buffers whose bytes say where they came from.
#include "mrh_xplan.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

namespace {

enum Kind { kHalo, kMerge, kGather };
const char* const kKindName[] = {"halo", "merge", "gather"};
constexpr uint64_t kRec = 24;             // bytes of a block record here (any size does)
constexpr uint64_t kUnit[2] = {20, 36};  // gather: bytes of a block's metadata (4-byte aligned only, as in the library) and of a triangle
constexpr int kAnyDest = 8;               // halo: the same records go to everybody

struct Case {
  Kind kind; int world; bool self; int root; std::string pattern;
  std::vector<uint64_t> counts;  // halo [world], merge [src * world + dest], gather [2 * rank + stream]
};

int failures = 0;

void fail(const Case& k, const char* fmt, ...) {
  if (++failures > 40) return;
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  fprintf(stderr, "FAIL %s world %d self-loop %d root %d counts %s: %s\n", kKindName[k.kind], k.world, (int) k.self, k.root, k.pattern.c_str(), buf);
}

int streams(const Case& k) { return k.kind == kGather ? 2 : 1; }
uint64_t unit(const Case& k, const int s) { return k.kind == kGather ? kUnit[s] : kRec; }

// what `dst` is to consume from `src` in stream s, by the exchange's definition (not by the plan): byte j says (src, dst, s, j)
std::vector<uint8_t> payload(const Case& k, const int src, const int dst, const int s) {
  uint64_t n = 0;
  if (k.kind == kHalo) n = k.counts[src];
  if (k.kind == kMerge) n = k.counts[(size_t) src * k.world + dst];
  if (k.kind == kGather && dst == k.root) n = k.counts[2 * (size_t) src + s];
  const unsigned tag = ((unsigned) src * 9u + (unsigned) (k.kind == kHalo ? kAnyDest : dst)) * 2u + (unsigned) s;  // < 256, one per (src, dst, s)
  std::vector<uint8_t> v(n * unit(k, s));
  for (size_t j = 0; j < v.size(); j++) v[j] = (uint8_t) (tag + j * 131u + (j >> 8));
  return v;
}

// what a rank packed on the send side of stream s
std::vector<uint8_t> packed(const Case& k, const int src, const int s) {
  if (k.kind == kHalo) return payload(k, src, kAnyDest, 0);
  if (k.kind == kGather) return payload(k, src, k.root, s);
  std::vector<uint8_t> v;
  for (int dst = 0; dst < k.world; dst++) { const std::vector<uint8_t> p = payload(k, src, dst, 0); v.insert(v.end(), p.begin(), p.end()); }
  return v;
}

XPlan plan_of(const Case& k, const int rank) {
  if (k.kind == kHalo) return xplan_halo(k.world, rank, k.self, k.counts.data(), kRec);
  if (k.kind == kMerge) return xplan_merge(k.world, rank, k.self, k.counts.data(), kRec);
  return xplan_gather(k.world, rank, k.self, k.root, k.counts.data(), kUnit);
}

struct Rank {
  XPlan plan;
  std::vector<uint8_t> send[2], recv;
};

void run_case(const Case& k) {
  const int world = k.world, ns = streams(k);
  std::vector<Rank> ranks((size_t) world);
  for (int r = 0; r < world; r++) {
    ranks[r].plan = plan_of(k, r);
    for (int s = 0; s < ns; s++) ranks[r].send[s] = packed(k, r, s);
    ranks[r].recv.assign(ranks[r].plan.recv_bytes, 0xEE);
  }
  for (int r = 0; r < world; r++) {
    const XPlan& p = ranks[r].plan;
    const bool consumer = k.kind != kGather || r == k.root;
    const XOwn own = k.self && consumer ? kOwnLooped : k.kind == kMerge ? kOwnInPlace : k.kind == kGather && consumer ? kOwnCopied : kOwnAbsent;
    if (p.own != own) fail(k, "rank %d: own part handled as %d, expected %d", r, (int) p.own, (int) own);
    // 2. no zero-size call; 3. receive ranges disjoint and inside the room asked for; 4. send ranges inside what was packed
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (const XPart& x : p.parts) {
      if (x.bytes == 0) fail(k, "rank %d: a zero-size %s, peer %d", r, x.send ? "send" : "receive", x.peer);
      if (x.stream < 0 || x.stream >= ns || x.peer < 0 || x.peer >= world) { fail(k, "rank %d: part with stream %d, peer %d", r, x.stream, x.peer); continue; }
      if (x.peer == r && !k.self) fail(k, "rank %d: a part to itself without the self-loop", r);
      if (x.send && x.off + x.bytes > ranks[r].send[x.stream].size())
        fail(k, "rank %d: send [%llu, +%llu) of stream %d past the %zu bytes packed", r, (unsigned long long) x.off, (unsigned long long) x.bytes, x.stream, ranks[r].send[x.stream].size());
      if (!x.send) ranges.push_back({p.area[x.stream] + x.off, x.bytes});
    }
    for (int s = 0; s < ns && p.own == kOwnCopied; s++)
      if (p.own_sent[s].bytes) ranges.push_back({p.area[s] + p.seg[s][r].off, p.own_sent[s].bytes});
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 0; i < ranges.size(); i++) {
      if (ranges[i].first + ranges[i].second > p.recv_bytes)
        fail(k, "rank %d: receive [%llu, +%llu) past the room of %llu bytes", r, (unsigned long long) ranges[i].first, (unsigned long long) ranges[i].second, (unsigned long long) p.recv_bytes);
      if (i && ranges[i - 1].first + ranges[i - 1].second > ranges[i].first)
        fail(k, "rank %d: receive ranges at %llu and %llu overlap", r, (unsigned long long) ranges[i - 1].first, (unsigned long long) ranges[i].first);
    }
    // 5. the gather's triangle area: behind the metadata, on a 256-byte boundary
    if (k.kind == kGather && consumer && (p.area[1] % 256 != 0 || p.area[1] < p.area[0] + p.area_bytes[0]))
      fail(k, "rank %d: triangle area at %llu, metadata of %llu bytes", r, (unsigned long long) p.area[1], (unsigned long long) p.area_bytes[0]);
  }
  // 1. sends match receives, pair by pair and in order; 6. delivery
  for (int a = 0; a < world; a++)
    for (int b = 0; b < world; b++) {
      std::vector<XPart> sends, recvs;
      for (const XPart& x : ranks[a].plan.parts) if (x.send && x.peer == b) sends.push_back(x);
      for (const XPart& x : ranks[b].plan.parts) if (!x.send && x.peer == a) recvs.push_back(x);
      if (sends.size() != recvs.size()) { fail(k, "%d sends %zu parts to %d, which posts %zu receives: a hang", a, sends.size(), b, recvs.size()); continue; }
      for (size_t i = 0; i < sends.size(); i++) {
        const XPart& sx = sends[i];
        const XPart& rx = recvs[i];
        if (sx.bytes != rx.bytes) { fail(k, "part %zu of %d -> %d: %llu bytes sent, %llu expected", i, a, b, (unsigned long long) sx.bytes, (unsigned long long) rx.bytes); continue; }
        const uint64_t to = ranks[b].plan.area[rx.stream] + rx.off;
        if (sx.off + sx.bytes <= ranks[a].send[sx.stream].size() && to + rx.bytes <= ranks[b].recv.size())
          memcpy(ranks[b].recv.data() + to, ranks[a].send[sx.stream].data() + sx.off, sx.bytes);
      }
    }
  // 6. every consumer segment holds exactly its source's bytes, and the segments with room tile their area in rank order
  uint64_t sum_out = 0, sum_in = 0;
  for (int r = 0; r < world; r++) {
    Rank& me = ranks[r];
    const XPlan& p = me.plan;
    sum_out += p.bytes_out; sum_in += p.bytes_in;
    if (k.kind == kGather && r != k.root) continue;
    for (int s = 0; s < ns; s++) {
      if (p.own == kOwnCopied && p.own_sent[s].bytes && p.area[s] + p.seg[s][r].off + p.own_sent[s].bytes <= me.recv.size() && p.own_sent[s].off + p.own_sent[s].bytes <= me.send[s].size())
        memcpy(me.recv.data() + p.area[s] + p.seg[s][r].off, me.send[s].data() + p.own_sent[s].off, p.own_sent[s].bytes);
      if ((int) p.seg[s].size() != world) { fail(k, "rank %d: %zu segments in stream %d", r, p.seg[s].size(), s); continue; }
      uint64_t at = 0;
      for (int src = 0; src < world; src++) {
        const XSeg& g = p.seg[s][src];
        const std::vector<uint8_t> want = payload(k, src, r, s);
        const bool has_room = src != r || p.own == kOwnLooped || p.own == kOwnCopied;
        if (g.off != at) fail(k, "rank %d: segment of source %d in stream %d at %llu, the one before ends at %llu", r, src, s, (unsigned long long) g.off, (unsigned long long) at);
        if (has_room) at += g.bytes;
        if (src == r && p.own == kOwnAbsent) continue;  // not consumed
        if (g.bytes != want.size()) { fail(k, "rank %d: %llu bytes from source %d in stream %d, %zu expected", r, (unsigned long long) g.bytes, src, s, want.size()); continue; }
        const std::vector<uint8_t>& buf = has_room ? me.recv : me.send[s];
        const uint64_t from = has_room ? p.area[s] + g.off : p.own_sent[s].off;
        if (!has_room && p.own_sent[s].bytes != g.bytes) fail(k, "rank %d: own part of %llu bytes on the send side, %llu in its segment", r, (unsigned long long) p.own_sent[s].bytes, (unsigned long long) g.bytes);
        if (from + g.bytes > buf.size()) fail(k, "rank %d: segment of source %d in stream %d lies past its buffer", r, src, s);
        else if (g.bytes && memcmp(buf.data() + from, want.data(), g.bytes) != 0) fail(k, "rank %d: the bytes from source %d in stream %d are not that source's", r, src, s);
      }
      if (at != p.area_bytes[s]) fail(k, "rank %d: the segments of stream %d end at %llu, the area holds %llu", r, s, (unsigned long long) at, (unsigned long long) p.area_bytes[s]);
    }
    if (p.area[ns - 1] + p.area_bytes[ns - 1] != p.recv_bytes) fail(k, "rank %d: room for %llu bytes, the areas end at %llu", r, (unsigned long long) p.recv_bytes, (unsigned long long) (p.area[ns - 1] + p.area_bytes[ns - 1]));
  }
  // 7. byte totals balance
  if (!k.self && sum_out != sum_in) fail(k, "%llu bytes out over all ranks, %llu in", (unsigned long long) sum_out, (unsigned long long) sum_in);
  if (k.kind == kMerge)
    for (int r = 0; r < world; r++) {
      const XPlan& p = ranks[r].plan;
      uint64_t row = 0, col = 0;
      for (int o = 0; o < world; o++) { row += k.counts[(size_t) r * world + o]; col += k.counts[(size_t) o * world + r]; }
      const uint64_t own = k.counts[(size_t) r * world + r];
      if (p.kept != own || p.sent != row - own || p.received != col - own || p.bytes_out != p.sent * kRec || p.bytes_in != p.received * kRec)
        fail(k, "rank %d: sent %llu received %llu kept %llu, the matrix says %llu %llu %llu", r, (unsigned long long) p.sent, (unsigned long long) p.received,
             (unsigned long long) p.kept, (unsigned long long) (row - own), (unsigned long long) (col - own), (unsigned long long) own);
    }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;  // the fixed seed
uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

// does count i of the exchange's agreed counts belong to rank r (as source or, in the merge, as destination)?
bool touches(const Kind kind, const int world, const size_t i, const int r) {
  if (kind == kHalo) return (int) i == r;
  if (kind == kGather) return (int) (i / 2) == r;
  return (int) (i / world) == r || (int) (i % world) == r;
}
bool sent_by(const Kind kind, const int world, const size_t i, const int r) { return kind == kMerge ? (int) (i / world) == r : touches(kind, world, i, r); }

int cases = 0;

void run_patterns(Case k) {
  const size_t n = k.kind == kHalo ? (size_t) k.world : k.kind == kMerge ? (size_t) k.world * k.world : 2 * (size_t) k.world;
  auto go = [&](const std::string& name) { k.pattern = name; run_case(k); cases++; };
  k.counts.assign(n, 0);
  go("all zero");
  for (int rep = 0; rep < 2; rep++) {
    for (size_t i = 0; i < n; i++) k.counts[i] = 1 + rng() % 47;
    go("random");
    for (size_t i = 0; i < n; i++) k.counts[i] = rng() % 2 ? 0 : 1 + rng() % 47;
    go("random, half of them zero");
  }
  for (int r = 0; r < k.world; r++) {
    for (size_t i = 0; i < n; i++) k.counts[i] = touches(k.kind, k.world, i, r) ? 0 : 1 + rng() % 47;
    go("rank " + std::to_string(r) + " has an empty map");
    for (size_t i = 0; i < n; i++) k.counts[i] = sent_by(k.kind, k.world, i, r) ? 1 + rng() % 47 : 0;
    go("rank " + std::to_string(r) + " holds everything");
  }
}

}  // namespace

int main() {
  for (int world = 1; world <= 8; world++)
    for (int self = 0; self < 2; self++)
      for (int kind = kHalo; kind <= kGather; kind++)
        for (int root = 0; root < (kind == kGather ? world : 1); root++) run_patterns(Case{(Kind) kind, world, self != 0, root, "", {}});
  printf("xplan_check: %d cases, %d failures\n", cases, failures);
  printf("xplan_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
