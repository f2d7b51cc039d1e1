// mrh_extract.h — the host side of mesh extraction behind the C ABI: marching cubes over the compacted block list
// (mrh_extract_triangles: kernels in mrh_mc.h, the block sort's in mrh_mc.h / mrh_sort.h), the post-process
// MeshExtractor::processTriangles on the device (kernels in mrh_mesh.h) or restated on the host, the read-back of V / C / F,
// the merge mode and the triangle-run calls of the sharded extraction.  Included by mrh_capi.hip, same translation unit: it
// needs the context's internals (mrh_ctx, HIP_TRY, regrow, arena_layout, compact_all, ensure_h_mc, the copy pool's widen_* calls).
#pragma once

namespace {

struct KeyHash3 {
  size_t operator()(const std::array<uint64_t, 3>& k) const {
    uint64_t h = k[0] * 0x9E3779B97F4A7C15ull;
    h ^= (k[1] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2));
    h ^= (k[2] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2));
    return (size_t) h;
  }
};
struct FaceHash {
  size_t operator()(const std::array<int32_t, 3>& f) const {
    uint64_t h = (uint64_t) (uint32_t) f[0] * 0x9E3779B97F4A7C15ull;
    h ^= ((uint64_t) (uint32_t) f[1] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2));
    h ^= ((uint64_t) (uint32_t) f[2] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2));
    return (size_t) h;
  }
};

// MeshExtractor::processTriangles for a single extraction (mesh_extractor.cpp:9-76):
// soup -> vertex merge (exact bit pattern, or floor(v/eps) cells; first occurrence keeps index and colour)
// -> drop degenerate faces -> drop repeated faces keeping the first.
void widen_quiesce();
void process_triangles(mrh_ctx* c) {
  const size_t nt = c->tris.size();
  widen_quiesce();  // a helper of the last extraction's widening may still be writing the arrays that are about to be replaced
  c->V.clear(); c->C.clear(); c->F.clear();
  if (nt == 0) return;
  std::vector<double> V, C;
  std::vector<int32_t> F;
  const double eps = (double) c->p.vertices_merging_threshold;
  const double inv_eps = eps != 0.0 ? 1.0 / eps : 0.0;
  std::unordered_map<std::array<uint64_t, 3>, int32_t, KeyHash3> vmap;
  vmap.reserve(nt * 3);
  std::vector<int32_t> faces(nt * 3);
  for (size_t i = 0; i < nt; i++)
    for (int k = 0; k < 3; k++) {
      const mrh_vertex& v = c->tris[i].v[k];
      const double p[3] = {(double) v.p[0], (double) v.p[1], (double) v.p[2]};
      std::array<uint64_t, 3> key;
      for (int a = 0; a < 3; a++) {
        if (eps == 0.0) memcpy(&key[a], &p[a], 8);
        else key[a] = (uint64_t) (uint32_t) mesh_cell(std::floor(p[a] * inv_eps));
      }
      const bool has_nan = p[0] != p[0] || p[1] != p[1] || p[2] != p[2];  // never equal to anything (Vector3dEqual)
      auto it = has_nan ? vmap.end() : vmap.find(key);
      int32_t idx;
      if (it != vmap.end()) idx = it->second;
      else {
        idx = (int32_t) (V.size() / 3);
        if (!has_nan) vmap.emplace(key, idx);
        V.insert(V.end(), {p[0], p[1], p[2]});
        C.insert(C.end(), {(double) v.c[0], (double) v.c[1], (double) v.c[2]});
      }
      faces[i * 3 + k] = idx;
    }
  std::unordered_map<std::array<int32_t, 3>, char, FaceHash> seen;
  seen.reserve(nt);
  for (size_t i = 0; i < nt; i++) {
    const std::array<int32_t, 3> f = {faces[i * 3], faces[i * 3 + 1], faces[i * 3 + 2]};
    if (f[0] == f[1] || f[0] == f[2] || f[1] == f[2]) continue;
    if (!seen.emplace(f, 1).second) continue;
    F.insert(F.end(), {f[0], f[1], f[2]});
  }
  c->V.assign(V.data(), V.data() + V.size());
  c->C.assign(C.data(), C.data() + C.size());
  c->F.assign(F.data(), F.data() + F.size());
}

// Results leave the device through a copy KERNEL writing pinned host memory, not through hipMemcpyAsync: the runtime's choice
// of SDMA engine for a stream is not stable within a process — the second context of a process (and every later one) moved its
// V / C / F at 22 GB/s instead of 54 (tools/dbg_extract2.py: 30 MB in 1.24 vs 0.56 ms; tools/micro/d2h_streams.hip and
// d2h_second_alloc.hip rule out the host buffer and the stream order in isolation) while 16-byte stores of a kernel reach 53-54 GB/s
// every time.  It also lets the copy read its sizes on the device: no host round trip between the post-process and the copy.
//   part p copies ceil(min(count[p], cap[p]) * unit[p] / 16) 16-byte words (both sides are padded to a multiple of 16 bytes)
struct CopyOut {
  const uint4* src[3];
  uint4* dst[3];
  const u64* count[3];  // device: elements of part p (nullptr: use fixed[p])
  u64 fixed[3], cap[3];
  u32 unit[3];          // bytes per element
};
__global__ __launch_bounds__(256) void k_copy_out(const CopyOut a) {
#pragma unroll 1
  for (int p = 0; p < 3; p++) {
    if (!a.dst[p]) continue;
    u64 n = a.count[p] ? *a.count[p] : a.fixed[p];
    if (n > a.cap[p]) n = a.cap[p];
    const size_t n16 = (size_t) ((n * a.unit[p] + 15) / 16);
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t) gridDim.x * 256) a.dst[p][i] = a.src[p][i];
  }
}
// V / C / F of an extraction are 48 B per vertex + 12 B per face as the reference hands them out (Eigen::MatrixXd / MatrixXi,
// geowrapper.h:91-93) — 30 MB at the driver's workload, 0.56 ms of a 1.3 ms extraction at the link's 54 GB/s.  The vertex
// arithmetic is fp32 (mesh_extractor.cu:6-36), so the doubles carry no more than the floats they are widened from: V and C cross the
// link as fp32 (24 B per vertex) into pinned staging, in 64 KiB chunks that each raise a flag word when they have landed, and
// host threads widen chunk after chunk into the caller-visible double arrays while the following chunks and the faces are still
// on the link (widen_from_staging below; (double) (float) is exact, the arrays are the same bytes as before).  F goes straight
// to its final buffer.  Few workgroups, each walking its chunks in order: the link is the bottleneck, and chunks must COMPLETE in
// order for the host to overlap, not all at the end.
constexpr u32 kStageChunk = 64u << 10;            // bytes
constexpr u32 kStageWords = kStageChunk / 16;     // uint4 per chunk
constexpr u32 kStageHdrWords = 16;                // u32 words of stage_ctl before the first flag
struct StageOut {
  const uint4* src[3];   // device: V32, C32, F
  uint4* dst[3];         // pinned: V32 staging, C32 staging, F
  const u64* totals;     // device: [0] vertices, [1] faces
  u64 cap_v, cap_f;      // elements the destinations hold
  u64* hdr;              // pinned: [0] vertices, [1] faces, [2] epoch (written last)
  u32* flags;            // pinned: chunk c of V32 -> flags[c], of C32 -> flags[flag_stride + c]
  u32 flag_stride;
  u32 epoch;
  // workgroups copy_wgs .. gridDim.x - 1 do not copy: they refill the post-process's index tables with "empty" for the next
  // extraction (the link keeps the copying workgroups busy for 0.35 ms; the fills used to cost 2 x 9 us up front)
  u32 copy_wgs;
  u32* clear;
  size_t clear_words;
};
__global__ __launch_bounds__(256) void k_stage_out(const StageOut a) {
  if (blockIdx.x >= a.copy_wgs) {
    const size_t n4 = a.clear_words / 4, stride = (size_t) (gridDim.x - a.copy_wgs) * 256;
    uint4* c4 = (uint4*) a.clear;
    const uint4 ff = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    for (size_t i = (size_t) (blockIdx.x - a.copy_wgs) * 256 + threadIdx.x; i < n4; i += stride) c4[i] = ff;
    if (blockIdx.x == a.copy_wgs && threadIdx.x < (a.clear_words & 3)) a.clear[n4 * 4 + threadIdx.x] = 0xFFFFFFFFu;
    return;
  }
  const u64 nv = a.totals[0], nf = a.totals[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.hdr[0] = nv; a.hdr[1] = nf;
    __hip_atomic_store(&a.hdr[2], (u64) a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (nv > a.cap_v || nf > a.cap_f) return;  // uniform: the host grows the buffers and launches again
  const size_t w16[3] = {(size_t) ((nv * 12 + 15) / 16), (size_t) ((nv * 12 + 15) / 16), (size_t) ((nf * 12 + 15) / 16)};
  const u32 nch[3] = {(u32) ((w16[0] + kStageWords - 1) / kStageWords), (u32) ((w16[1] + kStageWords - 1) / kStageWords),
                      (u32) ((w16[2] + kStageWords - 1) / kStageWords)};
  const u32 total = nch[0] + nch[1] + nch[2];
  for (u32 ch = blockIdx.x; ch < total; ch += a.copy_wgs) {  // uniform per workgroup
    const int p = ch < nch[0] ? 0 : (ch < nch[0] + nch[1] ? 1 : 2);
    const u32 lc = ch - (p > 0 ? nch[0] : 0u) - (p > 1 ? nch[1] : 0u);
    const size_t lo = (size_t) lc * kStageWords, hi = lo + kStageWords < w16[p] ? lo + kStageWords : w16[p];
    const uint4* __restrict__ src = a.src[p];
    uint4* __restrict__ dst = a.dst[p];
    uint4 r[kStageWords / 256];
#pragma unroll
    for (u32 k = 0; k < kStageWords / 256; k++) {
      const size_t i = lo + k * 256 + threadIdx.x;
      if (i < hi) r[k] = src[i];
    }
#pragma unroll
    for (u32 k = 0; k < kStageWords / 256; k++) {
      const size_t i = lo + k * 256 + threadIdx.x;
      if (i < hi) dst[i] = r[k];
    }
    if (p < 2) {
      // (the fence is needed — plain stores to the pinned buffer sit in the XCD's L2: with "stores acknowledged, then the flag" alone
      // tools/stress_extract.py read a torn mesh within 50 extractions — and it is not what the kernel waits for: write-through stores
      // (sc0 sc1) + acknowledgement + flag, no fence, gave the same 0.83-0.87 ms per extraction; profiles/r06/ab_stage_out_fences.txt)
      __threadfence_system();
      __syncthreads();
      if (threadIdx.x == 0) __hip_atomic_store(&a.flags[(p ? a.flag_stride : 0u) + lc], a.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
// host side of the above (defined with the copy pool further down): widens nfloat floats of each of the two staging parts into
// dst[0] / dst[1], chunk by chunk as flags[part][chunk] reaches `epoch` (flags == nullptr: everything has landed already).
// `drained(arg)` tells whether the stream has run dry (then a missing flag means a failed launch).  Returns false if it gave up.
bool widen_from_staging(double* const dst[2], const float* const src[2], const volatile u32* const flags[2], u32 epoch, size_t nfloat,
                        bool (*drained)(void*), void* arg);
void widen_prewake();
uint64_t widen_redone();

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the soup buffer: grow-only, owned by the context, valid until the next extraction
int ensure_soup(mrh_ctx* c, size_t n) {
  if (n <= c->soup_cap) return MRH_OK;
  return regrow(c, c->d_soup, c->soup_cap, n + n / 8, (n + n / 8) * sizeof(mrh_triangle) + 16);  // + 16: k_copy_out reads whole 16-byte words
}

// ---- the post-process on the device: MeshExtractor::processTriangles (mrh_mesh.h) and the way out of V / C / F ------------------

// The fp32 staging for nv vertices and nf faces (+ 4: the copy kernels read whole 16-byte words), and one flag word per chunk
// the staging holds.  The post-process grows them to the mesh it found; the prewarm (mrh_ctx::prewarm_on) to the mesh it expects.
void size_mesh_staging(mrh_ctx* c, const size_t nv, const size_t nf) {
  c->V32.resize_discard(nv * 3 + 4); c->C32.resize_discard(nv * 3 + 4);
  c->F.resize_discard(nf * 3 + 4);
  c->stage_ctl.resize_discard(kStageHdrWords + 2 * ((std::min(c->V32.cap, c->C32.cap) * 4 + kStageChunk - 1) / kStageChunk + 2));
}

// see mrh_ctx::prewarm_on
void prewarm_maybe(mrh_ctx* c) {
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

// the switches of the post-process, read once per call
struct MeshOpts {
  bool dbg;         // MRH_DEBUG: the phase line on stderr
  bool fill;        // MRH_MESH_FILL=1: fill the index tables even where the last extraction left them empty (A/B)
  bool d2h_memcpy;  // MRH_D2H_MEMCPY=1: hipMemcpyAsync instead of the copy kernel on the f64 link (A/B)
  int stage_wgs;    // MRH_STAGE_WGS: copying workgroups of k_stage_out (default 64)
};
MeshOpts read_mesh_opts() {
  const char* wgs = getenv("MRH_STAGE_WGS");
  return MeshOpts{getenv("MRH_DEBUG") != nullptr, getenv("MRH_MESH_FILL") != nullptr, getenv("MRH_D2H_MEMCPY") != nullptr, wgs ? std::max(1, atoi(wgs)) : 64};
}

// what the post-process kernels leave on the device for the read-back
struct MeshLink {
  u32 n;                            // soup vertices
  void *dV, *dC; int* dF;           // V and C: doubles with f64_link, floats otherwise
  u64* d_totals;                    // [0] vertices, [1] faces
  u32* tables; size_t table_words;  // the two index tables (the head of arena slot 1): the staged read-back leaves them empty again
};

// Arena set-up and the eight launches of the post-process: soup -> V / C / F and their totals, all on the device.
int mesh_link_kernels(mrh_ctx* c, const mrh_triangle* d_tris, const size_t nt, const MeshOpts& o, MeshLink* L) {
  hipStream_t s = c->stream;
  const u32 n = (u32) (nt * 3), ntr = (u32) nt;
  const double eps = (double) c->p.vertices_merging_threshold;
  const double inv_eps = eps != 0.0 ? 1.0 / eps : 0.0;
  const u32 cap = (u32) next_pow2((uint64_t) n * 2);  // load factor <= 1/2
  const u32 fcap = (u32) next_pow2((uint64_t) ntr * 2);
  const u32 vtiles = (n + kMeshTile - 1) / kMeshTile, ftiles = (ntr + 255) / 256;
  u32 *table, *ftable, *rep, *vloc, *corner, *floc, *tcount, *toff, *fcount, *foff;
  u64* d_totals;
  size_t clear_words = 0;
  MeshScratch m;
  int rc = arena_layout(c, 1, &m, [&](MeshScratch& a) {
    // The two index tables come first, so that they lie where the last extraction's lay: that extraction's read-back kernel left
    // them empty again (k_stage_out's extra workgroups clear them while the link is busy), and the two fills — 24 MB at the
    // driver's workload, ahead of the vertex and of the face kernels — are only needed when the scratch moved or grew.
    table = a.take<u32>(cap);
    ftable = a.take<u32>(fcap);
    clear_words = a.used / 4;
    rep = a.take<u32>(n);   vloc = a.take<u32>(n);   corner = a.take<u32>(n);
    floc = a.take<u32>(n);  // faces (nt <= n)
    tcount = a.take<u32>(vtiles);  toff = a.take<u32>(vtiles);  // first occurrences per vertex tile, and their scan
    fcount = a.take<u32>(ftiles);  foff = a.take<u32>(ftiles);  // kept faces per face tile
    d_totals = a.take<u64>(2);
  });
  if (rc) return rc;
  const bool tables_clean = !c->f64_link && c->mesh_clean_base == m.base && c->mesh_clean_words >= clear_words && !o.fill;
  c->mesh_clean_words = 0;  // dirty from here on, until a clear is enqueued
  const u32 gv = (n + 255) / 256, gf = (ntr + 255) / 256;
  const float* soup = (const float*) d_tris;
  if ((rc = ensure_h_mc(c))) return rc;
  const bool f64 = c->f64_link;
  if (!f64) widen_prewake();  // the helper threads are awake and spinning by the time the first chunk lands
  // V, C (at most n vertices each) and the faces (at most nt) share slot 2, sized by those bounds: nothing of the
  // post-process waits for a count from the device
  void* vcf = nullptr;
  const size_t vbytes = ((size_t) n * 3 * (f64 ? sizeof(double) : sizeof(float)) + 16 + 255) & ~(size_t) 255;  // + 16: the copy kernels read whole 16-byte words
  if ((rc = arena_get(c, 2, 2 * vbytes + (size_t) ntr * 3 * sizeof(int) + 16, &vcf))) return rc;
  void *dV = vcf, *dC = (char*) vcf + vbytes;
  int* dF = (int*) ((char*) vcf + 2 * vbytes);
  // ---- vertices
  if (!tables_clean) HIP_TRY(c, hipMemsetAsync(m.base, 0xFF, clear_words * 4, s));
  k_mesh_vertex_insert<<<(n + kMeshTile - 1) / kMeshTile, kMeshTile, 0, s>>>(soup, n, eps, inv_eps, table, cap - 1, rep);
  k_mesh_vertex_rep<<<vtiles, kMeshTile, 0, s>>>(soup, n, eps, inv_eps, table, cap - 1, rep, vloc, tcount);
  k_tile_scan<<<1, 1024, 0, s>>>(tcount, vtiles, toff, d_totals);
  if (f64) k_mesh_emit_vertices<double><<<gv, 256, 0, s>>>(soup, rep, vloc, toff, n, (double*) dV, (double*) dC, corner);
  else k_mesh_emit_vertices<float><<<gv, 256, 0, s>>>(soup, rep, vloc, toff, n, (float*) dV, (float*) dC, corner);
  // ---- faces
  k_mesh_face_insert<<<gf, 256, 0, s>>>(corner, ntr, ftable, fcap - 1);
  k_mesh_face_keep<<<gf, 256, 0, s>>>(corner, ntr, ftable, fcap - 1, floc, fcount);
  k_tile_scan<<<1, 1024, 0, s>>>(fcount, ftiles, foff, d_totals + 1);
  k_mesh_emit_faces<<<gf, 256, 0, s>>>(corner, floc, foff, ntr, dF);
  *L = MeshLink{n, dV, dC, dF, d_totals, (u32*) m.base, clear_words};
  return MRH_OK;
}

// (Tried in round 4: V and C on a second stream as soon as the vertices are final, next to the face kernels.  The copy kernel and
// k_mesh_face_insert do not share the memory system gracefully — the insert's atomics ran 37 -> 240-450 us whether the copy had
// 1 024 or 128 workgroups — and the extraction took as long as before.)

// ---- MRH_MESH_F64_LINK=1, the round-3 way out: doubles over the link.  V, C, F go out behind the post-process without the host
// in between (k_copy_out reads the two totals on the device), into the buffers of the previous extraction; if they turn out too
// small (or not pinned) they grow and the copy runs again.
bool f64_pinned(const mrh_ctx* c, const MeshOpts& o) { return c->V.dev && c->C.dev && c->F.dev && !o.d2h_memcpy; }
hipError_t copy_out_f64(mrh_ctx* c, const MeshLink& L, const bool by_kernel, const size_t nv_known, const size_t nf_known) {
  hipStream_t s = c->stream;
  if (by_kernel) {
    CopyOut a;
    a.src[0] = (const uint4*) L.dV; a.dst[0] = (uint4*) c->V.dev; a.count[0] = L.d_totals; a.cap[0] = c->V.cap / 3; a.unit[0] = 24;
    a.src[1] = (const uint4*) L.dC; a.dst[1] = (uint4*) c->C.dev; a.count[1] = L.d_totals; a.cap[1] = c->C.cap / 3; a.unit[1] = 24;
    a.src[2] = (const uint4*) L.dF; a.dst[2] = (uint4*) c->F.dev; a.count[2] = L.d_totals + 1; a.cap[2] = c->F.cap / 3; a.unit[2] = 12;
    a.fixed[0] = a.fixed[1] = a.fixed[2] = 0;
    k_copy_out<<<1024, 256, 0, s>>>(a);
    return hipGetLastError();
  }
  hipError_t e = hipMemcpyAsync(c->V.data(), L.dV, nv_known * 3 * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->C.data(), L.dC, nv_known * 3 * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && nf_known) e = hipMemcpyAsync(c->F.data(), L.dF, nf_known * 3 * sizeof(int), hipMemcpyDeviceToHost, s);
  return e;
}
int read_back_f64(mrh_ctx* c, const MeshLink& L, const MeshOpts& o) {
  hipStream_t s = c->stream;
  const double t0 = now_ms();
  const size_t cap_v = std::min(c->V.cap, c->C.cap) / 3, cap_f = c->F.cap / 3;
  const bool speculative = f64_pinned(c, o) && cap_v > 0 && c->V.data() && c->C.data() && c->F.data();
  if (speculative) HIP_TRY(c, copy_out_f64(c, L, true, 0, 0));
  HIP_TRY(c, hipMemcpyAsync(c->h_mc + HMC_VERTICES, L.d_totals, 2 * sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const double t1 = now_ms();
  const size_t nv = (size_t) c->h_mc[HMC_VERTICES], nf = (size_t) c->h_mc[HMC_FACES];
  const bool fits = speculative && nv <= cap_v && nf <= cap_f;
  c->V.resize_discard(nv * 3); c->C.resize_discard(nv * 3); c->F.resize_discard(std::max<size_t>(nf, 1) * 3);
  c->F.n = nf * 3;
  if (!fits) {
    HIP_TRY(c, copy_out_f64(c, L, f64_pinned(c, o), nv, nf));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  HIP_TRY(c, hipGetLastError());
  if (o.dbg) fprintf(stderr, "[mrhash_hip] mesh post-process: %u soup vertices -> %zu vertices, %zu faces | kernels%s %.2f ms, second copy (buffers grown) %.2f (%.1f MB)\n",
                     L.n, nv, nf, speculative ? " + copy to the host" : "", t1 - t0, now_ms() - t1, (nv * 48 + nf * 12) / 1e6);
  return MRH_OK;
}

// ---- the default way out: fp32 over the link, widened by the host as the chunks land (k_stage_out).  Speculative like the
// above: into the staging of the previous extraction, and again if that turns out too small.
bool stream_drained(void* stream) { return hipStreamQuery((hipStream_t) stream) != hipErrorNotReady; }
bool stage_ready(const mrh_ctx* c) { return c->V32.dev && c->C32.dev && c->F.dev && c->stage_ctl.dev; }
// The one launch site of k_stage_out.  The first launch of an extraction (`clear_pending`) also clears the index tables.
StageOut launch_stage_out(mrh_ctx* c, const MeshLink& L, const MeshOpts& o, bool* clear_pending, u32* epoch_out) {
  StageOut a;
  a.src[0] = (const uint4*) L.dV; a.src[1] = (const uint4*) L.dC; a.src[2] = (const uint4*) L.dF;
  a.dst[0] = (uint4*) c->V32.dev; a.dst[1] = (uint4*) c->C32.dev; a.dst[2] = (uint4*) c->F.dev;
  a.totals = L.d_totals;
  a.cap_v = std::min(c->V32.cap, c->C32.cap) / 3; a.cap_f = c->F.cap / 3;
  // one flag per chunk the staging can hold
  const u32 max_chunks = (u32) ((a.cap_v * 12 + 15) / 16 / kStageWords + 1);
  const size_t room = (c->stage_ctl.cap - kStageHdrWords) / 2;
  if (max_chunks > room) a.cap_v = (u64) (room > 1 ? (room - 1) : 0) * kStageChunk / 12;
  a.hdr = (u64*) c->stage_ctl.dev;
  a.flags = c->stage_ctl.dev + kStageHdrWords;
  a.flag_stride = (u32) room;
  if (++c->stage_epoch == 0) c->stage_epoch = 1;
  a.epoch = *epoch_out = c->stage_epoch;
  a.copy_wgs = (u32) o.stage_wgs;
  a.clear = L.tables;
  a.clear_words = *clear_pending ? L.table_words : 0;
  k_stage_out<<<o.stage_wgs + (*clear_pending ? 256 : 0), 256, 0, c->stream>>>(a);
  if (*clear_pending) { c->mesh_clean_base = L.tables; c->mesh_clean_words = L.table_words; }
  *clear_pending = false;
  return a;
}
// waits for the header of launch `epoch`; false: the stream ran dry without it (a failed launch)
bool wait_stage_hdr(mrh_ctx* c, const u32 epoch) {
  const volatile u64* hdr = (const volatile u64*) c->stage_ctl.data();
  for (u32 spins = 1;; spins++) {
    if (hdr[2] == (u64) epoch) break;
    MRH_CPU_RELAX();
    if ((spins & 1023u) == 0 && stream_drained(c->stream)) {  // dry: the header is there, or about to be — or the launch failed
      const auto t = std::chrono::steady_clock::now();
      while (hdr[2] != (u64) epoch && std::chrono::steady_clock::now() - t < std::chrono::milliseconds(200)) MRH_CPU_RELAX();
      if (hdr[2] == (u64) epoch) break;
      return false;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return true;
}
bool widen_staged(mrh_ctx* c, const u32 epoch, const size_t nv, const bool flagged) {
  double* const dst[2] = {c->V.data(), c->C.data()};
  const float* const src[2] = {c->V32.data(), c->C32.data()};
  const volatile u32* f0 = (const volatile u32*) c->stage_ctl.data() + kStageHdrWords;
  const volatile u32* const flags[2] = {flagged ? f0 : nullptr, flagged ? f0 + (c->stage_ctl.cap - kStageHdrWords) / 2 : nullptr};
  return widen_from_staging(dst, src, flags, epoch, nv * 3, stream_drained, c->stream);
}
int read_back_staged(mrh_ctx* c, const MeshLink& L, const MeshOpts& o) {
  hipStream_t s = c->stream;
  const double t0 = now_ms();
  bool clear_pending = true, done_ok = false;
  size_t nv = 0, nf = 0;
  double t1 = t0;
  if (stage_ready(c) && std::min(c->V32.cap, c->C32.cap) >= 3 && c->F.cap >= 3) {
    u32 epoch = 0;
    const StageOut a = launch_stage_out(c, L, o, &clear_pending, &epoch);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_mc + HMC_VERTICES, L.d_totals, 2 * sizeof(u64), hipMemcpyDeviceToHost, s));
    if (!wait_stage_hdr(c, epoch)) {
      HIP_TRY(c, hipStreamSynchronize(s));
      HIP_TRY(c, hipGetLastError());
      return fail(c, MRH_ERR_DEVICE, "mesh read-back: the staging kernel did not report");
    }
    const volatile u64* hdr = (const volatile u64*) c->stage_ctl.data();
    nv = (size_t) hdr[0]; nf = (size_t) hdr[1];
    if (nv <= a.cap_v && nf <= a.cap_f) {
      c->V.resize_discard(nv * 3); c->C.resize_discard(nv * 3);
      c->F.n = nf * 3;
      const bool ok = widen_staged(c, epoch, nv, true);
      HIP_TRY(c, hipStreamSynchronize(s));  // the faces, and the end of the launch
      HIP_TRY(c, hipGetLastError());
      if (!ok) return fail(c, MRH_ERR_DEVICE, "mesh read-back: a staged chunk never arrived");
      done_ok = true;
    } else {
      HIP_TRY(c, hipStreamSynchronize(s));
    }
    t1 = now_ms();
  } else {
    HIP_TRY(c, hipMemcpyAsync(c->h_mc + HMC_VERTICES, L.d_totals, 2 * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    nv = (size_t) c->h_mc[HMC_VERTICES]; nf = (size_t) c->h_mc[HMC_FACES];
    t1 = now_ms();
  }
  if (!done_ok) {  // first extraction, or the mesh outgrew the buffers: size them and go again
    size_mesh_staging(c, nv, std::max<size_t>(nf, 1));
    c->F.n = nf * 3;
    c->V.resize_discard(nv * 3); c->C.resize_discard(nv * 3);
    if (stage_ready(c)) {
      u32 epoch = 0;
      const StageOut a = launch_stage_out(c, L, o, &clear_pending, &epoch);
      HIP_TRY(c, hipGetLastError());
      bool ok = wait_stage_hdr(c, epoch) && nv <= a.cap_v && nf <= a.cap_f;
      if (ok) ok = widen_staged(c, epoch, nv, true);
      HIP_TRY(c, hipStreamSynchronize(s));
      HIP_TRY(c, hipGetLastError());
      if (!ok) return fail(c, MRH_ERR_DEVICE, "mesh read-back: the staged copy did not complete");
    } else {  // registration refused: plain copies, then the widening
      HIP_TRY(c, hipMemcpyAsync(c->V32.data(), L.dV, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
      HIP_TRY(c, hipMemcpyAsync(c->C32.data(), L.dC, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
      if (nf) HIP_TRY(c, hipMemcpyAsync(c->F.data(), L.dF, nf * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
      HIP_TRY(c, hipStreamSynchronize(s));
      (void) widen_staged(c, 0, nv, false);
    }
  }
  HIP_TRY(c, hipGetLastError());
  if (o.dbg) fprintf(stderr, "[mrhash_hip] mesh post-process: %u soup vertices -> %zu vertices, %zu faces | kernels + fp32 staging + widening %.2f ms, second pass (buffers grown) %.2f (%.1f MB over the link)\n",
                     L.n, nv, nf, t1 - t0, now_ms() - t1, (nv * 24 + nf * 12) / 1e6);
  return MRH_OK;
}

// MeshExtractor::processTriangles on the device (mrh_mesh.h): fills V / C / F from a triangle soup in device memory.
// MRH_MESH_HOST=1 keeps the host restatement above (same arrays; tests compare the two).
int process_triangles_device(mrh_ctx* c, const mrh_triangle* d_tris, const size_t nt) {
  // a helper that lost its core during the last extraction's widening may still be reading the staging this one is about to
  // rewrite, or writing the arrays it may regrow (CopyPool: the call no longer waits for its helpers)
  widen_quiesce();
  c->V.clear(); c->C.clear(); c->F.clear();
  if (nt == 0) return MRH_OK;
  if (nt * 3 >= (1ull << 30)) return fail(c, MRH_ERR_CAPACITY, "mesh post-process: %zu triangles exceed the 2^30 soup vertices one index table holds", nt);
  const MeshOpts o = read_mesh_opts();
  MeshLink L;
  const int rc = mesh_link_kernels(c, d_tris, nt, o, &L);
  if (rc) return rc;
  return c->f64_link ? read_back_f64(c, L, o) : read_back_staged(c, L, o);
}

// The post-process of a soup in device memory: on the device, or — MRH_MESH_HOST=1 — the soup to the host and the restatement
// there.  The caller synchronises the stream.
int post_process(mrh_ctx* c, const mrh_triangle* d_tris, const size_t nt) {
  if (!c->mesh_on_host) return process_triangles_device(c, d_tris, nt);
  c->tris.resize_discard(nt);
  HIP_TRY(c, hipMemcpyAsync(c->tris.data(), d_tris, nt * sizeof(mrh_triangle), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  process_triangles(c);
  return MRH_OK;
}

// ---- marching cubes: the stages of mrh_extract_triangles ---------------------------------------------------------------------
// the switches of an extraction, read once at the top of every call (tests toggle them between two extractions of one context)
struct ExtractOpts {
  bool dbg;               // MRH_DEBUG: the phase line on stderr
  bool radix_sort;        // MRH_MC_RADIX_SORT=1: the radix sort of mrh_sort.h for every list (A/B, tests)
  int slab_log2;          // MRH_MC_SLAB_LOG2=k (0 .. 20): runs of 2^k blocks dealt to the XCDs in turn (launch_mc); -1: off
  bool prescreen;         // MRH_MC_NO_PRESCREEN=1 switches the count pass's |sdf| bound off
  bool records;           // MRH_MC_NO_RECORDS=1 keeps the two-pass evaluation (tests compare the two)
  int records_per_block;  // MRH_MC_RECORDS_PER_BLOCK: the first record buffer (tests: one too small for the map); default 128
  bool coarse_known;      // MRH_MC_NO_COARSE_KNOWN=1: coarse voxels on the literal evaluation only (A/B, tests)
};
ExtractOpts read_extract_opts() {
  const char *slab = getenv("MRH_MC_SLAB_LOG2"), *per_block = getenv("MRH_MC_RECORDS_PER_BLOCK");
  return ExtractOpts{getenv("MRH_DEBUG") != nullptr, getenv("MRH_MC_RADIX_SORT") != nullptr, slab ? std::min(20, std::max(0, atoi(slab))) : -1,
                     getenv("MRH_MC_NO_PRESCREEN") == nullptr, getenv("MRH_MC_NO_RECORDS") == nullptr, per_block ? std::max(1, atoi(per_block)) : 128,
                     getenv("MRH_MC_NO_COARSE_KNOWN") == nullptr};
}

// arena slot 0: everything an extraction keeps on the device between the block count and the soup
struct McScratch {
  u64 *k_in, *k_out;     // position keys of the list; the radix sort's second key buffer
  int4 *sorted, *sorted2;  // the list in canonical order; the radix sort's second value buffer
  u32 *d_counts; u64 *d_offsets, *d_total;  // triangles per block, their exclusive scan, {triangles, record demand} (h_mc: HMC_TRIANGLES, HMC_RECORDS)
  u32* d_nb;             // 27-block neighbourhoods, kMcNbStride words a block
  uint8_t* d_per_voxel;  // triangles per voxel from the count pass: k_mc<emit> (the fallback of the record pass) skips the empty ones
  u32 *d_rec_base, *d_rec_n, *d_rec_ctr;  // McRecords: per block, and the two counters
  u32 *d_partial, *sort_tmp;  // k_block_rank: one row of partial ranks per slice; radix sort: 256 digit totals, then the tile histogram of a pass
};
void mc_layout(MeshScratch& a, const size_t n, const bool radix, McScratch* S) {
  const size_t rank_words = !radix ? n * ((n + kRankSlice - 1) / kRankSlice) : 1;
  const size_t sort_tiles = (n + kSortTile - 1) / kSortTile;
  const size_t tmp_bytes = radix ? (256 * sort_tiles + 256) * sizeof(u32) : 1;
  S->k_in = a.take<u64>(n); S->k_out = a.take<u64>(n); S->d_offsets = a.take<u64>(n);
  S->sorted = a.take<int4>(n); S->d_counts = a.take<u32>(n); S->d_nb = a.take<u32>(n * kMcNbStride);
  S->d_per_voxel = a.take<uint8_t>(n * 512); S->d_total = a.take<u64>(2);
  S->d_rec_base = a.take<u32>(n); S->d_rec_n = a.take<u32>(n); S->d_rec_ctr = a.take<u32>(2);
  S->d_partial = a.take<u32>(rank_words);
  S->sort_tmp = (u32*) a.take<char>(tmp_bytes);
  S->sorted2 = radix ? a.take<int4>(n) : nullptr;
}

// The list in canonical order -> S.sorted: by counting (mrh_mc.h: k_block_rank), or — lists beyond the counting rank — by the
// stable byte-wise radix sort of mrh_sort.h over the 64-bit position keys, the list entries riding along (eight passes; the
// first reads the list itself, the last lands in `sorted`).
void sort_blocks(mrh_ctx* c, const McScratch& S, const int n, const bool radix) {
  hipStream_t s = c->stream;
  k_list_keys<<<(n + 255) / 256, 256, 0, s>>>(c->tab.compact, n, S.k_in);
  if (!radix) {
    const int slices = (n + kRankSlice - 1) / kRankSlice;
    k_block_rank<<<dim3((n + 255) / 256, slices), 256, 0, s>>>(S.k_in, n, S.d_partial);
    k_block_scatter<<<(n + 255) / 256, 256, 0, s>>>(c->tab.compact, n, S.d_partial, slices, S.sorted);
    return;
  }
  u64* const ks[2] = {S.k_in, S.k_out};
  int4* const vs[2] = {S.sorted, S.sorted2};
  static_assert((64 / 8) % 2 == 0, "an even number of passes ends in the first buffer pair");
  (void) radix_sort_pairs<u64, int4>(s, ks, vs, (const int4*) c->tab.compact, (size_t) n, 64, S.sort_tmp, S.sort_tmp + 256);
}

// what the marching-cubes launches of one extraction share
struct McPass {
  int n, grid, flags;
  float sdf_bound;
  bool timed;        // profile mode: the launches carry the events of mrh_ctx::mc_ev
  bool use_records;
  McScratch S;
  McRecords R;
};

// One workgroup per block, block e = workgroup id: the eight XCDs walk the position-sorted list side by side, so a block's
// neighbours are staged by other XCDs at about the same time and their rows come out of the memory-side Infinity Cache
// (rocprofv3 counts 3.3 x the algorithmic bytes on the L2 -> fabric side).  Round 5 measured the alternative — runs of 2^k
// blocks dealt to the XCDs in turn, so that neighbours share an L2 (mc_first_block; MRH_MC_SLAB_LOG2=k switches it on): the
// fabric traffic falls to 261 / 253 / 217 / 172 / 160 MB for k = 3 / 5 / 7 / 9 / one run per XCD, and the count pass gets
// SLOWER with every step, 0.246 -> 0.258 / 0.263 / 0.284 / 0.350 / 0.347 ms (profiles/r05/README.md): the re-reads are
// Infinity Cache hits, not HBM traffic, and they are not what the kernel waits for.  Off by default.
void mc_pass_shape(const mrh_ctx* c, const ExtractOpts& o, const int n, McPass* p) {
  int slab_log2 = o.slab_log2;
  while (slab_log2 > 0 && ((size_t) 8 << slab_log2) > (size_t) n + 8) slab_log2--;  // never more than one run per XCD
  p->n = n;
  p->grid = slab_log2 < 0 ? n : (int) ((((size_t) n + ((size_t) 8 << slab_log2) - 1) >> (slab_log2 + 3)) << (slab_log2 + 3));
  // largest truncation a stored sample can carry (integration clamps to trunc + scale * depth, depth <= the integration distance)
  p->sdf_bound = c->has_camera && o.prescreen ? c->map.trunc + c->map.trunc_scale * c->cam.max_int_dist : 0.f;
  p->flags = (o.coarse_known ? 0 : 2)                       // bit 1: coarse voxels on the literal evaluation only
             | (slab_log2 < 0 ? 4 : (slab_log2 << 4));      // bit 2: block e = workgroup id; else bits 4..8: log2 of an XCD's run of blocks
  // kernel times for mrh_stats only in profile mode: launches that carry events switch the queue to its profiling mode,
  // which slows every later dispatch of the process
  p->timed = c->profile != 0;
}

// Corner records (mrh_mc.h McRecords): the count pass parks the corner values of every voxel that produces triangles, the
// emit pass interpolates them.  The buffer is sized from the last extraction's demand (first time: 128 records a block);
// if a block finds no room the whole extraction is emitted by k_mc<emit> and the buffer grows for the next one.
void ensure_mc_records(mrh_ctx* c, const ExtractOpts& o, McPass* p) {
  p->use_records = o.records;
  if (p->use_records && c->mc_rec_cap == 0) {
    const size_t cap = std::max<size_t>((size_t) p->n * (size_t) o.records_per_block, 16);
    if (dev_alloc(c, c->d_mc_recs, cap * kMcRecWords * sizeof(u32)) == hipSuccess) c->mc_rec_cap = cap;
    else { (void) hipGetLastError(); p->use_records = false; }  // no room for the records: the two-pass emit needs none
  }
  p->R.ctr = p->S.d_rec_ctr; p->R.recs = p->use_records ? c->d_mc_recs : nullptr; p->R.base = p->S.d_rec_base; p->R.count = p->S.d_rec_n;
  p->R.cap = (u32) std::min<size_t>(c->mc_rec_cap, 0xFFFFFFF0u);
}
// on every way out of the extraction, error returns included: room for this map's demand (+ 25 %) at the next one
struct GrowRecords {
  mrh_ctx* c;
  u64 demand = 0;  // known once the count pass has reported
  ~GrowRecords() {
    if (demand <= c->mc_rec_cap) return;
    (void) hipStreamSynchronize(c->stream);
    (void) dev_free(c, c->d_mc_recs);
    c->mc_rec_cap = 0;
    const size_t cap = (size_t) (demand + demand / 4);
    if (dev_alloc(c, c->d_mc_recs, cap * kMcRecWords * sizeof(u32)) == hipSuccess) c->mc_rec_cap = cap;
    else (void) hipGetLastError();  // no room: the next extraction starts from the default again
  }
};

// k_mc's arguments in the kernel's parameter order (mrh_mc.h); k_mc_emit_records takes a subset of them
struct McArgs {
  Map m; Tab t; const int4* sorted; int n;
  const u32* nb; u32* counts; const u64* offsets;
  mrh_triangle* out; u64 max_tris; uint8_t* per_voxel;
  float sdf_bound; int flags; McRecords R;
};
// The one launch site of k_mc<false> (the count pass) and k_mc<true> (the two-pass emit), and the one of k_mc_emit_records.
// Profile mode (`ev` given): the event pair is attached to the launch itself, as in back_as.
template <bool EMIT>
void launch_mc(const int grid, hipStream_t s, const EvPair* ev, const McArgs& a) {
  if (ev) hipExtLaunchKernelGGL((k_mc<EMIT>), dim3(grid), dim3(kMcThreads), 0, s, ev->a, ev->b, 0u, a.m, a.t, a.sorted, a.n, a.nb, a.counts, a.offsets, a.out,
                                a.max_tris, a.per_voxel, a.sdf_bound, a.flags, a.R);
  else k_mc<EMIT><<<grid, kMcThreads, 0, s>>>(a.m, a.t, a.sorted, a.n, a.nb, a.counts, a.offsets, a.out, a.max_tris, a.per_voxel, a.sdf_bound, a.flags, a.R);
}
void launch_mc_emit_records(const int grid, hipStream_t s, const EvPair* ev, const McArgs& a) {
  if (ev) hipExtLaunchKernelGGL(k_mc_emit_records, dim3(grid), dim3(kMcThreads), 0, s, ev->a, ev->b, 0u, a.m, a.t, a.sorted, a.n, a.R, a.offsets, a.out, a.max_tris,
                                a.flags);
  else k_mc_emit_records<<<grid, kMcThreads, 0, s>>>(a.m, a.t, a.sorted, a.n, a.R, a.offsets, a.out, a.max_tris, a.flags);
}
void launch_mc_count(mrh_ctx* c, const McPass& p) {
  const EvPair ev{c->mc_ev[0], c->mc_ev[1]};
  launch_mc<false>(p.grid, c->stream, p.timed ? &ev : nullptr,
                   McArgs{c->map, c->tab, p.S.sorted, p.n, p.S.d_nb, p.S.d_counts, nullptr, nullptr, 0, p.S.d_per_voxel, p.sdf_bound, p.flags, p.R});
}
// the emit pass into the soup buffer, at most `cap` triangles: from the corner records, or by evaluating the blocks again
void launch_mc_emit(mrh_ctx* c, const McPass& p, const u64 cap, const int flag_overflow, const bool from_records) {
  const EvPair ev{c->mc_ev[2], c->mc_ev[3]};
  McArgs a{c->map, c->tab, p.S.sorted, p.n, p.S.d_nb, p.S.d_counts, p.S.d_offsets, c->d_soup, cap, p.S.d_per_voxel, 0.f, flag_overflow | p.flags, p.R};
  if (from_records) return launch_mc_emit_records(p.grid, c->stream, p.timed ? &ev : nullptr, a);
  a.R = McRecords{nullptr, nullptr, nullptr, nullptr, 0};  // the two-pass emit reads none
  launch_mc<true>(p.grid, c->stream, p.timed ? &ev : nullptr, a);
}

// the soup for the caller (c->tris): through the copy kernel if the host buffer is pinned (see k_copy_out)
int soup_to_host(mrh_ctx* c, const u64 total) {
  hipStream_t s = c->stream;
  c->tris.resize_discard(total);
  if (c->tris.dev) {
    CopyOut a;
    for (int p = 0; p < 3; p++) { a.src[p] = nullptr; a.dst[p] = nullptr; a.count[p] = nullptr; a.fixed[p] = 0; a.cap[p] = 0; a.unit[p] = 0; }
    a.src[0] = (const uint4*) c->d_soup; a.dst[0] = (uint4*) c->tris.dev; a.fixed[0] = total; a.cap[0] = total; a.unit[0] = (u32) sizeof(mrh_triangle);
    k_copy_out<<<1024, 256, 0, s>>>(a);
  } else {
    HIP_TRY(c, hipMemcpyAsync(c->tris.data(), c->d_soup, total * sizeof(mrh_triangle), hipMemcpyDeviceToHost, s));
  }
  return MRH_OK;
}
// Where the soup goes: while a merge is on, the running mesh takes it (the post-process runs once, over everything, in
// mrh_mesh_merge_end); else the device post-process; with MRH_MESH_HOST=1 nothing here — the caller restates it on the host copy.
int deliver_soup(mrh_ctx* c, const u64 total) {
  hipStream_t s = c->stream;
  if (!c->merge_on) return c->mesh_on_host ? MRH_OK : process_triangles_device(c, c->d_soup, total);
  const size_t room = c->acc_n + total, cap = room + room / 2;
  if (room > c->acc_cap) {
    if (const int rc = regrow_keep(c, c->d_acc, c->acc_cap, cap, cap * sizeof(mrh_triangle), c->acc_n * sizeof(mrh_triangle))) return rc;
  }
  HIP_TRY(c, hipMemcpyAsync(c->d_acc + c->acc_n, c->d_soup, total * sizeof(mrh_triangle), hipMemcpyDeviceToDevice, s));
  c->acc_n += total;
  return MRH_OK;
}

// The extraction of a list of n > 0 blocks, compacted in c->tab.compact.  Everything between the block count and the triangle
// total stays on the device: canonical order (sort_blocks; key order == (x, y, z) order), the 27-block neighbourhoods resolved by
// one thread per (block, neighbour), per-block triangle counts -> exclusive scan (k_mc_scan_total) -> exact offsets, the emit
// pass launched right behind it.  The sorted list and the counts are read back only if somebody asks (mrh_get_triangle_blocks).
// t[1 .. 4]: the phase clock of MRH_DEBUG.
int extract_soup(mrh_ctx* c, const ExtractOpts& o, const int n, const bool want_soup, double* t, uint64_t* out_total) {
  hipStream_t s = c->stream;
  const bool radix = n > kRankSortMax || o.radix_sort;
  McPass p;
  MeshScratch arena;
  int rc = arena_layout(c, 0, &arena, [&](MeshScratch& a) { mc_layout(a, (size_t) n, radix, &p.S); });
  if (rc) return rc;
  if ((rc = ensure_h_mc(c))) return rc;
  sort_blocks(c, p.S, n, radix);
  k_mc_neighbors<<<(int) (((size_t) n * 32 + 255) / 256), 256, 0, s>>>(c->tab, p.S.sorted, n, p.S.d_nb);
  if (o.dbg) { HIP_TRY(c, hipStreamSynchronize(s)); t[1] = now_ms(); }
  mc_pass_shape(c, o, n, &p);
  c->last_mc_count_ms = c->last_mc_emit_ms = 0.f;
  c->last_mc_blocks = (uint64_t) n;
  if (p.timed)
    for (hipEvent_t& ev : c->mc_ev)
      if (!ev) HIP_TRY(c, event_new(c, ev, true));
  GrowRecords grow_records{c};
  ensure_mc_records(c, o, &p);
  if (p.use_records) HIP_TRY(c, hipMemsetAsync(p.S.d_rec_ctr, 0, 2 * sizeof(u32), s));
  launch_mc_count(c, p);
  // exact offsets + the total: one workgroup chains tiles of 8 192 counts through a carry (10^6 blocks: 122 tiles, ~0.2 ms
  // next to the ~20 ms of their count pass)
  k_mc_scan_total<<<1, 1024, 0, s>>>(p.S.d_counts, n, p.S.d_offsets, p.use_records ? p.S.d_rec_ctr : nullptr, p.S.d_total);
  HIP_TRY(c, hipMemcpyAsync(c->h_mc + HMC_TRIANGLES, p.S.d_total, 2 * sizeof(u64), hipMemcpyDeviceToHost, s));
  // The emit pass goes out BEFORE the host knows the total, into the soup buffer of the previous extraction (grow-only, 12 %
  // head room): a map that is extracted again — the usual case — needs no round trip between the two passes.  Writes beyond
  // the capacity are suppressed by the kernel; if the total turns out larger, the buffer grows and the pass runs again.
  const u64 spec_cap = std::min<u64>(c->soup_cap, c->max_triangles);
  // the host waits for the TOTAL, not for the emit pass behind it: it sizes and enqueues the post-process while the emit pass
  // runs (a stream synchronisation here left the GPU idle for the ~20 us of the host's round trip and first launch)
  if (!c->ev_mc_total) HIP_TRY(c, event_new(c, c->ev_mc_total, false));
  HIP_TRY(c, hipEventRecord(c->ev_mc_total, s));
  if (spec_cap > 0) launch_mc_emit(c, p, spec_cap, 0, p.use_records);
  HIP_TRY(c, hipEventSynchronize(c->ev_mc_total));
  const u64 total = c->h_mc[HMC_TRIANGLES];
  const bool records_ok = p.use_records && (c->h_mc[HMC_RECORDS] >> 63) == 0;
  const bool emitted = spec_cap > 0 && total <= spec_cap && (records_ok || !p.use_records);
  grow_records.demand = p.use_records ? c->h_mc[HMC_RECORDS] & ~(1ull << 63) : 0;
  if (o.dbg) t[2] = now_ms();
  c->tri_dev_n = n;
  c->d_tri_sorted = p.S.sorted;
  c->d_tri_counts = p.S.d_counts;
  if (total > c->max_triangles)
    return fail(c, MRH_ERR_CAPACITY, "triangle buffer full: %llu triangles > max_triangles %llu", (unsigned long long) total, (unsigned long long) c->max_triangles);
  if (total == 0) {
    if (p.timed) HIP_TRY(c, hipEventElapsedTime(&c->last_mc_count_ms, c->mc_ev[0], c->mc_ev[1]));
    HIP_TRY(c, hipGetLastError());
    return MRH_OK;
  }
  if (!emitted) {
    rc = ensure_soup(c, (size_t) total);
    if (rc) return rc;
    launch_mc_emit(c, p, total, 1, records_ok);
    if (p.use_records && !records_ok) c->mc_rec_fallbacks++;
  }
  c->soup_n = (size_t) total;
  if (p.timed) {
    HIP_TRY(c, hipEventSynchronize(c->mc_ev[3]));
    HIP_TRY(c, hipEventElapsedTime(&c->last_mc_count_ms, c->mc_ev[0], c->mc_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(&c->last_mc_emit_ms, c->mc_ev[2], c->mc_ev[3]));
  }
  if (o.dbg) { HIP_TRY(c, hipStreamSynchronize(s)); t[3] = now_ms(); }
  if (want_soup && (rc = soup_to_host(c, total))) return rc;
  if (o.dbg) { HIP_TRY(c, hipStreamSynchronize(s)); t[4] = now_ms(); }
  rc = deliver_soup(c, total);
  HIP_TRY(c, hipStreamSynchronize(s));
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  *out_total = total;
  return MRH_OK;
}

}  // namespace

extern "C" {

int mrh_extract_triangles(mrh_ctx* c, const mrh_triangle** out_tris, uint64_t* out_n) {
  int rc = ensure_ready(c, "mrh_extract_triangles");
  if (rc) return rc;
  if (!out_n) return MRH_ERR_INVALID_ARG;
  if (c->pending) return fail(c, MRH_ERR_STATE, "mrh_extract_triangles: an exchange is pending (call mrh_integrate_resume)");
  const ExtractOpts o = read_extract_opts();
  // out_tris == NULL: the caller only wants the mesh (mrh_extract_mesh) — the soup stays on the device.  The host
  // restatement of the post-process (MRH_MESH_HOST=1) reads the host copy, so it keeps it.
  const bool want_soup = out_tris != nullptr || c->mesh_on_host;
  uint64_t n_tris = 0;
  double t[6];
  t[0] = now_ms();
  for (int i = 1; i < 6; i++) t[i] = t[0];
  int n = 0;
  rc = compact_all(c, &n);  // the one scalar the host needs up front: it sizes the sort and the launches
  if (rc) return rc;
  c->n_extractions++;  // from here on the caller may hold pointers into the result buffers: the prewarm leaves them alone
  c->tris.clear();
  c->tri_blocks.clear();
  c->tri_counts.clear();
  c->tri_dev_n = 0;
  c->last_triangles = 0;
  c->soup_n = 0;
  if (n > 0 && (rc = extract_soup(c, o, n, want_soup, t, &n_tris))) return rc;
  c->last_triangles = n_tris;
  // no triangles (V / C / F are cleared), or MRH_MESH_HOST=1: the host restatement, over the host copy of the soup
  if (!c->merge_on && (n_tris == 0 || c->mesh_on_host)) process_triangles(c);
  t[5] = now_ms();
  if (o.dbg) fprintf(stderr, "[mrhash_hip] extract: %d blocks, %llu triangles | list+sort+neighbours %.2f ms, count+scan(+speculative emit) %.2f, emit %.2f, soup D2H %.2f, post-process + V/F/C D2H %.2f, total %.2f\n",
                     n, (unsigned long long) n_tris, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[5] - t[0]);
  if (out_tris) *out_tris = c->tris.empty() ? nullptr : c->tris.data();
  *out_n = n_tris;
  return MRH_OK;
}

// MeshExtractor::merge_mesh_ = true (geowrapper.cpp:161) ... the chunk loop ... the final mesh.  The reference runs
// processTriangles after every extraction, on (running mesh + new soup).  That equals ONE processTriangles over the soups back
// to back: the vertex merge keeps first occurrences with their indices and colours, and "drop degenerate faces" / "drop
// repeated faces keeping the first" are order-preserving filters, so applying them to a prefix first changes nothing
// (tests/test_geowrapper_gpu.py compares with the oracle, which restates the incremental form literally).
int mrh_mesh_merge_begin(mrh_ctx* c) {
  if (!c) return MRH_ERR_INVALID_ARG;
  c->n_extractions++;
  c->merge_on = true;
  c->acc_n = 0;
  c->V.clear(); c->C.clear(); c->F.clear();
  return MRH_OK;
}

int mrh_mesh_merge_end(mrh_ctx* c, uint64_t* out_total_triangles) {
  int rc = ensure_ready(c, "mrh_mesh_merge_end");
  if (rc) return rc;
  if (!c->merge_on) return fail(c, MRH_ERR_STATE, "mrh_mesh_merge_end: no merge in progress (mrh_mesh_merge_begin)");
  c->merge_on = false;
  if (out_total_triangles) *out_total_triangles = c->acc_n;
  c->last_triangles = c->acc_n;
  c->tris.clear();
  if (c->acc_n == 0) { c->V.clear(); c->C.clear(); c->F.clear(); return MRH_OK; }
  rc = post_process(c, c->d_acc, c->acc_n);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return rc;
}

int mrh_extract_mesh(mrh_ctx* c, const double** v, uint64_t* nv, const int32_t** f, uint64_t* nf, const double** col) {
  if (!c || !v || !nv || !f || !nf || !col) return MRH_ERR_INVALID_ARG;
  c->n_extractions++;  // the caller holds these pointers until the next extraction
  *v = c->V.empty() ? nullptr : c->V.data();
  *nv = c->V.size() / 3;
  *f = c->F.empty() ? nullptr : c->F.data();
  *nf = c->F.size() / 3;
  *col = c->C.empty() ? nullptr : c->C.data();
  return MRH_OK;
}

int mrh_get_triangle_blocks(mrh_ctx* c, const mrh_block_desc** out_descs, const uint32_t** out_counts, uint64_t* out_n) {
  if (!c || !out_descs || !out_counts || !out_n) return MRH_ERR_INVALID_ARG;
  if (c->tri_dev_n > 0) {  // the list and the counts of the last extraction are still where the kernels left them
    const size_t n = (size_t) c->tri_dev_n;
    std::vector<int4> list(n);
    c->tri_counts.resize(n);
    HIP_TRY(c, hipMemcpyAsync(list.data(), c->d_tri_sorted, n * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->tri_counts.data(), c->d_tri_counts, n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->tri_blocks.resize(n);
    for (size_t i = 0; i < n; i++) c->tri_blocks[i] = {list[i].x, list[i].y, list[i].z, (list[i].w & (int) kValCoarseBit) ? 1 : 0};
    c->tri_dev_n = 0;
  }
  *out_descs = c->tri_blocks.empty() ? nullptr : c->tri_blocks.data();
  *out_counts = c->tri_counts.empty() ? nullptr : c->tri_counts.data();
  *out_n = c->tri_blocks.size();
  return MRH_OK;
}

int mrh_process_triangles(mrh_ctx* c, const mrh_triangle* triangles, uint64_t n) {
  if (!c || (n && !triangles)) return MRH_ERR_INVALID_ARG;
  c->tris.assign(triangles, triangles + n);
  c->last_triangles = n;
  if (c->mesh_on_host || n == 0) { process_triangles(c); return MRH_OK; }
  int rc = ensure_ready(c, "mrh_process_triangles");
  if (rc) return rc;
  DevBuf<mrh_triangle> d_tris;
  HIP_TRY(c, d_tris.alloc(n));
  HIP_TRY(c, hipMemcpyAsync(d_tris, triangles, n * sizeof(mrh_triangle), hipMemcpyHostToDevice, c->stream));
  return process_triangles_device(c, d_tris, n);
}

int mrh_get_triangles_device(mrh_ctx* c, const mrh_triangle** out, uint64_t* out_n, int* out_is_device_memory) {
  if (!c || !out || !out_n) return MRH_ERR_INVALID_ARG;
  *out = c->soup_n ? c->d_soup : nullptr;
  *out_n = c->soup_n;
  if (out_is_device_memory) *out_is_device_memory = 1;
  return MRH_OK;
}

int mrh_process_triangle_runs(mrh_ctx* c, const mrh_block_desc* descs, const uint32_t* counts, uint64_t n_blocks, const mrh_triangle* triangles,
                              uint64_t n_triangles, int is_device_memory) {
  int rc = ensure_ready(c, "mrh_process_triangle_runs");
  if (rc) return rc;
  if ((n_blocks && (!descs || !counts)) || (n_triangles && !triangles)) return fail(c, MRH_ERR_INVALID_ARG, "mrh_process_triangle_runs: null argument");
  hipStream_t s = c->stream;
  // runs in input order -> canonical order (block position): a host sort of the few-byte descriptors, a device permutation
  // of the 72-byte triangles
  std::vector<uint64_t> src_off(n_blocks);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n_blocks; i++) { src_off[i] = total; total += counts[i]; }
  if (total != n_triangles) return fail(c, MRH_ERR_INVALID_ARG, "mrh_process_triangle_runs: the counts add up to %llu triangles, %llu given", (unsigned long long) total, (unsigned long long) n_triangles);
  std::vector<uint32_t> order(n_blocks);
  for (uint64_t i = 0; i < n_blocks; i++) order[i] = (uint32_t) i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (descs[a].x != descs[b].x) return descs[a].x < descs[b].x;
    if (descs[a].y != descs[b].y) return descs[a].y < descs[b].y;
    return descs[a].z < descs[b].z;
  });
  c->tri_dev_n = 0;
  c->tri_blocks.resize(n_blocks);
  c->tri_counts.resize(n_blocks);
  std::vector<ulonglong2> runs;  // {source offset, destination offset | count << 40}
  runs.reserve(n_blocks);
  uint64_t dst = 0;
  for (uint64_t k = 0; k < n_blocks; k++) {
    const uint32_t i = order[k];
    c->tri_blocks[k] = descs[i];
    c->tri_counts[k] = counts[i];
    if (counts[i]) runs.push_back(make_ulonglong2(src_off[i], dst | ((uint64_t) counts[i] << 40)));
    dst += counts[i];
  }
  c->tris.clear();
  c->last_triangles = n_triangles;
  c->soup_n = 0;
  if (n_triangles == 0) { c->V.clear(); c->C.clear(); c->F.clear(); return MRH_OK; }
  if (n_triangles >= (1ull << 40)) return fail(c, MRH_ERR_CAPACITY, "mrh_process_triangle_runs: too many triangles");
  rc = ensure_soup(c, (size_t) n_triangles);
  if (rc) return rc;
  DevBuf<mrh_triangle> staged;
  const mrh_triangle* d_in = triangles;
  if (!is_device_memory) {
    HIP_TRY(c, staged.alloc(n_triangles));
    HIP_TRY(c, hipMemcpyAsync(staged, triangles, n_triangles * sizeof(mrh_triangle), hipMemcpyHostToDevice, s));
    d_in = staged;
  }
  DevBuf<ulonglong2> d_runs;
  HIP_TRY(c, d_runs.alloc(runs.size()));
  HIP_TRY(c, hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(ulonglong2), hipMemcpyHostToDevice, s));
  k_permute_runs<<<(int) std::min<size_t>(runs.size(), 8192), 256, 0, s>>>((const ulonglong2*) d_runs, (int) runs.size(), (const uint4*) d_in, (uint4*) c->d_soup);
  c->soup_n = (size_t) n_triangles;
  rc = post_process(c, c->d_soup, (size_t) n_triangles);
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, hipGetLastError());
  return rc;
}

}  // extern "C"
