// mrh_hostcopy.h — the host's bulk copies: images into pinned staging (mrh_upload.h), fp32 staging widened into the caller's
// doubles (mrh_extract.h), both shared by one process-wide pool of helper threads.
// Plain host C++, no HIP header, nothing of the library's namespace: tests/host/hostcopy_check.cpp compiles it alone and runs the
// pool under AddressSanitizer + UBSan without a GPU.  The device pass of the library's translation unit sees the stubs at the end.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#if !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#define MRH_CPU_RELAX() _mm_pause()
#else
#define MRH_CPU_RELAX() ((void) 0)  // host code as the device pass sees it
#endif

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
bool widen_from_staging(double* const dst[2], const float* const src[2], const volatile uint32_t* const flags[2], uint32_t epoch, size_t nfloat,
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
bool widen_from_staging(double* const dst[2], const float* const src[2], const volatile uint32_t* const flags[2], uint32_t epoch, size_t nfloat,
                        bool (*drained)(void*), void* arg) { return false; }
void widen_prewake() {}
void widen_quiesce() {}
uint64_t widen_redone() { return 0; }
#endif
}  // namespace
