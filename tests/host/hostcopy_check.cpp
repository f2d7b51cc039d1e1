// Stand-alone check of mrhash_amd/csrc/mrh_hostcopy.h — the copy pool behind mrh_upload_* and the widening of an extracted mesh —
// on any CPU: no GPU, no HIP.  tests/test_hostcopy.py builds it with AddressSanitizer + UBSan and expects exit status 0.
//
// Copies go through copy_to_staging (inline below 4 chunks, the pool from there on, a ragged last chunk).  Widening goes through
// widen_from_staging with a second thread in the device's role: it publishes the chunk flags in reverse order, part 1 before
// part 0, so every helper meets flags that have not arrived yet.
#include "mrh_hostcopy.h"

#include <cstdio>

namespace {

int failures = 0;

template <typename T>
T* aligned(const size_t n) {
  const size_t bytes = (n * sizeof(T) + 31) / 32 * 32;
  return (T*) std::aligned_alloc(32, bytes ? bytes : 32);
}

void check_copy(const size_t n) {
  std::vector<unsigned char> src(n);
  unsigned char* dst = aligned<unsigned char>(n);
  for (int rep = 0; rep < 20; rep++) {
    for (size_t i = 0; i < n; i++) src[i] = (unsigned char) (i * 131u + (size_t) rep * 17u + (i >> 9));
    memset(dst, 0xA5, n);
    copy_to_staging(dst, src.data(), n);
    if (memcmp(dst, src.data(), n) != 0) {
      fprintf(stderr, "copy of %zu bytes, repetition %d: bytes differ\n", n, rep);
      failures++;
    }
  }
  std::free(dst);
}

void check_widen(const size_t nfloat, uint32_t& epoch) {
  const size_t per = (nfloat * sizeof(float) + CopyPool::kWidenChunk - 1) / CopyPool::kWidenChunk;
  float* src[2] = {aligned<float>(nfloat), aligned<float>(nfloat)};
  double* dst[2] = {aligned<double>(nfloat), aligned<double>(nfloat)};
  std::vector<uint32_t> words[2] = {std::vector<uint32_t>(per, 0u), std::vector<uint32_t>(per, 0u)};
  const volatile uint32_t* flags[2] = {words[0].data(), words[1].data()};
  for (int e = 0; e < 5; e++) {
    epoch++;
    for (int part = 0; part < 2; part++)
      for (size_t i = 0; i < nfloat; i++) {
        src[part][i] = (float) ((double) ((i * 2654435761u + epoch * 40503u + (unsigned) part) & 0xFFFFFFu) / 4099.0 - 2000.0);
        dst[part][i] = -1.0;
      }
    widen_prewake();
    std::thread device([&] {  // everything a chunk's flag covers was written before the thread started
      for (int part = 1; part >= 0; part--)
        for (size_t i = per; i-- > 0;) {
          std::atomic_thread_fence(std::memory_order_release);
          ((volatile uint32_t*) words[part].data())[i] = epoch;
        }
    });
    const bool ok = widen_from_staging(dst, src, flags, epoch, nfloat, nullptr, nullptr);
    device.join();
    widen_quiesce();
    if (!ok) {
      fprintf(stderr, "widening of %zu floats, epoch %u: gave up\n", nfloat, epoch);
      failures++;
    }
    size_t bad = 0;
    for (int part = 0; part < 2; part++)
      for (size_t i = 0; i < nfloat; i++) bad += dst[part][i] != (double) src[part][i];
    if (bad) {
      fprintf(stderr, "widening of %zu floats, epoch %u: %zu doubles differ\n", nfloat, epoch, bad);
      failures++;
    }
  }
  for (int part = 0; part < 2; part++) { std::free(src[part]); std::free(dst[part]); }
}

}  // namespace

int main() {
  const size_t k = CopyPool::kChunk;
  for (const size_t n : {(size_t) 1, (size_t) 31, 4 * k - 1, 4 * k, 5 * k + 17, (size_t) 3 << 20}) check_copy(n);
  uint32_t epoch = 0;
  for (const size_t n : {(size_t) 1, (size_t) 16384, (size_t) 16385, (size_t) 300001}) check_widen(n, epoch);
  widen_quiesce();
  printf("hostcopy_check: %d failures, %llu chunks redone\n", failures, (unsigned long long) widen_redone());
  return failures ? 1 : 0;
}
