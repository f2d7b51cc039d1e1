// track_solve_check.cpp — the host half of depth-frame tracking (mrhash_amd/csrc/mrh_tracksolve.h) on its own: a plain
// C++17 program that includes the header alone, for tests/test_track_host.py (g++ -ffp-contract=off, ASan + UBSan).
//
// stdin, per case: max_depth, min_pixels, the 32 sums, R (9) and t (3) as decimal / hexadecimal floating-point text.
// stdout, per case: "scale <S_a>", then "lost" or "xi <6 values>", "pose <R 9> <t 3>" after one update, "rms <value>", all in %a.
//
// Then the loop (mrh_track::Fit, fit_run, fit_report; D14 "Loop").  stdin, per case: the word "loop", max_depth, min_pixels,
// iterations, run (0: the observation is empty and fit_run is not called), the number of recorded steps, fail_at and fail_code (the
// callable returns fail_code at call fail_at; -1: never), the binary32 start pose R (9) and t (3), then 32 sums per recorded step.
// stdout, per case: "at <R 9> <t 3>" for every call of the callable — the pose it was handed — then "loop <return value> <status>
// <updates> <calls> <n>", "pose <R 9> <t 3>", "rms <value>" and "sums <32 values>", all as fit_report fills them.  A call beyond the
// recorded steps ends the program with status 3.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mrh_tracksolve.h"

// the fields mrh_track_info and mrh_align_info share, with a count of its own name
struct Report {
  int32_t status, iterations_done;
  uint64_t n;
  double rms;
  int64_t sums[mrh_track::kSumWords];
};

int main() {
  int cases = 0;
  for (;;) {
    float max_depth;
    unsigned min_pixels;
    int64_t sums[mrh_track::kSumWords];
    double R[9], t[3];
    if (scanf("%f %u", &max_depth, &min_pixels) != 2) break;
    for (int i = 0; i < mrh_track::kSumWords; i++)
      if (scanf("%" SCNd64, &sums[i]) != 1) return 2;
    for (int i = 0; i < 9; i++)
      if (scanf("%lf", &R[i]) != 1) return 2;
    for (int i = 0; i < 3; i++)
      if (scanf("%lf", &t[i]) != 1) return 2;
    const float s_a = mrh_track::angle_scale(max_depth);
    printf("scale %a\n", (double) s_a);
    double xi[6];
    if (!mrh_track::solve(sums, s_a, min_pixels, xi)) {
      printf("lost\n");
    } else {
      printf("xi");
      for (int i = 0; i < 6; i++) printf(" %a", xi[i]);
      printf("\n");
      mrh_track::update(R, t, xi);
      printf("pose");
      for (int i = 0; i < 9; i++) printf(" %a", R[i]);
      for (int i = 0; i < 3; i++) printf(" %a", t[i]);
      printf("\n");
    }
    printf("rms %a\n", mrh_track::rms(sums));
    cases++;
  }
  // the loop (mrh_track::fit_run) with a callable that replays recorded sums
  for (;;) {
    char word[8];
    float max_depth, R0[9], t0[3];
    unsigned min_count;
    int iterations, run, n_steps, fail_at, fail_code;
    if (scanf("%7s", word) != 1) break;
    if (strcmp(word, "loop") != 0) return 2;
    if (scanf("%f %u %d %d %d %d %d", &max_depth, &min_count, &iterations, &run, &n_steps, &fail_at, &fail_code) != 7) return 2;
    for (int i = 0; i < 9; i++)
      if (scanf("%f", &R0[i]) != 1) return 2;
    for (int i = 0; i < 3; i++)
      if (scanf("%f", &t0[i]) != 1) return 2;
    std::vector<int64_t> steps((size_t) n_steps * mrh_track::kSumWords);
    for (int64_t& v : steps)
      if (scanf("%" SCNd64, &v) != 1) return 2;
    mrh_track::Fit f(R0, t0);
    int calls = 0, rc = 0;
    bool overrun = false;
    if (run)
      rc = mrh_track::fit_run(f, iterations, mrh_track::angle_scale(max_depth), min_count, [&](const float* R, const float* t, int64_t* sums) {
        const int k = calls++;
        printf("at");
        for (int i = 0; i < 9; i++) printf(" %a", (double) R[i]);
        for (int i = 0; i < 3; i++) printf(" %a", (double) t[i]);
        printf("\n");
        if (k == fail_at) return fail_code;
        if (k >= n_steps) { overrun = true; return -100; }  // the loop asked for a step the case does not have
        for (int i = 0; i < mrh_track::kSumWords; i++) sums[i] = steps[(size_t) k * mrh_track::kSumWords + i];
        return 0;
      });
    if (overrun) return 3;
    float R[9], t[3];
    Report info;
    mrh_track::fit_report(f, R, t, &info, &Report::n);
    printf("loop %d %d %d %d %" PRIu64 "\n", rc, (int) info.status, (int) info.iterations_done, calls, info.n);
    printf("pose");
    for (int i = 0; i < 9; i++) printf(" %a", (double) R[i]);
    for (int i = 0; i < 3; i++) printf(" %a", (double) t[i]);
    printf("\nrms %a\nsums", info.rms);
    for (int i = 0; i < mrh_track::kSumWords; i++) printf(" %" PRId64, info.sums[i]);
    printf("\n");
    mrh_track::fit_report(f, R, t, (Report*) nullptr, &Report::n);  // no info struct: the pose alone
    cases++;
  }
  printf("track_solve_check: %d cases\n", cases);
  return 0;
}
