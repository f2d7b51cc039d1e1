// track_solve_check.cpp — the host half of depth-frame tracking (mrhash_amd/csrc/mrh_tracksolve.h) on its own: a plain
// C++17 program that includes the header alone, for tests/test_track_host.py (g++ -ffp-contract=off, ASan + UBSan).
//
// stdin, per case: max_depth, min_pixels, the 32 sums, R (9) and t (3) as decimal / hexadecimal floating-point text.
// stdout, per case: "scale <S_a>", then "lost" or "xi <6 values>", "pose <R 9> <t 3>" after one update, "rms <value>", all in %a.
#include <cinttypes>
#include <cstdio>

#include "mrh_tracksolve.h"

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
  printf("track_solve_check: %d cases\n", cases);
  return 0;
}
