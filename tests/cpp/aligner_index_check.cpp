// Stand-alone check of rollingdepth_amd/csrc/aligner_index.h (the snippet index map shared by the
// aligner kernels and the host-side validation) against brute-force enumeration of the reference's
// get_snippet_indice: starts = range(0, N − win + 1, ss), plus N − win when the range misses it.
// Built with g++ -fsanitize=address,undefined and run as a child process by tests/test_strided_cpu.py.
#include <cstdio>
#include <vector>

#include "aligner_index.h"

static long fails = 0;

#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (fails < 20) {                     \
        std::printf("FAIL " __VA_ARGS__);   \
        std::printf("  [%s]\n", #cond);     \
      }                                     \
      ++fails;                              \
    }                                       \
  } while (0)

int main() {
  long cases = 0;
  for (int N = 1; N <= 40; ++N)
    for (int w = 1; w <= 4; ++w)
      for (int dil = 1; dil <= 6; ++dil)
        for (int ss = 1; ss <= 8; ++ss) {
          const int win = (w - 1) * dil + 1;
          if (N < win) continue;
          ++cases;
          std::vector<int> starts;
          for (int q = 0; q < N - win + 1; q += ss) starts.push_back(q);
          if (starts.back() < N - win) starts.push_back(N - win);
          const int last = rdmi_snip_last(N, w, dil);
          const int n = rdmi_snip_count(last, ss);
          CHECK(last == N - win, "last N %d w %d dil %d ss %d: %d\n", N, w, dil, ss, last);
          CHECK(n == (int)starts.size(), "count N %d w %d dil %d ss %d: %d != %zu\n", N, w, dil, ss, n, starts.size());
          if (n != (int)starts.size()) continue;
          std::vector<int> at(N + 2 * win + 2, -1);  // brute-force inverse, frames −win−1 .. N+win
          const int lo = -win - 1;
          for (int k = 0; k < n; ++k) {
            const int q = rdmi_snip_start(k, ss, last);
            CHECK(q == starts[k], "start N %d w %d dil %d ss %d k %d: %d != %d\n", N, w, dil, ss, k, q, starts[k]);
            CHECK(rdmi_snip_at(q, ss, last, n) == k, "inverse N %d w %d dil %d ss %d k %d\n", N, w, dil, ss, k);
            for (int j = 0; j < w; ++j) {
              const int f = q + j * dil;
              CHECK(f >= 0 && f < N, "frame N %d w %d dil %d ss %d k %d j %d: %d\n", N, w, dil, ss, k, j, f);
            }
            if (q == starts[k]) at[q - lo] = k;
          }
          for (int q = lo; q < lo + (int)at.size(); ++q) {
            const int k = rdmi_snip_at(q, ss, last, n);
            CHECK(k == at[q - lo], "at N %d w %d dil %d ss %d q %d: %d != %d\n", N, w, dil, ss, q, k, at[q - lo]);
            if (k >= 0) CHECK(rdmi_snip_start(k, ss, last) == q, "start(at) N %d w %d dil %d ss %d q %d\n", N, w, dil, ss, q);
          }
        }
  std::printf("%ld cases, %ld failures\n", cases, fails);
  return fails ? 1 : 0;
}
