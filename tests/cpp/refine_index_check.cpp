// Stand-alone check of rollingdepth_amd/csrc/refine_index.h (the class-major snippet map of a strided
// refine step, shared by the averaging kernels and their host-side validation) against brute-force
// enumeration: per residue class r of the frames mod d, starts = range(0, L_r − w + 1, ss) in class
// positions, plus L_r − w when the range misses it; classes in ascending order.
// Built with g++ -fsanitize=address,undefined and run as a child process by tests/test_refine_stride_cpu.py.
#include <cstdio>
#include <vector>

#include "refine_index.h"

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
  for (int N = 3; N <= 40; ++N)
    for (int w = 1; w <= 4; ++w)
      for (int d = 1; d <= N / w; ++d)
        for (int ss = 1; ss <= w; ++ss) {
          ++cases;
          std::vector<int> starts;  // start frame of snippet k, class-major
          for (int r = 0; r < d; ++r) {
            int L = 0;
            for (int f = r; f < N; f += d) ++L;
            if (L < w) continue;
            std::vector<int> pos;
            for (int m = 0; m < L - w + 1; m += ss) pos.push_back(m);
            if (pos.back() < L - w) pos.push_back(L - w);
            for (int m : pos) starts.push_back(r + d * m);
          }
          const int n = rdmi_refine_count(N, w, d, ss);
          CHECK(n == (int)starts.size(), "count N %d w %d d %d ss %d: %d != %zu\n", N, w, d, ss, n, starts.size());
          if (n != (int)starts.size()) continue;
          const int span = (w - 1) * d, lo = -span - 2;
          std::vector<int> at(N + 2 * span + 4, -1);  // brute-force inverse, frames lo .. N + span + 1
          std::vector<int> cover(N, 0);
          for (int k = 0; k < n; ++k) {
            const int q = rdmi_refine_start(k, N, w, d, ss);  // index → start
            CHECK(q == starts[k], "start N %d w %d d %d ss %d k %d: %d != %d\n", N, w, d, ss, k, q, starts[k]);
            at[starts[k] - lo] = k;
            for (int j = 0; j < w; ++j) {
              const int f = starts[k] + j * d;
              CHECK(f >= 0 && f < N, "frame N %d w %d d %d ss %d k %d j %d: %d\n", N, w, d, ss, k, j, f);
              if (f >= 0 && f < N) ++cover[f];
            }
          }
          for (int q = lo; q < lo + (int)at.size(); ++q) {  // start → index, frames outside [0, N) included
            const int k = rdmi_refine_at(q, N, w, d, ss);
            CHECK(k == at[q - lo], "at N %d w %d d %d ss %d q %d: %d != %d\n", N, w, d, ss, q, k, at[q - lo]);
          }
          for (int f = 0; f < N; ++f) {  // the kernels' cover count: slots that find a snippet
            int cnt = 0;
            for (int j = 0; j < w; ++j) cnt += rdmi_refine_at(f - j * d, N, w, d, ss) >= 0 ? 1 : 0;
            CHECK(cnt == cover[f] && cnt > 0, "cover N %d w %d d %d ss %d f %d: %d != %d\n", N, w, d, ss, f, cnt, cover[f]);
          }
        }
  std::printf("%ld cases, %ld failures\n", cases, fails);
  return fails ? 1 : 0;
}
