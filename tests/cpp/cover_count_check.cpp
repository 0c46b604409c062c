// Stand-alone check of rdmi_cover_count (rollingdepth_amd/csrc/aligner_index.h: the cover count the
// sharded merge's finish kernel divides by) against brute-force enumeration of the reference's snippet
// lists: starts = range(0, N − win + 1, ss), plus N − win when the range misses it; snippet k covers
// frames start_k + j·dilation, j < length.  One- and two-dilation jobs, every frame (and two frames past
// either end, where the count is 0).
// Built with g++ -fsanitize=address,undefined and run as a child process by tests/test_shard_strided_cpu.py.
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

struct Layout {
  int w, dil, ss, last, n;
  std::vector<int> cover;  // brute force: snippets of this dilation covering frame f − LO
};

constexpr int LO = -2;  // first frame checked; the last is N + 1

int main() {
  long cases1 = 0, cases2 = 0;
  for (int N = 1; N <= 40; ++N) {
    std::vector<Layout> layouts;
    for (int w = 1; w <= 4; ++w)
      for (int dil = 1; dil <= 6; ++dil)
        for (int ss = 1; ss <= 8; ++ss) {
          const int win = (w - 1) * dil + 1;
          if (N < win) continue;
          std::vector<int> starts;
          for (int q = 0; q < N - win + 1; q += ss) starts.push_back(q);
          if (starts.back() < N - win) starts.push_back(N - win);
          Layout L{w, dil, ss, N - win, (int)starts.size(), std::vector<int>(N + 4, 0)};
          for (int q : starts)
            for (int j = 0; j < w; ++j) ++L.cover[q + j * dil - LO];
          CHECK(rdmi_snip_last(N, w, dil) == L.last && rdmi_snip_count(L.last, ss) == L.n,
                "layout N %d w %d dil %d ss %d\n", N, w, dil, ss);
          layouts.push_back(L);
        }
    for (const Layout& a : layouts) {
      ++cases1;
      for (int f = LO; f < N + 2; ++f) {
        const int got = rdmi_cover_count(1, &a.n, &a.dil, &a.w, &a.ss, &a.last, f);
        CHECK(got == a.cover[f - LO], "one N %d w %d dil %d ss %d f %d: %d != %d\n", N, a.w, a.dil, a.ss, f, got,
              a.cover[f - LO]);
      }
      for (const Layout& b : layouts) {
        ++cases2;
        const int n[2] = {a.n, b.n}, dil[2] = {a.dil, b.dil}, w[2] = {a.w, b.w}, ss[2] = {a.ss, b.ss},
                  last[2] = {a.last, b.last};
        for (int f = LO; f < N + 2; ++f) {
          const int got = rdmi_cover_count(2, n, dil, w, ss, last, f);
          const int want = a.cover[f - LO] + b.cover[f - LO];
          CHECK(got == want, "two N %d w %d,%d dil %d,%d ss %d,%d f %d: %d != %d\n", N, a.w, b.w, a.dil, b.dil, a.ss,
                b.ss, f, got, want);
        }
      }
    }
  }
  std::printf("%ld one-dilation cases, %ld two-dilation cases, %ld failures\n", cases1, cases2, fails);
  return fails ? 1 : 0;
}
