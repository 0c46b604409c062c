// Stand-alone check of rollingdepth_amd/csrc/aligner_ws.h (the workspace layout shared by
// rdmi_aligner_workspace and rdmi_aligner_optimize): every region inside the total, the regions
// pairwise disjoint and in the documented order, f64 regions at even float offsets, m / v / counters
// contiguous, and the total equal to the closed formula.
// Built with g++ -fsanitize=address,undefined and run as a child process by tests/test_strided_cpu.py.
#include <cstdio>

#include "aligner_ws.h"

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

struct Region {
  const char* name;
  long off, len;  // floats
  bool f64;
};

int main() {
  const long Ps[] = {1, 9, 5929};
  const int ntots[] = {1, 2, 12, 148, 1024};
  const int its[] = {0, 1, 20, 128, 129, 2000};
  const long PS = 8;
  long cases = 0;
  for (int N = 1; N <= 40; ++N)
    for (long P : Ps)
      for (int ntot : ntots)
        for (int iters : its)
          for (int hist = 0; hist < 2; ++hist) {
            ++cases;
            const rdmi_aligner_layout L = rdmi_aligner_ws_layout(N, P, ntot, iters, hist != 0);
            const long slots = !hist ? 0 : iters < 128 ? iters : 128;
            const long nps = ntot * PS, nfs = N * PS, pad = (ntot + 1) & ~1L;
            // the documented order, each with the floats its users touch
            const Region r[] = {
                {"gs", L.gs, 2 * nps, true},          {"gt", L.gt, 2 * nps, true},
                {"l1", L.l1, 2 * nps, true},          {"l2", L.l2, 2 * nps, true},
                {"fpart", L.fpart, 8 * nfs, true},    {"T", L.T, N * P, false},
                {"Td", L.Td, N * P, false},           {"m", L.m, 2L * ntot, false},
                {"v", L.v, 2L * ntot, false},         {"cnt", L.cnt, pad, false},
                {"bct", L.bct, 4L * (iters + 1), true},
                {"hl", L.hl, slots * 4 * nps, true},  {"hmm", L.hmm, slots * 2 * nfs, false},
                {"hst", L.hst, slots * 2 * ntot, false},
            };
            const int nr = sizeof r / sizeof r[0];
            CHECK(L.slots == slots, "slots N %d P %ld ntot %d iters %d hist %d: %ld\n", N, P, ntot, iters, hist, L.slots);
            CHECK(r[0].off == 0, "base N %d P %ld ntot %d iters %d hist %d\n", N, P, ntot, iters, hist);
            for (int i = 0; i < nr; ++i) {
              CHECK(r[i].off >= 0 && r[i].len >= 0 && r[i].off + r[i].len <= L.total,
                    "%s outside N %d P %ld ntot %d iters %d hist %d: %ld+%ld of %ld\n", r[i].name, N, P, ntot, iters,
                    hist, r[i].off, r[i].len, L.total);
              if (r[i].f64)
                CHECK(r[i].off % 2 == 0 && r[i].len % 2 == 0, "%s f64 at odd offset N %d P %ld ntot %d iters %d hist %d: %ld\n",
                      r[i].name, N, P, ntot, iters, hist, r[i].off);
              if (i + 1 < nr)  // in order and disjoint from every later region
                CHECK(r[i].off + r[i].len <= r[i + 1].off, "%s overlaps %s N %d P %ld ntot %d iters %d hist %d\n",
                      r[i].name, r[i + 1].name, N, P, ntot, iters, hist);
            }
            // one zeroing launch covers m, v and the counters
            CHECK(L.m + 2L * ntot == L.v && L.v + 2L * ntot == L.cnt && L.cnt + pad == L.bct,
                  "m/v/cnt not contiguous N %d P %ld ntot %d iters %d hist %d\n", N, P, ntot, iters, hist);
            long f = 8 * nps + 8 * nfs + 2 * N * P + 4L * ntot + pad + 4L * (iters + 1);
            if (hist) f += slots * (4 * nps + 2 * nfs + 2L * ntot) + 2;
            f += 64;
            CHECK(L.total == f, "total N %d P %ld ntot %d iters %d hist %d: %ld != %ld\n", N, P, ntot, iters, hist,
                  L.total, f);
          }
  std::printf("%ld cases, %ld failures\n", cases, fails);
  return fails ? 1 : 0;
}
