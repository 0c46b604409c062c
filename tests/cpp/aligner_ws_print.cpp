// Prints every offset of rdmi_aligner_ws_layout (csrc/aligner_ws.h) for the argument tuples on the command
// line, five integers each: N P ntot iters hist.  One output line per tuple:
//   N P ntot iters hist : gs gt l1 l2 fpart T Td m v cnt bct hl hmm hst slots total
// tests/test_aligner_step_cpu.py compares the lines with the Python mirror (tests/aligner_util.py::ws_layout)
// that the GPU tests read the workspace through.
#include <cstdio>
#include <cstdlib>

#include "aligner_ws.h"

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 1) % 5 != 0) {
    std::fprintf(stderr, "usage: %s N P ntot iters hist [N P ntot iters hist ...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 4 < argc; i += 5) {
    const int N = std::atoi(argv[i]);
    const long P = std::atol(argv[i + 1]);
    const int ntot = std::atoi(argv[i + 2]), iters = std::atoi(argv[i + 3]), hist = std::atoi(argv[i + 4]);
    const rdmi_aligner_layout L = rdmi_aligner_ws_layout(N, P, ntot, iters, hist != 0);
    std::printf("%d %ld %d %d %d : %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", N, P, ntot, iters,
                hist != 0, L.gs, L.gt, L.l1, L.l2, L.fpart, L.T, L.Td, L.m, L.v, L.cnt, L.bct, L.hl, L.hmm, L.hst,
                L.slots, L.total);
  }
  return 0;
}
