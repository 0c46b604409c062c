// Workspace layout of rdmi_aligner_optimize: one definition for rdmi_aligner_workspace (the size), for
// rdmi_aligner_optimize (the views) and for the CPU check program (tests/cpp/aligner_ws_check.cpp).
// Plain integer arithmetic on the arguments, no other dependency: the size depends on nothing else.
#pragma once

// Pixel chunks per frame / per snippet: frame_stats and snippet_grad run N·PS and ntot·PS
// workgroups (one workgroup per frame or snippet alone left most of the 256 CUs idle and each
// latency-bound), partial sums combined in a fixed chunk order by the consumer (deterministic).
constexpr int RDMI_ALIGNER_PS = 8;
// Iterations per block of history slots: the fused loop keeps per-iteration loss partials for at
// most HBLK iterations, so the workspace does not grow with the iteration count (1500 frames with
// [1,10,25] at 2000 iterations would otherwise need 1.4 GB).
constexpr int RDMI_ALIGNER_HBLK = 128;

// Offsets in floats from the (8-byte aligned) workspace base, in this order.  gs .. fpart, bct and hl
// hold doubles: their offsets are even.  m, v and cnt are contiguous (one launch zeroes them).
struct rdmi_aligner_layout {
  long gs, gt, l1, l2;  // [ntot][PS] doubles each: gradient and loss partials per snippet and pixel chunk
  long fpart;           // [N][PS][4] doubles
  long T, Td;           // [N][P] floats each
  long m, v;            // [2·ntot] floats each: Adam moments
  long cnt;             // [ntot] per-snippet arrival counters, padded to 8 bytes
  long bct;             // [iters + 1][2] doubles: Adam's bias corrections
  // the fused loop's per-iteration history slots, `slots` = min(iters, HBLK) with a history, else 0:
  long hl;              // [slots][2][ntot][PS] doubles: loss partials
  long hmm;             // [slots][N][PS][2] floats: chunk min / max
  long hst;             // [slots][2·ntot] floats: parameters before the update
  long slots;
  long total;           // floats to allocate (the regions, 2 more with a history, and 64)
};

inline rdmi_aligner_layout rdmi_aligner_ws_layout(int N, long P, int ntot, int iters, bool hist) {
  constexpr long PS = RDMI_ALIGNER_PS;
  const long nps = (long)ntot * PS, nfs = (long)N * PS;
  rdmi_aligner_layout L{};
  L.gs = 0;
  L.gt = L.gs + 2 * nps;
  L.l1 = L.gt + 2 * nps;
  L.l2 = L.l1 + 2 * nps;
  L.fpart = L.l2 + 2 * nps;
  L.T = L.fpart + 8 * nfs;
  L.Td = L.T + (long)N * P;
  L.m = L.Td + (long)N * P;
  L.v = L.m + 2L * ntot;
  L.cnt = L.v + 2L * ntot;
  L.bct = L.cnt + ((ntot + 1) & ~1L);
  L.hl = L.bct + 4L * (iters + 1);
  L.slots = !hist ? 0 : iters < RDMI_ALIGNER_HBLK ? iters : RDMI_ALIGNER_HBLK;
  L.hmm = L.hl + L.slots * 4 * nps;
  L.hst = L.hmm + L.slots * 2 * nfs;
  L.total = L.hst + L.slots * 2 * ntot + (hist ? 2 : 0) + 64;
  return L;
}
