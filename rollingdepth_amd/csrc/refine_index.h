// Snippet index map of one strided refine step (pipeline.refine_snippet_indice): the start step is
// taken inside each residue class of the frames mod d, so that every frame stays covered at every
// frame step d (get_snippet_indice's own `stride` leaves frame 1 in no snippet for any d > 1).
//   d   frame step inside a snippet (the step's dilation);  R = N % d
//   ss  start step, in class positions (1 <= ss <= w covers every frame of a class that holds a snippet)
// Class r (0 <= r < d) holds the frames r, r + d, r + 2d, ... — L_r = N / d + (r < R) of them, numbered
// 0, 1, 2, ... — and its snippets start at the positions of aligner_index.h's map for (last = L_r − w, ss);
// a class with L_r < w has none.  The snippet at position m of class r is the frames r + d·(m + j),
// j = 0 .. w−1.  Order: class-major (r ascending, then position ascending); the classes r < R hold
// c_hi = count(N/d + 1 − w, ss) snippets each and the others c_lo = count(N/d − w, ss).
// One definition for the device code (elementwise.hip), the host-side validation and the CPU check
// program (tests/cpp/refine_index_check.cpp): plain integer functions over aligner_index.h.
#pragma once

#include "aligner_index.h"

// number of snippets of a class of L frames (0 when no window of w fits)
RDMI_HD int rdmi_refine_class_count(int L, int w, int ss) { return L < w ? 0 : rdmi_snip_count(L - w, ss); }

// number of snippets of the step (N >= 1, w >= 1, d >= 1, ss >= 1)
RDMI_HD int rdmi_refine_count(int N, int w, int d, int ss) {
  const int R = N % d;
  return R * rdmi_refine_class_count(N / d + 1, w, ss) + (d - R) * rdmi_refine_class_count(N / d, w, ss);
}

// class-major index of the snippet that starts at frame q, or -1 when none does
RDMI_HD int rdmi_refine_at(int q, int N, int w, int d, int ss) {
  if (q < 0 || q >= N) return -1;
  const int R = N % d, r = q % d, m = q / d;
  const int c_hi = rdmi_refine_class_count(N / d + 1, w, ss), c_lo = rdmi_refine_class_count(N / d, w, ss);
  const int L = N / d + (r < R ? 1 : 0), c = r < R ? c_hi : c_lo;
  if (c == 0) return -1;
  const int i = rdmi_snip_at(m, ss, L - w, c);
  if (i < 0) return -1;
  return (r < R ? r : R) * c_hi + (r > R ? r - R : 0) * c_lo + i;
}

// first frame of snippet k (0 <= k < rdmi_refine_count)
RDMI_HD int rdmi_refine_start(int k, int N, int w, int d, int ss) {
  const int R = N % d;
  const int c_hi = rdmi_refine_class_count(N / d + 1, w, ss), c_lo = rdmi_refine_class_count(N / d, w, ss);
  int r, i, L;
  if (k < R * c_hi) {
    r = k / c_hi, i = k % c_hi, L = N / d + 1;
  } else {
    k -= R * c_hi;
    r = R + k / c_lo, i = k % c_lo, L = N / d;
  }
  return r + d * rdmi_snip_start(i, ss, L - w);
}
