// Snippet index map of one dilation (rollingdepth_pipeline.py:465-502, get_snippet_indice): the
// snippets start at range(0, last + 1, ss), plus the last window `last` when the range misses it.
//   stride  frame step inside a snippet (the dilation)
//   ss      start step: frame step between consecutive snippet starts (the reference's `stride`)
//   last    N − win, win = (w − 1)·stride + 1: the start of the last window that fits N frames
// One definition for the device code (aligner.hip, merge.hip), the host-side validation and the CPU check
// programs (tests/cpp/aligner_index_check.cpp, cover_count_check.cpp): plain integer functions, no
// other dependency.
#pragma once

#if defined(__HIPCC__)
#define RDMI_HD __host__ __device__ inline
#else
#define RDMI_HD inline
#endif

// start of the last window of length w and frame step `stride` in N frames (< 0: none fits)
RDMI_HD int rdmi_snip_last(int N, int w, int stride) { return N - ((w - 1) * stride + 1); }

// number of snippets (last >= 0, ss >= 1)
RDMI_HD int rdmi_snip_count(int last, int ss) { return last / ss + 1 + (last % ss != 0 ? 1 : 0); }

// first frame of snippet k (0 <= k < count)
RDMI_HD int rdmi_snip_start(int k, int ss, int last) {
  const long q = (long)k * ss;
  return q < last ? (int)q : last;
}

// the snippet that starts at frame q, or -1 when none does (n = rdmi_snip_count(last, ss))
RDMI_HD int rdmi_snip_at(int q, int ss, int last, int n) {
  if (q < 0 || q > last) return -1;
  if (q == last) return n - 1;
  return q % ss == 0 ? q / ss : -1;
}

// number of (dilation, slot) pairs covering frame f over nd dilations: slot j of dilation d covers f
// when a snippet of d starts at frame f − j·stride[d] (n[d] = rdmi_snip_count(last[d], ss[d]))
RDMI_HD int rdmi_cover_count(int nd, const int* n, const int* stride, const int* w, const int* ss, const int* last,
                             int f) {
  int cnt = 0;
  for (int d = 0; d < nd; ++d)
    for (int j = 0; j < w[d]; ++j) cnt += rdmi_snip_at(f - j * stride[d], ss[d], last[d], n[d]) >= 0 ? 1 : 0;
  return cnt;
}
