// What the optimiser (aligner.hip) and the merge family (merge.hip) share on the host: the limits of a job, the
// validation of its start steps against the index map (aligner_index.h), the choice of a kernel's <SS>.
#pragma once
#include <type_traits>

#include "common.h"
#include "aligner_index.h"

namespace rdmi {

constexpr int MAXD = 8;
constexpr int MAXR = 64;  // rows Σ w_d of the reference's M / M_depth / B tensors

// How much of a job an entry point checks.  Those from before rdmi_version 6 keep their leniency because callers
// rely on it (jobs built against version 1 leave start_step zeroed; the calls without start steps state no
// sequence length to check a layout against); the later ones never had it.
//   checks   entry points (rdmi_aligner_…)                                  start steps          layout checked
//   Lenient  merge, merge_partial_window, merge_finish_pieces               none travel: all 1   never
//   Lenient  optimize and the three merges' _strided forms                  0 (or NULL): 1, ≥ 0  if some step > 1
//   Strict   merge_moments, merge_partial_window_moments,
//            merge_finish_pieces_moments, merge_median,
//            merge_partial_window_terms                                     required, every ≥ 1  always
// Strict calls that take snippets also require Σ w_d ≤ MAXR, seq_len > 0 and x_f32 ∈ 0 … 2 (merge.hip).
enum class Checks { Lenient, Strict };

// The start steps of a job → ss[d], last[d]; *strided: some start step is > 1.  The layout check, before any
// launch: a window fits the N frames, n[d] is the count the map gives.
inline int start_steps(const char* what, Checks checks, int nd, const int* start_step, const int* n,
                       const int* stride, const int* w, int N, int* ss, int* last, bool* strided) {
  const bool strict = checks == Checks::Strict;
  *strided = false;
  for (int d = 0; start_step && d < nd; ++d)
    if (start_step[d] > 1) *strided = true;
  for (int d = 0; d < nd; ++d) {
    const int v = start_step ? start_step[d] : 1;
    if (strict) {
      RDMI_REQUIRE(v >= 1, RDMI_E_ARG, "%s: start step %d of dilation %d (>= 1 expected)", what, v, d);
      RDMI_REQUIRE(stride[d] >= 1 && w[d] >= 1, RDMI_E_ARG, "%s: dilation %d: length %d, frame stride %d", what, d,
                   w[d], stride[d]);
    }
    RDMI_REQUIRE(v >= 0, RDMI_E_ARG, "%s: start step %d of dilation %d", what, v, d);
    ss[d] = v ? v : 1;
    last[d] = rdmi_snip_last(N, w[d], stride[d]);
    if (!strict && !*strided) continue;
    RDMI_REQUIRE(stride[d] >= 1 && w[d] >= 1 && last[d] >= 0, RDMI_E_ARG,
                 "%s: dilation %d: a snippet of length %d and frame stride %d does not fit %d frames", what, d, w[d],
                 stride[d], N);
    const int want = rdmi_snip_count(last[d], ss[d]);
    RDMI_REQUIRE(n[d] == want, RDMI_E_ARG,
                 "%s: dilation %d: %d snippets, but start step %d over %d frames (length %d, frame stride %d) gives %d",
                 what, d, n[d], ss[d], N, w[d], stride[d], want);
  }
  return 0;
}

// A kernel's <SS>: launch(std::true_type) when some start step is > 1, launch(std::false_type) otherwise.
template <class F>
void with_ss(bool strided, F&& launch) {
  if (strided) launch(std::true_type{});
  else launch(std::false_type{});
}

}  // namespace rdmi
