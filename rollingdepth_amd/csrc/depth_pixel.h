// What the depth-metric kernels (metrics.hip) and the boundary kernel (boundary.hip) share per pixel: the octet
// loads of the three operand types, the alignment spaces, the aligned value of a pixel, and the dispatch of the
// eight input combinations to kernel template arguments.  Everything is internal to the including file.
#pragma once
#include "common.h"

#include <math.h>

#include <type_traits>

namespace {

// one octet of an operand as f32 (f16 → f32 is exact); cnt < 8 only for the short last octet
__device__ __forceinline__ void load_octet(const f16* p, bool vec, int cnt, float (&v)[8]) {
  if (vec && cnt == 8) {
    ld8(p, v);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < cnt ? (float)p[e] : 0.f;
  }
}
__device__ __forceinline__ void load_octet(const float* p, bool vec, int cnt, float (&v)[8]) {
  if (vec && cnt == 8) {
    ld8(p, v);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < cnt ? p[e] : 0.f;
  }
}
__device__ __forceinline__ void load_octet(const unsigned char* p, bool vec, int cnt, unsigned char (&m)[8]) {
  if (vec && cnt == 8) {
    const u32x2 w = *(const u32x2*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = (unsigned char)(w[e >> 2] >> (8 * (e & 3)));
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = e < cnt ? p[e] : (unsigned char)0;
  }
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < INFINITY; }  // false for NaN

// φ and φ⁻¹ of the alignment space.  1 / x is the IEEE division; a disparity ≤ 0 has no finite depth: +inf
template <int SPACE>
__device__ __forceinline__ double to_space(double g) {
  return SPACE == RDMI_SPACE_DISPARITY ? 1.0 / g : SPACE == RDMI_SPACE_LOG ? log(g) : g;
}
template <int SPACE>
__device__ __forceinline__ double from_space(double d) {
  if (SPACE == RDMI_SPACE_DISPARITY) return d > 0.0 ? 1.0 / d : (double)INFINITY;
  return SPACE == RDMI_SPACE_LOG ? exp(d) : d;
}

// the aligned depth of one pixel, clamped; `space` is uniform over the launch
__device__ __forceinline__ double aligned_depth(double s, float p, double t, int space, double clip_lo,
                                                double clip_hi) {
  double a = fma(s, (double)p, t);
  if (space == RDMI_SPACE_DISPARITY)
    a = from_space<RDMI_SPACE_DISPARITY>(a);
  else if (space == RDMI_SPACE_LOG)
    a = from_space<RDMI_SPACE_LOG>(a);
  return fmin(fmax(a, clip_lo), clip_hi);
}

// the per-pixel rule of depth_errors_k without the mask; pos: the target must also be > 0
template <bool HAS_G>
__device__ __forceinline__ bool pixel_valid(float p, float g, float lo, float hi, bool pos) {
  bool ok = finite_f(p);
  if (HAS_G) ok = ok & finite_f(g) & (g > lo) & (g < hi) & (!pos | (g > 0.f));
  return ok;
}

inline bool dtype_ok(int d) { return d == RDMI_F16 || d == RDMI_F32; }
inline bool space_ok(int s) {
  return s == RDMI_SPACE_DEPTH || s == RDMI_SPACE_DISPARITY || s == RDMI_SPACE_LOG;
}

// the eight input combinations — pred f16 / f32 × target f16 / f32 × mask or not — as types: f(tag<TP>, tag<TG>,
// bool_constant<MASK>) is called for the one the arguments name
template <typename T>
struct tag {
  using type = T;
};
template <typename F>
void with_input_types(int pred_dtype, int target_dtype, bool masked, F&& f) {
  auto with_target = [&](auto tp) {
    auto with_mask = [&](auto tg) {
      if (masked)
        f(tp, tg, std::true_type{});
      else
        f(tp, tg, std::false_type{});
    };
    if (target_dtype == RDMI_F32)
      with_mask(tag<float>{});
    else
      with_mask(tag<f16>{});
  };
  if (pred_dtype == RDMI_F32)
    with_target(tag<float>{});
  else
    with_target(tag<f16>{});
}

}  // namespace
