// Affine-invariant depth metrics (rdmi.h "Depth metrics"): per-frame moments of (pred, target) over the
// valid pixels, the least-squares scale / shift they give, and the error sums of s·pred + t against the
// target.  Everything is f64: the product of two f16 / f32 inputs is exact in it.
//
// Tiling, shared by the moments and the errors pass.  A frame's P pixels are cut into octets, octet o =
// elements 8o .. 8o+7 counted from the FRAME's first element, the last one possibly short.  Grid
// (bpf, N) with bpf = blocks_per_frame(P), a function of P alone; 256 threads; thread t of block b takes
// octets b·256 + t, + bpf·256, ... in rising order and adds their elements in rising order.  Which lane
// adds which element therefore depends on nothing but P — not on the device, not on N, not on where the
// buffers lie — and with the fixed butterfly / LDS / block-order reductions below every sum is
// reproducible bit for bit.  An operand whose octets are 16-byte aligned in this frame (its frame base
// is) is read with 16-byte loads (the u8 mask: 8-byte); one that is not is read element by element, in the
// same assignment, and so is the short last octet.  No atomics anywhere.
//
// Alignment space (rdmi.h RDMI_SPACE_*): the fit may be taken against φ(target) = target, 1 / target or
// ln target, and the aligned value is brought back to depth through φ⁻¹ before the clamp.  The space is a
// template parameter of the two streaming kernels; RDMI_SPACE_DEPTH instantiates the code they always had.
//
// Temporal pass (rdmi_depth_temporal): pair i compares frame i with frame i + k on the tiling above, the
// grid being (bpf, N − k).  Frame i's operands come in octets as before; frame i + k is read at the same
// pixel or, with a flow, at up to four bilinear taps with plain scalar loads.
#include "depth_pixel.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRow = 8;  // doubles per partial row (moments use the first 6)
constexpr int kFitThreads = 1024;  // the one workgroup of the fit kernel

// blocks per frame: one block per 4096 pixels (16 per thread), at most 256; more pixels than that are
// grid-strided.  P only.
inline int blocks_per_frame(long P) {
  const long b = (P + 4095) / 4096;
  return (int)(b < 1 ? 1 : b > 256 ? 256 : b);
}

// cross-lane move of an f64 as its two 32-bit halves
__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)b, o, 64);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(b >> 32), o, 64);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// butterfly: every lane ends with the same bits (a + b is commutative), in an order fixed by the lane ids
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor_f64(v, o);
  return v;
}

// K per-thread sums → one partial row: across the wave, then the four waves in wave order through LDS
template <int K>
__device__ __forceinline__ void block_reduce_store(double (&acc)[K], double* __restrict__ row) {
  __shared__ double red[kThreads / 64][kRow];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = wave_sum_f64(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    row[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// Walks this block's octets of frame blockIdx.y and calls f(p, g) for every VALID pixel, in the fixed order.
// POS: a valid target is also > 0 (the disparity and log spaces)
template <typename TP, typename TG, bool MASK, bool POS, typename F>
__device__ __forceinline__ void for_valid_pixels(const TP* __restrict__ pred, const TG* __restrict__ target,
                                                 const unsigned char* __restrict__ mask, long P, float lo, float hi,
                                                 F&& f) {
  const long base = (long)blockIdx.y * P;
  const TP* pp = pred + base;
  const TG* gp = target + base;
  const unsigned char* mp = MASK ? mask + base : nullptr;
  const bool pv = ((uintptr_t)pp & 15) == 0, gv = ((uintptr_t)gp & 15) == 0, mv = ((uintptr_t)mp & 7) == 0;
  const long noct = (P + 7) >> 3;
  const long step = (long)gridDim.x * kThreads;
  for (long o = (long)blockIdx.x * kThreads + threadIdx.x; o < noct; o += step) {
    const long e0 = o << 3;
    const int cnt = (int)(P - e0 < 8 ? P - e0 : 8);
    float p[8], g[8];
    unsigned char m[8];
    load_octet(pp + e0, pv, cnt, p);
    load_octet(gp + e0, gv, cnt, g);
    if (MASK) load_octet(mp + e0, mv, cnt, m);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // one predicate, formed without branches; the pixel's arithmetic runs under it alone
      bool ok = (e < cnt) & finite_f(p[e]) & finite_f(g[e]) & (g[e] > lo) & (g[e] < hi);
      if (MASK) ok = ok & (m[e] != 0);
      if (POS) ok = ok & (g[e] > 0.f);
      if (ok) f(p[e], g[e]);
    }
  }
}

template <typename TP, typename TG, bool MASK, int SPACE>
__global__ __launch_bounds__(kThreads) void depth_moments_k(const TP* __restrict__ pred,
                                                            const TG* __restrict__ target,
                                                            const unsigned char* __restrict__ mask, long P, float lo,
                                                            float hi, double* __restrict__ part) {
  double acc[6] = {0, 0, 0, 0, 0, 0};  // n, Σp, Σg, Σp², Σpg, Σg² with g = φ(target)
  constexpr bool POS = SPACE != RDMI_SPACE_DEPTH;
  for_valid_pixels<TP, TG, MASK, POS>(pred, target, mask, P, lo, hi, [&](float pf, float gf) {
    const double p = pf, g = to_space<SPACE>((double)gf);
    acc[0] += 1.0;
    acc[1] += p;
    acc[2] += g;
    acc[3] = fma(p, p, acc[3]);  // exact products in depth space: fma and mul + add round alike
    acc[4] = fma(p, g, acc[4]);
    acc[5] = fma(g, g, acc[5]);
  });
  block_reduce_store<6>(acc, part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * kRow);
}

template <typename TP, typename TG, bool MASK, int SPACE>
__global__ __launch_bounds__(kThreads) void depth_errors_k(const TP* __restrict__ pred, const TG* __restrict__ target,
                                                           const unsigned char* __restrict__ mask, long P, float lo,
                                                           float hi, const double* __restrict__ st, double clip_lo,
                                                           double clip_hi, double* __restrict__ part) {
  // n, Σ|a−g|, Σ|a−g|/g, Σ(a−g)², Σ(a−g)²/g, #δ<1.25, #δ<1.25², #δ<1.25³
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const double s = st[2 * blockIdx.y], t = st[2 * blockIdx.y + 1];
  constexpr bool POS = SPACE != RDMI_SPACE_DEPTH;
  if (s == s && t == t) {  // a frame without a fit contributes nothing
    for_valid_pixels<TP, TG, MASK, POS>(pred, target, mask, P, lo, hi, [&](float pf, float gf) {
      const double g = gf;
      double a = from_space<SPACE>(fma(s, (double)pf, t));
      a = fmin(fmax(a, clip_lo), clip_hi);
      const double ad = fabs(a - g);
      const double q = ad / g;
      acc[0] += 1.0;
      acc[1] += ad;
      acc[2] += q;
      acc[3] = fma(ad, ad, acc[3]);
      acc[4] = fma(ad, q, acc[4]);
      // max(a/g, g/a) < c  ⇔  max(a, g) < c·min(a, g) for positive a, g: no division, one rounding in c·x
      const double big = fmax(a, g), small = fmin(a, g);
      const bool pos = small > 0.0;
      acc[5] += (pos & (big < 1.25 * small)) ? 1.0 : 0.0;
      acc[6] += (pos & (big < 1.5625 * small)) ? 1.0 : 0.0;
      acc[7] += (pos & (big < 1.953125 * small)) ? 1.0 : 0.0;
    });
  }
  block_reduce_store<8>(acc, part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * kRow);
}

// ----------------------------------------------------------------------------- temporal pass
struct no_target {};  // TG of a call without a target

// (1−wy)·((1−wx)·v00 + wx·v01) + wy·((1−wx)·v10 + wx·v11); a tap of weight 0 is passed as 0 and adds an
// exact 0, so a single tap of weight 1 comes back as it is.  One function for the prediction and the target, every
// operation rounded on its own (no contraction into the caller's subtraction), so equal taps give equal bits.
__device__ __forceinline__ double bilerp(double wx, double wy, double v00, double v01, double v10, double v11) {
#pragma clang fp contract(off)
  const double ux = 1.0 - wx, uy = 1.0 - wy;
  return uy * (ux * v00 + wx * v01) + wy * (ux * v10 + wx * v11);
}

// Pair blockIdx.y: frame f = blockIdx.y against frame f' = f + k.  Frame f is walked in for_valid_pixels' octet
// order; frame f' is read at the same pixel (octet loads again) or, with FLOW, at the bilinear taps of
// (x + dx, y + dy) with scalar loads — a tap is addressed only after it is known to lie inside the frame.
template <typename TP, typename TG, bool MASK, bool FLOW>
__global__ __launch_bounds__(kThreads) void depth_temporal_k(
    const TP* __restrict__ pred, const TG* __restrict__ target, const unsigned char* __restrict__ mask,
    const float* __restrict__ flow, const unsigned char* __restrict__ pair_mask, int H, int W, int k, float lo,
    float hi, const double* __restrict__ st, int space, double clip_lo, double clip_hi, double* __restrict__ part) {
  constexpr bool HAS_G = !std::is_same<TG, no_target>::value;
  // n, Σ|Δa|, ΣΔa², Σ|Δa−Δg|, Σ(Δa−Δg)², Σ|Δg|, ΣΔg², ΣΔa·Δg
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const long P = (long)H * W;
  const long f0 = blockIdx.y, f1 = f0 + k;
  const double s0 = st[2 * f0], t0 = st[2 * f0 + 1], s1 = st[2 * f1], t1 = st[2 * f1 + 1];
  const bool pos = space != RDMI_SPACE_DEPTH;
  if (s0 == s0 && t0 == t0 && s1 == s1 && t1 == t1) {  // a pair without both fits contributes nothing
    const TP* pp0 = pred + f0 * P;
    const TP* pp1 = pred + f1 * P;
    const TG* gp0 = nullptr;
    const TG* gp1 = nullptr;
    if constexpr (HAS_G) {
      gp0 = target + f0 * P;
      gp1 = target + f1 * P;
    }
    const unsigned char* mp0 = MASK ? mask + f0 * P : nullptr;
    const unsigned char* mp1 = MASK ? mask + f1 * P : nullptr;
    const unsigned char* qp = pair_mask ? pair_mask + f0 * P : nullptr;
    const float* fl = FLOW ? flow + f0 * P * 2 : nullptr;
    const bool pv0 = ((uintptr_t)pp0 & 15) == 0, gv0 = ((uintptr_t)gp0 & 15) == 0, mv0 = ((uintptr_t)mp0 & 7) == 0;
    const bool pv1 = ((uintptr_t)pp1 & 15) == 0, gv1 = ((uintptr_t)gp1 & 15) == 0, mv1 = ((uintptr_t)mp1 & 7) == 0;
    const bool qv = ((uintptr_t)qp & 7) == 0;

    // one tap of frame f': its validity, its aligned value and its target
    auto tap = [&](int yy, int xx, double& av, double& gv) -> bool {
      const long q = (long)yy * W + xx;
      const float pt = (float)pp1[q];
      float gt = 0.f;
      if constexpr (HAS_G) gt = (float)gp1[q];
      bool v = pixel_valid<HAS_G>(pt, gt, lo, hi, pos);
      if (MASK) v = v & (mp1[q] != 0);
      av = aligned_depth(s1, pt, t1, space, clip_lo, clip_hi);
      gv = gt;
      return v;
    };

    const long noct = (P + 7) >> 3;
    const long step = (long)gridDim.x * kThreads;
    for (long o = (long)blockIdx.x * kThreads + threadIdx.x; o < noct; o += step) {
      const long e0 = o << 3;
      const int cnt = (int)(P - e0 < 8 ? P - e0 : 8);
      float p[8], g[8], p1[8], g1[8];
      unsigned char m[8], m1[8], pm[8];
      load_octet(pp0 + e0, pv0, cnt, p);
      if constexpr (HAS_G) load_octet(gp0 + e0, gv0, cnt, g);
      if (MASK) load_octet(mp0 + e0, mv0, cnt, m);
      if (qp) load_octet(qp + e0, qv, cnt, pm);
      if (!FLOW) {
        load_octet(pp1 + e0, pv1, cnt, p1);
        if constexpr (HAS_G) load_octet(gp1 + e0, gv1, cnt, g1);
        if (MASK) load_octet(mp1 + e0, mv1, cnt, m1);
      }
      int y = 0, x = 0;  // of element e0 + e
      if (FLOW) {
        y = (int)(e0 / W);
        x = (int)(e0 - (long)y * W);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ge = HAS_G ? g[e] : 0.f;
        bool ok = (e < cnt) & pixel_valid<HAS_G>(p[e], ge, lo, hi, pos);
        if (MASK) ok = ok & (m[e] != 0);
        if (qp) ok = ok & (pm[e] != 0);
        double a1 = 0.0, gg1 = 0.0;
        if (!FLOW) {
          const float g1e = HAS_G ? g1[e] : 0.f;
          ok = ok & pixel_valid<HAS_G>(p1[e], g1e, lo, hi, pos);
          if (MASK) ok = ok & (m1[e] != 0);
          if (ok) a1 = aligned_depth(s1, p1[e], t1, space, clip_lo, clip_hi);
          gg1 = g1e;
        } else if (ok) {
          const float dx = fl[2 * (e0 + e)], dy = fl[2 * (e0 + e) + 1];
          const double X = (double)x + (double)dx, Y = (double)y + (double)dy;
          // every tap of non-zero weight inside the frame ⇔ 0 ≤ X ≤ W − 1 and 0 ≤ Y ≤ H − 1 (a fractional X
          // below W − 1 has x0 + 1 ≤ W − 1); NaN and ±inf fail the comparisons
          ok = (X >= 0.0) & (X <= (double)(W - 1)) & (Y >= 0.0) & (Y <= (double)(H - 1));
          if (ok) {
            const double fx = floor(X), fy = floor(Y), wx = X - fx, wy = Y - fy;
            const int x0 = (int)fx, y0 = (int)fy;
            const bool nx = wx != 0.0, ny = wy != 0.0;
            double a00, a01 = 0.0, a10 = 0.0, a11 = 0.0, g00, g01 = 0.0, g10 = 0.0, g11 = 0.0;
            ok = tap(y0, x0, a00, g00);
            if (nx) ok = ok & tap(y0, x0 + 1, a01, g01);
            if (ny) ok = ok & tap(y0 + 1, x0, a10, g10);
            if (nx & ny) ok = ok & tap(y0 + 1, x0 + 1, a11, g11);
            a1 = bilerp(wx, wy, a00, a01, a10, a11);
            if (HAS_G) gg1 = bilerp(wx, wy, g00, g01, g10, g11);
          }
        }
        if (ok) {
          const double da = a1 - aligned_depth(s0, p[e], t0, space, clip_lo, clip_hi);
          acc[0] += 1.0;
          acc[1] += fabs(da);
          acc[2] = fma(da, da, acc[2]);
          if (HAS_G) {
            const double dg = gg1 - (double)ge, r = da - dg;
            acc[3] += fabs(r);
            acc[4] = fma(r, r, acc[4]);
            acc[5] += fabs(dg);
            acc[6] = fma(dg, dg, acc[6]);
            acc[7] = fma(da, dg, acc[7]);
          }
        }
        if (FLOW) {
          if (++x == W) {
            x = 0;
            ++y;
          }
        }
      }
    }
  }
  block_reduce_store<8>(acc, part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * kRow);
}

// out[f][k] = Σ_b part[f][b][k], b rising (k < K), for all frames: one thread per (f, k) chain, the chains
// first, first + step, ... to this thread
template <int K>
__device__ __forceinline__ void sum_rows(const double* __restrict__ part, int N, int bpf, double* __restrict__ out,
                                         long first, long step) {
  for (long i = first; i < (long)N * K; i += step) {
    const long f = i / K;
    const int k = (int)(i - f * K);
    const double* r = part + f * bpf * kRow + k;
    double v = 0.0;
    for (int b = 0; b < bpf; ++b) v += r[(long)b * kRow];
    out[i] = v;
  }
}

// (s, t) minimising Σ (s·p + t − g)² from the six moments; NaN where they do not determine a fit
__device__ __forceinline__ void solve_fit(const double (&m)[6], double& s, double& t) {
  const double n = m[0], sp = m[1], sg = m[2], spp = m[3], spg = m[4];
  const double det = n * spp - sp * sp;
  if (n < 2.0 || !(det > 0.0)) {
    s = t = __builtin_nan("");
    return;
  }
  s = (n * spg - sp * sg) / det;
  t = (spp * sg - sp * spg) / det;
}

__global__ __launch_bounds__(kFitThreads) void depth_fit_k(const double* __restrict__ part, int N, int bpf, int mode,
                                                        double* __restrict__ moments, double* __restrict__ st) {
  __shared__ double vid[6];
  if (mode == RDMI_FIT_NONE) {
    for (int f = threadIdx.x; f < N; f += blockDim.x) {
      st[2 * f] = 1.0;
      st[2 * f + 1] = 0.0;
    }
    if (!part) return;
  }
  sum_rows<6>(part, N, bpf, moments, threadIdx.x, blockDim.x);
  if (mode == RDMI_FIT_NONE) return;
  __threadfence_block();
  __syncthreads();  // the moments rows are read back below by other threads of this workgroup
  if (mode == RDMI_FIT_FRAME) {
    for (int f = threadIdx.x; f < N; f += blockDim.x) {
      double m[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) m[k] = moments[6 * (long)f + k];
      solve_fit(m, st[2 * f], st[2 * f + 1]);
    }
    return;
  }
  if (threadIdx.x < 6) {  // the video's moments: frames added in frame order
    double v = 0.0;
    for (int f = 0; f < N; ++f) v += moments[6 * (long)f + threadIdx.x];
    vid[threadIdx.x] = v;
  }
  __syncthreads();
  double m[6], s, t;
#pragma unroll
  for (int k = 0; k < 6; ++k) m[k] = vid[k];
  solve_fit(m, s, t);
  for (int f = threadIdx.x; f < N; f += blockDim.x) {
    st[2 * f] = s;
    st[2 * f + 1] = t;
  }
}

// one wave per workgroup, so that the chains spread over the CUs
__global__ __launch_bounds__(64) void depth_error_rows_k(const double* __restrict__ part, int N, int bpf,
                                                         double* __restrict__ sums) {
  sum_rows<8>(part, N, bpf, sums, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}


// the checks the moments and the errors pass share; 0 or RDMI_E_*
int check_inputs(const char* what, const void* pred, int pred_dtype, const void* target, int target_dtype, int N,
                 long P, float lo, float hi, const void* workspace, int space) {
  RDMI_REQUIRE(space_ok(space), RDMI_E_ARG, "%s: unknown space %d", what, space);
  RDMI_REQUIRE(pred && target && workspace, RDMI_E_ARG, "%s: null pointer", what);
  RDMI_REQUIRE(N >= 1 && P >= 1, RDMI_E_ARG, "%s: N (%d) and P (%ld) must be >= 1", what, N, P);
  RDMI_REQUIRE(dtype_ok(pred_dtype) && dtype_ok(target_dtype), RDMI_E_ARG,
               "%s: pred / target dtype %d / %d, f16 or f32 expected", what, pred_dtype, target_dtype);
  RDMI_REQUIRE(lo < hi, RDMI_E_ARG, "%s: valid range needs lo < hi, got %g, %g", what, (double)lo, (double)hi);
  RDMI_REQUIRE(N <= 65535, RDMI_E_UNSUPPORTED, "%s: at most 65535 frames per call, got %d", what, N);
  return 0;
}

// the alignment space as a type: f(integral_constant<int, RDMI_SPACE_*>) for a space that space_ok accepted
template <typename F>
void with_space(int space, F&& f) {
  if (space == RDMI_SPACE_DISPARITY)
    f(std::integral_constant<int, RDMI_SPACE_DISPARITY>{});
  else if (space == RDMI_SPACE_LOG)
    f(std::integral_constant<int, RDMI_SPACE_LOG>{});
  else
    f(std::integral_constant<int, RDMI_SPACE_DEPTH>{});
}

int depth_moments(const char* what, const void* pred, int pred_dtype, const void* target, int target_dtype,
                  const unsigned char* mask, int N, long P, float lo, float hi, int space, double* workspace,
                  void* stream) {
  const int rc = check_inputs(what, pred, pred_dtype, target, target_dtype, N, P, lo, hi, workspace, space);
  if (rc) return rc;
  const dim3 grid(blocks_per_frame(P), N);
  with_input_types(pred_dtype, target_dtype, mask != nullptr, [&](auto tp, auto tg, auto masked) {
    using TP = typename decltype(tp)::type;
    using TG = typename decltype(tg)::type;
    with_space(space, [&](auto sp) {
      hipLaunchKernelGGL((depth_moments_k<TP, TG, decltype(masked)::value, decltype(sp)::value>), grid,
                         dim3(kThreads), 0, (hipStream_t)stream, (const TP*)pred, (const TG*)target, mask, P, lo, hi,
                         workspace);
    });
  });
  return rdmi::check_launch(what);
}

int depth_errors(const char* what, const void* pred, int pred_dtype, const void* target, int target_dtype,
                 const unsigned char* mask, int N, long P, float lo, float hi, const double* st, int space,
                 float clip_lo, float clip_hi, double* workspace, double* sums, void* stream) {
  int rc = check_inputs(what, pred, pred_dtype, target, target_dtype, N, P, lo, hi, workspace, space);
  if (rc) return rc;
  RDMI_REQUIRE(st && sums, RDMI_E_ARG, "%s: null pointer", what);
  RDMI_REQUIRE(clip_lo <= clip_hi, RDMI_E_ARG, "%s: clip needs clip_lo <= clip_hi, got %g, %g", what,
               (double)clip_lo, (double)clip_hi);
  const int bpf = blocks_per_frame(P);
  const dim3 grid(bpf, N);
  with_input_types(pred_dtype, target_dtype, mask != nullptr, [&](auto tp, auto tg, auto masked) {
    using TP = typename decltype(tp)::type;
    using TG = typename decltype(tg)::type;
    with_space(space, [&](auto sp) {
      hipLaunchKernelGGL((depth_errors_k<TP, TG, decltype(masked)::value, decltype(sp)::value>), grid,
                         dim3(kThreads), 0, (hipStream_t)stream, (const TP*)pred, (const TG*)target, mask, P, lo, hi,
                         st, (double)clip_lo, (double)clip_hi, workspace);
    });
  });
  rc = rdmi::check_launch(what);
  if (rc) return rc;
  hipLaunchKernelGGL(depth_error_rows_k, dim3(rdmi::div_up((long)N * 8, 64)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)workspace, N, bpf, sums);
  return rdmi::check_launch("depth_error_rows");
}

}  // namespace

extern "C" long rdmi_depth_metrics_workspace(int N, long P) {
  if (N < 1 || P < 1) return 0;
  return (long)N * blocks_per_frame(P) * kRow;
}

extern "C" int rdmi_depth_moments(const void* pred, int pred_dtype, const void* target, int target_dtype,
                                  const unsigned char* mask, int N, long P, float lo, float hi, double* workspace,
                                  void* stream) {
  return depth_moments("depth_moments", pred, pred_dtype, target, target_dtype, mask, N, P, lo, hi, RDMI_SPACE_DEPTH,
                       workspace, stream);
}

extern "C" int rdmi_depth_moments_space(const void* pred, int pred_dtype, const void* target, int target_dtype,
                                        const unsigned char* mask, int N, long P, float lo, float hi, int space,
                                        double* workspace, void* stream) {
  return depth_moments("depth_moments_space", pred, pred_dtype, target, target_dtype, mask, N, P, lo, hi, space,
                       workspace, stream);
}

extern "C" int rdmi_depth_fit(const double* workspace, int N, long P, int mode, double* moments, double* st,
                              void* stream) {
  RDMI_REQUIRE(mode == RDMI_FIT_NONE || mode == RDMI_FIT_FRAME || mode == RDMI_FIT_VIDEO, RDMI_E_ARG,
               "depth_fit: unknown mode %d", mode);
  RDMI_REQUIRE(N >= 1 && P >= 1, RDMI_E_ARG, "depth_fit: N (%d) and P (%ld) must be >= 1", N, P);
  RDMI_REQUIRE(st && (mode == RDMI_FIT_NONE ? !workspace == !moments : workspace && moments), RDMI_E_ARG,
               "depth_fit: null pointer");
  hipLaunchKernelGGL(depth_fit_k, dim3(1), dim3(kFitThreads), 0, (hipStream_t)stream, workspace, N, blocks_per_frame(P),
                     mode, moments, st);
  return rdmi::check_launch("depth_fit");
}

extern "C" int rdmi_depth_errors(const void* pred, int pred_dtype, const void* target, int target_dtype,
                                 const unsigned char* mask, int N, long P, float lo, float hi, const double* st,
                                 float clip_lo, float clip_hi, double* workspace, double* sums, void* stream) {
  return depth_errors("depth_errors", pred, pred_dtype, target, target_dtype, mask, N, P, lo, hi, st,
                      RDMI_SPACE_DEPTH, clip_lo, clip_hi, workspace, sums, stream);
}

extern "C" int rdmi_depth_errors_space(const void* pred, int pred_dtype, const void* target, int target_dtype,
                                       const unsigned char* mask, int N, long P, float lo, float hi,
                                       const double* st, int space, float clip_lo, float clip_hi, double* workspace,
                                       double* sums, void* stream) {
  return depth_errors("depth_errors_space", pred, pred_dtype, target, target_dtype, mask, N, P, lo, hi, st, space,
                      clip_lo, clip_hi, workspace, sums, stream);
}

extern "C" int rdmi_depth_temporal(const void* pred, int pred_dtype, const void* target, int target_dtype,
                                   const unsigned char* mask, const float* flow, const unsigned char* pair_mask, int N,
                                   int H, int W, int frame_step, float lo, float hi, const double* st, int space,
                                   float clip_lo, float clip_hi, double* workspace, double* sums, void* stream) {
  RDMI_REQUIRE(pred && st && workspace && sums, RDMI_E_ARG, "depth_temporal: null pointer");
  RDMI_REQUIRE(N >= 2 && H >= 1 && W >= 1, RDMI_E_ARG, "depth_temporal: N (%d) must be >= 2, H (%d) and W (%d) >= 1",
               N, H, W);
  RDMI_REQUIRE(frame_step >= 1 && frame_step < N, RDMI_E_ARG, "depth_temporal: frame_step %d outside 1 .. N - 1 = %d",
               frame_step, N - 1);
  RDMI_REQUIRE(dtype_ok(pred_dtype) && (!target || dtype_ok(target_dtype)), RDMI_E_ARG,
               "depth_temporal: pred / target dtype %d / %d, f16 or f32 expected", pred_dtype, target_dtype);
  RDMI_REQUIRE(space_ok(space), RDMI_E_ARG, "depth_temporal: unknown space %d", space);
  RDMI_REQUIRE(!target || lo < hi, RDMI_E_ARG, "depth_temporal: valid range needs lo < hi, got %g, %g", (double)lo,
               (double)hi);
  RDMI_REQUIRE(clip_lo <= clip_hi, RDMI_E_ARG, "depth_temporal: clip needs clip_lo <= clip_hi, got %g, %g",
               (double)clip_lo, (double)clip_hi);
  const int pairs = N - frame_step;
  RDMI_REQUIRE(pairs <= 65535, RDMI_E_UNSUPPORTED,
               "depth_temporal: at most 65535 pairs per call, got N - frame_step = %d", pairs);
  const int bpf = blocks_per_frame((long)H * W);
  const dim3 grid(bpf, pairs);
  auto launch = [&](auto tp, auto tg, auto masked) {
    using TP = typename decltype(tp)::type;
    using TG = typename decltype(tg)::type;
    auto go = [&](auto flowed) {
      hipLaunchKernelGGL((depth_temporal_k<TP, TG, decltype(masked)::value, decltype(flowed)::value>), grid,
                         dim3(kThreads), 0, (hipStream_t)stream, (const TP*)pred, (const TG*)target, mask, flow,
                         pair_mask, H, W, frame_step, lo, hi, st, space, (double)clip_lo, (double)clip_hi, workspace);
    };
    if (flow)
      go(std::true_type{});
    else
      go(std::false_type{});
  };
  if (target) {
    with_input_types(pred_dtype, target_dtype, mask != nullptr, launch);
  } else {  // no target: with_input_types' pred and mask choices with no_target in the middle
    auto with_mask = [&](auto tp) {
      if (mask)
        launch(tp, tag<no_target>{}, std::true_type{});
      else
        launch(tp, tag<no_target>{}, std::false_type{});
    };
    if (pred_dtype == RDMI_F32)
      with_mask(tag<float>{});
    else
      with_mask(tag<f16>{});
  }
  const int rc = rdmi::check_launch("depth_temporal");
  if (rc) return rc;
  hipLaunchKernelGGL(depth_error_rows_k, dim3(rdmi::div_up((long)pairs * 8, 64)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)workspace, pairs, bpf, sums);
  return rdmi::check_launch("depth_error_rows");
}
