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
#include "common.h"

#include <math.h>

#include <type_traits>

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

// Walks this block's octets of frame blockIdx.y and calls f(p, g) for every VALID pixel, in the fixed order.
template <typename TP, typename TG, bool MASK, typename F>
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
      if (ok) f(p[e], g[e]);
    }
  }
}

template <typename TP, typename TG, bool MASK>
__global__ __launch_bounds__(kThreads) void depth_moments_k(const TP* __restrict__ pred,
                                                            const TG* __restrict__ target,
                                                            const unsigned char* __restrict__ mask, long P, float lo,
                                                            float hi, double* __restrict__ part) {
  double acc[6] = {0, 0, 0, 0, 0, 0};  // n, Σp, Σg, Σp², Σpg, Σg²
  for_valid_pixels<TP, TG, MASK>(pred, target, mask, P, lo, hi, [&](float pf, float gf) {
    const double p = pf, g = gf;
    acc[0] += 1.0;
    acc[1] += p;
    acc[2] += g;
    acc[3] = fma(p, p, acc[3]);  // exact products: fma and mul + add round alike
    acc[4] = fma(p, g, acc[4]);
    acc[5] = fma(g, g, acc[5]);
  });
  block_reduce_store<6>(acc, part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * kRow);
}

template <typename TP, typename TG, bool MASK>
__global__ __launch_bounds__(kThreads) void depth_errors_k(const TP* __restrict__ pred, const TG* __restrict__ target,
                                                           const unsigned char* __restrict__ mask, long P, float lo,
                                                           float hi, const double* __restrict__ st, double clip_lo,
                                                           double clip_hi, double* __restrict__ part) {
  // n, Σ|a−g|, Σ|a−g|/g, Σ(a−g)², Σ(a−g)²/g, #δ<1.25, #δ<1.25², #δ<1.25³
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const double s = st[2 * blockIdx.y], t = st[2 * blockIdx.y + 1];
  if (s == s && t == t) {  // a frame without a fit contributes nothing
    for_valid_pixels<TP, TG, MASK>(pred, target, mask, P, lo, hi, [&](float pf, float gf) {
      const double g = gf;
      double a = fma(s, (double)pf, t);
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

bool dtype_ok(int d) { return d == RDMI_F16 || d == RDMI_F32; }

// the checks the moments and the errors pass share; 0 or RDMI_E_*
int check_inputs(const char* what, const void* pred, int pred_dtype, const void* target, int target_dtype, int N,
                 long P, float lo, float hi, const void* workspace) {
  RDMI_REQUIRE(pred && target && workspace, RDMI_E_ARG, "%s: null pointer", what);
  RDMI_REQUIRE(N >= 1 && P >= 1, RDMI_E_ARG, "%s: N (%d) and P (%ld) must be >= 1", what, N, P);
  RDMI_REQUIRE(dtype_ok(pred_dtype) && dtype_ok(target_dtype), RDMI_E_ARG,
               "%s: pred / target dtype %d / %d, f16 or f32 expected", what, pred_dtype, target_dtype);
  RDMI_REQUIRE(lo < hi, RDMI_E_ARG, "%s: valid range needs lo < hi, got %g, %g", what, (double)lo, (double)hi);
  RDMI_REQUIRE(N <= 65535, RDMI_E_UNSUPPORTED, "%s: at most 65535 frames per call, got %d", what, N);
  return 0;
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

extern "C" long rdmi_depth_metrics_workspace(int N, long P) {
  if (N < 1 || P < 1) return 0;
  return (long)N * blocks_per_frame(P) * kRow;
}

extern "C" int rdmi_depth_moments(const void* pred, int pred_dtype, const void* target, int target_dtype,
                                  const unsigned char* mask, int N, long P, float lo, float hi, double* workspace,
                                  void* stream) {
  const int rc = check_inputs("depth_moments", pred, pred_dtype, target, target_dtype, N, P, lo, hi, workspace);
  if (rc) return rc;
  const dim3 grid(blocks_per_frame(P), N);
  with_input_types(pred_dtype, target_dtype, mask != nullptr, [&](auto tp, auto tg, auto masked) {
    using TP = typename decltype(tp)::type;
    using TG = typename decltype(tg)::type;
    hipLaunchKernelGGL((depth_moments_k<TP, TG, decltype(masked)::value>), grid, dim3(kThreads), 0,
                       (hipStream_t)stream, (const TP*)pred, (const TG*)target, mask, P, lo, hi, workspace);
  });
  return rdmi::check_launch("depth_moments");
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
  int rc = check_inputs("depth_errors", pred, pred_dtype, target, target_dtype, N, P, lo, hi, workspace);
  if (rc) return rc;
  RDMI_REQUIRE(st && sums, RDMI_E_ARG, "depth_errors: null pointer");
  RDMI_REQUIRE(clip_lo <= clip_hi, RDMI_E_ARG, "depth_errors: clip needs clip_lo <= clip_hi, got %g, %g",
               (double)clip_lo, (double)clip_hi);
  const int bpf = blocks_per_frame(P);
  const dim3 grid(bpf, N);
  with_input_types(pred_dtype, target_dtype, mask != nullptr, [&](auto tp, auto tg, auto masked) {
    using TP = typename decltype(tp)::type;
    using TG = typename decltype(tg)::type;
    hipLaunchKernelGGL((depth_errors_k<TP, TG, decltype(masked)::value>), grid, dim3(kThreads), 0,
                       (hipStream_t)stream, (const TP*)pred, (const TG*)target, mask, P, lo, hi, st, (double)clip_lo,
                       (double)clip_hi, workspace);
  });
  rc = rdmi::check_launch("depth_errors");
  if (rc) return rc;
  hipLaunchKernelGGL(depth_error_rows_k, dim3(rdmi::div_up((long)N * 8, 64)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)workspace, N, bpf, sums);
  return rdmi::check_launch("depth_error_rows");
}
