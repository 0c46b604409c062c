// Dense pyramidal Lucas–Kanade optical flow and the forward–backward check (since rdmi_version 10); the algorithm,
// operation by operation, is fixed in include/rdmi.h "Optical flow" and restated in f64 by tests/flow_util.py.
//
// luma_k, down_k: one output pixel per thread, grid-strided — HBM-bound row kernels like the elementwise family.
// lk_level_k, the hot path: a workgroup of kTileW × kTileH = 256 lanes owns that pixel tile of one pair.  It stages I0
// with an r + 1 halo (indices clamped to the image, which is exactly the clamped central difference's operand) in
// LDS, derives {Ix, Iy, I0} per halo-r position into one 16-byte LDS slot, and every lane then builds its structure
// tensor from LDS and runs all iterations with u, A and b in registers: no launch per iteration, no atomics, a
// fixed row-major summation order per lane.  A wave covers two tile rows of 32 consecutive pixels: its LDS reads
// are consecutive 16-byte slots (conflict-free ds_read_b128) and its I1 taps, plain cached global loads, fall on
// neighbouring addresses when the flow is smooth.  An LDS-staged I1 window has not been built or measured.
#include "common.h"

namespace {

constexpr int kTileW = 32, kTileH = 8, kBlock = kTileW * kTileH;
constexpr int kMaxR = RDMI_FLOW_MAX_RADIUS;
constexpr int kMaxLevels = RDMI_FLOW_MAX_LEVELS;
constexpr int kRawW = kTileW + 2 * (kMaxR + 1), kRawH = kTileH + 2 * (kMaxR + 1);  // I0, halo r + 1
constexpr int kGrW = kTileW + 2 * kMaxR, kGrH = kTileH + 2 * kMaxR;                // {Ix, Iy, I0}, halo r
constexpr long kMaxHW = 1L << 30;
constexpr int kGridCap = 16384;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// fmaxf / fminf return the other operand for a NaN: the result is always a finite value in [0, hi].  (float)(W − 1)
// can round up above 2^24, so the integer index taken from it is clamped once more.
__device__ __forceinline__ float clampf(float v, float hi) { return fminf(fmaxf(v, 0.0f), hi); }

template <typename T>
__global__ void luma_k(const T* __restrict__ x, long sn, long sc, long sy, long sx, int N, int H, int W,
                       float* __restrict__ out) {
  const long hw = (long)H * W, total = hw * N;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / hw;
    const int p = (int)(i - n * hw), y = p / W, xx = p - y * W;
    const T* q = x + n * sn + y * sy + xx * sx;
    const float r = (float)q[0], g = (float)q[sc], b = (float)q[2 * sc];
    out[i] = (0.299f * r + 0.587f * g) + 0.114f * b;
  }
}

// in [N][H][W] → out [N][Ho][Wo], Ho = ⌈H/2⌉, Wo = ⌈W/2⌉
__global__ void down_k(const float* __restrict__ in, int N, int H, int W, int Ho, int Wo, float* __restrict__ out) {
  const long hwo = (long)Ho * Wo, total = hwo * N;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / hwo;
    const int p = (int)(i - n * hwo), y = p / Wo, x = p - y * Wo;
    const float* f = in + n * ((long)H * W);
    const int y0 = 2 * y, y1 = min(2 * y + 1, H - 1), x0 = 2 * x, x1 = min(2 * x + 1, W - 1);
    const float a = f[y0 * W + x0], b = f[y0 * W + x1], c = f[y1 * W + x0], d = f[y1 * W + x1];
    out[i] = 0.25f * ((a + b) + (c + d));
  }
}

// (1 − wy)·((1 − wx)·v00 + wx·v01) + wy·((1 − wx)·v10 + wx·v11)
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float wx, float wy) {
  const float ux = 1.0f - wx, uy = 1.0f - wy;
  return uy * (ux * v00 + wx * v01) + wy * (ux * v10 + wx * v11);
}

__global__ __launch_bounds__(kBlock) void lk_level_k(const float* __restrict__ img, int H, int W, int first0,
                                                     int first1, const float* __restrict__ coarse, int Hc, int Wc,
                                                     float* __restrict__ flow, int r, int iterations, float damping,
                                                     int tiles_x) {
  __shared__ float raw[kRawH * kRawW];
  __shared__ f32x4 grad[kGrH * kGrW];
  const int pair = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x_base = tx * kTileW, y_base = ty * kTileH;
  const long hw = (long)H * W;
  const float* __restrict__ I0 = img + (long)(first0 + pair) * hw;  // 64-bit frame bases
  const float* __restrict__ I1 = img + (long)(first1 + pair) * hw;

  const int rw = kTileW + 2 * (r + 1), rh = kTileH + 2 * (r + 1);
  for (int i = threadIdx.x; i < rw * rh; i += kBlock) {
    const int ly = i / rw, lx = i - ly * rw;
    const int gy = clampi(y_base - (r + 1) + ly, H - 1), gx = clampi(x_base - (r + 1) + lx, W - 1);
    raw[ly * kRawW + lx] = I0[gy * W + gx];
  }
  __syncthreads();
  const int gw = kTileW + 2 * r, gh = kTileH + 2 * r;
  for (int i = threadIdx.x; i < gw * gh; i += kBlock) {
    const int ly = i / gw, lx = i - ly * gw;
    const float* c = &raw[(ly + 1) * kRawW + (lx + 1)];
    grad[ly * kGrW + lx] = f32x4{0.5f * (c[1] - c[-1]), 0.5f * (c[kRawW] - c[-kRawW]), c[0], 0.0f};
  }
  __syncthreads();

  const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
  const int px = x_base + lx, py = y_base + ly;
  if (px >= W || py >= H) return;
  // the window's taps inside the image, as offsets from p
  const int j_lo = max(-r, -py), j_hi = min(r, H - 1 - py), i_lo = max(-r, -px), i_hi = min(r, W - 1 - px);
  const f32x4* __restrict__ gp = &grad[(ly + r) * kGrW + (lx + r)];

  float axx = 0.0f, axy = 0.0f, ayy = 0.0f;
  for (int j = j_lo; j <= j_hi; ++j)
    for (int i = i_lo; i <= i_hi; ++i) {
      const f32x4 g = gp[j * kGrW + i];
      axx += g[0] * g[0];
      axy += g[0] * g[1];
      ayy += g[1] * g[1];
    }
  const float lam = damping * (0.5f * (axx + ayy)) + 1e-12f;
  const float a11 = axx + lam, a22 = ayy + lam;
  const float det = a11 * a22 - axy * axy;

  float ux = 0.0f, uy = 0.0f;
  if (coarse) {
    const float* __restrict__ cf = coarse + (long)pair * ((long)Hc * Wc) * 2;
    const float X = clampf(((float)px + 0.5f) * 0.5f - 0.5f, (float)(Wc - 1));
    const float Y = clampf(((float)py + 0.5f) * 0.5f - 0.5f, (float)(Hc - 1));
    const int x0 = min((int)X, Wc - 1), y0 = min((int)Y, Hc - 1), x1 = min(x0 + 1, Wc - 1), y1 = min(y0 + 1, Hc - 1);
    const float wx = X - (float)x0, wy = Y - (float)y0;
    const f32x2 c00 = *(const f32x2*)&cf[2 * (y0 * Wc + x0)], c01 = *(const f32x2*)&cf[2 * (y0 * Wc + x1)];
    const f32x2 c10 = *(const f32x2*)&cf[2 * (y1 * Wc + x0)], c11 = *(const f32x2*)&cf[2 * (y1 * Wc + x1)];
    ux = 2.0f * bilerp(c00[0], c01[0], c10[0], c11[0], wx, wy);
    uy = 2.0f * bilerp(c00[1], c01[1], c10[1], c11[1], wx, wy);
  }

  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
#pragma unroll 1
  for (int it = 0; it < iterations; ++it) {
    float bx = 0.0f, by = 0.0f;
    for (int j = j_lo; j <= j_hi; ++j) {
      const float Y = clampf((float)(py + j) + uy, hmax);
      const int y0 = min((int)Y, H - 1), y1 = min(y0 + 1, H - 1);
      const float wy = Y - (float)y0;
      const float* __restrict__ r0 = I1 + y0 * W;
      const float* __restrict__ r1 = I1 + y1 * W;
      for (int i = i_lo; i <= i_hi; ++i) {
        const float X = clampf((float)(px + i) + ux, wmax);
        const int x0 = min((int)X, W - 1), x1 = min(x0 + 1, W - 1);
        const float wx = X - (float)x0;
        const float v = bilerp(r0[x0], r0[x1], r1[x0], r1[x1], wx, wy);
        const f32x4 g = gp[j * kGrW + i];
        const float d = v - g[2];
        bx += g[0] * d;
        by += g[1] * d;
      }
    }
    float dux = -(a22 * bx - axy * by) / det;
    float duy = -(a11 * by - axy * bx) / det;
    const float n = sqrtf(dux * dux + duy * duy);
    if (n > 1.0f) {
      dux = dux / n;
      duy = duy / n;
    }
    ux += dux;
    uy += duy;
  }
  *(f32x2*)&flow[((long)pair * hw + (long)py * W + px) * 2] = f32x2{ux, uy};
}

__global__ void fb_check_k(const float* __restrict__ fwd, const float* __restrict__ bwd, int pairs, int H, int W,
                           float alpha, float beta, unsigned char* __restrict__ valid) {
  const long hw = (long)H * W, total = hw * pairs;
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / hw;
    const int p = (int)(i - n * hw), y = p / W, x = p - y * W;
    const f32x2 uf = *(const f32x2*)&fwd[2 * i];
    const float X = (float)x + uf[0], Y = (float)y + uf[1];
    unsigned char ok = 0;
    if (X >= 0.0f && X <= wmax && Y >= 0.0f && Y <= hmax) {  // false for a NaN: no address is formed from one
      const float* __restrict__ b = bwd + n * hw * 2;
      const int x0 = min((int)X, W - 1), y0 = min((int)Y, H - 1), x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
      const float wx = X - (float)x0, wy = Y - (float)y0;
      const f32x2 c00 = *(const f32x2*)&b[2 * (y0 * W + x0)], c01 = *(const f32x2*)&b[2 * (y0 * W + x1)];
      const f32x2 c10 = *(const f32x2*)&b[2 * (y1 * W + x0)], c11 = *(const f32x2*)&b[2 * (y1 * W + x1)];
      const float bx = bilerp(c00[0], c01[0], c10[0], c11[0], wx, wy);
      const float by = bilerp(c00[1], c01[1], c10[1], c11[1], wx, wy);
      const float sx = uf[0] + bx, sy = uf[1] + by;
      const float lhs = sx * sx + sy * sy;
      const float rhs = alpha * ((uf[0] * uf[0] + uf[1] * uf[1]) + (bx * bx + by * by)) + beta;
      ok = lhs <= rhs ? 1 : 0;
    }
    valid[i] = ok;
  }
}

inline int half_up(int v) { return (v + 1) / 2; }

int level_count(int H, int W, int r, int levels) {
  if (H < 1 || W < 1 || r < 1 || r > kMaxR) return 0;
  const int s = 4 * (2 * r + 1);
  int n = 1, h = half_up(H), w = half_up(W);
  while (n < kMaxLevels && (h < w ? h : w) >= s) {
    ++n;
    h = half_up(h);
    w = half_up(w);
  }
  return levels >= 1 && levels < n ? levels : n;
}

inline unsigned grid_for(long total) {
  long g = (total + 255) / 256;
  return (unsigned)(g > kGridCap ? kGridCap : g);
}

#define FLOW_SIZES(name)                                                                                     \
  RDMI_REQUIRE(H >= 1 && W >= 1, RDMI_E_ARG, name ": H (%d) and W (%d) must be positive", H, W);            \
  RDMI_REQUIRE((long)H * W <= kMaxHW, RDMI_E_UNSUPPORTED, name ": H·W = %ld above 2^30", (long)H * W)
#define FLOW_RADIUS(name) \
  RDMI_REQUIRE(radius >= 1 && radius <= kMaxR, RDMI_E_ARG, name ": radius %d outside 1 … %d", radius, kMaxR)
#define FLOW_ALIGNED(name, p, a, what) \
  RDMI_REQUIRE(((uintptr_t)(p) & ((a) - 1)) == 0, RDMI_E_ALIGN, name ": " what " not %d-byte aligned", (int)(a))

int launch_pyramid(const void* frames, int dtype, long sn, long sc, long sy, long sx, int N, int H, int W,
                   int levels, float* pyr, hipStream_t s) {
  const long total = (long)N * H * W;
  const dim3 g(grid_for(total)), b(256);
  if (dtype == RDMI_F32)
    hipLaunchKernelGGL(luma_k<float>, g, b, 0, s, (const float*)frames, sn, sc, sy, sx, N, H, W, pyr);
  else if (dtype == RDMI_F16)
    hipLaunchKernelGGL(luma_k<f16>, g, b, 0, s, (const f16*)frames, sn, sc, sy, sx, N, H, W, pyr);
  else
    hipLaunchKernelGGL(luma_k<unsigned char>, g, b, 0, s, (const unsigned char*)frames, sn, sc, sy, sx, N, H, W,
                       pyr);
  int rc = rdmi::check_launch("flow_luma");
  int h = H, w = W;
  float* src = pyr;
  for (int l = 1; l < levels && !rc; ++l) {
    const int ho = half_up(h), wo = half_up(w);
    float* dst = src + (long)N * h * w;
    hipLaunchKernelGGL(down_k, dim3(grid_for((long)N * ho * wo)), dim3(256), 0, s, src, N, h, w, ho, wo, dst);
    rc = rdmi::check_launch("flow_down");
    src = dst;
    h = ho;
    w = wo;
  }
  return rc;
}

int launch_lk(const float* img, int Hl, int Wl, int first0, int first1, int pairs, const float* coarse, int Hc,
              int Wc, float* flow, int radius, int iterations, float damping, hipStream_t s) {
  const int tiles_x = rdmi::div_up(Wl, kTileW), tiles_y = rdmi::div_up(Hl, kTileH);
  hipLaunchKernelGGL(lk_level_k, dim3((unsigned)(tiles_x * tiles_y), (unsigned)pairs), dim3(kBlock), 0, s, img, Hl,
                     Wl, first0, first1, coarse, Hc, Wc, flow, radius, iterations, damping, tiles_x);
  return rdmi::check_launch("flow_lk_level");
}

int launch_fb(const float* fwd, const float* bwd, int pairs, int H, int W, float alpha, float beta,
              unsigned char* valid, hipStream_t s) {
  hipLaunchKernelGGL(fb_check_k, dim3(grid_for((long)pairs * H * W)), dim3(256), 0, s, fwd, bwd, pairs, H, W, alpha,
                     beta, valid);
  return rdmi::check_launch("flow_fb_check");
}

// floats of pyramid levels [0, levels) of N frames, and of one direction's flows of the levels above 0
void layout(int N, int H, int W, int pairs, int levels, long* pyr_floats, long* coarse_floats) {
  long pf = 0, cf = 0;
  int h = H, w = W;
  for (int l = 0; l < levels; ++l) {
    pf += (long)N * h * w;
    if (l > 0) cf += (long)pairs * h * w * 2;
    h = half_up(h);
    w = half_up(w);
  }
  *pyr_floats = (pf + 3) / 4 * 4;  // keeps what follows 16-byte aligned
  *coarse_floats = (cf + 3) / 4 * 4;
}

}  // namespace

extern "C" int rdmi_flow_levels(int H, int W, int radius, int levels) { return level_count(H, W, radius, levels); }

extern "C" long rdmi_flow_workspace(int N, int H, int W, int frame_step, int radius, int levels, int backward) {
  if (N < 2 || H < 1 || W < 1 || (long)H * W > kMaxHW || frame_step < 1 || frame_step >= N || radius < 1 ||
      radius > kMaxR || levels > kMaxLevels)
    return 0;
  if (levels < 1) levels = level_count(H, W, radius, 0);
  long pf, cf;
  layout(N, H, W, N - frame_step, levels, &pf, &cf);
  return (pf + cf * (backward ? 2 : 1)) * 4;
}

extern "C" int rdmi_flow_pyramid(const void* frames, int dtype, long stride_n, long stride_c, long stride_y,
                                 long stride_x, int N, int H, int W, int levels, float* pyr, void* stream) {
  RDMI_REQUIRE(frames && pyr, RDMI_E_ARG, "flow_pyramid: null pointer");
  RDMI_REQUIRE(N >= 1, RDMI_E_ARG, "flow_pyramid: N (%d) must be positive", N);
  FLOW_SIZES("flow_pyramid");
  RDMI_REQUIRE(dtype == RDMI_F16 || dtype == RDMI_F32 || dtype == RDMI_U8, RDMI_E_ARG,
               "flow_pyramid: dtype %d (f16, f32 or u8)", dtype);
  RDMI_REQUIRE(levels >= 1 && levels <= kMaxLevels, RDMI_E_ARG, "flow_pyramid: levels %d outside 1 … %d", levels,
               kMaxLevels);
  FLOW_ALIGNED("flow_pyramid", pyr, 4, "pyr");
  return launch_pyramid(frames, dtype, stride_n, stride_c, stride_y, stride_x, N, H, W, levels, pyr,
                        (hipStream_t)stream);
}

extern "C" int rdmi_flow_lk_level(const float* img, int N, int Hl, int Wl, int first0, int first1, int pairs,
                                  const float* coarse, int Hc, int Wc, float* flow, int radius, int iterations,
                                  float damping, void* stream) {
  const int H = Hl, W = Wl;
  RDMI_REQUIRE(img && flow, RDMI_E_ARG, "flow_lk_level: null pointer");
  RDMI_REQUIRE(N >= 1 && pairs >= 1, RDMI_E_ARG, "flow_lk_level: N (%d) and pairs (%d) must be positive", N, pairs);
  FLOW_SIZES("flow_lk_level");
  RDMI_REQUIRE(first0 >= 0 && first1 >= 0 && (long)first0 + pairs <= N && (long)first1 + pairs <= N, RDMI_E_ARG,
               "flow_lk_level: frames %d / %d + %d pairs outside the %d frames", first0, first1, pairs, N);
  FLOW_RADIUS("flow_lk_level");
  RDMI_REQUIRE(iterations >= 1, RDMI_E_ARG, "flow_lk_level: iterations (%d) must be positive", iterations);
  RDMI_REQUIRE(damping >= 0.0f, RDMI_E_ARG, "flow_lk_level: damping %g (>= 0 expected)", (double)damping);
  RDMI_REQUIRE(!coarse || (Hc == half_up(Hl) && Wc == half_up(Wl)), RDMI_E_ARG,
               "flow_lk_level: coarse size %d x %d is not the halved %d x %d", Hc, Wc, half_up(Hl), half_up(Wl));
  RDMI_REQUIRE(pairs <= 65535, RDMI_E_UNSUPPORTED, "flow_lk_level: %d pairs (at most 65535 pairs)", pairs);
  FLOW_ALIGNED("flow_lk_level", img, 4, "img");
  FLOW_ALIGNED("flow_lk_level", flow, 8, "flow");
  FLOW_ALIGNED("flow_lk_level", coarse, 8, "coarse");
  return launch_lk(img, Hl, Wl, first0, first1, pairs, coarse, Hc, Wc, flow, radius, iterations, damping,
                   (hipStream_t)stream);
}

extern "C" int rdmi_flow_fb_check(const float* fwd, const float* bwd, int pairs, int H, int W, float alpha,
                                  float beta, unsigned char* valid, void* stream) {
  RDMI_REQUIRE(fwd && bwd && valid, RDMI_E_ARG, "flow_fb_check: null pointer");
  RDMI_REQUIRE(pairs >= 1, RDMI_E_ARG, "flow_fb_check: pairs (%d) must be positive", pairs);
  FLOW_SIZES("flow_fb_check");
  RDMI_REQUIRE(alpha >= 0.0f && beta >= 0.0f, RDMI_E_ARG, "flow_fb_check: tolerance (%g, %g) (>= 0 expected)",
               (double)alpha, (double)beta);
  FLOW_ALIGNED("flow_fb_check", fwd, 8, "fwd");
  FLOW_ALIGNED("flow_fb_check", bwd, 8, "bwd");
  return launch_fb(fwd, bwd, pairs, H, W, alpha, beta, valid, (hipStream_t)stream);
}

extern "C" int rdmi_flow_estimate(const void* frames, int dtype, long stride_n, long stride_c, long stride_y,
                                  long stride_x, int N, int H, int W, int frame_step, int levels, int radius,
                                  int iterations, float damping, int backward, float alpha, float beta, float* flow,
                                  float* flow_bwd, unsigned char* valid, void* workspace, void* stream) {
  RDMI_REQUIRE(frames && flow && workspace && (!backward || (flow_bwd && valid)), RDMI_E_ARG,
               "flow_estimate: null pointer");
  RDMI_REQUIRE(N >= 2, RDMI_E_ARG, "flow_estimate: N (%d) must be at least 2", N);
  FLOW_SIZES("flow_estimate");
  RDMI_REQUIRE(frame_step >= 1 && frame_step < N, RDMI_E_ARG, "flow_estimate: frame_step %d outside 1 … N - 1 = %d",
               frame_step, N - 1);
  RDMI_REQUIRE(dtype == RDMI_F16 || dtype == RDMI_F32 || dtype == RDMI_U8, RDMI_E_ARG,
               "flow_estimate: dtype %d (f16, f32 or u8)", dtype);
  FLOW_RADIUS("flow_estimate");
  RDMI_REQUIRE(levels <= kMaxLevels, RDMI_E_ARG, "flow_estimate: levels %d above %d", levels, kMaxLevels);
  RDMI_REQUIRE(iterations >= 1, RDMI_E_ARG, "flow_estimate: iterations (%d) must be positive", iterations);
  RDMI_REQUIRE(damping >= 0.0f, RDMI_E_ARG, "flow_estimate: damping %g (>= 0 expected)", (double)damping);
  RDMI_REQUIRE(alpha >= 0.0f && beta >= 0.0f, RDMI_E_ARG, "flow_estimate: tolerance (%g, %g) (>= 0 expected)",
               (double)alpha, (double)beta);
  const int pairs = N - frame_step;
  RDMI_REQUIRE(pairs <= 65535, RDMI_E_UNSUPPORTED, "flow_estimate: %d pairs (at most 65535 pairs)", pairs);
  FLOW_ALIGNED("flow_estimate", workspace, 16, "workspace");
  FLOW_ALIGNED("flow_estimate", flow, 8, "flow");
  FLOW_ALIGNED("flow_estimate", flow_bwd, 8, "flow_bwd");
  if (levels < 1) levels = level_count(H, W, radius, 0);
  hipStream_t s = (hipStream_t)stream;
  long pf, cf;
  layout(N, H, W, pairs, levels, &pf, &cf);
  float* pyr = (float*)workspace;
  float* cbuf[2] = {pyr + pf, pyr + pf + cf};
  int rc = launch_pyramid(frames, dtype, stride_n, stride_c, stride_y, stride_x, N, H, W, levels, pyr, s);
  // per level: its size, its pyramid offset, and the offset of its flow inside a direction's coarse buffer
  int hs[kMaxLevels], wsz[kMaxLevels];
  long poff[kMaxLevels], coff[kMaxLevels];
  {
    int h = H, w = W;
    long po = 0, co = 0;
    for (int l = 0; l < levels; ++l) {
      hs[l] = h;
      wsz[l] = w;
      poff[l] = po;
      coff[l] = co;
      po += (long)N * h * w;
      if (l > 0) co += (long)pairs * h * w * 2;
      h = half_up(h);
      w = half_up(w);
    }
  }
  for (int l = levels - 1; l >= 0 && !rc; --l)
    for (int dir = 0; dir < (backward ? 2 : 1) && !rc; ++dir) {
      float* out = l > 0 ? cbuf[dir] + coff[l] : (dir ? flow_bwd : flow);
      const float* coarse = l + 1 < levels ? cbuf[dir] + coff[l + 1] : nullptr;
      rc = launch_lk(pyr + poff[l], hs[l], wsz[l], dir ? frame_step : 0, dir ? 0 : frame_step, pairs, coarse,
                     coarse ? hs[l + 1] : 0, coarse ? wsz[l + 1] : 0, out, radius, iterations, damping, s);
    }
  if (!rc && backward) rc = launch_fb(flow, flow_bwd, pairs, H, W, alpha, beta, valid, s);
  return rc;
}
