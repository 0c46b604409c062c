// Joint bilateral upsampling (Kopf et al. 2007) of low-resolution maps along a full-resolution guide (since
// rdmi_version 11); the arithmetic, operation by operation, is fixed in include/rdmi.h "Guided upsampling" and
// restated in f64 and f32 by tests/upsample_util.py.
//
// jbu_k<R>: a workgroup of 256 lanes owns a kTileH × kTileW = 16 × 64 tile of output pixels of one frame.  The tile's
// low-resolution footprint (at most kTileH + 2R + 1 rows of kTileW + 2R + 1 columns, because h ≤ H and w ≤ W) is
// staged once in LDS: one 16-byte slot {g0, g1, g2, v0} per low-resolution pixel plus one f32 plane per further value
// channel, 45 KiB at R = 3 whatever C is (the 193 VGPRs of R = 3 allow two workgroups per CU, the LDS three; R = 1
// and 2 run four and three).  A wave owns four output rows and a lane one
// output column of them: the 64 lanes of a tap read share the low-resolution row and their columns never fall, rise
// by at most one from lane to lane, and repeat (broadcast) wherever they do not rise, so a wave's ds_read_b128 touches
// consecutive slots (at the 0.53 of 576 → 1080 the 28 lanes a lane group spans cover 16 slots = 64 banks) and its
// ds_read_b32 of a further channel consecutive banks.  The (2R)² exponents and the channel-0 values of a pixel stay
// in registers: the minimum and the weights are passes over registers.  The guide pixel and the staging are plain
// element loads (no wide path, so no alignment case), the store is one coalesced f32 row per wave.
#include "common.h"

#include <float.h>
#include <limits.h>
#include <math.h>

namespace {

constexpr int kTileW = 64, kTileH = 16, kBlock = 256, kRows = kTileH / (kBlock / kTileW);  // rows per lane
constexpr int kMaxC = 4;
constexpr double kLog2e = 1.4426950408889634074;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// source coordinate of output index i: ((i + 0.5)·scale − 0.5), every operation rounded once (no contraction)
__device__ __forceinline__ float src_coord(int i, float scale) {
  return __fsub_rn(__fmul_rn((float)i + 0.5f, scale), 0.5f);
}
__device__ __forceinline__ float ldg(const unsigned char* p, long o) { return (float)p[o]; }
__device__ __forceinline__ float ldg(const float* p, long o) { return p[o]; }
__device__ __forceinline__ float ldv(const f16* p, long o) { return (float)p[o]; }
__device__ __forceinline__ float ldv(const float* p, long o) { return p[o]; }

template <int R, typename VT, typename GT>
__global__ __launch_bounds__(kBlock) void jbu_k(const VT* __restrict__ values, const float* __restrict__ guide_lo,
                                                const GT* __restrict__ guide_hi, long sn, long sc, long sy, long sx,
                                                float guide_scale, int C, int h, int w, int H, int W, float scale_y,
                                                float scale_x, float cs, float cr, int tiles_x, int tiles,
                                                float* __restrict__ out) {
  constexpr int T = 2 * R, kFH = kTileH + T + 1, kFW = kTileW + T + 1;
  __shared__ f32x4 slot[kFH * kFW];
  __shared__ float extra[(kMaxC - 1) * kFH * kFW];

  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int Y0 = ty * kTileH, X0 = tx * kTileW;
  const int Y1 = min(Y0 + kTileH, H) - 1, X1 = min(X0 + kTileW, W) - 1;
  // the coordinate is monotone in the output index, so the tile's first and last pixel bound its footprint
  const int fy0 = max((int)floorf(src_coord(Y0, scale_y)) - R + 1, 0);
  const int fx0 = max((int)floorf(src_coord(X0, scale_x)) - R + 1, 0);
  const int fy1 = min(min((int)floorf(src_coord(Y1, scale_y)) + R, h - 1), fy0 + kFH - 1);
  const int fx1 = min(min((int)floorf(src_coord(X1, scale_x)) + R, w - 1), fx0 + kFW - 1);
  const int fh = fy1 - fy0 + 1, fw = fx1 - fx0 + 1;

  const long hw = (long)h * w;
  const float* __restrict__ gl = guide_lo + (long)n * 3 * hw;
  const VT* __restrict__ vl = values + (long)n * C * hw;
  for (int i = threadIdx.x; i < fh * fw; i += kBlock) {
    const int ly = i / fw, lx = i - ly * fw;
    const long src = (long)(fy0 + ly) * w + (fx0 + lx);
    const int dst = ly * kFW + lx;
    slot[dst] = f32x4{gl[src], gl[hw + src], gl[2 * hw + src], ldv(vl, src)};
    for (int k = 1; k < C; ++k) extra[(k - 1) * (kFH * kFW) + dst] = ldv(vl, k * hw + src);
  }
  __syncthreads();

  const int X = X0 + (threadIdx.x & (kTileW - 1));
  if (X >= W) return;
  const float inf = __builtin_inff();
  // the column taps of this lane: (qx − xl)²·cs, whether qx lies inside the image, and its LDS column
  const float xl = src_coord(X, scale_x);
  const int x0 = (int)floorf(xl);
  float ex[T];
  int cx[T];
  bool vx[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int qx = x0 - R + 1 + j;
    const float d = __fsub_rn((float)qx, xl);
    ex[j] = __fmul_rn(__fmul_rn(d, d), cs);
    vx[j] = qx >= 0 && qx < w;
    cx[j] = clampi(qx, fx0, fx1) - fx0;
  }
  const int cb = clampi(min(max(x0, 0), w - 1), fx0, fx1) - fx0;  // the base tap's column: x0 brought into the image

  const int row0 = Y0 + (threadIdx.x / kTileW) * kRows;
  const long HW = (long)H * W;
#pragma unroll 1
  for (int p = 0; p < kRows; ++p) {
    const int Y = row0 + p;
    if (Y >= H) return;
    const long go = (long)n * sn + (long)Y * sy + (long)X * sx;
    const float g0 = __fmul_rn(ldg(guide_hi, go), guide_scale);
    const float g1 = __fmul_rn(ldg(guide_hi, go + sc), guide_scale);
    const float g2 = __fmul_rn(ldg(guide_hi, go + 2 * sc), guide_scale);
    const float yl = src_coord(Y, scale_y);
    const int y0 = (int)floorf(yl);

    float e[T * T], v[T * T];
    int ry[T];
    float m = inf;
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const int qy = y0 - R + 1 + i;
      const float d = __fsub_rn((float)qy, yl);
      const float ey = __fmul_rn(__fmul_rn(d, d), cs);
      const bool vy = qy >= 0 && qy < h;
      ry[i] = (clampi(qy, fy0, fy1) - fy0) * kFW;
#pragma unroll
      for (int j = 0; j < T; ++j) {
        const f32x4 s = slot[ry[i] + cx[j]];
        const float d0 = __fsub_rn(g0, s[0]), d1 = __fsub_rn(g1, s[1]), d2 = __fsub_rn(g2, s[2]);
        const float dr = fmaf(d2, d2, fmaf(d1, d1, __fmul_rn(d0, d0)));
        const float q = fminf(fmaf(dr, cr, __fadd_rn(ey, ex[j])), FLT_MAX);  // also takes a NaN of 0·inf to FLT_MAX
        e[i * T + j] = (vy && vx[j]) ? q : inf;
        v[i * T + j] = s[3];
        m = fminf(m, e[i * T + j]);
      }
    }
    // the sums run over v − v_base, v_base the value at the base tap (y0, x0 brought into the image: always a tap):
    // a constant plane comes out exactly and the rounding errors scale with the taps' range, not with |v|
    const int rb = (clampi(min(max(y0, 0), h - 1), fy0, fy1) - fy0) * kFW + cb;
    const float vb = slot[rb][3];
    float sw = 0.0f, acc = 0.0f;
#pragma unroll
    for (int q = 0; q < T * T; ++q) {
      e[q] = __builtin_amdgcn_exp2f(__fsub_rn(m, e[q]));  // 1 at the minimum, 0 for a skipped tap
      sw = __fadd_rn(sw, e[q]);
      acc = fmaf(e[q], __fsub_rn(v[q], vb), acc);
    }
    const long oo = (long)n * C * HW + (long)Y * W + X;
    out[oo] = __fadd_rn(vb, __fdiv_rn(acc, sw));
#pragma unroll 1
    for (int k = 1; k < C; ++k) {
      const float* __restrict__ pl = &extra[(k - 1) * (kFH * kFW)];
      const float vk = pl[rb];
      float a = 0.0f;
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) a = fmaf(e[i * T + j], __fsub_rn(pl[ry[i] + cx[j]], vk), a);
      out[oo + k * HW] = __fadd_rn(vk, __fdiv_rn(a, sw));
    }
  }
}

template <int R, typename VT, typename GT>
void launch(const void* values, const float* guide_lo, const void* guide_hi, long sn, long sc, long sy, long sx,
            float guide_scale, int N, int C, int h, int w, int H, int W, float cs, float cr, int tiles_x, int tiles,
            float* out, hipStream_t s) {
  hipLaunchKernelGGL((jbu_k<R, VT, GT>), dim3((unsigned)((long)tiles * N)), dim3(kBlock), 0, s, (const VT*)values,
                     guide_lo, (const GT*)guide_hi, sn, sc, sy, sx, guide_scale, C, h, w, H, W, (float)h / (float)H,
                     (float)w / (float)W, cs, cr, tiles_x, tiles, out);
}

template <int R>
void launch_r(int values_dtype, int guide_dtype, const void* values, const float* guide_lo, const void* guide_hi,
              long sn, long sc, long sy, long sx, float guide_scale, int N, int C, int h, int w, int H, int W, float cs,
              float cr, int tiles_x, int tiles, float* out, hipStream_t s) {
#define JBU_GO(VT, GT) \
  launch<R, VT, GT>(values, guide_lo, guide_hi, sn, sc, sy, sx, guide_scale, N, C, h, w, H, W, cs, cr, tiles_x, tiles, out, s)
  if (values_dtype == RDMI_F16) {
    if (guide_dtype == RDMI_U8) JBU_GO(f16, unsigned char); else JBU_GO(f16, float);
  } else {
    if (guide_dtype == RDMI_U8) JBU_GO(float, unsigned char); else JBU_GO(float, float);
  }
#undef JBU_GO
}

}  // namespace

extern "C" int rdmi_joint_bilateral_upsample(const void* values, int values_dtype, const float* guide_lo,
                                             const void* guide_hi, int guide_dtype, long sn, long sc, long sy, long sx,
                                             float guide_scale, int N, int C, int h, int w, int H, int W, int radius,
                                             float sigma_spatial, float sigma_range, float* out, void* stream) {
  RDMI_REQUIRE(values && guide_lo && guide_hi && out, RDMI_E_ARG, "joint_bilateral_upsample: null pointer");
  RDMI_REQUIRE(N >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, RDMI_E_ARG,
               "joint_bilateral_upsample: N (%d), h x w (%d x %d) and H x W (%d x %d) must be positive", N, h, w, H, W);
  RDMI_REQUIRE(C >= 1 && C <= kMaxC, RDMI_E_ARG, "joint_bilateral_upsample: C %d outside 1 … %d", C, kMaxC);
  RDMI_REQUIRE(radius >= 1 && radius <= RDMI_JBU_MAX_RADIUS, RDMI_E_ARG,
               "joint_bilateral_upsample: radius %d outside 1 … %d", radius, RDMI_JBU_MAX_RADIUS);
  RDMI_REQUIRE(sigma_spatial > 0.0f && sigma_range > 0.0f, RDMI_E_ARG,
               "joint_bilateral_upsample: sigma_spatial %g, sigma_range %g (> 0 expected)", (double)sigma_spatial,
               (double)sigma_range);
  RDMI_REQUIRE(values_dtype == RDMI_F16 || values_dtype == RDMI_F32, RDMI_E_ARG,
               "joint_bilateral_upsample: values dtype %d (f16 or f32)", values_dtype);
  RDMI_REQUIRE(guide_dtype == RDMI_U8 || guide_dtype == RDMI_F32, RDMI_E_ARG,
               "joint_bilateral_upsample: guide dtype %d (u8 or f32)", guide_dtype);
  RDMI_REQUIRE(H >= h && W >= w, RDMI_E_UNSUPPORTED,
               "joint_bilateral_upsample: output %d x %d below the input %d x %d (an upsampler: H >= h and W >= w)", H,
               W, h, w);
  const int tiles_x = rdmi::div_up(W, kTileW), tiles_y = rdmi::div_up(H, kTileH);
  const long tiles = (long)tiles_x * tiles_y;
  RDMI_REQUIRE(tiles * N <= INT_MAX, RDMI_E_UNSUPPORTED, "joint_bilateral_upsample: %ld tiles of %d x %d (at most 2^31 - 1)",
               tiles * N, kTileH, kTileW);
  // log2 e / (2σ²), formed in f64 and rounded once; a σ so small that the f32 overflows gives +inf, which the
  // kernel's clamp of the exponent absorbs
  const float cs = (float)(kLog2e / (2.0 * (double)sigma_spatial * (double)sigma_spatial));
  const float cr = (float)(kLog2e / (2.0 * (double)sigma_range * (double)sigma_range));
  hipStream_t s = (hipStream_t)stream;
#define JBU_R(R) \
  launch_r<R>(values_dtype, guide_dtype, values, guide_lo, guide_hi, sn, sc, sy, sx, guide_scale, N, C, h, w, H, W, cs, cr, tiles_x, (int)tiles, out, s)
  if (radius == 1) JBU_R(1);
  else if (radius == 2) JBU_R(2);
  else JBU_R(3);
#undef JBU_R
  return rdmi::check_launch("joint_bilateral_upsample");
}
