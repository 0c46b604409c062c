// Flow-guided temporal filter of a depth video (since rdmi_version 13); the arithmetic, operation by operation, is
// fixed in include/rdmi.h "Temporal filter" and restated in f64 and f32 by tests/stabilize_util.py.
//
// tfilter_k<R>: a workgroup of 256 lanes owns a kTileW × kTileH = 32 × 8 pixel tile of one output frame, lanes along
// x, so a wave covers two rows of 32 pixels: its flow load of one neighbour is two runs of 256 contiguous bytes, its
// valid load two of 32, its d0 load and its store two of 128.  One launch covers all n frames and all 2R neighbours:
// d0 is read once and out written once.  The four taps of a neighbour are plain element loads through the caches
// (as in fb_check_k and depth_temporal_k): where the flow is smooth, neighbouring lanes read neighbouring
// addresses of two rows of the neighbour frame, and the 2R neighbour tiles of a workgroup (≈ 1 KiB each) live in L2
// for the workgroups of the next frames, which read them as their own d0 or as another neighbour.  No LDS: a staged
// window would bound the flow it can serve.  A pixel is one lane's fixed-order chain: no atomics, no
// workspace, nothing depends on n, f0, the alignment or the call.  Blocks run in dispatch order, frame-major; giving
// each XCD a contiguous range of frames (xcd_remap) measured 4 – 6 % slower.
#include "common.h"

#include <limits.h>

namespace {

constexpr int kTileW = 32, kTileH = 8, kBlock = kTileW * kTileH;
constexpr long kMaxHW = 1L << 30;
constexpr double kLog2e = 1.4426950408889634074;

__device__ __forceinline__ float ldv(const f16* p, long o) { return (float)p[o]; }
__device__ __forceinline__ float ldv(const float* p, long o) { return p[o]; }
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <int R, typename DT>
__global__ __launch_bounds__(kBlock) void tfilter_k(const DT* __restrict__ depth, int N, int H, int W, int f0, int n,
                                                    const float* __restrict__ flow,
                                                    const unsigned char* __restrict__ valid, float ct, float cd,
                                                    int tiles_x, int tiles, float* __restrict__ out) {
  const int fr = blockIdx.x / tiles, t = blockIdx.x - fr * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int x = tx * kTileW + (threadIdx.x & (kTileW - 1)), y = ty * kTileH + (threadIdx.x / kTileW);
  if (x >= W || y >= H) return;
  const long hw = (long)H * W, pix = (long)y * W + x;
  const int i = f0 + fr;
  const float d0 = ldv(depth, (long)i * hw + pix);
  float res = d0;
  if (finite_f(d0)) {
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    float acc = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int s = 0; s < 2 * R; ++s) {
      const int k = s < R ? s - R : s - R + 1, j = i + k;
      if (j < 0 || j >= N) continue;  // uniform over the workgroup; the slot's row is not read
      const long row = ((long)s * n + fr) * hw + pix;
      if (valid && valid[row] == 0) continue;
      const f32x2 u = *(const f32x2*)&flow[2 * row];
      const float X = __fadd_rn((float)x, u[0]), Y = __fadd_rn((float)y, u[1]);
      if (!(X >= 0.0f && X <= wmax && Y >= 0.0f && Y <= hmax)) continue;  // also a NaN: no address is formed from one
      const int x0 = min((int)X, W - 1), y0 = min((int)Y, H - 1), x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
      const float wx = __fsub_rn(X, (float)x0), wy = __fsub_rn(Y, (float)y0);
      const long base = (long)j * hw, r0 = base + (long)y0 * W, r1 = base + (long)y1 * W;
      const float a00 = ldv(depth, r0 + x0), a01 = ldv(depth, r0 + x1);
      const float a10 = ldv(depth, r1 + x0), a11 = ldv(depth, r1 + x1);
      // the lerp form: equal taps give that value exactly whatever wx and wy are
      const float t0 = fmaf(wx, __fsub_rn(a01, a00), a00), t1 = fmaf(wx, __fsub_rn(a11, a10), a10);
      const float dk = fmaf(wy, __fsub_rn(t1, t0), t0);
      if (!finite_f(dk)) continue;
      const float dl = __fsub_rn(dk, d0);
      const float e = fmaf(__fmul_rn(dl, dl), cd, __fmul_rn((float)(k * k), ct));
      const float w = __builtin_amdgcn_exp2f(-e);
      acc = fmaf(w, dl, acc);
      wsum = __fadd_rn(wsum, w);
    }
    res = __fadd_rn(d0, __fdiv_rn(acc, __fadd_rn(1.0f, wsum)));
  }
  out[(long)fr * hw + pix] = res;
}

template <int R>
void launch(const void* depth, int dtype, int N, int H, int W, int f0, int n, const float* flow,
            const unsigned char* valid, float ct, float cd, int tiles_x, int tiles, float* out, hipStream_t s) {
  const dim3 grid((unsigned)((long)tiles * n)), block(kBlock);
  if (dtype == RDMI_F16)
    hipLaunchKernelGGL((tfilter_k<R, f16>), grid, block, 0, s, (const f16*)depth, N, H, W, f0, n, flow, valid, ct, cd,
                       tiles_x, tiles, out);
  else
    hipLaunchKernelGGL((tfilter_k<R, float>), grid, block, 0, s, (const float*)depth, N, H, W, f0, n, flow, valid, ct,
                       cd, tiles_x, tiles, out);
}

// log2 e / (2σ²), formed in f64 and rounded to f32 once; 0 where the σ or the constant is unusable
float weight_constant(float sigma) {
  if (!(sigma > 0.0f)) return 0.0f;
  const float c = (float)(kLog2e / (2.0 * (double)sigma * (double)sigma));
  return c > 0.0f && c <= 3.402823466e38f ? c : 0.0f;
}

}  // namespace

extern "C" int rdmi_temporal_filter(const void* depth, int depth_dtype, int N, int H, int W, int f0, int n, int radius,
                                    const float* flow, const unsigned char* valid, float sigma_time,
                                    float sigma_depth, float* out, void* stream) {
  RDMI_REQUIRE(depth && flow && out, RDMI_E_ARG, "temporal_filter: null pointer");
  RDMI_REQUIRE(N >= 1 && H >= 1 && W >= 1 && n >= 1, RDMI_E_ARG,
               "temporal_filter: N (%d), H x W (%d x %d) and n (%d) must be positive", N, H, W, n);
  RDMI_REQUIRE(f0 >= 0 && (long)f0 + n <= N, RDMI_E_ARG, "temporal_filter: frames %d … %ld outside 0 … %d", f0,
               (long)f0 + n - 1, N - 1);
  RDMI_REQUIRE(radius >= 1 && radius <= RDMI_TFILTER_MAX_RADIUS, RDMI_E_ARG,
               "temporal_filter: radius %d outside 1 … %d", radius, RDMI_TFILTER_MAX_RADIUS);
  RDMI_REQUIRE(depth_dtype == RDMI_F16 || depth_dtype == RDMI_F32, RDMI_E_ARG,
               "temporal_filter: depth dtype %d (f16 or f32)", depth_dtype);
  const float ct = weight_constant(sigma_time), cd = weight_constant(sigma_depth);
  RDMI_REQUIRE(ct > 0.0f && cd > 0.0f, RDMI_E_ARG,
               "temporal_filter: sigma_time %g, sigma_depth %g (> 0, and log2 e / (2 sigma^2) finite and positive in "
               "f32, expected)", (double)sigma_time, (double)sigma_depth);
  RDMI_REQUIRE(((uintptr_t)flow & 7) == 0, RDMI_E_ALIGN, "temporal_filter: flow not 8-byte aligned");
  RDMI_REQUIRE(((uintptr_t)out & 3) == 0, RDMI_E_ALIGN, "temporal_filter: out not 4-byte aligned");
  RDMI_REQUIRE((long)H * W <= kMaxHW, RDMI_E_UNSUPPORTED, "temporal_filter: H·W = %ld above 2^30", (long)H * W);
  const int tiles_x = rdmi::div_up(W, kTileW), tiles_y = rdmi::div_up(H, kTileH);
  const long tiles = (long)tiles_x * tiles_y;
  RDMI_REQUIRE(tiles * n <= INT_MAX, RDMI_E_UNSUPPORTED, "temporal_filter: %ld tiles of %d x %d (at most 2^31 - 1)",
               tiles * n, kTileW, kTileH);
  hipStream_t s = (hipStream_t)stream;
#define TF_R(R) launch<R>(depth, depth_dtype, N, H, W, f0, n, flow, valid, ct, cd, tiles_x, (int)tiles, out, s)
  if (radius == 1) TF_R(1);
  else if (radius == 2) TF_R(2);
  else TF_R(3);
#undef TF_R
  return rdmi::check_launch("temporal_filter");
}
