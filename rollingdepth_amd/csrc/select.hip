// Exact order statistics on the device (since rdmi_version 9): a most-significant-digit radix select over the
// order-preserving key of select_key.h.  kSelectPasses counting passes read the data once each and build, for up
// to RDMI_SELECT_MAX quantiles together, the histogram of one key digit over the elements that share the digits
// chosen so far; between two passes a one-workgroup pick step turns the histogram into the next digit.  Nothing is
// sorted, nothing is copied and the host never waits: counting, picking and the final value all stay in stream order.
//
// Counting.  Every wave of a workgroup owns a private LDS histogram per quantile (integer ds_add, no float
// atomics); the workgroup adds its waves' histograms and issues one 64-bit global atomic add per non-empty bin.
// Integer sums do not depend on arrival order, so every result is bitwise reproducible.
// Contention.  A depth map is this kernel's bad case: in pass 0 nearly all of a [0, 2] map shares one or two
// exponent bins, so 64 lanes would queue on one LDS address.  wave_count() therefore peels: the first active
// lane's bin is broadcast, the lanes that hold the same bin are counted with a ballot and one lane adds the
// count.  While a peel keeps catching a quarter of the wave it repeats (up to kPeel times); what is left over —
// or everything, when the first peel shows the bins are spread — goes to per-lane LDS atomics.  A constant map
// costs one LDS add per wave and element slot.
// Quantiles whose chosen digits are still equal (always in pass 0, usually in pass 1 of a depth map) share one
// histogram: it is counted once and written to each of their rows.
#include "common.h"
#include "select_key.h"

static_assert(kSelectMax == RDMI_SELECT_MAX, "select_key.h and rdmi.h disagree on the quantile count");

namespace {

constexpr int kBlock = 256;       // 4 waves
constexpr int kWaves = kBlock / 64;
constexpr int kGridCap = 2048;    // capped, grid-strided: 8 workgroups (8 × 16 KiB of LDS) per CU on 256 CUs
constexpr int kPeel = 4;
constexpr long kMaxN = 1L << 42;  // a workgroup's share of n stays below 2^32: its 32-bit LDS counts cannot wrap

__global__ void zero_u64_k(unsigned long long* __restrict__ p, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0ull;
}

// Add the active lanes' bins to this wave's histogram.  Runs under any exec mask: ballots see the running lanes.
__device__ __forceinline__ void wave_count(unsigned* __restrict__ hw, bool active, unsigned bin) {
  unsigned long long todo = __ballot(active);
  if (todo == 0) return;
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < kPeel && todo != 0; ++it) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
    const unsigned long long same = __ballot(active && bin == b);
    if (lane == leader) atomicAdd(&hw[b], (unsigned)__popcll(same));
    active = active && bin != b;
    todo &= ~same;
    if (__popcll(same) < 16) break;  // the bins are spread: peeling on would cost more than it merges
  }
  if (active) atomicAdd(&hw[bin], 1u);
}

struct Prefixes {
  unsigned pf[kSelectMax];
  bool own[kSelectMax];  // quantile j counts its own histogram (no earlier quantile has the same prefix)
  int rep[kSelectMax];   // the quantile whose histogram j shares
};

__device__ __forceinline__ void count_value(unsigned (*__restrict__ hw)[kSelectBins], const Prefixes& P, int pass,
                                            unsigned pmask, int shift, float v, bool keep) {
  keep = keep && !rdmi_select_is_nan(v);
  const unsigned key = rdmi_select_key(v);
  const unsigned bin = (key >> shift) & (unsigned)(kSelectBins - 1);
  const unsigned hi = key & pmask;
#pragma unroll
  for (int j = 0; j < kSelectMax; ++j)
    if (P.own[j]) wave_count(hw[j], keep && hi == P.pf[j], bin);
}

// x: f32 (xf32) or f16, element-aligned.  Elements up to the first 16-byte boundary and after the last whole
// vector are read one by one, the body with 16-byte loads (4 floats / 8 halves per lane and step).
__global__ __launch_bounds__(kBlock) void select_hist_k(const void* __restrict__ x, int xf32,
                                                        const unsigned char* __restrict__ mask, long n,
                                                        const rdmi_select_state* __restrict__ st, int pass, int k,
                                                        unsigned long long* __restrict__ hist) {
  __shared__ unsigned h[kWaves][kSelectMax][kSelectBins];
  for (int i = threadIdx.x; i < kWaves * kSelectMax * kSelectBins; i += kBlock) (&h[0][0][0])[i] = 0u;
  Prefixes P;
#pragma unroll
  for (int j = 0; j < kSelectMax; ++j) {
    P.pf[j] = (pass > 0 && j < k) ? st->prefix[j] : 0u;
    P.rep[j] = j;
#pragma unroll
    for (int i = j - 1; i >= 0; --i)
      if (P.pf[i] == P.pf[j]) P.rep[j] = P.rep[i];
    P.own[j] = j < k && P.rep[j] == j;
  }
  __syncthreads();
  unsigned(*hw)[kSelectBins] = h[threadIdx.x >> 6];
  const unsigned pmask = rdmi_select_prefix_mask(pass);
  const int shift = rdmi_select_shift(pass);
  const long stride = (long)gridDim.x * kBlock;
  const long t0 = blockIdx.x * (long)kBlock + threadIdx.x;
  const int esz = xf32 ? 4 : 2, per = 16 / esz;
  long head = (long)(((16 - ((uintptr_t)x & 15)) & 15) / esz);
  if (head > n) head = n;
  const long nvec = (n - head) / per;
  const long tail0 = head + nvec * per;
  const char* xb = (const char*)x + head * esz;  // 16-byte aligned
  const unsigned char* mb = mask ? mask + head : nullptr;
  const bool mvec = mb && (((uintptr_t)mb & (uintptr_t)(per - 1)) == 0);  // `per` mask bytes in one aligned load
  for (long i = t0; i < nvec; i += stride) {
    unsigned long long mbits = ~0ull;  // byte e ≠ 0: keep element e
    if (mvec) {
      mbits = xf32 ? (unsigned long long)((const unsigned*)mb)[i] : ((const unsigned long long*)mb)[i];
    } else if (mb) {
      mbits = 0;
      for (int e = 0; e < per; ++e) mbits |= (unsigned long long)mb[i * per + e] << (8 * e);
    }
    if (xf32) {
      const f32x4 v = ((const f32x4*)xb)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) count_value(hw, P, pass, pmask, shift, v[e], ((mbits >> (8 * e)) & 0xff) != 0);
    } else {
      const f16x8 v = ((const f16x8*)xb)[i];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        count_value(hw, P, pass, pmask, shift, (float)v[e], ((mbits >> (8 * e)) & 0xff) != 0);
    }
  }
  // scalar head [0, head) and tail [tail0, n): fewer than 2·per elements, taken by the first lanes of the grid
  const long nscal = head + (n - tail0);
  for (long s = t0; s < nscal; s += stride) {
    const long i = s < head ? s : tail0 + (s - head);
    const float v = xf32 ? ((const float*)x)[i] : (float)((const f16*)x)[i];
    count_value(hw, P, pass, pmask, shift, v, mask ? mask[i] != 0 : true);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k * kSelectBins; i += kBlock) {
    const int j = i / kSelectBins, b = i % kSelectBins;
    int r = 0;
#pragma unroll
    for (int jj = 1; jj < kSelectMax; ++jj) r = j == jj ? P.rep[jj] : r;
    unsigned long long c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += h[w][r][b];
    if (c) atomicAdd(&hist[(long)j * kSelectBins + b], c);
  }
}

// One workgroup of kSelectBins threads: thread b stages bin b of each quantile's histogram in LDS, then thread j
// walks quantile j's with the shared pick function.
__global__ __launch_bounds__(kSelectBins) void select_pick_k(const unsigned long long* __restrict__ hist,
                                                             const double* __restrict__ q, int pass, int k,
                                                             rdmi_select_state* __restrict__ st,
                                                             float* __restrict__ out) {
  __shared__ uint64_t h[kSelectMax][kSelectBins];
  __shared__ uint64_t part[kSelectBins / 64];
  const int t = threadIdx.x;
  for (int j = 0; j < k; ++j) h[j][t] = hist[(long)j * kSelectBins + t];
  if (pass == 0) {  // cnt: the sum of the first histogram (every quantile's pass-0 histogram is the same)
    unsigned long long c = h[0][t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((t & 63) == 0) part[t >> 6] = c;
  }
  __syncthreads();
  if (t >= k) return;
  uint64_t cnt, rank;
  uint32_t prefix;
  if (pass == 0) {
    cnt = 0;
    for (int w = 0; w < kSelectBins / 64; ++w) cnt += part[w];
    if (t == 0) st->cnt = cnt;
    rank = cnt ? rdmi_select_rank(q[t], cnt) : 0;
    prefix = 0;
  } else {
    cnt = st->cnt;
    rank = st->rank[t];
    prefix = st->prefix[t];
  }
  int bin = 0;
  uint64_t rank_in = 0;
  if (cnt && rdmi_select_pick_bin(h[t], rank, &bin, &rank_in)) {
    prefix |= (uint32_t)bin << rdmi_select_shift(pass);
    rank = rank_in;
  }
  st->rank[t] = rank;
  st->prefix[t] = prefix;
  if (pass == kSelectPasses - 1) out[t] = cnt ? rdmi_select_value(prefix) : __builtin_nanf("");
}

// renorm_k's arithmetic and order (elementwise.hip), then the clamp; NaN passes through the comparisons
__global__ void renorm_clip_k(float* __restrict__ x, long n, const float* __restrict__ lohi) {
  const float lo = lohi[0];
  const float rng = lohi[1] - lo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = x[i] - lo;
    v = v / rng;
    v = v * 2.0f - 1.0f;
    x[i] = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
  }
}

int launch_hist(const void* x, int x_f32, const unsigned char* mask, long n, const rdmi_select_state* st, int pass,
                int k, unsigned long long* hist, hipStream_t s) {
  const int per = x_f32 ? 4 : 8;
  long g = (n + (long)kBlock * per - 1) / ((long)kBlock * per);
  if (g > kGridCap) g = kGridCap;
  hipLaunchKernelGGL(select_hist_k, dim3((unsigned)g), dim3(kBlock), 0, s, x, x_f32, mask, n, st, pass, k, hist);
  return rdmi::check_launch("select_hist");
}

int launch_pick(const unsigned long long* hist, const double* q, int pass, int k, rdmi_select_state* st, float* out,
                hipStream_t s) {
  hipLaunchKernelGGL(select_pick_k, dim3(1), dim3(kSelectBins), 0, s, hist, q, pass, k, st, out);
  return rdmi::check_launch("select_pick");
}

constexpr long kStateBytes = (sizeof(rdmi_select_state) + 255) / 256 * 256;
constexpr long kHistWords = (long)kSelectPasses * kSelectMax * kSelectBins;

}  // namespace

extern "C" int rdmi_select_bins(void) { return kSelectBins; }
extern "C" int rdmi_select_passes(void) { return kSelectPasses; }
extern "C" long rdmi_select_state_bytes(void) { return (long)sizeof(rdmi_select_state); }
extern "C" long rdmi_quantiles_workspace(void) { return kStateBytes + kHistWords * 8; }

#define SELECT_COMMON(name)                                                                                 \
  RDMI_REQUIRE(k >= 1 && k <= RDMI_SELECT_MAX, RDMI_E_ARG, name ": k %d outside 1 … %d", k, RDMI_SELECT_MAX)

extern "C" int rdmi_select_hist(const void* x, int x_f32, const unsigned char* mask, long n, const void* state,
                                int pass, int k, long long* hist, void* stream) {
  RDMI_REQUIRE(x && state && hist && n > 0, RDMI_E_ARG, "select_hist: null pointer or n <= 0");
  SELECT_COMMON("select_hist");
  RDMI_REQUIRE(pass >= 0 && pass < kSelectPasses, RDMI_E_ARG, "select_hist: pass %d outside 0 … %d", pass,
               kSelectPasses - 1);
  RDMI_REQUIRE(n < kMaxN, RDMI_E_UNSUPPORTED, "select_hist: n %ld ≥ 2^42", n);
  return launch_hist(x, x_f32, mask, n, (const rdmi_select_state*)state, pass, k, (unsigned long long*)hist,
                     (hipStream_t)stream);
}

extern "C" int rdmi_select_pick(const long long* hist, const double* q, int pass, int k, void* state, float* out,
                                void* stream) {
  RDMI_REQUIRE(hist && q && state && out, RDMI_E_ARG, "select_pick: null pointer");
  SELECT_COMMON("select_pick");
  RDMI_REQUIRE(pass >= 0 && pass < kSelectPasses, RDMI_E_ARG, "select_pick: pass %d outside 0 … %d", pass,
               kSelectPasses - 1);
  return launch_pick((const unsigned long long*)hist, q, pass, k, (rdmi_select_state*)state, out,
                     (hipStream_t)stream);
}

extern "C" int rdmi_quantiles(const void* x, int x_f32, const unsigned char* mask, long n, const double* q, int k,
                              float* out, void* workspace, void* stream) {
  RDMI_REQUIRE(x && q && out && workspace && n > 0, RDMI_E_ARG, "quantiles: null pointer or n <= 0");
  SELECT_COMMON("quantiles");
  RDMI_REQUIRE(n < kMaxN, RDMI_E_UNSUPPORTED, "quantiles: n %ld ≥ 2^42", n);
  RDMI_REQUIRE(((uintptr_t)workspace & 7) == 0, RDMI_E_ALIGN, "quantiles: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  rdmi_select_state* st = (rdmi_select_state*)workspace;
  unsigned long long* hist = (unsigned long long*)((char*)workspace + kStateBytes);
  hipLaunchKernelGGL(zero_u64_k, dim3(rdmi::div_up(kHistWords, 256)), dim3(256), 0, s, hist, (int)kHistWords);
  int rc = rdmi::check_launch("select_zero");
  for (int p = 0; p < kSelectPasses && !rc; ++p) {
    unsigned long long* hp = hist + (long)p * kSelectMax * kSelectBins;
    rc = launch_hist(x, x_f32, mask, n, st, p, k, hp, s);
    if (!rc) rc = launch_pick(hp, q, p, k, st, out, s);
  }
  return rc;
}

extern "C" int rdmi_renormalize_clip_f32(float* x, long n, const float* lohi, void* stream) {
  RDMI_REQUIRE(x && lohi && n > 0, RDMI_E_ARG, "renormalize_clip: bad args");
  long g = (n + 255) / 256;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(renorm_clip_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x, n, lohi);
  return rdmi::check_launch("renormalize_clip");
}
