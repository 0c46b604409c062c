// Depth boundaries (rdmi.h "Depth boundaries"): precision / recall counts of the occluding contours of the aligned
// prediction a against those of the target g.  Pixel i has an edge of map d in direction k at threshold τ iff its
// neighbour j in that direction is, like i, a valid pixel of the same frame and d(j) > τ·d(i): one f64 product, one
// comparison, no division.  Per frame, threshold and direction three integers are counted: TP = #(edge of a and of
// g), NP = #edge of a, NG = #edge of g, and per frame the valid horizontal and vertical pairs.
//
// One pass for all M ≤ 16 thresholds.  For a directed pair (i → j) the thresholds at which it is an edge form a
// set S ⊂ {0 … M − 1}, kept as a bit mask; the thresholds rise, so for d(i) > 0 — always true of a, and of g
// whenever lo ≥ 0 — S is a lower set {0 … L − 1} and is its level L = |S|.  Per direction and kind (TP from
// S_a ∩ S_g, NP from S_a, NG from S_g) an (M + 1)-bin histogram of the levels is kept, and count[m] = Σ_{L > m}
// hist[L].  A set that is not a lower set (a target ≤ 0, possible with lo < 0 in depth space) adds, for each of its
// members m, +1 to bin m + 1 and −1 to bin m: under the same suffix sum that is +1 at m exactly.  Bin 0 is never read,
// so a pair that is an edge nowhere — nearly all of them — touches no histogram.
//
// Tiling.  A frame's rows are cut into octets counted from the ROW's first pixel (octet o = pixels 8o … 8o + 7, the
// last one possibly short) and into strips of kRows rows; a unit is one octet column of one strip, unit u = strip ·
// octets_per_row + octet, and thread t of block b of a (blocks per frame, N) grid owns unit b·256 + t: consecutive
// lanes read consecutive octets of a row.  The owner of a unit visits the pairs whose FIRST pixel (the left one,
// the upper one) lies in it: it reads its kRows rows and the row below them, nine pixels of each — the ninth is
// the right neighbour of the octet's last pixel.  Each unordered pair is so visited once and yields direction R (or D)
// for its first pixel and L (or U) for its second.  An octet whose address is 16-byte aligned (the u8 mask: 8-byte)
// is read with wide loads, any other element by element, and so is the ninth pixel; every pixel, read as "own" or
// as a neighbour, wide or not, goes through boundary_pixel() below and gets the same bits (its only contractible
// expression is the explicit fma of aligned_depth; a comparison of a product has nothing to contract).
//
// Determinism.  Every count is an integer and every addition of integers is exact and order-free: the per-workgroup
// LDS histograms (32-bit atomics; a workgroup owns 256 · 8 · kRows pixels, far from overflow), the per-workgroup
// rows in the workspace, and their 64-bit sum per frame in depth_boundary_rows_k.  So the results are bitwise
// reproducible and do not depend on N, on the other frames, on the buffers' addresses or on the grid — there is no
// floating-point sum anywhere, and no floating-point atomic.  With an edge map requested the owner also reads the
// pixel left of its octet and the row above its strip, so that it alone writes its pixels' bytes, with plain stores.
#include "depth_pixel.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 4;                              // rows per strip
constexpr int kMaxT = RDMI_BOUNDARY_MAX_THRESHOLDS;   // thresholds per call
constexpr int kBins = kMaxT + 1;                      // levels 0 … M
constexpr int kHist = 4 * 3 * kBins;                  // [direction R, L, D, U][TP, NP, NG][level]
constexpr int kRowInts = 208;                         // a workgroup's row: the histograms, the two pair counts, padding
static_assert(kHist + 2 <= kRowInts, "row too short");

enum { DIR_R = 0, DIR_L = 1, DIR_D = 2, DIR_U = 3 };

struct boundary_args {
  double tau[kMaxT];
  const double* st;
  double clip_lo, clip_hi;
  float lo, hi;
  int H, W, M, space, edge_index;
  int octets, units;  // octets per row, units per frame
};

// what a frame's pixels share
struct frame_fit {
  double s, t, clip_lo, clip_hi;
  float lo, hi;
  int space;
  bool fit, pos;
};

// THE aligned value and validity of one pixel: in = inside the row and not masked out
__device__ __forceinline__ bool boundary_pixel(float p, float g, bool in, const frame_fit& F, double& a, double& gd) {
  a = aligned_depth(F.s, p, F.t, F.space, F.clip_lo, F.clip_hi);
  gd = (double)g;
  return in & F.fit & pixel_valid<true>(p, g, F.lo, F.hi, F.pos) & (a > 0.0) & (a < (double)INFINITY);
}

struct row9 {
  double a[9], g[9];
  unsigned ok;  // bit e: pixel x0 + e is valid
};

// pixels x0 … x0 + cnt − 1 of a row (off = their element offset in the frame), and the ninth when it exists
template <typename TP, typename TG, bool MASK>
__device__ __forceinline__ void load_row(const TP* __restrict__ pp, const TG* __restrict__ gp,
                                         const unsigned char* __restrict__ mp, long off, int cnt, bool ninth,
                                         const frame_fit& F, row9& r) {
  float p[8], g[8];
  unsigned char m[8];
  load_octet(pp + off, ((uintptr_t)(pp + off) & 15) == 0, cnt, p);
  load_octet(gp + off, ((uintptr_t)(gp + off) & 15) == 0, cnt, g);
  if (MASK) load_octet(mp + off, ((uintptr_t)(mp + off) & 7) == 0, cnt, m);
  r.ok = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bool in = e < cnt;
    if (MASK) in = in & (m[e] != 0);
    r.ok |= (unsigned)boundary_pixel(p[e], g[e], in, F, r.a[e], r.g[e]) << e;
  }
  r.a[8] = r.g[8] = 0.0;
  if (ninth) {
    bool in = true;
    if (MASK) in = mp[off + 8] != 0;
    r.ok |= (unsigned)boundary_pixel((float)pp[off + 8], (float)gp[off + 8], in, F, r.a[8], r.g[8]) << 8;
  }
}

// the thresholds at which j lies beyond i: bit m ⇔ d(j) > τ_m·d(i); f = i → j, b = j → i
struct pair_sets {
  unsigned af, ab, gf, gb;
};
__device__ __forceinline__ pair_sets beyond(const boundary_args& A, double ai, double aj, double gi, double gj) {
  pair_sets r{0u, 0u, 0u, 0u};
  // positive values and no edge at the lowest threshold: none at any (τ_m·d rises with m)
  const double t0 = A.tau[0];
  const bool quiet = (gi > 0.0) & (gj > 0.0) & !(aj > t0 * ai) & !(ai > t0 * aj) & !(gj > t0 * gi) & !(gi > t0 * gj);
  if (quiet) return r;
  for (int m = 0; m < A.M; ++m) {
    const double t = A.tau[m];
    r.af |= (unsigned)(aj > t * ai) << m;
    r.ab |= (unsigned)(ai > t * aj) << m;
    r.gf |= (unsigned)(gj > t * gi) << m;
    r.gb |= (unsigned)(gi > t * gj) << m;
  }
  return r;
}

// one set into one histogram (file header): a lower set is its level; any other set, member by member
__device__ __forceinline__ void add_set(int* h, unsigned s) {
  if (s == 0u) return;
  if ((s & (s + 1u)) == 0u) {
    atomicAdd(h + __popc(s), 1);
    return;
  }
  for (; s; s &= s - 1u) {
    const int m = __ffs((int)s) - 1;
    atomicAdd(h + m + 1, 1);
    atomicAdd(h + m, -1);
  }
}
// direction k of one pixel: TP, NP, NG
__device__ __forceinline__ void count_edge(int* hist, int k, unsigned sa, unsigned sg) {
  if ((sa | sg) == 0u) return;
  int* h = hist + k * 3 * kBins;
  add_set(h, sa & sg);
  add_set(h + kBins, sa);
  add_set(h + 2 * kBins, sg);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename TP, typename TG, bool MASK, bool EDGES>
__global__ __launch_bounds__(kThreads) void depth_boundary_k(const TP* __restrict__ pred,
                                                             const TG* __restrict__ target,
                                                             const unsigned char* __restrict__ mask,
                                                             const boundary_args A, unsigned char* __restrict__ edges,
                                                             int* __restrict__ part) {
  __shared__ int hist[kRowInts];  // kHist bins, then the horizontal and the vertical pair count
  if (threadIdx.x < kRowInts) hist[threadIdx.x] = 0;
  __syncthreads();

  const int f = blockIdx.y, H = A.H, W = A.W;
  const int u = blockIdx.x * kThreads + threadIdx.x;
  int nh = 0, nv = 0;
  if (u < A.units) {
    frame_fit F;
    F.s = A.st[2 * f];
    F.t = A.st[2 * f + 1];
    F.clip_lo = A.clip_lo;
    F.clip_hi = A.clip_hi;
    F.lo = A.lo;
    F.hi = A.hi;
    F.space = A.space;
    F.fit = (F.s == F.s) & (F.t == F.t);  // a frame without a fit has no valid pixel
    F.pos = A.space != RDMI_SPACE_DEPTH;
    const long base = (long)f * H * W;
    const TP* pp = pred + base;
    const TG* gp = target + base;
    const unsigned char* mp = MASK ? mask + base : nullptr;
    const int strip = u / A.octets, x0 = (u - strip * A.octets) * 8, y0 = strip * kRows;
    const int cnt = W - x0 < 8 ? W - x0 : 8;
    const bool ninth = x0 + 8 < W;
    const double te = A.tau[EDGES ? A.edge_index : 0];

    row9 cur, nxt;
    unsigned eb[8], ebn[8];  // the edge bytes of the current row and, so far, of the next
#pragma unroll
    for (int e = 0; e < 8; ++e) eb[e] = 0u;
    load_row<TP, TG, MASK>(pp, gp, mp, (long)y0 * W + x0, cnt, ninth, F, cur);
    if (EDGES && y0 > 0) {  // direction U of the strip's first row: its pairs belong to the strip above
      load_row<TP, TG, MASK>(pp, gp, mp, (long)(y0 - 1) * W + x0, cnt, false, F, nxt);
      const unsigned both = cur.ok & nxt.ok;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (both >> e & 1u)
          eb[e] |= (unsigned)(nxt.a[e] > te * cur.a[e]) << DIR_U | (unsigned)(nxt.g[e] > te * cur.g[e]) << (4 + DIR_U);
    }
    for (int r = 0; r < kRows; ++r) {
      const int y = y0 + r;
      if (y >= H) break;
      const long off = (long)y * W + x0;
      if (y + 1 < H)
        load_row<TP, TG, MASK>(pp, gp, mp, off + W, cnt, ninth, F, nxt);
      else
        nxt.ok = 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e) ebn[e] = 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (!(cur.ok >> e & 1u)) continue;
        if (cur.ok >> (e + 1) & 1u) {  // (x, y) – (x + 1, y)
          ++nh;
          const pair_sets s = beyond(A, cur.a[e], cur.a[e + 1], cur.g[e], cur.g[e + 1]);
          count_edge(hist, DIR_R, s.af, s.gf);
          count_edge(hist, DIR_L, s.ab, s.gb);
          if (EDGES) {
            eb[e] |= (s.af >> A.edge_index & 1u) << DIR_R | (s.gf >> A.edge_index & 1u) << (4 + DIR_R);
            if (e + 1 < 8) eb[e + 1] |= (s.ab >> A.edge_index & 1u) << DIR_L | (s.gb >> A.edge_index & 1u) << (4 + DIR_L);
          }
        }
        if (nxt.ok >> e & 1u) {  // (x, y) – (x, y + 1)
          ++nv;
          const pair_sets s = beyond(A, cur.a[e], nxt.a[e], cur.g[e], nxt.g[e]);
          count_edge(hist, DIR_D, s.af, s.gf);
          count_edge(hist, DIR_U, s.ab, s.gb);
          if (EDGES) {
            eb[e] |= (s.af >> A.edge_index & 1u) << DIR_D | (s.gf >> A.edge_index & 1u) << (4 + DIR_D);
            ebn[e] |= (s.ab >> A.edge_index & 1u) << DIR_U | (s.gb >> A.edge_index & 1u) << (4 + DIR_U);
          }
        }
      }
      if (EDGES) {
        if (x0 > 0 && (cur.ok & 1u)) {  // direction L of the octet's first pixel: that pair belongs to the octet before
          bool in = true;
          if (MASK) in = mp[off - 1] != 0;
          double al, gl;
          if (boundary_pixel((float)pp[off - 1], (float)gp[off - 1], in, F, al, gl))
            eb[0] |= (unsigned)(al > te * cur.a[0]) << DIR_L | (unsigned)(gl > te * cur.g[0]) << (4 + DIR_L);
        }
        unsigned char* ep = edges + base + off;
        if (cnt == 8 && ((uintptr_t)ep & 7) == 0) {
          *(u32x2*)ep = u32x2{eb[0] | eb[1] << 8 | eb[2] << 16 | eb[3] << 24, eb[4] | eb[5] << 8 | eb[6] << 16 | eb[7] << 24};
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e < cnt) ep[e] = (unsigned char)eb[e];
        }
      }
      cur = nxt;
#pragma unroll
      for (int e = 0; e < 8; ++e) eb[e] = ebn[e];
    }
  }
  nh = wave_sum_i(nh);
  nv = wave_sum_i(nv);
  if ((threadIdx.x & 63) == 0) {
    if (nh) atomicAdd(hist + kHist, nh);
    if (nv) atomicAdd(hist + kHist + 1, nv);
  }
  __syncthreads();
  if (threadIdx.x < kRowInts) part[((long)f * gridDim.x + blockIdx.x) * kRowInts + threadIdx.x] = hist[threadIdx.x];
}

// One workgroup per frame: the frame's rows added in 64-bit, element by element, then count[m] = Σ_{L > m} hist[L].
__global__ __launch_bounds__(kThreads) void depth_boundary_rows_k(const int* __restrict__ part, int bpf, int M,
                                                                  long long* __restrict__ counts,
                                                                  long long* __restrict__ pairs) {
  __shared__ long long tot[kRowInts];
  const int f = blockIdx.x, t = threadIdx.x;
  if (t < kRowInts) {
    const int* r = part + (long)f * bpf * kRowInts + t;
    long long v = 0;
    for (int b = 0; b < bpf; ++b) v += r[(long)b * kRowInts];
    tot[t] = v;
  }
  __syncthreads();
  for (int i = t; i < M * 12; i += kThreads) {  // counts [N][M][4][3]
    const int m = i / 12, kc = i - m * 12;
    long long v = 0;
    for (int L = m + 1; L <= M; ++L) v += tot[kc * kBins + L];
    counts[(long)f * M * 12 + i] = v;
  }
  if (t < 2) pairs[2 * (long)f + t] = tot[kHist + t];
}

// units per frame, or 0 when they do not fit the grid
long frame_units(int H, int W) { return (long)((W + 7) / 8) * ((H + kRows - 1) / kRows); }
int blocks_per_frame(long units) { return (int)((units + kThreads - 1) / kThreads); }

}  // namespace

extern "C" long rdmi_depth_boundary_workspace(int N, int H, int W, int M) {
  if (N < 1 || H < 1 || W < 1 || M < 1 || M > kMaxT) return 0;
  const long units = frame_units(H, W);
  if (units > 0x7fffff00L) return 0;
  return (long)N * blocks_per_frame(units) * kRowInts * (long)sizeof(int);
}

extern "C" int rdmi_depth_boundary(const void* pred, int pred_dtype, const void* target, int target_dtype,
                                   const unsigned char* mask, int N, int H, int W, float lo, float hi,
                                   const double* st, int space, double clip_lo, double clip_hi,
                                   const double* thresholds, int M, long long* counts, long long* pairs,
                                   unsigned char* edges, int edge_index, void* workspace, void* stream) {
  const char* what = "depth_boundary";
  RDMI_REQUIRE(pred && target && st && thresholds && counts && pairs && workspace, RDMI_E_ARG, "%s: null pointer",
               what);
  RDMI_REQUIRE(N >= 1 && H >= 1 && W >= 1, RDMI_E_ARG, "%s: N (%d), H (%d) and W (%d) must be >= 1", what, N, H, W);
  RDMI_REQUIRE(dtype_ok(pred_dtype) && dtype_ok(target_dtype), RDMI_E_ARG,
               "%s: pred / target dtype %d / %d, f16 or f32 expected", what, pred_dtype, target_dtype);
  RDMI_REQUIRE(space_ok(space), RDMI_E_ARG, "%s: unknown space %d", what, space);
  RDMI_REQUIRE(lo < hi, RDMI_E_ARG, "%s: valid range needs lo < hi, got %g, %g", what, (double)lo, (double)hi);
  RDMI_REQUIRE(clip_lo <= clip_hi, RDMI_E_ARG, "%s: clip needs clip_lo <= clip_hi, got %g, %g", what, clip_lo, clip_hi);
  RDMI_REQUIRE(M >= 1 && M <= kMaxT, RDMI_E_ARG, "%s: %d thresholds, 1 .. %d expected", what, M, kMaxT);
  for (int m = 0; m < M; ++m) {
    const double t = thresholds[m];
    RDMI_REQUIRE(t > 1.0 && t < (double)INFINITY, RDMI_E_ARG, "%s: threshold %d is %g, a finite value > 1 expected",
                 what, m, t);
    RDMI_REQUIRE(m == 0 || t > thresholds[m - 1], RDMI_E_ARG,
                 "%s: thresholds must rise strictly, got %g after %g at %d", what, t, thresholds[m - 1], m);
  }
  RDMI_REQUIRE(!edges || (edge_index >= 0 && edge_index < M), RDMI_E_ARG, "%s: edge_index %d outside 0 .. M - 1 = %d",
               what, edge_index, M - 1);
  RDMI_REQUIRE(((uintptr_t)workspace & 15) == 0, RDMI_E_ALIGN, "%s: workspace not 16-byte aligned", what);
  RDMI_REQUIRE(N <= 65535, RDMI_E_UNSUPPORTED, "%s: at most 65535 frames per call, got %d", what, N);
  const long units = frame_units(H, W);
  RDMI_REQUIRE(units <= 0x7fffff00L, RDMI_E_UNSUPPORTED, "%s: a frame of %d x %d pixels has too many tiles", what, H, W);

  boundary_args A;
  for (int m = 0; m < kMaxT; ++m) A.tau[m] = m < M ? thresholds[m] : (double)INFINITY;
  A.st = st;
  A.clip_lo = clip_lo;
  A.clip_hi = clip_hi;
  A.lo = lo;
  A.hi = hi;
  A.H = H;
  A.W = W;
  A.M = M;
  A.space = space;
  A.edge_index = edges ? edge_index : 0;
  A.octets = (W + 7) / 8;
  A.units = (int)units;
  const int bpf = blocks_per_frame(units);
  const dim3 grid(bpf, N);
  with_input_types(pred_dtype, target_dtype, mask != nullptr, [&](auto tp, auto tg, auto masked) {
    using TP = typename decltype(tp)::type;
    using TG = typename decltype(tg)::type;
    auto go = [&](auto with_edges) {
      hipLaunchKernelGGL((depth_boundary_k<TP, TG, decltype(masked)::value, decltype(with_edges)::value>), grid,
                         dim3(kThreads), 0, (hipStream_t)stream, (const TP*)pred, (const TG*)target, mask, A, edges,
                         (int*)workspace);
    };
    if (edges)
      go(std::true_type{});
    else
      go(std::false_type{});
  });
  const int rc = rdmi::check_launch(what);
  if (rc) return rc;
  hipLaunchKernelGGL(depth_boundary_rows_k, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, (const int*)workspace, bpf,
                     M, counts, pairs);
  return rdmi::check_launch("depth_boundary_rows");
}
