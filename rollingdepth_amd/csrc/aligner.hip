// DepthAligner on device (rollingdepth/depth_aligner.py).
//
// The reference runs 2000 Adam iterations of per-snippet scale/shift optimisation through
// autograd, with three host syncs per iteration (loss.item(), summ.min/max, :213).  Here one
// iteration is three kernels with no host involvement:
//   frame_stats  — per frame f and subsampled pixel p, the mean over every covering (dilation,
//                  slot) of A = x·s + t (one fma: rounded once, see mulrn below) and of
//                  1/clip(A, 1e-3) (the M / M_depth / B scatter and the .sum(0)/B.sum(0) of
//                  :169-191, summed in the reference's row order), plus
//                  the per-frame L1 scales mean|T| (:197-198) and min/max for the loss history;
//   snippet_grad — per snippet the analytic gradient of the L1 + inverse-depth L1 loss
//                  (:200-203) w.r.t. its s and t (sign(A−T)/scale, the clip mask A ≥ 1e-3, the
//                  −1/clip² of pow(−1)), reduced in f64 in a fixed order (deterministic);
//   adam         — soft constraints λ2·mean(relu(1−s)²) + λ3·mean(t²) (:205-209) and
//                  torch.optim.Adam's single-tensor update in its f32 op order (lerp — its weight < 0.5
//                  branch as one fma —, mul+addcmul, sqrt/bc2_sqrt + eps, addcdiv), loss history row.
// merge        — merge_scaled_triplets (:231-262): per frame the mean over all covering slots of
//                s·x+t, rounded through the snippet dtype where the reference computes in it.
// merge_moments — the same mean plus the per-pixel standard deviation of those slots' terms, in one pass
//                (the build's own; end of this file).
// merge_median — the per-pixel median of those slots' terms in place of their mean, optionally with their
//                median absolute deviation (the build's own; end of this file).
//
// Snippet lengths may differ per dilation (rollingdepth_pipeline.py:221-226).  The reference then
// scatters dilation i's slot j into row i·w_i + j of its [Σw, N, P] tensors M / M_depth / B
// (depth_aligner.py:169-188): rows of different dilations can coincide, and the later dilation's
// value overwrites the earlier one's at every frame both cover (B stays 1; the overwritten slot
// gets no gradient).  With one length for all dilations the rows are disjoint and the loops below
// reduce to the plain per-dilation, per-slot order.
//
// Start steps (get_snippet_indice's `stride`, rollingdepth_pipeline.py:465-502): the snippets of a
// dilation may start every ss frames plus the last window instead of at every frame.  The reference's
// optimize / merge_scaled_triplets take explicit index tensors, so the arithmetic above is unchanged;
// only "snippet k starts at frame k" becomes the map of aligner_index.h (integer, block-uniform,
// outside the pixel loops).  The kernels that derive frames are templated on SS; the SS = false
// instantiations are the start-step-1 kernels with their launch geometry and float operation order,
// and a job whose start steps are all 1 runs only those.  The loss denominator stays Σw · N · P.
// The sharded merge takes start steps through its _strided entry points (window sums: merge_k<true>;
// cover count: rdmi_cover_count).
#pragma clang fp contract(off)
#include <utility>

#include "common.h"
#include "aligner_index.h"
#include "aligner_ws.h"

namespace {

constexpr int MAXD = 8;
constexpr int MAXR = 64;  // rows Σ w_d of the reference's M / M_depth / B tensors
constexpr int PS = RDMI_ALIGNER_PS;      // pixel chunks per frame / per snippet (aligner_ws.h)
constexpr int HBLK = RDMI_ALIGNER_HBLK;  // iterations per block of history slots (aligner_ws.h)

struct AlP {
  const float* x[MAXD];
  float* s[MAXD];
  float* t[MAXD];
  int n[MAXD], stride[MAXD], off[MAXD];  // off: first global snippet index of dilation d
  int w[MAXD], rb[MAXD];                 // snippet length, first row (d·w_d) of dilation d
  int ss[MAXD], last[MAXD];              // start step, start of the last window (aligner_index.h)
  int nd, R, N;                          // R = Σ w_d rows
  long P;
  float lr, b1, b2, eps, lmda2, lmda3, dw, ls;
  // workspace views
  float *T, *Td;
  double* fpart;  // [N][PS][4]: Σ|T|, Σ|Td|, min T, max T over pixel chunk c of frame f
  double *gs, *gt, *l1, *l2;  // [ntot][PS]: per snippet and pixel chunk
  float *m, *v;  // Adam moments [2*Ntot] (s then t)
  const double* bct;  // [iters + 1][2]: Adam's bias corrections 1 − β1^step, 1 − β2^step (adam_bc_k)
  float* hist;
  int ntot;
};

// __fmul_rn / __fadd_rn are header functions compiled outside this file's fp contract(off): where a mulrn
// feeds an addrn directly the compiler contracts the pair to one fma, ONE rounding.  In the optimiser that is
// A = x·s + t in frame_stats_body and snippet_grad_body (v_pk_fma_f32 / v_fma_f32; the reference and the oracle
// round the product and the sum separately: A can differ from theirs by 1 ulp) and m + lw·diff in adam_param's
// lw < 0.5 lerp branch (not taken at the default β1 = 0.5).  Every other mulrn / addrn pair has a division or a
// second product between the two and stays two operations (v·β2 + (vw·g)·g is a packed multiply and an add), as
// do the plain operators.  tests/aligner_util.py restates exactly this (fused=True) and
// tests/test_aligner_step_gpu.py holds the kernels to it bitwise.  Writing the two as plain a * b, a + b under
// the pragma gives the two roundings but measured 0.5 % slower per iteration (aligner) — not kept.
__device__ __forceinline__ float mulrn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float addrn(float a, float b) { return __fadd_rn(a, b); }

template <int BS>
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double r = 0.0;
  for (int i = 0; i < BS / 64; ++i) r += sh[i];
  return r;
}

__device__ __forceinline__ long chunk_lo(long P, int c) { return P * c / PS; }

// The (dilation, snippet) whose slot holds row r of frame f in the reference's scatter (the LAST
// dilation writing that position), or d = -1 when no dilation covers it.
// SS: some dilation's snippets start more than one frame apart (start step > 1): snippet k starts at
// rdmi_snip_start(k) instead of frame k.  The SS = false instantiations are the start-step-1 kernels.
template <bool SS>
__device__ __forceinline__ int row_owner(const AlP& p, int r, int f, int& k_out) {
  for (int d = p.nd - 1; d >= 0; --d) {
    const int j = r - p.rb[d];
    if (j < 0 || j >= p.w[d]) continue;
    const int q = f - j * p.stride[d];
    const int k = SS ? rdmi_snip_at(q, p.ss[d], p.last[d], p.n[d]) : q;
    if (k < 0 || k >= p.n[d]) continue;
    k_out = k;
    return d;
  }
  return -1;
}

// Block sums of NV doubles at once, each in block_sum_d's order (the xor butterfly inside a wave,
// then the 4 wave partials in wave order): one LDS round instead of NV.  Result valid in thread 0.
template <int NV>
__device__ __forceinline__ void block_sums_d(double (&v)[NV]) {
  __shared__ double sh[NV][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += __shfl_xor(v[i], o, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int i = 0; i < NV; ++i) sh[i][threadIdx.x >> 6] = v[i];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double r = 0.0;
      for (int w = 0; w < 4; ++w) r += sh[i][w];
      v[i] = r;
    }
}

// One (frame f, pixel chunk c) work unit of frame_stats; thread 0 returns the chunk's min/max of T.
template <bool SS>
__device__ __forceinline__ void frame_stats_body(const AlP& p, int f, int c, float& mn_out, float& mx_out) {
  // the slots covering frame f in row order (block-uniform): snippet row pointer, s, t — one row
  // per lane of wave 0 (R <= MAXR = 64), compacted in row order by a ballot
  __shared__ const float* ex[MAXR];
  __shared__ float es[MAXR], et[MAXR];
  __shared__ int ecnt;
  if (threadIdx.x < 64) {
    const int r = threadIdx.x;
    int k = 0;
    const int d = r < p.R ? row_owner<SS>(p, r, f, k) : -1;
    const unsigned long long m = __ballot(d >= 0);
    if (d >= 0) {
      const int slot = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      ex[slot] = p.x[d] + ((long)k * p.w[d] + (r - p.rb[d])) * p.P;
      es[slot] = p.s[d][k];
      et[slot] = p.t[d][k];
    }
    if (r == 0) ecnt = __popcll(m);
  }
  __syncthreads();
  const int cnt = ecnt;
  double sa = 0.0, sd = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  const long p1 = chunk_lo(p.P, c + 1);
  // UP pixels per thread per round, the covering slots' values loaded EB slots at a time: a round's
  // loads are issued together instead of one dependent round trip per (pixel, slot).  The same sums
  // in the same order (slots in row order per pixel, pixels in increasing order per thread).
  constexpr int UP = 4, EB = 4;
  for (long pb = chunk_lo(p.P, c) + threadIdx.x; pb < p1; pb += 256 * UP) {
    float sum[UP], sumd[UP];
#pragma unroll
    for (int u = 0; u < UP; ++u) sum[u] = sumd[u] = 0.f;
    for (int e0 = 0; e0 < cnt; e0 += EB) {
      float xv[EB][UP];
#pragma unroll
      for (int q = 0; q < EB; ++q) {
        const float* xr = ex[e0 + q < cnt ? e0 + q : cnt - 1];
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          const long px = pb + 256L * u;
          xv[q][u] = (e0 + q < cnt && px < p1) ? xr[px] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < EB; ++q) {
        if (e0 + q >= cnt) break;
        const float se = es[e0 + q], te = et[e0 + q];
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          float a = addrn(mulrn(xv[q][u], se), te);
          float ac = fmaxf(a, 1e-3f);
          sum[u] = addrn(sum[u], a);
          sumd[u] = addrn(sumd[u], 1.0f / ac);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const long px = pb + 256L * u;
      if (px >= p1) break;
      float T = 0.f, Td = 0.f;
      if (cnt) {
        T = sum[u] / (float)cnt;
        Td = sumd[u] / (float)cnt;
      }
      p.T[(long)f * p.P + px] = T;
      p.Td[(long)f * p.P + px] = Td;
      sa += fabs((double)T);
      sd += fabs((double)Td);
      mn = fminf(mn, T);
      mx = fmaxf(mx, T);
    }
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  __shared__ float r[2][4];
  if ((threadIdx.x & 63) == 0) {
    r[0][threadIdx.x >> 6] = mn;
    r[1][threadIdx.x >> 6] = mx;
  }
  double v[2] = {sa, sd};
  block_sums_d<2>(v);  // its barrier also publishes r
  if (threadIdx.x == 0) {
    double* o = p.fpart + ((long)f * PS + c) * 4;
    o[0] = v[0];
    o[1] = v[1];
    mn_out = fminf(fminf(r[0][0], r[0][1]), fminf(r[0][2], r[0][3]));
    mx_out = fmaxf(fmaxf(r[1][0], r[1][1]), fmaxf(r[1][2], r[1][3]));
  }
}

template <bool SS>
__global__ __launch_bounds__(256) void frame_stats(AlP p) {
  const int f = blockIdx.x, c = blockIdx.y;
  float mn, mx;
  frame_stats_body<SS>(p, f, c, mn, mx);
  if (threadIdx.x == 0) {
    double* o = p.fpart + ((long)f * PS + c) * 4;
    o[2] = mn;
    o[3] = mx;
  }
}

// per-frame L1 scales mean|T|, mean|Td| (:197-198) from the chunk partials, chunk order fixed
__device__ __forceinline__ void frame_scales(const AlP& p, int f, float& sc, float& scd) {
  double A = 0.0, D = 0.0;
  for (int c = 0; c < PS; ++c) {
    A += p.fpart[((long)f * PS + c) * 4];
    D += p.fpart[((long)f * PS + c) * 4 + 1];
  }
  sc = (float)(A / (double)p.P);
  scd = (float)(D / (double)p.P);
}

// One (global snippet gk, pixel chunk c) work unit of snippet_grad; the loss partials go to
// l1o[gk·PS + c], l2o[gk·PS + c].  COHERENT: the gradient partials are stored as agent-scope atomics
// (device-coherent, read by another workgroup in the same launch).
template <bool COHERENT, bool SS>
__device__ __forceinline__ void snippet_grad_body(const AlP& p, int gk, int c, double* l1o, double* l2o) {
  const long p0 = chunk_lo(p.P, c), p1 = chunk_lo(p.P, c + 1);
  int d = 0;
  while (d + 1 < p.nd && gk >= p.off[d + 1]) ++d;
  const int k = gk - p.off[d];
  const float s = p.s[d][k], t = p.t[d][k];
  const float* x = p.x[d] + (long)k * p.w[d] * p.P;
  double gs = 0.0, gt = 0.0, l1 = 0.0, l2 = 0.0;
  for (int j = 0; j < p.w[d]; ++j) {
    const int f = (SS ? rdmi_snip_start(k, p.ss[d], p.last[d]) : k) + j * p.stride[d];
    int kk = 0;
    if (row_owner<SS>(p, p.rb[d] + j, f, kk) != d) continue;  // overwritten by a later dilation's slot
    const float* Tf = p.T + (long)f * p.P;
    const float* Tdf = p.Td + (long)f * p.P;
    // UP pixels per thread per round: the round's operand loads and the frame's scale partials are
    // issued together; the same terms accumulate in the same order (pixels increasing per thread)
    constexpr int UP = 4;
    for (long pb = p0 + threadIdx.x; pb < p1; pb += 256 * UP) {
      float xa[UP], ta[UP], tda[UP];
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const long px = pb + 256L * u;
        const bool ok = px < p1;
        xa[u] = ok ? x[(long)j * p.P + px] : 0.f;
        ta[u] = ok ? Tf[px] : 0.f;
        tda[u] = ok ? Tdf[px] : 0.f;
      }
      float scf, scdf;
      frame_scales(p, f, scf, scdf);
      const float isc = 1.0f / scf, iscd = 1.0f / scdf;
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        if (pb + 256L * u >= p1) break;
        const float xv = xa[u];
        float a = addrn(mulrn(xv, s), t);
        float z = a - ta[u];
        float ac = fmaxf(a, 1e-3f);
        float ad = 1.0f / ac;
        float zd = ad - tda[u];
        float g1 = (z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f)) * isc;
        float g2 = 0.f;
        if (a >= 1e-3f) g2 = (zd > 0.f ? 1.f : (zd < 0.f ? -1.f : 0.f)) * iscd * (-1.0f / (ac * ac));
        double g = (double)g1 + (double)p.dw * (double)g2;
        gs += g * (double)xv;
        gt += g;
        l1 += fabs((double)z) * (double)isc;
        l2 += fabs((double)zd) * (double)iscd;
      }
    }
  }
  double v[4] = {gs, gt, l1, l2};
  block_sums_d<4>(v);
  gs = v[0], gt = v[1], l1 = v[2], l2 = v[3];
  if (threadIdx.x == 0) {
    const long o = (long)gk * PS + c;
    if (COHERENT) {
      __hip_atomic_store(&p.gs[o], gs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&p.gt[o], gt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      p.gs[o] = gs;
      p.gt[o] = gt;
    }
    l1o[o] = l1;
    l2o[o] = l2;
  }
}

template <bool SS>
__global__ __launch_bounds__(256) void snippet_grad(AlP p) {
  snippet_grad_body<false, SS>(p, blockIdx.x, blockIdx.y, p.l1, p.l2);
}

// Loss-history row of iteration `step` (the closure's loss.item(), summ.min(), summ.max(), :213) from
// that iteration's loss partials l1/l2 [ntot·PS], chunk min/max mm(i) over N·PS chunks and the
// parameters BEFORE its update (sflat = [s | t] by global snippet index, or NULL: p.s / p.t).
template <typename MM>
__device__ __forceinline__ void hist_row(const AlP& p, int step, double denom, const double* l1, const double* l2,
                                         const float* sflat, MM mm) {
  __shared__ double sh[8];
  double L1 = 0.0, L2 = 0.0, soft = 0.0;
  for (int i = threadIdx.x; i < p.ntot * PS; i += 256) {
    L1 += l1[i];
    L2 += l2[i];
  }
  L1 = block_sum_d<256>(L1, sh);
  L2 = block_sum_d<256>(L2, sh);
  for (int d = 0; d < p.nd; ++d) {
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < p.n[d]; k += 256) {
      const float sv = sflat ? sflat[p.off[d] + k] : p.s[d][k];
      const float tv = sflat ? sflat[p.ntot + p.off[d] + k] : p.t[d][k];
      float r = fmaxf(0.f, 1.f - sv);
      a += (double)r * r;
      b += (double)tv * tv;
    }
    a = block_sum_d<256>(a, sh);
    b = block_sum_d<256>(b, sh);
    soft += p.lmda2 * a / p.n[d] + p.lmda3 * b / p.n[d];
  }
  float mn = INFINITY, mx = -INFINITY;
  for (long i = threadIdx.x; i < (long)p.N * PS; i += 256) {
    float lo, hi;
    mm(i, lo, hi);
    mn = fminf(mn, lo);
    mx = fmaxf(mx, hi);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  __shared__ float rmm[2][4];
  if ((threadIdx.x & 63) == 0) {
    rmm[0][threadIdx.x >> 6] = mn;
    rmm[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mn = fminf(fminf(rmm[0][0], rmm[0][1]), fminf(rmm[0][2], rmm[0][3]));
    mx = fmaxf(fmaxf(rmm[1][0], rmm[1][1]), fmaxf(rmm[1][2], rmm[1][3]));
    float* h = p.hist + 3L * (step - 1);
    h[0] = (float)(p.ls * (L1 / denom + p.dw * L2 / denom) + soft);
    h[1] = mn;
    h[2] = mx;
  }
  __syncthreads();
}

// torch.optim.Adam's update of parameter i (i < ntot: s of global snippet i, else t of i − ntot) at
// iteration `step`, its gradient = Σ_c of the chunk partials (chunk order fixed) · loss_scale/numel +
// the soft-constraint term.  Returns the parameter value before the update.
template <bool COHERENT>
__device__ __forceinline__ float adam_param(const AlP& p, int i, int step, double denom) {
  const double bc1 = p.bct[2 * step], bc2 = p.bct[2 * step + 1];
  const float step_size = (float)(p.lr / bc1);
  const float bc2s = (float)sqrt(bc2);
  const float lw = 1.0f - p.b1;   // lerp weight (1 - beta1)
  const float vw = 1.0f - p.b2;   // addcmul value (1 - beta2)
  const float gscale = (float)(p.ls / denom);
  const bool is_t = i >= p.ntot;
  const int gk = is_t ? i - p.ntot : i;
  int d = 0;
  while (d + 1 < p.nd && gk >= p.off[d + 1]) ++d;
  const int k = gk - p.off[d];
  float* prm = is_t ? &p.t[d][k] : &p.s[d][k];
  const float pv = *prm;
  const double* gp = (is_t ? p.gt : p.gs) + (long)gk * PS;
  double gsum = 0.0;
  for (int c = 0; c < PS; ++c)
    gsum += COHERENT ? __hip_atomic_load(gp + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : gp[c];
  float g = (float)(gsum * (double)gscale);
  const float nd = (float)p.n[d];
  if (!is_t) {
    float r = fmaxf(0.f, 1.f - pv);
    g = addrn(g, mulrn(mulrn(mulrn(p.lmda2, 2.0f), r), -1.0f) / nd);
  } else {
    g = addrn(g, mulrn(mulrn(p.lmda3, 2.0f), pv) / nd);
  }
  float m = p.m[i], v = p.v[i];
  const float diff = g - m;
  m = (lw < 0.5f) ? addrn(m, mulrn(lw, diff)) : g - mulrn(diff, 1.0f - lw);
  v = addrn(mulrn(v, p.b2), mulrn(mulrn(vw, g), g));
  const float den = addrn(sqrtf(v) / bc2s, p.eps);
  *prm = addrn(pv, mulrn(-step_size, m) / den);
  p.m[i] = m;
  p.v[i] = v;
  return pv;
}

__global__ __launch_bounds__(256) void adam_step(AlP p, int step, double denom) {
  // loss history (uses the parameters BEFORE this update, like the closure's loss)
  if (p.hist)
    hist_row(p, step, denom, p.l1, p.l2, nullptr, [&](long i, float& lo, float& hi) {
      lo = (float)p.fpart[i * 4 + 2];
      hi = (float)p.fpart[i * 4 + 3];
    });
  for (int i = threadIdx.x; i < 2 * p.ntot; i += 256) adam_param<false>(p, i, step, denom);
}

// snippet_grad with Adam fused in (the default loop: two launches per iteration).  The workgroup
// that finishes the LAST pixel chunk of snippet gk (a per-snippet arrival counter) applies Adam to
// s_gk and t_gk right there: their gradients need nothing else, and every reader of s_gk, t_gk in
// this launch is one of those chunks.  The hand-off is NOT a C++ release/acquire: the partials are
// relaxed agent-scope atomic stores, thread 0 waits for them with s_waitcnt vmcnt(0) (on gfx9 —
// this library is built for gfx950 only — vmcnt counts stores, and agent-scope atomics bypass the
// non-coherent caches, so they are visible device-wide once counted), then arrives with a relaxed
// fetch_add; the last arriver reads the partials as relaxed agent-scope atomic loads.  A true
// agent-scope release/acquire writes back / invalidates the XCD's whole L2 (1.6x slower loop).
// The loss history is deferred: the iteration's loss partials (hl), pre-update parameters (hst)
// and, in frame_stats, chunk min/max (hmm) go to per-iteration slots, and aligner_history turns
// each block of HBLK iterations into rows.  Same arithmetic in the same order as snippet_grad + adam_step: bitwise the
// same results (tests/test_aligner_gpu.py::test_aligner_fused_loop_bitwise).
template <bool SS>
__global__ __launch_bounds__(256) void snippet_grad_adam(AlP p, int it, long slot, double denom, unsigned* cnt,
                                                         double* hl, float* hst) {
  const long nps = (long)p.ntot * PS;
  const int gk = blockIdx.x;
  double* l1o = hl ? hl + slot * 2 * nps : p.l1;
  snippet_grad_body<true, SS>(p, gk, blockIdx.y, l1o, l1o + nps);
  // Hand-off without cache maintenance (see above): the partials were stored as agent-scope atomics
  // by thread 0, which waits for their completion (vmcnt) before it arrives; the last arriver reads
  // them the same way.
  __shared__ unsigned last;
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(&cnt[gk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == PS - 1;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x < 2) {
    const int i = threadIdx.x ? p.ntot + gk : gk;
    const float pv = adam_param<true>(p, i, it, denom);
    if (hst) hst[slot * 2 * p.ntot + i] = pv;
  }
  if (threadIdx.x == 0) cnt[gk] = 0u;  // re-armed for the next iteration (next launch)
}

template <bool SS>
__global__ __launch_bounds__(256) void frame_stats_hist(AlP p, float* hmm) {
  const int f = blockIdx.x, c = blockIdx.y;
  float mn, mx;
  frame_stats_body<SS>(p, f, c, mn, mx);
  if (hmm && threadIdx.x == 0) {
    hmm[((long)f * PS + c) * 2] = mn;
    hmm[((long)f * PS + c) * 2 + 1] = mx;
  }
}

// History rows of the fused loop for iterations it0 .. it0+gridDim.x-1, one workgroup per iteration;
// their per-iteration slots are slots 0 .. gridDim.x-1 (the loop writes iteration it into slot
// (it − 1) mod HBLK and turns every block of HBLK iterations into rows before reusing the slots).
__global__ __launch_bounds__(256) void aligner_history(AlP p, double denom, const double* hl, const float* hmm,
                                                       const float* hst, int it0) {
  const int slot = blockIdx.x, it = it0 + blockIdx.x;
  const long nps = (long)p.ntot * PS, nfs = (long)p.N * PS;
  const double* l1 = hl + (long)slot * 2 * nps;
  const float* mm = hmm + (long)slot * nfs * 2;
  hist_row(p, it, denom, l1, l1 + nps, hst + (long)slot * 2 * p.ntot, [&](long i, float& lo, float& hi) {
    lo = mm[i * 2];
    hi = mm[i * 2 + 1];
  });
}

// Adam's bias corrections of every step, once per optimisation (the same double pow the update
// evaluated per parameter before: two double pows off each iteration's critical path)
__global__ void adam_bc_k(AlP p, int iters, double* bct) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= iters; i += gridDim.x * blockDim.x) {
    bct[2 * i] = 1.0 - pow((double)p.b1, (double)i);
    bct[2 * i + 1] = 1.0 - pow((double)p.b2, (double)i);
  }
}

__global__ void zero_f32(float* x, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] = 0.f;
}

struct MergeP {
  const void* x[MAXD];
  const float* s[MAXD];
  const float* t[MAXD];
  int n[MAXD], stride[MAXD], w[MAXD];
  int k0[MAXD], nloc[MAXD];  // rows of x[d] are global snippets k0[d] .. k0[d]+nloc[d]-1
  int ss[MAXD], last[MAXD];  // start step, start of the last window (aligner_index.h; the SS = true kernels only)
  int nd, xf32;
  int sum_only;              // 1: write the per-frame f64 sum (sharded merge) to dsum, 0: the mean to out
  int f0;                    // first frame of out (out rows are frames f0 .. f0+gridDim.y-1)
  long HW;
  const float* shift;
  float* out;
  double* dsum;
};

// number of (dilation, slot) pairs covering frame f (the B.sum(0) of depth_aligner.py:190 / the
// length of the torch.cat of :258)
__device__ __forceinline__ int cover_count(const int* n, const int* stride, int nd, const int* w, int f) {
  int cnt = 0;
  for (int d = 0; d < nd; ++d)
    for (int j = 0; j < w[d]; ++j) {
      const int k = f - j * stride[d];
      cnt += (k >= 0 && k < n[d]) ? 1 : 0;
    }
  return cnt;
}

// The f32-arithmetic merges (x_f32 1 / 2) add the slots' f32 terms s·x + t in f64: the sum of a
// frame's few (≤ Σ w_d) f32 terms is exact whenever their exponents span ≤ ≈29 bits (all but rare
// rounding cases), so it does not depend on the order the terms are added in — the sharded merge (per-rank window sums, all-to-all, pieces added per frame, finish)
// gives bitwise the single-GPU result, and both round once, at the mean.  The f16-emulating mode 0
// (the reference's fp16 merge, RDMI_MERGE_F32=0) keeps its f32 running sum.
template <bool SS>
__global__ void merge_k(MergeP p) {
  const int f = p.f0 + blockIdx.y;
  const float sh = p.shift ? p.shift[0] : 0.f;
  for (long px = blockIdx.x * (long)blockDim.x + threadIdx.x; px < p.HW; px += (long)gridDim.x * blockDim.x) {
    float sum = 0.f;
    double dsum = 0.0;
    int cnt = 0;
    for (int d = 0; d < p.nd; ++d) {
      for (int j = p.w[d] - 1; j >= 0; --j) {  // boolean-mask order over [n_d, w]: k ascending
        const int q = f - j * p.stride[d];
        int k = SS ? rdmi_snip_at(q, p.ss[d], p.last[d], p.n[d]) : q;
        if (k < p.k0[d] || k >= p.k0[d] + p.nloc[d]) continue;
        long off = ((long)(k - p.k0[d]) * p.w[d] + j) * p.HW + px;
        float a;
        if (p.xf32 == 1) {
          float xs = ((const float*)p.x[d])[off] - sh;
          a = addrn(mulrn(xs, p.s[d][k]), p.t[d][k]);
        } else if (p.xf32 == 2) {  // f16 snippets, f32 arithmetic (no intermediate f16 rounding)
          float xs = (float)((const f16*)p.x[d])[off] - sh;
          a = addrn(mulrn(xs, p.s[d][k]), p.t[d][k]);
        } else {
          f16 xs = (f16)((float)((const f16*)p.x[d])[off] - sh);
          f16 sc = (f16)p.s[d][k], tr = (f16)p.t[d][k];
          f16 prod = (f16)((float)xs * (float)sc);
          a = (float)(f16)((float)prod + (float)tr);
        }
        if (p.xf32)
          dsum += (double)a;
        else
          sum = addrn(sum, a);
        ++cnt;
      }
    }
    const long o = (long)blockIdx.y * p.HW + px;
    if (p.sum_only)
      p.dsum[o] = p.xf32 ? dsum : (double)sum;
    else
      p.out[o] = p.xf32 ? (cnt ? (float)(dsum / (double)cnt) : 0.f) : (cnt ? sum / (float)cnt : 0.f);
  }
}

// sharded merge with frame windows, second half: the received pieces — piece q holds the sums of
// frames pf0[q] .. pf0[q]+pnf[q]-1 from one source rank, pieces back to back in `recv` — added per
// frame in piece (= source rank) order, ÷ the frame's cover count.  Frames of this rank's chunk that
// no piece covers are 0 (no slot covers them: cover count 0).
constexpr int MAXPIECES = 64;
struct PiecesP {
  int pf0[MAXPIECES], pnf[MAXPIECES];
  long poff[MAXPIECES];
  int np;
};

template <bool SS>
__global__ void merge_finish_pieces_k(MergeP p, PiecesP q, const double* __restrict__ recv) {
  const int fl = blockIdx.y, f = p.f0 + fl;
  const int cnt = SS ? rdmi_cover_count(p.nd, p.n, p.stride, p.w, p.ss, p.last, f)
                     : cover_count(p.n, p.stride, p.nd, p.w, f);
  for (long px = blockIdx.x * (long)blockDim.x + threadIdx.x; px < p.HW; px += (long)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int i = 0; i < q.np; ++i)
      if (f >= q.pf0[i] && f < q.pf0[i] + q.pnf[i]) s += recv[q.poff[i] + (long)(f - q.pf0[i]) * p.HW + px];
    p.out[(long)fl * p.HW + px] = cnt ? (float)(s / (double)cnt) : 0.f;
  }
}

struct PrepP {
  const void* x;
  int xf32;
  int n, w, H, W, border, factor, Hs, Ws;
  const float* shift;
  float* out;
};

__global__ void prepare_k(PrepP p) {
  const long P = (long)p.Hs * p.Ws;
  const long total = (long)p.n * p.w * P;
  const float sh = p.shift[0];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long img = i / P, q = i - img * P;
    int ys = (int)(q / p.Ws), xs = (int)(q - (long)ys * p.Ws);
    long src = img * p.H * p.W + (long)(p.border + ys * p.factor) * p.W + (p.border + xs * p.factor);
    float v;
    if (p.xf32)
      v = ((const float*)p.x)[src] - sh;
    else
      v = (float)(f16)((float)((const f16*)p.x)[src] - sh);
    p.out[i] = v;
  }
}

// RDMI_ALIGNER_FUSED (read per call: A/B and the bitwise tests): 0 the three-kernel loop, anything else
// or unset the two-launch loop (default).  The workspace is the same for both (aligner_ws.h).
int loop_mode() {
  const char* e = getenv("RDMI_ALIGNER_FUSED");
  return e && e[0] == '0' ? 0 : 1;
}

bool any_start_step(int nd, const int* start_step) {
  for (int d = 0; start_step && d < nd && d < MAXD; ++d)
    if (start_step[d] > 1) return true;
  return false;
}

// The start steps of a job (NULL or 0: 1) → ss[d], last[d]; *strided: some start step is > 1.  Only then
// is the snippet layout checked against the index map (aligner_index.h), before any launch: every start
// step ≥ 0, a window fits the N frames, n[d] is the count the map gives.
int start_steps(const char* what, int nd, const int* start_step, const int* n, const int* stride, const int* w, int N,
                int* ss, int* last, bool* strided) {
  *strided = any_start_step(nd, start_step);
  for (int d = 0; d < nd; ++d) {
    const int v = start_step ? start_step[d] : 1;
    RDMI_REQUIRE(v >= 0, RDMI_E_ARG, "%s: start step %d of dilation %d", what, v, d);
    ss[d] = v ? v : 1;
    last[d] = rdmi_snip_last(N, w[d], stride[d]);
    if (!*strided) continue;
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

}  // namespace

extern "C" long rdmi_aligner_workspace(const rdmi_aligner_args* a) {
  int ntot = 0;
  for (int d = 0; d < a->n_dil; ++d) ntot += a->n[d];
  return rdmi_aligner_ws_layout(a->seq_len, a->P, ntot, a->iters, a->history != nullptr).total;
}

extern "C" int rdmi_aligner_optimize(const rdmi_aligner_args* a, void* stream) {
  RDMI_REQUIRE(a && a->workspace && a->n_dil >= 1 && a->n_dil <= MAXD && a->P > 0 && a->seq_len > 0,
               RDMI_E_ARG, "aligner_optimize: bad args");
  hipStream_t st = (hipStream_t)stream;
  AlP p{};
  p.nd = a->n_dil;
  p.N = a->seq_len;
  p.P = a->P;
  int ntot = 0;
  for (int d = 0; d < p.nd; ++d) {
    RDMI_REQUIRE(a->x[d] && a->s[d] && a->t[d] && a->n[d] > 0, RDMI_E_ARG, "aligner_optimize: dilation %d", d);
    p.x[d] = a->x[d];
    p.s[d] = a->s[d];
    p.t[d] = a->t[d];
    p.n[d] = a->n[d];
    p.stride[d] = a->stride[d];
    p.off[d] = ntot;
    ntot += a->n[d];
    RDMI_REQUIRE(a->w[d] >= 1, RDMI_E_ARG, "aligner_optimize: snippet length %d of dilation %d", a->w[d], d);
    p.w[d] = a->w[d];
    p.R += a->w[d];
  }
  RDMI_REQUIRE(p.R <= MAXR, RDMI_E_ARG, "aligner_optimize: %d rows (at most %d)", p.R, MAXR);
  bool strided = false;
  if (int rc = start_steps("aligner_optimize", p.nd, a->start_step, p.n, p.stride, p.w, p.N, p.ss, p.last, &strided))
    return rc;
  for (int d = 0; d < p.nd; ++d) {
    p.rb[d] = d * p.w[d];  // the reference's torch.arange(i * w, (i + 1) * w), depth_aligner.py:182-188
    RDMI_REQUIRE(a->iters == 0 || p.rb[d] + p.w[d] <= p.R, RDMI_E_ARG,
                 "aligner_optimize: dilation %d rows %d..%d exceed the %d rows (the reference raises IndexError)", d,
                 p.rb[d], p.rb[d] + p.w[d] - 1, p.R);
  }
  p.ntot = ntot;
  p.lr = a->lr; p.b1 = a->beta1; p.b2 = a->beta2; p.eps = a->eps;
  p.lmda2 = a->lmda2; p.lmda3 = a->lmda3; p.dw = a->depth_w; p.ls = a->loss_scale;
  float* w = a->workspace;
  RDMI_REQUIRE(((uintptr_t)w & 7) == 0, RDMI_E_ALIGN, "aligner: workspace must be 8-byte aligned");
  p.hist = a->history;
  const rdmi_aligner_layout L = rdmi_aligner_ws_layout(p.N, p.P, ntot, a->iters, p.hist != nullptr);
  p.gs = (double*)(w + L.gs); p.gt = (double*)(w + L.gt); p.l1 = (double*)(w + L.l1); p.l2 = (double*)(w + L.l2);
  p.fpart = (double*)(w + L.fpart);
  p.T = w + L.T;
  p.Td = w + L.Td;
  p.m = w + L.m;
  p.v = w + L.v;
  unsigned* cnt = (unsigned*)(w + L.cnt);
  double* bct = (double*)(w + L.bct);
  p.bct = bct;
  const double denom = (double)p.R * p.N * (double)p.P;  // numel of the [Σw, N, P] loss tensor
  hipLaunchKernelGGL(zero_f32, dim3(16), dim3(256), 0, st, p.m, L.bct - L.m);  // m, v, cnt: contiguous
  hipLaunchKernelGGL(adam_bc_k, dim3(8), dim3(256), 0, st, p, a->iters, bct);
  int rc = rdmi::check_launch("aligner_zero");
  if (rc) return rc;
  if (loop_mode() != 0) {
    double* hl = p.hist ? (double*)(w + L.hl) : nullptr;
    float* hmm = p.hist ? w + L.hmm : nullptr;
    float* hst = p.hist ? w + L.hst : nullptr;
    int it0 = 1;  // first iteration whose history slots are not yet turned into rows
    for (int it = 1; it <= a->iters; ++it) {
      const long slot = (it - 1) % HBLK;
      float* hmms = hmm ? hmm + slot * 2 * p.N * PS : nullptr;
      if (strided) {
        hipLaunchKernelGGL(frame_stats_hist<true>, dim3(p.N, PS), dim3(256), 0, st, p, hmms);
        hipLaunchKernelGGL(snippet_grad_adam<true>, dim3(ntot, PS), dim3(256), 0, st, p, it, slot, denom, cnt, hl, hst);
      } else {
        hipLaunchKernelGGL(frame_stats_hist<false>, dim3(p.N, PS), dim3(256), 0, st, p, hmms);
        hipLaunchKernelGGL(snippet_grad_adam<false>, dim3(ntot, PS), dim3(256), 0, st, p, it, slot, denom, cnt, hl, hst);
      }
      rc = rdmi::check_launch("aligner_iteration");
      if (rc) return rc;
      if (p.hist && (it - it0 + 1 == HBLK || it == a->iters)) {
        hipLaunchKernelGGL(aligner_history, dim3(it - it0 + 1), dim3(256), 0, st, p, denom, (const double*)hl,
                           (const float*)hmm, (const float*)hst, it0);
        rc = rdmi::check_launch("aligner_history");
        if (rc) return rc;
        it0 = it + 1;
      }
    }
    return 0;
  }
  for (int it = 1; it <= a->iters; ++it) {
    if (strided) {
      hipLaunchKernelGGL(frame_stats<true>, dim3(p.N, PS), dim3(256), 0, st, p);
      hipLaunchKernelGGL(snippet_grad<true>, dim3(ntot, PS), dim3(256), 0, st, p);
    } else {
      hipLaunchKernelGGL(frame_stats<false>, dim3(p.N, PS), dim3(256), 0, st, p);
      hipLaunchKernelGGL(snippet_grad<false>, dim3(ntot, PS), dim3(256), 0, st, p);
    }
    hipLaunchKernelGGL(adam_step, dim3(1), dim3(256), 0, st, p, it, denom);
    rc = rdmi::check_launch("aligner_iteration");
    if (rc) return rc;
  }
  return 0;
}

extern "C" int rdmi_aligner_prepare(const void* x, int x_f32, int n, int w, int H, int W, int border, int factor,
                                    const float* shift, float* out, void* stream) {
  RDMI_REQUIRE(x && shift && out && H > 2 * border && W > 2 * border && factor > 0, RDMI_E_ARG,
               "aligner_prepare: bad args");
  PrepP p{x, x_f32, n, w, H, W, border, factor, (H - 2 * border + factor - 1) / factor,
          (W - 2 * border + factor - 1) / factor, shift, out};
  long total = (long)n * w * p.Hs * p.Ws;
  long g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(prepare_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, p);
  return rdmi::check_launch("aligner_prepare");
}

static int merge_launch(int n_dil, const void* const* xf, int x_f32, const float* const* s, const float* const* t,
                        const int* n, const int* stride, const int* k0, const int* nloc, const int* w, int f0, int nf,
                        long HW, const float* shift, float* out, double* dsum, void* stream,
                        const int* start_step = nullptr, int seq_len = 0) {
  RDMI_REQUIRE(n_dil >= 1 && n_dil <= MAXD && (out || dsum) && HW > 0 && nf >= 0 && f0 >= 0, RDMI_E_ARG,
               "aligner_merge: bad args");
  MergeP p{};
  for (int d = 0; d < n_dil; ++d) {
    const int kk = k0 ? k0[d] : 0, nl = nloc ? nloc[d] : n[d];
    RDMI_REQUIRE(kk >= 0 && nl >= 0 && kk + nl <= n[d] && w[d] >= 1 && (nl == 0 || (xf[d] && s[d] && t[d])),
                 RDMI_E_ARG, "aligner_merge: dilation %d rows %d+%d of %d, length %d", d, kk, nl, n[d], w[d]);
    p.x[d] = xf[d];
    p.s[d] = s[d];
    p.t[d] = t[d];
    p.n[d] = n[d];
    p.stride[d] = stride[d];
    p.k0[d] = kk;
    p.nloc[d] = nl;
    p.w[d] = w[d];
  }
  p.nd = n_dil; p.xf32 = x_f32; p.HW = HW; p.shift = shift; p.out = out; p.dsum = dsum;
  p.sum_only = dsum != nullptr; p.f0 = f0;
  bool strided = false;
  if (start_step)
    if (int rc = start_steps("aligner_merge_strided", n_dil, start_step, p.n, p.stride, p.w, seq_len, p.ss, p.last,
                             &strided))
      return rc;
  if (nf == 0) return 0;
  long gx = (HW + 255) / 256;
  if (gx > 1024) gx = 1024;
  if (strided)
    hipLaunchKernelGGL(merge_k<true>, dim3((unsigned)gx, nf), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(merge_k<false>, dim3((unsigned)gx, nf), dim3(256), 0, (hipStream_t)stream, p);
  return rdmi::check_launch("aligner_merge");
}

extern "C" int rdmi_aligner_merge(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                  const float* const* t, const int* n, const int* stride, const int* w, int seq_len, long HW,
                                  const float* shift, float* out, void* stream) {
  RDMI_REQUIRE(out, RDMI_E_ARG, "aligner_merge: null out");
  return merge_launch(n_dil, xf, x_f32, s, t, n, stride, nullptr, nullptr, w, 0, seq_len, HW, shift, out, nullptr,
                      stream);
}

extern "C" int rdmi_aligner_merge_strided(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                          const float* const* t, const int* n, const int* stride,
                                          const int* start_step, const int* w, int seq_len, long HW,
                                          const float* shift, float* out, void* stream) {
  RDMI_REQUIRE(out && start_step && n && stride && w, RDMI_E_ARG, "aligner_merge_strided: null argument");
  return merge_launch(n_dil, xf, x_f32, s, t, n, stride, nullptr, nullptr, w, 0, seq_len, HW, shift, out, nullptr,
                      stream, start_step, seq_len);
}

extern "C" int rdmi_aligner_merge_partial_window(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                                 const float* const* t, const int* n, const int* stride, const int* k0,
                                                 const int* nloc, const int* w, int f0, int nf, long HW,
                                                 const float* shift, double* sum_out, void* stream) {
  RDMI_REQUIRE(k0 && nloc && sum_out, RDMI_E_ARG, "aligner_merge_partial_window: k0/nloc/sum_out required");
  return merge_launch(n_dil, xf, x_f32, s, t, n, stride, k0, nloc, w, f0, nf, HW, shift, nullptr, sum_out, stream);
}

extern "C" int rdmi_aligner_merge_partial_window_strided(int n_dil, const void* const* xf, int x_f32,
                                                         const float* const* s, const float* const* t, const int* n,
                                                         const int* stride, const int* start_step, const int* k0,
                                                         const int* nloc, const int* w, int seq_len, int f0, int nf,
                                                         long HW, const float* shift, double* sum_out, void* stream) {
  RDMI_REQUIRE(k0 && nloc && sum_out && start_step && n && stride && w, RDMI_E_ARG,
               "aligner_merge_partial_window_strided: null argument");
  RDMI_REQUIRE(f0 >= 0 && nf >= 0 && f0 <= seq_len && nf <= seq_len - f0, RDMI_E_ARG,
               "aligner_merge_partial_window_strided: frames %d+%d outside the %d of the sequence", f0, nf, seq_len);
  return merge_launch(n_dil, xf, x_f32, s, t, n, stride, k0, nloc, w, f0, nf, HW, shift, nullptr, sum_out, stream,
                      start_step, seq_len);
}

static int finish_pieces_launch(int n_dil, const int* n, const int* stride, const int* w, int f0, int nf, long HW,
                                int npieces, const int* piece_f0, const int* piece_nf, const double* recv, float* out,
                                void* stream, const int* start_step = nullptr, int seq_len = 0) {
  RDMI_REQUIRE(n_dil >= 1 && n_dil <= MAXD && n && stride && w && (out || nf == 0) && HW > 0 && f0 >= 0 && nf >= 0 &&
                   npieces >= 0 && (npieces == 0 || (piece_f0 && piece_nf && recv)),
               RDMI_E_ARG, "aligner_merge_finish_pieces: bad args");
  MergeP p{};
  for (int d = 0; d < n_dil; ++d) {
    p.n[d] = n[d];
    p.stride[d] = stride[d];
    p.w[d] = w[d];
  }
  p.nd = n_dil; p.HW = HW;
  bool strided = false;
  if (start_step)
    if (int rc = start_steps("aligner_merge_finish_pieces_strided", n_dil, start_step, p.n, p.stride, p.w, seq_len,
                             p.ss, p.last, &strided))
      return rc;
  if (nf == 0) return 0;
  long off = 0;
  for (int i = 0; i < npieces; ++i) {
    RDMI_REQUIRE(piece_nf[i] >= 0 && piece_f0[i] >= f0 && piece_f0[i] + piece_nf[i] <= f0 + nf, RDMI_E_ARG,
                 "aligner_merge_finish_pieces: piece %d frames %d+%d outside %d+%d", i, piece_f0[i], piece_nf[i], f0, nf);
  }
  // The piece table travels in the kernel arguments (≤ MAXPIECES entries).  More pieces than that (one
  // per source rank and dilation: 3·W > 64 from W = 22 ranks on) are split by frame: each launch takes
  // a frame range and only the pieces that touch it, in their original (source-rank) order — every
  // frame still adds all of its pieces in that order within one thread, so the sums are those of a
  // single launch.  Only a single frame touched by more than MAXPIECES pieces is refused.
  auto touches = [&](int i, int a, int b) { return piece_nf[i] > 0 && piece_f0[i] < b && piece_f0[i] + piece_nf[i] > a; };
  long gx = (HW + 255) / 256;
  if (gx > 1024) gx = 1024;
  int fs = f0;
  while (fs < f0 + nf) {
    int fe = fs + 1, cnt = 0;
    for (int i = 0; i < npieces; ++i) cnt += touches(i, fs, fe);
    RDMI_REQUIRE(cnt <= MAXPIECES, RDMI_E_UNSUPPORTED,
                 "aligner_merge_finish_pieces: frame %d is covered by %d pieces (at most %d)", fs, cnt, MAXPIECES);
    while (fe < f0 + nf) {  // grow the range while its pieces still fit the table
      int c2 = 0;
      for (int i = 0; i < npieces; ++i) c2 += touches(i, fs, fe + 1);
      if (c2 > MAXPIECES) break;
      ++fe;
    }
    PiecesP q{};
    off = 0;
    for (int i = 0; i < npieces; ++i) {
      if (touches(i, fs, fe)) {
        q.pf0[q.np] = piece_f0[i];
        q.pnf[q.np] = piece_nf[i];
        q.poff[q.np] = off;
        ++q.np;
      }
      off += (long)piece_nf[i] * HW;
    }
    p.f0 = fs;
    p.out = out + (long)(fs - f0) * HW;
    if (strided)
      hipLaunchKernelGGL(merge_finish_pieces_k<true>, dim3((unsigned)gx, fe - fs), dim3(256), 0, (hipStream_t)stream, p,
                         q, recv);
    else
      hipLaunchKernelGGL(merge_finish_pieces_k<false>, dim3((unsigned)gx, fe - fs), dim3(256), 0, (hipStream_t)stream,
                         p, q, recv);
    if (int rc = rdmi::check_launch("aligner_merge_finish_pieces")) return rc;
    fs = fe;
  }
  return 0;
}

extern "C" int rdmi_aligner_merge_finish_pieces(int n_dil, const int* n, const int* stride, const int* w, int f0,
                                                int nf, long HW, int npieces, const int* piece_f0,
                                                const int* piece_nf, const double* recv, float* out, void* stream) {
  return finish_pieces_launch(n_dil, n, stride, w, f0, nf, HW, npieces, piece_f0, piece_nf, recv, out, stream);
}

extern "C" int rdmi_aligner_merge_finish_pieces_strided(int n_dil, const int* n, const int* stride,
                                                        const int* start_step, const int* w, int seq_len, int f0,
                                                        int nf, long HW, int npieces, const int* piece_f0,
                                                        const int* piece_nf, const double* recv, float* out,
                                                        void* stream) {
  RDMI_REQUIRE(start_step, RDMI_E_ARG, "aligner_merge_finish_pieces_strided: null start_step");
  RDMI_REQUIRE(f0 >= 0 && nf >= 0 && f0 <= seq_len && nf <= seq_len - f0, RDMI_E_ARG,
               "aligner_merge_finish_pieces_strided: frames %d+%d outside the %d of the sequence", f0, nf, seq_len);
  return finish_pieces_launch(n_dil, n, stride, w, f0, nf, HW, npieces, piece_f0, piece_nf, recv, out, stream,
                              start_step, seq_len);
}

// ------------------------------------------------------------------------------------------------
// Merge with the per-pixel spread of the merged terms (since rdmi_version 6).  A frame's covering terms
// a_i = s_k·(x − shift) + t_k, i = 1 … c, are the values merge_k forms in each x_f32 mode, visited in
// its (d ascending, j descending) order; beside their mean the kernels below keep Σa and Σa² in f64
// (a² of an f32 a is exact in f64) and write the population standard deviation
//   sqrt(max(0, Σa²/c − (Σa/c)²)),  evaluated in f64 and rounded once to f32,  0 where c ≤ 1.
// The f64 accumulation error of both sums is at most (c + 4)·2⁻⁵²·max a² in the variance.
// The mean is merge_k's, bitwise: f64 sum ÷ c rounded once in modes 1 / 2, the f32 running sum in mode 0
// (whose spread still comes from f64 sums of the same f16-rounded terms).
//
// An HBM-bound stream: every snippet pixel is read once.  Which snippet covers frame f in slot (d, j) is the
// same for the whole block, so the first wave resolves it once per block into an LDS table (row pointer,
// s, t), compacted in merge_k's order by a ballot; the pixel loop then only walks that table.  On the
// vector path (HW % 4 == 0, every base pointer 16-byte aligned) a lane owns 4 consecutive pixels: 16-byte
// loads of f32 rows, 8-byte loads of f16 rows, up to MOM_U rows' loads issued before the first is used.
namespace {

constexpr int MOM_U = 8;  // table rows whose loads are issued together (the fast preset has ≤ 6 per frame)
// Pixel groups per thread the grid is sized for: a block resolves its frame's table once for 4 · 256 groups.
// 100 × 768² f32, 98 + 50 snippets: 0.307 ms for 2 and 4, 0.314 for 8, 0.341 for 1 (profiles/merge_moments_probe.log)
constexpr int MOM_ITER = 4;

struct MomP {
  MergeP m;        // out = the mean (fused form); dsum unused
  float* std_out;  // fused form
  double* mom;     // sum-only form: [nf][2][HW], Σa then Σa² per frame (NULL: fused form)
};

struct MomEnt {
  const char* row;  // the covering snippet's slot row [HW]
  float s, t;
};

// The covering (d, j) of frame f among the rows this call holds, in merge_k's order → tab[0 .. c).
// Σ w_d ≤ MAXR = 64: one lane of the first wave per (d, j).
template <bool SS>
__device__ __forceinline__ int moments_table(const MergeP& p, int f, MomEnt* tab, int* cnt) {
  if (threadIdx.x < 64) {
    const int i = threadIdx.x;
    const int esz = p.xf32 == 1 ? 4 : 2;
    bool ok = false;
    MomEnt e{nullptr, 0.f, 0.f};
    int base = 0;
    for (int d = 0; d < p.nd; ++d) {  // d is uniform: the job's fields are read with scalar indices
      const int r = i - base;
      base += p.w[d];
      if (r < 0 || r >= p.w[d]) continue;
      const int j = p.w[d] - 1 - r;
      const int q = f - j * p.stride[d];
      const int k = SS ? rdmi_snip_at(q, p.ss[d], p.last[d], p.n[d]) : q;
      if (k < p.k0[d] || k >= p.k0[d] + p.nloc[d]) continue;
      ok = true;
      e.row = (const char*)p.x[d] + ((long)(k - p.k0[d]) * p.w[d] + j) * p.HW * esz;
      e.s = p.s[d][k];
      e.t = p.t[d][k];
    }
    const unsigned long long mask = __ballot(ok);
    if (ok) tab[__popcll(mask & ((1ull << i) - 1ull))] = e;
    if (i == 0) *cnt = __popcll(mask);
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*cnt);
}

// V consecutive pixels of a row, from pixel px on, as f32 (the f16 → f32 conversion is exact)
template <int V, bool XF32>
__device__ __forceinline__ void mom_load(const char* row, long px, float (&v)[V]) {
  if constexpr (XF32) {
    const float* r = (const float*)row + px;
    if constexpr (V == 4) {
      const f32x4 x = *(const f32x4*)r;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = x[e];
    } else {
      v[0] = r[0];
    }
  } else {
    const f16* r = (const f16*)row + px;
    if constexpr (V == 4) {
      const f16x4 x = *(const f16x4*)r;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (float)x[e];
    } else {
      v[0] = (float)r[0];
    }
  }
}

// One term, exactly as merge_k forms it.  In the f32 modes that is ONE rounding of s·(x − shift) + t: hipcc
// compiles merge_k's addrn(mulrn(xs, s), t) to a single v_fmac_f32 (the __f*_rn intrinsics do not keep the
// product's rounding, the file's `fp contract(off)` notwithstanding), so the fused multiply-add is written
// out here; the mean's bitwise tests against merge_k hold the two together.
__device__ __forceinline__ float mom_term(float x, float sh, float s, float t, bool f16_chain) {
  if (!f16_chain) return __builtin_fmaf(x - sh, s, t);
  const f16 xs = (f16)(x - sh);
  const f16 sc = (f16)s, tr = (f16)t;
  const f16 prod = (f16)((float)xs * (float)sc);
  return (float)(f16)((float)prod + (float)tr);
}

__device__ __forceinline__ float mom_std(double s1, double s2, int c) {
  if (c <= 1) return 0.f;
  const double m1 = s1 / (double)c, m2 = s2 / (double)c;
  const double var = m2 - m1 * m1;
  return (float)sqrt(var > 0.0 ? var : 0.0);
}

template <bool SS, int V, bool XF32>
__global__ __launch_bounds__(256) void merge_moments_k(MomP pp) {
  __shared__ MomEnt tab[MAXR];
  __shared__ int cnt_sh;
  const MergeP& p = pp.m;
  const int fl = blockIdx.y, f = p.f0 + fl;
  const int c = moments_table<SS>(p, f, tab, &cnt_sh);
  const float sh = p.shift ? p.shift[0] : 0.f;
  const bool chain = p.xf32 == 0;
  const long groups = p.HW / V;  // V == 4 only when HW % 4 == 0
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long px = g * V;
    float sum[V];
    double s1[V], s2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) sum[v] = 0.f, s1[v] = 0.0, s2[v] = 0.0;
    for (int e0 = 0; e0 < c; e0 += MOM_U) {
      float x[MOM_U][V];
#pragma unroll
      for (int u = 0; u < MOM_U; ++u)
        if (e0 + u < c) mom_load<V, XF32>(tab[e0 + u].row, px, x[u]);
#pragma unroll
      for (int u = 0; u < MOM_U; ++u)
        if (e0 + u < c) {
          const float s = tab[e0 + u].s, t = tab[e0 + u].t;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const float a = mom_term(x[u][v], sh, s, t, chain);
            const double ad = (double)a;
            sum[v] = addrn(sum[v], a);
            s1[v] += ad;
            s2[v] += ad * ad;
          }
        }
    }
    if (pp.mom) {
      double* o1 = pp.mom + ((long)fl * 2) * p.HW + px;
      double* o2 = o1 + p.HW;
      if constexpr (V == 4) {
        typedef double f64x2 __attribute__((ext_vector_type(2)));
        *(f64x2*)o1 = f64x2{s1[0], s1[1]};
        *(f64x2*)(o1 + 2) = f64x2{s1[2], s1[3]};
        *(f64x2*)o2 = f64x2{s2[0], s2[1]};
        *(f64x2*)(o2 + 2) = f64x2{s2[2], s2[3]};
      } else {
        o1[0] = s1[0];
        o2[0] = s2[0];
      }
    } else {
      float mean[V], sd[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        mean[v] = chain ? (c ? sum[v] / (float)c : 0.f) : (c ? (float)(s1[v] / (double)c) : 0.f);
        sd[v] = mom_std(s1[v], s2[v], c);
      }
      const long o = (long)fl * p.HW + px;
      if constexpr (V == 4) {
        *(f32x4*)(p.out + o) = f32x4{mean[0], mean[1], mean[2], mean[3]};
        *(f32x4*)(pp.std_out + o) = f32x4{sd[0], sd[1], sd[2], sd[3]};
      } else {
        p.out[o] = mean[0];
        pp.std_out[o] = sd[0];
      }
    }
  }
}

// merge_finish_pieces_k for the two moments: recv holds [2][HW] per frame of a piece (q.poff counts
// doubles), both added per frame in piece (= source rank) order, ÷ the frame's cover count.
template <bool SS>
__global__ void merge_finish_moments_k(MergeP p, PiecesP q, const double* __restrict__ recv, float* std_out) {
  const int fl = blockIdx.y, f = p.f0 + fl;
  const int cnt = SS ? rdmi_cover_count(p.nd, p.n, p.stride, p.w, p.ss, p.last, f)
                     : cover_count(p.n, p.stride, p.nd, p.w, f);
  for (long px = blockIdx.x * (long)blockDim.x + threadIdx.x; px < p.HW; px += (long)gridDim.x * blockDim.x) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < q.np; ++i)
      if (f >= q.pf0[i] && f < q.pf0[i] + q.pnf[i]) {
        const double* r = recv + q.poff[i] + (long)(f - q.pf0[i]) * 2 * p.HW + px;
        s1 += r[0];
        s2 += r[p.HW];
      }
    p.out[(long)fl * p.HW + px] = cnt ? (float)(s1 / (double)cnt) : 0.f;
    std_out[(long)fl * p.HW + px] = mom_std(s1, s2, cnt);
  }
}

// The start steps of a moments call: always given, every one ≥ 1 (all ones: start step 1), and the layout
// always checked against the index map before any launch.
int moments_start_steps(const char* what, int nd, const int* start_step, const int* n, const int* stride,
                        const int* w, int N, int* ss, int* last, bool* strided) {
  *strided = false;
  for (int d = 0; d < nd; ++d) {
    RDMI_REQUIRE(start_step[d] >= 1, RDMI_E_ARG, "%s: start step %d of dilation %d (>= 1 expected)", what,
                 start_step[d], d);
    ss[d] = start_step[d];
    if (ss[d] > 1) *strided = true;
    RDMI_REQUIRE(stride[d] >= 1 && w[d] >= 1, RDMI_E_ARG, "%s: dilation %d: length %d, frame stride %d", what, d, w[d],
                 stride[d]);
    last[d] = rdmi_snip_last(N, w[d], stride[d]);
    RDMI_REQUIRE(last[d] >= 0, RDMI_E_ARG,
                 "%s: dilation %d: a snippet of length %d and frame stride %d does not fit %d frames", what, d, w[d],
                 stride[d], N);
    const int want = rdmi_snip_count(last[d], ss[d]);
    RDMI_REQUIRE(n[d] == want, RDMI_E_ARG,
                 "%s: dilation %d: %d snippets, but start step %d over %d frames (length %d, frame stride %d) gives %d",
                 what, d, n[d], ss[d], N, w[d], stride[d], want);
  }
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The argument and layout checks every moments / median call makes before any launch, and the job they fill
// (outputs are the caller's to set).
int moments_fill(const char* what, int n_dil, const void* const* xf, int x_f32, const float* const* s,
                 const float* const* t, const int* n, const int* stride, const int* start_step, const int* k0,
                 const int* nloc, const int* w, int seq_len, int f0, int nf, long HW, const float* shift, MergeP& p,
                 bool* strided) {
  RDMI_REQUIRE(n_dil >= 1 && n_dil <= MAXD && xf && s && t && n && stride && start_step && w && HW > 0 &&
                   seq_len > 0 && x_f32 >= 0 && x_f32 <= 2,
               RDMI_E_ARG, "%s: bad args", what);
  RDMI_REQUIRE(f0 >= 0 && nf >= 0 && f0 <= seq_len && nf <= seq_len - f0, RDMI_E_ARG,
               "%s: frames %d+%d outside the %d of the sequence", what, f0, nf, seq_len);
  int rows = 0;
  for (int d = 0; d < n_dil; ++d) {
    const int kk = k0 ? k0[d] : 0, nl = nloc ? nloc[d] : n[d];
    RDMI_REQUIRE(kk >= 0 && nl >= 0 && kk + nl <= n[d] && w[d] >= 1 && (nl == 0 || (xf[d] && s[d] && t[d])),
                 RDMI_E_ARG, "%s: dilation %d rows %d+%d of %d, length %d", what, d, kk, nl, n[d], w[d]);
    p.x[d] = xf[d];
    p.s[d] = s[d];
    p.t[d] = t[d];
    p.n[d] = n[d];
    p.stride[d] = stride[d];
    p.k0[d] = kk;
    p.nloc[d] = nl;
    p.w[d] = w[d];
    rows += w[d];
  }
  RDMI_REQUIRE(rows <= MAXR, RDMI_E_UNSUPPORTED, "%s: snippet lengths sum to %d (at most %d)", what, rows, MAXR);
  p.nd = n_dil; p.xf32 = x_f32; p.HW = HW; p.shift = shift; p.f0 = f0;
  return moments_start_steps(what, n_dil, start_step, p.n, p.stride, p.w, seq_len, p.ss, p.last, strided);
}

int moments_launch(const char* what, int n_dil, const void* const* xf, int x_f32, const float* const* s,
                   const float* const* t, const int* n, const int* stride, const int* start_step, const int* k0,
                   const int* nloc, const int* w, int seq_len, int f0, int nf, long HW, const float* shift,
                   float* mean_out, float* std_out, double* mom_out, void* stream) {
  MomP pp{};
  MergeP& p = pp.m;
  bool strided = false;
  if (int rc = moments_fill(what, n_dil, xf, x_f32, s, t, n, stride, start_step, k0, nloc, w, seq_len, f0, nf, HW,
                            shift, p, &strided))
    return rc;
  p.out = mean_out;
  pp.std_out = std_out;
  pp.mom = mom_out;
  if (nf == 0) return 0;
  bool vec = HW % 4 == 0 && aligned16(mean_out) && aligned16(std_out) && aligned16(mom_out);
  for (int d = 0; d < n_dil; ++d) vec = vec && (p.nloc[d] == 0 || aligned16(p.x[d]));
  const long groups = vec ? HW / 4 : HW;
  long gx = (groups + 256 * MOM_ITER - 1) / (256 * MOM_ITER);
  if (gx > 1024) gx = 1024;
  const dim3 grid((unsigned)gx, nf), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define RDMI_MOM_LAUNCH(SS_, V_, F32_) hipLaunchKernelGGL((merge_moments_k<SS_, V_, F32_>), grid, blk, 0, st, pp)
#define RDMI_MOM_PICK(SS_)                           \
  do {                                               \
    if (vec && x_f32 == 1) RDMI_MOM_LAUNCH(SS_, 4, true);       \
    else if (vec) RDMI_MOM_LAUNCH(SS_, 4, false);    \
    else if (x_f32 == 1) RDMI_MOM_LAUNCH(SS_, 1, true);         \
    else RDMI_MOM_LAUNCH(SS_, 1, false);             \
  } while (0)
  if (strided)
    RDMI_MOM_PICK(true);
  else
    RDMI_MOM_PICK(false);
#undef RDMI_MOM_PICK
#undef RDMI_MOM_LAUNCH
  return rdmi::check_launch(what);
}

}  // namespace

extern "C" int rdmi_aligner_merge_moments(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                          const float* const* t, const int* n, const int* stride,
                                          const int* start_step, const int* w, int seq_len, long HW,
                                          const float* shift, float* mean_out, float* std_out, void* stream) {
  RDMI_REQUIRE(mean_out && std_out, RDMI_E_ARG, "aligner_merge_moments: null output");
  return moments_launch("aligner_merge_moments", n_dil, xf, x_f32, s, t, n, stride, start_step, nullptr, nullptr, w,
                        seq_len, 0, seq_len, HW, shift, mean_out, std_out, nullptr, stream);
}

extern "C" int rdmi_aligner_merge_partial_window_moments(int n_dil, const void* const* xf, int x_f32,
                                                         const float* const* s, const float* const* t, const int* n,
                                                         const int* stride, const int* start_step, const int* k0,
                                                         const int* nloc, const int* w, int seq_len, int f0, int nf,
                                                         long HW, const float* shift, double* mom_out, void* stream) {
  RDMI_REQUIRE(k0 && nloc && mom_out, RDMI_E_ARG, "aligner_merge_partial_window_moments: k0/nloc/mom_out required");
  return moments_launch("aligner_merge_partial_window_moments", n_dil, xf, x_f32, s, t, n, stride, start_step, k0,
                        nloc, w, seq_len, f0, nf, HW, shift, nullptr, nullptr, mom_out, stream);
}

extern "C" int rdmi_aligner_merge_finish_pieces_moments(int n_dil, const int* n, const int* stride,
                                                        const int* start_step, const int* w, int seq_len, int f0,
                                                        int nf, long HW, int npieces, const int* piece_f0,
                                                        const int* piece_nf, const double* recv, float* mean_out,
                                                        float* std_out, void* stream) {
  const char* what = "aligner_merge_finish_pieces_moments";
  RDMI_REQUIRE(n_dil >= 1 && n_dil <= MAXD && n && stride && start_step && w && HW > 0 && seq_len > 0 &&
                   npieces >= 0 && (npieces == 0 || (piece_f0 && piece_nf && recv)),
               RDMI_E_ARG, "%s: bad args", what);
  RDMI_REQUIRE(f0 >= 0 && nf >= 0 && f0 <= seq_len && nf <= seq_len - f0, RDMI_E_ARG,
               "%s: frames %d+%d outside the %d of the sequence", what, f0, nf, seq_len);
  RDMI_REQUIRE((mean_out && std_out) || nf == 0, RDMI_E_ARG, "%s: null output", what);
  MergeP p{};
  for (int d = 0; d < n_dil; ++d) {
    p.n[d] = n[d];
    p.stride[d] = stride[d];
    p.w[d] = w[d];
  }
  p.nd = n_dil; p.HW = HW;
  bool strided = false;
  if (int rc = moments_start_steps(what, n_dil, start_step, p.n, p.stride, p.w, seq_len, p.ss, p.last, &strided))
    return rc;
  for (int i = 0; i < npieces; ++i)
    RDMI_REQUIRE(piece_nf[i] >= 0 && piece_f0[i] >= f0 && piece_f0[i] + piece_nf[i] <= f0 + nf, RDMI_E_ARG,
                 "%s: piece %d frames %d+%d outside %d+%d", what, i, piece_f0[i], piece_nf[i], f0, nf);
  if (nf == 0) return 0;
  // A piece table wider than MAXPIECES is split by frame range, as rdmi_aligner_merge_finish_pieces does:
  // every frame still adds all of its pieces in source-rank order within one thread.
  auto touches = [&](int i, int a, int b) { return piece_nf[i] > 0 && piece_f0[i] < b && piece_f0[i] + piece_nf[i] > a; };
  long gx = (HW + 255) / 256;
  if (gx > 1024) gx = 1024;
  int fs = f0;
  while (fs < f0 + nf) {
    int fe = fs + 1, cnt = 0;
    for (int i = 0; i < npieces; ++i) cnt += touches(i, fs, fe);
    RDMI_REQUIRE(cnt <= MAXPIECES, RDMI_E_UNSUPPORTED, "%s: frame %d is covered by %d pieces (at most %d)", what, fs,
                 cnt, MAXPIECES);
    while (fe < f0 + nf) {
      int c2 = 0;
      for (int i = 0; i < npieces; ++i) c2 += touches(i, fs, fe + 1);
      if (c2 > MAXPIECES) break;
      ++fe;
    }
    PiecesP q{};
    long off = 0;
    for (int i = 0; i < npieces; ++i) {
      if (touches(i, fs, fe)) {
        q.pf0[q.np] = piece_f0[i];
        q.pnf[q.np] = piece_nf[i];
        q.poff[q.np] = off;
        ++q.np;
      }
      off += (long)piece_nf[i] * 2 * HW;
    }
    p.f0 = fs;
    p.out = mean_out + (long)(fs - f0) * HW;
    float* sd = std_out + (long)(fs - f0) * HW;
    if (strided)
      hipLaunchKernelGGL(merge_finish_moments_k<true>, dim3((unsigned)gx, fe - fs), dim3(256), 0, (hipStream_t)stream,
                         p, q, recv, sd);
    else
      hipLaunchKernelGGL(merge_finish_moments_k<false>, dim3((unsigned)gx, fe - fs), dim3(256), 0, (hipStream_t)stream,
                         p, q, recv, sd);
    if (int rc = rdmi::check_launch(what)) return rc;
    fs = fe;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Median merge (since rdmi_version 7): per pixel the median of a frame's covering terms — the f32 values
// mom_term forms, the ones merge_k averages — and optionally their median absolute deviation.
//   median: the terms sorted ascending; c odd: the middle one; c even: (float)(((double)lo + (double)hi) · 0.5)
//           of the two middle ones; c = 0: 0.
//   MAD:    d_i = fabsf(a_i − median), one f32 subtraction; the median of the d_i by the same rule (raw: no
//           1.4826 factor); 0 for c ≤ 1.
// Inputs are finite; NaN and the sign of a zero are not part of the contract.  The result depends only on the
// multiset of terms: the sharded form may hand them over in any order.
//
// c is uniform per block.  A lane holds its pixel's terms in registers, padded to the kernel's capacity CAP
// (8 / 16 / 32 / 64, picked per launch from the layout's largest cover count) with ⌊(CAP − c)/2⌋ values of −inf
// and the rest +inf, so that after a Batcher odd-even merge sort — a fixed compare-exchange network, every
// index a compile-time constant, v_min_f32 / v_max_f32 — the two middle terms sit at CAP/2 − 1 and CAP/2
// whatever c is.  The deviations are formed from the sorted array (the same multiset), the −inf pads put back,
// and the network run again.  CAP ≤ 16 takes 4 pixels per lane on the vector path of merge_moments_k, the
// larger capacities one pixel per lane.
namespace {

struct MedNet {
  int n;
  unsigned char lo[544], hi[544];
};

// Batcher's odd-even merge sort for cap = 2^k inputs as a list of compare-exchanges (19 / 63 / 191 / 543 for
// 8 / 16 / 32 / 64)
constexpr MedNet med_net(int cap) {
  MedNet r{};
  for (int p = 1; p < cap; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j <= cap - 1 - k; j += 2 * k)
        for (int i = 0; i < k && i + j + k < cap; ++i)
          if ((i + j) / (p * 2) == (i + j + k) / (p * 2)) {
            r.lo[r.n] = (unsigned char)(i + j);
            r.hi[r.n] = (unsigned char)(i + j + k);
            ++r.n;
          }
  return r;
}

// the 0-1 principle: a network that sorts every 0/1 input sorts every input
constexpr bool med_net_sorts01(int cap) {
  const MedNet net = med_net(cap);
  for (unsigned m = 0; m < (1u << cap); ++m) {
    unsigned v = m;
    for (int i = 0; i < net.n; ++i) {
      const unsigned a = (v >> net.lo[i]) & 1u, b = (v >> net.hi[i]) & 1u;
      if (a > b) v ^= (1u << net.lo[i]) | (1u << net.hi[i]);
    }
    for (int i = 0; i + 1 < cap; ++i)
      if (((v >> i) & 1u) > ((v >> (i + 1)) & 1u)) return false;
  }
  return true;
}

template <int CAP>
struct MedNetOf {
  static constexpr MedNet net = med_net(CAP);
};
static_assert(MedNetOf<8>::net.n == 19 && MedNetOf<16>::net.n == 63 && MedNetOf<32>::net.n == 191 &&
                  MedNetOf<64>::net.n == 543,
              "Batcher's odd-even merge sort");
static_assert(med_net_sorts01(8), "the 8-input network sorts");

template <int CAP, int V, int K>
__device__ __forceinline__ void med_cmpex(float (&a)[CAP][V]) {
  constexpr int lo = MedNetOf<CAP>::net.lo[K], hi = MedNetOf<CAP>::net.hi[K];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float x = a[lo][v], y = a[hi][v];
    a[lo][v] = __builtin_fminf(x, y);
    a[hi][v] = __builtin_fmaxf(x, y);
  }
}

template <int CAP, int V, int K0, int... K>
__device__ __forceinline__ void med_sort_part(float (&a)[CAP][V], std::integer_sequence<int, K...>) {
  (med_cmpex<CAP, V, K0 + K>(a), ...);
}

// a[0 .. CAP) ascending, per pixel column; the list is applied 64 compare-exchanges at a time
template <int CAP, int V, int K0 = 0>
__device__ __forceinline__ void med_sort(float (&a)[CAP][V]) {
  constexpr int n = MedNetOf<CAP>::net.n, m = n - K0 < 64 ? n - K0 : 64;
  med_sort_part<CAP, V, K0>(a, std::make_integer_sequence<int, m>{});
  if constexpr (K0 + m < n) med_sort<CAP, V, K0 + m>(a);
}

// the median of c values sorted into a padded array: the two middle terms are at CAP/2 − 1 and CAP/2
template <int CAP, int V>
__device__ __forceinline__ void med_middle(const float (&a)[CAP][V], int c, float (&m)[V]) {
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float lo = a[CAP / 2 - 1][v], hi = a[CAP / 2][v];
    m[v] = c == 0 ? 0.f : ((c & 1) ? lo : (float)(((double)lo + (double)hi) * 0.5));
  }
}

template <int V>
__device__ __forceinline__ void med_store(float* o, const float (&m)[V]) {
  if constexpr (V == 4)
    *(f32x4*)o = f32x4{m[0], m[1], m[2], m[3]};
  else
    o[0] = m[0];
}

// A table entry is the same in every lane: through readfirstlane it lives in scalar registers, not in CAP × 4
// vector registers for the whole pixel loop.
__device__ __forceinline__ const char* med_uniform(const char* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const char*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float med_uniform(float x) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x)));
}

// One frame's pixels: tab[0 .. c) are its terms' rows (RAW: the rows hold the terms themselves, f32),
// c ≤ CAP; med / mad: the frame's output rows (mad may be null).
template <int CAP, int V, bool XF32, bool RAW>
__device__ __forceinline__ void median_pixels(const MomEnt* tab, int c, float sh, bool chain, long HW, float* med,
                                              float* mad) {
  const int nlo = (CAP - c) >> 1;
  const float ninf = -__builtin_inff(), pinf = __builtin_inff();
  const long groups = HW / V;  // V == 4 only when HW % 4 == 0
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long px = g * V;
    float a[CAP][V];
#pragma unroll
    for (int u0 = 0; u0 < CAP; u0 += MOM_U) {  // MOM_U rows' loads issued before the first is used
#pragma unroll
      for (int u = u0; u < u0 + MOM_U; ++u)
        if (u < c) mom_load<V, XF32>(med_uniform(tab[u].row), px, a[u]);
#pragma unroll
      for (int u = u0; u < u0 + MOM_U; ++u) {
        if (u < c) {
          if constexpr (!RAW) {
            const float s = med_uniform(tab[u].s), t = med_uniform(tab[u].t);
#pragma unroll
            for (int v = 0; v < V; ++v) a[u][v] = mom_term(a[u][v], sh, s, t, chain);
          }
        } else {
          const float pad = u - c < nlo ? ninf : pinf;
#pragma unroll
          for (int v = 0; v < V; ++v) a[u][v] = pad;
        }
      }
    }
    med_sort<CAP, V>(a);
    float m[V];
    med_middle<CAP, V>(a, c, m);
    med_store<V>(med + px, m);
    if (mad) {
#pragma unroll
      for (int u = 0; u < CAP; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float d = __builtin_fabsf(a[u][v] - m[v]);  // +inf for the pads
          a[u][v] = u < nlo ? ninf : d;                     // the sorted array starts with the −inf pads
        }
      med_sort<CAP, V>(a);
      med_middle<CAP, V>(a, c, m);
      med_store<V>(mad + px, m);
    }
  }
}

struct MedP {
  MergeP m;     // out = the median (fused form)
  float* mad;   // fused form; NULL: none
  int strided;  // a start step > 1: the index map of aligner_index.h
};

template <int CAP, int V, bool XF32>
__global__ __launch_bounds__(256) void merge_median_k(MedP pp) {
  __shared__ MomEnt tab[MAXR];
  __shared__ int cnt_sh;
  const MergeP& p = pp.m;
  const int fl = blockIdx.y, f = p.f0 + fl;
  int c = pp.strided ? moments_table<true>(p, f, tab, &cnt_sh) : moments_table<false>(p, f, tab, &cnt_sh);
  if (c > CAP) c = CAP;  // the host picked CAP ≥ the layout's largest cover count
  median_pixels<CAP, V, XF32, false>(tab, c, p.shift ? p.shift[0] : 0.f, p.xf32 == 0, p.HW, p.out + (long)fl * p.HW,
                                     pp.mad ? pp.mad + (long)fl * p.HW : nullptr);
}

// Sharded form, first half: the terms of this rank's snippets, unreduced.  Frame f0 + i's go to rows
// row_off[i] … of terms_out in the merge's order; never more than row_off[i + 1] − row_off[i] of them and
// never past `rows`.
template <int V, bool XF32>
__global__ __launch_bounds__(256) void merge_terms_k(MedP pp, const int* __restrict__ row_off, long rows,
                                                     float* __restrict__ terms_out) {
  __shared__ MomEnt tab[MAXR];
  __shared__ int cnt_sh;
  const MergeP& p = pp.m;
  const int fl = blockIdx.y, f = p.f0 + fl;
  int c = pp.strided ? moments_table<true>(p, f, tab, &cnt_sh) : moments_table<false>(p, f, tab, &cnt_sh);
  const long r0 = row_off[fl], room = (long)row_off[fl + 1] - r0;
  if (r0 < 0 || room <= 0 || r0 >= rows) return;
  if (c > room) c = (int)room;
  if (c > rows - r0) c = (int)(rows - r0);
  c = __builtin_amdgcn_readfirstlane(c);
  const float sh = p.shift ? p.shift[0] : 0.f;
  const bool chain = p.xf32 == 0;
  const long groups = p.HW / V;
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long px = g * V;
    for (int e0 = 0; e0 < c; e0 += MOM_U) {
      float x[MOM_U][V];
#pragma unroll
      for (int u = 0; u < MOM_U; ++u)
        if (e0 + u < c) mom_load<V, XF32>(tab[e0 + u].row, px, x[u]);
#pragma unroll
      for (int u = 0; u < MOM_U; ++u)
        if (e0 + u < c) {
          const float s = tab[e0 + u].s, t = tab[e0 + u].t;
          float a[V];
#pragma unroll
          for (int v = 0; v < V; ++v) a[v] = mom_term(x[u][v], sh, s, t, chain);
          med_store<V>(terms_out + (r0 + e0 + u) * p.HW + px, a);
        }
    }
  }
}

// Sharded form, second half: frame i selects over rows row_idx[frame_off[i] … frame_off[i + 1]) of `rows`
// ([n_rows][HW] f32), at most max_count ≤ CAP of them; indices outside [0, n_rows) are skipped.
template <int CAP, int V>
__global__ __launch_bounds__(256) void median_rows_k(const float* __restrict__ rows, long n_rows,
                                                     const int* __restrict__ frame_off,
                                                     const int* __restrict__ row_idx, long HW, int max_count,
                                                     float* med, float* mad) {
  __shared__ MomEnt tab[MAXR];
  __shared__ int cnt_sh;
  const int fl = blockIdx.y;
  if (threadIdx.x < 64) {
    const int i = threadIdx.x;
    const int b = frame_off[fl];
    int n = frame_off[fl + 1] - b;
    if (n > max_count) n = max_count;
    if (b < 0) n = 0;
    bool ok = false;
    MomEnt e{nullptr, 1.f, 0.f};
    if (i < n) {
      const long r = row_idx[b + i];
      if (r >= 0 && r < n_rows) {
        ok = true;
        e.row = (const char*)(rows + r * HW);
      }
    }
    const unsigned long long mask = __ballot(ok);
    if (ok) tab[__popcll(mask & ((1ull << i) - 1ull))] = e;
    if (i == 0) cnt_sh = __popcll(mask);
  }
  __syncthreads();
  int c = __builtin_amdgcn_readfirstlane(cnt_sh);
  if (c > CAP) c = CAP;
  median_pixels<CAP, V, true, true>(tab, c, 0.f, false, HW, med + (long)fl * HW, mad ? mad + (long)fl * HW : nullptr);
}

int median_capacity(int c) { return c <= 8 ? 8 : c <= 16 ? 16 : c <= 32 ? 32 : 64; }

dim3 median_grid(long groups, int nf) {
  long gx = (groups + 256 * MOM_ITER - 1) / (256 * MOM_ITER);
  if (gx > 1024) gx = 1024;
  return dim3((unsigned)gx, nf);
}

}  // namespace

extern "C" int rdmi_aligner_merge_median(int n_dil, const void* const* xf, int x_f32, const float* const* s,
                                         const float* const* t, const int* n, const int* stride,
                                         const int* start_step, const int* w, int seq_len, long HW,
                                         const float* shift, float* med_out, float* mad_out, void* stream) {
  const char* what = "aligner_merge_median";
  RDMI_REQUIRE(med_out, RDMI_E_ARG, "%s: null output", what);
  MedP pp{};
  MergeP& p = pp.m;
  bool strided = false;
  if (int rc = moments_fill(what, n_dil, xf, x_f32, s, t, n, stride, start_step, nullptr, nullptr, w, seq_len, 0,
                            seq_len, HW, shift, p, &strided))
    return rc;
  p.out = med_out;
  pp.mad = mad_out;
  pp.strided = strided;
  int cmax = 0;
  for (int f = 0; f < seq_len; ++f) {
    const int c = rdmi_cover_count(p.nd, p.n, p.stride, p.w, p.ss, p.last, f);
    if (c > cmax) cmax = c;
  }
  const int cap = median_capacity(cmax);
  bool vec = cap <= 16 && HW % 4 == 0 && aligned16(med_out) && aligned16(mad_out);
  for (int d = 0; d < n_dil; ++d) vec = vec && (p.nloc[d] == 0 || aligned16(p.x[d]));
  const dim3 grid = median_grid(vec ? HW / 4 : HW, seq_len), blk(256);
  hipStream_t st = (hipStream_t)stream;
  const bool f32 = x_f32 == 1;
#define RDMI_MED_LAUNCH(CAP_, V_, F32_) hipLaunchKernelGGL((merge_median_k<CAP_, V_, F32_>), grid, blk, 0, st, pp)
#define RDMI_MED_PICK(CAP_, V_)               \
  do {                                        \
    if (f32) RDMI_MED_LAUNCH(CAP_, V_, true); \
    else RDMI_MED_LAUNCH(CAP_, V_, false);    \
  } while (0)
  if (cap == 8 && vec) RDMI_MED_PICK(8, 4);
  else if (cap == 8) RDMI_MED_PICK(8, 1);
  else if (cap == 16 && vec) RDMI_MED_PICK(16, 4);
  else if (cap == 16) RDMI_MED_PICK(16, 1);
  else if (cap == 32) RDMI_MED_PICK(32, 1);
  else RDMI_MED_PICK(64, 1);
#undef RDMI_MED_PICK
#undef RDMI_MED_LAUNCH
  return rdmi::check_launch(what);
}

extern "C" int rdmi_aligner_merge_partial_window_terms(int n_dil, const void* const* xf, int x_f32,
                                                       const float* const* s, const float* const* t, const int* n,
                                                       const int* stride, const int* start_step, const int* k0,
                                                       const int* nloc, const int* w, int seq_len, int f0, int nf,
                                                       long HW, const float* shift, const int* row_off, long rows,
                                                       float* terms_out, void* stream) {
  const char* what = "aligner_merge_partial_window_terms";
  RDMI_REQUIRE(k0 && nloc, RDMI_E_ARG, "%s: k0/nloc required", what);
  MedP pp{};
  MergeP& p = pp.m;
  bool strided = false;
  if (int rc = moments_fill(what, n_dil, xf, x_f32, s, t, n, stride, start_step, k0, nloc, w, seq_len, f0, nf, HW,
                            shift, p, &strided))
    return rc;
  pp.strided = strided;
  long want = 0;  // the rows this window holds, from the index map
  for (int f = f0; f < f0 + nf; ++f)
    for (int d = 0; d < n_dil; ++d)
      for (int j = 0; j < p.w[d]; ++j) {
        const int k = rdmi_snip_at(f - j * p.stride[d], p.ss[d], p.last[d], p.n[d]);
        want += k >= p.k0[d] && k < p.k0[d] + p.nloc[d] ? 1 : 0;
      }
  RDMI_REQUIRE(rows == want, RDMI_E_ARG, "%s: %ld rows, but the frames %d+%d hold %ld terms of the snippets given",
               what, rows, f0, nf, want);
  if (nf == 0 || rows == 0) return 0;
  RDMI_REQUIRE(row_off && terms_out, RDMI_E_ARG, "%s: null row_off / terms_out", what);
  bool vec = HW % 4 == 0 && aligned16(terms_out);
  for (int d = 0; d < n_dil; ++d) vec = vec && (p.nloc[d] == 0 || aligned16(p.x[d]));
  const dim3 grid = median_grid(vec ? HW / 4 : HW, nf), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define RDMI_TERMS_LAUNCH(V_, F32_) \
  hipLaunchKernelGGL((merge_terms_k<V_, F32_>), grid, blk, 0, st, pp, row_off, rows, terms_out)
  if (vec && x_f32 == 1) RDMI_TERMS_LAUNCH(4, true);
  else if (vec) RDMI_TERMS_LAUNCH(4, false);
  else if (x_f32 == 1) RDMI_TERMS_LAUNCH(1, true);
  else RDMI_TERMS_LAUNCH(1, false);
#undef RDMI_TERMS_LAUNCH
  return rdmi::check_launch(what);
}

extern "C" int rdmi_aligner_median_rows(const float* rows, long n_rows, const int* frame_off, const int* row_idx,
                                        int nf, long HW, int max_count, float* med_out, float* mad_out,
                                        void* stream) {
  const char* what = "aligner_median_rows";
  RDMI_REQUIRE(nf >= 0 && HW > 0 && n_rows >= 0, RDMI_E_ARG, "%s: nf %d, HW %ld, n_rows %ld", what, nf, HW, n_rows);
  RDMI_REQUIRE(max_count >= 1 && max_count <= MAXR, RDMI_E_ARG, "%s: max_count %d (1 … %d expected)", what, max_count,
               MAXR);
  if (nf == 0) return 0;
  RDMI_REQUIRE(frame_off && med_out && (n_rows == 0 || (rows && row_idx)), RDMI_E_ARG, "%s: null argument", what);
  const int cap = median_capacity(max_count);
  const bool vec = cap <= 16 && HW % 4 == 0 && aligned16(rows) && aligned16(med_out) && aligned16(mad_out);
  const dim3 grid = median_grid(vec ? HW / 4 : HW, nf), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define RDMI_ROWS_LAUNCH(CAP_, V_)                                                                               \
  hipLaunchKernelGGL((median_rows_k<CAP_, V_>), grid, blk, 0, st, rows, n_rows, frame_off, row_idx, HW, max_count, \
                     med_out, mad_out)
  if (cap == 8 && vec) RDMI_ROWS_LAUNCH(8, 4);
  else if (cap == 8) RDMI_ROWS_LAUNCH(8, 1);
  else if (cap == 16 && vec) RDMI_ROWS_LAUNCH(16, 4);
  else if (cap == 16) RDMI_ROWS_LAUNCH(16, 1);
  else if (cap == 32) RDMI_ROWS_LAUNCH(32, 1);
  else RDMI_ROWS_LAUNCH(64, 1);
#undef RDMI_ROWS_LAUNCH
  return rdmi::check_launch(what);
}
