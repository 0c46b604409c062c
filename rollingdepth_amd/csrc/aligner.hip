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
// The merge of the aligned snippets (merge_scaled_triplets, :231-262) and its variants are in merge.hip.
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
#pragma clang fp contract(off)
#include "aligner_job.h"
#include "aligner_ws.h"

namespace {

using rdmi::MAXD;
using rdmi::MAXR;
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
  if (int rc = rdmi::start_steps("aligner_optimize", rdmi::Checks::Lenient, p.nd, a->start_step, p.n, p.stride, p.w,
                                 p.N, p.ss, p.last, &strided))
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
      rdmi::with_ss(strided, [&](auto ss) {
        constexpr bool SS = decltype(ss)::value;
        hipLaunchKernelGGL(frame_stats_hist<SS>, dim3(p.N, PS), dim3(256), 0, st, p, hmms);
        hipLaunchKernelGGL(snippet_grad_adam<SS>, dim3(ntot, PS), dim3(256), 0, st, p, it, slot, denom, cnt, hl, hst);
      });
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
    rdmi::with_ss(strided, [&](auto ss) {
      constexpr bool SS = decltype(ss)::value;
      hipLaunchKernelGGL(frame_stats<SS>, dim3(p.N, PS), dim3(256), 0, st, p);
      hipLaunchKernelGGL(snippet_grad<SS>, dim3(ntot, PS), dim3(256), 0, st, p);
    });
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
