// The merge of the snippets the optimiser (aligner.hip) has co-aligned:
// merge         — merge_scaled_triplets (rollingdepth/depth_aligner.py:231-262): per frame the mean over all
//                 covering slots of s·x+t, rounded through the snippet dtype where the reference computes in it.
// merge_moments — the same mean plus the per-pixel standard deviation of those slots' terms, in one pass.
// merge_median  — the per-pixel median of those slots' terms in place of their mean, optionally with their
//                 median absolute deviation.
// The sharded merge takes start steps (aligner.hip) through its _strided entry points (window sums:
// merge_k<true>; cover count: rdmi_cover_count); the entry points of the other two always take them.
#pragma clang fp contract(off)
#include <utility>

#include "aligner_job.h"
#include "merge_pieces.h"

namespace {

using rdmi::Checks;
using rdmi::MAXD;
using rdmi::MAXR;
using rdmi::with_ss;

// as in aligner.hip (where the one rounding of a mulrn that feeds an addrn is explained)
__device__ __forceinline__ float mulrn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float addrn(float a, float b) { return __fadd_rn(a, b); }

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
// no piece covers are 0 (no slot covers them: cover count 0).  PiecesP: merge_pieces.h.
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

// Host side.  The grid for nf frames of `items` pixels (or pixel groups), `per` of them to a thread of a block:
dim3 merge_grid(long items, int per, int nf) {
  const long gx = (items + 256 * per - 1) / (256 * per);
  return dim3((unsigned)(gx > 1024 ? 1024 : gx), nf);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_window(const char* what, int f0, int nf, int seq_len) {
  RDMI_REQUIRE(f0 >= 0 && nf >= 0 && f0 <= seq_len && nf <= seq_len - f0, RDMI_E_ARG,
               "%s: frames %d+%d outside the %d of the sequence", what, f0, nf, seq_len);
  return 0;
}

// The layout of a job: all a finish call states of it (it takes no snippets).
void fill_layout(int n_dil, const int* n, const int* stride, const int* w, MergeP& p) {
  for (int d = 0; d < n_dil; ++d) p.n[d] = n[d], p.stride[d] = stride[d], p.w[d] = w[d];
  p.nd = n_dil;
}

// The per-dilation arguments of a call that takes snippets, checked, → the job (k0 / nloc NULL: whole snippets;
// the caller has checked n_dil).  Checks::Strict (aligner_job.h): also Σ w_d ≤ MAXR, the table of moments_table.
int fill_job(const char* what, Checks checks, int n_dil, const void* const* xf, const float* const* s,
             const float* const* t, const int* n, const int* stride, const int* k0, const int* nloc, const int* w,
             MergeP& p) {
  int rows = 0;
  for (int d = 0; d < n_dil; ++d) {
    const int kk = k0 ? k0[d] : 0, nl = nloc ? nloc[d] : n[d];
    RDMI_REQUIRE(kk >= 0 && nl >= 0 && kk + nl <= n[d] && w[d] >= 1 && (nl == 0 || (xf[d] && s[d] && t[d])),
                 RDMI_E_ARG, "%s: dilation %d rows %d+%d of %d, length %d", what, d, kk, nl, n[d], w[d]);
    p.x[d] = xf[d]; p.s[d] = s[d]; p.t[d] = t[d];
    p.k0[d] = kk; p.nloc[d] = nl;
    rows += w[d];
  }
  RDMI_REQUIRE(checks == Checks::Lenient || rows <= MAXR, RDMI_E_UNSUPPORTED,
               "%s: snippet lengths sum to %d (at most %d)", what, rows, MAXR);
  fill_layout(n_dil, n, stride, w, p);
  return 0;
}

// The checks every Checks::Strict entry point that takes snippets makes before any launch, and the job they
// fill (outputs are the caller's to set).
int strict_job(const char* what, int n_dil, const void* const* xf, int x_f32, const float* const* s,
               const float* const* t, const int* n, const int* stride, const int* start_step, const int* k0,
               const int* nloc, const int* w, int seq_len, int f0, int nf, long HW, const float* shift, MergeP& p,
               bool* strided) {
  RDMI_REQUIRE(n_dil >= 1 && n_dil <= MAXD && xf && s && t && n && stride && start_step && w && HW > 0 &&
                   seq_len > 0 && x_f32 >= 0 && x_f32 <= 2,
               RDMI_E_ARG, "%s: bad args", what);
  if (int rc = check_window(what, f0, nf, seq_len)) return rc;
  if (int rc = fill_job(what, Checks::Strict, n_dil, xf, s, t, n, stride, k0, nloc, w, p)) return rc;
  p.xf32 = x_f32; p.HW = HW; p.shift = shift; p.f0 = f0;
  return rdmi::start_steps(what, Checks::Strict, n_dil, start_step, p.n, p.stride, p.w, seq_len, p.ss, p.last,
                           strided);
}

int merge_launch(int n_dil, const void* const* xf, int x_f32, const float* const* s, const float* const* t,
                 const int* n, const int* stride, const int* k0, const int* nloc, const int* w, int f0, int nf, long HW,
                 const float* shift, float* out, double* dsum, void* stream, const int* start_step = nullptr,
                 int seq_len = 0) {
  RDMI_REQUIRE(n_dil >= 1 && n_dil <= MAXD && (out || dsum) && HW > 0 && nf >= 0 && f0 >= 0, RDMI_E_ARG,
               "aligner_merge: bad args");
  MergeP p{};
  if (int rc = fill_job("aligner_merge", Checks::Lenient, n_dil, xf, s, t, n, stride, k0, nloc, w, p)) return rc;
  p.xf32 = x_f32; p.HW = HW; p.shift = shift; p.out = out; p.dsum = dsum;
  p.sum_only = dsum != nullptr; p.f0 = f0;
  bool strided = false;
  if (int rc = !start_step ? 0 : rdmi::start_steps("aligner_merge_strided", Checks::Lenient, n_dil, start_step, p.n,
                                                   p.stride, p.w, seq_len, p.ss, p.last, &strided))
    return rc;
  if (nf == 0) return 0;
  with_ss(strided, [&](auto ss) {
    hipLaunchKernelGGL(merge_k<decltype(ss)::value>, merge_grid(HW, 1, nf), dim3(256), 0, (hipStream_t)stream, p);
  });
  return rdmi::check_launch("aligner_merge");
}

// The finish of a sharded merge over frames f0 .. f0+nf-1 whose pieces hold dpp doubles per pixel: the pieces
// checked against the window, then launch(range) once per piece range (merge_pieces.h).
template <class F>
int finish_ranges(const char* what, int f0, int nf, long HW, int dpp, int npieces, const int* piece_f0,
                  const int* piece_nf, F&& launch) {
  for (int i = 0; i < npieces; ++i)
    RDMI_REQUIRE(piece_nf[i] >= 0 && piece_f0[i] >= f0 && piece_f0[i] + piece_nf[i] <= f0 + nf, RDMI_E_ARG,
                 "%s: piece %d frames %d+%d outside %d+%d", what, i, piece_f0[i], piece_nf[i], f0, nf);
  PieceRange r{};
  r.fe = f0;
  while (const int more = next_piece_range(r, f0, nf, npieces, piece_f0, piece_nf, dpp, HW)) {
    RDMI_REQUIRE(more > 0, RDMI_E_UNSUPPORTED, "%s: frame %d is covered by %d pieces (at most %d)", what, r.fs,
                 r.count, MAXPIECES);
    launch(r);
    if (int rc = rdmi::check_launch(what)) return rc;
  }
  return 0;
}

int finish_pieces_launch(int n_dil, const int* n, const int* stride, const int* w, int f0, int nf, long HW,
                         int npieces, const int* piece_f0, const int* piece_nf, const double* recv, float* out,
                         void* stream, const int* start_step = nullptr, int seq_len = 0) {
  const char* what = "aligner_merge_finish_pieces";
  RDMI_REQUIRE(n_dil >= 1 && n_dil <= MAXD && n && stride && w && (out || nf == 0) && HW > 0 && f0 >= 0 && nf >= 0 &&
                   npieces >= 0 && (npieces == 0 || (piece_f0 && piece_nf && recv)),
               RDMI_E_ARG, "%s: bad args", what);
  MergeP p{};
  fill_layout(n_dil, n, stride, w, p);
  p.HW = HW;
  bool strided = false;
  if (int rc = !start_step ? 0 : rdmi::start_steps("aligner_merge_finish_pieces_strided", Checks::Lenient, n_dil,
                                                   start_step, p.n, p.stride, p.w, seq_len, p.ss, p.last, &strided))
    return rc;
  if (nf == 0) return 0;  // before the pieces are looked at
  return finish_ranges(what, f0, nf, HW, 1, npieces, piece_f0, piece_nf, [&](const PieceRange& r) {
    p.f0 = r.fs;
    p.out = out + (long)(r.fs - f0) * HW;
    with_ss(strided, [&](auto ss) {
      hipLaunchKernelGGL(merge_finish_pieces_k<decltype(ss)::value>, merge_grid(HW, 1, r.fe - r.fs), dim3(256), 0,
                         (hipStream_t)stream, p, r.q, recv);
    });
  });
}

}  // namespace

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
  if (int rc = check_window("aligner_merge_partial_window_strided", f0, nf, seq_len)) return rc;
  return merge_launch(n_dil, xf, x_f32, s, t, n, stride, k0, nloc, w, f0, nf, HW, shift, nullptr, sum_out, stream,
                      start_step, seq_len);
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
  if (int rc = check_window("aligner_merge_finish_pieces_strided", f0, nf, seq_len)) return rc;
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

int moments_launch(const char* what, int n_dil, const void* const* xf, int x_f32, const float* const* s,
                   const float* const* t, const int* n, const int* stride, const int* start_step, const int* k0,
                   const int* nloc, const int* w, int seq_len, int f0, int nf, long HW, const float* shift,
                   float* mean_out, float* std_out, double* mom_out, void* stream) {
  MomP pp{};
  MergeP& p = pp.m;
  bool strided = false;
  if (int rc = strict_job(what, n_dil, xf, x_f32, s, t, n, stride, start_step, k0, nloc, w, seq_len, f0, nf, HW,
                          shift, p, &strided))
    return rc;
  p.out = mean_out; pp.std_out = std_out; pp.mom = mom_out;
  if (nf == 0) return 0;
  bool vec = HW % 4 == 0 && aligned16(mean_out) && aligned16(std_out) && aligned16(mom_out);
  for (int d = 0; d < n_dil; ++d) vec = vec && (p.nloc[d] == 0 || aligned16(p.x[d]));
  const dim3 grid = merge_grid(vec ? HW / 4 : HW, MOM_ITER, nf), blk(256);
  hipStream_t st = (hipStream_t)stream;
  with_ss(strided, [&](auto ss) {
#define RDMI_MOM_LAUNCH(V_, F32_) \
  hipLaunchKernelGGL((merge_moments_k<decltype(ss)::value, V_, F32_>), grid, blk, 0, st, pp)
    if (vec && x_f32 == 1) RDMI_MOM_LAUNCH(4, true);
    else if (vec) RDMI_MOM_LAUNCH(4, false);
    else if (x_f32 == 1) RDMI_MOM_LAUNCH(1, true);
    else RDMI_MOM_LAUNCH(1, false);
#undef RDMI_MOM_LAUNCH
  });
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
  if (int rc = check_window(what, f0, nf, seq_len)) return rc;
  RDMI_REQUIRE((mean_out && std_out) || nf == 0, RDMI_E_ARG, "%s: null output", what);
  MergeP p{};
  fill_layout(n_dil, n, stride, w, p);
  p.HW = HW;
  bool strided = false;
  if (int rc = rdmi::start_steps(what, Checks::Strict, n_dil, start_step, p.n, p.stride, p.w, seq_len, p.ss, p.last,
                                 &strided))
    return rc;
  return finish_ranges(what, f0, nf, HW, 2, npieces, piece_f0, piece_nf, [&](const PieceRange& r) {
    p.f0 = r.fs;
    p.out = mean_out + (long)(r.fs - f0) * HW;
    with_ss(strided, [&](auto ss) {
      hipLaunchKernelGGL(merge_finish_moments_k<decltype(ss)::value>, merge_grid(HW, 1, r.fe - r.fs), dim3(256), 0,
                         (hipStream_t)stream, p, r.q, recv, std_out + (long)(r.fs - f0) * HW);
    });
  });
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

// A median kernel's <CAP, V>: launch(CAP, V) as integral constants (4 pixels per lane: CAP ≤ 16 only).
template <int I>
using Int = std::integral_constant<int, I>;
template <class F>
void with_cap(int cap, bool vec, F&& launch) {
  if (cap == 8 && vec) launch(Int<8>{}, Int<4>{});
  else if (cap == 8) launch(Int<8>{}, Int<1>{});
  else if (cap == 16 && vec) launch(Int<16>{}, Int<4>{});
  else if (cap == 16) launch(Int<16>{}, Int<1>{});
  else if (cap == 32) launch(Int<32>{}, Int<1>{});
  else launch(Int<64>{}, Int<1>{});
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
  if (int rc = strict_job(what, n_dil, xf, x_f32, s, t, n, stride, start_step, nullptr, nullptr, w, seq_len, 0,
                          seq_len, HW, shift, p, &strided))
    return rc;
  p.out = med_out; pp.mad = mad_out; pp.strided = strided;
  int cmax = 0;
  for (int f = 0; f < seq_len; ++f) {
    const int c = rdmi_cover_count(p.nd, p.n, p.stride, p.w, p.ss, p.last, f);
    if (c > cmax) cmax = c;
  }
  const int cap = median_capacity(cmax);
  bool vec = cap <= 16 && HW % 4 == 0 && aligned16(med_out) && aligned16(mad_out);
  for (int d = 0; d < n_dil; ++d) vec = vec && (p.nloc[d] == 0 || aligned16(p.x[d]));
  const dim3 grid = merge_grid(vec ? HW / 4 : HW, MOM_ITER, seq_len), blk(256);
  hipStream_t st = (hipStream_t)stream;
  with_cap(cap, vec, [&](auto c, auto v) {
    constexpr int CAP = decltype(c)::value, V = decltype(v)::value;
    if (x_f32 == 1) hipLaunchKernelGGL((merge_median_k<CAP, V, true>), grid, blk, 0, st, pp);
    else hipLaunchKernelGGL((merge_median_k<CAP, V, false>), grid, blk, 0, st, pp);
  });
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
  if (int rc = strict_job(what, n_dil, xf, x_f32, s, t, n, stride, start_step, k0, nloc, w, seq_len, f0, nf, HW,
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
  const dim3 grid = merge_grid(vec ? HW / 4 : HW, MOM_ITER, nf), blk(256);
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
  const dim3 grid = merge_grid(vec ? HW / 4 : HW, MOM_ITER, nf), blk(256);
  hipStream_t st = (hipStream_t)stream;
  with_cap(cap, vec, [&](auto c, auto v) {
    hipLaunchKernelGGL((median_rows_k<decltype(c)::value, decltype(v)::value>), grid, blk, 0, st, rows, n_rows,
                       frame_off, row_idx, HW, max_count, med_out, mad_out);
  });
  return rdmi::check_launch(what);
}
