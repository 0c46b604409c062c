// The piece table of the sharded merge's second half (merge.hip, merge_finish_pieces_k / merge_finish_moments_k)
// and the host loop that cuts a frame window into launches whose tables fit.  Plain C++, no HIP, no error
// reporting of its own: tests/cpp/merge_pieces_check.cpp builds it stand-alone.
//
// The pieces lie back to back in the receive buffer, piece i holding dpp · HW doubles for each of its
// piece_nf[i] frames (dpp = 1: the sums; 2: Σa then Σa²).  The table travels in the kernel arguments (≤ MAXPIECES
// entries).  More pieces than that (one per source rank and dilation: 3·W > 64 from W = 22 ranks on) are split
// by frame: each launch takes a frame range and only the pieces that touch it, in their original (source-rank)
// order — every frame still adds all of its pieces in that order within one thread, so the sums are those of a
// single launch.  Only a single frame touched by more than MAXPIECES pieces is refused.
#pragma once

namespace {  // internal to each file that includes it, as the kernels that take a PiecesP are

constexpr int MAXPIECES = 64;

struct PiecesP {
  int pf0[MAXPIECES], pnf[MAXPIECES];  // first frame and frame count of a piece
  long poff[MAXPIECES];                // its offset in the receive buffer, in doubles
  int np;
};

struct PieceRange {
  int fs, fe;  // frames fs .. fe-1 (start with fe = the window's first frame f0)
  PiecesP q;   // the pieces that touch them
  int count;   // when refused: the number of pieces touching frame fs
};

// The next range of the window f0 .. f0+nf-1, from frame r.fe on, grown while its pieces fit one table.
// 1: r holds it; 0: the window is exhausted; -1: frame r.fs alone is touched by r.count > MAXPIECES pieces.
// Zero-length pieces are never listed; a listed piece's offset counts every earlier piece, listed or not.
inline int next_piece_range(PieceRange& r, int f0, int nf, int npieces, const int* piece_f0, const int* piece_nf,
                            int dpp, long HW) {
  auto touches = [&](int i, int a, int b) {  // piece i has a frame in [a, b)
    return piece_nf[i] > 0 && piece_f0[i] < b && piece_f0[i] + piece_nf[i] > a;
  };
  auto touching = [&](int a, int b) {
    int c = 0;
    for (int i = 0; i < npieces; ++i) c += touches(i, a, b);
    return c;
  };
  const int end = f0 + nf;
  r.fs = r.fe;
  if (r.fs >= end) return 0;
  r.count = touching(r.fs, r.fs + 1);
  if (r.count > MAXPIECES) return -1;
  r.fe = r.fs + 1;
  while (r.fe < end && touching(r.fs, r.fe + 1) <= MAXPIECES) ++r.fe;
  r.q = PiecesP{};
  long off = 0;
  for (int i = 0; i < npieces; ++i) {
    if (touches(i, r.fs, r.fe)) {
      r.q.pf0[r.q.np] = piece_f0[i];
      r.q.pnf[r.q.np] = piece_nf[i];
      r.q.poff[r.q.np] = off;
      ++r.q.np;
    }
    off += (long)piece_nf[i] * dpp * HW;
  }
  return 1;
}

}  // namespace
