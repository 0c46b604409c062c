// Stand-alone check of rollingdepth_amd/csrc/merge_pieces.h: the loop that cuts the frame window of a sharded
// merge's finish into launches whose piece tables hold at most MAXPIECES entries.  Every case runs with 1 and
// with 2 doubles per pixel.  Built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_merge_pieces_cpu.py.
#include <cstdio>
#include <vector>

#include "merge_pieces.h"

static long fails = 0, cases = 0;

#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (fails < 20) {                     \
        std::printf("FAIL " __VA_ARGS__);   \
        std::printf("  [%s]\n", #cond);     \
      }                                     \
      ++fails;                              \
    }                                       \
  } while (0)

struct Pieces {
  std::vector<int> f0, nf;
  void add(int first, int count) {
    f0.push_back(first);
    nf.push_back(count);
  }
  int n() const { return (int)f0.size(); }
};

static bool touches(const Pieces& p, int i, int a, int b) {
  return p.nf[i] > 0 && p.f0[i] < b && p.f0[i] + p.nf[i] > a;
}
static int touching(const Pieces& p, int a, int b) {
  int c = 0;
  for (int i = 0; i < p.n(); ++i) c += touches(p, i, a, b);
  return c;
}

// Runs the splitter over the window and checks what holds for every accepted job: the ranges partition
// [f0, f0 + nf), each is as long as its table allows, and its table lists exactly the pieces with a frame in it,
// in their original order, none of length 0, each at the offset of ALL earlier pieces.  Returns the ranges.
static std::vector<PieceRange> run(const char* name, int f0, int nf, const Pieces& p, int dpp, long HW) {
  ++cases;
  std::vector<PieceRange> out;
  PieceRange r{};
  r.fe = f0;
  int st, prev = f0;
  while ((st = next_piece_range(r, f0, nf, p.n(), p.f0.data(), p.nf.data(), dpp, HW)) > 0) {
    CHECK(r.fs == prev && r.fe > r.fs && r.fe <= f0 + nf, "%s dpp %d: range %d..%d after %d\n", name, dpp, r.fs, r.fe,
          prev);
    if (r.fe <= prev) return out;  // no progress: do not loop
    prev = r.fe;
    CHECK(r.q.np >= 0 && r.q.np <= MAXPIECES, "%s dpp %d: %d entries\n", name, dpp, r.q.np);
    CHECK(r.fe == f0 + nf || touching(p, r.fs, r.fe + 1) > MAXPIECES, "%s dpp %d: range %d..%d stops early\n", name,
          dpp, r.fs, r.fe);
    int e = 0;
    long off = 0;
    for (int i = 0; i < p.n(); ++i) {
      if (touches(p, i, r.fs, r.fe)) {
        CHECK(e < r.q.np && e < MAXPIECES && r.q.pf0[e] == p.f0[i] && r.q.pnf[e] == p.nf[i] && r.q.poff[e] == off,
              "%s dpp %d: range %d..%d entry %d is not piece %d at %ld\n", name, dpp, r.fs, r.fe, e, i, off);
        CHECK(p.nf[i] > 0, "%s dpp %d: zero-length piece %d listed\n", name, dpp, i);
        ++e;
      }
      off += (long)p.nf[i] * dpp * HW;
    }
    CHECK(e == r.q.np, "%s dpp %d: range %d..%d lists %d pieces, %d touch it\n", name, dpp, r.fs, r.fe, r.q.np, e);
    out.push_back(r);
  }
  CHECK(st == 0, "%s dpp %d: refused at frame %d (%d pieces)\n", name, dpp, r.fs, r.count);
  CHECK(prev == f0 + nf, "%s dpp %d: ranges end at %d of %d\n", name, dpp, prev, f0 + nf);
  return out;
}

int main() {
  for (int dpp = 1; dpp <= 2; ++dpp) {
    {  // 70 one-frame pieces over 70 frames (HW = 2^28: the offsets pass 2^31).  A table holds 64, so the first
       // range takes the first 64 frames and a second the other 6; every offset is i · dpp · HW.
      const long HW = 1L << 28;
      Pieces p;
      for (int i = 0; i < 70; ++i) p.add(5 + i, 1);
      const auto rs = run("one per frame", 5, 70, p, dpp, HW);
      CHECK(rs.size() == 2 && rs[0].fs == 5 && rs[0].fe == 69 && rs[0].q.np == 64 && rs[1].fe == 75 && rs[1].q.np == 6,
            "one per frame dpp %d: %zu ranges\n", dpp, rs.size());
      int i = 0;
      for (const auto& r : rs)
        for (int e = 0; e < r.q.np; ++e, ++i)
          CHECK(r.q.pf0[e] == 5 + i && r.q.poff[e] == (long)i * dpp * HW, "one per frame dpp %d: piece %d\n", dpp, i);
      CHECK(i == 70, "one per frame dpp %d: %d pieces listed\n", dpp, i);
    }
    {  // 70 pieces that each span all of a 4-frame window: refused, naming frame f0 and count 70
      ++cases;
      Pieces p;
      for (int i = 0; i < 70; ++i) p.add(9, 4);
      PieceRange r{};
      r.fe = 9;
      const int st = next_piece_range(r, 9, 4, p.n(), p.f0.data(), p.nf.data(), dpp, 7);
      CHECK(st == -1 && r.fs == 9 && r.count == 70, "all span dpp %d: %d, frame %d, count %d\n", dpp, st, r.fs,
            r.count);
    }
    {  // the per-frame count reaches 64 and never exceeds it: 3 pieces span the 40-frame window, 61 one-frame
       // pieces sit on frame 10, one more on each later frame; the long and the short ones interleaved
      const int f0 = 2;
      Pieces p;
      p.add(f0, 40);
      for (int i = 0; i < 30; ++i) p.add(f0 + 10, 1);
      p.add(f0, 40);
      for (int f = 39; f >= 11; --f) p.add(f0 + f, 1);
      for (int i = 0; i < 31; ++i) p.add(f0 + 10, 1);
      p.add(f0, 40);
      int most = 0;
      for (int f = f0; f < f0 + 40; ++f) most = touching(p, f, f + 1) > most ? touching(p, f, f + 1) : most;
      CHECK(most == 64, "reaches 64: the job's largest count is %d\n", most);
      const auto rs = run("reaches 64", f0, 40, p, dpp, 9);
      CHECK(rs.size() == 2 && rs[0].fe == f0 + 11 && rs[0].q.np == 64 && rs[1].q.np == 32,
            "reaches 64 dpp %d: %zu ranges\n", dpp, rs.size());
    }
    {  // zero-length pieces: never listed, and they advance the offset by 0
      Pieces p;
      p.add(3, 0);
      p.add(3, 2);
      p.add(4, 0);
      p.add(5, 3);
      p.add(8, 0);  // at the window's end
      p.add(3, 5);
      const auto rs = run("zero-length", 3, 5, p, dpp, 11);
      CHECK(rs.size() == 1 && rs[0].q.np == 3 && rs[0].q.poff[0] == 0 && rs[0].q.poff[1] == 2L * dpp * 11 &&
                rs[0].q.poff[2] == 5L * dpp * 11,
            "zero-length dpp %d\n", dpp);
      Pieces z;  // only zero-length pieces, 70 of them on one frame: an empty table, not a refusal
      for (int i = 0; i < 70; ++i) z.add(4, 0);
      const auto zs = run("only zero-length", 3, 5, z, dpp, 11);
      CHECK(zs.size() == 1 && zs[0].q.np == 0, "only zero-length dpp %d\n", dpp);
    }
    {  // nf = 0: no range, whatever the pieces; npieces = 0: one range over the window with an empty table
      Pieces p;
      p.add(6, 0);
      CHECK(run("nf 0", 6, 0, p, dpp, 5).empty(), "nf 0 dpp %d\n", dpp);
      CHECK(run("nf 0, no pieces", 6, 0, Pieces{}, dpp, 5).empty(), "nf 0, no pieces dpp %d\n", dpp);
      ++cases;
      PieceRange r{};
      r.fe = 6;
      const int st = next_piece_range(r, 6, 12, 0, nullptr, nullptr, dpp, 5);
      CHECK(st == 1 && r.fs == 6 && r.fe == 18 && r.q.np == 0, "no pieces dpp %d: %d, %d..%d\n", dpp, st, r.fs, r.fe);
      CHECK(next_piece_range(r, 6, 12, 0, nullptr, nullptr, dpp, 5) == 0, "no pieces dpp %d: a second range\n", dpp);
    }
  }
  std::printf("%ld cases, %ld failures\n", cases, fails);
  return fails ? 1 : 0;
}
