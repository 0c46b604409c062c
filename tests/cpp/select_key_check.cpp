// Stand-alone check of rollingdepth_amd/csrc/select_key.h (the key, digits, rank rule and histogram walk that the
// radix-select kernels of select.hip and their CPU reference share).
// Built with g++ -fsanitize=address,undefined and run as a child process by tests/test_quantile_cpu.py.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "select_key.h"

static long fails = 0, cases = 0;

#define CHECK(cond, ...)                    \
  do {                                      \
    ++cases;                                \
    if (!(cond)) {                          \
      if (fails < 20) {                     \
        std::printf("FAIL " __VA_ARGS__);   \
        std::printf("  [%s]\n", #cond);     \
      }                                     \
      ++fails;                              \
    }                                       \
  } while (0)

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float dmin = std::numeric_limits<float>::denorm_min();
  // ascending edge values; −0 and +0 are adjacent and share a key
  const std::vector<float> v = {
      -inf, -FLT_MAX, std::nextafterf(-FLT_MAX, 0.f), std::nextafterf(-1.f, -2.f), -1.f, std::nextafterf(-1.f, 0.f),
      std::nextafterf(-FLT_MIN, -1.f), -FLT_MIN, std::nextafterf(-FLT_MIN, 0.f), -2 * dmin, -dmin, -0.f, 0.f, dmin,
      2 * dmin, std::nextafterf(FLT_MIN, 0.f), FLT_MIN, std::nextafterf(FLT_MIN, 1.f), std::nextafterf(1.f, 0.f), 1.f,
      std::nextafterf(1.f, 2.f), std::nextafterf(FLT_MAX, 0.f), FLT_MAX, inf};
  for (size_t i = 0; i < v.size(); ++i) {
    const uint32_t k = rdmi_select_key(v[i]);
    CHECK(!rdmi_select_is_nan(v[i]), "nan flag on %a\n", v[i]);
    const float back = rdmi_select_value(k);
    if (v[i] == 0.f)
      CHECK(rdmi_select_bits(back) == 0u, "zero %a comes back as bits %08x\n", v[i], rdmi_select_bits(back));
    else
      CHECK(rdmi_select_bits(back) == rdmi_select_bits(v[i]), "inverse %a -> %08x -> %a\n", v[i], k, back);
    uint32_t re = 0;  // the digits recompose the key, most significant first
    for (int p = 0; p < kSelectPasses; ++p) {
      const uint32_t d = rdmi_select_digit(k, p);
      CHECK(d < (uint32_t)kSelectBins, "digit %u of pass %d\n", d, p);
      CHECK((k & rdmi_select_prefix_mask(p)) == re, "prefix mask pass %d key %08x\n", p, k);
      re |= d << rdmi_select_shift(p);
    }
    CHECK(re == k, "digits of %08x recompose to %08x\n", k, re);
    if (i + 1 < v.size()) {
      const uint32_t k1 = rdmi_select_key(v[i + 1]);
      if (v[i] == 0.f && v[i + 1] == 0.f)
        CHECK(k == k1, "-0 / +0 keys %08x %08x\n", k, k1);
      else
        CHECK(v[i] < v[i + 1] && k < k1, "order %a (%08x) vs %a (%08x)\n", v[i], k, v[i + 1], k1);
    }
  }
  CHECK(rdmi_select_key(-0.f) == 0x80000000u && rdmi_select_key(0.f) == 0x80000000u, "zero key\n");
  CHECK(rdmi_select_is_nan(std::nanf("")) && rdmi_select_is_nan(-std::nanf("")), "nan flag\n");
  CHECK(rdmi_select_shift(0) == 32 - kSelectDigitBits && rdmi_select_shift(kSelectPasses - 1) == 0, "shifts\n");
  CHECK(rdmi_select_prefix_mask(0) == 0u, "pass 0 has no prefix\n");

  // the pick walk
  std::vector<uint64_t> h(kSelectBins, 0);
  int bin = -7;
  uint64_t in = 99;
  CHECK(!rdmi_select_pick_bin(h.data(), 0, &bin, &in) && bin == -7 && in == 99, "empty histogram\n");
  h[0] = 3, h[5] = 2, h[kSelectBins - 1] = 4;  // values 0..2 | 3..4 | 5..8
  CHECK(rdmi_select_pick_bin(h.data(), 0, &bin, &in) && bin == 0 && in == 0, "first bin: %d %llu\n", bin,
        (unsigned long long)in);
  CHECK(rdmi_select_pick_bin(h.data(), 2, &bin, &in) && bin == 0 && in == 2, "last of first bin: %d\n", bin);
  CHECK(rdmi_select_pick_bin(h.data(), 3, &bin, &in) && bin == 5 && in == 0, "boundary: %d %llu\n", bin,
        (unsigned long long)in);
  CHECK(rdmi_select_pick_bin(h.data(), 4, &bin, &in) && bin == 5 && in == 1, "inside bin 5: %d\n", bin);
  CHECK(rdmi_select_pick_bin(h.data(), 5, &bin, &in) && bin == kSelectBins - 1 && in == 0, "last bin start: %d\n", bin);
  CHECK(rdmi_select_pick_bin(h.data(), 8, &bin, &in) && bin == kSelectBins - 1 && in == 3, "last bin end: %d\n", bin);
  CHECK(!rdmi_select_pick_bin(h.data(), 9, &bin, &in), "rank past the total\n");
  std::vector<uint64_t> one(kSelectBins, 0);
  one[17] = 1000;  // all counts in one bin
  CHECK(rdmi_select_pick_bin(one.data(), 0, &bin, &in) && bin == 17 && in == 0, "one bin, rank 0\n");
  CHECK(rdmi_select_pick_bin(one.data(), 999, &bin, &in) && bin == 17 && in == 999, "one bin, last rank\n");
  std::vector<uint64_t> big(kSelectBins, 0);
  big[1] = (1ull << 33) + 5, big[2] = 1ull << 40, big[200] = 7;  // counts above 2^32
  CHECK(rdmi_select_pick_bin(big.data(), (1ull << 33) + 4, &bin, &in) && bin == 1 && in == (1ull << 33) + 4, "big 1\n");
  CHECK(rdmi_select_pick_bin(big.data(), (1ull << 33) + 5, &bin, &in) && bin == 2 && in == 0, "big boundary\n");
  CHECK(rdmi_select_pick_bin(big.data(), (1ull << 33) + 5 + (1ull << 40) + 6, &bin, &in) && bin == 200 && in == 6,
        "big last\n");

  // the rank rule
  const uint64_t c40 = 1ull << 40;
  CHECK(rdmi_select_rank(0.0, 1) == 0 && rdmi_select_rank(1.0, 1) == 0 && rdmi_select_rank(0.5, 1) == 0, "cnt 1\n");
  CHECK(rdmi_select_rank(0.0, c40) == 0 && rdmi_select_rank(1.0, c40) == c40 - 1, "cnt 2^40 ends\n");
  CHECK(rdmi_select_rank(0.5, c40) == (c40 - 1) / 2, "cnt 2^40 median: %llu\n",
        (unsigned long long)rdmi_select_rank(0.5, c40));
  CHECK(rdmi_select_rank(0.25, 5) == 1 && rdmi_select_rank(0.5, 5) == 2 && rdmi_select_rank(0.99, 5) == 3, "cnt 5\n");
  CHECK(rdmi_select_rank(0.02, 101) == 2 && rdmi_select_rank(0.98, 101) == 98, "percentiles of 101\n");

  // a whole select over the edge values, digit by digit, against their sorted order
  for (size_t want = 0; want < v.size(); ++want) {
    uint32_t prefix = 0;
    uint64_t r = want;
    bool ok = true;
    for (int p = 0; p < kSelectPasses && ok; ++p) {
      std::vector<uint64_t> hh(kSelectBins, 0);
      for (float x : v) {
        const uint32_t k = rdmi_select_key(x);
        if ((k & rdmi_select_prefix_mask(p)) == prefix) ++hh[rdmi_select_digit(k, p)];
      }
      int b = 0;
      ok = rdmi_select_pick_bin(hh.data(), r, &b, &r);
      prefix |= (uint32_t)b << rdmi_select_shift(p);
    }
    const float got = rdmi_select_value(prefix);
    CHECK(ok && (got == v[want]) && (v[want] != 0.f || rdmi_select_bits(got) == 0u), "select rank %zu: %a != %a\n",
          want, got, v[want]);
  }
  std::printf("%ld cases, %ld failures\n", cases, fails);
  return fails ? 1 : 0;
}
