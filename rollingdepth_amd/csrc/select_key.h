// Exact order statistics by radix select (select.hip): the key, its digits, the rank rule and the pick step.
//   key     an f32 value → a 32-bit unsigned key whose unsigned order is the value's numeric order: negatives
//           have all bits flipped, non-negatives the sign bit; −0.0 is first made +0.0 (what v + 0.0f gives), so
//           the two zeros share a key; ±inf are ordered like any value; a NaN has no key (rdmi_select_is_nan) and
//           is skipped by the counting pass like a masked-out element.  f16 inputs are widened to f32 first (exact).
//   digits  the key is consumed most significant digit first, kSelectPasses digits of kSelectDigitBits bits;
//           one counting pass builds the kSelectBins-bin histogram of one digit over the elements whose higher
//           digits equal the prefix chosen so far.
//   rank    for a fraction q in [0, 1] and cnt counted values the 0-based rank floor(q · (double)(cnt − 1)): one
//           f64 multiply, bit-identical on host and device; the result is the data value of that rank (no
//           interpolation; numpy's method="lower" whenever both rank formulas are exact).
//   pick    given one pass's histogram and the remaining rank: the bin that holds the rank and the rank inside it.
// One definition for the device code (select.hip) and the CPU check program (tests/cpp/select_key_check.cpp):
// plain integer / f64 functions, no other dependency.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RDMI_SELECT_HD __host__ __device__ inline
#else
#define RDMI_SELECT_HD inline
#endif

constexpr int kSelectDigitBits = 8;
constexpr int kSelectBins = 1 << kSelectDigitBits;   // bins of one pass's histogram
constexpr int kSelectPasses = 32 / kSelectDigitBits;  // passes over the data
constexpr int kSelectMax = 4;                         // quantiles found together (RDMI_SELECT_MAX)
static_assert(kSelectDigitBits * kSelectPasses == 32, "the digits must tile the 32-bit key");

// What the passes of one select share, in device memory: written by the pick step, read by the next counting pass.
struct rdmi_select_state {
  uint64_t cnt;               // counted values (unmasked, not NaN): the sum of pass 0's histogram
  uint64_t rank[kSelectMax];  // remaining rank of each quantile inside the bins chosen so far
  uint32_t prefix[kSelectMax];  // the digits chosen so far, in place (lower bits zero)
  uint32_t pad[2];
};

RDMI_SELECT_HD uint32_t rdmi_select_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

RDMI_SELECT_HD bool rdmi_select_is_nan(float v) { return (rdmi_select_bits(v) & 0x7fffffffu) > 0x7f800000u; }

// the key of a non-NaN value
RDMI_SELECT_HD uint32_t rdmi_select_key(float v) {
  uint32_t b = rdmi_select_bits(v);
  if ((b << 1) == 0) b = 0;  // −0.0 → +0.0: the bits of v + 0.0f, taken without a float operation
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the value of a key
RDMI_SELECT_HD float rdmi_select_value(uint32_t key) {
  const uint32_t b = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  float v;
  memcpy(&v, &b, 4);
  return v;
}

// bit position of pass p's digit (pass 0 takes the most significant one)
RDMI_SELECT_HD int rdmi_select_shift(int pass) { return 32 - kSelectDigitBits * (pass + 1); }

RDMI_SELECT_HD uint32_t rdmi_select_digit(uint32_t key, int pass) {
  return (key >> rdmi_select_shift(pass)) & (uint32_t)(kSelectBins - 1);
}

// the key bits above pass p's digit: the prefix that passes 0 … p − 1 chose (0 for pass 0)
RDMI_SELECT_HD uint32_t rdmi_select_prefix_mask(int pass) {
  return pass == 0 ? 0u : ~0u << (32 - kSelectDigitBits * pass);
}

// 0-based rank of the fraction q among cnt ≥ 1 values
RDMI_SELECT_HD uint64_t rdmi_select_rank(double q, uint64_t cnt) {
  const double r = q * (double)(cnt - 1);  // ≥ 0 and ≤ cnt − 1 for q in [0, 1]: the conversion truncates = floor
  const uint64_t k = (uint64_t)r;
  return k < cnt ? k : cnt - 1;
}

// Walk one histogram: the first bin whose running count exceeds `rank`, and the rank inside that bin.
// false when the histogram holds no more than `rank` values (nothing counted: bin and rank_in are left alone).
RDMI_SELECT_HD bool rdmi_select_pick_bin(const uint64_t* hist, uint64_t rank, int* bin, uint64_t* rank_in) {
  uint64_t below = 0;
  for (int b = 0; b < kSelectBins; ++b) {
    const uint64_t c = hist[b];
    if (rank - below < c) {
      *bin = b;
      *rank_in = rank - below;
      return true;
    }
    below += c;
  }
  return false;
}
