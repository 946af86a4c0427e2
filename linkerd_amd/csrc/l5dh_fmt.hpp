// l5dh_fmt.hpp -- Java number texts for host and device: Long.toString, the unsigned
// 64-bit decimal, and Double.toString / Float.toString as JDK 8 prints them
// (sun.misc.FloatingDecimal: BinaryToASCIIBuffer.dtoa + getChars).  A port of linkerd_amd/javafmt.py, which restates
// that algorithm and is pinned by raw JDK-8 texts (tests/test_javafmt.py); the names
// follow that module.  Plain C++ when __HIPCC__ is absent.
//
// Domain of format_double: +-0.0, NaN, +-Infinity and finite 2^-64 <= |x| < 2^64 (all
// that sum / count of two int64 can be).  Anything else -- and anything that would leave
// the fixed-width integer below -- returns FMT_RANGE and writes nothing meaningful:
// a value is never printed wrongly.
//
// The three arithmetic forms of the digit loop are not interchangeable and are selected
// as the JDK selects them (Bbits, tenSbits): the 32-bit and 64-bit forms let 10 M wrap
// (the JDK's `m > 0` test catches it, and its high test is `>`), the big form is exact
// and tests high with `>=`.  Wrapping is done in unsigned types and cast.
//
// Width of the big form's integer.  With x = f 2^e (f the stripped fraction, nFractBits
// bits) the JDK scales B = x 10^B5 2^nTinyBits and S = 10^S5 2^nTinyBits, drops their
// common power of two, and shifts both up by -M2 when the half-ulp M would be fractional.
//   x >= 1:  B5 = 0 and x 2^nTinyBits is either x itself (< 2^64) or f (< 2^53).
//   x < 1:   B5 = -decExp <= 20, and B = f 10^B5 < 2^53 10^20 < 2^120.
//   shifted: then B2 = 54 - nFractBits (+1), so B < 2^55 5^20 < 2^102.
// The estimate makes B / S lie in [0.1, 10), so 10 S <= 100 B < 2^127; the loop keeps
// B < 10 S, and 10^k M passes B + 10^k M >= 10 S at most one step late, so M, B + M and
// 2 B - 10 S stay below 2^132.  (javafmt's own B, 10 S and M 10^18 over 38 700 sampled
// doubles of the domain reach 110 bits.)  192 bits leave 60 bits of margin; a carry or a
// shift out of them raises the overflow mark, which ends in FMT_RANGE.
//
// Domain of format_float: every float.  The same 192 bits cover the whole float range
// (f is the float's fraction widened to the double layout, nFractBits <= 24, and
// nSignificantBits = 24, or fewer for a subnormal):
//   x >= 1:  B5 = 0, B = x 2^nTinyBits is x itself (< 2^128) or f (< 2^24); S = 10^S5 with
//            S5 <= 38, so S < 2^127 and 10 S < 2^131.  Shifted up by -M2 <= 25 only when
//            nTinyBits > 0, i.e. x < 2^24: B < 2^50.
//   x < 1:   B5 = -decExp <= 46 (2^-149 = 1.4E-45), 5^46 < 2^107, and after the common power
//            of two is dropped B2 = 0, then the shift -M2 = nSignificantBits + 1 - nFractBits
//            <= 25: B < 2^24 2^107 2^25 = 2^156.  (With B / S in [0.1, 10) and S = 2^S2,
//            S2 <= 149 - B5 + 25, the values met are far smaller: S2 = 112 at FLT_MIN, 106 at
//            the least subnormal.)
// As above 10 S <= 100 B and M, B + M, 2 B - 10 S stay within 12 bits of B: below 2^168.
// So for a float (dtoa<true>) 5^k is taken beyond the 27 powers that fit a word
// (Big::mul_pow5, n5bits' 3 k as the JDK estimates it); format_double (dtoa<false>) keeps
// its bounds and its code.  The overflow mark still ends in FMT_RANGE.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define L5DH_HD __host__ __device__ inline
// (a kernel's formatter stays part of the kernel however many kernels format: no call, no stack)
#define L5DH_HD_FLAT __host__ __device__ __forceinline__
#else
#define L5DH_HD inline
#define L5DH_HD_FLAT inline
#endif

namespace l5dh {
namespace fmt {

constexpr int DOUBLE_CHARS = 26;  // = L5DH_DOUBLE_CHARS (FloatingDecimal's own buffer)
constexpr int FLOAT_CHARS = 16;   // = L5DH_FLOAT_CHARS: "-1.17549435E-38" is the longest, 15
constexpr int LONG_CHARS = 20;    // = L5DH_LONG_CHARS: "-9223372036854775808", "18446744073709551615"
constexpr int FMT_RANGE = -1;     // outside the domain

// ---- integers ---------------------------------------------------------------------
L5DH_HD int ulong_digits(uint64_t v) {
  int n = 1;
  for (uint64_t p = 10ull; n < 20 && v >= p; p *= 10ull) ++n;  // (10^19 fits; the loop ends at 20)
  return n;
}

// (the magnitude is taken unsigned: -2^63 has no signed negation)
L5DH_HD uint64_t long_magnitude(int64_t v) { return v < 0 ? 0ull - (uint64_t)v : (uint64_t)v; }

L5DH_HD int long_digits(int64_t v) { return ulong_digits(long_magnitude(v)) + (v < 0 ? 1 : 0); }

template <class Ch>
L5DH_HD int format_ulong(uint64_t v, Ch* out) {
  const int n = ulong_digits(v);
  for (int i = n - 1; i >= 0; --i) {
    out[i] = (Ch)('0' + (int)(v % 10ull));
    v /= 10ull;
  }
  return n;
}

template <class Ch>
L5DH_HD int format_long(int64_t v, Ch* out) {  // Long.toString
  if (v < 0) {
    out[0] = (Ch)'-';
    return 1 + format_ulong(long_magnitude(v), out + 1);
  }
  return format_ulong((uint64_t)v, out);
}

// ---- Double.toString ----------------------------------------------------------------
constexpr int EXP_SHIFT = 52;
constexpr uint64_t FRACT_HOB = 1ull << EXP_SHIFT;
constexpr int EXP_BIAS = 1023;
constexpr int MAX_SMALL_BIN_EXP = 62;
constexpr int MIN_SMALL_BIN_EXP = -21;
constexpr int N_POW5 = 27;      // FloatingDecimal.N_5_BITS has 27 entries; 5^26 < 2^63
constexpr int MAX_DIGITS = 24;  // (the JDK's digit buffer holds 20)

L5DH_HD int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

L5DH_HD uint64_t pow5(int k) {  // k < N_POW5
  uint64_t p = 1ull;
  for (int i = 0; i < k; ++i) p *= 5ull;
  return p;
}

constexpr int MAX_POW5 = 47;    // 5^k of the big form: a float needs k <= 46 (5^47 < 2^110)

// N_5_BITS[k]; Wide: past the table the JDK's own estimate 3 k (>= 81: the big form)
template <bool Wide>
L5DH_HD int n5bits(int k) { return !Wide || k < N_POW5 ? bit_length(pow5(k)) : 3 * k; }

// INSIGNIFICANT_DIGITS[p2].  On the exact-long path binExp <= 62, so p2 = binExp - 54 <= 8
// for a double: the table's first 16 entries, a nibble each (0 0 0 0 1 1 1 2 2 2 3 3 3 3 4
// 4).  For a float (Wide) p2 = binExp - 25 <= 37: the table is floor(p2 log10 2) for p2 < 63,
// taken as 1233 / 4096.
template <bool Wide>
L5DH_HD int insignificant_digits(int p2) {
  return Wide ? (p2 * 1233) >> 12 : (int)((0x4433332221110000ull >> (4 * p2)) & 15ull);
}

// floor((d2 - 1.5) 0.289529654 + 0.176091259 + binExp log10(2)), d2 in [1, 2): each step
// rounded on its own (no contraction), in javafmt's order.
L5DH_HD int estimate_dec_exp(uint64_t fract_bits, int bin_exp) {
  const uint64_t bits = ((uint64_t)EXP_BIAS << EXP_SHIFT) | (fract_bits & (FRACT_HOB - 1));
  double d2;
  __builtin_memcpy(&d2, &bits, 8);
#if defined(__HIP_DEVICE_COMPILE__)
  const double a = __dadd_rn(__dmul_rn(__dsub_rn(d2, 1.5), 0.289529654), 0.176091259);
  const double d = __dadd_rn(a, __dmul_rn((double)bin_exp, 0.301029995663981));
#else
  volatile double t = d2 - 1.5;
  t = t * 0.289529654;
  t = t + 0.176091259;
  volatile double u = (double)bin_exp * 0.301029995663981;
  const double d = t + u;
#endif
  int e = (int)d;  // (|d| < 400)
  if ((double)e > d) --e;
  return e;
}

struct Digits {
  uint8_t d[MAX_DIGITS];
  int n = 0;
  int dec_exponent = 0;
  bool bad = false;  // more digits than the buffer holds, or a quotient above 9
  L5DH_HD void push(int q) {
    if (n < MAX_DIGITS && q >= 0 && q <= 9)
      d[n++] = (uint8_t)q;
    else
      bad = true;
  }
  L5DH_HD void roundup() {
    int i = n - 1;
    int q = d[i];
    if (q == 9) {
      while (q == 9 && i > 0) {
        d[i] = 0;
        --i;
        q = d[i];
      }
      if (q == 9) {  // carry out: high-order 1, rest 0s, larger exponent
        ++dec_exponent;
        d[0] = 1;
        return;
      }
    }
    d[i] = (uint8_t)(q + 1);
  }
};

// The fixed-width unsigned integer of the big form: 192 bits, least significant word
// first.  Every loop has constant bounds, so the words stay in registers on the device.
struct Big {
  static constexpr int W = 6;
  uint32_t w[W];
  bool ovf;  // a carry or a shift left the width: the result is FMT_RANGE
  L5DH_HD explicit Big(uint64_t v) : ovf(false) {
    for (int i = 0; i < W; ++i) w[i] = 0u;
    w[0] = (uint32_t)v;
    w[1] = (uint32_t)(v >> 32);
  }
  L5DH_HD void mul(uint32_t m) {
    uint64_t carry = 0ull;
    for (int i = 0; i < W; ++i) {
      const uint64_t t = (uint64_t)w[i] * m + carry;
      w[i] = (uint32_t)t;
      carry = t >> 32;
    }
    ovf = ovf || carry != 0ull;
  }
  L5DH_HD void mul_pow5(int k) {  // 5^13 < 2^32; any k >= 0
    for (; k >= 13; k -= 13) mul(1220703125u);
    mul((uint32_t)pow5(k));
  }
  L5DH_HD void shl(int n) {  // n >= 0
    for (; n >= 32; n -= 32) {
      ovf = ovf || w[W - 1] != 0u;
      for (int i = W - 1; i > 0; --i) w[i] = w[i - 1];
      w[0] = 0u;
    }
    if (n > 0) {
      ovf = ovf || (w[W - 1] >> (32 - n)) != 0u;
      for (int i = W - 1; i > 0; --i) w[i] = (w[i] << n) | (w[i - 1] >> (32 - n));
      w[0] <<= n;
    }
  }
  L5DH_HD void add(const Big& o) {
    uint64_t carry = 0ull;
    for (int i = 0; i < W; ++i) {
      const uint64_t t = (uint64_t)w[i] + o.w[i] + carry;
      w[i] = (uint32_t)t;
      carry = t >> 32;
    }
    ovf = ovf || o.ovf || carry != 0ull;
  }
  L5DH_HD void sub(const Big& o) {  // *this >= o
    uint64_t borrow = 0ull;
    for (int i = 0; i < W; ++i) {
      const uint64_t t = (uint64_t)w[i] - o.w[i] - borrow;
      w[i] = (uint32_t)t;
      borrow = (t >> 32) & 1ull;
    }
  }
  L5DH_HD int cmp(const Big& o) const {
    int r = 0;
    for (int i = 0; i < W; ++i) r = w[i] != o.w[i] ? (w[i] < o.w[i] ? -1 : 1) : r;
    return r;
  }
  // q, *this = divmod(*this, s) by compare-and-subtract (q < 10 by the estimate; 10 stands
  // for "more", which Digits::push refuses)
  L5DH_HD int divmod(const Big& s) {
    int q = 0;
    while (q < 10 && cmp(s) >= 0) {
      sub(s);
      ++q;
    }
    return q;
  }
};

// A word of the 32-bit (narrow) or 64-bit form, read as the signed value the JDK compares.
L5DH_HD int64_t sw(bool narrow, uint64_t v) { return narrow ? (int64_t)(int32_t)(uint32_t)v : (int64_t)v; }

// FloatingDecimal.BinaryToASCIIBuffer.dtoa with isCompatibleFormat = true: fract_bits in
// the double layout with FRACT_HOB set; n_significant_bits = 53 for a double, 24 for a
// float, fewer for a float's subnormal.  Wide (the float's range): 5^k is taken up to
// MAX_POW5; else, as a double of format_double's domain needs, only while it fits a word.
template <bool Wide>
L5DH_HD bool dtoa(int bin_exp, uint64_t fract_bits, int n_sig, Digits& out) {
  const int n_significant_bits = Wide ? n_sig : EXP_SHIFT + 1;  // (a double's is a constant)
  const int tail_zeros = __builtin_ctzll(fract_bits);
  const int n_fract_bits = EXP_SHIFT + 1 - tail_zeros;
  const int n_tiny_bits = n_fract_bits - bin_exp - 1 > 0 ? n_fract_bits - bin_exp - 1 : 0;
  if (bin_exp >= MIN_SMALL_BIN_EXP && bin_exp <= MAX_SMALL_BIN_EXP && n_tiny_bits == 0) {
    // (n_tiny_bits == 0: n_fract_bits + N_5_BITS[0] < 64 holds, and bin_exp >= 0)
    // integral value that fits a long: print its digits exactly
    int insignificant = 0;
    if (bin_exp > n_significant_bits) {
      const int p2 = bin_exp - n_significant_bits - 1;
      insignificant = p2 > 1 ? insignificant_digits<Wide>(p2) : 0;
    }
    uint64_t lv = bin_exp >= EXP_SHIFT ? fract_bits << (bin_exp - EXP_SHIFT) : fract_bits >> (EXP_SHIFT - bin_exp);
    int dec_exponent = 0;
    if (insignificant) {
      uint64_t pow10 = 1ull;
      for (int i = 0; i < insignificant; ++i) pow10 *= 10ull;
      const uint64_t residue = lv % pow10;
      lv /= pow10;
      dec_exponent += insignificant;
      if (residue >= (pow10 >> 1)) ++lv;
    }
    uint8_t s[LONG_CHARS];
    const int len = format_ulong(lv, s);
    int keep = len;
    while (keep > 1 && s[keep - 1] == '0') --keep;
    for (int i = 0; i < keep; ++i) out.push(s[i] - '0');
    out.dec_exponent = dec_exponent + len;
    return !out.bad;
  }
  int dec_exp = estimate_dec_exp(fract_bits, bin_exp);
  const int B5 = -dec_exp > 0 ? -dec_exp : 0;
  int B2 = B5 + n_tiny_bits + bin_exp;
  const int S5 = dec_exp > 0 ? dec_exp : 0;
  int S2 = S5 + n_tiny_bits;
  const int M5 = B5;
  int M2 = B2 - n_significant_bits;
  // (outside the domain: 5^k leaves the table, or a word)
  if (Wide ? (B5 + 1 > MAX_POW5 || S5 + 1 > MAX_POW5) : (B5 >= N_POW5 - 1 || S5 + 1 >= N_POW5)) return false;
  fract_bits >>= tail_zeros;
  B2 -= n_fract_bits - 1;
  const int common2 = B2 < S2 ? B2 : S2;
  B2 -= common2;
  S2 -= common2;
  M2 -= common2;
  if (n_fract_bits == 1) M2 -= 1;  // exact power of two: the next smaller number is half as far
  if (M2 < 0) {
    B2 -= M2;
    S2 -= M2;
    M2 = 0;
  }
  if (B2 < 0 || S2 < 0) return false;  // (never for a double of the domain)
  const int Bbits = n_fract_bits + B2 + n5bits<Wide>(B5);
  const int tenSbits = S2 + 1 + n5bits<Wide>(S5 + 1);
  bool low, high;
  int low_digit_difference;  // its sign only
  if (Bbits < 64 && tenSbits < 64) {
    // int (32-bit) or long (64-bit) arithmetic: b, s and 10 s are exact; m may wrap, which
    // the JDK catches with `m > 0` (then both stopping tests hold).
    const bool narrow = Bbits < 32 && tenSbits < 32;
    uint64_t b = (fract_bits * pow5(B5)) << B2;
    const uint64_t s = pow5(S5) << S2;
    uint64_t m = pow5(M5) << M2;
    const uint64_t tens = s * 10ull;
    int q = 0;
    for (; q < 10 && b >= s; ++q) b -= s;
    b *= 10ull;
    m *= 10ull;
    low = (int64_t)b < sw(narrow, m);
    high = sw(narrow, b + m) > (int64_t)tens;
    if (q == 0 && !high)
      --dec_exp;  // the estimate was one too high: drop the leading zero
    else
      out.push(q);
    if (dec_exp < -3 || dec_exp >= 8) high = low = false;  // E-form: at least two digits
    while (!low && !high && !out.bad) {
      q = 0;
      for (; q < 10 && b >= s; ++q) b -= s;
      b *= 10ull;
      m *= 10ull;
      if (sw(narrow, m) > 0) {
        low = (int64_t)b < sw(narrow, m);
        high = sw(narrow, b + m) > (int64_t)tens;
      } else {
        low = high = true;
      }
      out.push(q);
    }
    const int64_t ldd = (int64_t)((b << 1) - tens);  // (|2 b - 10 s| < 10 s: exact in either width)
    low_digit_difference = ldd > 0 ? 1 : (ldd < 0 ? -1 : 0);
  } else {
    // FDBigInteger arithmetic (exact); note the `>=` in the high test
    Big Sval(Wide ? 1ull : pow5(S5)), Bval(fract_bits), Mval(1ull), tenSval(1ull);
    if (Wide) Sval.mul_pow5(S5);
    Sval.shl(S2);
    Bval.mul_pow5(B5);
    Bval.shl(B2);
    Mval.mul_pow5(M5 + 1);  // 10 M
    Mval.shl(M2 + 1);
    tenSval.mul_pow5(S5 + 1);
    tenSval.shl(S2 + 1);
    int q = Bval.divmod(Sval);
    Bval.mul(10u);
    Big sum = Bval;
    sum.add(Mval);
    low = Bval.cmp(Mval) < 0;
    high = sum.cmp(tenSval) >= 0;
    if (q == 0 && !high)
      --dec_exp;
    else
      out.push(q);
    if (dec_exp < -3 || dec_exp >= 8) high = low = false;
    while (!low && !high && !out.bad) {
      q = Bval.divmod(Sval);
      Bval.mul(10u);
      Mval.mul(10u);
      sum = Bval;
      sum.add(Mval);
      low = Bval.cmp(Mval) < 0;
      high = sum.cmp(tenSval) >= 0;
      out.push(q);
      if (Bval.ovf || Mval.ovf || sum.ovf) out.bad = true;
    }
    low_digit_difference = 0;
    if (high && low) {
      Big twice = Bval;
      twice.shl(1);
      low_digit_difference = twice.cmp(tenSval);
      if (twice.ovf) out.bad = true;
    }
    if (Sval.ovf || Bval.ovf || Mval.ovf || tenSval.ovf || sum.ovf) out.bad = true;
  }
  if (out.bad || out.n == 0) return false;
  out.dec_exponent = dec_exp + 1;
  if (high) {
    if (low) {
      if (low_digit_difference == 0) {
        if (out.d[out.n - 1] & 1) out.roundup();  // tie: round to an even last digit
      } else if (low_digit_difference > 0) {
        out.roundup();
      }
    } else {
      out.roundup();
    }
  }
  return true;
}

// BinaryToASCIIBuffer.getChars: plain form for 1e-3 <= |x| < 1e7, `0.00x`, or `E`.
template <class Ch>
L5DH_HD int get_chars(bool neg, const Digits& d, Ch* out) {
  int p = 0;
  const int n = d.n, e = d.dec_exponent;
  if (neg) out[p++] = (Ch)'-';
  if (e > 0 && e < 8) {
    const int k = n < e ? n : e;
    for (int i = 0; i < k; ++i) out[p++] = (Ch)('0' + d.d[i]);
    for (int i = k; i < e; ++i) out[p++] = (Ch)'0';
    out[p++] = (Ch)'.';
    if (k < n)
      for (int i = k; i < n; ++i) out[p++] = (Ch)('0' + d.d[i]);
    else
      out[p++] = (Ch)'0';
  } else if (e <= 0 && e > -3) {
    out[p++] = (Ch)'0';
    out[p++] = (Ch)'.';
    for (int i = 0; i < -e; ++i) out[p++] = (Ch)'0';
    for (int i = 0; i < n; ++i) out[p++] = (Ch)('0' + d.d[i]);
  } else {
    out[p++] = (Ch)('0' + d.d[0]);
    out[p++] = (Ch)'.';
    if (n > 1)
      for (int i = 1; i < n; ++i) out[p++] = (Ch)('0' + d.d[i]);
    else
      out[p++] = (Ch)'0';
    out[p++] = (Ch)'E';
    int x = e - 1;
    if (x < 0) {
      out[p++] = (Ch)'-';
      x = -x;
    }
    p += format_ulong((uint64_t)x, out + p);
  }
  return p;
}

template <class Ch>
L5DH_HD int put_text(const char* s, Ch* out) {
  int p = 0;
  for (; s[p]; ++p) out[p] = (Ch)s[p];
  return p;
}

// java.lang.Double.toString(double) on JDK 8 into out[DOUBLE_CHARS]: the length, or
// FMT_RANGE outside the domain.
template <class Ch>
L5DH_HD_FLAT int format_double(double x, Ch* out) {
  uint64_t bits;
  __builtin_memcpy(&bits, &x, 8);
  const bool neg = (bits >> 63) != 0ull;
  int bin_exp = (int)((bits >> EXP_SHIFT) & 0x7FFull);
  uint64_t fract = bits & (FRACT_HOB - 1);
  if (bin_exp == 0x7FF) return fract ? put_text("NaN", out) : put_text(neg ? "-Infinity" : "Infinity", out);
  if (bin_exp == 0) return fract ? FMT_RANGE : put_text(neg ? "-0.0" : "0.0", out);  // (subnormals: below 2^-64)
  bin_exp -= EXP_BIAS;
  if (bin_exp < -64 || bin_exp > 63) return FMT_RANGE;
  Digits d;
  if (!dtoa<false>(bin_exp, fract | FRACT_HOB, EXP_SHIFT + 1, d)) return FMT_RANGE;
  if (d.n + 7 > DOUBLE_CHARS) return FMT_RANGE;  // (sign, `.`, `E`, three exponent characters, `0.00`)
  return get_chars(neg, d, out);
}

// java.lang.Float.toString(float) on JDK 8 into out[FLOAT_CHARS]: the float widened to the
// double layout (fraction left-aligned to bit 52, a subnormal normalised and its
// significant bits counted), then the same dtoa and getChars.  The length, or FMT_RANGE.
template <class Ch>
L5DH_HD_FLAT int format_float(float x, Ch* out) {
  constexpr int F_FRAC = 23, F_BIAS = 127;
  uint32_t bits;
  __builtin_memcpy(&bits, &x, 4);
  const bool neg = (bits >> 31) != 0u;
  int bin_exp = (int)((bits >> F_FRAC) & 0xFFu);
  uint64_t fract = (uint64_t)(bits & ((1u << F_FRAC) - 1u)) << (EXP_SHIFT - F_FRAC);
  if (bin_exp == 0xFF) return fract ? put_text("NaN", out) : put_text(neg ? "-Infinity" : "Infinity", out);
  int n_sig = F_FRAC + 1;
  if (bin_exp == 0) {
    if (!fract) return put_text(neg ? "-0.0" : "0.0", out);
    const int lead = __builtin_clzll(fract);
    const int shift = lead - (63 - EXP_SHIFT);
    fract <<= shift;  // (its leading one arrives at FRACT_HOB)
    bin_exp = 1 - shift;
    n_sig = 64 - lead - (EXP_SHIFT - F_FRAC);
  } else {
    fract |= FRACT_HOB;
  }
  bin_exp -= F_BIAS;
  Digits d;
  if (!dtoa<true>(bin_exp, fract, n_sig, d)) return FMT_RANGE;
  if (d.n + 7 > FLOAT_CHARS) return FMT_RANGE;  // (nine digits at most, beside sign, `.`, `E-38` or `0.00`)
  return get_chars(neg, d, out);
}

}  // namespace fmt
}  // namespace l5dh
