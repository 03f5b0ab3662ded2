// simdjson_amd/csrc/sj_dtoa.h -- the bits of a finite binary64 -> the text the reference's to_chars(double) gives for it (what simdjson::minify prints for a
// double element): the SHORTEST decimal digits that read back as the same double and, among those, the closest to it, laid out with a trailing ".0" on an integral value,
// as 0.000ddd down to 1e-4, as plain digits below 1e15 and as d.ddde+XX / de-XX elsewhere.
//
// Behaviour restated (not code).  The digits: R. Giulietti, "The Schubfach way to render doubles" (2020; the algorithm of Java's Double.toString since JDK 19):
// with v = c 2^q and k = floor(log10(2^q)) the candidates are the two multiples of 10^k -- and, one digit shorter, of 10^(k+1) -- that bracket v; whichever lies inside
// v's rounding interval wins, the shorter first, the closer on a tie of lengths.  The interval's ends and v itself are scaled by 10^-k with ONE 64 x 128 -> 192-bit
// product each against g(-k) of sj_pow10_table.inc, keeping a sticky bit ("round to odd") so that every comparison is exact.  No floating point anywhere.
// The reference reaches the same digits another way (Dragonbox: J. Jeon, 2020); shortest-and-closest is a property of the VALUE, so the two agree on every double
// (tests/test_dtoa.py: the fixture's table, and two million random bit patterns and every power of two against the live reference).
// The layout: what the reference's format_buffer does with min_exp = -4 and max_exp = 15 (src/to_chars.cpp of the reference, format_buffer), restated in dtoa_layout.
//
// All functions are host + device: the kernels of sjgpu_json.hip and tests/host/test_dtoa.cpp (g++) use the same code.  Nothing here indexes a local array at run time:
// the digits leave least significant first, straight to where they belong in `out`.
#ifndef SJGPU_SJ_DTOA_H
#define SJGPU_SJ_DTOA_H

#include "sj_number.h"

namespace sjgpu {

constexpr int POW10_SMALLEST = -292, POW10_LARGEST = 324;
constexpr u32 DTOA_MAX_BYTES = 24; // -d.dddddddddddddddde-XXX
#if defined(__HIPCC__)
static __device__ const u64 d_pow10_128[2 * (POW10_LARGEST - POW10_SMALLEST + 1)] = {
#include "sj_pow10_table.inc"
};
#endif
static const u64 h_pow10_128[2 * (POW10_LARGEST - POW10_SMALLEST + 1)] = {
#include "sj_pow10_table.inc"
};
SJ_HD u64 pow10_word(int k, int which) { // which: 0 = high, 1 = low
#if defined(__HIP_DEVICE_COMPILE__)
  return d_pow10_128[2 * (k - POW10_SMALLEST) + which];
#else
  return h_pow10_128[2 * (k - POW10_SMALLEST) + which];
#endif
}

// floor(log10(2^e)), floor(log10(3/4 2^e)), floor(log2(10^e)) for the exponents a double meets (the paper's section 9.2: fixed-point multiples of log10(2) and log2(10))
SJ_HD int floor_log10_pow2(int e) { return int((long long)e * 1262611 >> 22); }
SJ_HD int floor_log10_three_quarters_pow2(int e) { return int(((long long)e * 1262611 - 524031) >> 22); }
SJ_HD int floor_log2_pow10(int e) { return int((long long)e * 1741647 >> 19); }

// the top 64 bits of g * cp (g: 128 bits as hi, lo; cp < 2^64), the lowest of them set when anything below is: a value that compares like the exact product
SJ_HD u64 mul_round_to_odd(u64 g_hi, u64 g_lo, u64 cp) {
  u64 x_hi, x_lo, y_hi, y_lo;
  mul64x64(g_lo, cp, x_hi, x_lo);
  mul64x64(g_hi, cp, y_hi, y_lo);
  const u64 mid = y_lo + x_hi;
  const u64 top = y_hi + (mid < y_lo ? 1u : 0u);
  return top | (mid > 1u ? 1u : 0u);
}

struct decimal64 {
  u64 digits; // 1 .. 17 digits, no trailing zero
  int exponent; // value = digits * 10^exponent
};

SJ_HD bool dtoa_is_finite(u64 bits) { return ((bits >> 52) & 0x7FFu) != 0x7FFu; }

// the shortest digits of |the double whose bits these are|: finite and not zero
SJ_HD decimal64 dtoa_shortest(u64 bits) {
  const u64 fraction = bits & 0x000FFFFFFFFFFFFFull;
  const int biased = int((bits >> 52) & 0x7FFu);
  u64 c;
  int q;
  u64 digits;
  int exponent;
  bool done = false;
  if (biased != 0) {
    c = fraction | 0x0010000000000000ull;
    q = biased - 1075;
    if (q <= 0 && q > -53 && (c & ((1ull << -q) - 1u)) == 0) { // an integer below 2^53: itself
      digits = c >> -q;
      exponent = 0;
      done = true;
    }
  } else {
    c = fraction;
    q = -1074;
  }
  if (!done) {
    const bool even = (c & 1u) == 0;
    const bool closer_below = fraction == 0 && biased > 1; // the gap below a power of two is half the gap above it
    const u64 cbl = 4u * c - 2u + (closer_below ? 1u : 0u), cb = 4u * c, cbr = 4u * c + 2u;
    const int k = closer_below ? floor_log10_three_quarters_pow2(q) : floor_log10_pow2(q);
    const int h = q + floor_log2_pow10(-k) + 1; // 1 .. 4
    const u64 g_hi = pow10_word(-k, 0), g_lo = pow10_word(-k, 1);
    const u64 vbl = mul_round_to_odd(g_hi, g_lo, cbl << h), vb = mul_round_to_odd(g_hi, g_lo, cb << h), vbr = mul_round_to_odd(g_hi, g_lo, cbr << h);
    const u64 lower = vbl + (even ? 0u : 1u), upper = vbr - (even ? 0u : 1u); // an even significand's interval is closed: the ends round back to it
    const u64 s = vb >> 2;
    exponent = k;
    bool settled = false;
    if (s >= 10u) { // one digit fewer
      const u64 sp = s / 10u;
      const bool below_in = lower <= 40u * sp, above_in = 40u * sp + 40u <= upper;
      if (below_in != above_in) {
        digits = sp + (above_in ? 1u : 0u);
        exponent = k + 1;
        settled = true;
      }
    }
    if (!settled) {
      const bool below_in = lower <= 4u * s, above_in = 4u * s + 4u <= upper;
      if (below_in != above_in) {
        digits = s + (above_in ? 1u : 0u);
      } else { // both or neither: the closer one, the even one at the midpoint
        const u64 mid = 4u * s + 2u;
        const bool up = vb > mid || (vb == mid && (s & 1u));
        digits = s + (up ? 1u : 0u);
      }
    }
  }
  for (int round = 0; round < 17 && digits % 10u == 0; round++) { // (digits is not zero)
    digits /= 10u;
    exponent++;
  }
  decimal64 r;
  r.digits = digits;
  r.exponent = exponent;
  return r;
}

// how many decimal digits v has (v = 0: one)
SJ_HD u32 decimal_digits(u64 v) {
  u32 n = 1;
  u64 bound = 10u;
  while (n < 20u && v >= bound) { // (10^19 < 2^64 < 10^20)
    n++;
    if (n < 20u) { bound *= 10u; }
  }
  return n;
}

// the digits of v into out[0 .. n), n = decimal_digits(v), the last one first
SJ_HD void write_decimal(u8 *out, u64 v, u32 n) {
  for (u32 i = n; i > 0; i--) {
    out[i - 1u] = u8('0' + u32(v % 10u));
    v /= 10u;
  }
}

// where the layout puts k digits with decimal exponent e: n = k + e is the position of the decimal point behind the first digit
struct dtoa_layout {
  u32 kind;   // 0: ddd000.0   1: dd.ddd   2: 0.000ddd   3: d.ddde+XX / de+XX
  u32 length; // of the magnitude, without a sign
};
SJ_HD dtoa_layout dtoa_layout_of(u32 k, int e) {
  const int n = int(k) + e;
  dtoa_layout L;
  if (int(k) <= n && n <= 15) {
    L.kind = 0;
    L.length = u32(n) + 2u;
  } else if (0 < n && n <= 15) {
    L.kind = 1;
    L.length = k + 1u;
  } else if (-4 < n && n <= 0) {
    L.kind = 2;
    L.length = 2u + u32(-n) + k;
  } else {
    const int x = n - 1 < 0 ? 1 - n : n - 1;
    L.kind = 3;
    L.length = (k == 1u ? 1u : k + 1u) + 2u + (x < 100 ? 2u : 3u);
  }
  return L;
}

// the length of the text of a finite double, sign included: 3 .. 24
SJ_HD u32 dtoa_length(u64 bits) {
  const u32 sign = u32(bits >> 63);
  if ((bits << 1) == 0) { return sign + 3u; } // 0.0, -0.0
  const decimal64 d = dtoa_shortest(bits);
  return sign + dtoa_layout_of(decimal_digits(d.digits), d.exponent).length;
}

// the text of a finite double into out[0 .. dtoa_length(bits)) -> that length
SJ_HD u32 dtoa_write(u64 bits, u8 *out) {
  u32 at = 0;
  if (bits >> 63) { out[at++] = u8('-'); }
  if ((bits << 1) == 0) {
    out[at] = u8('0');
    out[at + 1u] = u8('.');
    out[at + 2u] = u8('0');
    return at + 3u;
  }
  const decimal64 d = dtoa_shortest(bits);
  const u32 k = decimal_digits(d.digits);
  const dtoa_layout L = dtoa_layout_of(k, d.exponent);
  const int n = int(k) + d.exponent;
  u8 *p = out + at;
  if (L.kind == 0) {
    write_decimal(p, d.digits, k);
    for (u32 i = k; i < u32(n); i++) { p[i] = u8('0'); }
    p[n] = u8('.');
    p[n + 1] = u8('0');
  } else if (L.kind == 1) { // the digits one place apart around the point
    u64 v = d.digits;
    for (u32 i = k; i > 0; i--) {
      const u32 pos = i - 1u < u32(n) ? i - 1u : i;
      p[pos] = u8('0' + u32(v % 10u));
      v /= 10u;
    }
    p[n] = u8('.');
  } else if (L.kind == 2) {
    const u32 pad = u32(-n);
    p[0] = u8('0');
    p[1] = u8('.');
    for (u32 i = 0; i < pad; i++) { p[2u + i] = u8('0'); }
    write_decimal(p + 2u + pad, d.digits, k);
  } else {
    u32 end;
    if (k == 1u) {
      p[0] = u8('0' + u32(d.digits));
      end = 1u;
    } else {
      u64 v = d.digits;
      for (u32 i = k; i > 1u; i--) {
        p[i] = u8('0' + u32(v % 10u));
        v /= 10u;
      }
      p[0] = u8('0' + u32(v));
      p[1] = u8('.');
      end = k + 1u;
    }
    int x = n - 1;
    p[end++] = u8('e');
    p[end++] = u8(x < 0 ? '-' : '+');
    x = x < 0 ? -x : x;
    if (x >= 100) {
      p[end++] = u8('0' + u32(x / 100));
      x %= 100;
    }
    p[end++] = u8('0' + u32(x / 10));
    p[end++] = u8('0' + u32(x % 10));
  }
  return at + L.length;
}

} // namespace sjgpu
#endif
