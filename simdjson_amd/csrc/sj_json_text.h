// simdjson_amd/csrc/sj_json_text.h -- the JSON text of a string and of an integer, as the reference's mini_formatter writes them (include/simdjson/dom/serialization-inl.h
// of the reference: string, number(int64_t), number(uint64_t); behaviour restated, not code).
//   a string   its UNESCAPED bytes between quotes: " and \ behind a backslash, 0x08 / 0x09 / 0x0a / 0x0c / 0x0d as \b \t \n \f \r, every other byte up to 0x1f as \u00xx with
//              lower-case hex, every other byte -- 0x7f, the bytes of multi-byte characters and a / included -- as it is
//   an int64   an optional '-' and the shortest decimal of the magnitude (-9223372036854775808 has no positive twin: the magnitude is taken in 64 unsigned bits)
//   a uint64   decimal_digits / write_decimal of sj_dtoa.h
// Every function comes as a pair: the length alone (the count pass) and the bytes (the fill pass), which writes out[0 .. length) and, given `room` bytes, never beyond
// them.  Host + device: the kernels of sjgpu_json.hip and tests/host (g++) use the same code.  Nothing here indexes a local array at run time.
#ifndef SJGPU_SJ_JSON_TEXT_H
#define SJGPU_SJ_JSON_TEXT_H

#include "sj_dtoa.h"

namespace sjgpu {

SJ_HD u32 int64_text_length(u64 bits) {
  const bool negative = (bits >> 63) != 0;
  return (negative ? 1u : 0u) + decimal_digits(negative ? 0u - bits : bits);
}
SJ_HD u32 int64_text_write(u64 bits, u8 *out) {
  const bool negative = (bits >> 63) != 0;
  const u64 magnitude = negative ? 0u - bits : bits;
  const u32 n = decimal_digits(magnitude);
  if (negative) { out[0] = u8('-'); }
  write_decimal(out + (negative ? 1u : 0u), magnitude, n);
  return n + (negative ? 1u : 0u);
}

// how many bytes the byte c takes inside the quotes: 1, 2 or 6
SJ_HD u32 escaped_size(u32 c) {
  if (c >= 0x20u) { return c == '"' || c == '\\' ? 2u : 1u; }
  return c == 0x08u || c == 0x09u || c == 0x0Au || c == 0x0Cu || c == 0x0Du ? 2u : 6u;
}
// the letter behind the backslash of a two-byte escape
SJ_HD u32 escape_letter(u32 c) { return c == 0x08u ? 'b' : c == 0x09u ? 't' : c == 0x0Au ? 'n' : c == 0x0Cu ? 'f' : c == 0x0Du ? 'r' : c; }
SJ_HD u32 hex_digit(u32 v) { return v < 10u ? '0' + v : 'a' + (v - 10u); }

// whether one of the eight bytes of w is below 0x20, a quote or a backslash (exact: the borrow of a byte that qualifies can only reach bytes above it)
SJ_HD bool any_byte_needs_escape(u64 w) {
  const u64 ones = 0x0101010101010101ull, high = 0x8080808080808080ull;
  const u64 below = (w - ones * 0x20u) & ~w;
  const u64 q = w ^ (ones * 0x22u), b = w ^ (ones * 0x5Cu);
  return ((below | ((q - ones) & ~q) | ((b - ones) & ~b)) & high) != 0;
}
SJ_HD u64 load8(const u8 *p) {
  u64 w;
  __builtin_memcpy(&w, p, 8);
  return w;
}

// the length of the quoted, escaped text of s[0 .. len): at least 2.  Reads s[0 .. len) and nothing else
SJ_HD u64 escaped_length(const u8 *s, u32 len) {
  u64 total = 2;
  u32 i = 0;
  for (; i + 8u <= len; i += 8u) {
    if (!any_byte_needs_escape(load8(s + i))) {
      total += 8u;
    } else {
      for (u32 j = 0; j < 8u; j++) { total += escaped_size(s[i + j]); }
    }
  }
  for (; i < len; i++) { total += escaped_size(s[i]); }
  return total;
}

// one byte inside the quotes to out[0 ..], no byte at or beyond out + room -> its size
SJ_HD u32 escape_byte(u32 c, u8 *out, u64 room) {
  const u32 size = escaped_size(c);
  if (size > room) { return size; }
  if (size == 1u) {
    out[0] = u8(c);
  } else if (size == 2u) {
    out[0] = u8('\\');
    out[1] = u8(escape_letter(c));
  } else {
    out[0] = u8('\\');
    out[1] = u8('u');
    out[2] = u8('0');
    out[3] = u8('0');
    out[4] = u8(hex_digit(c >> 4));
    out[5] = u8(hex_digit(c & 15u));
  }
  return size;
}

// the quoted, escaped text of s[0 .. len) to out[0 .. escaped_length(s, len)), no byte at or beyond out + room -> its length.  Eight bytes that need no escape move as
// one word: a store that lies inside the text's own bytes, wherever they begin
SJ_HD u64 escape_write(const u8 *s, u32 len, u8 *out, u64 room) {
  u64 at = 0;
  if (at < room) { out[at] = u8('"'); }
  at++;
  u32 i = 0;
  for (; i + 8u <= len; i += 8u) {
    const u64 w = load8(s + i);
    if (!any_byte_needs_escape(w) && at + 8u <= room) {
      __builtin_memcpy(out + at, &w, 8);
      at += 8u;
    } else {
      for (u32 j = 0; j < 8u; j++) { at += escape_byte(s[i + j], out + at, at < room ? room - at : 0u); }
    }
  }
  for (; i < len; i++) { at += escape_byte(s[i], out + at, at < room ? room - at : 0u); }
  if (at < room) { out[at] = u8('"'); }
  return at + 1u;
}

// s[0 .. len) as it is to out[0 .. len), no byte at or beyond out + room -> len.  Eight bytes at a time while they fit, as escape_write moves them
SJ_HD u64 raw_write(const u8 *s, u64 len, u8 *out, u64 room) {
  const u64 n = len < room ? len : room;
  u64 i = 0;
  for (; i + 8u <= n; i += 8u) {
    const u64 w = load8(s + i);
    __builtin_memcpy(out + i, &w, 8);
  }
  for (; i < n; i++) { out[i] = s[i]; }
  return len;
}

// Where one writer of text writes: out[0 .. room), `at` counts on beyond it.  FILL = false is the count pass: nothing is stored, `at` is the length.
// (the sink of sjgpu_write.hip; sjgpu_json.hip keeps the one it was measured with)
template <bool FILL>
struct text_sink {
  u8 *out;
  u64 room, at;
  SJ_HD void put(u32 c) {
    if (FILL && at < room) { out[at] = u8(c); }
    at++;
  }
  SJ_HD void put_null() { put('n'); put('u'); put('l'); put('l'); }
  SJ_HD void put_bool(bool v) {
    if (v) {
      put('t'); put('r'); put('u'); put('e');
    } else {
      put('f'); put('a'); put('l'); put('s'); put('e');
    }
  }
  // what: 0 an int64, 1 a uint64, 2 a finite double, each as its 64 bits
  SJ_HD void put_number(u32 what, u64 v) {
    u32 length = 0;
    const bool fits = FILL && at + DTOA_MAX_BYTES <= room; // (24 >= the 20 of an integer)
    if (!fits) { length = what == 2u ? dtoa_length(v) : what == 0u ? int64_text_length(v) : decimal_digits(v); }
    if (FILL && (fits || at + length <= room)) {
      u8 *p = out + at;
      if (what == 2u) {
        length = dtoa_write(v, p);
      } else if (what == 0u) {
        length = int64_text_write(v, p);
      } else {
        length = decimal_digits(v);
        write_decimal(p, v, length);
      }
    }
    at += length;
  }
  SJ_HD void put_string(const u8 *s, u32 len) {
    if (FILL) {
      at += escape_write(s, len, out + (at < room ? at : room), at < room ? room - at : 0u);
    } else {
      at += escaped_length(s, len);
    }
  }
  SJ_HD void put_raw(const u8 *s, u64 len) {
    if (FILL) {
      at += raw_write(s, len, out + (at < room ? at : room), at < room ? room - at : 0u);
    } else {
      at += len;
    }
  }
};

} // namespace sjgpu
#endif
