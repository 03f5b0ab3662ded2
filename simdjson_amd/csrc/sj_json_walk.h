// simdjson_amd/csrc/sj_json_walk.h -- the one-lane walk of a cell's sub-tape, writing or counting its JSON text: what k_json_count / k_json_fill (sjgpu_json.hip) and the
// kernels of sjgpu_json_wide.hip share, the code as it was measured in sjgpu_json.hip, unchanged.  Device code: include it behind sjgpu_device.h, sj_json_text.h and
// sj_query_program.h, inside a unit's own anonymous namespace (every unit gets its own copy).
// PRETTY = true is the reference's pretty_formatter (include/sjgpu_pretty.h): the same walk with a layout around every word, decided at compile time --
// the minify instantiations hold none of it.
#ifndef SJGPU_SJ_JSON_WALK_H
#define SJGPU_SJ_JSON_WALK_H

namespace sjgpu {
namespace {

constexpr u32 JSON_THREADS = 256;
constexpr u32 JSON_MAX_WORKGROUPS = 512;
constexpr u32 JSON_REGISTER_LEVELS = 64, JSON_STRIP_WORDS = 63, JSON_MAX_LEVELS = JSON_REGISTER_LEVELS + 64 * JSON_STRIP_WORDS;
constexpr u64 LOW32 = 0xFFFFFFFFull, PAYLOAD = 0x00FFFFFFFFFFFFFFull;

typedef u32 __attribute__((aligned(1))) u32_unaligned;

// "is level L an object": a register for the first 64 levels, the lane's strip beyond
struct level_bits {
  u64 low;
  u64 *strip;
  __device__ __forceinline__ void set(u32 L, bool object) {
    if (L < JSON_REGISTER_LEVELS) {
      low = (low & ~(1ull << L)) | (u64(object) << L);
    } else {
      const u32 at = L - JSON_REGISTER_LEVELS;
      const u64 bit = 1ull << (at & 63u);
      const u64 word = strip[at >> 6]; // (what lies above the bit is of no level that is open: never read before it is set)
      strip[at >> 6] = object ? word | bit : word & ~bit;
    }
  }
  __device__ __forceinline__ bool get(u32 L) const {
    if (L < JSON_REGISTER_LEVELS) { return (low >> L) & 1u; }
    const u32 at = L - JSON_REGISTER_LEVELS;
    return (strip[at >> 6] >> (at & 63u)) & 1u;
  }
};

// where a lane writes: out[0 .. room), `at` counts on beyond it
template <bool FILL>
struct json_sink {
  u8 *out;
  u64 room, at;
  __device__ __forceinline__ void put(u32 c) {
    if (FILL && at < room) { out[at] = u8(c); }
    at++;
  }
  // n blanks, n a multiple of 4 up to 60 (an indent): sixteen, eight and four at a time while they fit, wherever they begin
  __device__ __forceinline__ void put_spaces(u32 n) {
    if (FILL && at + n <= room) {
      const u64 blanks[2] = {0x2020202020202020ull, 0x2020202020202020ull};
      u8 *p = out + at;
      u32 i = 0;
      for (; i + 16u <= n; i += 16u) { __builtin_memcpy(p + i, blanks, 16); }
      if (i + 8u <= n) {
        __builtin_memcpy(p + i, blanks, 8);
        i += 8u;
      }
      if (i + 4u <= n) { __builtin_memcpy(p + i, blanks, 4); }
      at += n;
    } else {
      for (u32 i = 0; i < n; i++) { put(' '); }
    }
  }
  __device__ __forceinline__ void put_literal(u32 t) { // t, f, n
    if (t == 't') {
      put('t'); put('r'); put('u'); put('e');
    } else if (t == 'f') {
      put('f'); put('a'); put('l'); put('s'); put('e');
    } else {
      put('n'); put('u'); put('l'); put('l');
    }
  }
  // l, u or d with the value word v (a finite double)
  __device__ __forceinline__ void put_number(u32 t, u64 v) {
    u32 length = 0;
    const bool fits = FILL && at + DTOA_MAX_BYTES <= room; // (24 >= the 20 of an integer)
    if (!fits) { length = t == 'd' ? dtoa_length(v) : t == 'l' ? int64_text_length(v) : decimal_digits(v); }
    if (FILL && (fits || at + length <= room)) {
      u8 *p = out + at;
      if (t == 'd') {
        length = dtoa_write(v, p);
      } else if (t == 'l') {
        length = int64_text_write(v, p);
      } else {
        length = decimal_digits(v);
        write_decimal(p, v, length);
      }
    }
    at += length;
  }
  __device__ __forceinline__ void put_string(const u8 *s, u32 len) {
    if (FILL) {
      at += escape_write(s, len, out + (at < room ? at : room), at < room ? room - at : 0u);
    } else {
      at += escaped_length(s, len);
    }
  }
};

// The text of the container whose opening word is tape[low] and whose closing word is tape[high - 1] (k_rows_locate found both inside the document that begins at
// `base`, and the opening word to say so).  -> true with the length in sink.at; false: the sub-tape is not well formed (only !FILL decides that in full -- the fill
// runs behind a count that said true, keeps every bound and stops at the sink's room)
// PRETTY: with l = (the containers open around a word) mod 16, a child of a container lies behind "\n" and 4 l blanks, a , in front of them from the second child on;
// a value follows its key's ": "; a container that has children closes behind "\n" and its own 4 l blanks.  A container with l = 15 is FLAT -- the reference leaves its
// loop there and starts afresh for every child --: no newline and no blank inside it, its children have l = 0 again, and each of them, like the root, ends with "\n"
template <bool FILL, bool PRETTY = false>
__device__ __forceinline__ bool walk_cell(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 low, u64 high, u64 base, u64 str_base, u64 str_end, u64 *strip,
                                          json_sink<FILL> &sink) {
  level_bits levels = {0, strip};
  u32 depth = 0, need = 0; // need: 0 nothing, 1 a comma, 2 a colon in front of the next word's text
  bool in_object = false, key_next = false;
  u64 i = low;
  while (i < high) {
    const u64 w = tape[i];
    const u32 t = u32(w >> 56);
    if (t == '}' || t == ']') {
      if (depth == 0 || in_object != (t == '}') || (in_object && !key_next)) { return false; } // nothing open, the other kind, or a key without its value
      if (!FILL) {
        const u64 o = base + (w & LOW32);
        if (o < low || o >= i) { return false; }
        const u64 ow = tape[o];
        if (u32(ow >> 56) != (in_object ? u32('{') : u32('[')) || base + (ow & LOW32) != i + 1u) { return false; }
      }
      depth--;
      if (PRETTY && need != 0 && (depth & 15u) != 15u) { // (need == 0: the word in front opened it)
        sink.put('\n');
        sink.put_spaces(4u * (depth & 15u));
      }
      sink.put(t);
      if (PRETTY && (depth & 15u) == 0) { sink.put('\n'); }
      i++;
      if (depth == 0) { return i == high; }
      in_object = levels.get(depth - 1u);
      key_next = in_object;
      need = 1;
      continue;
    }
    if (depth == 0 && i != low) { return false; }
    const bool is_key = key_next;
    if (is_key && t != '"') { return false; }
    if (need == 1) { sink.put(','); }
    if (need == 2) { sink.put(':'); }
    const bool restart = PRETTY && (depth & 15u) == 0; // the root, or a child of a flat container
    if (PRETTY && depth != 0 && !restart) {
      if (need == 2) {
        sink.put(' ');
      } else {
        sink.put('\n');
        sink.put_spaces(4u * (depth & 15u));
      }
    }
    if (t == '{' || t == '[') {
      if (depth >= JSON_MAX_LEVELS) { return false; }
      in_object = t == '{';
      levels.set(depth, in_object);
      depth++;
      sink.put(t);
      key_next = in_object;
      need = 0;
      i++;
      continue;
    }
    if (depth == 0) { return false; } // (a cell's sub-tape begins with an opening word)
    if (t == '"') {
      const u64 rec = str_base + (w & PAYLOAD);
      if (rec + 4u > str_end) { return false; }
      const u32 len = *reinterpret_cast<const u32_unaligned *>(sbuf + rec);
      if (rec + 4u + u64(len) > str_end) { return false; }
      sink.put_string(sbuf + rec + 4u, len);
      i++;
    } else if (t == 'l' || t == 'u' || t == 'd') {
      if (i + 1u >= high) { return false; }
      const u64 v = tape[i + 1u];
      if (t == 'd' && !dtoa_is_finite(v)) { return false; }
      sink.put_number(t, v);
      i += 2u;
    } else if (t == 't' || t == 'f' || t == 'n') {
      sink.put_literal(t);
      i++;
    } else {
      return false;
    }
    if (PRETTY && restart && !is_key) { sink.put('\n'); }
    need = is_key ? 2u : 1u;
    key_next = in_object && !is_key;
  }
  return false; // the cell's words ran out with a container open
}

// the text of root r: a scalar from the cell itself, a located container from its sub-tape.  -> its status; the length in sink.at (0 with a status)
// (PRETTY: every served text ends with "\n")
template <bool FILL, bool PRETTY = false>
__device__ __forceinline__ u32 serialize_root(const u64 *__restrict__ tape, const u8 *__restrict__ sbuf, u64 string_bytes, const doc_span_dev *__restrict__ table, u32 m, u32 t, u64 v,
                                              u64 *strip, json_sink<FILL> &sink) {
  bool ok = true;
  if (m > ROWS_SPECIAL) {
    return rows_code(m);
  } else if (m == ROWS_SPECIAL) {
    if (t == '"') {
      const u64 at = v & LOW32, len = v >> 32;
      ok = at + len <= string_bytes;
      if (ok) { sink.put_string(sbuf + at, u32(len)); }
    } else if (t == 'l' || t == 'u' || t == 'd') {
      ok = t != 'd' || dtoa_is_finite(v);
      if (ok) { sink.put_number(t, v); }
    } else {
      sink.put_literal(t);
    }
    if (PRETTY && ok) { sink.put('\n'); }
  } else {
    const uint4 a = *reinterpret_cast<const uint4 *>(table + m), b = *reinterpret_cast<const uint4 *>(table + m + 1u);
    const u64 base = a.z, doc_end = b.z, str_base = a.w, str_end = b.w;
    const u64 low = v & LOW32, high = v >> 32;
    ok = high <= doc_end && walk_cell<FILL, PRETTY>(tape, sbuf, low, high, base, str_base, str_end, strip, sink);
  }
  if (!ok) {
    sink.at = 0;
    return QUERY_NO_SUCH_FIELD;
  }
  return 0;
}

} // namespace
} // namespace sjgpu
#endif
