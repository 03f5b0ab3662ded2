// tests/golden/nested_write_golden.cpp -- asks the REAL reference for the nested JSON of a table whose fields may be LISTS: simdjson::builder::string_builder's
// append_key_value(key, std::vector<std::optional<T>>) for a list, a std::optional<std::vector<...>> that holds nothing for an invalid list, start_array() /
// append() / append_comma() / end_array() for a row that is an array, append() alone for a bare value, and -- for JSON texts, which the builder takes as they are --
// append_raw() between a start_array() and an end_array() of our own.  The yardstick of sjgpu_write_nested_device (include/sjgpu_nested.h).  What the builder leaves
// to its user is done here as a user does it: the comma between two fields, leaving a field that holds nothing out, the line feed behind a record -- and, under
// BARE with OMIT_NULLS, appending nothing at all for a value that holds nothing (that rule is ours: such a row is empty, without its line feed).
// Built and run by tests/golden/make_nested_write_golden.py only (-std=c++20, against the reference's public headers and oracle/_ref/libsjref.so); its binary is
// never committed.
// stdin:  [u32 tables] then per table [u32 rows][u32 fields], per field [u32 key length][key][u32 kind][u8 list], then row by row, field by field: a plain
//         field's cell [u8 valid] + its payload, a list field's list [u8 valid] and, when valid, [u32 elements] + as many cells.  A cell's payload, when valid:
//         [u64 bits] (kinds 1 .. 4: int64, uint64, double, bool) or [u32 length][bytes] (5, 9: a string; 8: a JSON text)
// stdout: per table and per legal flags (1 leave nulls out, 2 a line feed, 4 array rows, 8 bare rows)  T <table> <flags>  then one line per row: its text as hex
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <string_view>
#include <vector>

using simdjson::builder::string_builder;

struct cell {
  bool valid = false;
  uint64_t bits = 0;
  std::string bytes;
};
struct value { // a plain field's cell, or a list
  cell one;
  bool list_valid = false;
  std::vector<cell> elements;
};
struct field {
  std::string key;
  uint32_t kind = 0;
  bool list = false;
};

static bool read_exact(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
static bool read_u32(uint32_t *v) { return read_exact(v, 4); }
static bool read_blob(std::string *s) {
  uint32_t n;
  if (!read_u32(&n)) { return false; }
  s->resize(n);
  return read_exact(&(*s)[0], n);
}
static bool read_cell(uint32_t kind, cell *c) {
  uint8_t valid;
  if (!read_exact(&valid, 1)) { return false; }
  c->valid = valid != 0;
  if (!c->valid) { return true; }
  return kind <= 4 ? read_exact(&c->bits, 8) : read_blob(&c->bytes);
}

static bool holds(uint32_t kind, const cell &c) { return c.valid && !(kind == 8 && c.bytes.empty()); } // an empty JSON text is no value

// X through the builder: behind its key in an object, alone in an array or as a bare row
template <class X>
static void put(string_builder &b, bool keyed, std::string_view key, const X &x) {
  if (keyed) {
    b.append_key_value(key, x);
  } else {
    b.append(x);
  }
}

template <class T, class MAKE>
static void put_list(string_builder &b, bool keyed, std::string_view key, const value &v, MAKE make) {
  if (!v.list_valid) {
    put(b, keyed, key, std::optional<std::vector<std::optional<T>>>{});
    return;
  }
  std::vector<std::optional<T>> list;
  for (const cell &c : v.elements) { list.push_back(c.valid ? std::optional<T>(make(c)) : std::optional<T>{}); }
  put(b, keyed, key, list);
}

static void put_value(string_builder &b, bool keyed, const field &f, const value &v) {
  const std::string_view key(f.key.data(), f.key.size());
  if (!f.list) {
    const cell &c = v.one;
    if (!holds(f.kind, c)) {
      if (keyed) { b.append_key_value(key, nullptr); } else { b.append_null(); }
    } else if (f.kind == 1) {
      int64_t x;
      memcpy(&x, &c.bits, 8);
      put(b, keyed, key, x);
    } else if (f.kind == 2) {
      put(b, keyed, key, uint64_t(c.bits));
    } else if (f.kind == 3) {
      double x;
      memcpy(&x, &c.bits, 8);
      put(b, keyed, key, x);
    } else if (f.kind == 4) {
      put(b, keyed, key, c.bits != 0);
    } else if (f.kind == 8) {
      if (keyed) { b.escape_and_append_with_quotes(key); b.append_colon(); }
      b.append_raw(std::string_view(c.bytes.data(), c.bytes.size()));
    } else {
      put(b, keyed, key, std::string_view(c.bytes.data(), c.bytes.size()));
    }
    return;
  }
  if (f.kind == 1) {
    put_list<int64_t>(b, keyed, key, v, [](const cell &c) { int64_t x; memcpy(&x, &c.bits, 8); return x; });
  } else if (f.kind == 2) {
    put_list<uint64_t>(b, keyed, key, v, [](const cell &c) { return uint64_t(c.bits); });
  } else if (f.kind == 3) {
    put_list<double>(b, keyed, key, v, [](const cell &c) { double x; memcpy(&x, &c.bits, 8); return x; });
  } else if (f.kind == 4) {
    put_list<bool>(b, keyed, key, v, [](const cell &c) { return c.bits != 0; });
  } else if (f.kind == 8) { // raw JSON elements: the array is ours, the elements go in as they are
    if (keyed) { b.escape_and_append_with_quotes(key); b.append_colon(); }
    if (!v.list_valid) {
      b.append_null();
      return;
    }
    b.start_array();
    for (size_t i = 0; i < v.elements.size(); i++) {
      if (i) { b.append_comma(); }
      const cell &c = v.elements[i];
      if (holds(8, c)) {
        b.append_raw(std::string_view(c.bytes.data(), c.bytes.size()));
      } else {
        b.append_null();
      }
    }
    b.end_array();
  } else {
    put_list<std::string_view>(b, keyed, key, v, [](const cell &c) { return std::string_view(c.bytes.data(), c.bytes.size()); });
  }
}

int main() {
  uint32_t tables;
  if (!read_u32(&tables)) { return 2; }
  for (uint32_t t = 0; t < tables; t++) {
    uint32_t rows, K;
    if (!read_u32(&rows) || !read_u32(&K)) { return 2; }
    std::vector<field> fields(K);
    for (field &f : fields) {
      uint8_t list;
      if (!read_blob(&f.key) || !read_u32(&f.kind) || !read_exact(&list, 1)) { return 2; }
      f.list = list != 0;
    }
    std::vector<value> values(size_t(rows) * K);
    for (uint32_t r = 0; r < rows; r++) {
      for (uint32_t k = 0; k < K; k++) {
        value &v = values[size_t(r) * K + k];
        if (!fields[k].list) {
          if (!read_cell(fields[k].kind, &v.one)) { return 2; }
          continue;
        }
        uint8_t valid;
        uint32_t m;
        if (!read_exact(&valid, 1)) { return 2; }
        v.list_valid = valid != 0;
        if (!v.list_valid) { continue; }
        if (!read_u32(&m)) { return 2; }
        v.elements.resize(m);
        for (cell &c : v.elements) { if (!read_cell(fields[k].kind, &c)) { return 2; } }
      }
    }
    for (uint32_t flags = 0; flags < 16; flags++) {
      const bool omit = flags & 1u, newline = flags & 2u, array = flags & 4u, bare = flags & 8u;
      if ((array && (omit || bare)) || (bare && K != 1)) { continue; }
      printf("T %u %u\n", t, flags);
      for (uint32_t r = 0; r < rows; r++) {
        string_builder b;
        if (array) { b.start_array(); } else if (!bare) { b.start_object(); }
        bool first = true;
        for (uint32_t k = 0; k < K; k++) {
          const value &v = values[size_t(r) * K + k];
          const bool something = fields[k].list ? v.list_valid : holds(fields[k].kind, v.one);
          if (!something && omit) { continue; }
          if (!first) { b.append_comma(); }
          first = false;
          put_value(b, !array && !bare, fields[k], v);
        }
        if (array) { b.end_array(); } else if (!bare) { b.end_object(); }
        if (newline && !(bare && first)) { b.append('\n'); }
        std::string_view text;
        if (b.view().get(text)) { fprintf(stderr, "the builder ran out of memory\n"); return 1; }
        for (unsigned char ch : text) { printf("%02x", ch); }
        printf("\n");
      }
    }
  }
  return 0;
}
