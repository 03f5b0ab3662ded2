// tests/golden/write_records_golden.cpp -- asks the REAL reference for the JSON records of a table of columns: per row simdjson::builder::string_builder's
// start_object(), append_key_value(key, value) per field with append_comma() between two fields, end_object() -- the yardstick of sjgpu_write_records_device
// (include/sjgpu_write.h).  What the builder leaves to its user is done here as a user does it: the comma between two fields, null for a cell that holds nothing
// (append_key_value(key, nullptr), which is append_null()), leaving such a field out instead, a JSON text taken as it is (the quoted key, append_colon(),
// append_raw()), and the line feed behind a record.  Built and run by tests/golden/make_write_records_golden.py only (against the reference's public headers and
// oracle/_ref/libsjref.so); its binary is never committed.
// stdin:  [u32 tables] then per table [u32 rows][u32 columns], per column [u32 key length][key][u32 kind], then row by row, column by column, one cell:
//         [u8 valid] and, when valid, [u64 bits] (kinds 1 .. 4: int64, uint64, double, bool) or [u32 length][bytes] (5, 9: a string; 8: a JSON text)
// stdout: per table and per flags 0 .. 3 (1: leave nulls out, 2: a line feed)  T <table> <flags>  then one line per row: its text as hex (never empty)
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

using simdjson::builder::string_builder;

struct cell {
  bool valid;
  uint64_t bits;
  std::string bytes;
};
struct column {
  std::string key;
  uint32_t kind;
};

static bool read_exact(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
static bool read_u32(uint32_t *v) { return read_exact(v, 4); }
static bool read_blob(std::string *s) {
  uint32_t n;
  if (!read_u32(&n)) { return false; }
  s->resize(n);
  return read_exact(&(*s)[0], n);
}

int main() {
  uint32_t tables;
  if (!read_u32(&tables)) { return 2; }
  for (uint32_t t = 0; t < tables; t++) {
    uint32_t rows, K;
    if (!read_u32(&rows) || !read_u32(&K)) { return 2; }
    std::vector<column> columns(K);
    for (column &c : columns) { if (!read_blob(&c.key) || !read_u32(&c.kind)) { return 2; } }
    std::vector<cell> cells(size_t(rows) * K);
    for (uint32_t r = 0; r < rows; r++) {
      for (uint32_t k = 0; k < K; k++) {
        cell &c = cells[size_t(r) * K + k];
        uint8_t valid;
        if (!read_exact(&valid, 1)) { return 2; }
        c.valid = valid != 0;
        c.bits = 0;
        if (!c.valid) { continue; }
        if (columns[k].kind <= 4) {
          if (!read_exact(&c.bits, 8)) { return 2; }
        } else if (!read_blob(&c.bytes)) {
          return 2;
        }
      }
    }
    for (uint32_t flags = 0; flags < 4; flags++) {
      printf("T %u %u\n", t, flags);
      for (uint32_t r = 0; r < rows; r++) {
        string_builder b;
        b.start_object();
        bool first = true;
        for (uint32_t k = 0; k < K; k++) {
          const cell &c = cells[size_t(r) * K + k];
          const std::string_view key(columns[k].key.data(), columns[k].key.size());
          const uint32_t kind = columns[k].kind;
          const bool holds = c.valid && !(kind == 8 && c.bytes.empty()); // an empty JSON text is no value
          if (!holds && (flags & 1u)) { continue; }
          if (!first) { b.append_comma(); }
          first = false;
          if (!holds) {
            b.append_key_value(key, nullptr);
          } else if (kind == 1) {
            int64_t v;
            memcpy(&v, &c.bits, 8);
            b.append_key_value(key, v);
          } else if (kind == 2) {
            b.append_key_value(key, uint64_t(c.bits));
          } else if (kind == 3) {
            double v;
            memcpy(&v, &c.bits, 8);
            b.append_key_value(key, v);
          } else if (kind == 4) {
            b.append_key_value(key, c.bits != 0);
          } else if (kind == 8) {
            b.escape_and_append_with_quotes(key);
            b.append_colon();
            b.append_raw(std::string_view(c.bytes.data(), c.bytes.size()));
          } else {
            b.append_key_value(key, std::string_view(c.bytes.data(), c.bytes.size()));
          }
        }
        b.end_object();
        if (flags & 2u) { b.append('\n'); }
        std::string_view text;
        if (b.view().get(text)) { fprintf(stderr, "the builder ran out of memory\n"); return 1; }
        for (unsigned char ch : text) { printf("%02x", ch); }
        printf("\n");
      }
    }
  }
  return 0;
}
