// tests/golden/fields_golden.cpp -- asks the REAL reference for the fields of every element e of doc.at_path_with_wildcard(p): e.get_object() and
// `for (dom::key_value_pair f : object)`, and for the size() of e's container; and for dom::array::size() of three arrays around the saturation of the tape's
// count field.  Built and run by tests/golden/make_fields_golden.py only (against the reference's public headers and oracle/_ref/libsjref.so); its binary
// is never committed.
// stdin:  [u32 documents][u32 row paths] then every document and row path as [u32 length][bytes]
// stdout: per document and row path one line
//   R E <code> | R <rows>     doc.at_path_with_wildcard(row path) failed, or found that many elements
// and behind `R <rows>` one line per row:
//   <size> E <code>                     e.get_object() failed with that simdjson::error_code
//   <size> F;<key>:<value>;<key>:...    its fields in iteration order (F alone: none): the key's bytes as hex, the value as tests/golden/paths_golden.cpp renders
//                                       a match (l|u|d <bits>, t, f, n, s <hex>, { <words>, [ <words>)
//   <size>: dom::object(e).size() / dom::array(e).size() for an object / array row, 17 for a scalar row
// then three lines `A <elements> <size>`: dom::array::size() of [1,1,...] with 0xFFFFFE, 0xFFFFFF and 0x1000000 elements, built in memory.
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace simdjson;

static bool read_u32(uint32_t *v) { return fread(v, 4, 1, stdin) == 1; }
static bool read_blob(std::string *s) {
  uint32_t n;
  if (!read_u32(&n)) { return false; }
  s->resize(n);
  return n == 0 || fread(&(*s)[0], 1, n, stdin) == n;
}

// the tape words an element takes: a number two, a container its brackets and what lies between (a key is one word), everything else one
static uint64_t words(dom::element e) {
  switch (e.type()) {
    case dom::element_type::ARRAY: {
      uint64_t n = 2;
      for (dom::element child : dom::array(e)) { n += words(child); }
      return n;
    }
    case dom::element_type::OBJECT: {
      uint64_t n = 2;
      for (dom::key_value_pair field : dom::object(e)) { n += 1 + words(field.value); }
      return n;
    }
    case dom::element_type::INT64:
    case dom::element_type::UINT64:
    case dom::element_type::DOUBLE:
      return 2;
    default:
      return 1;
  }
}

static bool render(dom::element e) {
  switch (e.type()) {
    case dom::element_type::ARRAY: printf("[ %llu", (unsigned long long)words(e)); break;
    case dom::element_type::OBJECT: printf("{ %llu", (unsigned long long)words(e)); break;
    case dom::element_type::INT64: { int64_t v = int64_t(e); uint64_t b; memcpy(&b, &v, 8); printf("l %llu", (unsigned long long)b); break; }
    case dom::element_type::UINT64: printf("u %llu", (unsigned long long)uint64_t(e)); break;
    case dom::element_type::DOUBLE: { double v = double(e); uint64_t b; memcpy(&b, &v, 8); printf("d %llu", (unsigned long long)b); break; }
    case dom::element_type::STRING: {
      std::string_view s = std::string_view(e);
      printf("s ");
      for (unsigned char c : s) { printf("%02x", c); }
      break;
    }
    case dom::element_type::BOOL: printf(bool(e) ? "t" : "f"); break;
    case dom::element_type::NULL_VALUE: printf("n"); break;
    default: fprintf(stderr, "an element type this fixture does not cover\n"); return false;
  }
  return true;
}

int main() {
  uint32_t ndocs, nrows;
  if (!read_u32(&ndocs) || !read_u32(&nrows)) { return 2; }
  std::vector<std::string> docs(ndocs), row_paths(nrows);
  for (std::string &d : docs) { if (!read_blob(&d)) { return 2; } }
  for (std::string &p : row_paths) { if (!read_blob(&p)) { return 2; } }
  dom::parser parser;
  for (const std::string &d : docs) {
    dom::element root;
    const error_code pe = parser.parse(padded_string(d)).get(root);
    if (pe) { fprintf(stderr, "the reference rejects a document (%d): %s\n", int(pe), d.c_str()); return 1; }
    for (const std::string &rp : row_paths) {
      std::vector<dom::element> rows;
      const error_code re = root.at_path_with_wildcard(std::string_view(rp.data(), rp.size())).get(rows);
      if (re) { printf("R E %d\n", int(re)); continue; }
      printf("R %zu\n", rows.size());
      for (dom::element e : rows) {
        dom::object obj;
        const error_code oe = e.get_object().get(obj);
        size_t size = 17;
        if (!oe) {
          size = obj.size();
        } else if (e.type() == dom::element_type::ARRAY) {
          size = dom::array(e).size();
        }
        printf("%zu ", size);
        if (oe) { printf("E %d\n", int(oe)); continue; }
        printf("F");
        for (dom::key_value_pair f : obj) {
          printf(";");
          for (unsigned char c : f.key) { printf("%02x", c); }
          printf(":");
          if (!render(f.value)) { return 1; }
        }
        printf("\n");
      }
    }
  }
  for (size_t n : {size_t(0xFFFFFE), size_t(0xFFFFFF), size_t(0x1000000)}) {
    std::string big;
    big.reserve(2 * n + 2);
    big += '[';
    for (size_t i = 0; i < n; i++) { big += i ? ",1" : "1"; }
    big += ']';
    dom::parser large;
    dom::array a;
    const error_code e = large.parse(padded_string(big)).get_array().get(a);
    if (e) { fprintf(stderr, "the reference rejects the array of %zu elements (%d)\n", n, int(e)); return 1; }
    printf("A %zu %zu\n", n, a.size());
  }
  return 0;
}
