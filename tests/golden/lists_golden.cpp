// tests/golden/lists_golden.cpp -- asks the REAL reference what e.at_path_with_wildcard(q) gives for every e of doc.at_path_with_wildcard(p), cell by cell.
// Built and run by tests/golden/make_lists_golden.py only (against the reference's public headers and oracle/_ref/libsjref.so); its
// binary is never committed.
// stdin:  [u32 documents][u32 row paths][u32 child paths] then every document, row path and child path as [u32 length][bytes]
// stdout: per document and row path one line
//   R E <code> | R <rows>     doc.at_path_with_wildcard(row path) failed, or found that many elements
// and behind `R <rows>`, per row and child path (rows outermost) one line rendered as tests/golden/paths_golden.cpp renders a cell:
//   E <code>            at_path_with_wildcard failed with that simdjson::error_code
//   M;<match>;<match>   its matches in the order of the vector it returned (M alone: none), each rendered as
//   l|u|d <bits>        a number: the 64 bits of the int64 / uint64 / double, in decimal
//   t | f | n
//   s <hex>             a string's bytes
//   { <words> | [ <words>   a container and the tape words it spans, both bracket words included
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
  uint32_t ndocs, nrows, npaths;
  if (!read_u32(&ndocs) || !read_u32(&nrows) || !read_u32(&npaths)) { return 2; }
  std::vector<std::string> docs(ndocs), row_paths(nrows), paths(npaths);
  for (std::string &d : docs) { if (!read_blob(&d)) { return 2; } }
  for (std::string &p : row_paths) { if (!read_blob(&p)) { return 2; } }
  for (std::string &p : paths) { if (!read_blob(&p)) { return 2; } }
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
        for (const std::string &p : paths) {
          std::vector<dom::element> found;
          const error_code ec = e.at_path_with_wildcard(std::string_view(p.data(), p.size())).get(found);
          if (ec) { printf("E %d\n", int(ec)); continue; }
          printf("M");
          for (dom::element h : found) {
            printf(";");
            if (!render(h)) { return 1; }
          }
          printf("\n");
        }
      }
    }
  }
  return 0;
}
