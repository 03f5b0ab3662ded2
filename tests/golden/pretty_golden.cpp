// tests/golden/pretty_golden.cpp -- asks the REAL reference for the indented JSON text of the elements of a column: the elements e of doc.at_path_with_wildcard(p),
// each as simdjson::prettify(e) -- the path $ stands for the document's root element.  Built and run by tests/golden/make_pretty_golden.py only (against the
// reference's public headers and oracle/_ref/libsjref.so); its binary is never committed.
// stdin:  [u32 documents] then every document as [u32 length][bytes]; [u32 cases] then every case as [u32 document][u32 length][path]
// stdout: per case    C E <code> | C <cells>   then one line per cell: its text as hex (a text is never empty)
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
#include <string>
#include <string_view>
#include <vector>

using namespace simdjson;

static bool read_u32(uint32_t *v) { return fread(v, 4, 1, stdin) == 1; }
static bool read_blob(std::string *s) {
  uint32_t n;
  if (!read_u32(&n)) { return false; }
  s->resize(n);
  return n == 0 || fread(&(*s)[0], 1, n, stdin) == n;
}

int main() {
  uint32_t ndocs, ncases;
  if (!read_u32(&ndocs)) { return 2; }
  std::vector<std::string> docs(ndocs);
  for (std::string &d : docs) { if (!read_blob(&d)) { return 2; } }
  if (!read_u32(&ncases)) { return 2; }
  dom::parser parser;
  for (uint32_t c = 0; c < ncases; c++) {
    uint32_t which;
    std::string path;
    if (!read_u32(&which) || !read_blob(&path) || which >= ndocs) { return 2; }
    dom::element root;
    const error_code pe = parser.parse(padded_string(docs[which])).get(root);
    if (pe) { fprintf(stderr, "the reference rejects document %u (%d)\n", which, int(pe)); return 1; }
    std::vector<dom::element> rows;
    if (path == "$") { // the document's root itself (at_path_with_wildcard answers a bare $ with INVALID_JSON_POINTER)
      rows.push_back(root);
    } else {
      const error_code re = root.at_path_with_wildcard(std::string_view(path.data(), path.size())).get(rows);
      if (re) { printf("C E %d\n", int(re)); continue; }
    }
    printf("C %zu\n", rows.size());
    for (dom::element e : rows) {
      const std::string text = simdjson::prettify(e);
      for (unsigned char ch : text) { printf("%02x", ch); }
      printf("\n");
    }
  }
  return 0;
}
