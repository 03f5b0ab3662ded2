// tests/golden/pivot_golden.cpp -- asks the REAL reference what element::at_key(k) and element::at_key_case_insensitive(k) answer for every record of a set and
// every key of a list (the yardstick of sjgpu_pivot_fields_device, include/sjgpu_pivot.h).  Built and run by tests/golden/make_pivot_golden.py only (against the
// reference's public headers and oracle/_ref/libsjref.so); its binary is never committed.
// stdin:  [u32 sets] then per set [u32 records][u32 keys] and every record (one JSON document) and key as [u32 length][bytes]
// stdout: per set, record and key two lines -- at_key, then at_key_case_insensitive --, each
//   E <code>     the simdjson::error_code of the answer
//   V <text>     simdjson::minify(element)
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
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

static void answer(simdjson_result<dom::element> r) {
  dom::element e;
  const error_code code = r.get(e);
  if (code) {
    printf("E %d\n", int(code));
    return;
  }
  const std::string text = simdjson::minify(e);
  printf("V %s\n", text.c_str());
}

int main() {
  uint32_t sets;
  if (!read_u32(&sets)) { return 2; }
  dom::parser parser;
  for (uint32_t s = 0; s < sets; s++) {
    uint32_t nrecords, nkeys;
    if (!read_u32(&nrecords) || !read_u32(&nkeys)) { return 2; }
    std::vector<std::string> records(nrecords), keys(nkeys);
    for (std::string &r : records) { if (!read_blob(&r)) { return 2; } }
    for (std::string &k : keys) { if (!read_blob(&k)) { return 2; } }
    for (const std::string &r : records) {
      dom::element root;
      const error_code pe = parser.parse(padded_string(r)).get(root);
      if (pe) { fprintf(stderr, "the reference rejects a record (%d): %s\n", int(pe), r.c_str()); return 1; }
      for (const std::string &k : keys) {
        const std::string_view key(k.data(), k.size());
        answer(root.at_key(key));
        answer(root.at_key_case_insensitive(key));
      }
    }
  }
  return 0;
}
