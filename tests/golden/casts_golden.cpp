// tests/golden/casts_golden.cpp -- asks the REAL reference what the typed getters give: parse(`[X]`).at_pointer(p).get_int64() and its six siblings, for
// every scalar or container X and every pointer p it is handed -- the element itself and results that failed on the way.
// Built and run by tests/golden/make_casts_golden.py only (against the reference's public headers and oracle/_ref/libsjref.so); its
// binary is never committed.
// stdin:  [u32 values][u32 pointers] then every value X and every pointer as [u32 length][bytes]
// stdout: per value one line `P <code>` when the reference rejects `[X]`, else per pointer one line of seven answers joined by `;`, in the order
//         get_int64, get_uint64, get_double, get_bool, get_string, get_array, get_object:
//   E <code>       the getter failed with that simdjson::error_code (a failed at_pointer forwards its own)
//   <16 hex>       the 64 bits of the int64 / uint64 / double; a bool is 1 or 0
//   S <hex>        a string's bytes
//   A <n> | O <n>  an array and its elements, an object and its fields
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace simdjson;

static bool read_u32(uint32_t *v) { return fread(v, 4, 1, stdin) == 1; }
static bool read_blob(std::string *s) {
  uint32_t n;
  if (!read_u32(&n)) { return false; }
  s->resize(n);
  return n == 0 || fread(&(*s)[0], 1, n, stdin) == n;
}

template <class T> static void bits(simdjson_result<T> r) {
  T v;
  const error_code e = std::move(r).get(v);
  if (e) { printf("E %d", int(e)); return; }
  uint64_t b = 0;
  memcpy(&b, &v, sizeof v);
  printf("%016llx", (unsigned long long)b);
}

int main() {
  uint32_t nvalues, npointers;
  if (!read_u32(&nvalues) || !read_u32(&npointers)) { return 2; }
  std::vector<std::string> values(nvalues), pointers(npointers);
  for (std::string &x : values) { if (!read_blob(&x)) { return 2; } }
  for (std::string &p : pointers) { if (!read_blob(&p)) { return 2; } }
  dom::parser parser;
  for (const std::string &x : values) {
    dom::element root;
    const error_code pe = parser.parse(padded_string("[" + x + "]")).get(root);
    if (pe) { printf("P %d\n", int(pe)); continue; }
    for (const std::string &p : pointers) {
      simdjson_result<dom::element> r = root.at_pointer(std::string_view(p.data(), p.size()));
      bits(r.get_int64());
      printf(";");
      bits(r.get_uint64());
      printf(";");
      bits(r.get_double());
      printf(";");
      {
        bool v;
        const error_code e = r.get_bool().get(v);
        if (e) { printf("E %d", int(e)); } else { printf("%016llx", v ? 1ull : 0ull); }
      }
      printf(";");
      {
        std::string_view v;
        const error_code e = r.get_string().get(v);
        if (e) { printf("E %d", int(e)); } else {
          printf("S ");
          for (unsigned char c : v) { printf("%02x", c); }
        }
      }
      printf(";");
      {
        dom::array v;
        const error_code e = r.get_array().get(v);
        if (e) { printf("E %d", int(e)); } else { printf("A %zu", v.size()); }
      }
      printf(";");
      {
        dom::object v;
        const error_code e = r.get_object().get(v);
        if (e) { printf("E %d", int(e)); } else { printf("O %zu", v.size()); }
      }
      printf("\n");
    }
  }
  return 0;
}
