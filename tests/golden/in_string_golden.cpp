// tests/golden/in_string_golden.cpp -- asks the REAL reference what the getters for numbers held in strings give: for every content c it is handed,
// On-Demand parses `["c"]` and the array's one element answers get_int64_in_string(), get_uint64_in_string() and get_double_in_string().
// Built and run by tests/golden/make_in_string_golden.py only (against the reference's public headers and oracle/_ref/libsjref.so); its
// binary is never committed.
// stdin:  [u32 contents] then every content as [u32 length][bytes] (its own raw JSON form: the generator checks that)
// stdout: per content one line of three answers joined by `;`, in the order int64, uint64, double:
//   E <code>   the getter failed with that simdjson::error_code        <16 hex>   the 64 bits of the int64 / uint64 / double
//   a line `P <code>` where the document itself is refused (the generator accepts none)
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace simdjson;

static bool read_u32(uint32_t *v) { return fread(v, 4, 1, stdin) == 1; }

template <class T> static void bits(simdjson_result<T> r) {
  T v;
  const error_code e = std::move(r).get(v);
  if (e) { printf("E %d", int(e)); return; }
  uint64_t b = 0;
  memcpy(&b, &v, sizeof v);
  printf("%016llx", (unsigned long long)b);
}

// the array's first element of a fresh iteration: a value is consumed by the getter that succeeds
template <class F> static bool ask(ondemand::parser &parser, const padded_string &json, F &&getter) {
  ondemand::document doc;
  if (const error_code e = parser.iterate(json).get(doc)) { printf("P %d", int(e)); return false; }
  ondemand::array arr;
  if (const error_code e = doc.get_array().get(arr)) { printf("P %d", int(e)); return false; }
  for (auto element : arr) {
    ondemand::value v;
    if (const error_code e = element.get(v)) { printf("P %d", int(e)); return false; }
    getter(v);
    return true;
  }
  printf("P -1");
  return false;
}

int main() {
  uint32_t n;
  if (!read_u32(&n)) { return 2; }
  ondemand::parser parser;
  for (uint32_t k = 0; k < n; k++) {
    uint32_t len;
    if (!read_u32(&len)) { return 2; }
    std::string c(len, '\0');
    if (len && fread(&c[0], 1, len, stdin) != len) { return 2; }
    const padded_string json("[\"" + c + "\"]");
    if (ask(parser, json, [](ondemand::value &v) { bits(v.get_int64_in_string()); })) {
      printf(";");
      ask(parser, json, [](ondemand::value &v) { bits(v.get_uint64_in_string()); });
      printf(";");
      ask(parser, json, [](ondemand::value &v) { bits(v.get_double_in_string()); });
    }
    printf("\n");
  }
  return 0;
}
