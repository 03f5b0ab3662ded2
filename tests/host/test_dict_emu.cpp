// tests/host/test_dict_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_dict.hip (compiled as C++ against tests/host/emu, with the scans of sjgpu_finish.hip) run the
// launch sequences of sjgpu_dictionary_encode_device and sjgpu_cell_kinds_by_code_device (include/sjgpu_dict.h) -- the memsets, the insert, the heads, the scan, the
// codes, the fill; the memset and the census -- over rows of cells and a string buffer the test made.  What the C-ABI decides from the eight bytes it read back
// (SJGPU_E_INTERNAL, SJGPU_E_OVERFLOW: no fill) is decided here the same way.  tests/test_dict_emu.py compares what comes out with tests/dictionary_model.py.
// stdin, one record per call:
//   [u64 string bytes][string buffer][u32 n][u8 tags[n]][u64 values[n]][u8 value-row tags[n]][u64 value-row values[n]]
//   [u32 capacity: 0 exact, 1 one short, 2 none and null outputs][u32 censuses][u32 groups[censuses]: 0xFFFFFFFF = as many as there are distinct strings]
// stdout, per record:
//   [i32 code: 0, -5 or -7][u64 distinct][i32 codes[n]][u32 first[written]][u64 dictionary values[written]][u8 dictionary tags[written]][u32 counts[written]]
//   then per census [u32 kinds[groups * 16]], written = distinct when the code is 0, else 0
// Every output and the workspace lie at their exact sizes between poisoned guards (the byte rows begin at odd addresses): a byte outside is exit code 1, and so
// is a dictionary slot of [0, distinct) or a code that was left unwritten.
#include "sjgpu.h"
#include "sjgpu_dict.h"
#include "sjgpu_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sjgpu;

constexpr size_t GUARD = 256;
constexpr uint8_t POISON = 0x5A;

struct guarded {
  std::vector<uint8_t> store;
  uint8_t *p = nullptr;
  size_t bytes = 0;
  // `bytes` at an address that is `align`-aligned plus `skew`, poison all around and inside
  void make(size_t n, size_t align, size_t skew = 0) {
    bytes = n;
    store.assign(n + 2 * GUARD + align + skew, POISON);
    uintptr_t a = reinterpret_cast<uintptr_t>(store.data()) + GUARD;
    a = (a + align - 1) / align * align + skew;
    p = reinterpret_cast<uint8_t *>(a);
  }
  bool intact() const {
    for (const uint8_t *q = store.data(); q < p; q++) { if (*q != POISON) { return false; } }
    for (const uint8_t *q = p + bytes; q < store.data() + store.size(); q++) { if (*q != POISON) { return false; } }
    return true;
  }
  bool untouched() const {
    for (uint8_t b : store) { if (b != POISON) { return false; } }
    return true;
  }
};

static bool read_exact(void *dst, size_t n) { return n == 0 || fread(dst, 1, n, stdin) == n; }

int main() {
  sj_emu::max_concurrent_workgroups = 4;
  unsigned long records = 0;
  for (;;) {
    uint64_t string_bytes;
    if (fread(&string_bytes, 8, 1, stdin) != 1) { break; }
    guarded sbuf, tag, value, vtag, vvalue;
    sbuf.make(string_bytes, 1, 3); // the strings begin at any byte
    uint32_t n, capacity, censuses;
    if (!read_exact(sbuf.p, sbuf.bytes) || !read_exact(&n, 4)) { return 2; }
    tag.make(n, 2, 1);
    value.make(size_t(n) * 8, 8);
    vtag.make(n, 2, 1);
    vvalue.make(size_t(n) * 8, 8);
    if (!read_exact(tag.p, tag.bytes) || !read_exact(value.p, value.bytes) || !read_exact(vtag.p, vtag.bytes) || !read_exact(vvalue.p, vvalue.bytes) ||
        !read_exact(&capacity, 4) || !read_exact(&censuses, 4)) {
      return 2;
    }
    std::vector<uint32_t> groups(censuses);
    if (!read_exact(groups.data(), size_t(censuses) * 4)) { return 2; }
    records++;
    guarded codes, ws;
    codes.make(size_t(n) * 4, 4);
    ws.make(n ? dict_workspace_bytes(n) : 0, 256);
    const uint64_t *value_p = reinterpret_cast<const uint64_t *>(value.p);
    int32_t *codes_p = reinterpret_cast<int32_t *>(codes.p);
    if (!dict_encode_args_ok(sbuf.p, string_bytes, value_p, tag.p, n, codes_p, nullptr, nullptr, nullptr, nullptr, 0)) {
      fprintf(stderr, "record %lu: the argument check refuses a good call\n", records);
      return 1;
    }
    dict_result_dev result = {0, 0};
    if (n) {
      const dict_result_dev *result_dev = nullptr;
      if (launch_dict_encode(value_p, tag.p, n, sbuf.p, string_bytes, codes_p, ws.p, nullptr, &result_dev) != hipSuccess) { return 1; }
      memcpy(&result, result_dev, sizeof result);
    }
    const uint64_t distinct = result.distinct;
    const uint64_t dict_cap = capacity == 0 ? distinct : capacity == 1 ? (distinct ? distinct - 1 : 0) : 0;
    const int32_t code = result.failed ? SJGPU_E_INTERNAL : distinct > dict_cap ? SJGPU_E_OVERFLOW : 0;
    guarded dict_value, dict_tag, dict_first, dict_count;
    dict_value.make(dict_cap * 8, 8);
    dict_tag.make(dict_cap, 2, 1);
    dict_first.make(dict_cap * 4, 4);
    dict_count.make(dict_cap * 4, 4);
    if (!code && distinct) {
      launch_dict_fill(value_p, n, ws.p, reinterpret_cast<uint64_t *>(dict_value.p), dict_tag.p, reinterpret_cast<uint32_t *>(dict_first.p),
                       reinterpret_cast<uint32_t *>(dict_count.p), nullptr);
    }
    std::vector<guarded> kinds(censuses);
    for (uint32_t c = 0; c < censuses; c++) {
      const uint32_t G = groups[c] == 0xFFFFFFFFu ? uint32_t(distinct) : groups[c];
      groups[c] = G;
      kinds[c].make(size_t(G) * 64, 4);
      uint32_t *kinds_p = G ? reinterpret_cast<uint32_t *>(kinds[c].p) : nullptr;
      if (!cell_kinds_by_code_args_ok(codes_p, vvalue.p, vtag.p, n, G, kinds_p)) { fprintf(stderr, "record %lu: the census refuses a good call\n", records); return 1; }
      if (launch_cell_kinds_by_code(codes_p, reinterpret_cast<const uint64_t *>(vvalue.p), vtag.p, n, G, kinds_p, nullptr) != hipSuccess) { return 1; }
      if (!kinds[c].intact()) { fprintf(stderr, "record %lu: the census wrote outside its counters\n", records); return 1; }
    }
    if (!codes.intact() || !ws.intact() || !sbuf.intact() || !tag.intact() || !value.intact() || !vtag.intact() || !vvalue.intact() || !dict_value.intact() ||
        !dict_tag.intact() || !dict_first.intact() || !dict_count.intact()) {
      fprintf(stderr, "record %lu: a kernel wrote outside its outputs\n", records);
      return 1;
    }
    if (code && (!dict_value.untouched() || !dict_tag.untouched() || !dict_first.untouched() || !dict_count.untouched())) {
      fprintf(stderr, "record %lu: the dictionary was written although it does not fit\n", records);
      return 1;
    }
    const uint64_t written = code ? 0 : distinct;
    for (uint64_t j = 0; j < written; j++) {
      if (dict_tag.p[j] != '"') { fprintf(stderr, "record %lu: dictionary slot %llu was not written\n", records, (unsigned long long)j); return 1; }
    }
    for (uint32_t i = 0; i < n; i++) {
      if (codes_p[i] == 0x5A5A5A5A) { fprintf(stderr, "record %lu: code %u was not written\n", records, i); return 1; }
    }
    fwrite(&code, 4, 1, stdout);
    fwrite(&distinct, 8, 1, stdout);
    fwrite(codes.p, 4, n, stdout);
    fwrite(dict_first.p, 4, written, stdout);
    fwrite(dict_value.p, 8, written, stdout);
    fwrite(dict_tag.p, 1, written, stdout);
    fwrite(dict_count.p, 4, written, stdout);
    for (uint32_t c = 0; c < censuses; c++) { fwrite(kinds[c].p, 4, size_t(groups[c]) * 16, stdout); }
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
