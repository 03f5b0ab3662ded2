// tests/host/test_pivot_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_pivot.hip (compiled as C++ against tests/host/emu) run the launch sequence of
// sjgpu_pivot_fields_device (include/sjgpu_pivot.h) -- the argument check, the fill, the scatter -- over fields the test made.  tests/test_pivot_emu.py compares
// what comes out with tests/pivot_model.py.
// stdin, one record per call:
//   [u32 rows][u32 fields][u32 groups][u32 columns][u32 has_map][u32 skew: 1 = the output words begin 8 bytes past a 16-byte address]
//   [u32 offsets[rows + 1]][u8 status[rows]][i32 codes[fields]][u64 values[fields]][u8 tags[fields]][i32 map[groups] when has_map]
// stdout, per record: [i32 code: 0 or -4][u8 tags[columns * rows]][u64 values[columns * rows]]
// The inputs lie in heap blocks of exactly their size (the sanitizer build sees a read one byte outside), the outputs at exactly columns * rows cells between
// poisoned guards, the tag row at an odd address.  A byte outside, a cell left unwritten where the call answered 0, an input that changed, or a second run that
// gives other bytes is exit code 1.  Before the first record the argument check is asked the refusals of the header.
#include "sjgpu.h"
#include "sjgpu_pivot.h"
#include "sjgpu_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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
};

// an input at its exact size on the heap, and a copy to compare it with afterwards
template <class T> struct exact {
  std::unique_ptr<T[]> mem;
  std::vector<T> copy;
  bool read(size_t n) {
    mem.reset(new T[n]);
    copy.resize(n);
    if (n && fread(mem.get(), sizeof(T), n, stdin) != n) { return false; }
    if (n) { memcpy(copy.data(), mem.get(), n * sizeof(T)); }
    return true;
  }
  const T *get() const { return copy.empty() ? nullptr : mem.get(); } // (nothing to read: the call gets a null pointer)
  bool unchanged() const { return copy.empty() || memcmp(copy.data(), mem.get(), copy.size() * sizeof(T)) == 0; }
};

static bool refusals() {
  alignas(16) static uint64_t words[8];
  const void *a = words, *odd8 = reinterpret_cast<const uint8_t *>(words) + 4, *odd4 = reinterpret_cast<const uint8_t *>(words) + 2;
  void *out = words + 4;
  const auto ok = [&](const void *offsets, const void *status, uint32_t rows, const void *codes, const void *value, const void *tag, uint64_t fields, const void *map,
                      uint32_t groups, uint32_t columns, const void *value_out, const void *tag_out) {
    return pivot_args_ok(offsets, status, rows, codes, value, tag, fields, map, groups, columns, value_out, tag_out);
  };
  bool good = ok(a, a, 1, a, a, a, 1, a, 1, 1, out, out) && ok(a, a, 1, a, a, a, 1, nullptr, 0, 1, out, out) && ok(a, a, 1, nullptr, nullptr, nullptr, 0, nullptr, 3, 1, out, out) &&
              ok(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 7, nullptr, nullptr) && ok(nullptr, nullptr, 7, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr) &&
              ok(a, a, 0xFFFFFFF0u, a, a, a, 1, a, 1, 1, out, out) && ok(a, a, 0xFFFF, a, a, a, 0xFFFFFFFFull, a, 1, 0x10000, out, out);
  bool bad = ok(a, a, 0xFFFFFFF1u, a, a, a, 1, a, 1, 1, out, out) || ok(a, a, 0x10000, a, a, a, 1, a, 1, 0x10000, out, out) || ok(a, a, 1, a, odd8, a, 1, a, 1, 1, out, out) ||
             ok(a, a, 1, a, a, a, 1, a, 1, 1, odd8, out) || ok(odd4, a, 1, a, a, a, 1, a, 1, 1, out, out) || ok(a, a, 1, odd4, a, a, 1, a, 1, 1, out, out) ||
             ok(a, a, 1, a, a, a, 1, odd4, 1, 1, out, out) || ok(nullptr, a, 1, a, a, a, 1, a, 1, 1, out, out) || ok(a, nullptr, 1, a, a, a, 1, a, 1, 1, out, out) ||
             ok(a, a, 1, a, a, a, 1, a, 1, 1, nullptr, out) || ok(a, a, 1, a, a, a, 1, a, 1, 1, out, nullptr) || ok(a, a, 1, nullptr, a, a, 1, a, 1, 1, out, out) ||
             ok(a, a, 1, a, nullptr, a, 1, a, 1, 1, out, out) || ok(a, a, 1, a, a, nullptr, 1, a, 1, 1, out, out) || ok(a, a, 1, a, a, a, 1ull << 32, a, 1, 1, out, out) ||
             ok(a, a, 1, a, a, a, 1, a, 0, 1, out, out) || ok(nullptr, nullptr, 0, nullptr, a, a, 1, nullptr, 0, 0, nullptr, nullptr);
  return good && !bad;
}

int main() {
  sj_emu::max_concurrent_workgroups = 4;
  if (!refusals()) { fprintf(stderr, "the argument check disagrees with the header\n"); return 1; }
  unsigned long records = 0;
  for (;;) {
    uint32_t head[6];
    if (fread(head, 4, 6, stdin) != 6) { break; }
    const uint32_t rows = head[0], fields = head[1], groups = head[2], columns = head[3], has_map = head[4], skew = head[5];
    records++;
    exact<uint32_t> offsets;
    exact<uint8_t> status, tags;
    exact<int32_t> codes, map;
    exact<uint64_t> values;
    if (!offsets.read(size_t(rows) + 1) || !status.read(rows) || !codes.read(fields) || !values.read(fields) || !tags.read(fields) || !map.read(has_map ? groups : 0)) { return 2; }
    const size_t cells = size_t(columns) * rows;
    const int32_t *map_p = has_map ? map.mem.get() : nullptr;
    std::vector<uint8_t> first_tags;
    std::vector<uint64_t> first_values;
    int32_t code = 0;
    for (int run = 0; run < 2; run++) {
      guarded value_out, tag_out;
      value_out.make(cells * 8, 16, skew ? 8 : 0);
      tag_out.make(cells, 2, 1);
      uint64_t *value_out_p = reinterpret_cast<uint64_t *>(value_out.p);
      code = pivot_args_ok(offsets.mem.get(), status.mem.get(), rows, codes.get(), values.get(), tags.get(), fields, map_p, groups, columns, value_out_p, tag_out.p) ? 0 : SJGPU_E_BADARG;
      if (code) { fprintf(stderr, "record %lu: the argument check refuses a good call\n", records); return 1; }
      if (rows && columns) {
        launch_pivot_fields(offsets.mem.get(), status.mem.get(), rows, codes.get(), values.get(), tags.get(), fields, map_p, groups, columns, value_out_p, tag_out.p, nullptr);
      }
      if (!value_out.intact() || !tag_out.intact()) { fprintf(stderr, "record %lu: a kernel wrote outside its outputs\n", records); return 1; }
      if (!offsets.unchanged() || !status.unchanged() || !codes.unchanged() || !values.unchanged() || !tags.unchanged() || !map.unchanged()) {
        fprintf(stderr, "record %lu: an input was written\n", records);
        return 1;
      }
      for (size_t c = 0; c < cells; c++) {
        if (tag_out.p[c] == POISON || value_out_p[c] == 0x5A5A5A5A5A5A5A5Aull) { fprintf(stderr, "record %lu: cell %zu was not written\n", records, c); return 1; }
      }
      if (run == 0) {
        first_tags.assign(tag_out.p, tag_out.p + cells);
        first_values.assign(value_out_p, value_out_p + cells);
      } else if ((cells && memcmp(first_tags.data(), tag_out.p, cells)) || (cells && memcmp(first_values.data(), value_out_p, cells * 8))) {
        fprintf(stderr, "record %lu: two runs gave different bytes\n", records);
        return 1;
      }
    }
    fwrite(&code, 4, 1, stdout);
    fwrite(first_tags.data(), 1, cells, stdout);
    fwrite(first_values.data(), 8, cells, stdout);
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
