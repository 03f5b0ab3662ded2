// tests/host/test_cast_strings_emu.cpp -- CPU tier: the KERNEL SOURCE sjgpu_cast_strings.hip (compiled as C++ against tests/host/emu) runs what
// sjgpu_cast_string_cells_device (include/sjgpu_cast_strings.h) enqueues -- the memset of the counters, k_cast_string_cells, k_cast_strings_exact -- over cells
// and a string buffer the test made, behind the argument check the C-ABI asks (sjgpu_internal.h: cast_string_cells_args_ok) and with its order: refused, K == 0,
// the launcher.  tests/test_cast_strings_emu.py compares what comes out with tests/in_string_model.py.
// stdin, one record per call:
//   [u32 n][u32 K][u32 in place: 0 / 1][u32 spoil][u64 string_bytes][u8 getters[K]][u8 tags[K * n]][u64 values[K * n]][u8 string buffer[string_bytes]]
//   spoil: 0 nothing; what the call is handed instead of a good argument -- 1 value null, 2 tag null, 3 counts null, 4 value_out null, 5 code_out null,
//   6 valid_out null, 7 getters null, 8 value + 4 bytes, 9 value_out + 4, 10 valid_out + 4, 11 counts + 2, 12 string buffer null
// stdout, per record: [i32 code] and, when it is 0 with K > 0:
//   [u64 value_out[K * n]][u8 code_out[K * n]][u64 valid_out[K * ceil(n / 64)]][u32 counts[K * 8]]
// Every array lies at its exact size between poisoned guards (the byte rows begin at odd addresses): a byte written outside, an input changed by a call that
// is not in place, or anything written by a refused call or a call with K == 0 is exit code 1.  The string buffer is a heap block of its own that ENDS with the
// buffer's last byte and begins at an odd address: built with -fsanitize=address, a byte read behind it stops the program.
#include "sjgpu.h"
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
    uint32_t n;
    if (fread(&n, 4, 1, stdin) != 1) { break; }
    uint32_t K, in_place, spoil;
    uint64_t string_bytes;
    if (!read_exact(&K, 4) || !read_exact(&in_place, 4) || !read_exact(&spoil, 4) || !read_exact(&string_bytes, 8)) { return 2; }
    records++;
    const size_t cells = size_t(K) * n, words = size_t(K) * ((size_t(n) + 63) / 64);
    std::vector<uint8_t> getters(K + 1);
    guarded value, tag, value_out, code_out, valid_out, counts;
    value.make(cells * 8, 8);
    tag.make(cells, 2, 1);
    if (!read_exact(getters.data(), K) || !read_exact(tag.p, cells) || !read_exact(value.p, cells * 8)) { return 2; }
    // one byte of slack in front (an odd address), none behind
    std::unique_ptr<uint8_t[]> block(new uint8_t[string_bytes + 1]);
    uint8_t *sbuf = block.get() + 1;
    if (!read_exact(sbuf, string_bytes)) { return 2; }
    const std::vector<uint8_t> tag_before(tag.p, tag.p + cells), value_before(value.p, value.p + cells * 8), sbuf_before(sbuf, sbuf + string_bytes);
    value_out.make(in_place ? 0 : cells * 8, 8);
    code_out.make(in_place ? 0 : cells, 2, 1);
    valid_out.make(words * 8, 8);
    counts.make(size_t(K) * 8 * 4, 4);
    const void *a_value = spoil == 1 ? nullptr : value.p + (spoil == 8 ? 4 : 0), *a_tag = spoil == 2 ? nullptr : tag.p;
    void *a_counts = spoil == 3 ? nullptr : counts.p + (spoil == 11 ? 2 : 0);
    void *a_value_out = spoil == 4 ? nullptr : (in_place ? value.p : value_out.p) + (spoil == 9 ? 4 : 0);
    void *a_code_out = spoil == 5 ? nullptr : (in_place ? tag.p : code_out.p);
    void *a_valid_out = spoil == 6 ? nullptr : valid_out.p + (spoil == 10 ? 4 : 0);
    const uint8_t *a_getters = spoil == 7 ? nullptr : getters.data();
    const void *a_sbuf = spoil == 12 ? nullptr : sbuf;

    int32_t code = 0;
    if (!cast_string_cells_args_ok(a_sbuf, string_bytes, a_value, a_tag, n, K, a_getters, a_value_out, a_code_out, a_valid_out, a_counts)) {
      code = SJGPU_E_BADARG;
    } else if (K) {
      if (launch_cast_string_cells(static_cast<const uint8_t *>(a_sbuf), string_bytes, static_cast<const uint64_t *>(a_value), static_cast<const uint8_t *>(a_tag), n, K, a_getters,
                                   static_cast<uint64_t *>(a_value_out), static_cast<uint8_t *>(a_code_out), static_cast<uint64_t *>(a_valid_out), static_cast<uint32_t *>(a_counts),
                                   nullptr) != hipSuccess) { return 2; }
    }
    if (!value.intact() || !tag.intact() || !value_out.intact() || !code_out.intact() || !valid_out.intact() || !counts.intact() ||
        memcmp(sbuf, sbuf_before.data(), string_bytes)) {
      fprintf(stderr, "record %lu: the call wrote outside its outputs\n", records);
      return 1;
    }
    if ((code || !K) && (!value_out.untouched() || !code_out.untouched() || !valid_out.untouched() || !counts.untouched() || memcmp(tag.p, tag_before.data(), cells) ||
                         memcmp(value.p, value_before.data(), cells * 8))) {
      fprintf(stderr, "record %lu: a call that was refused or had no rows wrote something\n", records);
      return 1;
    }
    if (!in_place && (memcmp(tag.p, tag_before.data(), cells) || memcmp(value.p, value_before.data(), cells * 8))) {
      fprintf(stderr, "record %lu: the call changed its input\n", records);
      return 1;
    }
    if (!code && n == 0 && (!value_out.untouched() || !code_out.untouched() || !valid_out.untouched())) {
      fprintf(stderr, "record %lu: rows without cells: only the counts are to be written\n", records);
      return 1;
    }
    fwrite(&code, 4, 1, stdout);
    if (!code && K) {
      fwrite(in_place ? value.p : value_out.p, 8, cells, stdout);
      fwrite(in_place ? tag.p : code_out.p, 1, cells, stdout);
      fwrite(valid_out.p, 8, words, stdout);
      fwrite(counts.p, 4, size_t(K) * 8, stdout);
    }
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
