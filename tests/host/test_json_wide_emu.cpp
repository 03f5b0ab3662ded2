// tests/host/test_json_wide_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_json_wide.hip (compiled as C++ against tests/host/emu, with k_rows_locate and the total of
// sjgpu_query.hip, the scans of sjgpu_finish.hip and the narrow count of sjgpu_json.hip) run the launch sequence of sjgpu_serialize_cells_wide_device
// (include/sjgpu_json_wide.h) -- the table check, locate, the extents and their scan, the range space's size read back, the count, the total read back, the fill -- over a
// stream and a row of cells the test made.  What the C-ABI decides from the sixteen bytes it reads back (SJGPU_E_RANGE: the narrow count for the statuses alone;
// CAPACITY, SJGPU_E_OVERFLOW: no fill) is decided here the same way.  tests/test_json_wide_emu.py compares what comes out with tests/json_text_model.py.
// stdin and stdout: the records of tests/host/test_json_emu.cpp, byte for byte; a call refused with SJGPU_E_RANGE (-8) writes its offsets as it found them (poisoned).
// Every input, every output and both workspaces lie at their exact sizes between poisoned guards (the byte rows begin at odd addresses): a byte written outside is
// exit code 1, and so is an offset, a status or a character of [0, bytes) that was left unwritten where the poison can tell, characters written although they do not
// fit, or an offset written by a call that was refused for its range.
#include "sjgpu.h"
#include "sjgpu_json_wide.h"
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
    uint64_t tape_words, string_bytes;
    if (fread(&tape_words, 8, 1, stdin) != 1) { break; }
    guarded tape, sbuf, table, tag, value;
    tape.make(tape_words * 8, 8);
    if (!read_exact(tape.p, tape.bytes) || !read_exact(&string_bytes, 8)) { return 2; }
    sbuf.make(string_bytes, 1, 3); // the strings begin at any byte
    uint32_t docs, rows, capacity;
    if (!read_exact(sbuf.p, sbuf.bytes) || !read_exact(&docs, 4)) { return 2; }
    table.make((size_t(docs) + 1) * 16, 16);
    if (!read_exact(table.p, table.bytes) || !read_exact(&rows, 4)) { return 2; }
    tag.make(rows, 2, 1);
    value.make(size_t(rows) * 8, 8);
    if (!read_exact(tag.p, tag.bytes) || !read_exact(value.p, value.bytes) || !read_exact(&capacity, 4)) { return 2; }
    records++;
    const uint64_t *tape_p = reinterpret_cast<const uint64_t *>(tape.p), *value_p = reinterpret_cast<const uint64_t *>(value.p);
    const doc_span_dev *spans = reinterpret_cast<const doc_span_dev *>(table.p);
    guarded offsets, status, roots, words, bad, chars;
    offsets.make((size_t(rows) + 1) * 4, 4);
    status.make(rows, 2, 1);
    roots.make(rows ? json_wide_root_bytes(rows) : 0, 256);
    bad.make(4, 4);
    uint32_t *offsets_p = reinterpret_cast<uint32_t *>(offsets.p);
    int32_t code = 0;
    uint64_t bytes = 0, range_words = 0;
    memset(bad.p, 0, 4);
    launch_query_check_table(spans, docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(bad.p), nullptr);
    if (*reinterpret_cast<uint32_t *>(bad.p)) {
      code = SJGPU_E_BADARG;
    } else if (rows == 0) {
      offsets_p[0] = 0;
    } else {
      range_words = launch_json_wide_extents(tape_p, spans, docs, value_p, tag.p, rows, roots.p, nullptr)->total;
      if (range_words > 0xFFFFFFF0ull) {
        code = SJGPU_E_RANGE;
        const size_t narrow = (json_workspace_bytes(rows) + 255) & ~size_t(255);
        words.make(narrow + (size_t(rows) + 1) * 4, 256);
        (void)launch_json_count(tape_p, sbuf.p, string_bytes, spans, docs, value_p, tag.p, rows, json_wide_where(roots.p, rows), reinterpret_cast<uint32_t *>(words.p + narrow),
                                status.p, words.p, nullptr);
      } else {
        words.make(json_wide_word_bytes(rows, range_words), 256);
        const count_total_dev *total = nullptr;
        if (launch_json_wide_count(tape_p, sbuf.p, string_bytes, spans, value_p, tag.p, rows, range_words, offsets_p, status.p, roots.p, words.p, nullptr, &total) != hipSuccess) {
          return 3;
        }
        bytes = total->total;
      }
    }
    const uint64_t chars_cap = capacity == 0 ? bytes : capacity == 1 ? (bytes ? bytes - 1 : 0) : 0;
    chars.make(chars_cap, 2, 1);
    if (!code && bytes > 0xFFFFFFFFull) { code = 1; }
    if (!code && bytes > chars_cap) { code = SJGPU_E_OVERFLOW; }
    if (!code && bytes) {
      launch_json_wide_fill(tape_p, sbuf.p, string_bytes, spans, value_p, tag.p, rows, range_words, chars.p, roots.p, words.p, nullptr);
    }
    if (!tape.intact() || !sbuf.intact() || !table.intact() || !tag.intact() || !value.intact() || !offsets.intact() || !status.intact() || !roots.intact() || !words.intact() ||
        !chars.intact()) {
      fprintf(stderr, "record %lu: a kernel wrote outside its outputs\n", records);
      return 1;
    }
    if (code && !chars.untouched()) { fprintf(stderr, "record %lu: characters were written although they do not fit\n", records); return 1; }
    if (code == SJGPU_E_RANGE && !offsets.untouched()) { fprintf(stderr, "record %lu: offsets were written by a call refused for its range\n", records); return 1; }
    if (code != SJGPU_E_BADARG) {
      if (code != SJGPU_E_RANGE && (offsets_p[0] != 0 || offsets_p[rows] != uint32_t(bytes))) { fprintf(stderr, "record %lu: the offsets do not end at the total\n", records); return 1; }
      for (uint32_t r = 0; r < rows; r++) {
        if (status.p[r] == POISON) { fprintf(stderr, "record %lu: status %u was not written\n", records, r); return 1; }
        if (code != SJGPU_E_RANGE && offsets_p[r + 1] < offsets_p[r] && bytes <= 0xFFFFFFFFull) { fprintf(stderr, "record %lu: the offsets run backwards at %u\n", records, r); return 1; }
      }
    }
    const uint64_t written = code ? 0 : bytes;
    fwrite(&code, 4, 1, stdout);
    fwrite(&bytes, 8, 1, stdout);
    if (code == SJGPU_E_BADARG) { continue; }
    fwrite(offsets.p, 4, size_t(rows) + 1, stdout);
    fwrite(status.p, 1, rows, stdout);
    fwrite(chars.p, 1, written, stdout);
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
