// tests/host/test_paths_wide_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_query.hip (compiled as C++ against tests/host/emu, with the scans of
// sjgpu_finish.hip) run launch_paths_wide -- the whole level loop of sjgpu_at_paths_wide_device behind the table check: annotation, frontiers, read-backs,
// offsets, emission -- over tapes the oracle built on the CPU, and then the gather of include/sjgpu_query.h over the flattened column.  The paths are
// compiled by the host code the C-ABI uses (sj_path_program.h).  tests/test_paths_wide_emu.py compares what comes out with tests/path_model.py.
// stdin and stdout: those of tests/host/test_paths_emu.cpp, one record per stream:
//   [u32 docs][u64 tape words][u64 string bytes][tape][string records][table: docs + 1 entries of 16 bytes][u32 K][u32 lens[K]][the paths' bytes]
//   [u64 matches][u8 status[K * docs]][u32 offsets[K * docs + 1]][u8 tags[matches]][u64 values[matches]] then the gather over the matches:
//   [u64 total][u32 offsets[matches + 1]][u8 chars[total]]
// The loop runs twice per record, as a caller without a guess runs it: with room for nothing (the rows stay untouched, offsets and statuses are complete),
// then at the exact capacity.  Every output and the workspace lie at their exact size between poisoned guards (and the byte rows begin at an odd
// address): a byte outside is exit code 1.
#include "sjgpu.h"
#include "sjgpu_internal.h"
#include "sj_path_program.h"

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
};

static bool read_exact(void *dst, size_t n) { return n == 0 || fread(dst, 1, n, stdin) == n; }

int main() {
  sj_emu::max_concurrent_workgroups = 4;
  unsigned long records = 0;
  for (;;) {
    uint32_t docs;
    if (fread(&docs, 4, 1, stdin) != 1) { break; }
    uint64_t tape_words, string_bytes;
    if (!read_exact(&tape_words, 8) || !read_exact(&string_bytes, 8)) { return 2; }
    guarded tape, sbuf, table;
    tape.make(tape_words * 8, 8);
    sbuf.make(string_bytes, 1, 3); // the records begin at any byte
    table.make((size_t(docs) + 1) * 16, 16);
    if (!read_exact(tape.p, tape.bytes) || !read_exact(sbuf.p, sbuf.bytes) || !read_exact(table.p, table.bytes)) { return 2; }
    uint32_t K;
    if (!read_exact(&K, 4)) { return 2; }
    std::vector<uint32_t> lens(K);
    if (!read_exact(lens.data(), size_t(K) * 4)) { return 2; }
    size_t total_len = 0;
    for (uint32_t l : lens) { total_len += l; }
    std::vector<uint8_t> paths(total_len + 1);
    if (!read_exact(paths.data(), total_len)) { return 2; }
    records++;
    path_program prog;
    if (!compile_path_program(paths.data(), lens.data(), K, &prog)) { fprintf(stderr, "record %lu: the paths are beyond the limits\n", records); return 1; }
    guarded program, bad;
    program.make(prog.bytes.size(), 16);
    memcpy(program.p, prog.bytes.data(), prog.bytes.size());
    bad.make(4, 4);
    memset(bad.p, 0, 4);
    const size_t cells = size_t(K) * docs;
    const doc_span_dev *spans = reinterpret_cast<const doc_span_dev *>(table.p);
    const uint64_t *tape_words_p = reinterpret_cast<const uint64_t *>(tape.p);
    launch_query_check_table(spans, docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(bad.p), nullptr);
    if (*reinterpret_cast<uint32_t *>(bad.p)) { fprintf(stderr, "record %lu: the table check refuses a table the oracle's tapes were laid out by\n", records); return 1; }
    uint64_t matches = 0;
    guarded offsets, status, value, tag;
    for (int attempt = 0; attempt < 2; attempt++) { // room for nothing, then for exactly what the first run asked for
      const uint64_t cap = attempt ? matches : 0;
      guarded ws;
      offsets.make((cells + 1) * 4, 4);
      status.make(cells, 2, 1);
      value.make(cap * 8, 8);
      tag.make(cap, 2, 1);
      ws.make(K && docs ? paths_wide_workspace_bytes(K, docs, tape_words) : 0, 256);
      uint64_t found = 0;
      if (K && docs) {
        uint32_t readback = 0;
        const hipError_t e = launch_paths_wide(tape_words_p, tape_words, sbuf.p, spans, docs, program.p, prog.bytes.data(), prog.levels_at, prog.tokens_at, prog.keys_at, K,
                                               reinterpret_cast<uint32_t *>(offsets.p), status.p, reinterpret_cast<uint64_t *>(value.p), tag.p, cap, ws.p, &readback, nullptr, &found);
        if (e != hipSuccess) { fprintf(stderr, "record %lu: launch_paths_wide failed\n", records); return 1; }
      } else {
        memset(offsets.p, 0, 4);
      }
      if (!value.intact() || !tag.intact() || !offsets.intact() || !status.intact() || !ws.intact() || !tape.intact() || !sbuf.intact() || !table.intact() || !program.intact() ||
          !bad.intact()) {
        fprintf(stderr, "record %lu: the wide call wrote outside its outputs (capacity %llu)\n", records, (unsigned long long)cap);
        return 1;
      }
      if (attempt == 0) {
        matches = found;
      } else if (found != matches) {
        fprintf(stderr, "record %lu: the second run found %llu matches, the first %llu\n", records, (unsigned long long)found, (unsigned long long)matches);
        return 1;
      }
      if (attempt == 0 && matches == 0) { break; } // (complete already: there is nothing to write)
    }
    fwrite(&matches, 8, 1, stdout);
    fwrite(status.p, 1, cells, stdout);
    fwrite(offsets.p, 4, cells + 1, stdout);
    fwrite(tag.p, 1, matches, stdout);
    fwrite(value.p, 8, matches, stdout);
    // ---- the gather over the flattened column: one row of `matches` cells ----------------------------------------------------------------------
    {
      const uint32_t rows = uint32_t(matches);
      guarded goffsets, gws, chars;
      goffsets.make((size_t(rows) + 1) * 4, 4);
      gws.make(gather_workspace_bytes(rows), 256);
      const void *total_dev = launch_gather_offsets(reinterpret_cast<const uint64_t *>(value.p), tag.p, rows, string_bytes, reinterpret_cast<uint32_t *>(goffsets.p), gws.p, nullptr);
      uint64_t total;
      memcpy(&total, total_dev, 8);
      chars.make(total, 1, 1);
      launch_gather_copy(sbuf.p, reinterpret_cast<const uint64_t *>(value.p), reinterpret_cast<const uint32_t *>(goffsets.p), rows, total, chars.p, nullptr);
      if (!goffsets.intact() || !gws.intact() || !chars.intact() || !value.intact() || !tag.intact()) {
        fprintf(stderr, "record %lu: the gather wrote outside its outputs\n", records);
        return 1;
      }
      fwrite(&total, 8, 1, stdout);
      fwrite(goffsets.p, 4, size_t(rows) + 1, stdout);
      fwrite(chars.p, 1, total, stdout);
    }
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
