// tests/host/test_lists_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_query.hip (compiled as C++ against tests/host/emu, with the scans of
// sjgpu_finish.hip) run the launch sequence of sjgpu_at_paths_from_cells_device (include/sjgpu_lists.h) -- the table check, k_rows_locate, the rooted count,
// the total and the scan, the rooted fill -- over tapes the oracle built on the CPU and root cells the test made.  The paths are compiled by the host code
// the C-ABI uses (sj_path_program.h), and what the C-ABI decides from the total it read back (SJGPU_E_OVERFLOW: no fill) is decided here the same way.
// tests/test_lists_emu.py compares what comes out with tests/lists_model.py.
// stdin, one record per call:
//   [u32 docs][u64 tape words][u64 string bytes][tape][string records][table: docs + 1 entries of 16 bytes]
//   [u32 rows][u8 root tags[rows]][u64 root values[rows]][u32 K][u32 lens[K]][the paths' bytes][u32 capacity: 0 exact, 1 one short, 2 none and null outputs]
// stdout, per record:
//   [i32 code: 0 or -5][u64 matches][u8 status[K * rows]][u32 offsets[K * rows + 1]][u8 tags[written]][u64 values[written]], written = matches when the code is 0, else 0
// Every output and the roots' verdicts lie at their exact sizes between poisoned guards (the byte rows and the root tags begin at odd addresses): a byte
// outside is exit code 1.  Paths beyond the limits (K > 64, 1024 bytes, 32 levels, 32 tokens, 8 wildcards) are exit code 3: the call refuses them before
// anything runs.
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
    uint32_t docs;
    if (fread(&docs, 4, 1, stdin) != 1) { break; }
    uint64_t tape_words, string_bytes;
    if (!read_exact(&tape_words, 8) || !read_exact(&string_bytes, 8)) { return 2; }
    guarded tape, sbuf, table, root_tag, root_value;
    tape.make(tape_words * 8, 8);
    sbuf.make(string_bytes, 1, 3); // the records begin at any byte
    table.make((size_t(docs) + 1) * 16, 16);
    if (!read_exact(tape.p, tape.bytes) || !read_exact(sbuf.p, sbuf.bytes) || !read_exact(table.p, table.bytes)) { return 2; }
    uint32_t rows;
    if (!read_exact(&rows, 4)) { return 2; }
    root_tag.make(rows, 2, 1);
    root_value.make(size_t(rows) * 8, 8);
    if (!read_exact(root_tag.p, root_tag.bytes) || !read_exact(root_value.p, root_value.bytes)) { return 2; }
    uint32_t K;
    if (!read_exact(&K, 4)) { return 2; }
    std::vector<uint32_t> lens(K);
    if (!read_exact(lens.data(), size_t(K) * 4)) { return 2; }
    size_t total_len = 0;
    for (uint32_t l : lens) { total_len += l; }
    std::vector<uint8_t> paths(total_len + 1);
    uint32_t capacity;
    if (!read_exact(paths.data(), total_len) || !read_exact(&capacity, 4)) { return 2; }
    records++;
    path_program prog;
    if (!compile_path_program(paths.data(), lens.data(), K, &prog)) { fprintf(stderr, "record %lu: the paths are beyond the limits\n", records); return 3; }
    guarded program, bad, where, offsets, status, ws;
    program.make(prog.bytes.size(), 16);
    memcpy(program.p, prog.bytes.data(), prog.bytes.size());
    bad.make(4, 4);
    memset(bad.p, 0, 4);
    const size_t cells = size_t(K) * rows;
    where.make(size_t(rows) * 4, 4);
    offsets.make((cells + 1) * 4, 4);
    status.make(cells, 2, 1);
    ws.make(paths_workspace_bytes(K, rows), 256);
    const doc_span_dev *spans = reinterpret_cast<const doc_span_dev *>(table.p);
    const uint64_t *tape_p = reinterpret_cast<const uint64_t *>(tape.p), *roots_p = reinterpret_cast<const uint64_t *>(root_value.p);
    launch_query_check_table(spans, docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(bad.p), nullptr);
    if (*reinterpret_cast<uint32_t *>(bad.p)) { fprintf(stderr, "record %lu: the table check refuses a table the oracle's tapes were laid out by\n", records); return 1; }
    uint64_t matches = 0;
    if (K && rows) {
      const void *total_dev = launch_paths_rooted_count(tape_p, sbuf.p, spans, docs, roots_p, root_tag.p, rows, reinterpret_cast<uint32_t *>(where.p), program.p, prog.levels_at,
                                                        prog.tokens_at, prog.keys_at, K, reinterpret_cast<uint32_t *>(offsets.p), status.p, ws.p, nullptr);
      memcpy(&matches, total_dev, 8);
    } else {
      memset(offsets.p, 0, 4);
    }
    const uint64_t match_cap = capacity == 0 ? matches : capacity == 1 ? (matches ? matches - 1 : 0) : 0;
    const int32_t code = matches > match_cap ? SJGPU_E_OVERFLOW : 0;
    guarded value, tag;
    value.make(match_cap * 8, 8);
    tag.make(match_cap, 2, 1);
    if (!code && matches) {
      launch_paths_rooted_fill(tape_p, sbuf.p, spans, roots_p, rows, reinterpret_cast<const uint32_t *>(where.p), program.p, prog.levels_at, prog.tokens_at, prog.keys_at, K,
                               reinterpret_cast<const uint32_t *>(offsets.p), capacity == 2 ? nullptr : reinterpret_cast<uint64_t *>(value.p), capacity == 2 ? nullptr : tag.p, nullptr);
    }
    if (!value.intact() || !tag.intact() || !offsets.intact() || !status.intact() || !where.intact() || !ws.intact() || !tape.intact() || !sbuf.intact() || !table.intact() ||
        !program.intact() || !bad.intact() || !root_tag.intact() || !root_value.intact()) {
      fprintf(stderr, "record %lu: the walk wrote outside its outputs\n", records);
      return 1;
    }
    if (code && (!value.untouched() || !tag.untouched())) {
      fprintf(stderr, "record %lu: matches were written although they do not fit\n", records);
      return 1;
    }
    const uint64_t written = code ? 0 : matches;
    fwrite(&code, 4, 1, stdout);
    fwrite(&matches, 8, 1, stdout);
    fwrite(status.p, 1, cells, stdout);
    fwrite(offsets.p, 4, cells + 1, stdout);
    fwrite(tag.p, 1, written, stdout);
    fwrite(value.p, 8, written, stdout);
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
