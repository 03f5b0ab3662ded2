// tests/host/test_rows_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_query.hip (compiled as C++ against tests/host/emu) run the launch sequence of
// sjgpu_at_pointers_from_cells_device (include/sjgpu_rows.h) -- the table check, k_rows_locate, k_at_pointers_rooted -- over tapes the oracle built on the CPU
// and root cells the test made.  The pointers are compiled by the host code the C-ABI uses (sj_query_program.h).  tests/test_rows_emu.py compares what
// comes out with tests/rows_model.py.
// stdin, one record per call:
//   [u32 docs][u64 tape words][u64 string bytes][tape][string records][table: docs + 1 entries of 16 bytes]
//   [u32 rows][u8 root tags[rows]][u64 root values[rows]][u32 K][u32 lens[K]][the pointers' bytes]
// stdout, per record: [u8 tags[K * rows]][u64 values[K * rows]]
// Every output and the roots' verdicts lie at their exact sizes between poisoned guards (the tag rows and the root tags begin at odd addresses): a byte
// outside is exit code 1.  Pointers beyond the limits (K > 64, 1024 bytes, 32 tokens) are exit code 3: the call refuses them before anything runs.
#include "sjgpu.h"
#include "sjgpu_internal.h"
#include "sj_query_program.h"

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
    std::vector<uint8_t> pointers(total_len + 1);
    if (!read_exact(pointers.data(), total_len)) { return 2; }
    records++;
    query_program prog;
    if (!compile_query_program(pointers.data(), lens.data(), K, &prog)) { fprintf(stderr, "record %lu: the pointers are beyond the limits\n", records); return 3; }
    guarded program, bad, where, value, tag;
    program.make(prog.bytes.size(), 16);
    memcpy(program.p, prog.bytes.data(), prog.bytes.size());
    bad.make(4, 4);
    memset(bad.p, 0, 4);
    const size_t cells = size_t(K) * rows;
    where.make(size_t(rows) * 4, 4);
    value.make(cells * 8, 8);
    tag.make(cells, 2, 1);
    const doc_span_dev *spans = reinterpret_cast<const doc_span_dev *>(table.p);
    launch_query_check_table(spans, docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(bad.p), nullptr);
    if (*reinterpret_cast<uint32_t *>(bad.p)) { fprintf(stderr, "record %lu: the table check refuses a table the oracle's tapes were laid out by\n", records); return 1; }
    if (K && rows) {
      launch_at_pointers_rooted(reinterpret_cast<const uint64_t *>(tape.p), sbuf.p, spans, docs, reinterpret_cast<const uint64_t *>(root_value.p), root_tag.p, rows,
                                reinterpret_cast<uint32_t *>(where.p), program.p, prog.tokens_at, prog.keys_at, K, reinterpret_cast<uint64_t *>(value.p), tag.p, nullptr);
    }
    if (!value.intact() || !tag.intact() || !where.intact() || !tape.intact() || !sbuf.intact() || !table.intact() || !program.intact() || !bad.intact() || !root_tag.intact() ||
        !root_value.intact()) {
      fprintf(stderr, "record %lu: the walk wrote outside its columns\n", records);
      return 1;
    }
    fwrite(tag.p, 1, cells, stdout);
    fwrite(value.p, 8, cells, stdout);
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
