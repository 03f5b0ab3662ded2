// tests/host/test_fields_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_query.hip (compiled as C++ against tests/host/emu, with the scans of
// sjgpu_finish.hip) run the launch sequences of sjgpu_object_fields_from_cells_device and sjgpu_cell_sizes_device (include/sjgpu_fields.h) -- the table
// check, k_rows_locate, the count, the total and the scan, the fill; k_rows_locate and k_cell_sizes -- over tapes the oracle built on the CPU (some of them
// patched by the test) and root cells the test made.  What the C-ABI decides from the total it read back (SJGPU_E_OVERFLOW: no fill) is decided here the
// same way.  tests/test_fields_emu.py compares what comes out with tests/fields_model.py.
// stdin, one record per call:
//   [u32 docs][u64 tape words][u64 string bytes][tape][string records][table: docs + 1 entries of 16 bytes]
//   [u32 rows][u8 root tags[rows]][u64 root values[rows]][u32 capacity: 0 exact, 1 one short, 2 none and null outputs]
// stdout, per record:
//   [i32 code: 0 or -5][u64 fields][u8 status[rows]][u32 offsets[rows + 1]][u8 key tags[written]][u64 key values[written]][u8 tags[written]][u64 values[written]]
//   [u32 sizes[rows]][u8 size codes[rows]], written = fields when the code is 0, else 0
// Every output and the roots' verdicts lie at their exact sizes between poisoned guards (the byte rows and the root tags begin at odd addresses): a byte
// outside is exit code 1, and so is a slot of [0, fields) the fill left unwritten in a tag row.
#include "sjgpu.h"
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
    uint32_t docs;
    if (fread(&docs, 4, 1, stdin) != 1) { break; }
    uint64_t tape_words, string_bytes;
    if (!read_exact(&tape_words, 8) || !read_exact(&string_bytes, 8)) { return 2; }
    guarded tape, sbuf, table, root_tag, root_value;
    tape.make(tape_words * 8, 8);
    sbuf.make(string_bytes, 1, 3); // the records begin at any byte
    table.make((size_t(docs) + 1) * 16, 16);
    if (!read_exact(tape.p, tape.bytes) || !read_exact(sbuf.p, sbuf.bytes) || !read_exact(table.p, table.bytes)) { return 2; }
    uint32_t rows, capacity;
    if (!read_exact(&rows, 4)) { return 2; }
    root_tag.make(rows, 2, 1);
    root_value.make(size_t(rows) * 8, 8);
    if (!read_exact(root_tag.p, root_tag.bytes) || !read_exact(root_value.p, root_value.bytes) || !read_exact(&capacity, 4)) { return 2; }
    records++;
    guarded bad, where, offsets, status, ws, size, size_code;
    bad.make(4, 4);
    memset(bad.p, 0, 4);
    where.make(size_t(rows) * 4, 4);
    offsets.make((size_t(rows) + 1) * 4, 4);
    status.make(rows, 2, 1);
    ws.make(rows ? paths_workspace_bytes(1, rows) : 0, 256);
    size.make(size_t(rows) * 4, 4);
    size_code.make(rows, 2, 1);
    const doc_span_dev *spans = reinterpret_cast<const doc_span_dev *>(table.p);
    const uint64_t *tape_p = reinterpret_cast<const uint64_t *>(tape.p), *roots_p = reinterpret_cast<const uint64_t *>(root_value.p);
    uint32_t *where_p = reinterpret_cast<uint32_t *>(where.p), *offsets_p = reinterpret_cast<uint32_t *>(offsets.p);
    launch_query_check_table(spans, docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(bad.p), nullptr);
    if (*reinterpret_cast<uint32_t *>(bad.p)) { fprintf(stderr, "record %lu: the table check refuses a table the oracle's tapes were laid out by\n", records); return 1; }
    uint64_t fields = 0;
    if (rows) {
      const void *total_dev = launch_object_fields_count(tape_p, spans, docs, roots_p, root_tag.p, rows, where_p, offsets_p, status.p, ws.p, nullptr);
      memcpy(&fields, total_dev, 8);
    } else {
      memset(offsets.p, 0, 4);
    }
    const uint64_t field_cap = capacity == 0 ? fields : capacity == 1 ? (fields ? fields - 1 : 0) : 0;
    const int32_t code = fields > field_cap ? SJGPU_E_OVERFLOW : 0;
    guarded key_value, key_tag, value, tag;
    key_value.make(field_cap * 8, 8);
    key_tag.make(field_cap, 2, 1);
    value.make(field_cap * 8, 8);
    tag.make(field_cap, 2, 1);
    if (!code && fields) {
      const bool none = capacity == 2;
      launch_object_fields_fill(tape_p, sbuf.p, spans, roots_p, rows, where_p, offsets_p, none ? nullptr : reinterpret_cast<uint64_t *>(key_value.p), none ? nullptr : key_tag.p,
                                none ? nullptr : reinterpret_cast<uint64_t *>(value.p), none ? nullptr : tag.p, nullptr);
    }
    if (rows) { // the second call's launches: the verdicts once more, then the sizes
      launch_cell_sizes(tape_p, spans, docs, roots_p, root_tag.p, rows, where_p, reinterpret_cast<uint32_t *>(size.p), size_code.p, nullptr);
    }
    if (!key_value.intact() || !key_tag.intact() || !value.intact() || !tag.intact() || !offsets.intact() || !status.intact() || !where.intact() || !ws.intact() ||
        !tape.intact() || !sbuf.intact() || !table.intact() || !bad.intact() || !root_tag.intact() || !root_value.intact() || !size.intact() || !size_code.intact()) {
      fprintf(stderr, "record %lu: a kernel wrote outside its outputs\n", records);
      return 1;
    }
    if (code && (!key_value.untouched() || !key_tag.untouched() || !value.untouched() || !tag.untouched())) {
      fprintf(stderr, "record %lu: fields were written although they do not fit\n", records);
      return 1;
    }
    const uint64_t written = code ? 0 : fields;
    for (uint64_t i = 0; i < written; i++) { // (no tag is the poison: '"' or 20 for a key, a tape tag or 20 for a value)
      if (key_tag.p[i] == POISON || tag.p[i] == POISON) { fprintf(stderr, "record %lu: slot %llu was not written\n", records, (unsigned long long)i); return 1; }
    }
    fwrite(&code, 4, 1, stdout);
    fwrite(&fields, 8, 1, stdout);
    fwrite(status.p, 1, rows, stdout);
    fwrite(offsets.p, 4, size_t(rows) + 1, stdout);
    fwrite(key_tag.p, 1, written, stdout);
    fwrite(key_value.p, 8, written, stdout);
    fwrite(tag.p, 1, written, stdout);
    fwrite(value.p, 8, written, stdout);
    fwrite(size.p, 4, rows, stdout);
    fwrite(size_code.p, 1, rows, stdout);
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
