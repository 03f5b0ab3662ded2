// tests/host/test_nested_emu.cpp -- CPU tier: the KERNEL SOURCES of sjgpu_write.hip (compiled as C++ against tests/host/emu, with the total of sjgpu_query.hip and the
// scans of sjgpu_finish.hip) run the launch sequence of sjgpu_write_nested_device (include/sjgpu_nested.h) -- the host's table (sj_nested_table.h: the argument
// checks, the escaped keys), count, total, scan, fill -- over fields the test made.  What the C-ABI decides from the eight bytes it reads back (CAPACITY,
// SJGPU_E_OVERFLOW: no fill) is decided here the same way.  tests/test_nested_emu.py compares what comes out with tests/nested_write_model.py.  The twin of
// tests/host/test_write_emu.cpp.
// stdin, one record per call:
//   [u32 n][u32 K][u32 flags][u32 capacity: 0 exact, 1 one short, 2 none and a null chars][u32 skew: the output characters begin at a 16-byte line + skew]
//   per field [u32 key length][key][u32 kind][u8 has values][u8 has valid][u8 has offsets][u8 has chars][u8 has list offsets][u8 has list valid][u16 0]
//             [u64 chars_bytes][u64 bytes of chars that follow][u64 elements]
//             [u64 values[m]] [u64 valid[ceil(m / 64)]] [u32 offsets[m + 1]] [chars] [u32 list offsets[n + 1]] [u64 list valid[ceil(n / 64)]], each only when the
//             field has it; m = elements for a list field (one that has list offsets), n for a plain one
// stdout, per record:
//   [i32 code: 0, 1, -5, or -4 for arguments the table refuses][u64 bytes][u32 offsets[n + 1]][u8 status[n]][u64 counts[6]][u8 chars[written]],
//   written = bytes when the code is 0, else 0; nothing behind the code and the bytes for -4
// Every input, every output, the table and the workspace lie at their exact sizes between poisoned guards (the byte rows begin at odd addresses): a byte written
// outside is exit code 1, and so is an offset, a status or a count that was left unwritten where the poison can tell, or characters written although they do not fit.
#include "sjgpu.h"
#include "sjgpu_nested.h"
#include "sjgpu_internal.h"
#include "sj_nested_table.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
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

struct column_data {
  std::string key;
  guarded values, valid, offsets, chars, list_offsets, list_valid;
};

static bool read_exact(void *dst, size_t n) { return n == 0 || fread(dst, 1, n, stdin) == n; }

int main() {
  sj_emu::max_concurrent_workgroups = 4;
  unsigned long records = 0;
  for (;;) {
    uint32_t head[5];
    if (fread(head, 4, 5, stdin) != 5) { break; }
    const uint32_t n = head[0], K = head[1], flags = head[2], capacity = head[3], skew = head[4];
    records++;
    std::vector<std::unique_ptr<column_data>> data;
    std::vector<sjgpu_write_field> columns(K);
    for (uint32_t k = 0; k < K; k++) {
      data.emplace_back(new column_data);
      column_data &d = *data.back();
      uint32_t key_len, kind;
      uint8_t has[8];
      uint64_t chars_bytes, chars_len, elements;
      if (!read_exact(&key_len, 4)) { return 2; }
      d.key.resize(key_len);
      if (!read_exact(&d.key[0], key_len) || !read_exact(&kind, 4) || !read_exact(has, 8) || !read_exact(&chars_bytes, 8) || !read_exact(&chars_len, 8) ||
          !read_exact(&elements, 8)) { return 2; }
      sjgpu_write_field &f = columns[k];
      memset(&f, 0, sizeof f);
      sjgpu_write_column &c = f.col;
      c.key = reinterpret_cast<const uint8_t *>(d.key.data());
      c.key_len = key_len;
      c.kind = kind;
      c.chars_bytes = chars_bytes;
      f.elements = elements;
      const size_t m = has[4] ? size_t(elements) : size_t(n);
      if (has[0]) { d.values.make(m * 8, 8); if (!read_exact(d.values.p, d.values.bytes)) { return 2; } c.values_dev = d.values.p; }
      if (has[1]) { d.valid.make((m + 63) / 64 * 8, 8); if (!read_exact(d.valid.p, d.valid.bytes)) { return 2; } c.valid_dev = d.valid.p; }
      if (has[2]) { d.offsets.make((m + 1) * 4, 4); if (!read_exact(d.offsets.p, d.offsets.bytes)) { return 2; } c.offsets_dev = d.offsets.p; }
      if (has[3]) { d.chars.make(chars_len, 2, 1); if (!read_exact(d.chars.p, d.chars.bytes)) { return 2; } c.chars_dev = d.chars.p; }
      if (has[4]) { d.list_offsets.make((size_t(n) + 1) * 4, 4); if (!read_exact(d.list_offsets.p, d.list_offsets.bytes)) { return 2; } f.list_offsets_dev = d.list_offsets.p; }
      if (has[5]) { d.list_valid.make((size_t(n) + 63) / 64 * 8, 8); if (!read_exact(d.list_valid.p, d.list_valid.bytes)) { return 2; } f.list_valid_dev = d.list_valid.p; }
    }
    guarded offsets, status, counts, ws, block, chars;
    offsets.make((size_t(n) + 1) * 4, 4);
    status.make(n, 2, 1);
    counts.make(48, 8);
    ws.make(n ? write_workspace_bytes(n) : 0, 256);
    uint32_t *offsets_p = reinterpret_cast<uint32_t *>(offsets.p);
    int32_t code = 0;
    uint64_t bytes = 0;
    write_table table;
    if (!make_nested_table(columns.data(), K, n, flags, &table)) {
      code = SJGPU_E_BADARG;
    } else if (n == 0) {
      offsets_p[0] = 0;
      memset(counts.p, 0, 48);
    }
    block.make(table.bytes.size(), 8);
    if (!table.bytes.empty()) { memcpy(block.p, table.bytes.data(), table.bytes.size()); }
    const write_field_dev *cols = reinterpret_cast<const write_field_dev *>(block.p);
    const uint8_t *keys = block.p + table.keys_at;
    if (!code && n) {
      const count_total_dev *total = launch_nested_count(cols, keys, K, n, flags, offsets_p, status.p, reinterpret_cast<uint64_t *>(counts.p), ws.p, nullptr);
      bytes = total->total;
    }
    const uint64_t chars_cap = capacity == 0 ? bytes : capacity == 1 ? (bytes ? bytes - 1 : 0) : 0;
    chars.make(chars_cap, 16, skew & 15u);
    if (!code && bytes > 0xFFFFFFFFull) { code = 1; }
    if (!code && bytes > chars_cap) { code = SJGPU_E_OVERFLOW; }
    if (!code && bytes) { launch_nested_fill(cols, keys, K, n, flags, offsets_p, capacity == 2 ? nullptr : chars.p, nullptr); }
    bool inputs_intact = block.intact() && (table.bytes.empty() || memcmp(block.p, table.bytes.data(), table.bytes.size()) == 0);
    for (const auto &d : data) { inputs_intact = inputs_intact && d->values.intact() && d->valid.intact() && d->offsets.intact() && d->chars.intact() && d->list_offsets.intact() && d->list_valid.intact(); }
    if (!inputs_intact || !offsets.intact() || !status.intact() || !counts.intact() || !ws.intact() || !chars.intact()) {
      fprintf(stderr, "record %lu: a kernel wrote outside its outputs\n", records);
      return 1;
    }
    if (code && !chars.untouched()) { fprintf(stderr, "record %lu: characters were written although they do not fit\n", records); return 1; }
    fwrite(&code, 4, 1, stdout);
    fwrite(&bytes, 8, 1, stdout);
    if (code == SJGPU_E_BADARG) {
      if (!offsets.untouched() || !status.untouched() || !counts.untouched()) { fprintf(stderr, "record %lu: refused arguments, and an output was written\n", records); return 1; }
      continue;
    }
    if (offsets_p[0] != 0 || offsets_p[n] != uint32_t(bytes)) { fprintf(stderr, "record %lu: the offsets do not end at the total\n", records); return 1; }
    for (uint32_t r = 0; r < n; r++) {
      if (status.p[r] == POISON) { fprintf(stderr, "record %lu: status %u was not written\n", records, r); return 1; }
      if (offsets_p[r + 1] < offsets_p[r] && bytes <= 0xFFFFFFFFull) { fprintf(stderr, "record %lu: the offsets run backwards at %u\n", records, r); return 1; }
    }
    for (int i = 0; i < 48; i += 8) {
      if (counts.p[i + 7] == POISON) { fprintf(stderr, "record %lu: count %d was not written\n", records, i / 8); return 1; }
    }
    const uint64_t written = code ? 0 : bytes;
    fwrite(offsets.p, 4, size_t(n) + 1, stdout);
    fwrite(status.p, 1, n, stdout);
    fwrite(counts.p, 8, 6, stdout);
    fwrite(chars.p, 1, written, stdout);
  }
  fflush(stdout);
  fprintf(stderr, "%lu records\n", records);
  return 0;
}
