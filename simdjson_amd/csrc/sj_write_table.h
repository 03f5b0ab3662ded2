// simdjson_amd/csrc/sj_write_table.h -- what sjgpu_write_records_device (include/sjgpu_write.h) decides and makes on the HOST before anything is enqueued: the
// argument checks of its columns and the block that goes up -- the column table the kernels of sjgpu_write.hip read and, behind it, every column's escaped "key":
// prefix, made by the code the device escapes strings with (sj_json_text.h).  Host only; shared by the entry point (sjgpu_capi_stage2.hip) and tests/host.
#ifndef SJGPU_SJ_WRITE_TABLE_H
#define SJGPU_SJ_WRITE_TABLE_H

#include <cstring>
#include <vector>

#include "sjgpu_internal.h"
#include "sjgpu_write.h"
#include "sj_json_text.h"

namespace sjgpu {

// the block: [K write_column_dev][the prefixes back to back]; keys_at: where the prefixes begin (8-byte aligned)
struct write_table {
  std::vector<uint8_t> bytes;
  size_t keys_at = 0;
};

inline bool write_misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// everything of SJGPU_E_BADARG that concerns the columns, n and the flags -> false; true with the table made (K == 0: an empty one)
inline bool make_write_table(const sjgpu_write_column *columns, uint32_t K, uint32_t n, uint32_t flags, write_table *table) {
  if (K > WRITE_MAX_COLUMNS || (K && !columns) || (flags & ~uint32_t(SJGPU_WRITE_OMIT_NULLS | SJGPU_WRITE_NEWLINE)) || uint64_t(n) + 1 > 0xFFFFFFF0ull) { return false; }
  size_t prefixes = 0;
  for (uint32_t k = 0; k < K; k++) {
    const sjgpu_write_column &c = columns[k];
    const bool valued = (c.kind >= SJGPU_COL_INT64 && c.kind <= SJGPU_COL_BOOL) || c.kind == SJGPU_COL_STRING_CELLS;
    const bool ranged = c.kind == SJGPU_COL_STRING || c.kind == SJGPU_COL_JSON;
    if (!valued && !ranged) { return false; }
    if (c.key_len > WRITE_MAX_KEY || (c.key_len && !c.key)) { return false; }
    if (write_misaligned(c.values_dev, 8) || write_misaligned(c.valid_dev, 8) || write_misaligned(c.offsets_dev, 4) || c.chars_bytes > 0xFFFFFFFFull) { return false; }
    if (n && ((valued && !c.values_dev) || (ranged && !c.offsets_dev) || ((ranged || c.kind == SJGPU_COL_STRING_CELLS) && c.chars_bytes && !c.chars_dev))) { return false; }
    prefixes += size_t(escaped_length(c.key, c.key_len)) + 1;
    if (prefixes > WRITE_MAX_PREFIXES) { return false; }
  }
  table->keys_at = size_t(K) * sizeof(write_column_dev);
  table->bytes.assign(table->keys_at + prefixes, 0);
  size_t at = 0;
  for (uint32_t k = 0; k < K; k++) {
    const sjgpu_write_column &c = columns[k];
    const bool valued = (c.kind >= SJGPU_COL_INT64 && c.kind <= SJGPU_COL_BOOL) || c.kind == SJGPU_COL_STRING_CELLS;
    write_column_dev d;
    std::memset(&d, 0, sizeof d);
    d.values = valued ? static_cast<const uint64_t *>(c.values_dev) : nullptr;
    d.valid = static_cast<const uint64_t *>(c.valid_dev);
    d.offsets = valued ? nullptr : static_cast<const uint32_t *>(c.offsets_dev);
    d.chars = c.kind >= SJGPU_COL_STRING ? static_cast<const uint8_t *>(c.chars_dev) : nullptr;
    d.chars_bytes = c.kind >= SJGPU_COL_STRING ? c.chars_bytes : 0;
    d.kind = c.kind;
    d.key_at = uint32_t(at);
    const size_t quoted = size_t(escaped_length(c.key, c.key_len));
    uint8_t *out = table->bytes.data() + table->keys_at + at;
    (void)escape_write(c.key, c.key_len, out, quoted);
    out[quoted] = uint8_t(':');
    d.key_len = uint32_t(quoted + 1);
    at += quoted + 1;
    std::memcpy(table->bytes.data() + size_t(k) * sizeof(write_column_dev), &d, sizeof d);
  }
  return true;
}

} // namespace sjgpu
#endif
