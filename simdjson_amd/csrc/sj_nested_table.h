// simdjson_amd/csrc/sj_nested_table.h -- what sjgpu_write_nested_device (include/sjgpu_nested.h) decides and makes on the HOST before anything is enqueued, the
// sibling of sj_write_table.h: the argument checks of its fields and flags and the block that goes up -- the field table the kernels k_nested_* of sjgpu_write.hip
// read and, behind it, every field's escaped "key": prefix (none under SJGPU_WRITE_ARRAY_ROWS and SJGPU_WRITE_BARE, where keys are not looked at).
// Host only; shared by the entry point (sjgpu_capi_stage2.hip) and tests/host.
#ifndef SJGPU_SJ_NESTED_TABLE_H
#define SJGPU_SJ_NESTED_TABLE_H

#include "sjgpu_nested.h"
#include "sj_write_table.h"

namespace sjgpu {

// everything of SJGPU_E_BADARG that concerns the fields, n and the flags -> false; true with the table made: [K write_field_dev][the prefixes back to back]
inline bool make_nested_table(const sjgpu_write_field *fields, uint32_t K, uint32_t n, uint32_t flags, write_table *table) {
  const uint32_t all = SJGPU_WRITE_OMIT_NULLS | SJGPU_WRITE_NEWLINE | SJGPU_WRITE_ARRAY_ROWS | SJGPU_WRITE_BARE;
  if (K > WRITE_MAX_COLUMNS || (K && !fields) || (flags & ~all) || uint64_t(n) + 1 > 0xFFFFFFF0ull) { return false; }
  const bool array = (flags & SJGPU_WRITE_ARRAY_ROWS) != 0, bare = (flags & SJGPU_WRITE_BARE) != 0, keyed = !array && !bare;
  if ((array && (flags & SJGPU_WRITE_OMIT_NULLS)) || (array && bare) || (bare && K != 1)) { return false; }
  size_t prefixes = 0;
  for (uint32_t k = 0; k < K; k++) {
    const sjgpu_write_field &f = fields[k];
    const sjgpu_write_column &c = f.col;
    const bool list = f.list_offsets_dev != nullptr;
    const bool valued = (c.kind >= SJGPU_COL_INT64 && c.kind <= SJGPU_COL_BOOL) || c.kind == SJGPU_COL_STRING_CELLS;
    const bool ranged = c.kind == SJGPU_COL_STRING || c.kind == SJGPU_COL_JSON;
    if (!valued && !ranged) { return false; }
    if (keyed && (c.key_len > WRITE_MAX_KEY || (c.key_len && !c.key))) { return false; }
    if (write_misaligned(c.values_dev, 8) || write_misaligned(c.valid_dev, 8) || write_misaligned(c.offsets_dev, 4) || c.chars_bytes > 0xFFFFFFFFull) { return false; }
    if (list && (write_misaligned(f.list_offsets_dev, 4) || write_misaligned(f.list_valid_dev, 8) || f.elements > 0xFFFFFFF0ull - 1)) { return false; }
    const bool read = list ? n != 0 && f.elements != 0 : n != 0; // whether a kernel may read the column's arrays at all
    if (read && ((valued && !c.values_dev) || (ranged && !c.offsets_dev) || ((ranged || c.kind == SJGPU_COL_STRING_CELLS) && c.chars_bytes && !c.chars_dev))) { return false; }
    if (keyed) {
      prefixes += size_t(escaped_length(c.key, c.key_len)) + 1;
      if (prefixes > WRITE_MAX_PREFIXES) { return false; }
    }
  }
  table->keys_at = size_t(K) * sizeof(write_field_dev);
  table->bytes.assign(table->keys_at + prefixes, 0);
  size_t at = 0;
  for (uint32_t k = 0; k < K; k++) {
    const sjgpu_write_field &f = fields[k];
    const sjgpu_write_column &c = f.col;
    const bool list = f.list_offsets_dev != nullptr;
    const bool valued = (c.kind >= SJGPU_COL_INT64 && c.kind <= SJGPU_COL_BOOL) || c.kind == SJGPU_COL_STRING_CELLS;
    write_field_dev d;
    std::memset(&d, 0, sizeof d);
    d.col.values = valued ? static_cast<const uint64_t *>(c.values_dev) : nullptr;
    d.col.valid = static_cast<const uint64_t *>(c.valid_dev);
    d.col.offsets = valued ? nullptr : static_cast<const uint32_t *>(c.offsets_dev);
    d.col.chars = c.kind >= SJGPU_COL_STRING ? static_cast<const uint8_t *>(c.chars_dev) : nullptr;
    d.col.chars_bytes = c.kind >= SJGPU_COL_STRING ? c.chars_bytes : 0;
    d.col.kind = c.kind;
    d.list_offsets = static_cast<const uint32_t *>(f.list_offsets_dev);
    d.list_valid = list ? static_cast<const uint64_t *>(f.list_valid_dev) : nullptr;
    d.elements = list ? f.elements : 0;
    if (keyed) {
      d.col.key_at = uint32_t(at);
      const size_t quoted = size_t(escaped_length(c.key, c.key_len));
      uint8_t *out = table->bytes.data() + table->keys_at + at;
      (void)escape_write(c.key, c.key_len, out, quoted);
      out[quoted] = uint8_t(':');
      d.col.key_len = uint32_t(quoted + 1);
      at += quoted + 1;
    }
    std::memcpy(table->bytes.data() + size_t(k) * sizeof(write_field_dev), &d, sizeof d);
  }
  return true;
}

} // namespace sjgpu
#endif
