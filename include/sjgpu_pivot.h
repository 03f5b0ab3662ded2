/* include/sjgpu_pivot.h -- C-ABI of libsjgpu.so, a map column pivoted into a record table: the fields of every row (parent row, key code, value cell -- the
 * long format sjgpu_object_fields_from_cells_device and sjgpu_dictionary_encode_device leave on the device) scattered into one column per key (the wide
 * format): batched element::at_key for every learned key, and, through the column map, element::at_key_case_insensitive.
 * An extension of include/sjgpu_dict.h and the headers below it (the cell encoding, the fields' rows and the codes are declared there, in
 * include/sjgpu_fields.h and in include/sjgpu_query.h); a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_PIVOT_H
#define SJGPU_PIVOT_H

#include "sjgpu_dict.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched `for (key k : keys) column[k][r] = object(row r).at_key(k)` over listed fields (k_pivot_fill, k_pivot_scatter) ---------------------------
 * Inputs, as the existing calls leave them, all device memory:
 *   offsets_dev[0 .. rows], status_dev[0 .. rows), value_dev / tag_dev[0 .. fields)    those of sjgpu_object_fields_from_cells_device: the slots of row r are
 *                                                                                      offsets[r] .. offsets[r + 1], in the reference's iteration order
 *   codes_dev[0 .. fields)            int32, what sjgpu_dictionary_encode_device made of that call's key row: the code of slot i's key, -1 for none
 *   column_of_code_dev[0 .. groups)   int32, the output column of every code, or NULL: column = code.  Several codes may share a column: that is how the
 *                                     spellings of one key (ID / Id / id) become one column
 * No tape, no string buffer and no document table is read.
 * Output: cell (c, r) lies at index c * rows + r of value_out_dev (u64) and tag_out_dev (bytes) -- the row-per-column layout of
 * sjgpu_at_pointers_from_cells_device, so every *_from_cells call, the cast, the census, the gather and the serializers take a column as it lies.
 * Cell (c, r):
 *   status[r] != 0    tag = status[r], value 0, for every column: the codes element::at_key answers for that root -- 17 for a non-object, a forwarded
 *                     17 / 19 / 20 / 22, 20 for a root that disagrees with its tape.  The row's slice is not looked at.
 *   status[r] == 0    the value and tag of the FIRST slot i in [offsets[r], offsets[r + 1]) whose column is c, copied unchanged; tag 20 (NO_SUCH_FIELD), value 0
 *                     when there is none.  The column of slot i is codes[i] when the map is NULL, else column_of_code[codes[i]].  A slot is ignored when its
 *                     code is negative or >= groups, or when its column is negative or >= columns.  Among several codes on one column the order of the ROW
 *                     decides, not the order of the codes: "the first field that matches wins" is the reference's rule for at_key and for
 *                     at_key_case_insensitive alike (include/simdjson/dom/object-inl.h:246-278).
 *   a row with status 0 whose slice runs backwards (offsets[r] > offsets[r + 1]) or ends beyond `fields`: every cell tag 20, value 0; none of its slots is read.
 * Every one of the columns * rows cells is written; nothing is written outside the two output arrays and nothing is read outside the arrays named.  The outputs
 * must not overlap the inputs.  The result is a pure function of the inputs: which lane ran first shows nowhere, and two runs give the same bytes.
 * rows == 0 or columns == 0: 0, nothing written.  fields == 0 is served: every cell is 20 or its row's status.
 * SJGPU_E_BADARG, before anything is enqueued: ctx null; columns * rows above 0xFFFFFFF0 (a caller with more cells pivots in chunks of columns, which is what the
 * map is for: the codes of the other chunks map to -1); value_dev or value_out_dev not 8-byte aligned; offsets_dev, codes_dev or column_of_code_dev not 4-byte
 * aligned (status_dev and the tag rows begin at any byte); with rows * columns > 0 a null offsets_dev, status_dev, value_out_dev or tag_out_dev; with
 * fields > 0 a null codes_dev, value_dev or tag_dev; fields beyond 32 bits; a non-null map with groups == 0.
 * Returns 0 or a negative SJGPU_E_*; what a cell met is in its tag, never in the return value.
 * Only enqueues on `stream`: two launches, no memset, no read-back, no block of the context, no workspace, no wait for the context's previous query.  The map is
 * device memory: nothing is uploaded.
 *
 * How.  k_pivot_fill gives every cell its default -- its row's status, or 20 -- and value 0: one lane per two cells, a 16-byte store for the two words (an
 * 8-byte one at an odd end) and two byte stores, consecutive lanes on consecutive cells.  k_pivot_scatter, behind it on the stream, is one lane per row,
 * consecutive lanes on consecutive rows; a lane takes its row's slots from the LAST to the FIRST and stores each at its cell, so the first field's store is the
 * last one to land: a lane's own stores to one address stay in program order.  No atomics, nothing that depends on scheduling.  Records that share a key order
 * store column c from consecutive lanes to consecutive addresses.
 * Cost, not hidden: the fill writes 9 bytes per cell; the scatter reads 13 bytes per slot (code, word, tag; 4 more through a map) with a stride of one row's
 * slots between neighbouring lanes, and writes 9 bytes per slot that has a column.  One object of a million fields is ONE lane's work, as in every other call
 * here; a cooperative road for one huge object is not built.
 * Measured (MI355X, scripts/pivot_once.py, profiles/pivot.txt, medians of 20, one twitter-like document of 256 MiB, 344 727 rows), beside the only road there was
 * to the same table, sjgpu_at_pointers_from_cells_device for `/` + each key: the users (5 fields a row, G = 5, 1.7 M cells) 0.022 ms against 0.357 ms; the
 * statuses (9 fields a row with nested values, G = 9, 3.1 M cells) 0.056 ms against 0.817 ms -- about 15 times, of which the fill is 0.011 and 0.013 ms.  Both roads
 * first pay the fields call (0.21 / 0.31 ms) and the encode (0.44 / 0.71 ms) to learn the keys at all.  These tables are small (15 and 28 MB written) and G is
 * far below 64; no input with G near or above 64 was measured, and nothing says where the pointer road, which needs neither fields nor codes for keys the
 * caller already knows, would win.  The other scatter shape -- a workgroup per tile of rows, one lane per slot, coalesced loads and scattered stores -- is not
 * built and was not measured. */
int sjgpu_pivot_fields_device(sjgpu_ctx *ctx, const void *offsets_dev /* rows + 1 u32 */, const void *status_dev /* rows bytes */, uint32_t rows,
                              const void *codes_dev /* fields int32 */, const void *value_dev /* fields u64 */, const void *tag_dev /* fields bytes */, uint64_t fields,
                              const void *column_of_code_dev /* groups int32, or NULL = identity */, uint32_t groups, uint32_t columns,
                              void *value_out_dev /* columns * rows u64 */, void *tag_out_dev /* columns * rows bytes */, void *stream);

#ifdef __cplusplus
}
#endif
#endif
