/* include/sjgpu_nested.h -- C-ABI of libsjgpu.so, list columns and array rows as nested JSON: the writer of include/sjgpu_write.h with fields that are LISTS (Arrow's
 * list<>: offsets into element arrays) and two row shapes beside the object -- the array [v0,v1,...] and the bare value -- so that what sjgpu_at_paths_from_cells_device
 * and sjgpu_cast_cells_device leave (one ragged list column per path) is written back on the device, and struct columns, list<struct> and list<list<T>> compose out of
 * calls: the counterpart of the reference's string_builder::append(range), start_array / append_comma / end_array (include/simdjson/generic/builder/json_string_builder.h).
 * An extension of include/sjgpu_write.h, which it does not change: sjgpu_write_column, sjgpu_write_records_device and their behaviour stay as they are; a header of its own
 * so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_NESTED_H
#define SJGPU_NESTED_H

#include "sjgpu_write.h"

#ifdef __cplusplus
extern "C" {
#endif

/* row shapes, beside SJGPU_WRITE_OMIT_NULLS = 1 and SJGPU_WRITE_NEWLINE = 2 (sjgpu_write_records_device keeps refusing them) */
enum { SJGPU_WRITE_ARRAY_ROWS = 4, SJGPU_WRITE_BARE = 8 };

typedef struct sjgpu_write_field {        /* HOST memory, K of them */
  sjgpu_write_column col;                 /* list_offsets_dev == null: a plain column over n rows, word for word as in sjgpu_write.h.
                                             Otherwise the ELEMENTS: kind (1-5, 8, 9), values_dev / valid_dev / offsets_dev / chars_dev over `elements` entries
                                             (offsets_dev: elements + 1 words; valid_dev: ceil(elements / 64) words, indexed by the ELEMENT's index, or null); key: the field's */
  const void *list_offsets_dev;           /* u32[n + 1], Arrow list<> offsets into the element arrays; [0] need not be 0 (row k * rows .. of the offsets
                                             sjgpu_at_paths_from_cells_device returns), [n] need not be `elements` */
  const void *list_valid_dev;             /* u64[ceil(n/64)], validity of the LISTS, LSB first, or null: every list valid.  Bits at and beyond n are NOT looked at */
  uint64_t elements;                      /* m, the entries of the element arrays */
} sjgpu_write_field;

/* ---- batched string_builder with lists: one JSON value per row (k_nested_count, k_nested_fill) ----------------------------------------------------------------
 * Row r of K fields.  A plain field (list_offsets_dev == null) is the cell of sjgpu_write.h: its text, what makes it invalid, null or omission, all as there.
 * A LIST field's cell is
 *   a valid list     [ + the elements list_offsets[r] .. list_offsets[r + 1] joined by , + ]; an empty list is [].  An element is written exactly as the plain writer
 *                    writes a cell of that kind (INT64, UINT64, DOUBLE, BOOL, STRING, JSON, STRING_CELLS: sjgpu_write.h).  An INVALID element is ALWAYS null, under
 *                    SJGPU_WRITE_OMIT_NULLS too -- a position in an array means something, and it is what the reference's append(range of std::optional) writes.
 *                    Invalid are: an element whose bit in col.valid_dev is 0 (indexed by the element's index), a DOUBLE that is not finite, a JSON element of length 0.
 *                    The value word and the offsets of an element whose validity bit is 0 are not read.
 *   an invalid list  (its bit in list_valid_dev is 0) a field like any invalid cell: null, or left out with its comma under OMIT_NULLS.  Its list offsets are not
 *                    read: garbage under a 0 bit is not status 19.
 * Row shapes:
 *   default                  the object {"key0":v0,...}: byte for byte what sjgpu_write_records_device writes when no field is a list
 *   SJGPU_WRITE_ARRAY_ROWS   [v0,v1,...,vK-1] (start_array, append, append_comma, end_array).  Keys are not looked at: they may be null and do not count against
 *                            the prefix limits (key_len is not looked at either).  An invalid value is null.  K == 0: [].
 *   SJGPU_WRITE_BARE         K must be 1; the row is the value alone, no brackets of its own, no key.  An invalid value is null; under OMIT_NULLS such a row has
 *                            length 0 -- no newline either --, with status 0: exactly what SJGPU_COL_JSON takes for "no value", so nulls survive composition
 *   SJGPU_WRITE_NEWLINE      as before: one \n that counts in the row's length (not behind a row of length 0)
 * Composition: a struct column is sjgpu_write_records_device over the child columns, taken as a SJGPU_COL_JSON column; a list<struct> the same over the element rows,
 * taken as a list field of JSON elements; a list<list<T>> this call over the inner lists with SJGPU_WRITE_BARE, taken as JSON elements.
 *   status_dev[r]   0, or 19 (INDEX_OUT_OF_BOUNDS): a VALID list whose offsets run backwards or end beyond `elements`; a VALID element of kind 5, 8 or 9 of a valid
 *                   list that does not lie inside chars_dev[0 .. chars_bytes); the plain fields' cases of sjgpu_write.h.  Such a row has length 0 -- no newline
 *                   either --, and nothing outside the declared arrays is read
 *   offsets_dev[0 .. n], chars_dev   as in sjgpu_write.h
 *   counts_dev[0 .. 6)   u64: [0] rows served (status 0), [1] rows with status 19, [2] top-level fields of served rows written as null or left out (an invalid
 *                        list counts once), [3] doubles that are not finite among [2] and [5], [4] elements written in served rows, [5] of those, elements written
 *                        as null.  (A row with status 19 counts nowhere else.)
 * n == 0: 0 with offsets_dev[0] = 0 and six zero counts.
 * Capacity, word for word the plain writer's: chars_cap too small: SJGPU_E_OVERFLOW, *bytes_out says what is needed, offsets_dev, status_dev and counts_dev are complete
 * and nothing is written to chars_dev; chars_cap == 0 with a null chars_dev is how to ask.  A total beyond 32 bits: CAPACITY (1) -- the total out-parameter holds
 * the 64-bit total, status and counts are complete, offsets_dev is written but meaningless (its 32-bit words wrapped) and nothing is written to the data arrays.
 * SJGPU_E_BADARG, before anything is read or enqueued: everything sjgpu_write_records_device refuses, applied per field (a null `fields` when K > 0; the key limits
 * only where keys are written); a flag outside the four; ARRAY_ROWS with OMIT_NULLS; ARRAY_ROWS with BARE; BARE with K != 1; a list field whose element kind is
 * outside 1-5, 8, 9; list_offsets_dev not 4-byte, list_valid_dev not 8-byte aligned; elements + 1 beyond 0xFFFFFFF0; for a list field, when n > 0 and
 * elements > 0, a null element array that the kind reads (values_dev: 1-4, 9; offsets_dev: 5, 8; chars_dev: 5, 8, 9 with chars_bytes > 0).  A list field of no
 * elements may leave its element arrays null.  list_valid_dev and elements of a plain field are not looked at.
 * Nothing is written outside offsets_dev[0 .. n], status_dev[0 .. n), chars_dev[0 .. *bytes_out) and the six counts; nothing is read outside the fields' declared arrays.
 * The outputs must not overlap the inputs.
 * The field table and the escaped keys go up through the block the context owns, as in sjgpu_write_records_device: the call first WAITS for the context's previous user
 * of that block, and the block is free again when the call returns.
 * Returns 0, CAPACITY or a negative SJGPU_E_*; what a row is shows in its status, never in the return value.
 * Four launches and a memset: count, the total, the scan, fill.  Waits for the stream: the total is read back, and the texts are complete on return.  UTF-8 is not
 * validated.
 * The cost: a row is ONE lane's work, its lists included, and a lane reads its list's elements one after the other: rows of very different lengths leave the lanes of
 * a wave waiting for the longest, and one huge list is one lane's (a breadth-first writer for it is not built).
 * The fill: a workgroup takes 256 consecutive rows at a time; their texts are one contiguous span of chars_dev.  A span of at most 28 KiB is put together in LDS, a row
 * per lane, and leaves in 16-byte stores aligned to the output; a longer one -- with lists, many are -- is written by its lanes straight to chars_dev.  Which of the
 * two follows from offsets_dev alone.  (Cutting a longer span into groups of 128, 64 or 32 rows that fit was built and measured, and lost to the direct road: it is
 * compiled out.)  The fill never writes at or beyond offsets[r + 1], whatever the inputs say by then. */
int sjgpu_write_nested_device(sjgpu_ctx *ctx, const sjgpu_write_field *fields, uint32_t K, uint32_t n, uint32_t flags,
                              void *offsets_dev /* n + 1 u32 */, void *status_dev /* n bytes */, void *chars_dev, uint64_t chars_cap,
                              void *counts_dev /* 6 u64 */, void *stream, uint64_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif
