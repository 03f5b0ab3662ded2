/* include/sjgpu_write.h -- C-ABI of libsjgpu.so, typed columns as JSON records: row r of K device-resident columns written on the device as the object
 * {"key0":v0,"key1":v1,...}, every row's text into one `offsets` / `chars` pair (Arrow's utf8 layout) -- the way back from columns to JSON, the counterpart of the
 * reference's simdjson::builder::string_builder (include/simdjson/generic/builder/json_string_builder.h) for data that lives in device memory.
 * An extension of include/sjgpu_json.h and the headers below it (what sjgpu_cast_cells_device, sjgpu_gather_strings_device and sjgpu_serialize_cells_device leave is
 * declared there); a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_WRITE_H
#define SJGPU_WRITE_H

#include "sjgpu_json.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what a column holds */
enum { SJGPU_COL_INT64 = 1, SJGPU_COL_UINT64 = 2, SJGPU_COL_DOUBLE = 3, SJGPU_COL_BOOL = 4,   /* = SJGPU_GET_* 1..4 */
       SJGPU_COL_STRING = 5,        /* offsets_dev u32[n+1] + chars_dev: what sjgpu_gather_strings_device returns */
       SJGPU_COL_JSON = 8,          /* offsets_dev + chars_dev copied as they are (append_raw): what sjgpu_serialize_cells_device returns */
       SJGPU_COL_STRING_CELLS = 9 };/* values_dev[r] = offset | length << 32 into chars_dev: the word of a '"' cell, chars_dev the string buffer */
enum { SJGPU_WRITE_OMIT_NULLS = 1, SJGPU_WRITE_NEWLINE = 2 };

typedef struct sjgpu_write_column {          /* HOST memory, K of them */
  const uint8_t *key; uint32_t key_len;      /* HOST, the UNESCAPED key, any bytes (NUL, quotes) */
  uint32_t kind;
  const void *values_dev;                    /* u64[n]: kinds 1-4 and 9 (BOOL: zero / non-zero; what sjgpu_cast_cells_device writes) */
  const void *valid_dev;                     /* u64[ceil(n/64)], Arrow validity, LSB first, or null: every cell valid.  Bits at and beyond n are NOT looked at */
  const void *offsets_dev; const void *chars_dev; uint64_t chars_bytes;   /* kinds 5, 8 (offsets + chars) and 9 (chars only) */
} sjgpu_write_column;

/* ---- batched string_builder: one JSON object per row (k_write_count, k_write_fill) ----------------------------------------------------------------------------
 * The bytes of row r are exactly what the reference's string_builder holds after start_object(), append_key_value(key, v) for every field in column order with the
 * caller's append_comma() between two fields, end_object() (a JSON cell: escape_and_append_with_quotes(key), append_colon(), append_raw(text)):
 *   {  the fields joined by ,  }   and, under SJGPU_WRITE_NEWLINE, one \n that counts in the row's length: the chars are then an NDJSON stream sjgpu_parse_many reads
 *   a field       " + the escaped key + ": + the value; duplicate keys are written as they come, the empty key is ""
 *   INT64 UINT64  the shortest decimal, -9223372036854775808 and 18446744073709551615 included
 *   DOUBLE        the reference's to_chars(double), as sjgpu_serialize_cells_device writes a d cell; -0.0 is -0.0
 *   BOOL          false for a zero word, true for any other
 *   STRING, STRING_CELLS and keys   between quotes: " as \" and \ as \\, 0x08 0x09 0x0a 0x0c 0x0d as \b \t \n \f \r, every other byte up to 0x1f as \u00xx in
 *                 lower-case hex (the reference's control_chars[]), every byte from 0x20 up as it is, the bytes of multi-byte characters included
 *   JSON          the cell's bytes as they are; whether they are JSON is the caller's business, as with append_raw
 * An INVALID cell is written as null (the reference's append_null(), what it writes for an empty optional); under SJGPU_WRITE_OMIT_NULLS the field and its comma are
 * left out instead, and a row whose fields are all left out is {}.  Invalid are: a cell whose validity bit is 0; a DOUBLE that is not finite -- THIS RULE IS OURS: the
 * reference is built with SIMDJSON_ENABLE_NAN_INF 0 and has no text for one, and no JSON text has one either --; and a JSON cell of length 0 (what
 * sjgpu_serialize_cells_device leaves for a cell it refused).  The value word and the offsets of a cell whose validity bit is 0 are not read.
 *   status_dev[r]   0, or 19 (INDEX_OUT_OF_BOUNDS) when a VALID cell of kind 5, 8 or 9 does not lie inside its chars_dev[0 .. chars_bytes): offsets that run backwards,
 *                   an end beyond chars_bytes, offset + length beyond it.  Such a row has length 0 -- no newline either --, and nothing outside the declared ranges is read
 *   offsets_dev[0 .. n]   u32, the exclusive sum of the rows' lengths; offsets_dev[n] == *bytes_out
 *   chars_dev             the rows back to back, no terminators
 *   counts_dev[0 .. 4)    u64: [0] rows served (status 0), [1] rows with status 19, [2] cells of served rows written as null or left out, [3] of those, doubles
 *                         that are not finite.  (The cells of a row with status 19 count nowhere: nothing was written for them.)
 * K == 0: {} per row.  n == 0: 0 with offsets_dev[0] = 0 and four zero counts.
 * chars_cap too small: SJGPU_E_OVERFLOW, *bytes_out says what is needed, offsets_dev, status_dev and counts_dev are complete and nothing is written to chars_dev;
 * chars_cap == 0 with a null chars_dev is how to ask.  A total beyond 32 bits: CAPACITY (1) -- the total out-parameter holds
 * the 64-bit total, status and counts are complete, offsets_dev is written but meaningless (its 32-bit words wrapped) and nothing is written to the data arrays.
 * SJGPU_E_BADARG, before anything is read or enqueued: a null ctx, offsets_dev, counts_dev or bytes_out, a null status_dev when n > 0, a null chars_dev when
 * chars_cap > 0, a null columns when K > 0, a null key with key_len > 0; when n > 0, a null values_dev (kinds 1-4, 9), offsets_dev (5, 8) or chars_dev (5, 8, 9 with
 * chars_bytes > 0) of a column; a kind or a flag outside the lists; K > 64; key_len > 1024; escaped "key": prefixes that together exceed 8 192 bytes; values_dev,
 * valid_dev or counts_dev not 8-byte, a column's or the output's offsets_dev not 4-byte aligned (chars and status begin at any byte); a chars_bytes beyond 32 bits;
 * n + 1 beyond 0xFFFFFFF0.
 * Nothing is written outside offsets_dev[0 .. n], status_dev[0 .. n), chars_dev[0 .. *bytes_out) and the four counts; nothing is read outside the columns' declared
 * arrays.  The outputs must not overlap the inputs.
 * The keys are escaped once on the host -- by the code the device uses for strings -- and go up with the column table through a block the context owns, the block of
 * the compiled pointers of sjgpu_at_pointers_device; as there, the call first WAITS for the context's previous user of that block.  The block is free again when the
 * call returns.
 * Returns 0, CAPACITY or a negative SJGPU_E_*; what a row is shows in its status, never in the return value.
 * Four launches and a memset: count, the total, the scan, fill.  Waits for the stream: the total is read back, and the texts are complete on return.
 * UTF-8 is NOT validated, in keys or in strings -- nor does the reference: string_builder::validate_unicode() is a call of its own there, and
 * sjgpu_validate_utf8_device over chars_dev[0 .. *bytes_out) is its counterpart here.
 * The fill: a workgroup takes 256 consecutive rows at a time; their texts are one contiguous span of chars_dev.  A span of at most 28 KiB is put together in LDS, a row
 * per lane, and leaves in 16-byte stores aligned to the output; a longer one (a long string among the rows) is written by its lanes straight to chars_dev.  Which of the
 * two follows from offsets_dev alone.  A double is converted twice, once for its length and once for its digits. */
int sjgpu_write_records_device(sjgpu_ctx *ctx, const sjgpu_write_column *columns, uint32_t K, uint32_t n, uint32_t flags,
                               void *offsets_dev /* n + 1 u32 */, void *status_dev /* n bytes */, void *chars_dev, uint64_t chars_cap,
                               void *counts_dev /* 4 u64 */, void *stream, uint64_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif
