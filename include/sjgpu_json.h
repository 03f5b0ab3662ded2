/* include/sjgpu_json.h -- C-ABI of libsjgpu.so, cells as JSON text: every cell of one row -- an object, an array or a scalar -- serialised on the device the way
 * simdjson::minify(element) / simdjson::to_string(element) serialise an element, into one `offsets` / `chars` pair (Arrow's utf8 layout, its `json` extension type):
 * what a loader keeps of a field that is too irregular to flatten.
 * An extension of include/sjgpu_dict.h and the headers below it (the cell encoding, the root cells and the tapes, string records and document table it reads are
 * declared there, in include/sjgpu_query.h and in include/sjgpu_stream.h); a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_JSON_H
#define SJGPU_JSON_H

#include "sjgpu_dict.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched `simdjson::minify(e)` rooted at cells (k_rows_locate, k_json_count, k_json_fill) ----------------------------------------------------------------
 * tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows: those of sjgpu_object_fields_from_cells_device, word for
 * word -- one row of `rows` cells in the encoding of sjgpu_at_pointers_device over the SAME tapes, both root pointers null only when rows is 0 --, with its alignments,
 * null rules and refusals.
 *
 * The bytes of row r are exactly what the reference's simdjson::minify(e) returns for the element e that cell r describes (include/simdjson/dom/serialization-inl.h,
 * mini_formatter):
 *   containers    { } [ ], a , between siblings, a : behind a key, no blanks; the fields in the tape's order, duplicate keys included
 *   t f n         true false null
 *   l u           the shortest decimal of the int64 / uint64, -9223372036854775808 and 18446744073709551615 included
 *   d             the reference's to_chars(double) (src/to_chars.cpp): the shortest digits that read back as the same double and the closest to it, a trailing .0 on
 *                 an integral value below 1e15, 0.000ddd down to 1e-4, otherwise d.ddde+XX / de-XX with a sign and at least two exponent digits; -0.0 is -0.0
 *   strings, keys the UNESCAPED bytes of the string buffer between quotes: " as \" and \ as \\, 0x08 0x09 0x0a 0x0c 0x0d as \b \t \n \f \r, every other byte up to
 *                 0x1f as \u00xx in lower-case hex, every other byte as it is -- a source \/ or é comes out as / and as the two UTF-8 bytes
 * A scalar root is served from the cell itself and needs no tape; a string cell is its quoted, escaped text.
 *   status_dev[r]   0 for a served cell; 17 / 19 / 20 / 22 forwarded from a cell that already held that code; 20, with length 0, for a { or [ root that disagrees
 *                   with the tape (the test of sjgpu_at_pointers_from_cells_device), a string cell outside string_buf_dev[0 .. string_bytes), any byte that is neither
 *                   a tag nor a code, and a sub-tape that is not well formed
 * A sub-tape is NOT WELL FORMED when, between the cell's opening word and its high index, it holds a tag outside { } [ ] " l u d t f n; a string word whose record
 * does not lie inside its document's part of the string buffer; a number without its second word; a double that is no finite number (no JSON text has one); a word
 * that is no string where an object expects a key, or an object that closes behind a key; a closing word that does not match -- not of the kind of the level it
 * closes, or not pointing back at an opening word of that kind that points just behind it --; more than 4 096 nesting levels below the root; or a walk that does not
 * end exactly at the cell's high index.  No tape of sjgpu_parse / sjgpu_stage2_many_device is any of that.  It is decided in the count, so the fill never meets it.
 *   offsets_dev[0 .. rows]   u32, the exclusive sum of the lengths; offsets_dev[rows] == *bytes_out
 *   chars_dev                the texts back to back, no terminators
 * The pair is Arrow's utf8 layout, and what the consumers of sjgpu_gather_strings_device's offsets / chars take.
 * chars_cap too small: SJGPU_E_OVERFLOW, *bytes_out says what is needed, offsets_dev and status_dev are complete and nothing is written to chars_dev; chars_cap == 0
 * with a null chars_dev is how to ask.  A total beyond 32 bits: CAPACITY (1) -- the total out-parameter holds
 * the 64-bit total, status and counts are complete, offsets_dev is written but meaningless (its 32-bit words wrapped) and nothing is written to the data arrays.
 * rows == 0: 0 with offsets_dev[0] = 0.  docs == 0 is served: no container root has a document.
 * SJGPU_E_BADARG, before anything is read or enqueued: a null pointer (status_dev may be null when rows is 0, chars_dev when chars_cap is 0), tape_dev or
 * root_value_dev not 8-byte, docs_dev not 16-byte, offsets_dev not 4-byte aligned (status_dev, chars_dev and root_tag_dev begin at any byte), tape_words or
 * string_bytes beyond 32 bits, docs or rows + 1 beyond 0xFFFFFFF0; and a table whose tape_begin / string_begin run backwards or end beyond tape_words / string_bytes.
 * Nothing is written outside offsets_dev[0 .. rows], status_dev[0 .. rows) and chars_dev[0 .. *bytes_out); nothing is read outside tape_dev[0 .. tape_words),
 * string_buf_dev[0 .. string_bytes), the docs + 1 table entries and the rows root cells.  The outputs must not overlap the inputs.
 * Returns 0, CAPACITY or a negative SJGPU_E_*; what a root is shows in its status, never in the return value.
 * Five launches: locate, count, the total, the scan, fill.  Waits for the stream: the total is read back, and the texts are complete on return.
 * Workspace: 16 bytes per workgroup, the scan's block sums and 504 bytes per resident lane (at most 512 workgroups of 256 lanes: 63 MiB) for nesting levels beyond 64.
 * Cost, not hidden: ONE LANE PER CELL, in both passes.  A lane walks its cell's words one after the other and writes its bytes itself -- eight at a time inside a
 * string that needs no escape, one at a time elsewhere --, so a row of many small cells runs wide and a root that is one 256 MiB document is ONE lane's work.  A double
 * is converted twice, once for its length and once for its digits.  Lanes of one wave whose cells differ in size wait for the longest. */
int sjgpu_serialize_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                 uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev /* rows + 1 u32 */,
                                 void *status_dev /* rows bytes */, void *chars_dev, uint64_t chars_cap, void *stream, uint64_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif
