/* include/sjgpu_fields.h -- C-ABI of libsjgpu.so, map columns over device tapes: the FIELDS of the object each cell of one row describes -- keys as
 * string cells, values as cells, one ragged pair of rows (Arrow's map<string, value>) -- and the size() of each cell's container.
 * An extension of include/sjgpu_cast.h, include/sjgpu_lists.h and include/sjgpu_rows.h (the cell encoding, the root cells and the tapes, string records
 * and document table it reads are declared there, in include/sjgpu_query.h and in include/sjgpu_stream.h); a header of its own so that programs built
 * against the other headers are not rebuilt for it. */
#ifndef SJGPU_FIELDS_H
#define SJGPU_FIELDS_H

#include "sjgpu_cast.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched `for (dom::key_value_pair f : dom::object(e))` rooted at cells (k_rows_locate, k_object_fields_count, k_object_fields_fill) -----------
 * Every other query call needs the caller to know the keys; `$.*` gives an object's values and drops its keys.  Here the keys are data: the reference's
 * iteration over an object (include/simdjson/dom/object-inl.h:85-96, the iterator :309-325) for every cell of a row at once.
 *
 * tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows: those of
 * sjgpu_at_paths_from_cells_device, word for word -- one row of `rows` cells in the encoding of sjgpu_at_pointers_device over the SAME tapes, both root
 * pointers null only when rows is 0 --, with its alignments, null rules and refusals.
 *   offsets_dev[0 .. rows]   u32, the exclusive sum of the roots' field counts; offsets_dev[rows] == *fields_out.  It keeps the parent row of every field.
 *   status_dev[r]            by the root cell r:
 *     {  agreeing with the tape (the test of sjgpu_at_pointers_from_cells_device)      0; its fields are slots offsets[r] .. offsets[r + 1], in the
 *                                                                                      reference's iteration order (the tape's), duplicate keys included
 *     [  agreeing with the tape, and " l u d t f n                                     17 (element::get_object, element-inl.h:326-334), no field
 *     17, 19, 20, 22                                                                   that code, forwarded (element-inl.h:52-55), no field
 *     { or [ that disagrees with the tape, or any byte that is no tag and no code      20, no field
 *   slot i:
 *     key_tag_dev[i]     '"'
 *     key_value_dev[i]   (length << 32) | the absolute offset of the key's first byte in string_buf_dev: the string cell of the key's tape word, so a key
 *                        with NUL or escaped characters is its unescaped bytes
 *     value_dev[i], tag_dev[i]   the field's value in the cell encoding, offsets and indices absolute
 * Composition: key_value_dev / key_tag_dev[0 .. *fields_out) is a row of string cells, a valid input of sjgpu_gather_strings_device (the keys as offsets +
 * characters) and of sjgpu_cast_cells_device; value_dev / tag_dev[0 .. *fields_out) is a row of cells, a valid input of every *_from_cells call (this one
 * included: a second nesting level is one more call) and of the cast.
 * field_cap too small: SJGPU_E_OVERFLOW, *fields_out says what is needed, offsets_dev and status_dev are complete and nothing is written to the four cell
 * arrays.  A total beyond 32 bits: CAPACITY (1) -- the total out-parameter holds
 * the 64-bit total, status and counts are complete, offsets_dev is written but meaningless (its 32-bit words wrapped) and nothing is written to the data arrays.
 * rows == 0: 0 with offsets_dev[0] = 0.  docs == 0 is served: no container root has a document.
 * SJGPU_E_BADARG, before anything is read or enqueued: a null pointer (status_dev may be null when rows is 0, the four cell arrays when field_cap is 0),
 * tape_dev, root_value_dev, key_value_dev or value_dev not 8-byte, docs_dev not 16-byte, offsets_dev not 4-byte aligned (status_dev, the tag rows and
 * root_tag_dev begin at any byte), tape_words or string_bytes beyond 32 bits, docs or rows + 1 beyond 0xFFFFFFF0; and a table whose tape_begin /
 * string_begin run backwards or end beyond tape_words / string_bytes.
 * The count does not walk: an object's opening word carries its field count in 24 bits (tape_ref::scope_count), and that is the root's count.  The
 * reference saturates it at 0xFFFFFF; only a root whose count field reads 0xFFFFFF is walked to be counted (bounded by the cell's high half cut to the
 * document's end).  The fill walks once.  It never writes at or beyond offsets[r + 1], whatever the tape says, and slots of a root it did not reach (a
 * count field that claims more fields than the walk finds -- no tape of sjgpu_stage2_many_device has one) are written as key tag 20, value tag 20 and
 * both words 0: every slot in [0, *fields_out) is written.
 * Nothing is read outside tape_dev[0 .. tape_words), string_buf_dev[0 .. string_bytes), the docs + 1 table entries and the rows root cells.  Nothing is
 * written outside offsets_dev[0 .. rows], status_dev[0 .. rows) and the four cell arrays' [0 .. *fields_out).  The outputs must not overlap the roots.
 * Returns 0, CAPACITY or a negative SJGPU_E_*; what a root is shows in its status, never in the return value.
 * Four launches: locate, count, the scan with its 64-bit total, fill.  Waits for the stream: the total is read back, and the rows are complete on return.
 * Cost, not hidden: one lane per root; the count is one table search and one tape word per root, the fill linear in the fields of its root with four
 * stores per field.  A root that is one object of a million fields is ONE lane's work. */
int sjgpu_object_fields_from_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes,
                                          const void *docs_dev, uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows,
                                          void *offsets_dev /* rows + 1 u32 */, void *status_dev /* rows bytes */, void *key_value_dev, void *key_tag_dev,
                                          void *value_dev, void *tag_dev, uint64_t field_cap, void *stream, uint64_t *fields_out);

/* ---- batched dom::object::size() / dom::array::size() of cells (k_rows_locate, k_cell_sizes) --------------------------------------------------------
 * size_dev[r] (u32, 4-byte aligned) / code_dev[r] (a byte, at any address), by the root cell r:
 *   { or [ agreeing with the tape      the count field of its opening word, code 0.  This is the value dom::object::size() / dom::array::size() return --
 *                                      they read the same 24 bits --, the saturated 0xFFFFFF of a container with 16 777 215 children or more included
 *   " l u d t f n                      0, code 17
 *   17, 19, 20, 22                     0, that code
 *   anything else                      0, code 20
 * O(1) per cell: no walk.  The tapes, the table, the roots, their alignments and refusals as above (string_buf_dev is not needed); rows == 0 is 0 and
 * nothing is done.  Only enqueues on `stream` behind the table check (which waits, as in sjgpu_at_pointers_from_cells_device); the roots' verdicts lie in
 * a block the context owns, guarded by the event of the query calls. */
int sjgpu_cell_sizes_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *docs_dev, uint32_t docs, const void *root_value_dev,
                            const void *root_tag_dev, uint32_t rows, void *size_dev /* rows u32 */, void *code_dev /* rows bytes */, void *stream);

#ifdef __cplusplus
}
#endif
#endif
