/* include/sjgpu_rows.h -- C-ABI of libsjgpu.so, record tables over device tapes: K JSON pointers resolved against the CELLS of one row
 * -- the elements a query found --, typed columns aligned with those cells out.
 * An extension of include/sjgpu_paths.h and include/sjgpu_query.h (the cell encoding, the pointer rules and the tapes, string records
 * and document table it reads are declared there and in include/sjgpu_stream.h); a header of its own so that programs built against
 * the other headers are not rebuilt for it. */
#ifndef SJGPU_ROWS_H
#define SJGPU_ROWS_H

#include "sjgpu_paths.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched dom::element::at_pointer rooted at cells (k_rows_locate, k_at_pointers_rooted in sjgpu_query.hip) -------------------
 * The reference's users write `for (element e : doc.at_path_with_wildcard(p)) e.at_pointer(q)`: dom::element::at_pointer
 * (include/simdjson/dom/element-inl.h:410-446, with the object and array functions sjgpu_query.h cites) works on any element, and
 * on a child it is the recursion step of at_pointer on its parent -- doc.at_pointer(a).at_pointer(b) is doc.at_pointer(a + b)
 * whenever the first call succeeds.  K wildcard paths cannot be zipped into a table (a row that lacks a field contributes nothing
 * to a ragged column); K pointers asked of the cells of `$.statuses[*]` can: a row that lacks a field holds a code.
 *
 * root_value_dev[0 .. rows) / root_tag_dev[0 .. rows): one row of cells in the encoding of sjgpu_at_pointers_device -- a row of its
 * output, the flattened value_dev / tag_dev of sjgpu_at_paths_device or sjgpu_at_paths_wide_device (rows = *matches_out), or a row
 * of this call's own output -- over the SAME tape_dev, string_buf_dev and docs_dev (docs + 1 table entries).
 * pointers, pointer_lens, K: as for sjgpu_at_pointers_device (host memory, K <= 64, each <= 1024 bytes, at most 32 tokens, the lazy
 * token rules).
 * value_dev: K * rows 64-bit words, row k = pointer k.   tag_dev: K * rows bytes, the same order.  Cell k * rows + r is what
 * E.at_pointer(pointer k) gives in the reference, E the element root cell r describes, in the same encoding; a row of the output is
 * again a valid row of roots and a valid input of sjgpu_gather_strings_device.  By the tag of the root cell:
 *   { or [             the root's low 32 bits are the absolute index c of its opening word, its high 32 bits the absolute index behind
 *                      its closing word.  Its document is the d with tape_begin[d] < c < tape_begin[d + 1], found by a search in the
 *                      table; the walk of sjgpu_at_pointers_device starts at c instead of behind the document's root word and follows
 *                      no level beyond the cell's high half or the document's end.  A cell that disagrees with the tape -- c outside
 *                      every document or on a root word, the top byte of tape_dev[c] not the cell's tag, tape_begin[d] + the low 32
 *                      bits of tape_dev[c] not the cell's high half -- gives NO_SUCH_FIELD 20 for every pointer, and nothing is
 *                      followed.
 *   " l u d t f n      the empty pointer gives the root cell unchanged, value and tag, without a look at the tape or the string
 *                      buffer; any other pointer gives what a scalar answers: 22 when it does not begin with `/` or its first `~` is
 *                      malformed, else 20.
 *   17, 19, 20, 22     the same code with value 0 for every pointer: what simdjson_result<element>::at_pointer does with an error.
 *   any other byte     NO_SUCH_FIELD 20, value 0, for every pointer.
 * A non-empty pointer that does not begin with `/` is 22 for every root that is a scalar or a container cell that agrees with the tape.
 * Every cell is written; nothing is written outside value_dev[0 .. K * rows) and tag_dev[0 .. K * rows) (rows of tag_dev begin at
 * any byte); nothing is read outside tape_dev[0 .. tape_words), string_buf_dev[0 .. string_bytes), the docs + 1 table entries and the
 * rows root cells.  The outputs must not overlap the roots.
 * Cost: one lane walks one cell, consecutive lanes consecutive roots of one pointer (K rows of ceil(rows / 256) workgroups, the
 * pointer's tokens and keys in LDS once per workgroup, coalesced stores).  A cell costs time linear in the SIBLINGS it passes on the
 * levels of its pointer, as in sjgpu_at_pointers_device: a root that is one object of a million fields is one lane's work.  In front
 * of the walk one lane per ROOT, once per call whatever K is, classifies the root, finds its document with log2(docs) table reads
 * and compares the cell with one tape word (the locate step); the K lanes that share a root pay neither.  Its verdicts take 4 bytes
 * per root in a block the context owns (grown on demand; its failure is SJGPU_E_NOMEM).
 * tape_dev, root_value_dev and value_dev 8-byte aligned, docs_dev 16-byte; a null pointer, K > 64, a pointer beyond the limits, or a
 * table whose tape_begin / string_begin run backwards or end beyond tape_words / string_bytes: SJGPU_E_BADARG.  K == 0 or rows == 0:
 * 0, nothing written.  docs == 0 is served: no container root has a document.  Returns 0 or a negative SJGPU_E_*; what a cell meets
 * is in its tag, never in the return value.
 * Synchronisation: that of sjgpu_at_pointers_device.  The table check reads one word back, so the call waits for what `stream` held
 * when it was called and for that check; the locate step and the walk are only enqueued -- the columns are complete when `stream`
 * has reached the end of the call's work.  The compiled pointers and the roots' verdicts lie in a block the context owns: a call
 * waits for the walk of the context's previous call before it writes that block again. */
int sjgpu_at_pointers_from_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes,
                                        const void *docs_dev, uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows,
                                        const uint8_t *pointers, const uint32_t *pointer_lens, uint32_t K,
                                        void *value_dev /* K * rows u64 */, void *tag_dev /* K * rows bytes */, void *stream);

#ifdef __cplusplus
}
#endif
#endif
