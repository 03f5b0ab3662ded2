/* include/sjgpu_lists.h -- C-ABI of libsjgpu.so, list columns over device tapes: K JSONPaths with wildcards resolved against the CELLS
 * of one row -- the elements a query found --, one RAGGED column out whose cells are the rows of that table (Arrow's list<>).
 * An extension of include/sjgpu_rows.h and include/sjgpu_paths.h (the cell encoding, the level program, the root cells and the tapes,
 * string records and document table it reads are declared there, in include/sjgpu_query.h and in include/sjgpu_stream.h); a header of
 * its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_LISTS_H
#define SJGPU_LISTS_H

#include "sjgpu_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched dom::element::at_path_with_wildcard rooted at cells (k_rows_locate, k_at_paths_rooted in sjgpu_query.hip) ------------
 * The reference's users write `for (element e : doc.at_path_with_wildcard(p)) for (element h : e.at_path_with_wildcard(q)) ...`:
 * dom::element::at_path_with_wildcard works on any element (include/simdjson/dom/element-inl.h:448-459) and on a failed result
 * (:139-142).  The flat path p + q from the document's root finds the same elements, but its cells are per DOCUMENT: which row each
 * match belongs to is lost.  Here the cells are the rows: the hashtags of each status, the indices of each hashtag.
 *
 * root_value_dev[0 .. rows) / root_tag_dev[0 .. rows): one row of cells in the encoding of sjgpu_at_pointers_device, as for
 * sjgpu_at_pointers_from_cells_device -- a row of its output or of sjgpu_at_pointers_device's, the flattened value_dev / tag_dev of
 * either paths call or of this call (rows = *matches_out) -- over the SAME tape_dev, string_buf_dev and docs_dev (docs + 1 table
 * entries).  Both may be null when rows is 0 (a call that found nothing had no room to give).
 * paths, path_lens, K, offsets_dev, status_dev, value_dev, tag_dev, match_cap, matches_out: the contract of sjgpu_at_paths_device, word
 * for word, with `rows` in the place of `docs`: the level program of sj_path_program.h and its limits (K <= 64, a path <= 1024 bytes,
 * at most 32 levels, 32 pointer tokens, 8 wildcards), the lazy pointer rules, the alignments and refusals.
 * Cell c = k * rows + r is what E.at_path_with_wildcard(path k) gives in the reference, E the element root cell r describes:
 *   offsets_dev[0 .. K * rows]  u32, the exclusive sum of the cells' match counts; offsets_dev[K * rows] == *matches_out
 *   status_dev[c]               0, 17, 19, 20 or 22; a cell with a status other than 0 has no matches
 *   value_dev[i], tag_dev[i]    match i in the cell encoding, offsets and indices absolute in string_buf_dev / tape_dev
 * By the tag of the root cell:
 *   { or [ agreeing with the tape (the test of sjgpu_at_pointers_from_cells_device: the low 32 bits c lie inside a document behind
 *                      its root word, tape_dev[c] carries the tag and tape_begin[d] + its low 32 bits is the cell's high half)
 *                      the walk of sjgpu_at_paths_device with the cell's opening word in the place of the document's root.  A code
 *                      at depth 0 (17, 19, 20, 22) is the cell's status, deeper codes are swallowed.  No level is followed beyond the
 *                      cell's high half or the document's end.
 *   { or [ that disagrees with the tape, or any byte that is no tag and no code
 *                      status 20, no match, nothing followed.
 *   " l u d t f n      status 0, no match, for every path, the empty and the malformed ones included (element-inl.h:456-457).
 *   17, 19, 20, 22     that code as status, no match, for every path (element-inl.h:139-142).
 * Composition: value_dev / tag_dev[0 .. *matches_out) is ONE flattened pair of rows in the cell encoding: a valid input of this call
 * (a third nesting level is one more call), of sjgpu_at_pointers_from_cells_device and of sjgpu_gather_strings_device.
 * match_cap too small: SJGPU_E_OVERFLOW, *matches_out says what is needed, offsets_dev and status_dev are complete and nothing is
 * written to value_dev or tag_dev.  A total beyond 32 bits: CAPACITY (1) -- the total out-parameter holds
 * the 64-bit total, status and counts are complete, offsets_dev is written but meaningless (its 32-bit words wrapped) and nothing is written to the data arrays.
 * K == 0 or rows == 0: 0 with offsets_dev[0] = 0.  docs == 0
 * is served: no container root has a document.  SJGPU_E_BADARG: a null pointer (value_dev and tag_dev may be null when match_cap is 0),
 * tape_dev, root_value_dev or value_dev not 8-byte, docs_dev not 16-byte, offsets_dev not 4-byte aligned (status_dev, tag_dev and
 * root_tag_dev begin at any byte), K or a path beyond the limits, K * rows + 1 beyond 0xFFFFFFF0 -- refused before anything is read
 * or enqueued --, or a table whose tape_begin / string_begin run backwards or end beyond tape_words / string_bytes.
 * Nothing is read outside tape_dev[0 .. tape_words), string_buf_dev[0 .. string_bytes), the docs + 1 table entries and the rows root
 * cells.  Nothing is written outside offsets_dev[0 .. K * rows], status_dev[0 .. K * rows) and value_dev / tag_dev[0 .. *matches_out):
 * the fill never writes at or beyond offsets[c + 1], whatever the tape says.  The outputs must not overlap the roots.
 * Returns 0, CAPACITY or a negative SJGPU_E_*; what a cell meets is in its status, never in the return value.
 * Four launches: locate, count, the scan with its 64-bit total, fill.  Waits for the stream: the total is read back, and the columns
 * are complete on return.
 * Cost, not hidden: one lane walks one cell, twice (count, then fill); consecutive lanes take consecutive roots of one path (K rows
 * of ceil(rows / 256) workgroups, the path's levels, tokens and keys in LDS once per workgroup).  A cell costs time linear in the
 * siblings it passes and in the elements it visits under its wildcards.  The locate step runs once per ROOT, whatever K is (log2(docs)
 * table reads and one tape word); its verdicts take 4 bytes per root in a block the context owns (grown on demand; its failure is
 * SJGPU_E_NOMEM) and are shared by all K paths and by both passes.  A root that is one array of a million elements is ONE lane's work;
 * a breadth-first rooted variant that would share it among lanes is not built. */
int sjgpu_at_paths_from_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes,
                                     const void *docs_dev, uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows,
                                     const uint8_t *paths, const uint32_t *path_lens, uint32_t K,
                                     void *offsets_dev /* K * rows + 1 u32 */, void *status_dev /* K * rows bytes */,
                                     void *value_dev, void *tag_dev, uint64_t match_cap, void *stream, uint64_t *matches_out);

#ifdef __cplusplus
}
#endif
#endif
