/* include/sjgpu_json_wide.h -- C-ABI of libsjgpu.so, cells as JSON text, BREADTH FIRST: sjgpu_serialize_cells_device (include/sjgpu_json.h) with one lane per tape
 * word where that call has one lane per cell -- what makes minify(doc) / to_string(element) of ONE large parsed document, of `$.statuses`, or of any large sub-tree a
 * query found a wide piece of work.
 * An extension of include/sjgpu_json.h, which it does not change; a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_JSON_WIDE_H
#define SJGPU_JSON_WIDE_H

#include "sjgpu_json.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the words of the located container roots laid end to end, plus one slot per other root, exceed 0xFFFFFFF0: take sjgpu_serialize_cells_device, or split the row */
#define SJGPU_E_RANGE (-8)

/* ---- batched `simdjson::minify(e)` rooted at cells, one lane per tape word (sjgpu_json_wide.hip) ------------------------------------------------------------------
 * The sixteen parameters of sjgpu_serialize_cells_device in its order, and ITS CONTRACT, WORD FOR WORD: on every input, well formed or not, offsets_dev[0 .. rows],
 * status_dev, chars_dev[0 .. *bytes_out) and *bytes_out are bit for bit what that call leaves; so are the returns 0, SJGPU_E_OVERFLOW and CAPACITY with what each
 * leaves behind, the SJGPU_E_BADARG refusals before anything is read, rows == 0 and docs == 0, and "nothing written outside, nothing read outside".  Which sub-tapes
 * are NOT WELL FORMED is the same verdict: every condition of that header is a predicate on one word and the state in front of it, and the state computed in parallel
 * equals the walk's up to the first word that violates one.
 *
 * One refusal more.  The RANGE SPACE of a call is the words of its located container roots (high - low each, overlapping and repeated roots counted as often as they
 * are asked for) plus ONE slot for every other root -- a scalar, a code, a cell that disagrees with the tape.  The scans index it with 32-bit words, as everywhere:
 *   SJGPU_E_RANGE   the range space exceeds 0xFFFFFFF0 slots.  Found after the roots were located; status_dev is complete (the narrow call's statuses, made by its
 *                   count), nothing else is written, *bytes_out is 0.  Take sjgpu_serialize_cells_device, or split the row.
 *
 * How it works: the heads of the range space (a number's second word is none) by a running maximum, the nesting depth by a sum, and whether a string is a key and
 * which of , and : precedes a word by ONE exclusive scan of four 64-bit words per slot (two bits per nesting level: "this level is an object", "an even number of
 * words was seen at it"); then a length per head, their scan, and one lane per head writing its own bytes.  A root that nests 64 or more levels below itself is handed,
 * whole, to the one-lane walk of the narrow call.  The number of launches depends neither on the data nor on the nesting depth.
 *
 * Cost, not hidden:
 *   Workspace (the context's, grown on demand; its failure is SJGPU_E_NOMEM): 10 bytes per slot of the range space (head 1, depth 4, length / offset 4, prefix 1) plus
 *   44 bytes per 256 slots and the scans' block sums, 16 bytes per root, and the narrow call's 504 bytes per resident lane of the lanes that walk deep roots (at most
 *   63 MiB): the root of one 256 MiB twitter-like document, 22.6 M words, asks for 0.23 GB.
 *   The call WAITS FOR THE STREAM TWICE before the fill -- the size of the range space is read back to size the workspace, then the total -- and once more behind
 *   the fill: the texts are complete on return.  About two dozen launches, whatever the rows hold, against the narrow call's five.
 *   A STRING IS STILL ONE LANE'S WORK, in both passes: a cell that is one 100 MB string is as slow here as there.  A double is converted twice.
 *   Bytes leave one lane at a time, straight to chars_dev; a workgroup's span is not staged.
 * WHICH CALL TO TAKE IS THE CALLER'S DECISION; nothing chooses automatically.  Measured on an MI355X (profiles/json_text_wide.txt; medians of 20):
 *   ONE cell, the root of one twitter-like document: this call wins at every size measured, from 64 KiB on -- 0.185 ms against 12.3 ms at 64 KiB, 0.196 ms against
 *   195 ms at 1 MiB, 0.40 ms against 3.16 s at 16 MiB; 256 MiB take 3.9 ms (51 GB/s of text, 32 times sjgpu_minify_device over the source).  A call costs about
 *   0.18 ms whatever it holds.
 *   Rows of many small cells: the NARROW call wins on every leg -- 344 727 small containers 0.45 ms against 1.28 ms here, the 344 727 whole records of one document
 *   2.82 against 5.41 ms, the 862 116 roots of an NDJSON stream 2.03 against 2.64 ms, 1 048 576 doubles 0.19 against 0.34 ms. */
int sjgpu_serialize_cells_wide_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                      uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev /* rows + 1 u32 */,
                                      void *status_dev /* rows bytes */, void *chars_dev, uint64_t chars_cap, void *stream, uint64_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif
