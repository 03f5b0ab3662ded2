/* include/sjgpu_pretty.h -- C-ABI of libsjgpu.so, cells as INDENTED JSON text: every cell of one row serialised on the device the way simdjson::prettify(element)
 * serialises an element -- the third of the reference's three ways out of a parsed element (include/simdjson/dom/serialization.h: to_string, minify, prettify), the one
 * for people: record 17 of a stream, every document of an NDJSON stream as a block, one irregular column kept readable.
 * An extension of include/sjgpu_json_wide.h, which it does not change; a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_PRETTY_H
#define SJGPU_PRETTY_H

#include "sjgpu_json_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched `simdjson::prettify(e)` rooted at cells (sjgpu_json.hip, sjgpu_json_wide.hip: the PRETTY instantiations of their kernels) -------------------------
 * sjgpu_prettify_cells_device: the sixteen parameters of sjgpu_serialize_cells_device (include/sjgpu_json.h) in its order, and ITS CONTRACT, WORD FOR WORD -- the
 * statuses and which sub-tapes are NOT WELL FORMED; SJGPU_E_BADARG before anything is read or enqueued; SJGPU_E_OVERFLOW with *bytes_out saying what is needed, offsets
 * and status complete and nothing written to chars_dev, chars_cap == 0 with a null chars_dev being how to ask; CAPACITY (1) beyond 32 bits with the 64-bit total;
 * rows == 0 and docs == 0; nothing written or read outside the ranges named there; the texts complete on return.  THE TEXT IS THE ONLY DIFFERENCE.
 * sjgpu_prettify_cells_wide_device: the same for the call of include/sjgpu_json_wide.h -- one lane per tape word --, SJGPU_E_RANGE and the hand-off of a root that nests
 * 64 or more levels below itself to the one-lane walk included.  Its outputs are sjgpu_prettify_cells_device's bit for bit on every input, well formed or not.
 *
 * The bytes of row r are exactly what the reference's simdjson::prettify(e) returns for the element e that cell r describes (pretty_formatter driven by
 * string_builder::append(element), include/simdjson/dom/serialization-inl.h).  Scalars, strings and keys are the bytes of sjgpu_serialize_cells_device; the layout:
 * let a be the number of containers open around a word inside the cell (the cell's own container has a = 0) and l = a mod 16.  The indent step is 4; prettify() has no
 * knob for it and neither has this call.
 *   a container that has children, l != 15   its bracket and \n; every child behind 4 (l + 1) blanks, siblings separated by ,\n; a key as "key": with ONE blank behind
 *                                            the colon; the close is \n, 4 l blanks, the bracket
 *   an empty container                       [] or {}, nothing between, at any a
 *   a container with l = 15                  (the 16th, 32nd, ... level) FLAT: the reference leaves its loop there and starts afresh for every child.  The bracket, the
 *                                            children separated by a bare , and keys as "key": WITHOUT the blank, the bracket, no newline in front of it.  Every child is
 *                                            written as an element of its own: its children have l = 0 again, and it ENDS WITH A \n OF ITS OWN, a scalar too.
 *                                            Reproduced, not repaired.
 *   every served cell                        ends with ONE \n: a scalar root is its text and \n, a string cell its quoted text and \n.  A refused cell has length 0
 *                                            and no newline.
 * So an indent never exceeds 60 blanks, and json.loads of a cell's text is json.loads of its minified text.
 *
 * Every byte of the layout is a function of ONE WORD AND THE STATE IN FRONT OF IT: the depth, "the parent is an object", "this is a key", "this is the first child", and
 * for a closing word whether the word in front of it opened it.  The one-lane walk carries the depth it has; the wide call's count has the depth, the kind and the
 * parity per word already and looks at one word more.
 *
 * Cost, not hidden:
 *   The launches, the waits for the stream and the workspace are the minify twin's, exactly: five launches and one wait in front of the fill for the narrow call, about
 *   two dozen and two waits for the wide one, one wait behind the fill for both; 10 bytes per slot of the range space for the wide call -- the byte that held the
 *   prefix character holds the layout's code --, and the 504 bytes per resident lane for nesting beyond 64 levels.  Nothing grows.
 *   The TEXT grows: a newline and an indent per child, a blank per field.  The narrow call writes an indent sixteen, eight and four blanks at a time, and so does a
 *   lane of the wide call; everything else leaves one lane as it does there.
 *   A STRING IS STILL ONE LANE'S WORK, in both passes and in both calls.  A double is converted twice.  A root that is one large document is ONE lane's work in the
 *   narrow call.
 * WHICH CALL TO TAKE IS THE CALLER'S DECISION, by the rule of include/sjgpu_json_wide.h: one large root or a few -- the wide call; rows of many small cells -- the narrow
 * one.  Measured on an MI355X beside the minify twins on the same rows (profiles/pretty_text.txt; medians of 20), narrow / wide:
 *   344 727 small containers, 3.48 times the bytes: 0.488 against 0.409 ms / 1.303 against 1.266 ms; the 344 727 whole records of one document, 1.68 times the bytes:
 *   2.969 against 2.822 / 5.499 against 5.411 ms; the 862 116 roots of an NDJSON stream, 1.15 times: 2.091 against 2.031 / 2.680 against 2.638 ms; 1 048 576 doubles:
 *   0.181 against 0.176 / 0.332 against 0.331 ms.  ONE cell, the root of one twitter-like document, 2.2 times the bytes: 64 KiB 13.4 against 12.3 ms / 0.179 against
 *   0.177 ms; 1 MiB 215 against 195 ms / 0.214 against 0.215 ms; 16 MiB, wide, 0.390 against 0.383 ms; 256 MiB, wide, 3.98 against 3.87 ms (435.5 MB, 109 GB/s of text).
 *   1.00 to 1.19 times the twin's time for 1.05 to 3.48 times its bytes: neither call is bound by the bytes it stores, so the yardstick "the twin scaled by bytes" is
 *   met with room everywhere. */
int sjgpu_prettify_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev /* rows + 1 u32 */,
                                void *status_dev /* rows bytes */, void *chars_dev, uint64_t chars_cap, void *stream, uint64_t *bytes_out);
int sjgpu_prettify_cells_wide_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                     uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev /* rows + 1 u32 */,
                                     void *status_dev /* rows bytes */, void *chars_dev, uint64_t chars_cap, void *stream, uint64_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif
