/* include/sjgpu_query.h -- C-ABI of libsjgpu.so, queries over device tapes: K JSON pointers (RFC 6901) resolved against the root of every
 * document of a tape stream, typed columns out; one string column turned into offsets + characters.
 * An extension of include/sjgpu_stream.h (the tapes, string records and document table it reads are declared there); a header of its own
 * so that programs built against sjgpu.h or sjgpu_stream.h alone are not rebuilt for it. */
#ifndef SJGPU_QUERY_H
#define SJGPU_QUERY_H

#include "sjgpu_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched dom::element::at_pointer over resident tapes (sjgpu_query.hip) -----------------------------------------------------
 * Cell (pointer k, document d) is what dom::parser::parse(bytes of document d).at_pointer(pointer k) gives in the reference
 * (include/simdjson/dom/element-inl.h:410-446, object-inl.h:104-147 and :246-254, array-inl.h:94-121 and array::at,
 * jsonpathutil.h:20-50): the element found, or INCORRECT_TYPE 17, INDEX_OUT_OF_BOUNDS 19, NO_SUCH_FIELD 20, INVALID_JSON_POINTER 22.
 * The reference's rules are lazy -- a token's defect is reported only when the walk reaches that token, and which defect it is depends
 * on the element that stands there: an object reads the token as a key (`~0`, `~1` unescaped; any other `~`, a last one included, is
 * 22 before any lookup; the FIRST field whose unescaped key has the token's length and bytes wins, else 20), an array as an index
 * (`-` as the whole rest 19; a non-digit 17; a leading zero in front of more digits, or no digit, 22; an index beyond size_t or beyond
 * the elements 19), a scalar answers a non-empty rest with 20, or with 22 when the first `~` of the rest is malformed.  Only a
 * non-empty pointer that does not begin with `/` is 22 for every document.  The empty pointer is the root.
 *
 * pointers: K byte strings back to back in HOST memory, pointer_lens[k] their lengths (K <= 64, each <= 1024 bytes, at most 32 tokens).
 * tape_dev[0 .. tape_words) / string_buf_dev[0 .. string_bytes) / docs_dev[0 .. docs]: what sjgpu_stage2_many_device delivered for
 * `docs` documents (docs + 1 table entries).  The output of sjgpu_stage2_device is served by a table of two entries
 * {0, 0, 0, 0} {n, len, words, bytes}.
 * value_dev: K * docs 64-bit words, row k = pointer k.   tag_dev: K * docs bytes, the same order.
 *   tag_dev[k * docs + d]    success: the tape tag of the element found, one of { [ " l u d t f n;  failure: 17, 19, 20 or 22 (every
 *                            code is below '"' = 34: one byte says both)
 *   value_dev[k * docs + d]  l, u, d: the tape's second word unchanged (int64, uint64, the bits of the double)
 *                            t, f, n: 1, 0, 0
 *                            "      : (length << 32) | offset into string_buf_dev of the string's first character (the record's
 *                                     payload + 4, made absolute with the table's string_begin)
 *                            {, [   : (absolute index behind its closing word << 32) | absolute index of its opening word: the
 *                                     sub-tape is the slice tape_dev[low .. high)
 *                            failure: 0
 * Every cell is written; nothing is written outside value_dev[0 .. K * docs) and tag_dev[0 .. K * docs) (rows of tag_dev begin at any
 * byte); nothing is read outside tape_dev[0 .. tape_words), string_buf_dev[0 .. string_bytes) and the docs + 1 table entries: a tape
 * word or a payload that points elsewhere ends the cell's walk as "not found" instead of being followed.
 * Cost: one lane walks one cell, consecutive lanes consecutive documents of one pointer.  A cell costs time linear in the SIBLINGS it
 * passes on the levels of its path -- the fields in front of the key, the elements in front of the index; a sibling is stepped over
 * in O(1) whatever it contains, so subtrees that are skipped cost nothing.  A single level of millions of siblings is walked by one
 * lane: there is no cooperative walk.
 * tape_dev and value_dev 8-byte aligned, docs_dev 16-byte; a null pointer, K > 64, a pointer beyond the limits, or a table whose
 * tape_begin / string_begin run backwards or end beyond tape_words / string_bytes: SJGPU_E_BADARG.  K == 0 or docs == 0: 0, nothing
 * written.  Returns 0 or a negative SJGPU_E_*; what a cell meets is in its tag, never in the return value.
 * Synchronisation: the table check reads one word back, so the call waits for what `stream` held when it was called and for that
 * check; the walk itself is only enqueued -- the columns are complete when `stream` has reached the end of the call's work.  The
 * compiled pointers go up through a block the context owns: a call waits for the walk of the context's previous call before it
 * writes that block again.
 * Destroying a context: sjgpu_ctx_destroy (sjgpu.h) waits for the context's OWN stream only, never for a stream the caller passed to
 * a *_device call, and then parks the context, workspaces included, for the next sjgpu_ctx_create.  The caller must therefore have
 * waited for every stream that still holds work of the context -- an enqueued walk of this call, say -- before it destroys it. */
int sjgpu_at_pointers_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes,
                             const void *docs_dev, uint32_t docs, const uint8_t *pointers, const uint32_t *pointer_lens, uint32_t K,
                             void *value_dev, void *tag_dev, void *stream);

/* ---- one column -> offsets + characters ------------------------------------------------------------------------------------------
 * value_row_dev / tag_row_dev: one row (docs cells) of the columns above.  A cell whose tag is '"' contributes its bytes, every other
 * cell nothing (and so does a string cell that points outside string_buf_dev[0 .. string_bytes)).
 *   offsets_dev[0 .. docs]  u32, the exclusive sum of the lengths; offsets_dev[docs] == *bytes_out
 *   chars_dev               the characters back to back; neither the records' length words nor their terminators
 * chars_cap too small: SJGPU_E_OVERFLOW, *bytes_out says what is needed, the offsets are complete and nothing is written to chars_dev.
 * A total beyond 32 bits: CAPACITY (1) -- the total out-parameter holds
 * the 64-bit total, status and counts are complete, offsets_dev is written but meaningless (its 32-bit words wrapped) and nothing is written to the data arrays.
 * docs == 0: 0 with offsets_dev[0] = 0.  offsets_dev 4-byte, value_row_dev 8-byte aligned
 * (SJGPU_E_BADARG otherwise); chars_dev and tag_row_dev begin at any byte.  The copy is chunk-parallel (16 bytes of the OUTPUT per lane,
 * its cell found by a search in the offsets): one long string among short ones is shared by as many lanes as it has chunks.
 * Waits for the stream: the total is read back. */
int sjgpu_gather_strings_device(sjgpu_ctx *ctx, const void *string_buf_dev, uint64_t string_bytes, const void *value_row_dev, const void *tag_row_dev,
                                uint32_t docs, void *offsets_dev /* docs + 1 u32 */, void *chars_dev, uint64_t chars_cap, void *stream, uint64_t *bytes_out);

#ifdef __cplusplus
}
#endif
#endif
