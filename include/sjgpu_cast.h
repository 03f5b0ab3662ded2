/* include/sjgpu_cast.h -- C-ABI of libsjgpu.so, typed getters over a column: get<T> asked of every CELL of a row -- values, a validity
 * bitmap and a code per cell out (Arrow's layout) --, and the census of a row's tags a loader picks T from.
 * An extension of include/sjgpu_lists.h, include/sjgpu_rows.h, include/sjgpu_paths.h and include/sjgpu_query.h (the cell encoding is
 * declared there); a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_CAST_H
#define SJGPU_CAST_H

#include "sjgpu_lists.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched dom::element::get<T> over cells (k_cast_cells, k_cell_kinds in sjgpu_cast.hip) ----------------------------------------
 * The reference's users write `doc.at_pointer("/id").get<int64_t>()`: the getters of include/simdjson/dom/element-inl.h:219-316
 * (get_bool, get_string, get_uint64, get_int64, get_double; get_array / get_object :317-334), and on a failed result
 * simdjson_result<element>::get_* forwards the result's own code (:60-83).  The cells of the query calls are one step short of that:
 * a `u` cell read as int64 goes negative, an `l` read as double is a bit pattern.  Here the rules run on the device, cell by cell.
 *
 * value_dev / tag_dev: K rows of n cells in the encoding of sjgpu_at_pointers_device, cell c = k * n + i (indices are 64 bits wide:
 * K * n may pass 2^32) -- a K-row output of sjgpu_at_pointers_device or sjgpu_at_pointers_from_cells_device, or, with K = 1, the
 * flattened value_dev / tag_dev of any paths call.  K <= 64, n any uint32_t.  value_dev 8-byte aligned, rows of tag_dev begin at any
 * byte.  Neither call reads the tape or the string buffer: a string, array or object getter hands the cell's word on.
 *
 * sjgpu_cast_cells_device: row k asks getters[k] (host memory, K bytes, each SJGPU_GET_*) of each of its cells.  With t the cell's
 * tag byte and w its word:
 *   getter                 code 0 for                       value written                                   otherwise
 *   SJGPU_GET_INT64        l; u with w <= INT64_MAX         w                                               u above: 18
 *   SJGPU_GET_UINT64       u; l with int64(w) >= 0          w                                               negative l: 18
 *   SJGPU_GET_DOUBLE       d; l; u                          w; the bits of double(int64_t(w)); of double(uint64_t(w)), both rounded
 *                                                           to nearest even as the host's cast rounds
 *   SJGPU_GET_BOOL         t; f                             1; 0
 *   SJGPU_GET_STRING       "                                w (offset and length, as sjgpu_gather_strings_device reads them)
 *   SJGPU_GET_ARRAY        [                                w
 *   SJGPU_GET_OBJECT       {                                w
 * Any other of the nine tags { [ " l u d t f n: INCORRECT_TYPE 17 (a null is 17 for every getter).  A byte in 1 .. 33 is a code the
 * cell already held (17, 19, 20, 22 from the query calls): it is forwarded unchanged as the cell's code.  Byte 0 and any byte >= 34
 * that is no tag (Z, r, } and ] among them; the reference answers 17 for a BIGINT, too): 17.  Every cell with a code other than 0
 * gets value 0.  NUMBER_OUT_OF_RANGE 18 comes from nowhere else.
 *   value_out_dev[c]   u64, K * n of them        code_out_dev[c]   one byte, K * n of them (rows begin at any byte)
 *   valid_out_dev      row k is W = ceil(n / 64) 64-bit words from word k * W; bit i % 64 of word i / 64 is (code == 0), the bits at
 *                      and beyond n in a row's last word are 0: Arrow's validity bitmap, least significant bit first, every row
 *                      8-byte aligned
 *   counts_out_dev     u32[k * 4 + 0] cells with code 0, [+ 1] cells whose tag is n, [+ 2] cells with code 18, [+ 3] cells whose tag
 *                      was a code in 1 .. 33
 * Every cell, bitmap word and count is written; nothing is written outside these four ranges.  value_out_dev may be exactly value_dev
 * and code_out_dev exactly tag_dev (each lane reads its cell before it writes it: the cast works in place); any other overlap of an
 * output with an input or with another output is not allowed.
 *
 * sjgpu_cell_kinds_device: the census of row k in kinds_dev[k * 16 ..], sixteen u32:
 *   [0 .. 8]   cells with the tags { [ " l u d t f n, in this order ([3] counts every l)
 *   [9]        l cells whose value is negative (a u word on a tape is above INT64_MAX by construction: with [3], [4] and [9] the
 *              choice between int64, uint64 and double needs no look at the values)
 *   [10 .. 13] cells with the codes 17, 19, 20, 22
 *   [14]       every other byte         [15] always 0
 *
 * Both calls.  SJGPU_E_BADARG, decided before anything is enqueued: ctx null; K > 64; value_dev, value_out_dev or valid_out_dev not
 * 8-byte aligned, kinds_dev or counts_out_dev not 4-byte aligned; with K > 0 a null kinds_dev, counts_out_dev or getters, or a getter
 * outside 1 .. 7; with K * n > 0 any other null pointer.  K == 0: 0, nothing written.  n == 0 with K > 0: the K rows of counts or
 * kinds are written as zeros and nothing else is.  Returns 0 or a negative SJGPU_E_*; what a cell meets is in its code.
 * Synchronisation: no host wait and no read-back; the outputs are complete when `stream` has reached the end of the call's work.
 * The getters travel as a by-value kernel argument of 64 bytes: no block of the context, no upload and no event is involved, and a
 * call does not wait for the context's previous query.
 * Cost, not hidden: both are elementwise and memory-bound.  The cast moves 18 bytes per cell (9 in, 9 out) and one bit; the census
 * reads 9.  One memset of 16 K (64 K) bytes and one launch of K rows of workgroups of 256 lanes (at most 2 048 over all rows), a lane
 * per cell, grid-stride; a wave's 64 consecutive cells are one bitmap word, which is the wave's ballot; the counts are popcounts of ballots,
 * summed per workgroup in LDS and added with one atomic per slot and workgroup -- none per cell.  A table of a few million cells is
 * launch-bound: the two calls cost two launches and two memsets however small n is. */
enum { SJGPU_GET_INT64 = 1, SJGPU_GET_UINT64 = 2, SJGPU_GET_DOUBLE = 3, SJGPU_GET_BOOL = 4,
       SJGPU_GET_STRING = 5, SJGPU_GET_ARRAY = 6, SJGPU_GET_OBJECT = 7 };

int sjgpu_cell_kinds_device(sjgpu_ctx *ctx, const void *value_dev, const void *tag_dev, uint32_t n, uint32_t K,
                            void *kinds_dev /* K * 16 u32 */, void *stream);

int sjgpu_cast_cells_device(sjgpu_ctx *ctx, const void *value_dev, const void *tag_dev, uint32_t n, uint32_t K,
                            const uint8_t *getters /* K bytes, HOST */,
                            void *value_out_dev /* K * n u64 */, void *code_out_dev /* K * n bytes */,
                            void *valid_out_dev /* K * ceil(n / 64) u64 */, void *counts_out_dev /* K * 4 u32 */, void *stream);

#ifdef __cplusplus
}
#endif
#endif
