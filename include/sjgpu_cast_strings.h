/* include/sjgpu_cast_strings.h -- C-ABI of libsjgpu.so, numbers held in strings: get_int64_in_string, get_uint64_in_string and
 * get_double_in_string asked of every CELL of a row -- values, a validity bitmap and a code per cell out, as sjgpu_cast_cells_device
 * gives them.  An extension of include/sjgpu_cast.h (the cells, the rows and the output shape are declared there); a header of its
 * own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_CAST_STRINGS_H
#define SJGPU_CAST_STRINGS_H

#include "sjgpu_cast.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched get_*_in_string over cells (k_cast_string_cells, k_cast_strings_exact in sjgpu_cast_strings.hip) ------------------------
 * Feeds written by JavaScript carry their 64-bit ids, prices and timestamps as strings: `"id_str": "505874924095815700"`.  The
 * reference's users write `value.get_int64_in_string()`: ondemand::value::get_int64_in_string, get_uint64_in_string and
 * get_double_in_string (include/simdjson/generic/ondemand/value-inl.h:62-82), whose rules are numberparsing::parse_integer_in_string,
 * parse_unsigned_in_string and parse_double_in_string (include/simdjson/generic/numberparsing.h:1266-1305, :1130-1177, :1626-1716).
 * sjgpu_cast_cells_device answers INCORRECT_TYPE for such a cell; here the string is read where it lies in the string buffer and parsed
 * on the device.
 *
 * value_dev / tag_dev, n, K <= 64, the alignments, value_out_dev / code_out_dev / valid_out_dev and the in-place rule (value_out_dev may
 * be exactly value_dev and code_out_dev exactly tag_dev, no other overlap) are those of sjgpu_cast_cells_device.  string_buf_dev /
 * string_bytes: the string buffer the cells' words point into (that of the parse the cells came from; any alignment).  The word of a
 * `"` cell is (length << 32) | offset, as sjgpu_gather_strings_device reads it.  getters: host memory, K bytes, row k asks getters[k]:
 * SJGPU_GETS_INT64, SJGPU_GETS_UINT64 or SJGPU_GETS_DOUBLE, optionally or-ed with the flag SJGPU_GETS_OR_NUMBER.
 *
 * The rule per cell, t its tag byte and w its word:
 *   t in 1 .. 33           a code the cell already held: forwarded, value 0
 *   t == '"', offset + length <= string_bytes
 *                          the reference's parse_*_in_string over the cell's `length` unescaped bytes followed by a closing quote.  The
 *                          end is the LENGTH: a `"` byte among the content is an ordinary non-digit.  Code 0: the value is the int64,
 *                          the uint64, or the 64 bits of the double.  Otherwise INCORRECT_TYPE 17 or NUMBER_ERROR 9 in the order the
 *                          reference makes its checks, value 0:
 *                            integers   no digit, or more than 19 (uint64: 20) digits: 17, BEFORE a leading zero followed by a digit: 9;
 *                                       then any byte behind the digits (`1.5`, `1e2`, `1 `): 9; then out of range: 17.  A `-` is no digit
 *                                       for the unsigned rule (`-0`: int64 0, uint64 17).  At most the first 22 bytes matter.
 *                            double     no digit first (the empty string, `-`, `+1`, ` 1`, `.5`, `NaN`, `Infinity`): 17; a leading zero
 *                                       followed by a digit, no digit behind the point, an exponent of no or of more than 19 digits
 *                                       (zeros count: `1e00000000000000000001` is 9), any byte behind the number: 9.  What is left is THE
 *                                       correctly rounded binary64 of the text (a zero mantissa: +-0.0 under every exponent; `-0` has the
 *                                       sign bit), 9 where it would be infinite (`1e309`).
 *   t == '"' pointing outside string_buf_dev[0 .. string_bytes): 17, nothing is read.
 *   any other tag, flag off: 17.  (The reference skips the first byte of a value that is no string unseen and so answers 9 for `123` and
 *                          `[1]`, 17 for `true`, `1.5` and `{}`: an accident of its implementation, not a rule, and not repeated here.)
 *   any other tag, flag SJGPU_GETS_OR_NUMBER on: the cells l, u and d are answered by the get<T> rule of sjgpu_cast_cells_device for the
 *                          same T (NUMBER_OUT_OF_RANGE 18 included), everything else is 17: the mixed column `"price": 12` / `"price": "12"`.
 *
 * counts_out_dev[k * 8 ..], eight u32 per row:
 *   [0] cells with code 0        [1] cells whose tag is n        [2] cells with code 9        [3] cells that held a code (1 .. 33)
 *   [4] cells refused for what they are: no string (flag off), neither a string nor a number (flag on); held codes are not among them
 *   [5] string cells decided by the exact road (below): under SJGPU_GETS_DOUBLE the strings of more than 32 bytes, whatever they hold, and
 *       the numbers of more than 19 significant digits; none under the integer getters
 *   [6] string cells that point outside the buffer        [7] always 0
 * Every cell, every bitmap word and every count is written; nothing is written outside the four output ranges.  No byte is read
 * outside string_buf_dev[0 .. string_bytes), whatever the base pointer's alignment, and none outside the two input rows.
 *
 * The difference from On-Demand.  On-Demand parses the RAW text of the document, so a 12 whose 2 is written as the escape
 * backslash-u-0032 is NUMBER_ERROR there.  A DOM holds
 * only the unescaped string, and that is what a cell points at: here the same field is 12.  This is what parse_*_in_string over
 * element.get_string() would give.  For every string written without a backslash the two agree bit for bit
 * (tests/golden/in_string.json holds the reference's answers for such strings only).
 *
 * Not here.  get_float_in_string: binary32 cannot be had by rounding the binary64 (the reference says so at parse_float), and this
 * library has no decimal-to-binary32 conversion.  Arrow utf8 columns (offsets + characters) as input: the call reads cells.
 *
 * SJGPU_E_BADARG, decided before anything is enqueued: ctx null; K > 64; value_dev, value_out_dev or valid_out_dev not 8-byte aligned,
 * counts_out_dev not 4-byte aligned; with K > 0 a null counts_out_dev or getters, or a getter whose low four bits are outside 1 .. 3 or
 * that has any bit but 0x10 above them; with K * n > 0 any other null pointer -- string_buf_dev only while string_bytes > 0.  K == 0: 0,
 * nothing written.  n == 0 with K > 0: the K * 8 counts are written as zeros and nothing else is.  Returns 0 or a negative SJGPU_E_*;
 * what a cell meets is in its code.
 * Synchronisation: the call only enqueues -- no host wait, no read-back; the outputs are complete when `stream` has reached the end of
 * the call's work.  The getters travel as a by-value kernel argument; no block of the context, no upload and no event is involved.
 * Cost, not hidden.  One memset of 32 K bytes and two launches.  The first kernel has the shape of sjgpu_cast_cells_device's (K rows
 * of workgroups of 256 lanes, at most 2 048 over all rows, a lane per cell, grid-stride; the ballot is the bitmap word, the counts are
 * popcounts) and adds, per string cell, one or two 16-byte loads at the string's own address: scattered short reads, which are bound
 * by the number of memory transactions, not by bytes.  It settles every integer and every double of at most 19 significant digits in
 * a string of at most 32 bytes.  The other doubles wait for the second kernel, which is always enqueued, leaves at once when no cell
 * of its row waits, and otherwise decides each waiting cell with exact big-integer arithmetic in LDS: the few, as on the
 * tape.  A 17-digit double never waits (0 of 1 048 576 reprs of random doubles did).
 * Measured on an MI355X (scripts/cast_strings_once.py, profiles/cast_strings.txt; medians of 20, rows of 18-digit ids under
 * SJGPU_GETS_INT64; SJGPU_GETS_DOUBLE costs 2 to 8 % more), beside sjgpu_cast_cells_device and sjgpu_gather_strings_device on the same row:
 *   one dense array document, strings 23 bytes apart      1 M cells  0.042 ms   1.2 x the cast   0.44 x the gather
 *                                                         16 M cells  0.339 ms   4.3 x the cast   0.39 x the gather
 *   a stream of 350-byte documents, one id_str each        1 M cells  0.053 ms   1.6 x the cast   0.21 x the gather
 *                                                          4 M cells  0.170 ms   3.9 x the cast   0.24 x the gather
 * A million cells is launch-bound for all three calls; beyond that the call costs about four times the cast of the same row -- the
 * cast moves 18 bytes per cell, this call touches a line of the string buffer per cell on top -- and less than half of what gathering
 * the characters alone costs, before any copy to the host and any loop there.  At a million cells, strings that lie a document apart (363 bytes in the
 * string buffer) cost 1.26 times what strings 23 bytes apart cost: every cell is a line of its own there. */
enum { SJGPU_GETS_INT64 = 1, SJGPU_GETS_UINT64 = 2, SJGPU_GETS_DOUBLE = 3,   /* get_*_in_string */
       SJGPU_GETS_OR_NUMBER = 0x10 };                                         /* flag, or-ed into a getter byte */

int sjgpu_cast_string_cells_device(sjgpu_ctx *ctx, const void *string_buf_dev, uint64_t string_bytes,
                                   const void *value_dev, const void *tag_dev, uint32_t n, uint32_t K,
                                   const uint8_t *getters /* K bytes, HOST */,
                                   void *value_out_dev /* K * n u64 */, void *code_out_dev /* K * n bytes */,
                                   void *valid_out_dev /* K * ceil(n / 64) u64 */, void *counts_out_dev /* K * 8 u32 */,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif
