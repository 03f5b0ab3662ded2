/* include/sjgpu_dict.h -- C-ABI of libsjgpu.so, dictionaries over device cells: a row of string cells as int32 codes plus a small dictionary in order of first
 * occurrence (pandas' factorize, Arrow's dictionary_encode), and the census of a value row per code -- what a loader needs for a categorical column and for
 * learning the keys of a set of records and the kinds of values under each key.
 * An extension of include/sjgpu_fields.h and the headers below it (the cell encoding, the string buffer and the census are declared there, in
 * include/sjgpu_cast.h and in include/sjgpu_query.h); a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_DICT_H
#define SJGPU_DICT_H

#include "sjgpu_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef SJGPU_E_INTERNAL
#define SJGPU_E_INTERNAL (-7) /* a bounded loop of the library ran out where its invariant says it cannot: a bug of the library, never the caller's data */
#endif

/* ---- batched `std::unordered_map<std::string_view, ...> m; for (cell) m[get_string(cell)]...` (k_dict_insert, k_dict_heads, k_dict_codes, k_dict_fill) -----
 * The input is ONE row of n cells in the encoding of sjgpu_at_pointers_device: any row of a query call, the key row of
 * sjgpu_object_fields_from_cells_device, a flattened column of the paths calls, or the dictionary row of this call.  No tape and no document table is read.
 *
 * Which cells count.  A cell is a STRING when its tag is '"' and offset + length <= string_bytes (value = (length << 32) | offset: the rule of
 * sjgpu_gather_strings_device).  Every other cell is NULL: every other tag, every code 17 / 19 / 20 / 22, any other byte, and a string cell that points
 * outside string_buf_dev[0 .. string_bytes).
 * Equality.  Two strings are equal when they have the same length and the same bytes in string_buf_dev -- std::string_view == on what get_string() returns,
 * the UNESCAPED bytes: the JSON strings "\u0041" and "A" are one string.  A NUL is a byte like any other: "a\u0000b", "a" and "a\u0000" are three strings.  "" is a string and
 * gets an entry.  Nothing is case-folded or normalised.
 * Outputs.
 *   codes_dev[i]        int32: the index of cell i's string in the dictionary, -1 for a null
 *   the dictionary is in order of FIRST OCCURRENCE: entry j belongs to the j-th distinct string met when the row is read from cell 0 upwards, and
 *   dict_first_dev[j]   u32, the row of that first occurrence (ascending in j)
 *   dict_value_dev[j]   u64, that cell's word, unchanged
 *   dict_tag_dev[j]     '"'
 *   dict_count_dev[j]   u32, the number of cells with code j (their sum is the number of string cells)
 * The result is a pure function of the inputs: which lane met a string first on the device shows nowhere.
 * Composition: dict_value_dev / dict_tag_dev[0 .. *distinct_out) is a row of string cells, a valid input of sjgpu_gather_strings_device (the dictionary as
 * offsets + characters) and of this call (which gives the codes 0 .. *distinct_out - 1 back).  codes_dev is the codes_dev of sjgpu_cell_kinds_by_code_device.
 * Every code and every slot in [0, *distinct_out) of the four arrays is written; nothing is written outside them.  The tag rows begin at any byte.  No output
 * may overlap an input or another output.
 * Capacity, limits, refusals (those of the ragged calls).  dict_cap too small: SJGPU_E_OVERFLOW, *distinct_out says what is needed, codes_dev is complete
 * (codes do not depend on the capacity) and nothing is written to the four dictionary arrays: dict_cap == 0 with null arrays is how to ask.
 * n == 0: 0 with *distinct_out = 0 and nothing written.  n above 2^30: SJGPU_E_BADARG (the table's slots are u32).
 * SJGPU_E_BADARG, before anything is read or enqueued: ctx, string_buf_dev or distinct_out null; with n > 0 value_row_dev, tag_row_dev or codes_dev null; with
 * dict_cap > 0 one of the four dictionary arrays null; value_row_dev or dict_value_dev not 8-byte aligned; codes_dev, dict_first_dev or dict_count_dev not
 * 4-byte aligned; string_bytes beyond 32 bits.
 * Returns 0 or a negative SJGPU_E_*.  SJGPU_E_INTERNAL: a probe found no slot in a table that is at most half full -- cannot happen, and is reported instead
 * of looped on.  Waits for the stream: the total is read back, and the outputs are complete on return.
 *
 * How.  An open-addressed table of S = the smallest power of two >= 2 n u32 slots in the context's workspace, each 0xFFFFFFFF (empty) or a row.  A lane hashes
 * its string to 64 bits, the length mixed in, and probes linearly: an empty slot is claimed with a compare-and-swap of the lane's row; an occupied slot is
 * compared with the lane's string (the cell word, then the length, then the bytes) and is the string's slot when equal.  No lane waits for another: the probe is
 * bounded by S steps.  Its first two steps are the wave's: the lanes that read "empty" at one slot elect one of them for the compare-and-swap and share its outcome,
 * so that a column of one value does not queue one atomic per cell on one word.  Once every lane of a wave has its slot, the lanes that share one elect the lowest (rows are consecutive: it holds the smallest row),
 * which does ONE atomicAdd of the group's size beside the slot and, unless the row it saw there is already no larger, ONE atomicMin of its row into it -- a column
 * of one distinct value costs one or two atomics per wave, not two per cell.  The slot ends holding the smallest row of its group; row r is a head when table[slot_of[r]] == r; an exclusive scan of the head flags is
 * the dictionary index; heads write their entry and every row writes codes[r] = rank[table[slot_of[r]]].
 * Three memsets (8 S + 8 bytes) and seven launches at the most (insert, heads, the scan's one to three, codes, fill); one read-back of 8 bytes.
 * Workspace: 8 S + 8 n bytes and the scan's block sums, 24 to 40 bytes per cell.
 * Cost, not hidden: one lane per cell.  A lane reads its own string once to hash it and once more per occupied slot it compares with, 8 bytes at a time; a
 * string of a megabyte is ONE lane's work, and so is comparing two strings that differ in their last byte.  A row of distinct strings is bound by scattered
 * probes into a table of 8 n bytes; a row of few distinct strings by reading the row and the atomics of one leader per wave and distinct string in it. */
int sjgpu_dictionary_encode_device(sjgpu_ctx *ctx, const void *string_buf_dev, uint64_t string_bytes, const void *value_row_dev, const void *tag_row_dev, uint32_t n,
                                   void *codes_dev /* n int32 */, void *dict_value_dev /* dict_cap u64 */, void *dict_tag_dev /* dict_cap bytes */,
                                   void *dict_first_dev /* dict_cap u32 */, void *dict_count_dev /* dict_cap u32 */, uint64_t dict_cap, void *stream,
                                   uint64_t *distinct_out);

/* ---- the census of a value row per code (k_cell_kinds_by_code_lds, k_cell_kinds_by_code_global) ---------------------------------------------------------------
 * Cell i of value_dev / tag_dev -- the value row that lies beside a key row -- is counted in row codes_dev[i] of kinds_dev: kinds_dev[g * 16 ..] are the sixteen
 * counters of sjgpu_cell_kinds_device (include/sjgpu_cast.h) over the cells whose code is g; the classification is that call's, not restated here.
 * A code outside 0 .. groups - 1, the -1 of a null included, is counted in nobody's row.  Every counter is written: the call memsets them.
 * groups == 0: 0, nothing written.  n == 0: 0 with the groups rows zeroed.
 * SJGPU_E_BADARG, decided before anything is enqueued (the census's rules): ctx null; value_dev not 8-byte, codes_dev or kinds_dev not 4-byte aligned; groups * 16
 * beyond 32 bits; with groups > 0 a null kinds_dev; with groups * n > 0 any other null pointer.
 * Only enqueues on `stream`: a memset and one launch, no read-back, no block of the context, no wait for its previous query.
 * Cost, not hidden: up to 512 groups (32 KiB) a workgroup keeps its histogram in LDS -- one LDS atomic per cell, two for a negative l -- and adds its non-zero
 * counters to kinds_dev with one atomic each, at most 1 024 workgroups; the lanes of a wave that count the same kind under the same code queue on one LDS word.
 * Above 512 groups every counted cell is one global atomic (two for a negative l) on kinds_dev. */
int sjgpu_cell_kinds_by_code_device(sjgpu_ctx *ctx, const void *codes_dev /* n int32 */, const void *value_dev, const void *tag_dev, uint32_t n, uint32_t groups,
                                    void *kinds_dev /* groups * 16 u32 */, void *stream);

#ifdef __cplusplus
}
#endif
#endif
