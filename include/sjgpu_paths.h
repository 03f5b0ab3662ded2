/* include/sjgpu_paths.h -- C-ABI of libsjgpu.so, JSONPath with wildcards over device tapes: K paths resolved against the root of every
 * document of a tape stream, one RAGGED column out (a variable number of matches per cell, CSR style).
 * An extension of include/sjgpu_query.h (the cell encoding and the tapes, string records and document table it reads are declared there
 * and in include/sjgpu_stream.h); a header of its own so that programs built against the other headers are not rebuilt for it. */
#ifndef SJGPU_PATHS_H
#define SJGPU_PATHS_H

#include "sjgpu_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched dom::element::at_path_with_wildcard over resident tapes (k_at_paths in sjgpu_query.hip) ---------------------------
 * Cell (path k, document d) is what dom::parser::parse(bytes of document d).at_path_with_wildcard(path k) gives in the reference
 * (include/simdjson/dom/element-inl.h:448-459, object-inl.h:155-244, array-inl.h:129-214, jsonpathutil.h:58-161): an error code, or
 * the list of the elements matched, depth first and in document order.  The reference parses the path while it recurses; what is
 * left of the path at recursion depth i depends on the path alone, so the path is compiled once per call into one LEVEL per depth
 * (simdjson_amd/csrc/sj_path_program.h).  With r the string left, `$` an optional first byte:
 *   r is empty, or continues with neither `.` nor `[`                       INVALID_JSON_POINTER 22
 *   r holds no `*`                  at_pointer of r converted to a pointer (`.k` and `[k]` become `/k`; an unclosed `[` is 22): one
 *                                   match, or the pointer's code with the lazy rules of sjgpu_at_pointers_device
 *   r is exactly `[*]` or `.*`      every child value matches: an array's elements, an object's values
 *   r begins `[*]` or `.*`          every child value goes on with the rest of r
 *   r begins `.key`, `['key']` or `["key"]`   at_pointer("/" + key), the key's bytes raw: a `~` is read by the pointer's rules, a `/`
 *                                   makes two tokens, an array reads the key as an index.  An error means no match; the element
 *                                   found goes on with the rest of r
 *   anything else while a `*` lies ahead (`[0]`, an unterminated `['k`, `..`)           22
 * A scalar that reaches any depth contributes nothing and is no error: a scalar ROOT gives status 0 and no match for every path, the
 * empty one included.  A code is the cell's status only at depth 0 (17, 19, 20 or 22 on a container root); at any deeper level it is
 * swallowed and that branch contributes nothing.  So `$.a[0].c[*]` matches nothing (`[0]` in front of a `*` is 22, below the
 * root), and `$.a[*]['b']` matches nothing either (`['b']` behind the last `*` is converted to the pointer `/'b'`).
 *
 * paths: K byte strings back to back in HOST memory, path_lens[k] their lengths.  Limits: K <= 64, a path <= 1024 bytes, at most 32
 * levels, at most 32 pointer tokens over all levels of a path, at most 8 wildcards.
 * tape_dev / string_buf_dev / docs_dev: as for sjgpu_at_pointers_device (docs + 1 table entries).
 * Cell c = k * docs + d.
 *   offsets_dev[0 .. K * docs]  u32, the exclusive sum of the cells' match counts: cell c owns value_dev / tag_dev[offsets[c] ..
 *                               offsets[c + 1]), and offsets_dev[K * docs] == *matches_out
 *   status_dev[c]               0, 17, 19, 20 or 22; a cell with a status other than 0 has no matches
 *   value_dev[i], tag_dev[i]    match i in the cell encoding of sjgpu_at_pointers_device (tag_dev: the tape tag of the element; value_dev:
 *                               the number, 1 / 0, a string's (length << 32) | offset, a container's sub-tape bounds -- offsets and
 *                               indices absolute in string_buf_dev / tape_dev)
 * value_dev and tag_dev are ONE flattened pair of rows: a valid input of sjgpu_gather_strings_device with docs = *matches_out, whose
 * offsets then give one string slice per match.
 * match_cap (the matches value_dev and tag_dev have room for) too small: SJGPU_E_OVERFLOW, *matches_out says what is needed,
 * offsets_dev and status_dev are complete and nothing is written to value_dev or tag_dev.  A total beyond 32 bits: CAPACITY (1) -- the total out-parameter holds
 * the 64-bit total, status and counts are complete, offsets_dev is written but meaningless (its 32-bit words wrapped) and nothing is written to the data arrays.
 * K == 0 or docs == 0: 0 with offsets_dev[0] = 0.  Nothing is written outside offsets_dev[0 .. K * docs], status_dev[0 .. K * docs),
 * value_dev / tag_dev[0 .. *matches_out): the fill never writes at or beyond offsets[c + 1], whatever the tape says.  Nothing is read
 * outside the arrays and the table: a tape word that points elsewhere ends its level instead of being followed.
 * SJGPU_E_BADARG: a null pointer (value_dev and tag_dev may be null when match_cap is 0), tape_dev or value_dev not 8-byte, docs_dev
 * not 16-byte, offsets_dev not 4-byte aligned (status_dev and tag_dev begin at any byte), K or a path beyond the limits, K * docs + 1
 * beyond 0xFFFFFFF0 (the scan over the counts indexes its entries with 32-bit words), or a table whose tape_begin / string_begin
 * run backwards or end beyond tape_words / string_bytes.  Returns 0, CAPACITY or a negative SJGPU_E_*; what a cell meets is in its
 * status, never in the return value.
 * Three launches: count (the walk, counting), an exclusive scan in place over the K * docs + 1 counts with a 64-bit total beside it,
 * fill (the same walk, writing).  Waits for the stream: the total is read back, and the columns are complete on return.
 * Cost, not hidden: one lane walks one cell, consecutive lanes consecutive documents of one path.  A cell costs time linear in the
 * siblings it passes and in the elements it visits under its wildcards, twice, and all of it is ONE lane's work: `$.statuses[*].user.id`
 * over one large document runs on one lane.  The fill's stores are one run per lane, not coalesced across lanes.  The
 * frontier-per-level (breadth-first) expansion that shares one document among lanes is sjgpu_at_paths_wide_device below. */
int sjgpu_at_paths_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes,
                          const void *docs_dev, uint32_t docs, const uint8_t *paths, const uint32_t *path_lens, uint32_t K,
                          void *offsets_dev /* K * docs + 1 u32 */, void *status_dev /* K * docs bytes */,
                          void *value_dev, void *tag_dev, uint64_t match_cap, void *stream, uint64_t *matches_out);

/* ---- the same column, breadth first (the k_wide_* kernels in sjgpu_query.hip) ------------------------------------------------------
 * The contract of sjgpu_at_paths_device, word for word: the cells, the level program and its limits, the alignments and refusals, K == 0 /
 * docs == 0, CAPACITY for a total beyond 32 bits and what it leaves behind, SJGPU_E_OVERFLOW with offsets_dev and status_dev complete, *matches_out set and nothing
 * written to value_dev / tag_dev, nothing written outside the contracted ranges, nothing read outside the three arrays, and the call
 * waits for the stream.  Over tapes that sjgpu_stage2_device / sjgpu_stage2_many_device delivered all four outputs are bit for bit those
 * of sjgpu_at_paths_device.  Over words that are no tape the results are unspecified; the call still ends, stays inside its arrays and
 * never writes at or beyond match_cap.
 * How: the elements of ALL documents that wait for a level of a path are one ascending list of tape indices, and a level turns that
 * list into the next.  `.key` levels and the pointer behind the last `*` take one lane per element of the list.  A wildcard level lays
 * the words of the list's containers end to end and takes one lane per WORD: a word is a child when it begins an element one nesting
 * level below its container, which an annotation of the tape (a bit and a depth per word, made once per call for all K paths) answers
 * without a walk.  The match list of a path is ascending, so the cells of its documents are slices of it found by a search.
 * Capacity: the levels run twice -- once for statuses, offsets and the total, once more to write when the total fits -- except for the
 * last path, whose matches are still in the workspace; with K == 1 they run once.
 * Workspace (the context's, grown on demand; its failure is SJGPU_E_NOMEM): 25 bytes per tape word -- annotation 5, two
 * lists 8, the wildcard level's extents, child ranks and counts 12 -- plus 4 per document and the scans' block sums, whatever K is:
 * the tapes of a 256 MiB document of 40 M words ask for 1 GB.
 * Costs, not hidden:
 *   the annotation is linear in tape_words, once per call, whatever the paths touch;
 *   a wildcard level is linear in the summed extents (closing word - opening word - 1) of the list's containers, spread over lanes:
 *   `$.statuses[*].user.id` looks at every word of the document once per run, with as many lanes as there are words;
 *   a `.key` / pointer level is still ONE lane per element, linear in the siblings it passes: a key searched in one object of a million
 *   fields stays one lane's work;
 *   every path costs a handful of launches per level and one 4-byte read-back the host waits for per `.key` level, two per wildcard
 *   level.  For streams of small records sjgpu_at_paths_device is therefore expected to stay the faster call; that is not measured.
 * Which of the two calls to take is the caller's decision: choosing automatically needs the measured crossover, and is not built. */
int sjgpu_at_paths_wide_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes,
                               const void *docs_dev, uint32_t docs, const uint8_t *paths, const uint32_t *path_lens, uint32_t K,
                               void *offsets_dev /* K * docs + 1 u32 */, void *status_dev /* K * docs bytes */,
                               void *value_dev, void *tag_dev, uint64_t match_cap, void *stream, uint64_t *matches_out);

#ifdef __cplusplus
}
#endif
#endif
