// simdjson_amd/csrc/sjgpu_internal.h -- launch interface between the C-ABI (sjgpu_capi*.hip, sjgpu_ctx.h) and the
// gfx950 kernels (sjgpu_kernels.hip).  Geometry:
//
//   block   = 64 input bytes                = one lane
//   chunk   = 64 blocks = 4 KiB             = one wave64 pass
//   segment = SEG_CHUNKS chunks = 16 KiB    = one wave's (= one workgroup's) contiguous share
//
// Device workspace per context (all sized from `capacity`, resident in HBM between calls):
//   masks  2 planes x [ceil(cap/64)] x u64  per block: plane 0 = final structural mask (resolved segments) or
//                                  candidates; plane 1 = string_tail (unresolved segments only)
//   summ   [nseg + ngroups] x seg_summary  per-segment carry summary (quote parity, counts for both
//                                  in-string hypotheses, error bits), then the same per group of 64 segments
//   pref   [ngroups] x seg_prefix  per-group resolved carry-in (in-string bit, output base)
//   result                          one scan_result, mirrored to pinned host memory
#ifndef SJGPU_INTERNAL_H
#define SJGPU_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sjgpu {

constexpr uint32_t BLOCK_BYTES = 64;
constexpr uint32_t CHUNK_BYTES = 4096;
constexpr uint32_t SEG_CHUNKS = 4;
constexpr uint32_t SEG_BYTES = CHUNK_BYTES * SEG_CHUNKS;

// summary flags
constexpr uint32_t SF_PARITY = 1u;     // odd number of unescaped quotes in the segment
constexpr uint32_t SF_CTRL_IF_OUT = 2u; // control char inside a string if the segment starts OUTSIDE a string
constexpr uint32_t SF_CTRL_IF_IN = 4u;  // ... if it starts INSIDE a string
constexpr uint32_t SF_UTF8 = 8u;        // UTF-8 error in the segment
constexpr uint32_t SF_RESOLVED = 16u;   // the segment fixed its own in-string carry-in (first control character): its
                                        // mask plane 0 is final and both counts are equal
constexpr uint32_t SF_TOKENS = 32u;     // launch_stage1 with a token stream: the segment's structural bytes lie in its staging area
constexpr uint32_t SF_SPARSE = 64u;     // round 6: at most SPARSE_MAX candidates in the segment: the start of its plane-0 area holds them as a LIST of words
                                        // (bits 0-13 the candidate's byte offset inside the segment, bit 31 its string_tail bit) instead of 2 x 2 KiB of planes
constexpr uint32_t SPARSE_MAX = 32u;    // one 128-byte line of list words per sparse segment

struct seg_summary {
  uint32_t count_if_out; // structurals (stage1) / kept bytes (minify) if the segment starts outside a string
  uint32_t count_if_in;  // ... inside a string
  uint32_t flags;
  uint32_t xw;           // the x word of the summary (sj_xcarry.h): what a wrong look-back assumption changes, and what the successor's x is
};
struct seg_prefix {
  uint32_t base; // exclusive prefix of counts = first output slot of the segment
  uint32_t in_string; // bit 0: inside a string; bit 1: x, "the look-back assumption of this segment / group is wrong"
};
struct scan_result_dev {
  uint32_t n;
  uint32_t flags;
  uint64_t out_len;
};

inline uint32_t num_segments(uint64_t len) { return uint32_t((len + SEG_BYTES - 1) / SEG_BYTES); }
// split pipeline's resolve is two-level: 64 segments (1 MiB of input) form a group
constexpr uint32_t RESOLVE_GROUP = 64;
inline uint32_t num_groups(uint64_t len) { return (num_segments(len) + RESOLVE_GROUP - 1) / RESOLVE_GROUP; }

// single-pass pipeline (sjgpu_fused.hip): tile = one 256-thread workgroup = 4 waves x 4 chunks = 64 KiB;
// workspace = one 8-byte descriptor per tile + the ticket word behind them.
constexpr uint32_t FUSED_WAVE_CHUNKS = 4;
constexpr uint32_t FUSED_TILE_BYTES = 4 * FUSED_WAVE_CHUNKS * CHUNK_BYTES;
// k_minify_onchip (bytes of the pending tile wait in LDS): two chunks per wave, 4 or 8 waves per workgroup
constexpr uint32_t ONCHIP_WAVE_CHUNKS = 2;
constexpr uint32_t ONCHIP_TILE_BYTES = 4 * ONCHIP_WAVE_CHUNKS * CHUNK_BYTES;
// inputs up to FUSED_SMALL_BELOW use 16 KiB tiles (one chunk per wave): 4x the parallelism, 1/4 of the per-tile latency
constexpr uint64_t FUSED_SMALL_BELOW = uint64_t(8) << 20;
inline uint32_t num_fused_tiles(uint64_t len) { // descriptor words a context needs for documents up to len
  const uint64_t big = (len + ONCHIP_TILE_BYTES - 1) / ONCHIP_TILE_BYTES; // the smallest tile any large-input kernel uses
  const uint64_t small_len = len < FUSED_SMALL_BELOW ? len : FUSED_SMALL_BELOW;
  const uint64_t small = (small_len + FUSED_TILE_BYTES / FUSED_WAVE_CHUNKS - 1) / (FUSED_TILE_BYTES / FUSED_WAVE_CHUNKS);
  return uint32_t(big > small ? big : small);
}

// ---- launchers (sjgpu_kernels.hip); every one only enqueues on `stream` ---------------------------------
// ev: nullptr, or PROFILE_EVENTS events recorded around the kernels: ev[k], ev[k+1] bracket slot k (slot 0 includes the
// escape-table launch and the workspace clears in front of the first scan kernel; unused slots measure zero).
constexpr int PROFILE_SLOTS = 3;
constexpr int PROFILE_EVENTS = PROFILE_SLOTS + 1;
// carry: state in front of byte 0 when the buffer is a shard of a larger document; 0 for a whole document.
// Shards are cut by sjgpu_clean_cut, so the in-string bit is the ONLY state that crosses a cut.
constexpr uint32_t CARRY_IN_STRING = 1u; // the first byte scanned is inside a string
constexpr uint32_t CARRY_SHARD = 2u;     // minify: report out_len even if the scan ends inside a string
constexpr uint32_t CARRY_MORE = 4u;      // the scan does not end at the end of the input: no "sequence open at EOF" check
constexpr uint32_t CARRY_X = 8u;         // x in front of the first span (sj_xcarry.h): SJGPU_F_RANGE_CARRY of the range in front
constexpr uint32_t CARRY_DEBUG_LATE_TICKET = 0x100u; // A/B switch of the pipelined kernel (env SJGPU_LATE_TICKET)
constexpr uint32_t CARRY_DEBUG_NO_SPAN_HINT = 0x200u; // A/B switch: emission counts the span itself (env SJGPU_NO_SPAN_HINT)
constexpr uint32_t CARRY_DEBUG_LATE_LOOKBACK = 0x800u; // A/B switch of the pipelined kernels: the pending tile's look-back BEHIND the scan's barrier, as in rounds 1-5 (env SJGPU_LATE_LOOKBACK)
constexpr uint32_t CARRY_DEBUG_TOP_BARRIER = 0x1000u;  // A/B switch of the pipelined kernels: the third barrier, at the loop top, as in rounds 1-5 (env SJGPU_TOP_BARRIER)
constexpr uint32_t CARRY_DEBUG_TWO_TICKETS = 0x2000u;  // A/B switch of the pipelined kernels: tickets from two counters, even / odd tiles by the workgroup's parity (env SJGPU_TWO_TICKETS)
constexpr uint32_t CARRY_DEBUG_QUEUE_UTF8 = 0x400u;   // A/B switch: dense non-ASCII chunks are queued like sparse ones (env SJGPU_UTF8_QUEUE_ONLY)
// A scan covers bytes [begin, len) of a buffer whose bytes [0, begin) are resident too (the look-back of escapes,
// previous scalar and UTF-8 state reads them); begin is a multiple of RANGE_ALIGN.  Offsets stay relative to byte 0
// and are appended at output slot base0.  A whole document is {0, 0, 0}.
struct scan_origin {
  uint64_t begin;
  uint32_t base0;
  uint32_t carry;
};
constexpr uint64_t RANGE_ALIGN = uint64_t(1) << 20; // one resolve group = 16 large tiles = 64 small tiles
// tokstage / tok (both or neither): the token-byte stream beside the offsets -- tok[i] = buf[idx[i]] for i < n.  tokstage: scratch of num_segments(len -
// org.begin) * SEG_BYTES bytes, 16-byte aligned (the segments' structural bytes wait there between the two kernels); tok: room for n bytes
void launch_stage1(const uint8_t *buf, uint64_t len, uint4 *masks, seg_summary *summ, seg_prefix *pref, uint32_t *idx,
                   uint64_t idx_words, scan_result_dev *result, scan_origin org, hipStream_t stream, hipEvent_t *ev, uint8_t *tokstage = nullptr,
                   uint8_t *tok = nullptr);
void launch_minify(const uint8_t *buf, uint64_t len, seg_summary *summ, seg_prefix *pref, uint8_t *dst,
                   scan_result_dev *result, scan_origin org, hipStream_t stream, hipEvent_t *ev);
// result->n = parity; workspace: one byte per 16 KiB segment of the buffer (the per-segment parities and x words, folded by a second launch)
void launch_string_parity(const uint8_t *buf, uint64_t len, scan_result_dev *result, uint8_t *workspace, hipStream_t stream);
// (rounds 1-3 built an escape table in front of every large scan -- one byte per 16 KiB boundary: is the byte behind it escaped? -- by walking
// back over the backslash run in front; round 4 carries that bit through the summaries instead, sj_xcarry.h, and the table is gone.)
// one byte per 16 KiB segment of a 4 GiB buffer: the per-segment scratch of launch_string_parity
constexpr size_t SEGMENT_BYTES_TABLE = ((uint64_t(1) << 32) / SEG_BYTES + 1024) & ~size_t(1023);
// bytes [begin, len) of buf; begin > 0 (a multiple of 4 KiB): a later range of a resident buffer, the flags add up in *result;
// more: the input continues behind len
void launch_validate_utf8(const uint8_t *buf, uint64_t len, scan_result_dev *result, hipStream_t stream, hipEvent_t *ev,
                          uint64_t begin = 0, bool more = false);
// single-pass variants: desc holds num_fused_tiles(capacity) + FUSED_WORKSPACE_EXTRA_WORDS words; only profile slot 0 is used.
// clean: *result, the descriptors and the control words behind them are all zero on the device.  Every (un-traced) single-pass kernel leaves them
// that way when it ends -- its last workgroup to leave clears what the call used (sjgpu_fused.hip: leave_and_clean) -- so a caller that cleared the
// whole workspace once, when it allocated it, passes true from then on and a call is ONE dispatch; with false the launcher clears in front of the kernel.
constexpr uint32_t FUSED_WORKSPACE_EXTRA_WORDS = 18; // control words: [ticket, workgroups gone][flags, -], fourteen words of distance, [second ticket counter] (its own 128-byte line)
const char *launch_stage1_fused(const uint8_t *buf, uint64_t len, uint64_t *desc, uint32_t *idx, uint64_t idx_words,
                                scan_result_dev *result, scan_origin org, uint32_t max_workgroups, hipStream_t stream,
                                hipEvent_t *ev, bool clean = false, uint8_t *tok = nullptr); // tok: the token-byte stream beside the offsets (round 6: gathered at emission) // -> name of the scan kernel launched
// round 6: the one-pass kernel for PLAIN input (every 16 KiB segment pins its own string state at a control character of its first chunk, no span assumed its
// escape carry): additive prefixes, emission deferred by one tile (sjgpu_fused.hip: k_stage1_direct).  Input that is not plain: SJGPU_F_INTERNAL in the result.
// Needs num_direct_words(len) + FUSED_WORKSPACE_EXTRA_WORDS descriptor words (never more than num_fused_tiles(len) from 8 MiB on).
const char *launch_stage1_direct(const uint8_t *buf, uint64_t len, uint64_t *desc, uint32_t *idx, uint64_t idx_words, scan_result_dev *result, scan_origin org,
                                 uint32_t max_workgroups, hipStream_t stream, hipEvent_t *ev, bool clean = false);
void launch_stage1_fused_traced(const uint8_t *buf, uint64_t len, uint64_t *desc, uint32_t *idx, uint64_t idx_words,
                                scan_result_dev *result, uint32_t max_workgroups, hipStream_t stream, uint64_t *trace,
                                uint32_t trace_tiles); // 8 wall_clock64 stamps (100 MHz) per tile
// ---- the structural list after the scan (sjgpu_finish.hip) ----------------------------------------------------------------
enum : uint32_t { FIN_SEARCH = 0, FIN_KEEP_GIVEN = 1, FIN_TOO_LARGE = 2, FIN_COUNT_BELOW = 3 };
struct finish_state {            // device-resident, zero-initialised; read back by the host once the kernels are done
  uint32_t n_in, n_cur, n_report; // structurals handed in / the boundary search runs on / the reference's `n` after the filter
  uint32_t next_start;            // where the next batch begins (len unless a separator says otherwise)
  uint32_t kept, keep, verdict;   // compacted length; structurals of complete documents; FIN_*
  uint32_t separators, last_sep_index_plus1, last_sep_pos_plus1; // root commas / record separators seen
  uint32_t boundary_plus1;        // list index + 1 of the last value that directly follows a value
  int32_t obj_balance, arr_balance;
  uint32_t arrivals;              // workgroups of k_tail_balance that have added their part (the last one resolves)
  uint32_t pad[2];
};
size_t finish_workspace_bytes(uint32_t n);
// modes 1..6 of sjgpu_stage1_mode on the n raw structurals idx[0..n) (n > 0) of buf[0..len): filters the list in place
// (json_sequence / comma_delimited) and leaves the decision in the finish_state at the start of `workspace`
void launch_finish(int mode, const uint8_t *buf, uint64_t len, uint32_t *idx, uint32_t n, void *workspace, hipStream_t stream);
// depth[i] = nesting depth in front of structural i for i in [0, n], depth[n] = behind the last; scratch: depth_scan_scratch_bytes(n)
size_t depth_scan_scratch_bytes(uint32_t n);
// tok (optional): the token stream of the list (tok[i] = buf[idx[i]]); with it neither buf nor idx is read
void launch_depth_scan(const uint8_t *buf, const uint32_t *idx, uint32_t n, int32_t *depth, void *scratch, hipStream_t stream, const uint8_t *tok = nullptr);

// ---- one workgroup per document (sjgpu_small.hip) ---------------------------------------------------------------------
// in_off: byte offset of the document in the input block (a multiple of 64); out_off: first output unit of the document in
// the output block (stage 1: words, a multiple of 4, room for len + 3; minify: bytes, a multiple of 16, room for len)
struct doc_desc {
  uint64_t in_off;
  uint64_t out_off;
  uint32_t len;
  uint32_t flags;
};
constexpr uint32_t DOC_KEEP_UNCLOSED = 1u; // minify: report out_len even if the document ends inside a string
// documents up to this size take the one-workgroup kernel when they come one by one (sjgpu_stage1 & co.)
constexpr size_t DOCS_SINGLE_MAX = size_t(64) << 10;
// op 0 stage 1, 1 minify, 2 validate_utf8; docs == nullptr: one document, described by `single`.  in_base / out_base /
// results may be device memory or page-locked host memory (the kernel then moves the bytes across PCIe itself).
void launch_docs(int op, const uint8_t *in_base, const doc_desc *docs, doc_desc single, uint32_t count, void *out_base,
                 scan_result_dev *results, hipStream_t stream);

uint32_t launch_stage1_pipelined_traced(const uint8_t *buf, uint64_t len, uint64_t *desc, uint32_t *idx, uint64_t idx_words,
                                        scan_result_dev *result, uint32_t max_workgroups, hipStream_t stream,
                                        uint64_t *trace, uint32_t max_records); // -> workgroups launched (32 records of 8 stamps each)
const char *launch_minify_fused(const uint8_t *buf, uint64_t len, uint64_t *desc, uint8_t *dst, scan_result_dev *result,
                                scan_origin org, uint32_t max_workgroups, hipStream_t stream, hipEvent_t *ev, bool clean = false);

// ---- strings (sjgpu_strings.hip) -------------------------------------------------------------------------------
struct strings_result_dev {
  uint64_t bytes;     // string buffer bytes used
  uint32_t strings;   // records written
  uint32_t first_bad; // index of the first structural whose string the reference rejects, 0xFFFFFFFF = none
  uint32_t overflow;  // a record did not fit into the caller's buffer
  uint32_t path;      // which kernels wrote the buffer: 1 = the stream compaction (sjgpu_string_stream.hip), 2 = the per-string walk
};
// scratch of one string pass, carved from one allocation of strings_scratch_bytes(n, len) bytes (256-byte aligned pieces)
constexpr size_t STRS_SUMMARY_BYTES = 32, STRS_BASE_BYTES = 16;
struct strings_scratch {
  void *ctrl;        // 64 bytes: scan lengths, which path writes the buffer, totals (sjgpu_string_stream.hip: strs_ctrl)
  int *partial;      // block sums of the scans
  int *kord;         // n + 2 ints of room: string tokens per tile of 4096 structurals (then their prefixes) and one bit per structural (sjgpu_string_stream.hip)
  uint32_t *outq;    // n + 2: where the k-th string's record begins
  void *seg_summary; // per 16 KiB segment of the document
  void *seg_base;
  size_t bytes;
};
strings_scratch carve_strings_scratch(void *base, uint32_t n, uint64_t len);
size_t strings_scratch_bytes(uint32_t n, uint64_t len);
// the buffer as a stream compaction of the document (sjgpu_string_stream.hip); leaves in the control block whether the
// per-string kernels have to run instead
void enqueue_string_stream(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint32_t n, bool allow_replacement, uint8_t *out, uint64_t out_cap,
                           uint32_t *offsets, strings_result_dev *res, const strings_scratch &w, hipStream_t s, const int *listed);
// What the string pass hands to a caller that finishes the records itself (the tape): where the k-th string's record begins, and the device
// flag that says whether the stream compaction wrote the buffer (then the length words are still missing) or the per-string kernels did.
struct strings_handoff {
  const uint32_t *outq;
  const uint32_t *go_stream;
};
// listed (optional): device pointer to the number of string tokens of the list, counted by the caller (launch_tape_front) -- the pass then
// neither counts them itself nor writes offsets / length words for the stream's records (the caller does, from the handoff: the k-th string
// token's record begins at outq[k])
// roads: which of the two roads to the buffer are enqueued.  STRINGS_BOTH: the stream compaction and, behind it, the per-string kernels, which return at once
// when the stream took the document (the decision is taken on the device: stand-alone sjgpu_parse_strings_device).  STRINGS_STREAM_ONLY: the stream alone --
// a document it declines comes back with res->path == 2 and NOTHING written, and the caller enqueues the pass again with STRINGS_WALK_ONLY (the verdict
// overridden: the per-string kernels write).  sjgpu_stage2_device takes that optimistic route: five launches that nearly always do nothing are not enqueued.
enum : int { STRINGS_BOTH = 0, STRINGS_STREAM_ONLY = 1, STRINGS_WALK_ONLY = 2 };
strings_handoff launch_parse_strings(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint32_t n, bool allow_replacement, uint8_t *out, uint64_t out_cap,
                                     uint32_t *offsets, strings_result_dev *res, void *scratch, hipStream_t s, const int *listed = nullptr, int roads = STRINGS_BOTH);
// ---- the tape (sjgpu_tape.hip) ----------------------------------------------------------------------------------
struct tape_result_dev {
  uint64_t error_key;   // smallest (list index << 8 | rank << 4 | error_code) over all offending tokens, ~0 = none (sj_tape_rules.h)
  uint64_t tape_words;  // words of the finished tape (both root words included)
  uint32_t slow_numbers; // number tokens that took the big-integer decision
  uint32_t overflow;    // the caller's tape was too small
  uint32_t max_level;   // the highest nesting level among the brackets and commas: 64 and more needs the sort's second pass (launch_tape's `deep`)
  uint32_t pad;
};
constexpr uint32_t TAPE_ONE_PASS_LEVELS = 64; // levels one pass of the sort tells apart
size_t tape_workspace_bytes(uint32_t n, uint64_t len);
// stage 2 of buf[0..len) from its structural list idx[0..n] (idx[n] = len), in two halves around the string pass: launch_tape_front leaves
// the token bytes and the block totals of the per-token counters in the workspace and returns the number of string tokens (device);
// launch_tape writes the reference's tape (and the length words of the string records when the stream compaction wrote them).
// workspace: tape_workspace_bytes(n, len), its first bytes are the tape_result_dev afterwards
// tok (optional): the token stream of the list (tok[i] = buf[idx[i]], sjgpu_stage1_tokens_device): the front then reads it instead of gathering
const int *launch_tape_front(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint32_t n, uint32_t max_depth, void *workspace, hipStream_t s,
                             const uint8_t *tok = nullptr);
// deep: enqueue the sort's second pass (documents nested 64 deep and more).  Without it a deeper document comes back with max_level >= 64 in the result and
// a tape that is NOT valid: the caller runs the three launches again with deep = true (sjgpu_stage2_device: optimistic, five launches saved on nearly every call).
void launch_tape(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint32_t n, uint32_t max_depth, const uint32_t *str_offsets, strings_handoff strs,
                 uint8_t *string_buf, uint64_t *tape, uint64_t tape_cap, void *workspace, hipStream_t s, bool deep = true);
// ---- the tapes of a document stream (sjgpu_tape_many.hip: sjgpu_stage2_many_device) --------------------------------------------------------------
// launch_tape over a list that holds one document after the other (walk_document<STREAMING = true>): the FLAT tape -- word k of the whole list at
// flat_tape[k + 1], bracket payloads in those coordinates, no root words; room for 2 n + 2 words always suffices --, doc_flag[0 .. n] (1: the token has
// depth 0 in front of it and begins a document; the sentinel: 0) and doc_str[i], written for the tokens that carry a flag only: where the string records
// of their document begin.  res->tape_words = the words of the tokens alone.  launch_tape_front is the single document's.
void launch_tape_stream(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint32_t n, uint32_t max_depth, const uint32_t *str_offsets, strings_handoff strs,
                        uint8_t *string_buf, uint64_t *flat_tape, uint64_t flat_cap, void *workspace, hipStream_t s, bool deep, int *doc_flag, uint32_t *doc_str);
// what the relocation reads of the tape workspace once launch_tape_stream has run: tokc[i + 2] = byte of token i, tpos[0 .. n] = flat tape positions,
// the result, and the device word that holds n + 1 (the length of a scan over per-token arrays)
struct tape_stream_view {
  const uint8_t *tokc;
  const int *tpos;
  tape_result_dev *res;
  const uint32_t *n_plus_1;
};
tape_stream_view tape_workspace_view(void *workspace, uint32_t n, uint64_t len);
// One entry of the document table (include/sjgpu_stream.h: sjgpu_doc_span, the same four words)
struct doc_span_dev {
  uint32_t first_token, byte_begin, tape_begin, string_begin;
};
// what one run over the list leaves for the host, 16 bytes: the documents the list holds, and -- when the tape's or the strings' result carries an
// error -- the first token of the document that holds the offending list index and its byte offset (a cut between two documents)
struct many_result_dev {
  uint32_t docs, cut_token, cut_byte, has_error;
};
struct many_workspace {
  uint64_t *flat_tape; // 2 n + 4 words
  int *doc_ord;        // n + 1: the flags, then (scanned in place) the documents that begin in front of token i
  uint32_t *doc_str;   // n + 1
  int *partial;        // the scan's block sums
  size_t flat_cap, bytes;
};
many_workspace carve_many_workspace(void *base, uint32_t n);
size_t many_workspace_bytes(uint32_t n, uint64_t len);
// behind launch_tape_stream: doc_ord becomes the exclusive scan of the flags; *out = the number of documents and, from the smaller of the two results'
// error keys, the cut in front of the broken document
void launch_many_ordinals(const uint32_t *idx, uint32_t n, const many_workspace &m, const tape_stream_view &v, const strings_result_dev *sres, many_result_dev *out,
                          hipStream_t s);
// behind that, for a run WITHOUT an error and with room for everything (docs + 1 table entries, flat words + 2 docs tape words): the document table and
// the tapes, document by document
// (docs, total_words: what the host read back -- the table has docs + 1 entries, nothing is written at or beyond tape[total_words]; table: 16-byte aligned)
void launch_many_relocate(const uint32_t *idx, uint32_t n, uint32_t docs, uint64_t total_words, const many_workspace &m, const tape_stream_view &v,
                          const strings_result_dev *sres, doc_span_dev *table, uint64_t *tape, hipStream_t s);
// ---- queries over device tapes (sjgpu_query.hip: sjgpu_at_pointers_device, sjgpu_gather_strings_device) ------------------------------------------
// *bad |= 1 (a device word the caller cleared) when the table's tape_begin / string_begin run backwards or its last entry lies beyond the arrays
void launch_query_check_table(const doc_span_dev *table, uint32_t docs, uint64_t tape_words, uint64_t string_bytes, uint32_t *bad, hipStream_t s);
// program: what compile_query_program (sj_query_program.h) left, in device memory, 16-byte aligned; K >= 1, docs >= 1; a table that passed the check
void launch_at_pointers(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program, uint32_t tokens_at,
                        uint32_t keys_at, uint32_t K, uint64_t *value, uint8_t *tag, hipStream_t s);
// the same walk rooted at the cells of one row (include/sjgpu_rows.h): k_rows_locate settles every root once in where[0 .. rows) (device memory), k_at_pointers_rooted
// walks the K * rows cells.  K >= 1, rows >= 1, docs >= 0; a table that passed the check
void launch_at_pointers_rooted(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag,
                               uint32_t rows, uint32_t *where, const uint8_t *program, uint32_t tokens_at, uint32_t keys_at, uint32_t K, uint64_t *value, uint8_t *tag,
                               hipStream_t s);
// offsets[0 .. docs] = exclusive sum of the string cells' lengths; -> the device address of the 64-bit total (workspace: gather_workspace_bytes(docs), 256-byte aligned)
size_t gather_workspace_bytes(uint32_t docs);
const void *launch_gather_offsets(const uint64_t *value, const uint8_t *tag, uint32_t docs, uint64_t string_bytes, uint32_t *offsets, void *workspace, hipStream_t s);
// total: what the host read back and found to fit chars
void launch_gather_copy(const uint8_t *string_buf, const uint64_t *value, const uint32_t *offsets, uint32_t docs, uint64_t total, uint8_t *chars, hipStream_t s);
// ---- paths with wildcards over device tapes (sjgpu_query.hip: sjgpu_at_paths_device) ---------------------------------------------------------------
// program: what compile_path_program (sj_path_program.h) left, in device memory, 16-byte aligned; K >= 1, docs >= 1, K * docs + 1 entries the scan takes;
// a table that passed the check.  launch_paths_count: status[c] and, in offsets[0 .. K * docs], the exclusive sum of the cells' match counts;
// -> the device address of the 64-bit total (workspace: paths_workspace_bytes(K, docs), 256-byte aligned).
size_t paths_workspace_bytes(uint32_t K, uint32_t docs);
const void *launch_paths_count(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program, uint32_t levels_at,
                               uint32_t tokens_at, uint32_t keys_at, uint32_t K, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s);
// behind it, when the total fits: match j of cell c to value / tag[offsets[c] + j], never at or beyond offsets[c + 1]
void launch_paths_fill(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program, uint32_t levels_at, uint32_t tokens_at,
                       uint32_t keys_at, uint32_t K, const uint32_t *offsets, uint64_t *value, uint8_t *tag, hipStream_t s);
// ---- the paths rooted at the cells of one row (sjgpu_query.hip: sjgpu_at_paths_from_cells_device, include/sjgpu_lists.h) ------------------------------------------
// launch_paths_count / launch_paths_fill with `rows` root cells in the place of the documents: K >= 1, rows >= 1, docs >= 0, K * rows + 1 entries the scan takes,
// workspace paths_workspace_bytes(K, rows); where[0 .. rows) (device memory): the roots' verdicts, which k_rows_locate leaves in front of the count and the fill reads again
const void *launch_paths_rooted_count(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value,
                                      const uint8_t *root_tag, uint32_t rows, uint32_t *where, const uint8_t *program, uint32_t levels_at, uint32_t tokens_at, uint32_t keys_at,
                                      uint32_t K, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s);
void launch_paths_rooted_fill(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, const uint64_t *root_value, uint32_t rows, const uint32_t *where,
                              const uint8_t *program, uint32_t levels_at, uint32_t tokens_at, uint32_t keys_at, uint32_t K, const uint32_t *offsets, uint64_t *value, uint8_t *tag,
                              hipStream_t s);
// ---- the fields of the cells' objects, the sizes of the cells' containers (sjgpu_query.hip: sjgpu_object_fields_from_cells_device, sjgpu_cell_sizes_device,
// include/sjgpu_fields.h) ----------------------------------------------------------------------------------------------------------------------------------------
// rows >= 1, docs >= 0, rows + 1 entries the scan takes; a table that passed the check; where[0 .. rows) (device memory): k_rows_locate's verdicts, made here.
// launch_object_fields_count: status[r] and, in offsets[0 .. rows], the exclusive sum of the roots' field counts (an opening word's count field; walked only where it
// reads saturated) -> the device address of the 64-bit total (workspace: paths_workspace_bytes(1, rows), 256-byte aligned).  launch_object_fields_fill, when the total
// fits: field j of root r to the four rows at offsets[r] + j, never at or beyond offsets[r + 1]; what the walk did not reach below it is padded (tags 20, words 0).
const void *launch_object_fields_count(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows,
                                       uint32_t *where, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s);
void launch_object_fields_fill(const uint64_t *tape, const uint8_t *string_buf, const doc_span_dev *table, const uint64_t *root_value, uint32_t rows, const uint32_t *where,
                               const uint32_t *offsets, uint64_t *key_value, uint8_t *key_tag, uint64_t *value, uint8_t *tag, hipStream_t s);
// size[r] / code[r]: the count field of a located container's opening word and 0, or 0 and the root's code (a scalar: INCORRECT_TYPE)
void launch_cell_sizes(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows, uint32_t *where,
                       uint32_t *size, uint8_t *code, hipStream_t s);
// ---- what k_rows_locate leaves per root, for every unit that reads it (sjgpu_query.hip, sjgpu_json.hip) --------------------------------------------------------
//   d < ROWS_SPECIAL             a container cell that agrees with the tape: the document it lies in
//   ROWS_SPECIAL                 a scalar root
//   ROWS_SPECIAL | (code - 16)   a root that answers `code`: rows_code
constexpr uint32_t ROWS_SPECIAL = 0xFFFFFFF0u;
constexpr uint32_t rows_code(uint32_t m) { return (m & 15u) + 16u; }
// where[0 .. rows) (device memory) = the verdicts of the rows root cells; rows >= 1, docs >= 0, a table that passed the check
void launch_rows_locate(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows, uint32_t *where,
                        hipStream_t s);
// what a count leaves in front of its scan, 16 bytes of device memory: the sum of the per-cell counts in 64 bits (the scan's words wrap at 2^32) and entries + 1, the
// length of the scan.  launch_count_total: one workgroup adds the count kernel's `blocks` block sums
struct count_total_dev {
  uint64_t total;
  uint32_t n_plus_1, pad;
};
void launch_count_total(const uint64_t *block_sums, uint32_t blocks, uint32_t entries, count_total_dev *ctrl, hipStream_t s);
// ---- the same cells, breadth first (sjgpu_query.hip: sjgpu_at_paths_wide_device) ------------------------------------------------------------------------
// The whole call behind the table check, K >= 1 and docs >= 1: the annotation of the tape (a head bit and a nesting depth per word), the starting frontier, the
// levels of every path with their 4-byte read-backs of frontier sizes (into *readback: host memory, pinned where the copy is a real one), statuses, offsets and
// the total in *matches_out; then, when the total fits match_cap and 32 bits, the levels once more for every path but the last (whose list is still there) and
// the matches into value / tag.  Waits for the stream.  program / program_host: compile_path_program's bytes in device memory (16-byte aligned) and on the host.
// Workspace: 256-byte aligned, 25 bytes per tape word (head 1, depth 4, two frontiers 4 + 4, extents 4, child ranks 4, counts 4) + 4 per document + the scans'
// block sums; 12 more per document where there are more documents than tape words.  The paths share it, K does not enter.
size_t paths_wide_workspace_bytes(uint32_t K, uint32_t docs, uint64_t tape_words);
hipError_t launch_paths_wide(const uint64_t *tape, uint64_t tape_words, const uint8_t *string_buf, const doc_span_dev *table, uint32_t docs, const uint8_t *program,
                             const uint8_t *program_host, uint32_t levels_at, uint32_t tokens_at, uint32_t keys_at, uint32_t K, uint32_t *offsets, uint8_t *status,
                             uint64_t *value, uint8_t *tag, uint64_t match_cap, void *workspace, uint32_t *readback, hipStream_t s, uint64_t *matches_out);
// ---- typed getters over cells (sjgpu_cast.hip: sjgpu_cell_kinds_device, sjgpu_cast_cells_device, include/sjgpu_cast.h) --------------------------------------
// What the two calls refuse before anything is enqueued (the C-ABI adds the null context): K beyond CAST_MAX_ROWS, the alignments, with K > 0 a null census / counts
// block / getter list or a getter outside 1 .. 7, with K * n > 0 any other null pointer.  The CPU tier asks the same functions.
constexpr uint32_t CAST_MAX_ROWS = 64;
inline bool cast_misaligned(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }
inline bool cell_kinds_args_ok(const void *value, const void *tag, uint32_t n, uint32_t K, const void *kinds) {
  if (K > CAST_MAX_ROWS || cast_misaligned(value, 8) || cast_misaligned(kinds, 4)) { return false; }
  if (K && !kinds) { return false; }
  return !(K && n) || (value && tag);
}
inline bool cast_cells_args_ok(const void *value, const void *tag, uint32_t n, uint32_t K, const uint8_t *getters, const void *value_out, const void *code_out,
                               const void *valid_out, const void *counts) {
  if (K > CAST_MAX_ROWS || cast_misaligned(value, 8) || cast_misaligned(value_out, 8) || cast_misaligned(valid_out, 8) || cast_misaligned(counts, 4)) { return false; }
  if (K && (!counts || !getters)) { return false; }
  for (uint32_t k = 0; k < K; k++) {
    if (getters[k] < 1 || getters[k] > 7) { return false; }
  }
  return !(K && n) || (value && tag && value_out && code_out && valid_out);
}
// Arguments that passed the check, 1 <= K <= CAST_MAX_ROWS.  A memset of the K * 16 (K * 4) counters and, when n > 0, one launch of K rows of workgroups; the
// getters ride in the kernel's arguments.  -> what the memset returned (the launch's error is hipGetLastError's)
hipError_t launch_cell_kinds(const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t K, uint32_t *kinds, hipStream_t s);
hipError_t launch_cast_cells(const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t K, const uint8_t *getters, uint64_t *value_out, uint8_t *code_out,
                             uint64_t *valid_out, uint32_t *counts, hipStream_t s);
// ---- numbers held in strings (sjgpu_cast_strings.hip: sjgpu_cast_string_cells_device, include/sjgpu_cast_strings.h) ------------------------------------------
// What the call refuses before anything is enqueued (the C-ABI adds the null context): the cast's table with the getters 1 .. 3, optionally or-ed with 0x10, and
// a null string buffer while it has bytes and there are cells.  The CPU tier asks the same function.
inline bool cast_string_cells_args_ok(const void *string_buf, uint64_t string_bytes, const void *value, const void *tag, uint32_t n, uint32_t K, const uint8_t *getters,
                                      const void *value_out, const void *code_out, const void *valid_out, const void *counts) {
  if (K > CAST_MAX_ROWS || cast_misaligned(value, 8) || cast_misaligned(value_out, 8) || cast_misaligned(valid_out, 8) || cast_misaligned(counts, 4)) { return false; }
  if (K && (!counts || !getters)) { return false; }
  for (uint32_t k = 0; k < K; k++) {
    if ((getters[k] & 0x0Fu) < 1 || (getters[k] & 0x0Fu) > 3 || (getters[k] & 0xE0u)) { return false; }
  }
  return !(K && n) || (value && tag && value_out && code_out && valid_out && (string_buf || !string_bytes));
}
// Arguments that passed the check, 1 <= K <= CAST_MAX_ROWS.  A memset of the K * 8 counters and, when n > 0, two launches: the kernel that settles what fits
// its registers and the one that decides the cells it parked (it leaves at once where there are none).  -> what the memset returned
hipError_t launch_cast_string_cells(const uint8_t *string_buf, uint64_t string_bytes, const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t K, const uint8_t *getters,
                                    uint64_t *value_out, uint8_t *code_out, uint64_t *valid_out, uint32_t *counts, hipStream_t s);
// ---- a dictionary of a row of string cells, the census per code (sjgpu_dict.hip: sjgpu_dictionary_encode_device, sjgpu_cell_kinds_by_code_device,
// include/sjgpu_dict.h) -----------------------------------------------------------------------------------------------------------------------------------------
// What the two calls refuse before anything is read or enqueued (the C-ABI adds the null context and *distinct_out); the CPU tier asks the same functions.
constexpr uint32_t DICT_MAX_ROWS = 1u << 30; // the table has 2 n slots at the least, and a slot's index is a u32 whose top value means "none"
inline bool dict_encode_args_ok(const void *string_buf, uint64_t string_bytes, const void *value_row, const void *tag_row, uint32_t n, const void *codes, const void *dict_value,
                                const void *dict_tag, const void *dict_first, const void *dict_count, uint64_t dict_cap) {
  if (n > DICT_MAX_ROWS || string_bytes > 0xFFFFFFFFull) { return false; }
  if (cast_misaligned(value_row, 8) || cast_misaligned(dict_value, 8) || cast_misaligned(codes, 4) || cast_misaligned(dict_first, 4) || cast_misaligned(dict_count, 4)) { return false; }
  if (!string_buf || (n && (!value_row || !tag_row || !codes))) { return false; }
  return !dict_cap || (dict_value && dict_tag && dict_first && dict_count);
}
inline bool cell_kinds_by_code_args_ok(const void *codes, const void *value, const void *tag, uint32_t n, uint32_t groups, const void *kinds) {
  if (cast_misaligned(codes, 4) || cast_misaligned(value, 8) || cast_misaligned(kinds, 4) || uint64_t(groups) * 16 > 0xFFFFFFFFull) { return false; }
  if (groups && !kinds) { return false; }
  return !(groups && n) || (codes && value && tag);
}
// what the encode leaves for the host, 8 bytes at a 4-byte aligned address of the workspace: the distinct strings, and non-zero when a probe ran out of slots
struct dict_result_dev {
  uint32_t distinct, failed;
};
// Arguments that passed the check, 1 <= n <= DICT_MAX_ROWS; workspace: dict_workspace_bytes(n), 256-byte aligned.  Three memsets, the insert, the heads, the scan
// and the codes: codes[0 .. n) are complete when they have run, *result is where the dict_result_dev lies.  -> what the memsets returned
size_t dict_workspace_bytes(uint32_t n);
hipError_t launch_dict_encode(const uint64_t *value, const uint8_t *tag, uint32_t n, const uint8_t *string_buf, uint64_t string_bytes, int32_t *codes, void *workspace,
                              hipStream_t s, const dict_result_dev **result);
// behind it, over the same workspace, when the distinct strings fit: entry j of the four arrays for every j < distinct
void launch_dict_fill(const uint64_t *value, uint32_t n, void *workspace, uint64_t *dict_value, uint8_t *dict_tag, uint32_t *dict_first, uint32_t *dict_count, hipStream_t s);
// a memset of the groups * 16 counters and, when n > 0, one launch: up to 512 groups the histogram lies in LDS, above that every cell adds to global memory
hipError_t launch_cell_kinds_by_code(const int32_t *codes, const uint64_t *value, const uint8_t *tag, uint32_t n, uint32_t groups, uint32_t *kinds, hipStream_t s);
// ---- a map column pivoted into a record table (sjgpu_pivot.hip: sjgpu_pivot_fields_device, include/sjgpu_pivot.h) ------------------------------------------------
// What the call refuses before anything is enqueued (the C-ABI adds the null context); the CPU tier asks the same function.
constexpr uint64_t PIVOT_MAX_CELLS = 0xFFFFFFF0ull;
inline bool pivot_args_ok(const void *offsets, const void *status, uint32_t rows, const void *codes, const void *value, const void *tag, uint64_t fields,
                          const void *column_of_code, uint32_t groups, uint32_t columns, const void *value_out, const void *tag_out) {
  if (uint64_t(columns) * rows > PIVOT_MAX_CELLS || fields > 0xFFFFFFFFull) { return false; }
  if (cast_misaligned(value, 8) || cast_misaligned(value_out, 8) || cast_misaligned(offsets, 4) || cast_misaligned(codes, 4) || cast_misaligned(column_of_code, 4)) { return false; }
  if (uint64_t(columns) * rows > 0 && (!offsets || !status || !value_out || !tag_out)) { return false; }
  if (fields > 0 && (!codes || !value || !tag)) { return false; }
  return !(column_of_code && groups == 0);
}
// Arguments that passed the check, rows >= 1, columns >= 1: the fill (every cell's default) and, behind it, the scatter (one lane per row, its slots from the last
// to the first).  Two launches, nothing else.
void launch_pivot_fields(const uint32_t *offsets, const uint8_t *status, uint32_t rows, const int32_t *codes, const uint64_t *value, const uint8_t *tag, uint32_t fields,
                         const int32_t *column_of_code, uint32_t groups, uint32_t columns, uint64_t *value_out, uint8_t *tag_out, hipStream_t s);
// ---- cells as JSON text (sjgpu_json.hip: sjgpu_serialize_cells_device, include/sjgpu_json.h) -----------------------------------------------------------------
// rows >= 1, docs >= 0, rows + 1 entries the scan takes; a table that passed the check; where[0 .. rows) (device memory): k_rows_locate's verdicts, made here;
// workspace: json_workspace_bytes(rows), 256-byte aligned, the same for both launches.  launch_json_count: status[r] and, in offsets[0 .. rows], the exclusive sum of the
// cells' text lengths -> where the 64-bit total lies.  launch_json_fill, when the total fits: the bytes of cell r to chars[offsets[r] .. offsets[r + 1]), never beyond
size_t json_workspace_bytes(uint32_t rows);
const count_total_dev *launch_json_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value,
                                         const uint8_t *root_tag, uint32_t rows, uint32_t *where, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s);
void launch_json_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                      uint32_t rows, const uint32_t *where, const uint32_t *offsets, uint8_t *chars, void *workspace, hipStream_t s);
// (launch_pretty_*: the same launches around the kernels' PRETTY instantiations, sjgpu_prettify_cells_device of include/sjgpu_pretty.h; the same workspace)
const count_total_dev *launch_pretty_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value,
                                           const uint8_t *root_tag, uint32_t rows, uint32_t *where, uint32_t *offsets, uint8_t *status, void *workspace, hipStream_t s);
void launch_pretty_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                        uint32_t rows, const uint32_t *where, const uint32_t *offsets, uint8_t *chars, void *workspace, hipStream_t s);
// ---- cells as JSON text, breadth first (sjgpu_json_wide.hip: sjgpu_serialize_cells_wide_device, include/sjgpu_json_wide.h) -------------------------------------
// rows >= 1, docs >= 0; a table that passed the check.  Two blocks of device memory, both 256-byte aligned: root_space, json_wide_root_bytes(rows), which holds the
// verdicts of k_rows_locate (json_wide_where), the roots' first slots and their flags; word_space, json_wide_word_bytes(rows, R), asked for once R is known.
// launch_json_wide_extents: locate, the extents and their scan -> where R, the size of the range space, lies in 64 bits (->total).  R <= 0xFFFFFFF0 is the caller's to
// check.  launch_json_wide_count: status[r] and offsets[0 .. rows], -> *total: where the 64-bit total of the texts lies; -> what the memsets returned.
// launch_json_wide_fill, when the total fits: the bytes of cell r to chars[offsets[r] .. offsets[r + 1]), never beyond.  json_wide_share: the slots of one workgroup
// (a wave's share is 64 of them, a lane's 1), for the tests that stand on their edges
size_t json_wide_root_bytes(uint32_t rows);
size_t json_wide_word_bytes(uint32_t rows, uint64_t range_words);
uint32_t *json_wide_where(void *root_space, uint32_t rows);
uint32_t json_wide_share();
const count_total_dev *launch_json_wide_extents(const uint64_t *tape, const doc_span_dev *table, uint32_t docs, const uint64_t *root_value, const uint8_t *root_tag, uint32_t rows,
                                                void *root_space, hipStream_t s);
hipError_t launch_json_wide_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value,
                                  const uint8_t *root_tag, uint32_t rows, uint64_t range_words, uint32_t *offsets, uint8_t *status, void *root_space, void *word_space,
                                  hipStream_t s, const count_total_dev **total);
void launch_json_wide_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                           uint32_t rows, uint64_t range_words, uint8_t *chars, void *root_space, void *word_space, hipStream_t s);
// (launch_pretty_wide_*: sjgpu_prettify_cells_wide_device of include/sjgpu_pretty.h, behind the same launch_json_wide_extents and over the same two blocks)
hipError_t launch_pretty_wide_count(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value,
                                    const uint8_t *root_tag, uint32_t rows, uint64_t range_words, uint32_t *offsets, uint8_t *status, void *root_space, void *word_space,
                                    hipStream_t s, const count_total_dev **total);
void launch_pretty_wide_fill(const uint64_t *tape, const uint8_t *string_buf, uint64_t string_bytes, const doc_span_dev *table, const uint64_t *root_value, const uint8_t *root_tag,
                             uint32_t rows, uint64_t range_words, uint8_t *chars, void *root_space, void *word_space, hipStream_t s);
// ---- typed columns as JSON records (sjgpu_write.hip: sjgpu_write_records_device, include/sjgpu_write.h) -----------------------------------------------------
// One column as the kernels read it, K of them in device memory (sj_write_table.h makes them from the caller's sjgpu_write_column and escapes the keys):
// key_at / key_len: the column's escaped "key": prefix inside the `keys` bytes.
struct write_column_dev {
  const uint64_t *values, *valid;
  const uint32_t *offsets;
  const uint8_t *chars;
  uint64_t chars_bytes;
  uint32_t kind, key_at, key_len, pad;
};
constexpr uint32_t WRITE_MAX_COLUMNS = 64, WRITE_MAX_KEY = 1024, WRITE_MAX_PREFIXES = 8192;
// n >= 1, n + 1 entries the scan takes; cols[0 .. K) and keys in device memory; workspace: write_workspace_bytes(n), 256-byte aligned.  launch_write_count: status[r],
// the four counts (zeroed here, on the same stream) and, in offsets[0 .. n], the exclusive sum of the rows' text lengths -> where the 64-bit total lies.
// launch_write_fill, when the total fits: the bytes of row r to chars[offsets[r] .. offsets[r + 1]), never beyond
size_t write_workspace_bytes(uint32_t n);
const count_total_dev *launch_write_count(const write_column_dev *cols, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, uint32_t *offsets, uint8_t *status,
                                          uint64_t *counts, void *workspace, hipStream_t s);
void launch_write_fill(const write_column_dev *cols, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, const uint32_t *offsets, uint8_t *chars, hipStream_t s);
// the rows one workgroup iteration takes, the grid's cap and the LDS window of the staged road, for the tests that stand on their edges
uint32_t write_rows_per_step();
uint32_t write_max_workgroups();
uint32_t write_window_bytes();
// ---- list columns and array rows as nested JSON (sjgpu_write.hip: sjgpu_write_nested_device, include/sjgpu_nested.h) ----------------------------------------
// One field as the kernels read it (sj_nested_table.h makes them from the caller's sjgpu_write_field): list_offsets == nullptr: `col` is a plain column over the
// rows; otherwise `col` is the ELEMENTS, `elements` of them, and row r's list is list_offsets[r] .. list_offsets[r + 1]
struct write_field_dev {
  write_column_dev col;
  const uint32_t *list_offsets;
  const uint64_t *list_valid;
  uint64_t elements;
};
// as launch_write_count / launch_write_fill, with the same workspace (write_workspace_bytes(n)); SIX counts
const count_total_dev *launch_nested_count(const write_field_dev *fields, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, uint32_t *offsets, uint8_t *status,
                                           uint64_t *counts, void *workspace, hipStream_t s);
void launch_nested_fill(const write_field_dev *fields, const uint8_t *keys, uint32_t K, uint32_t n, uint32_t flags, const uint32_t *offsets, uint8_t *chars, hipStream_t s);
// On-Demand's raw key comparison over the whole list (sjgpu_strings.hip); names_block: [u32 lens[K]][name bytes back to back] in device memory
void launch_match_keys(const uint8_t *buf, uint64_t len, const uint32_t *idx, uint32_t n, const uint8_t *names_block, uint32_t K, uint32_t *out, uint32_t *matches,
                       hipStream_t s);
// in-place exclusive scan of a[0 .. *n_ptr) (n_max >= *n_ptr sizes the grid); partial: blocks_for(n_max, 4096) + 64 ints (sjgpu_finish.hip)
void enqueue_scan(int *a, uint32_t n_max, const uint32_t *n_ptr, int *partial, hipStream_t s);
// in-place exclusive scan of a[0 .. count), count <= 2^20, by one workgroup (sjgpu_finish.hip: k_scan_partials)
void launch_scan_partials(int *a, uint32_t count, hipStream_t s);

} // namespace sjgpu
#endif
