// simdjson_amd/csrc/sjgpu_capi_stage2.hip -- the C-ABI of include/sjgpu.h, include/sjgpu_stream.h, include/sjgpu_query.h, include/sjgpu_paths.h, include/sjgpu_rows.h, include/sjgpu_lists.h and include/sjgpu_cast.h, what follows the structural list on the device: the strings of a
// document, On-Demand's raw key comparison, stage 2 (the DOM tape of a document, the tapes of a document stream), sjgpu_parse and sjgpu_parse_many, and the queries over the tapes
// (JSON pointers -> typed columns, a string column -> offsets + characters).  Shared with the other units: sjgpu_ctx.h.
#include "sjgpu_ctx.h"
#include "sjgpu_query.h"
#include "sjgpu_paths.h"
#include "sjgpu_rows.h"
#include "sjgpu_lists.h"
#include "sjgpu_cast.h"
#include "sjgpu_cast_strings.h"
#include "sjgpu_fields.h"
#include "sjgpu_dict.h"
#include "sjgpu_pivot.h"
#include "sjgpu_json.h"
#include "sjgpu_json_wide.h"
#include "sjgpu_pretty.h"
#include "sjgpu_write.h"
#include "sj_path_program.h"
#include "sj_write_table.h"
#include "sj_nested_table.h"

extern "C" {

// ---- the strings of a document, unescaped (sjgpu_strings.hip) ----------------------------------------------------------------
int sjgpu_parse_strings_device(sjgpu_ctx *ctx, const void *buf_dev, size_t len, const void *idx_dev, uint32_t n, int allow_replacement,
                               void *string_buf_dev, size_t string_buf_bytes, void *offsets_dev, void *stream, uint64_t *bytes_out,
                               uint32_t *strings_out, uint32_t *first_bad_out) {
  if (!ctx || !buf_dev || !idx_dev || !string_buf_dev) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(buf_dev) & 3u) || (reinterpret_cast<uintptr_t>(offsets_dev) & 3u)) { return SJGPU_E_BADARG; }
  if (len > 2400000000ull || n >= 0xFFFFFFF0u) { return E_CAPACITY; } // record offsets are 32 bits: 5 (len + 1) / 3 bytes of records at most
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  // [result: 32 B, padded to 256][scratch of the string pass][offsets when the caller keeps none]
  const size_t scratch_at = 256, scratch = strings_scratch_bytes(n, len), offs_at = scratch_at + scratch;
  int rc = ensure_tmp(ctx, offs_at + (offsets_dev ? 0 : (size_t(n) + 1) * sizeof(uint32_t)));
  if (rc) { return rc; }
  uint8_t *tmp = static_cast<uint8_t *>(static_cast<void *>(ctx->d_tmp));
  strings_result_dev *res = reinterpret_cast<strings_result_dev *>(tmp);
  uint32_t *offsets = offsets_dev ? static_cast<uint32_t *>(offsets_dev) : reinterpret_cast<uint32_t *>(tmp + offs_at);
  hipStream_t s = pick(ctx, stream);
  // optimistic like stage 2: the stream compaction alone; a document it declines (path 2, nothing written) is run again through the per-string kernels
  strings_result_dev h;
  for (int roads = STRINGS_STREAM_ONLY;; roads = STRINGS_WALK_ONLY) {
    launch_parse_strings(static_cast<const uint8_t *>(buf_dev), len, static_cast<const uint32_t *>(idx_dev), n, allow_replacement != 0,
                         static_cast<uint8_t *>(string_buf_dev), string_buf_bytes, offsets, res, tmp + scratch_at, s, nullptr, roads);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    if (roads == STRINGS_WALK_ONLY || h.path != 2 || h.overflow) { break; }
  }
  ctx->last_string_path = h.path;
  if (bytes_out) { *bytes_out = h.bytes; }
  if (strings_out) { *strings_out = h.strings; }
  if (first_bad_out) { *first_bad_out = h.first_bad; }
  if (h.overflow) { return SJGPU_E_OVERFLOW; }
  return h.first_bad != 0xFFFFFFFFu ? 5 /* STRING_ERROR */ : 0;
}

int sjgpu_debug_string_path(const sjgpu_ctx *ctx) { return ctx ? int(ctx->last_string_path) : SJGPU_E_BADARG; }

// ---- On-Demand's raw key comparison (sjgpu_strings.hip) ---------------------------------------------------------------------------------
int sjgpu_match_keys_device(sjgpu_ctx *ctx, const void *buf_dev, size_t len, const void *idx_dev, uint32_t n, const uint8_t *names, const uint32_t *name_lens,
                            uint32_t K, void *match_dev, void *stream, uint32_t *matches_out) {
  if (!ctx || !buf_dev || !idx_dev || !match_dev || !names || !name_lens || K == 0 || K > 256u || (reinterpret_cast<uintptr_t>(match_dev) & 3u)) { return SJGPU_E_BADARG; }
  size_t total = 0;
  for (uint32_t k = 0; k < K; k++) { total += name_lens[k]; }
  if (total > (size_t(64) << 10)) { return SJGPU_E_BADARG; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  const size_t block = size_t(K) * sizeof(uint32_t) + total;
  int rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_stage2), &ctx->d_stage2_bytes, 256 + block);
  if (rc) { return rc; }
  std::vector<uint8_t> host(block);
  std::memcpy(host.data(), name_lens, size_t(K) * sizeof(uint32_t));
  std::memcpy(host.data() + size_t(K) * sizeof(uint32_t), names, total);
  hipStream_t s = pick(ctx, stream);
  uint32_t *d_matches = reinterpret_cast<uint32_t *>(ctx->d_stage2);
  uint8_t *d_block = ctx->d_stage2 + 256;
  SJ_TRY(ctx, hipMemcpyAsync(d_block, host.data(), block, hipMemcpyHostToDevice, s));
  SJ_TRY(ctx, hipStreamSynchronize(s)); // `host` leaves scope with this call
  launch_match_keys(static_cast<const uint8_t *>(buf_dev), len, static_cast<const uint32_t *>(idx_dev), n, d_block, K, static_cast<uint32_t *>(match_dev), d_matches, s);
  SJ_TRY(ctx, hipGetLastError());
  uint32_t m = 0;
  SJ_TRY(ctx, hipMemcpyAsync(&m, d_matches, sizeof m, hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (matches_out) { *matches_out = m; }
  return 0;
}

// ---- stage 2: the tape (sjgpu_tape.hip) -------------------------------------------------------------------------------------------------
int sjgpu_stage2_device(sjgpu_ctx *ctx, const void *buf_dev, size_t len, const void *idx_dev, uint32_t n, uint32_t max_depth, void *tape_dev,
                        size_t tape_cap_words, void *string_buf_dev, size_t string_buf_bytes, void *stream, uint64_t *tape_words_out,
                        uint64_t *string_bytes_out) {
  return sjgpu_stage2_tokens_device(ctx, buf_dev, len, idx_dev, n, nullptr, max_depth, tape_dev, tape_cap_words, string_buf_dev, string_buf_bytes, stream, tape_words_out,
                                    string_bytes_out);
}

int sjgpu_stage2_tokens_device(sjgpu_ctx *ctx, const void *buf_dev, size_t len, const void *idx_dev, uint32_t n, const void *tok_dev, uint32_t max_depth,
                               void *tape_dev, size_t tape_cap_words, void *string_buf_dev, size_t string_buf_bytes, void *stream, uint64_t *tape_words_out,
                               uint64_t *string_bytes_out) {
  if (!ctx || !buf_dev || !idx_dev || !tape_dev || !string_buf_dev || max_depth == 0 || max_depth > 4095u) { return SJGPU_E_BADARG; }
  // buf_dev: 16-byte aligned like every device entry point (the string stream's chunk loads are 16-byte loads of an aligned buffer)
  if ((reinterpret_cast<uintptr_t>(buf_dev) & 15u) || (reinterpret_cast<uintptr_t>(tape_dev) & 7u) || (reinterpret_cast<uintptr_t>(idx_dev) & 3u)) { return SJGPU_E_BADARG; }
  if (tape_words_out) { *tape_words_out = 0; }
  if (string_bytes_out) { *string_bytes_out = 0; }
  if (n == 0) { return E_EMPTY; } // walk_document: at_eof() (json_iterator.h:126)
  if (len > 2400000000ull || n >= 0xFFFFFFF0u) { return E_CAPACITY; } // the string pass's 32-bit record offsets
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  // [strings result 32 B, padded to 256][scratch of the string pass][string offsets, n + 1 words][tape workspace]
  const size_t scratch_at = 256, scratch = strings_scratch_bytes(n, len), offs_at = scratch_at + scratch;
  const size_t tape_at = (offs_at + (size_t(n) + 1) * sizeof(uint32_t) + 255) & ~size_t(255);
  int rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_stage2), &ctx->d_stage2_bytes, tape_at + tape_workspace_bytes(n, len));
  if (rc) { return rc; }
  uint8_t *ws = ctx->d_stage2;
  // the string pass's result lives in the tape workspace's first slot, 64 bytes behind the tape's own result (the slot has 256; k_tape_init clears it, k_strs_init
  // -- later in the stream -- fills it): both results come back in ONE copy (each copy is a 5 us launch of the runtime's copy kernel)
  strings_result_dev *sres = reinterpret_cast<strings_result_dev *>(ws + tape_at + 64);
  uint32_t *offsets = reinterpret_cast<uint32_t *>(ws + offs_at);
  hipStream_t s = pick(ctx, stream);
  // Optimistic: the string buffer by the stream compaction alone, the sort in one pass -- what nearly every document needs.  A document the stream declines
  // (a string the reference rejects, quotes glued to scalars, a look-back that settles nothing) or one nested 64 deep and more says so in its results and is
  // run again with the per-string kernels / the sort's second pass enqueued: ten launches that nearly always did nothing are gone from the common call.
  strings_result_dev hs;
  tape_result_dev ht;
  int roads = STRINGS_STREAM_ONLY;
  bool deep = false;
  for (;;) {
    const int *string_tokens = launch_tape_front(static_cast<const uint8_t *>(buf_dev), len, static_cast<const uint32_t *>(idx_dev), n, max_depth, ws + tape_at, s,
                                                 static_cast<const uint8_t *>(tok_dev));
    const strings_handoff strs = launch_parse_strings(static_cast<const uint8_t *>(buf_dev), len, static_cast<const uint32_t *>(idx_dev), n, false,
                                                      static_cast<uint8_t *>(string_buf_dev), string_buf_bytes, offsets, sres, ws + scratch_at, s, string_tokens, roads);
    launch_tape(static_cast<const uint8_t *>(buf_dev), len, static_cast<const uint32_t *>(idx_dev), n, max_depth, offsets, strs, static_cast<uint8_t *>(string_buf_dev),
                static_cast<uint64_t *>(tape_dev), tape_cap_words, ws + tape_at, s, deep);
    SJ_TRY(ctx, hipGetLastError());
    // (into page-locked memory: a copy into a variable on the stack goes through the runtime's staging buffer and waits for it, twice per call)
    uint8_t *const pinned = reinterpret_cast<uint8_t *>(ctx->h_result);
    static_assert(sizeof(strings_result_dev) <= 64 && sizeof(tape_result_dev) <= 64, "the pinned block's slots");
    SJ_TRY(ctx, hipMemcpyAsync(pinned + 64, ws + tape_at, 128, hipMemcpyDeviceToHost, s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    memcpy(&ht, pinned + 64, sizeof(ht));
    memcpy(&hs, pinned + 128, sizeof(hs));
    bool again = false;
    if (roads == STRINGS_STREAM_ONLY && hs.path == 2 && !hs.overflow) { roads = STRINGS_WALK_ONLY; again = true; }
    if (!deep && ht.max_level >= TAPE_ONE_PASS_LEVELS) { deep = true; again = true; }
    if (!again) { break; }
  }
  ctx->last_string_path = hs.path;
  // the first offender in list order decides; a string's content ranks behind its own position in the grammar (sj_tape_rules.h)
  uint64_t key = ht.error_key;
  if (hs.first_bad != 0xFFFFFFFFu) {
    const uint64_t sk = (uint64_t(hs.first_bad) << 8) | (2u << 4) | 5u; // STRING_ERROR
    if (sk < key) { key = sk; }
  }
  if (key != ~uint64_t(0)) { return int(key & 0xFu); }
  if (hs.overflow || ht.overflow) { return SJGPU_E_OVERFLOW; }
  if (tape_words_out) { *tape_words_out = ht.tape_words; }
  if (string_bytes_out) { *string_bytes_out = hs.bytes; }
  return 0;
}

// ---- stage 2 of a document stream: one tape per document (sjgpu_tape_many.hip) --------------------------------------------------------------
// One run over idx[0 .. n) of buf[0 .. len): the token front, the string pass, the STREAM tape into workspace, the document ordinals.  The results come
// back in one copy; the optimistic roads (string stream alone, the sort in one pass) are repeated like sjgpu_stage2_device repeats them.
namespace {
struct many_run {
  tape_result_dev ht;
  strings_result_dev hs;
  many_result_dev hm;
  many_workspace mw;
  tape_stream_view view;
  strings_result_dev *sres;
};
int run_many(sjgpu_ctx *ctx, const uint8_t *buf, size_t len, const uint32_t *idx, uint32_t n, uint32_t max_depth, uint8_t *string_buf, size_t string_buf_bytes,
             hipStream_t s, many_run *r) {
  // [strings result 32 B, padded to 256][scratch of the string pass][string offsets, n + 1 words][tape workspace][flat tape, ordinals, record starts]
  const size_t scratch_at = 256, scratch = strings_scratch_bytes(n, len), offs_at = scratch_at + scratch;
  const size_t tape_at = (offs_at + (size_t(n) + 1) * sizeof(uint32_t) + 255) & ~size_t(255);
  const size_t many_at = (tape_at + tape_workspace_bytes(n, len) + 255) & ~size_t(255);
  int rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_stage2), &ctx->d_stage2_bytes, many_at + many_workspace_bytes(n, len));
  if (rc) { return rc; }
  uint8_t *ws = ctx->d_stage2;
  // the tape workspace's first slot of 256 bytes, cleared by k_tape_init: [0] the tape's result, [64] the strings', [96] this unit's -- one copy of 128 bytes
  r->sres = reinterpret_cast<strings_result_dev *>(ws + tape_at + 64);
  many_result_dev *mres = reinterpret_cast<many_result_dev *>(ws + tape_at + 96);
  static_assert(sizeof(strings_result_dev) <= 32 && sizeof(many_result_dev) <= 32, "the slots of the result block");
  uint32_t *offsets = reinterpret_cast<uint32_t *>(ws + offs_at);
  r->mw = carve_many_workspace(ws + many_at, n);
  r->view = tape_workspace_view(ws + tape_at, n, len);
  int roads = STRINGS_STREAM_ONLY;
  bool deep = false;
  for (;;) {
    const int *string_tokens = launch_tape_front(buf, len, idx, n, max_depth, ws + tape_at, s, nullptr);
    const strings_handoff strs = launch_parse_strings(buf, len, idx, n, false, string_buf, string_buf_bytes, offsets, r->sres, ws + scratch_at, s, string_tokens, roads);
    launch_tape_stream(buf, len, idx, n, max_depth, offsets, strs, string_buf, r->mw.flat_tape, r->mw.flat_cap, ws + tape_at, s, deep, r->mw.doc_ord, r->mw.doc_str);
    launch_many_ordinals(idx, n, r->mw, r->view, r->sres, mres, s);
    SJ_TRY(ctx, hipGetLastError());
    uint8_t *const pinned = reinterpret_cast<uint8_t *>(ctx->h_result);
    SJ_TRY(ctx, hipMemcpyAsync(pinned + 64, ws + tape_at, 128, hipMemcpyDeviceToHost, s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    memcpy(&r->ht, pinned + 64, sizeof(r->ht));
    memcpy(&r->hs, pinned + 128, sizeof(r->hs));
    memcpy(&r->hm, pinned + 160, sizeof(r->hm));
    bool again = false;
    if (roads == STRINGS_STREAM_ONLY && r->hs.path == 2 && !r->hs.overflow) { roads = STRINGS_WALK_ONLY; again = true; }
    if (!deep && r->ht.max_level >= TAPE_ONE_PASS_LEVELS) { deep = true; again = true; }
    if (!again) { break; }
  }
  ctx->last_string_path = r->hs.path;
  return 0;
}
} // namespace

int sjgpu_stage2_many_device(sjgpu_ctx *ctx, const void *buf_dev, size_t len, const void *idx_dev, uint32_t n, uint32_t max_depth, void *tape_dev,
                             size_t tape_cap_words, void *string_buf_dev, size_t string_buf_bytes, void *docs_dev, size_t doc_cap, void *stream,
                             uint32_t *docs_out, uint64_t *tape_words_out, uint64_t *string_bytes_out) {
  if (docs_out) { *docs_out = 0; }
  if (tape_words_out) { *tape_words_out = 0; }
  if (string_bytes_out) { *string_bytes_out = 0; }
  if (!ctx || !buf_dev || !idx_dev || !tape_dev || !string_buf_dev || !docs_dev || max_depth == 0 || max_depth > 4095u) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(buf_dev) & 15u) || (reinterpret_cast<uintptr_t>(tape_dev) & 7u) || (reinterpret_cast<uintptr_t>(idx_dev) & 3u) ||
      (reinterpret_cast<uintptr_t>(docs_dev) & 15u)) { return SJGPU_E_BADARG; }
  if (n == 0) { return E_EMPTY; } // walk_document: at_eof() (json_iterator.h:126)
  if (len > 2400000000ull || n >= 0xFFFFFFF0u) { return E_CAPACITY; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  const uint8_t *buf = static_cast<const uint8_t *>(buf_dev);
  const uint32_t *idx = static_cast<const uint32_t *>(idx_dev);
  many_run r;
  int rc = run_many(ctx, buf, len, idx, n, max_depth, static_cast<uint8_t *>(string_buf_dev), string_buf_bytes, s, &r);
  if (rc) { return rc; }
  int code = 0;
  uint32_t n_run = n;
  if (r.hm.has_error) {
    // document_stream stops at the first broken document.  Its code is the smallest error key of the whole list; what is delivered is the list in front of
    // the document that holds that key -- run again, because a stray bracket behind the error may have paired with a bracket of an earlier document.
    uint64_t key = r.ht.error_key;
    if (r.hs.first_bad != 0xFFFFFFFFu) {
      const uint64_t sk = (uint64_t(r.hs.first_bad) << 8) | (2u << 4) | 5u; // STRING_ERROR
      if (sk < key) { key = sk; }
    }
    code = int(key & 0xFu);
    n_run = r.hm.cut_token;
    if (n_run == 0) { return code; } // the first document is the broken one
    const size_t len_run = r.hm.cut_byte; // idx[n_run]: the prefix ends where its sentinel would stand
    rc = run_many(ctx, buf, len_run, idx, n_run, max_depth, static_cast<uint8_t *>(string_buf_dev), string_buf_bytes, s, &r);
    if (rc) { return rc; }
    if (r.hm.has_error) { return E_UNEXPECTED; } // (a prefix of complete documents in front of the first error is valid)
  }
  if (r.hs.overflow || r.ht.overflow) { return SJGPU_E_OVERFLOW; }
  const uint32_t docs = r.hm.docs;
  const uint64_t total = r.ht.tape_words + 2ull * docs;
  if (total > 0x7FFFFFFFull) { return E_CAPACITY; } // tape positions are 31 bits
  if (size_t(docs) + 1 > doc_cap) {
    if (docs_out) { *docs_out = docs + 1; } // the entries the table needs
    return SJGPU_E_OVERFLOW;
  }
  if (total > tape_cap_words) { return SJGPU_E_OVERFLOW; }
  launch_many_relocate(idx, n_run, docs, total, r.mw, r.view, r.sres, static_cast<doc_span_dev *>(docs_dev), static_cast<uint64_t *>(tape_dev), s);
  SJ_TRY(ctx, hipGetLastError());
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (docs_out) { *docs_out = docs; }
  if (tape_words_out) { *tape_words_out = total; }
  if (string_bytes_out) { *string_bytes_out = r.hs.bytes; }
  return code;
}

int sjgpu_parse_many(sjgpu_ctx *ctx, const uint8_t *buf, size_t len, uint32_t max_depth, uint64_t *tape_out, size_t tape_cap_words, uint8_t *string_buf_out,
                     size_t string_buf_bytes, sjgpu_doc_span *docs_out_host, size_t doc_cap, uint32_t *docs_out, uint64_t *tape_words_out,
                     uint64_t *string_bytes_out) {
  if (docs_out) { *docs_out = 0; }
  if (tape_words_out) { *tape_words_out = 0; }
  if (string_bytes_out) { *string_bytes_out = 0; }
  if (!ctx || !tape_out || !string_buf_out || !docs_out_host) { return SJGPU_E_BADARG; }
  if (len > ctx->capacity) { return E_CAPACITY; }
  if (len == 0) { return E_EMPTY; }
  if (!buf) { return SJGPU_E_BADARG; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure_staging_in(ctx, len);
  if (rc) { return rc; }
  size_t idx_bytes = ctx->d_idx_words * sizeof(uint32_t);
  rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_idx), &idx_bytes, (grown(len) + 16) * sizeof(uint32_t));
  ctx->d_idx_words = idx_bytes / sizeof(uint32_t);
  if (rc) { return rc; }
  hipStream_t s = ctx->stream;
  SJ_TRY(ctx, hipMemcpyAsync(ctx->d_in, buf, len, hipMemcpyHostToDevice, s));
  sjgpu_scan_result res{0, 0, 0};
  for (int attempt = 0; attempt < 2; attempt++) { // a single-pass scan that gives up is re-run on the split pipeline
    enqueue_stage1(ctx, use_fused(ctx, len, 0) && attempt == 0, ctx->d_in, len, ctx->d_idx, ctx->d_idx_words, s, nullptr);
    SJ_ENQUEUED(ctx);
    rc = fetch_result(ctx, s, &res);
    if (rc) { return rc; }
    if (!(res.flags & SJGPU_F_INTERNAL)) { break; }
  }
  if (res.flags & (SJGPU_F_INTERNAL | SJGPU_F_IDX_OVERFLOW)) { return E_UNEXPECTED; }
  const int e1 = sjgpu_stage1_error_from_flags(res.n, res.flags); // (the errors of stage 1 concern the whole buffer and come first)
  if (e1) { return e1; }
  // [tapes: 4 n words always suffice, and so do len + 3 n (len + 3 per document)][table: n + 1 entries][string records]
  const size_t tape_words_cap = (size_t(res.n) < len ? 4 * size_t(res.n) : len + 3 * size_t(res.n)) + 8, table_at = tape_words_cap * sizeof(uint64_t), table_cap = size_t(res.n) + 1;
  const size_t str_at = (table_at + table_cap * sizeof(sjgpu_doc_span) + 255) & ~size_t(255), str_cap = 5 * (len / 3) + 256;
  rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_doc), &ctx->d_doc_bytes, str_at + str_cap);
  if (rc) { return rc; }
  uint64_t tw = 0, sb = 0;
  uint32_t docs = 0;
  const int code = sjgpu_stage2_many_device(ctx, ctx->d_in, len, ctx->d_idx, res.n, max_depth, ctx->d_doc, tape_words_cap, ctx->d_doc + str_at, str_cap,
                                            ctx->d_doc + table_at, table_cap, s, &docs, &tw, &sb);
  if (code < 0) { return code; }
  if (docs == 0) { return code; } // nothing delivered (the first document is broken)
  if (tw > tape_cap_words || sb > string_buf_bytes) { return SJGPU_E_OVERFLOW; }
  if (size_t(docs) + 1 > doc_cap) {
    if (docs_out) { *docs_out = docs + 1; }
    return SJGPU_E_OVERFLOW;
  }
  SJ_TRY(ctx, hipMemcpyAsync(tape_out, ctx->d_doc, tw * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  if (sb) { SJ_TRY(ctx, hipMemcpyAsync(string_buf_out, ctx->d_doc + str_at, sb, hipMemcpyDeviceToHost, s)); }
  SJ_TRY(ctx, hipMemcpyAsync(docs_out_host, ctx->d_doc + table_at, (size_t(docs) + 1) * sizeof(sjgpu_doc_span), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (docs_out) { *docs_out = docs; }
  if (tape_words_out) { *tape_words_out = tw; }
  if (string_bytes_out) { *string_bytes_out = sb; }
  return code;
}

int sjgpu_parse(sjgpu_ctx *ctx, const uint8_t *buf, size_t len, uint32_t max_depth, uint64_t *tape_out, size_t tape_cap_words, uint8_t *string_buf_out,
                size_t string_buf_bytes, uint64_t *tape_words_out, uint64_t *string_bytes_out) {
  if (!ctx || !tape_out || !string_buf_out) { return SJGPU_E_BADARG; }
  if (tape_words_out) { *tape_words_out = 0; }
  if (string_bytes_out) { *string_bytes_out = 0; }
  if (len > ctx->capacity) { return E_CAPACITY; }
  if (len == 0) { return E_EMPTY; }
  if (!buf) { return SJGPU_E_BADARG; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure_staging_in(ctx, len);
  if (rc) { return rc; }
  size_t idx_bytes = ctx->d_idx_words * sizeof(uint32_t);
  rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_idx), &idx_bytes, (grown(len) + 16) * sizeof(uint32_t));
  ctx->d_idx_words = idx_bytes / sizeof(uint32_t);
  if (rc) { return rc; }
  const size_t tape_words_cap = len + 8, str_cap = 5 * (len / 3) + 256, str_at = tape_words_cap * sizeof(uint64_t);
  rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_doc), &ctx->d_doc_bytes, str_at + str_cap);
  if (rc) { return rc; }
  hipStream_t s = ctx->stream;
  SJ_TRY(ctx, hipMemcpyAsync(ctx->d_in, buf, len, hipMemcpyHostToDevice, s));
  sjgpu_scan_result res{0, 0, 0};
  for (int attempt = 0; attempt < 2; attempt++) { // a single-pass scan that gives up is re-run on the split pipeline
    enqueue_stage1(ctx, use_fused(ctx, len, 0) && attempt == 0, ctx->d_in, len, ctx->d_idx, ctx->d_idx_words, s, nullptr);
    SJ_ENQUEUED(ctx);
    rc = fetch_result(ctx, s, &res);
    if (rc) { return rc; }
    if (!(res.flags & SJGPU_F_INTERNAL)) { break; }
  }
  if (res.flags & (SJGPU_F_INTERNAL | SJGPU_F_IDX_OVERFLOW)) { return E_UNEXPECTED; }
  const int e1 = sjgpu_stage1_error_from_flags(res.n, res.flags);
  if (e1) { return e1; }
  uint64_t tw = 0, sb = 0;
  rc = sjgpu_stage2_device(ctx, ctx->d_in, len, ctx->d_idx, res.n, max_depth, ctx->d_doc, tape_words_cap, ctx->d_doc + str_at, str_cap, s, &tw, &sb);
  if (rc) { return rc; }
  if (tw > tape_cap_words || sb > string_buf_bytes) { return SJGPU_E_OVERFLOW; }
  SJ_TRY(ctx, hipMemcpyAsync(tape_out, ctx->d_doc, tw * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  if (sb) { SJ_TRY(ctx, hipMemcpyAsync(string_buf_out, ctx->d_doc + str_at, sb, hipMemcpyDeviceToHost, s)); }
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (tape_words_out) { *tape_words_out = tw; }
  if (string_bytes_out) { *string_bytes_out = sb; }
  return 0;
}

// ---- queries over device tapes (sjgpu_query.hip) ---------------------------------------------------------------------------------------------
} // extern "C"

namespace {
// What sjgpu_at_pointers_device and sjgpu_at_pointers_from_cells_device do before their walk: the argument checks they share, the pointer program, K == 0 / no lanes,
// the wait for the context's previous walk, the context's block -- [0] the table check's word, [256] the program, [*extra_at] `extra` bytes more for the caller --, the
// upload and the table check.  lanes: the cells of one row (documents, or root cells).  -> 0 with *done = false: the program lies at ctx->d_query + 256 and the table
// passed; *done = true: the call is over with the code returned.
int pointers_begin(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev, uint32_t docs,
                   uint32_t lanes, const uint8_t *pointers, const uint32_t *pointer_lens, uint32_t K, void *value_dev, void *tag_dev, void *stream, size_t extra,
                   query_program *prog, size_t *extra_at, hipStream_t *stream_out, bool *done) {
  *done = true;
  if (!ctx || !tape_dev || !string_buf_dev || !docs_dev || !value_dev || !tag_dev || (K && (!pointers || !pointer_lens))) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(tape_dev) & 7u) || (reinterpret_cast<uintptr_t>(value_dev) & 7u) || (reinterpret_cast<uintptr_t>(docs_dev) & 15u)) { return SJGPU_E_BADARG; }
  if (tape_words > 0xFFFFFFFFull || string_bytes > 0xFFFFFFFFull || docs >= 0xFFFFFFF0u) { return SJGPU_E_BADARG; } // the table's words are 32 bits
  if (!compile_query_program(pointers, pointer_lens, K, prog)) { return SJGPU_E_BADARG; }
  if (K == 0 || lanes == 0) { return 0; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  // the blocks are the context's: the walk of the previous call must have read its pointers before they are overwritten
  if (ctx->query_in_flight) {
    SJ_TRY(ctx, hipEventSynchronize(ctx->ev_query));
    ctx->query_in_flight = false;
  }
  if (!ctx->ev_query) { SJ_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_query, hipEventDisableTiming)); }
  const size_t block = 256 + prog->bytes.size(); // what goes up
  *extra_at = (block + 255) & ~size_t(255);
  int rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_query), &ctx->d_query_bytes, extra ? *extra_at + extra : block);
  if (rc) { return rc; }
  if (ctx->h_query_bytes < block) {
    if (ctx->h_query) { (void)hipHostFree(ctx->h_query); ctx->h_query = nullptr; ctx->h_query_bytes = 0; }
    SJ_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_query), block, hipHostMallocDefault));
    ctx->h_query_bytes = block;
  }
  std::memset(ctx->h_query, 0, 256);
  std::memcpy(ctx->h_query + 256, prog->bytes.data(), prog->bytes.size());
  hipStream_t s = pick(ctx, stream);
  *stream_out = s;
  SJ_TRY(ctx, hipMemcpyAsync(ctx->d_query, ctx->h_query, block, hipMemcpyHostToDevice, s));
  launch_query_check_table(static_cast<const doc_span_dev *>(docs_dev), docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(ctx->d_query), s);
  SJ_TRY(ctx, hipGetLastError());
  uint32_t *const bad = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192); // (the pinned block's last slot: the scan and stage 2 use [0, 192))
  SJ_TRY(ctx, hipMemcpyAsync(bad, ctx->d_query, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (*bad) { return SJGPU_E_BADARG; }
  *done = false;
  return 0;
}
} // namespace

extern "C" {

int sjgpu_at_pointers_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                             uint32_t docs, const uint8_t *pointers, const uint32_t *pointer_lens, uint32_t K, void *value_dev, void *tag_dev, void *stream) {
  query_program prog;
  size_t extra_at = 0;
  hipStream_t s = nullptr;
  bool done = true;
  const int rc = pointers_begin(ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, docs, pointers, pointer_lens, K, value_dev, tag_dev, stream, 0, &prog,
                                &extra_at, &s, &done);
  if (done) { return rc; }
  launch_at_pointers(static_cast<const uint64_t *>(tape_dev), static_cast<const uint8_t *>(string_buf_dev), static_cast<const doc_span_dev *>(docs_dev), docs, ctx->d_query + 256,
                     prog.tokens_at, prog.keys_at, K, static_cast<uint64_t *>(value_dev), static_cast<uint8_t *>(tag_dev), s);
  SJ_TRY(ctx, hipGetLastError());
  SJ_TRY(ctx, hipEventRecord(ctx->ev_query, s));
  ctx->query_in_flight = true;
  return 0;
}

// the same walk rooted at the cells of one row (include/sjgpu_rows.h).  The roots' verdicts (k_rows_locate, 4 bytes per root) lie behind the program in the
// context's block: the event that guards the program guards them
int sjgpu_at_pointers_from_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                        uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, const uint8_t *pointers,
                                        const uint32_t *pointer_lens, uint32_t K, void *value_dev, void *tag_dev, void *stream) {
  if (!root_value_dev || !root_tag_dev || (reinterpret_cast<uintptr_t>(root_value_dev) & 7u) || rows >= 0xFFFFFFF0u) { return SJGPU_E_BADARG; }
  query_program prog;
  size_t where_at = 0;
  hipStream_t s = nullptr;
  bool done = true;
  const int rc = pointers_begin(ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, rows, pointers, pointer_lens, K, value_dev, tag_dev, stream,
                                size_t(rows) * sizeof(uint32_t), &prog, &where_at, &s, &done);
  if (done) { return rc; }
  launch_at_pointers_rooted(static_cast<const uint64_t *>(tape_dev), static_cast<const uint8_t *>(string_buf_dev), static_cast<const doc_span_dev *>(docs_dev), docs,
                            static_cast<const uint64_t *>(root_value_dev), static_cast<const uint8_t *>(root_tag_dev), rows, reinterpret_cast<uint32_t *>(ctx->d_query + where_at),
                            ctx->d_query + 256, prog.tokens_at, prog.keys_at, K, static_cast<uint64_t *>(value_dev), static_cast<uint8_t *>(tag_dev), s);
  SJ_TRY(ctx, hipGetLastError());
  SJ_TRY(ctx, hipEventRecord(ctx->ev_query, s));
  ctx->query_in_flight = true;
  return 0;
}

int sjgpu_gather_strings_device(sjgpu_ctx *ctx, const void *string_buf_dev, uint64_t string_bytes, const void *value_row_dev, const void *tag_row_dev, uint32_t docs,
                                void *offsets_dev, void *chars_dev, uint64_t chars_cap, void *stream, uint64_t *bytes_out) {
  if (bytes_out) { *bytes_out = 0; }
  if (!ctx || !string_buf_dev || !offsets_dev || (docs && (!value_row_dev || !tag_row_dev)) || (chars_cap && !chars_dev)) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(offsets_dev) & 3u) || (reinterpret_cast<uintptr_t>(value_row_dev) & 7u) || docs >= 0xFFFFFFF0u) { return SJGPU_E_BADARG; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure_tmp(ctx, gather_workspace_bytes(docs));
  if (rc) { return rc; }
  hipStream_t s = pick(ctx, stream);
  const uint64_t *value = static_cast<const uint64_t *>(value_row_dev);
  uint32_t *offsets = static_cast<uint32_t *>(offsets_dev);
  const void *total_dev = launch_gather_offsets(value, static_cast<const uint8_t *>(tag_row_dev), docs, string_bytes, offsets, ctx->d_tmp, s);
  SJ_TRY(ctx, hipGetLastError());
  uint64_t *const total = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  SJ_TRY(ctx, hipMemcpyAsync(total, total_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t bytes = *total;
  if (bytes_out) { *bytes_out = bytes; }
  if (bytes > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (bytes > chars_cap) { return SJGPU_E_OVERFLOW; }
  launch_gather_copy(static_cast<const uint8_t *>(string_buf_dev), value, offsets, docs, bytes, static_cast<uint8_t *>(chars_dev), s);
  SJ_TRY(ctx, hipGetLastError());
  SJ_TRY(ctx, hipStreamSynchronize(s));
  return 0;
}

// ---- paths with wildcards over device tapes (k_at_paths and the k_wide_* kernels in sjgpu_query.hip) -------------------------------------------------
} // extern "C"

namespace {
// What sjgpu_at_paths_device, sjgpu_at_paths_wide_device and sjgpu_at_paths_from_cells_device do before their first kernel: the argument checks they share, the level
// program, K == 0 / no lanes, the context's block -- [0] the table check's word, [256] the program, [*extra_at] `extra` bytes more for the caller -- and the road's
// workspace in d_tmp (wide: paths_wide_workspace_bytes, else paths_workspace_bytes), the upload and the table check.  lanes: the cells of one path (documents, or root
// cells).  -> 0 with *done = false: the program lies at ctx->d_query + 256 and the table passed; *done = true: the call is over with the code returned.
int paths_begin(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev, uint32_t docs,
                uint32_t lanes, const uint8_t *paths, const uint32_t *path_lens, uint32_t K, void *offsets_dev, void *status_dev, void *value_dev, void *tag_dev, uint64_t match_cap,
                void *stream, uint64_t *matches_out, bool wide, size_t extra, path_program *prog, size_t *extra_at, hipStream_t *stream_out, bool *done) {
  *done = true;
  if (matches_out) { *matches_out = 0; }
  if (!ctx || !tape_dev || !string_buf_dev || !docs_dev || !offsets_dev || !matches_out || (K && (!paths || !path_lens)) || (K && lanes && !status_dev) ||
      (match_cap && (!value_dev || !tag_dev))) {
    return SJGPU_E_BADARG;
  }
  if ((reinterpret_cast<uintptr_t>(tape_dev) & 7u) || (reinterpret_cast<uintptr_t>(value_dev) & 7u) || (reinterpret_cast<uintptr_t>(docs_dev) & 15u) ||
      (reinterpret_cast<uintptr_t>(offsets_dev) & 3u)) {
    return SJGPU_E_BADARG;
  }
  if (tape_words > 0xFFFFFFFFull || string_bytes > 0xFFFFFFFFull || docs >= 0xFFFFFFF0u || lanes >= 0xFFFFFFF0u) { return SJGPU_E_BADARG; } // the table's words are 32 bits
  if (!compile_path_program(paths, path_lens, K, prog)) { return SJGPU_E_BADARG; }
  if (uint64_t(K) * lanes + 1 > 0xFFFFFFF0ull) { return SJGPU_E_BADARG; } // the scan's entries are indexed by 32-bit words
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  *stream_out = s;
  if (K == 0 || lanes == 0) {
    SJ_TRY(ctx, hipMemsetAsync(offsets_dev, 0, sizeof(uint32_t), s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    return 0;
  }
  // the blocks are the context's: the walk of the previous call must have read its program before it is overwritten
  if (ctx->query_in_flight) {
    SJ_TRY(ctx, hipEventSynchronize(ctx->ev_query));
    ctx->query_in_flight = false;
  }
  const size_t block = 256 + prog->bytes.size(); // [0] the table check's word, [256] the program
  *extra_at = (block + 255) & ~size_t(255);
  int rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_query), &ctx->d_query_bytes, extra ? *extra_at + extra : block);
  if (rc) { return rc; }
  rc = ensure_tmp(ctx, wide ? paths_wide_workspace_bytes(K, docs, tape_words) : paths_workspace_bytes(K, lanes));
  if (rc) { return rc; }
  if (ctx->h_query_bytes < block) {
    if (ctx->h_query) { (void)hipHostFree(ctx->h_query); ctx->h_query = nullptr; ctx->h_query_bytes = 0; }
    SJ_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_query), block, hipHostMallocDefault));
    ctx->h_query_bytes = block;
  }
  std::memset(ctx->h_query, 0, 256);
  std::memcpy(ctx->h_query + 256, prog->bytes.data(), prog->bytes.size());
  SJ_TRY(ctx, hipMemcpyAsync(ctx->d_query, ctx->h_query, block, hipMemcpyHostToDevice, s));
  launch_query_check_table(static_cast<const doc_span_dev *>(docs_dev), docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(ctx->d_query), s);
  SJ_TRY(ctx, hipGetLastError());
  uint32_t *const bad = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192); // (the pinned block's last slot, as in sjgpu_at_pointers_device)
  SJ_TRY(ctx, hipMemcpyAsync(bad, ctx->d_query, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (*bad) { return SJGPU_E_BADARG; }
  *done = false;
  return 0;
}
} // namespace

extern "C" {

int sjgpu_at_paths_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev, uint32_t docs,
                          const uint8_t *paths, const uint32_t *path_lens, uint32_t K, void *offsets_dev, void *status_dev, void *value_dev, void *tag_dev, uint64_t match_cap,
                          void *stream, uint64_t *matches_out) {
  path_program prog;
  size_t extra_at = 0;
  hipStream_t s = nullptr;
  bool done = true;
  const int rc = paths_begin(ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, docs, paths, path_lens, K, offsets_dev, status_dev, value_dev, tag_dev,
                             match_cap, stream, matches_out, false, 0, &prog, &extra_at, &s, &done);
  if (done) { return rc; }
  uint32_t *offsets = static_cast<uint32_t *>(offsets_dev);
  const doc_span_dev *table = static_cast<const doc_span_dev *>(docs_dev);
  const uint64_t *tape = static_cast<const uint64_t *>(tape_dev);
  const uint8_t *sbuf = static_cast<const uint8_t *>(string_buf_dev);
  const void *total_dev = launch_paths_count(tape, sbuf, table, docs, ctx->d_query + 256, prog.levels_at, prog.tokens_at, prog.keys_at, K, offsets,
                                             static_cast<uint8_t *>(status_dev), ctx->d_tmp, s);
  SJ_TRY(ctx, hipGetLastError());
  uint64_t *const total = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  SJ_TRY(ctx, hipMemcpyAsync(total, total_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t matches = *total;
  *matches_out = matches;
  if (matches > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (matches > match_cap) { return SJGPU_E_OVERFLOW; }
  if (matches) {
    launch_paths_fill(tape, sbuf, table, docs, ctx->d_query + 256, prog.levels_at, prog.tokens_at, prog.keys_at, K, offsets, static_cast<uint64_t *>(value_dev),
                      static_cast<uint8_t *>(tag_dev), s);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s)); // (the program block and the workspace are free again when the call returns)
  }
  return 0;
}

// the same cells, breadth first: the level loop is launch_paths_wide's (sjgpu_query.hip), which the CPU tier runs too
int sjgpu_at_paths_wide_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev, uint32_t docs,
                               const uint8_t *paths, const uint32_t *path_lens, uint32_t K, void *offsets_dev, void *status_dev, void *value_dev, void *tag_dev,
                               uint64_t match_cap, void *stream, uint64_t *matches_out) {
  path_program prog;
  size_t extra_at = 0;
  hipStream_t s = nullptr;
  bool done = true;
  const int rc = paths_begin(ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, docs, paths, path_lens, K, offsets_dev, status_dev, value_dev, tag_dev,
                             match_cap, stream, matches_out, true, 0, &prog, &extra_at, &s, &done);
  if (done) { return rc; }
  uint32_t *const readback = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  uint64_t matches = 0;
  SJ_TRY(ctx, launch_paths_wide(static_cast<const uint64_t *>(tape_dev), tape_words, static_cast<const uint8_t *>(string_buf_dev), static_cast<const doc_span_dev *>(docs_dev), docs,
                                ctx->d_query + 256, prog.bytes.data(), prog.levels_at, prog.tokens_at, prog.keys_at, K, static_cast<uint32_t *>(offsets_dev),
                                static_cast<uint8_t *>(status_dev), static_cast<uint64_t *>(value_dev), static_cast<uint8_t *>(tag_dev), match_cap, ctx->d_tmp, readback, s, &matches));
  *matches_out = matches;
  if (matches > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (matches > match_cap) { return SJGPU_E_OVERFLOW; }
  return 0;
}

// the depth-first walk rooted at the cells of one row (include/sjgpu_lists.h).  The roots' verdicts (k_rows_locate, 4 bytes per root) lie behind the program in the
// context's block, made once in front of the count and read by both passes of all K paths
int sjgpu_at_paths_from_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                     uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, const uint8_t *paths, const uint32_t *path_lens, uint32_t K,
                                     void *offsets_dev, void *status_dev, void *value_dev, void *tag_dev, uint64_t match_cap, void *stream, uint64_t *matches_out) {
  if (matches_out) { *matches_out = 0; }
  if ((rows && (!root_value_dev || !root_tag_dev)) || (reinterpret_cast<uintptr_t>(root_value_dev) & 7u)) { return SJGPU_E_BADARG; }
  path_program prog;
  size_t where_at = 0;
  hipStream_t s = nullptr;
  bool done = true;
  const int rc = paths_begin(ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, rows, paths, path_lens, K, offsets_dev, status_dev, value_dev, tag_dev,
                             match_cap, stream, matches_out, false, size_t(rows) * sizeof(uint32_t), &prog, &where_at, &s, &done);
  if (done) { return rc; }
  uint32_t *offsets = static_cast<uint32_t *>(offsets_dev);
  const doc_span_dev *table = static_cast<const doc_span_dev *>(docs_dev);
  const uint64_t *tape = static_cast<const uint64_t *>(tape_dev);
  const uint8_t *sbuf = static_cast<const uint8_t *>(string_buf_dev);
  const uint64_t *root_value = static_cast<const uint64_t *>(root_value_dev);
  uint32_t *where = reinterpret_cast<uint32_t *>(ctx->d_query + where_at);
  const void *total_dev = launch_paths_rooted_count(tape, sbuf, table, docs, root_value, static_cast<const uint8_t *>(root_tag_dev), rows, where, ctx->d_query + 256, prog.levels_at,
                                                    prog.tokens_at, prog.keys_at, K, offsets, static_cast<uint8_t *>(status_dev), ctx->d_tmp, s);
  SJ_TRY(ctx, hipGetLastError());
  uint64_t *const total = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  SJ_TRY(ctx, hipMemcpyAsync(total, total_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t matches = *total;
  *matches_out = matches;
  if (matches > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (matches > match_cap) { return SJGPU_E_OVERFLOW; }
  if (matches) {
    launch_paths_rooted_fill(tape, sbuf, table, root_value, rows, where, ctx->d_query + 256, prog.levels_at, prog.tokens_at, prog.keys_at, K, offsets,
                             static_cast<uint64_t *>(value_dev), static_cast<uint8_t *>(tag_dev), s);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s)); // (the program block, the verdicts and the workspace are free again when the call returns)
  }
  return 0;
}

// ---- the fields and the sizes of the cells' containers (k_object_fields_count, k_object_fields_fill, k_cell_sizes in sjgpu_query.hip; include/sjgpu_fields.h) ----
} // extern "C"

namespace {
// What the two calls do before their first kernel, behind their own null checks: the checks on the tapes, the table and the roots that
// sjgpu_at_paths_from_cells_device makes, rows == 0, the wait for the context's previous walk, the context's block -- [0] the table check's word, [256] the roots'
// verdicts (4 bytes per root) --, `workspace` bytes of d_tmp and the table check.  -> 0 with *done = false: the table passed; *done = true: the call is over
int fields_begin(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, uint64_t string_bytes, const void *docs_dev, uint32_t docs, const void *root_value_dev,
                 const void *root_tag_dev, uint32_t rows, size_t workspace, void *stream, hipStream_t *stream_out, bool *done) {
  *done = true;
  if (!ctx || !tape_dev || !docs_dev || (rows && (!root_value_dev || !root_tag_dev))) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(tape_dev) & 7u) || (reinterpret_cast<uintptr_t>(root_value_dev) & 7u) || (reinterpret_cast<uintptr_t>(docs_dev) & 15u)) { return SJGPU_E_BADARG; }
  if (tape_words > 0xFFFFFFFFull || string_bytes > 0xFFFFFFFFull || docs >= 0xFFFFFFF0u || uint64_t(rows) + 1 > 0xFFFFFFF0ull) { return SJGPU_E_BADARG; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  *stream_out = s;
  if (rows == 0) { *done = false; return 0; } // (the caller has nothing to launch)
  if (ctx->query_in_flight) { // the block is the context's: the walk of the previous call must have read it
    SJ_TRY(ctx, hipEventSynchronize(ctx->ev_query));
    ctx->query_in_flight = false;
  }
  if (!ctx->ev_query) { SJ_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_query, hipEventDisableTiming)); }
  int rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_query), &ctx->d_query_bytes, 256 + size_t(rows) * sizeof(uint32_t));
  if (rc) { return rc; }
  if (workspace) {
    rc = ensure_tmp(ctx, workspace);
    if (rc) { return rc; }
  }
  SJ_TRY(ctx, hipMemsetAsync(ctx->d_query, 0, 256, s));
  launch_query_check_table(static_cast<const doc_span_dev *>(docs_dev), docs, tape_words, string_bytes, reinterpret_cast<uint32_t *>(ctx->d_query), s);
  SJ_TRY(ctx, hipGetLastError());
  uint32_t *const bad = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192); // (the pinned block's last slot, as in sjgpu_at_pointers_device)
  SJ_TRY(ctx, hipMemcpyAsync(bad, ctx->d_query, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (*bad) { return SJGPU_E_BADARG; }
  *done = false;
  return 0;
}
} // namespace

extern "C" {

int sjgpu_object_fields_from_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                          uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev, void *status_dev,
                                          void *key_value_dev, void *key_tag_dev, void *value_dev, void *tag_dev, uint64_t field_cap, void *stream, uint64_t *fields_out) {
  if (fields_out) { *fields_out = 0; }
  if (!string_buf_dev || !offsets_dev || !fields_out || (rows && !status_dev) || (field_cap && (!key_value_dev || !key_tag_dev || !value_dev || !tag_dev))) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(offsets_dev) & 3u) || (reinterpret_cast<uintptr_t>(key_value_dev) & 7u) || (reinterpret_cast<uintptr_t>(value_dev) & 7u)) { return SJGPU_E_BADARG; }
  hipStream_t s = nullptr;
  bool done = true;
  const int rc = fields_begin(ctx, tape_dev, tape_words, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows, rows ? paths_workspace_bytes(1, rows) : 0, stream, &s,
                              &done);
  if (done) { return rc; }
  if (rows == 0) {
    SJ_TRY(ctx, hipMemsetAsync(offsets_dev, 0, sizeof(uint32_t), s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    return 0;
  }
  uint32_t *offsets = static_cast<uint32_t *>(offsets_dev);
  const doc_span_dev *table = static_cast<const doc_span_dev *>(docs_dev);
  const uint64_t *tape = static_cast<const uint64_t *>(tape_dev);
  const uint64_t *root_value = static_cast<const uint64_t *>(root_value_dev);
  uint32_t *where = reinterpret_cast<uint32_t *>(ctx->d_query + 256);
  const void *total_dev = launch_object_fields_count(tape, table, docs, root_value, static_cast<const uint8_t *>(root_tag_dev), rows, where, offsets,
                                                     static_cast<uint8_t *>(status_dev), ctx->d_tmp, s);
  SJ_TRY(ctx, hipGetLastError());
  uint64_t *const total = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  SJ_TRY(ctx, hipMemcpyAsync(total, total_dev, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t fields = *total;
  *fields_out = fields;
  if (fields > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (fields > field_cap) { return SJGPU_E_OVERFLOW; }
  if (fields) {
    launch_object_fields_fill(tape, static_cast<const uint8_t *>(string_buf_dev), table, root_value, rows, where, offsets, static_cast<uint64_t *>(key_value_dev),
                              static_cast<uint8_t *>(key_tag_dev), static_cast<uint64_t *>(value_dev), static_cast<uint8_t *>(tag_dev), s);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s)); // (the verdicts and the workspace are free again when the call returns)
  }
  return 0;
}

// only enqueued behind the table check: the event that guards the context's block guards the verdicts
int sjgpu_cell_sizes_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *docs_dev, uint32_t docs, const void *root_value_dev, const void *root_tag_dev,
                            uint32_t rows, void *size_dev, void *code_dev, void *stream) {
  if ((rows && (!size_dev || !code_dev)) || (reinterpret_cast<uintptr_t>(size_dev) & 3u)) { return SJGPU_E_BADARG; }
  hipStream_t s = nullptr;
  bool done = true;
  // (no string is read: the table's string_begin words, 32 bits each, have no end to stay below)
  const int rc = fields_begin(ctx, tape_dev, tape_words, 0xFFFFFFFFull, docs_dev, docs, root_value_dev, root_tag_dev, rows, 0, stream, &s, &done);
  if (done || rows == 0) { return rc; }
  launch_cell_sizes(static_cast<const uint64_t *>(tape_dev), static_cast<const doc_span_dev *>(docs_dev), docs, static_cast<const uint64_t *>(root_value_dev),
                    static_cast<const uint8_t *>(root_tag_dev), rows, reinterpret_cast<uint32_t *>(ctx->d_query + 256), static_cast<uint32_t *>(size_dev),
                    static_cast<uint8_t *>(code_dev), s);
  SJ_TRY(ctx, hipGetLastError());
  SJ_TRY(ctx, hipEventRecord(ctx->ev_query, s));
  ctx->query_in_flight = true;
  return 0;
}

// ---- cells as JSON text (k_json_count, k_json_fill in sjgpu_json.hip; include/sjgpu_json.h) --------------------------------------------------------------
// The fields call's prologue and shape: the verdicts in the context's block, the count's total read back, the fill only when it fits
// (pretty: sjgpu_prettify_cells_device, include/sjgpu_pretty.h -- the same call around the other instantiation of the two kernels)
static int serialize_cells(bool pretty, sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev, uint32_t docs,
                           const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev, void *status_dev, void *chars_dev, uint64_t chars_cap,
                           void *stream, uint64_t *bytes_out) {
  if (bytes_out) { *bytes_out = 0; }
  if (!string_buf_dev || !offsets_dev || !bytes_out || (rows && !status_dev) || (chars_cap && !chars_dev)) { return SJGPU_E_BADARG; }
  if (reinterpret_cast<uintptr_t>(offsets_dev) & 3u) { return SJGPU_E_BADARG; }
  hipStream_t s = nullptr;
  bool done = true;
  const int rc = fields_begin(ctx, tape_dev, tape_words, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows, rows ? json_workspace_bytes(rows) : 0, stream, &s, &done);
  if (done) { return rc; }
  if (rows == 0) {
    SJ_TRY(ctx, hipMemsetAsync(offsets_dev, 0, sizeof(uint32_t), s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    return 0;
  }
  uint32_t *offsets = static_cast<uint32_t *>(offsets_dev);
  const doc_span_dev *table = static_cast<const doc_span_dev *>(docs_dev);
  const uint64_t *tape = static_cast<const uint64_t *>(tape_dev);
  const uint8_t *sbuf = static_cast<const uint8_t *>(string_buf_dev);
  const uint64_t *root_value = static_cast<const uint64_t *>(root_value_dev);
  const uint8_t *root_tag = static_cast<const uint8_t *>(root_tag_dev);
  uint32_t *where = reinterpret_cast<uint32_t *>(ctx->d_query + 256);
  const count_total_dev *total_dev = (pretty ? launch_pretty_count : launch_json_count)(tape, sbuf, string_bytes, table, docs, root_value, root_tag, rows, where, offsets,
                                                                                        static_cast<uint8_t *>(status_dev), ctx->d_tmp, s);
  SJ_TRY(ctx, hipGetLastError());
  uint64_t *const total = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  SJ_TRY(ctx, hipMemcpyAsync(total, &total_dev->total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t bytes = *total;
  *bytes_out = bytes;
  if (bytes > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (bytes > chars_cap) { return SJGPU_E_OVERFLOW; }
  if (bytes) {
    (pretty ? launch_pretty_fill : launch_json_fill)(tape, sbuf, string_bytes, table, root_value, root_tag, rows, where, offsets, static_cast<uint8_t *>(chars_dev), ctx->d_tmp, s);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s)); // (the verdicts and the workspace are free again when the call returns)
  }
  return 0;
}

int sjgpu_serialize_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev, uint32_t docs,
                                 const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev, void *status_dev, void *chars_dev, uint64_t chars_cap,
                                 void *stream, uint64_t *bytes_out) {
  return serialize_cells(false, ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows, offsets_dev, status_dev, chars_dev, chars_cap,
                         stream, bytes_out);
}
int sjgpu_prettify_cells_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev, uint32_t docs,
                                const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev, void *status_dev, void *chars_dev, uint64_t chars_cap,
                                void *stream, uint64_t *bytes_out) {
  return serialize_cells(true, ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows, offsets_dev, status_dev, chars_dev, chars_cap,
                         stream, bytes_out);
}

// ---- cells as JSON text, breadth first (sjgpu_json_wide.hip; include/sjgpu_json_wide.h) ------------------------------------------------------------------------
// The narrow call's refusals, prologue and decisions, word for word.  Two waits in front of the fill: the size of the range space sizes the workspace (and is what
// SJGPU_E_RANGE refuses), the total decides the fill.  The roots' block lies behind the context's query block, the slots' in d_tmp
// (pretty: sjgpu_prettify_cells_wide_device, include/sjgpu_pretty.h)
static int serialize_cells_wide(bool pretty, sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev, void *status_dev, void *chars_dev,
                                uint64_t chars_cap, void *stream, uint64_t *bytes_out) {
  if (bytes_out) { *bytes_out = 0; }
  if (!string_buf_dev || !offsets_dev || !bytes_out || (rows && !status_dev) || (chars_cap && !chars_dev)) { return SJGPU_E_BADARG; }
  if (reinterpret_cast<uintptr_t>(offsets_dev) & 3u) { return SJGPU_E_BADARG; }
  hipStream_t s = nullptr;
  bool done = true;
  int rc = fields_begin(ctx, tape_dev, tape_words, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows, 0, stream, &s, &done);
  if (done) { return rc; }
  if (rows == 0) {
    SJ_TRY(ctx, hipMemsetAsync(offsets_dev, 0, sizeof(uint32_t), s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    return 0;
  }
  uint32_t *offsets = static_cast<uint32_t *>(offsets_dev);
  const doc_span_dev *table = static_cast<const doc_span_dev *>(docs_dev);
  const uint64_t *tape = static_cast<const uint64_t *>(tape_dev);
  const uint8_t *sbuf = static_cast<const uint8_t *>(string_buf_dev);
  const uint64_t *root_value = static_cast<const uint64_t *>(root_value_dev);
  const uint8_t *root_tag = static_cast<const uint8_t *>(root_tag_dev);
  uint8_t *status = static_cast<uint8_t *>(status_dev);
  // (the table check is over and the stream drained: the query block may move)
  rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_query), &ctx->d_query_bytes, 256 + json_wide_root_bytes(rows));
  if (rc) { return rc; }
  void *root_space = ctx->d_query + 256;
  uint64_t *const total = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  const count_total_dev *range_dev = launch_json_wide_extents(tape, table, docs, root_value, root_tag, rows, root_space, s);
  SJ_TRY(ctx, hipGetLastError());
  SJ_TRY(ctx, hipMemcpyAsync(total, &range_dev->total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t range_words = *total;
  if (range_words > 0xFFFFFFF0ull) {
    // the statuses alone, by the narrow count, its offsets into the workspace: nothing else of the caller's is written
    const size_t narrow = (json_workspace_bytes(rows) + 255) & ~size_t(255);
    rc = ensure_tmp(ctx, narrow + (size_t(rows) + 1) * sizeof(uint32_t));
    if (rc) { return rc; }
    (void)(pretty ? launch_pretty_count : launch_json_count)(tape, sbuf, string_bytes, table, docs, root_value, root_tag, rows, json_wide_where(root_space, rows),
                                                             reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ctx->d_tmp) + narrow), status, ctx->d_tmp, s);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s));
    return SJGPU_E_RANGE;
  }
  rc = ensure_tmp(ctx, json_wide_word_bytes(rows, range_words));
  if (rc) { return rc; }
  const count_total_dev *total_dev = nullptr;
  SJ_TRY(ctx, (pretty ? launch_pretty_wide_count : launch_json_wide_count)(tape, sbuf, string_bytes, table, root_value, root_tag, rows, range_words, offsets, status, root_space, ctx->d_tmp, s, &total_dev));
  SJ_TRY(ctx, hipGetLastError());
  SJ_TRY(ctx, hipMemcpyAsync(total, &total_dev->total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t bytes = *total;
  *bytes_out = bytes;
  if (bytes > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (bytes > chars_cap) { return SJGPU_E_OVERFLOW; }
  if (bytes) {
    (pretty ? launch_pretty_wide_fill : launch_json_wide_fill)(tape, sbuf, string_bytes, table, root_value, root_tag, rows, range_words, static_cast<uint8_t *>(chars_dev), root_space,
                                                               ctx->d_tmp, s);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s)); // (the roots' block and the workspace are free again when the call returns)
  }
  return 0;
}

int sjgpu_serialize_cells_wide_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                      uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev, void *status_dev, void *chars_dev,
                                      uint64_t chars_cap, void *stream, uint64_t *bytes_out) {
  return serialize_cells_wide(false, ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows, offsets_dev, status_dev, chars_dev,
                              chars_cap, stream, bytes_out);
}
int sjgpu_prettify_cells_wide_device(sjgpu_ctx *ctx, const void *tape_dev, uint64_t tape_words, const void *string_buf_dev, uint64_t string_bytes, const void *docs_dev,
                                     uint32_t docs, const void *root_value_dev, const void *root_tag_dev, uint32_t rows, void *offsets_dev, void *status_dev, void *chars_dev,
                                     uint64_t chars_cap, void *stream, uint64_t *bytes_out) {
  return serialize_cells_wide(true, ctx, tape_dev, tape_words, string_buf_dev, string_bytes, docs_dev, docs, root_value_dev, root_tag_dev, rows, offsets_dev, status_dev, chars_dev,
                              chars_cap, stream, bytes_out);
}

// ---- typed columns as JSON records (k_write_count, k_write_fill in sjgpu_write.hip; include/sjgpu_write.h) -------------------------------------------------
// The serializer's shape: the count's total read back, the fill only when it fits.  The column table and the escaped keys (sj_write_table.h) go up through the
// context's block as the compiled pointers of sjgpu_at_pointers_device do -- behind the same wait for the block's previous user --; the call ends with the stream
// drained on every road, so the block is free again when it returns and no event is recorded
// (shared with sjgpu_write_nested_device: `nested` says whose table this is -- write_field_dev and six counts, or write_column_dev and four)
static int write_through_block(sjgpu_ctx *ctx, const write_table &table, bool nested, uint32_t K, uint32_t n, uint32_t flags, void *offsets_dev, void *status_dev,
                               void *chars_dev, uint64_t chars_cap, void *counts_dev, void *stream, uint64_t *bytes_out) {
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = pick(ctx, stream);
  if (n == 0) {
    SJ_TRY(ctx, hipMemsetAsync(offsets_dev, 0, sizeof(uint32_t), s));
    SJ_TRY(ctx, hipMemsetAsync(counts_dev, 0, (nested ? 6 : 4) * sizeof(uint64_t), s));
    SJ_TRY(ctx, hipStreamSynchronize(s));
    return 0;
  }
  if (ctx->query_in_flight) { // the block is the context's: the walk of the previous call must have read it
    SJ_TRY(ctx, hipEventSynchronize(ctx->ev_query));
    ctx->query_in_flight = false;
  }
  const size_t block = 256 + table.bytes.size(); // (the block's first 256 bytes are the table check's in the query calls: left alone here)
  int rc = grow(ctx, reinterpret_cast<void **>(&ctx->d_query), &ctx->d_query_bytes, block);
  if (rc) { return rc; }
  rc = ensure_tmp(ctx, write_workspace_bytes(n));
  if (rc) { return rc; }
  if (ctx->h_query_bytes < block) {
    if (ctx->h_query) { (void)hipHostFree(ctx->h_query); ctx->h_query = nullptr; ctx->h_query_bytes = 0; }
    SJ_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_query), block, hipHostMallocDefault));
    ctx->h_query_bytes = block;
  }
  if (!table.bytes.empty()) {
    std::memcpy(ctx->h_query + 256, table.bytes.data(), table.bytes.size());
    SJ_TRY(ctx, hipMemcpyAsync(ctx->d_query + 256, ctx->h_query + 256, table.bytes.size(), hipMemcpyHostToDevice, s));
  }
  const write_column_dev *cols = reinterpret_cast<const write_column_dev *>(ctx->d_query + 256);
  const write_field_dev *fields = reinterpret_cast<const write_field_dev *>(ctx->d_query + 256);
  const uint8_t *keys = ctx->d_query + 256 + table.keys_at;
  uint32_t *offsets = static_cast<uint32_t *>(offsets_dev);
  const count_total_dev *total_dev =
      nested ? launch_nested_count(fields, keys, K, n, flags, offsets, static_cast<uint8_t *>(status_dev), static_cast<uint64_t *>(counts_dev), ctx->d_tmp, s)
             : launch_write_count(cols, keys, K, n, flags, offsets, static_cast<uint8_t *>(status_dev), static_cast<uint64_t *>(counts_dev), ctx->d_tmp, s);
  SJ_TRY(ctx, hipGetLastError());
  uint64_t *const total = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192);
  SJ_TRY(ctx, hipMemcpyAsync(total, &total_dev->total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  const uint64_t bytes = *total;
  *bytes_out = bytes;
  if (bytes > 0xFFFFFFFFull) { return E_CAPACITY; } // the offsets are 32 bits
  if (bytes > chars_cap) { return SJGPU_E_OVERFLOW; }
  if (bytes) {
    if (nested) {
      launch_nested_fill(fields, keys, K, n, flags, offsets, static_cast<uint8_t *>(chars_dev), s);
    } else {
      launch_write_fill(cols, keys, K, n, flags, offsets, static_cast<uint8_t *>(chars_dev), s);
    }
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s)); // (the block and the workspace are free again when the call returns)
  }
  return 0;
}

int sjgpu_write_records_device(sjgpu_ctx *ctx, const sjgpu_write_column *columns, uint32_t K, uint32_t n, uint32_t flags, void *offsets_dev, void *status_dev, void *chars_dev,
                               uint64_t chars_cap, void *counts_dev, void *stream, uint64_t *bytes_out) {
  if (bytes_out) { *bytes_out = 0; }
  if (!ctx || !offsets_dev || !counts_dev || !bytes_out || (n && !status_dev) || (chars_cap && !chars_dev)) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(offsets_dev) & 3u) || (reinterpret_cast<uintptr_t>(counts_dev) & 7u)) { return SJGPU_E_BADARG; }
  write_table table;
  if (!make_write_table(columns, K, n, flags, &table)) { return SJGPU_E_BADARG; }
  return write_through_block(ctx, table, false, K, n, flags, offsets_dev, status_dev, chars_dev, chars_cap, counts_dev, stream, bytes_out);
}

// ---- list columns and array rows as nested JSON (k_nested_count, k_nested_fill in sjgpu_write.hip; include/sjgpu_nested.h) -------------------------------------
// The plain writer's call over the field table of sj_nested_table.h: the same block, the same waits, the same workspace
int sjgpu_write_nested_device(sjgpu_ctx *ctx, const sjgpu_write_field *fields, uint32_t K, uint32_t n, uint32_t flags, void *offsets_dev, void *status_dev, void *chars_dev,
                              uint64_t chars_cap, void *counts_dev, void *stream, uint64_t *bytes_out) {
  if (bytes_out) { *bytes_out = 0; }
  if (!ctx || !offsets_dev || !counts_dev || !bytes_out || (n && !status_dev) || (chars_cap && !chars_dev)) { return SJGPU_E_BADARG; }
  if ((reinterpret_cast<uintptr_t>(offsets_dev) & 3u) || (reinterpret_cast<uintptr_t>(counts_dev) & 7u)) { return SJGPU_E_BADARG; }
  write_table table;
  if (!make_nested_table(fields, K, n, flags, &table)) { return SJGPU_E_BADARG; }
  return write_through_block(ctx, table, true, K, n, flags, offsets_dev, status_dev, chars_dev, chars_cap, counts_dev, stream, bytes_out);
}

// ---- typed getters over cells (k_cell_kinds, k_cast_cells in sjgpu_cast.hip; include/sjgpu_cast.h) ------------------------------------------------------
// Elementwise over the cells alone: no block of the context, no upload, no event, no wait -- a memset of the counters and one launch, only enqueued
int sjgpu_cell_kinds_device(sjgpu_ctx *ctx, const void *value_dev, const void *tag_dev, uint32_t n, uint32_t K, void *kinds_dev, void *stream) {
  if (!ctx || !cell_kinds_args_ok(value_dev, tag_dev, n, K, kinds_dev)) { return SJGPU_E_BADARG; }
  if (K == 0) { return 0; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  SJ_TRY(ctx, launch_cell_kinds(static_cast<const uint64_t *>(value_dev), static_cast<const uint8_t *>(tag_dev), n, K, static_cast<uint32_t *>(kinds_dev), pick(ctx, stream)));
  SJ_TRY(ctx, hipGetLastError());
  return 0;
}

int sjgpu_cast_cells_device(sjgpu_ctx *ctx, const void *value_dev, const void *tag_dev, uint32_t n, uint32_t K, const uint8_t *getters, void *value_out_dev,
                            void *code_out_dev, void *valid_out_dev, void *counts_out_dev, void *stream) {
  if (!ctx || !cast_cells_args_ok(value_dev, tag_dev, n, K, getters, value_out_dev, code_out_dev, valid_out_dev, counts_out_dev)) { return SJGPU_E_BADARG; }
  if (K == 0) { return 0; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  SJ_TRY(ctx, launch_cast_cells(static_cast<const uint64_t *>(value_dev), static_cast<const uint8_t *>(tag_dev), n, K, getters, static_cast<uint64_t *>(value_out_dev),
                                static_cast<uint8_t *>(code_out_dev), static_cast<uint64_t *>(valid_out_dev), static_cast<uint32_t *>(counts_out_dev), pick(ctx, stream)));
  SJ_TRY(ctx, hipGetLastError());
  return 0;
}

// ---- numbers held in strings (k_cast_string_cells, k_cast_strings_exact in sjgpu_cast_strings.hip; include/sjgpu_cast_strings.h) ---------------------------
// Over the cells and the string buffer alone, as the cast above: a memset of the counters and two launches, only enqueued
int sjgpu_cast_string_cells_device(sjgpu_ctx *ctx, const void *string_buf_dev, uint64_t string_bytes, const void *value_dev, const void *tag_dev, uint32_t n, uint32_t K,
                                   const uint8_t *getters, void *value_out_dev, void *code_out_dev, void *valid_out_dev, void *counts_out_dev, void *stream) {
  if (!ctx || !cast_string_cells_args_ok(string_buf_dev, string_bytes, value_dev, tag_dev, n, K, getters, value_out_dev, code_out_dev, valid_out_dev, counts_out_dev)) {
    return SJGPU_E_BADARG;
  }
  if (K == 0) { return 0; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  SJ_TRY(ctx, launch_cast_string_cells(static_cast<const uint8_t *>(string_buf_dev), string_bytes, static_cast<const uint64_t *>(value_dev), static_cast<const uint8_t *>(tag_dev), n,
                                       K, getters, static_cast<uint64_t *>(value_out_dev), static_cast<uint8_t *>(code_out_dev), static_cast<uint64_t *>(valid_out_dev),
                                       static_cast<uint32_t *>(counts_out_dev), pick(ctx, stream)));
  SJ_TRY(ctx, hipGetLastError());
  return 0;
}

// ---- a dictionary of a row of string cells, the census per code (sjgpu_dict.hip; include/sjgpu_dict.h) -----------------------------------------------------
// The encode reads the cells and the string buffer alone: no block of the context and no event, its table lies in d_tmp.  The codes are enqueued in front of the
// read-back: they are complete whatever the capacity says
int sjgpu_dictionary_encode_device(sjgpu_ctx *ctx, const void *string_buf_dev, uint64_t string_bytes, const void *value_row_dev, const void *tag_row_dev, uint32_t n,
                                   void *codes_dev, void *dict_value_dev, void *dict_tag_dev, void *dict_first_dev, void *dict_count_dev, uint64_t dict_cap, void *stream,
                                   uint64_t *distinct_out) {
  if (distinct_out) { *distinct_out = 0; }
  if (!ctx || !distinct_out ||
      !dict_encode_args_ok(string_buf_dev, string_bytes, value_row_dev, tag_row_dev, n, codes_dev, dict_value_dev, dict_tag_dev, dict_first_dev, dict_count_dev, dict_cap)) {
    return SJGPU_E_BADARG;
  }
  if (n == 0) { return 0; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure_tmp(ctx, dict_workspace_bytes(n));
  if (rc) { return rc; }
  hipStream_t s = pick(ctx, stream);
  const uint64_t *value = static_cast<const uint64_t *>(value_row_dev);
  const dict_result_dev *result_dev = nullptr;
  SJ_TRY(ctx, launch_dict_encode(value, static_cast<const uint8_t *>(tag_row_dev), n, static_cast<const uint8_t *>(string_buf_dev), string_bytes,
                                 static_cast<int32_t *>(codes_dev), ctx->d_tmp, s, &result_dev));
  SJ_TRY(ctx, hipGetLastError());
  dict_result_dev *const result = reinterpret_cast<dict_result_dev *>(reinterpret_cast<uint8_t *>(ctx->h_result) + 192); // (the pinned block's last slot, as in the gather)
  SJ_TRY(ctx, hipMemcpyAsync(result, result_dev, sizeof(dict_result_dev), hipMemcpyDeviceToHost, s));
  SJ_TRY(ctx, hipStreamSynchronize(s));
  if (result->failed) { return SJGPU_E_INTERNAL; }
  const uint64_t distinct = result->distinct;
  *distinct_out = distinct;
  if (distinct > dict_cap) { return SJGPU_E_OVERFLOW; }
  if (distinct) {
    launch_dict_fill(value, n, ctx->d_tmp, static_cast<uint64_t *>(dict_value_dev), static_cast<uint8_t *>(dict_tag_dev), static_cast<uint32_t *>(dict_first_dev),
                     static_cast<uint32_t *>(dict_count_dev), s);
    SJ_TRY(ctx, hipGetLastError());
    SJ_TRY(ctx, hipStreamSynchronize(s)); // (the workspace is free again when the call returns)
  }
  return 0;
}

// elementwise over the cells and their codes, as sjgpu_cell_kinds_device: a memset of the counters and one launch, only enqueued
int sjgpu_cell_kinds_by_code_device(sjgpu_ctx *ctx, const void *codes_dev, const void *value_dev, const void *tag_dev, uint32_t n, uint32_t groups, void *kinds_dev,
                                    void *stream) {
  if (!ctx || !cell_kinds_by_code_args_ok(codes_dev, value_dev, tag_dev, n, groups, kinds_dev)) { return SJGPU_E_BADARG; }
  if (groups == 0) { return 0; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  SJ_TRY(ctx, launch_cell_kinds_by_code(static_cast<const int32_t *>(codes_dev), static_cast<const uint64_t *>(value_dev), static_cast<const uint8_t *>(tag_dev), n, groups,
                                        static_cast<uint32_t *>(kinds_dev), pick(ctx, stream)));
  SJ_TRY(ctx, hipGetLastError());
  return 0;
}

// ---- a map column pivoted into a record table (sjgpu_pivot.hip; include/sjgpu_pivot.h) --------------------------------------------------------------------------
// Over the fields' rows, their codes and the map alone: two launches, only enqueued -- no block of the context, no workspace, no event
int sjgpu_pivot_fields_device(sjgpu_ctx *ctx, const void *offsets_dev, const void *status_dev, uint32_t rows, const void *codes_dev, const void *value_dev, const void *tag_dev,
                              uint64_t fields, const void *column_of_code_dev, uint32_t groups, uint32_t columns, void *value_out_dev, void *tag_out_dev, void *stream) {
  if (!ctx || !pivot_args_ok(offsets_dev, status_dev, rows, codes_dev, value_dev, tag_dev, fields, column_of_code_dev, groups, columns, value_out_dev, tag_out_dev)) {
    return SJGPU_E_BADARG;
  }
  if (rows == 0 || columns == 0) { return 0; }
  SJ_TRY(ctx, hipSetDevice(ctx->device));
  launch_pivot_fields(static_cast<const uint32_t *>(offsets_dev), static_cast<const uint8_t *>(status_dev), rows, static_cast<const int32_t *>(codes_dev),
                      static_cast<const uint64_t *>(value_dev), static_cast<const uint8_t *>(tag_dev), uint32_t(fields), static_cast<const int32_t *>(column_of_code_dev), groups,
                      columns, static_cast<uint64_t *>(value_out_dev), static_cast<uint8_t *>(tag_out_dev), pick(ctx, stream));
  SJ_TRY(ctx, hipGetLastError());
  return 0;
}

} // extern "C"
