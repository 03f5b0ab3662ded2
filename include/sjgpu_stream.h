/* include/sjgpu_stream.h -- C-ABI of libsjgpu.so, document streams: stage 2 of a resident NDJSON buffer, one DOM tape per document.
 * An extension of include/sjgpu.h (contexts, error codes, stage 1 and the single document's stage 2 are declared there); a header of
 * its own so that programs built against sjgpu.h alone -- the simdjson plug-in shim and the test programs that link it -- are
 * not rebuilt for it. */
#ifndef SJGPU_STREAM_H
#define SJGPU_STREAM_H

#include "sjgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- stage 2 of a resident document STREAM: one DOM tape per document ---------------------------------------------------------
 * What dom_parser_implementation::stage2_next (include/simdjson/internal/dom_parser_implementation.h:107) leaves document by
 * document when document_stream::next_document drives it -- walk_document<STREAMING = true>, json_iterator.h:120-244 -- for
 * ALL documents of the list, from one call (sjgpu_tape_many.hip).
 * idx_dev[0..n] = the list of buf_dev[0..len) with its first sentinel as sjgpu_stage1_device (regular mode) or
 * sjgpu_stage1_finish_device (a streaming mode) left it: the tokens of document 0, then of document 1, ...  A document starts
 * at every token that has nesting depth 0 in front of it and ends where the depth returns to 0 (a root scalar is one token):
 * `1 2 3` is three documents, `[] {}` two.
 * On return, for the *docs_out documents delivered:
 *   tape_dev        the tapes back to back; the slice of document d is word for word what the reference's dom::parser::parse of
 *                   that document's bytes alone leaves in doc.tape: root word 'r' | words first, 'r' | 0 last, container
 *                   payloads relative to the slice's first word;
 *   string_buf_dev  the string records back to back; the slice of document d is the reference's doc.string_buf of that
 *                   document, and the string payloads of its tape are relative to the slice;
 *   docs_dev        *docs_out + 1 entries of sjgpu_doc_span, byte_begin = idx[first_token].  The last entry holds the first token
 *                   NOT delivered (n on success), its byte offset (len on success), the total tape words and string bytes.
 * Errors follow document_stream: the call returns the code the streaming walk meets FIRST (the codes of sjgpu_stage2_device),
 * *docs_out = the complete documents in front of the broken one, and those are delivered in full; nothing is promised about
 * what lies behind.  n == 0 is EMPTY with *docs_out = 0.  A broken stream costs two runs: the list is run again up to the
 * broken document.
 * Sizes that always suffice: tape 4 n words (a token writes at most two, a document adds two root words and has at least one
 * token; the tight figure is len + 3 docs, how the reference sizes each document); table n + 1 entries; string_buf_dev as for
 * sjgpu_stage2_device.  Tape positions are 31 bits: a stream whose words do not fit is CAPACITY.  A tape, string buffer or table
 * that is too small is SJGPU_E_OVERFLOW and nothing is written beyond the capacity given; when it is the table, *docs_out says
 * how many entries were needed.  buf_dev and docs_dev 16-byte aligned, tape_dev 8-byte, idx_dev 4-byte (SJGPU_E_BADARG
 * otherwise); max_depth and the CAPACITY limits as for sjgpu_stage2_device.  Waits for the stream. */
typedef struct sjgpu_doc_span {
  uint32_t first_token;  /* list index of the document's first token */
  uint32_t byte_begin;   /* idx[first_token] */
  uint32_t tape_begin;   /* first word of the document's tape */
  uint32_t string_begin; /* first byte of the document's string records */
} sjgpu_doc_span;
int sjgpu_stage2_many_device(sjgpu_ctx *ctx, const void *buf_dev, size_t len, const void *idx_dev, uint32_t n, uint32_t max_depth, void *tape_dev,
                             size_t tape_cap_words, void *string_buf_dev, size_t string_buf_bytes, void *docs_dev, size_t doc_cap /* entries; docs + 1 needed */,
                             void *stream, uint32_t *docs_out, uint64_t *tape_words_out, uint64_t *string_bytes_out);
/* sjgpu_parse for a HOST buffer that holds a stream: upload, regular stage 1 (its errors concern the whole buffer and come
 * first), sjgpu_stage2_many_device, three downloads (tapes, string records, table).  The caller's arrays are sized like the
 * device call's; too small a one is SJGPU_E_OVERFLOW. */
int sjgpu_parse_many(sjgpu_ctx *ctx, const uint8_t *buf, size_t len, uint32_t max_depth, uint64_t *tape_out, size_t tape_cap_words,
                     uint8_t *string_buf_out, size_t string_buf_bytes, sjgpu_doc_span *docs_out_host, size_t doc_cap, uint32_t *docs_out,
                     uint64_t *tape_words_out, uint64_t *string_bytes_out);

#ifdef __cplusplus
}
#endif
#endif
