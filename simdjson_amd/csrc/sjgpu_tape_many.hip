// simdjson_amd/csrc/sjgpu_tape_many.hip -- stage 2 of a document STREAM on the device: one DOM tape per document (sjgpu_stage2_many_device).
//
// The reference walks a stream one document at a time: dom_parser_implementation::stage2_next = walk_document<STREAMING = true>
// (/root/reference/src/generic/stage2/json_iterator.h:120-244), driven by document_stream::next_document.  The streaming walk differs from the regular one
// in two places (:139-144, :237-240): the outer bracket is not compared with the list's last token, and what follows the root value is the next document.
// Here the whole list goes through the token kernels of sjgpu_tape.hip ONCE, in their STREAM instantiation (a token with depth 0 in front of it is a root),
// which leaves
//   * a FLAT tape in workspace: the words of all tokens in list order, bracket payloads as positions of the whole list, no root words;
//   * one flag per token: "begins a document", and for those tokens where their document's string records begin;
// and three small passes, each behind a launch boundary, turn that into what the reference would have left document by document:
//   k_many_locate    (behind a scan of the flags -> document ordinals) the number of documents, and for a list with an error the cut in front of the
//                    document that holds the first offending token;
//   k_many_table     the document table: first token, byte offset, tape position and string offset of every document, and the totals;
//   k_many_relocate  every token's one or two words from the flat tape to [flat position + 2 * ordinal + 1] -- each document gains its two root words --
//                    with the payloads rebased to the document: string payloads minus the document's first record, bracket payloads minus its flat base.
// Errors: document_stream stops at the first broken document and delivers what lies in front of it.  Sorting the brackets by level lets a stray closing
// bracket behind a broken document pair with an opening bracket of an EARLIER, valid document, so a run that reported an error is not relocated: the
// caller (sjgpu_capi_stage2.hip) runs the list again up to the cut, a prefix that is valid by construction -- the optimistic-then-again shape
// sjgpu_stage2_device has for its string roads and for the sort's second pass.  No kernel here waits for another workgroup.
#include "sjgpu_device.h"
#include "sj_tape_rules.h"

namespace sjgpu {
namespace {

constexpr u32 MANY_THREADS = 256, MANY_PER = 4;

// one thread: the documents of the list, and the cut in front of the first broken one
__global__ void k_many_locate(const int *__restrict__ ord, const u32 *__restrict__ idx, u32 n, const tape_result_dev *__restrict__ res,
                              const strings_result_dev *__restrict__ sres, many_result_dev *__restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) { return; }
  u64 key = res->error_key;
  if (sres->first_bad != 0xFFFFFFFFu) {
    const u64 sk = error_key(sres->first_bad, 2, SJ_STRING_ERROR); // a string's content ranks behind its own position in the grammar
    key = sk < key ? sk : key;
  }
  many_result_dev r;
  r.docs = u32(ord[n]); // the scan was exclusive over n + 1 entries: the flags of tokens 0 .. n - 1
  r.cut_token = n;
  r.cut_byte = idx[n];
  r.has_error = key != NO_ERROR_KEY ? 1u : 0u;
  if (r.has_error) {
    // Everything in front of the first error is what the serial walk saw: the flags there are sound, whatever lies behind.  The offending index e (the
    // sentinel: e == n, "the list ends inside a container") belongs to the document whose flag is the last at or in front of e.
    const u64 e64 = key >> 8;
    const u32 e = e64 < n ? u32(e64) : n;
    const int upto = e < n ? ord[e + 1] : ord[n]; // flags of tokens 0 .. e (token 0 always carries one: >= 1)
    u32 lo = 0, hi = e < n ? e : n - 1u; // the smallest i with ord[i + 1] >= upto: the token that carries that flag
    while (lo < hi) {
      const u32 mid = lo + (hi - lo) / 2u;
      if (ord[mid + 1] >= upto) { hi = mid; } else { lo = mid + 1u; }
    }
    r.cut_token = lo;
    r.cut_byte = idx[lo];
    r.docs = upto > 0 ? u32(upto) - 1u : 0u; // the complete documents in front of the broken one
  }
  *out = r;
}

// the document table: entry d from the token that begins document d, entry `docs` (the totals) from the sentinel
__global__ __launch_bounds__(MANY_THREADS) void k_many_table(const int *__restrict__ ord, const u32 *__restrict__ idx, const int *__restrict__ tpos,
                                                            const u32 *__restrict__ doc_str, const strings_result_dev *__restrict__ sres, u32 n, u32 docs,
                                                            doc_span_dev *__restrict__ table) {
  const u64 i64 = u64(blockIdx.x) * MANY_THREADS + threadIdx.x;
  if (i64 > n) { return; }
  const u32 i = u32(i64);
  const u32 d = u32(ord[i]);
  if (d > docs) { return; } // (the host sized the table for docs + 1 entries from this very scan)
  doc_span_dev e;
  e.first_token = i;
  e.byte_begin = idx[i];
  e.tape_begin = u32(tpos[i]) + 2u * d;
  if (i == n) {
    if (d != docs) { return; }
    e.string_begin = u32(sres->bytes);
  } else {
    if (ord[i + 1] == ord[i] || d == docs) { return; } // no flag
    e.string_begin = doc_str[i];
  }
  table[d] = e;
}

// four consecutive tokens per thread, like k_tok_apply.  total: the words of all tapes (nothing is written at or beyond it).
__global__ __launch_bounds__(MANY_THREADS) void k_many_relocate(const u8 *__restrict__ tokc, const int *__restrict__ tpos, const int *__restrict__ ord,
                                                               const u64 *__restrict__ flat, const doc_span_dev *__restrict__ table, u32 n, u32 docs, u64 total,
                                                               u64 *__restrict__ tape) {
  const u64 i0_64 = (u64(blockIdx.x) * MANY_THREADS + threadIdx.x) * MANY_PER;
  if (i0_64 >= n) { return; }
  const u32 i0 = u32(i0_64);
  typedef u32 __attribute__((aligned(1))) u32_unaligned;
  const u32 four = *reinterpret_cast<const u32_unaligned *>(tokc + 2 + i0_64); // (tokc[i + 2] = token i; the array has room for n + 9 bytes)
  int tp[MANY_PER + 1], od[MANY_PER + 1];
  if (i0 + MANY_PER <= n) { // entries i0 .. i0 + 4 exist (both arrays have n + 1)
    const int4 t4 = *reinterpret_cast<const int4 *>(tpos + i0), o4 = *reinterpret_cast<const int4 *>(ord + i0);
    tp[0] = t4.x; tp[1] = t4.y; tp[2] = t4.z; tp[3] = t4.w; tp[4] = tpos[i0 + 4];
    od[0] = o4.x; od[1] = o4.y; od[2] = o4.z; od[3] = o4.w; od[4] = ord[i0 + 4];
  } else {
#pragma unroll
    for (u32 q = 0; q <= MANY_PER; q++) {
      const u32 at = i0 + q <= n ? i0 + q : n;
      tp[q] = tpos[at];
      od[q] = ord[at];
    }
  }
  // the table entries of the (at most four, nearly always one) documents of these tokens: requested at once
  uint4 span[MANY_PER];
#pragma unroll
  for (u32 j = 0; j < MANY_PER; j++) {
    const u32 d = u32(od[j + 1]) - 1u; // the flags of tokens 0 .. i, minus one: token i's document
    span[j] = d < docs ? *reinterpret_cast<const uint4 *>(table + d) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (u32 j = 0; j < MANY_PER; j++) {
    const u32 i = i0 + j;
    if (i >= n) { break; }
    const u32 d = u32(od[j + 1]) - 1u;
    if (d >= docs) { continue; } // (cannot happen in a run without an error)
    const u32 c = (four >> (8u * j)) & 0xFFu;
    const u32 words = u32(tp[j + 1] - tp[j]);
    const u32 out_base = span[j].z;                 // where document d's tape begins
    const u32 flat_base = out_base - 2u * d;        // ... and where its tokens' words begin in the flat tape
    const u64 at = u64(u32(tp[j])) + 2u * u64(d) + 1u;
    if (words != 0u && at + words <= total) {
      u64 w = flat[u64(u32(tp[j])) + 1u];
      // strings: the record's offset inside the document's own string buffer (tape_builder.h:184 starts every document at the buffer's first byte);
      // brackets: both payloads -- the partner's position (+ 1 for an opening bracket) in the low half, the count above it untouched -- leave the list's
      // coordinates for the document's.  Neither subtraction borrows: the payload is not smaller than the base.
      if (c == '"') { w -= span[j].w; }
      else if (is_open_char(c) || is_close_char(c)) { w -= flat_base; }
      tape[at] = w;
      if (words == 2u) { tape[at + 1u] = flat[u64(u32(tp[j])) + 2u]; } // a number's value word
    }
    if (od[j + 1] != od[j]) { // the token begins document d: both root words (visit_document_end, tape_builder.h:160-165)
      const u32 next = table[d + 1u].tape_begin; // (entry `docs` holds the totals)
      if (next > out_base && next <= total) {
        tape[out_base] = tape_word('r', u64(next - out_base));
        tape[next - 1u] = tape_word('r', 0);
      }
    }
  }
}

static inline u32 blocks_of(u64 n, u32 per) { return u32((n + per - 1) / per); }

} // namespace

many_workspace carve_many_workspace(void *base_, uint32_t n) {
  uint8_t *base = static_cast<uint8_t *>(base_);
  many_workspace m{};
  size_t at = 0;
  auto take = [&](size_t bytes) { uint8_t *p = base ? base + at : nullptr; at += (bytes + 255) & ~size_t(255); return p; };
  const size_t n1 = size_t(n) + 1;
  m.flat_cap = 2 * n1 + 2; // a token writes at most two words; position k of the list lives at [k + 1]
  m.flat_tape = reinterpret_cast<uint64_t *>(take(m.flat_cap * 8));
  m.doc_ord = reinterpret_cast<int *>(take(n1 * 4 + 64));
  m.doc_str = reinterpret_cast<uint32_t *>(take(n1 * 4 + 64));
  m.partial = reinterpret_cast<int *>(take((n1 / 4096 + 80) * 4));
  m.bytes = at;
  return m;
}
size_t many_workspace_bytes(uint32_t n, uint64_t len) {
  (void)len;
  return carve_many_workspace(nullptr, n).bytes;
}

void launch_many_ordinals(const uint32_t *idx, uint32_t n, const many_workspace &m, const tape_stream_view &v, const strings_result_dev *sres, many_result_dev *out,
                          hipStream_t s) {
  enqueue_scan(m.doc_ord, n + 1, v.n_plus_1, m.partial, s);
  hipLaunchKernelGGL(k_many_locate, dim3(1), dim3(64), 0, s, m.doc_ord, idx, n, v.res, sres, out);
}

void launch_many_relocate(const uint32_t *idx, uint32_t n, uint32_t docs, uint64_t total_words, const many_workspace &m, const tape_stream_view &v,
                          const strings_result_dev *sres, doc_span_dev *table, uint64_t *tape, hipStream_t s) {
  hipLaunchKernelGGL(k_many_table, dim3(blocks_of(u64(n) + 1, MANY_THREADS)), dim3(MANY_THREADS), 0, s, m.doc_ord, idx, v.tpos, m.doc_str, sres, n, docs, table);
  hipLaunchKernelGGL(k_many_relocate, dim3(blocks_of(n, MANY_THREADS * MANY_PER)), dim3(MANY_THREADS), 0, s, v.tokc, v.tpos, m.doc_ord, m.flat_tape, table, n, docs,
                     total_words, tape);
}

} // namespace sjgpu
