// tests/host/test_tape_many_emu.cpp -- CPU tier: the stage-2 KERNEL SOURCES of a document stream (sjgpu_tape.hip in its STREAM instantiation,
// sjgpu_tape_many.hip, the string pass and the scans, compiled as C++ against tests/host/emu) run the launches of sjgpu_stage2_many_device on whole
// streams and are compared, document by document, with the oracle's serial walk over each document's OWN bytes (oracle/sj_oracle_stage2.c, pinned
// against the reference's dom::parser::parse): the code and the number of documents delivered always; every tape word, every byte of the string
// records and every table entry of the documents delivered.
// Input on stdin, one record per stream:
//   [u32 length][bytes][u32 max_depth][i32 want_docs][i32 want_code][u32 count][u32 begin[count]]
// want_docs >= 0: the expectation is given (a hand-written row); the delivered documents are then checked against the oracle's parse of the bytes the
// table itself delimits.  want_docs < 0: begin[] are the byte offsets of the stream's documents; the oracle parses them one after the other, the
// first one it rejects gives the code and the number of documents in front of it, and the table's byte_begin must be begin[].
#include "sjgpu.h"
#include "sjgpu_internal.h"
#include "sj_oracle.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sjgpu;

static void *aligned(std::vector<uint8_t> &store, size_t bytes, uint8_t fill) {
  store.assign(bytes + 512, fill);
  uintptr_t p = reinterpret_cast<uintptr_t>(store.data());
  p = (p + 255) & ~uintptr_t(255);
  return reinterpret_cast<void *>(p);
}

struct parsed {
  int code;
  std::vector<uint64_t> tape;
  std::vector<uint8_t> strings;
};
static parsed oracle_parse(const uint8_t *bytes, size_t len, uint32_t max_depth) {
  parsed p;
  std::vector<uint8_t> padded(bytes, bytes + len);
  padded.resize(len + 64, 0x20);
  std::vector<uint32_t> idx(len + 16);
  uint32_t n = 0;
  p.code = sjo_stage1(padded.data(), len, SJO_REGULAR, len ? len : 1, idx.data(), &n);
  if (p.code) { return p; }
  p.tape.resize(len + 8);
  p.strings.resize(5 * (len / 3) + 128);
  uint64_t tw = 0, sb = 0;
  p.code = sjo_stage2(padded.data(), len, idx.data(), n, max_depth, p.tape.data(), p.tape.size(), p.strings.data(), p.strings.size(), &tw, &sb);
  p.tape.resize(p.code ? 0 : tw);
  p.strings.resize(p.code ? 0 : sb);
  return p;
}

struct run_out {
  tape_result_dev ht;
  strings_result_dev hs;
  many_result_dev hm;
  many_workspace mw;
  tape_stream_view view;
  strings_result_dev *sres;
};
// one run over idx[0 .. n) of doc[0 .. len), as sjgpu_capi_stage2.hip lays it out
static void run_many(std::vector<uint8_t> &ws_store, const uint8_t *doc, size_t len, const uint32_t *idx, uint32_t n, uint32_t max_depth, uint8_t *sbuf, size_t str_cap,
                     run_out *r, unsigned long *reruns) {
  const size_t scratch_at = 256, scratch = strings_scratch_bytes(n, len), offs_at = scratch_at + scratch;
  const size_t tape_at = (offs_at + (size_t(n) + 1) * 4 + 255) & ~size_t(255);
  const size_t many_at = (tape_at + tape_workspace_bytes(n, len) + 255) & ~size_t(255);
  uint8_t *ws = static_cast<uint8_t *>(aligned(ws_store, many_at + many_workspace_bytes(n, len), 0xA5)); // the workspace is NOT zeroed by the caller
  r->sres = reinterpret_cast<strings_result_dev *>(ws + tape_at + 64);
  many_result_dev *mres = reinterpret_cast<many_result_dev *>(ws + tape_at + 96);
  uint32_t *offsets = reinterpret_cast<uint32_t *>(ws + offs_at);
  r->mw = carve_many_workspace(ws + many_at, n);
  r->view = tape_workspace_view(ws + tape_at, n, len);
  int roads = STRINGS_STREAM_ONLY;
  bool deep = false;
  for (;;) {
    const int *string_tokens = launch_tape_front(doc, len, idx, n, max_depth, ws + tape_at, nullptr);
    const strings_handoff strs = launch_parse_strings(doc, len, idx, n, false, sbuf, str_cap, offsets, r->sres, ws + scratch_at, nullptr, string_tokens, roads);
    launch_tape_stream(doc, len, idx, n, max_depth, offsets, strs, sbuf, r->mw.flat_tape, r->mw.flat_cap, ws + tape_at, nullptr, deep, r->mw.doc_ord, r->mw.doc_str);
    launch_many_ordinals(idx, n, r->mw, r->view, r->sres, mres, nullptr);
    r->ht = *reinterpret_cast<const tape_result_dev *>(ws + tape_at);
    r->hs = *r->sres;
    r->hm = *mres;
    bool again = false;
    if (roads == STRINGS_STREAM_ONLY && r->hs.path == 2 && !r->hs.overflow) { roads = STRINGS_WALK_ONLY; again = true; }
    if (!deep && r->ht.max_level >= TAPE_ONE_PASS_LEVELS) { deep = true; again = true; }
    if (!again) { break; }
    (*reruns)++;
  }
}

int main() {
  sj_emu::max_concurrent_workgroups = 4;
  unsigned long streams = 0, skipped = 0, delivered = 0, broken = 0, reruns = 0, second_runs = 0, codes[32] = {0};
  std::vector<uint8_t> doc_store, ws_store, tape_store, sbuf_store, idx_store, table_store;
  for (;;) {
    uint32_t len;
    if (fread(&len, 4, 1, stdin) != 1) { break; }
    uint8_t *doc = static_cast<uint8_t *>(aligned(doc_store, size_t(len) + 4096, '"')); // what lies behind the stream is no padding: quotes and backslashes
    for (size_t k = len; k < size_t(len) + 4096; k += 2) { doc[k] = '\\'; }
    if (len && fread(doc, 1, len, stdin) != len) { return 2; }
    uint32_t max_depth, count;
    int32_t want_docs, want_code;
    if (fread(&max_depth, 4, 1, stdin) != 1 || fread(&want_docs, 4, 1, stdin) != 1 || fread(&want_code, 4, 1, stdin) != 1 || fread(&count, 4, 1, stdin) != 1) { return 2; }
    std::vector<uint32_t> begin(size_t(count) + 1, len);
    if (count && fread(begin.data(), 4, count, stdin) != count) { return 2; }
    streams++;
    uint32_t *idx = static_cast<uint32_t *>(aligned(idx_store, (size_t(len) + 16) * 4, 0xEE));
    uint32_t n = 0;
    {
      std::vector<uint8_t> padded(doc, doc + len);
      padded.resize(size_t(len) + 64, 0x20);
      const int e1 = sjo_stage1(padded.data(), len, SJO_REGULAR, len ? len : 1, idx, &n);
      if (e1 == SJO_EMPTY || n == 0) { // sjgpu_stage2_many_device: n == 0 is EMPTY, nothing delivered
        if (want_docs >= 0 && (want_docs != 0 || want_code != SJO_EMPTY)) { fprintf(stderr, "MISMATCH: an empty list is 0 documents, code 13 (stream %lu)\n", streams); return 1; }
        codes[SJO_EMPTY]++;
        continue;
      }
      if (e1) { skipped++; continue; } // stage 1 rejects the whole buffer: not this call's business
    }
    // ---- the expectation -----------------------------------------------------------------------------------------------------------------
    std::vector<parsed> want;
    if (want_docs < 0) {
      want_code = 0;
      for (uint32_t d = 0; d < count; d++) {
        parsed p = oracle_parse(doc + begin[d], begin[d + 1] - begin[d], max_depth);
        if (p.code) { want_code = p.code; break; }
        want.push_back(std::move(p));
      }
      want_docs = int32_t(want.size());
    }
    // ---- the device road, as sjgpu_stage2_many_device runs it ---------------------------------------------------------------------------------
    const size_t str_cap = 5 * (size_t(len) / 3) + 256, tape_cap = 4 * size_t(n) + 8, table_cap = size_t(n) + 1;
    uint8_t *sbuf = static_cast<uint8_t *>(aligned(sbuf_store, str_cap, 0x5A));
    uint64_t *tape = static_cast<uint64_t *>(aligned(tape_store, tape_cap * 8, 0x5A));
    doc_span_dev *table = static_cast<doc_span_dev *>(aligned(table_store, table_cap * sizeof(doc_span_dev), 0x5A));
    run_out r;
    run_many(ws_store, doc, len, idx, n, max_depth, sbuf, str_cap, &r, &reruns);
    int got_code = 0;
    uint32_t n_run = n, got_docs = 0;
    bool deliver = true;
    if (r.hm.has_error) {
      uint64_t key = r.ht.error_key;
      if (r.hs.first_bad != 0xFFFFFFFFu) {
        const uint64_t sk = (uint64_t(r.hs.first_bad) << 8) | (2u << 4) | 5u;
        if (sk < key) { key = sk; }
      }
      got_code = int(key & 0xFu);
      broken++;
      n_run = r.hm.cut_token;
      if (n_run > n || r.hm.cut_byte != idx[n_run]) { fprintf(stderr, "MISMATCH: the cut (token %u, byte %u) is no token of the list (stream %lu)\n", n_run, r.hm.cut_byte, streams); return 1; }
      if (n_run == 0) { deliver = false; }
      else {
        second_runs++;
        run_many(ws_store, doc, r.hm.cut_byte, idx, n_run, max_depth, sbuf, str_cap, &r, &reruns);
        if (r.hm.has_error) { fprintf(stderr, "MISMATCH: the prefix in front of the broken document reports an error itself (key %llx, stream %lu)\n", (unsigned long long)r.ht.error_key, streams); return 1; }
      }
    }
    uint64_t total = 0;
    if (deliver) {
      if (r.hs.overflow || r.ht.overflow) { fprintf(stderr, "MISMATCH: overflow with buffers that always suffice (stream %lu)\n", streams); return 1; }
      got_docs = r.hm.docs;
      total = r.ht.tape_words + 2ull * got_docs;
      if (size_t(got_docs) + 1 > table_cap || total > tape_cap) { fprintf(stderr, "MISMATCH: %u documents, %llu words do not fit what always suffices (stream %lu)\n", got_docs, (unsigned long long)total, streams); return 1; }
      launch_many_relocate(idx, n_run, got_docs, total, r.mw, r.view, r.sres, table, tape, nullptr);
    }
    codes[got_code & 31]++;
    if (got_code != want_code || int32_t(got_docs) != want_docs) {
      fprintf(stderr, "MISMATCH: %u documents delivered, code %d; expected %d, code %d (stream %lu, %u bytes, max_depth %u): %.*s\n", got_docs, got_code, want_docs, want_code, streams, len,
              max_depth, int(len > 300 ? 300 : len), (const char *)doc);
      return 1;
    }
    if (!deliver) { continue; }
    // ---- the table and the slices ----------------------------------------------------------------------------------------------------------
    const doc_span_dev last = table[got_docs];
    if (last.first_token != n_run || last.byte_begin != idx[n_run] || last.tape_begin != total || last.string_begin != r.hs.bytes) {
      fprintf(stderr, "MISMATCH: the table's last entry {%u, %u, %u, %u}, expected {%u, %u, %llu, %llu} (stream %lu)\n", last.first_token, last.byte_begin, last.tape_begin,
              last.string_begin, n_run, idx[n_run], (unsigned long long)total, (unsigned long long)r.hs.bytes, streams);
      return 1;
    }
    for (size_t k = total; k < tape_cap; k++) { if (tape[k] != 0x5A5A5A5A5A5A5A5Aull) { fprintf(stderr, "MISMATCH: tape word %zu behind the %llu delivered was written (stream %lu)\n", k, (unsigned long long)total, streams); return 1; } }
    for (size_t k = size_t(got_docs) + 1; k < table_cap; k++) { if (table[k].first_token != 0x5A5A5A5Au) { fprintf(stderr, "MISMATCH: table entry %zu behind the last was written (stream %lu)\n", k, streams); return 1; } }
    for (uint32_t d = 0; d < got_docs; d++) {
      const doc_span_dev a = table[d], b = table[d + 1];
      if (a.byte_begin != idx[a.first_token] || a.first_token >= b.first_token || a.tape_begin >= b.tape_begin || a.string_begin > b.string_begin ||
          (d == 0 && (a.first_token != 0 || a.tape_begin != 0 || a.string_begin != 0))) {
        fprintf(stderr, "MISMATCH: table entry %u {%u, %u, %u, %u} (stream %lu)\n", d, a.first_token, a.byte_begin, a.tape_begin, a.string_begin, streams);
        return 1;
      }
      parsed derived;
      const parsed *w;
      if (d < want.size()) {
        w = &want[d];
        if (a.byte_begin != begin[d]) { fprintf(stderr, "MISMATCH: document %u begins at byte %u, expected %u (stream %lu)\n", d, a.byte_begin, begin[d], streams); return 1; }
      } else {
        derived = oracle_parse(doc + a.byte_begin, b.byte_begin - a.byte_begin, max_depth);
        if (derived.code) { fprintf(stderr, "MISMATCH: the oracle rejects delivered document %u (code %d, stream %lu)\n", d, derived.code, streams); return 1; }
        w = &derived;
      }
      const size_t words = b.tape_begin - a.tape_begin, bytes = b.string_begin - a.string_begin;
      if (words != w->tape.size() || memcmp(tape + a.tape_begin, w->tape.data(), words * 8) != 0) {
        fprintf(stderr, "MISMATCH: the tape of document %u differs (%zu words, the oracle %zu; stream %lu, %u documents): %.*s\n", d, words, w->tape.size(), streams, got_docs,
                int(b.byte_begin - a.byte_begin > 200 ? 200 : b.byte_begin - a.byte_begin), (const char *)doc + a.byte_begin);
        for (size_t k = 0; k < words && k < w->tape.size(); k++) {
          if (tape[a.tape_begin + k] != w->tape[k]) { fprintf(stderr, "  word %zu: %016llx, the oracle %016llx\n", k, (unsigned long long)tape[a.tape_begin + k], (unsigned long long)w->tape[k]); break; }
        }
        return 1;
      }
      if (bytes != w->strings.size() || memcmp(sbuf + a.string_begin, w->strings.data(), bytes) != 0) {
        fprintf(stderr, "MISMATCH: the string records of document %u differ (%zu bytes, the oracle %zu; stream %lu)\n", d, bytes, w->strings.size(), streams);
        return 1;
      }
      delivered++;
    }
  }
  printf("%lu streams, %lu documents delivered, 0 mismatches; %lu broken streams, %lu second runs, %lu skipped;", streams, delivered, broken, second_runs, skipped);
  for (int k = 0; k < 32; k++) { if (codes[k]) { printf(" code %d: %lu", k, codes[k]); } }
  printf(" (repeated roads: %lu)\n", reruns);
  return 0;
}
