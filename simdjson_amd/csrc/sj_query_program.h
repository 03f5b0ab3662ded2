// simdjson_amd/csrc/sj_query_program.h -- JSON pointers compiled ONCE per call, on the host, into the program the walk of sjgpu_query.hip runs per cell.
// The reference's at_pointer parses the pointer while it walks (dom/object-inl.h:104-147, dom/array-inl.h:94-121, jsonpathutil.h:20-50,
// dom/element-inl.h:410-446), and what a token means depends on the element the walk finds there.  Nothing of that parse depends on the DOCUMENT
// beyond the element's kind, so every token is read in all three ways here and the kernel only picks one and compares:
//   as a key      the bytes with ~0 / ~1 unescaped, or INVALID_JSON_POINTER when a `~` is followed by anything else (the end of the token included)
//   as an index   the number, or the code parse_json_pointer_array_index gives -- the characters are tested in order, and per character "not a digit"
//                 (INCORRECT_TYPE) comes first, then "a leading zero in front of more" (INVALID_JSON_POINTER), then "beyond size_t"
//                 (INDEX_OUT_OF_BOUNDS); no character at all is INVALID_JSON_POINTER; `-` as the WHOLE rest of the pointer is INDEX_OUT_OF_BOUNDS
//   by a scalar   is_pointer_well_formed of the rest from this token's slash on: only the FIRST `~` of the rest is looked at
// Plain C++ (no HIP): shared by the C-ABI and by the CPU-tier driver of the kernels.
#ifndef SJ_QUERY_PROGRAM_H
#define SJ_QUERY_PROGRAM_H

#include <stdint.h>
#include <string.h>

#include <vector>

namespace sjgpu {

constexpr uint32_t QUERY_MAX_POINTERS = 64, QUERY_MAX_POINTER_BYTES = 1024, QUERY_MAX_TOKENS = 32;
constexpr uint32_t QUERY_INCORRECT_TYPE = 17, QUERY_INDEX_OUT_OF_BOUNDS = 19, QUERY_NO_SUCH_FIELD = 20, QUERY_INVALID_JSON_POINTER = 22;
// the key bytes of one pointer, every key padded to a multiple of 8: at most 1024 bytes of tokens and 7 bytes of padding per token
constexpr uint32_t QUERY_KEY_AREA = QUERY_MAX_POINTER_BYTES + 8 * QUERY_MAX_TOKENS;

struct query_token { // 32 bytes
  uint32_t key_off;     // where the unescaped key begins in its pointer's key area (a multiple of 8)
  uint32_t key_len;
  uint32_t key_code;    // 0, or INVALID_JSON_POINTER: an object that meets this token answers with it before any lookup
  uint32_t arr_code;    // 0, or what an array that meets this token answers
  uint64_t arr_index;   // arr_code == 0: the index
  uint32_t scalar_code; // what a scalar that meets this token answers: NO_SUCH_FIELD or INVALID_JSON_POINTER
  uint32_t pad;
};
struct query_pointer { // 16 bytes
  uint32_t first_token; // index into the tokens of the program
  uint32_t tokens;
  uint32_t code;        // INVALID_JSON_POINTER: not empty and no leading slash -- the answer for every document; else 0
  uint32_t keys_at;     // where the pointer's key area begins in the program's key bytes (a multiple of 8)
};
// [query_pointer x K][query_token x tokens][key bytes]
struct query_program {
  std::vector<uint8_t> bytes;
  uint32_t tokens_at = 0, keys_at = 0;
};

// the tokens of ONE pointer p[0 .. L) that begins with a slash, appended to toks and to keys (keys_base: where this pointer's key area begins in keys; key_off
// is counted from there).  *count: the tokens this key area holds so far; -> false: more than `room` of them.  Shared with sj_path_program.h.
inline bool append_pointer_tokens(const uint8_t *p, uint32_t L, uint32_t keys_base, uint32_t room, std::vector<query_token> *toks, std::vector<uint8_t> *keys_out, uint32_t *count) {
  std::vector<uint8_t> &keys = *keys_out;
  uint32_t slash = 0;
  while (slash < L) {
    uint32_t end = slash + 1;
    while (end < L && p[end] != '/') { end++; }
    if (*count == room) { return false; }
    const uint8_t *t = p + slash + 1;
    const uint32_t tl = end - slash - 1;
    query_token q;
    memset(&q, 0, sizeof q);
    // as a key
    q.key_off = uint32_t(keys.size()) - keys_base;
    for (uint32_t j = 0; j < tl; j++) {
      if (t[j] != '~') { keys.push_back(t[j]); continue; }
      const uint8_t next = j + 1 < tl ? t[j + 1] : 0; // (the reference reads the terminator behind its copy of the token)
      if (next == '0') { keys.push_back('~'); j++; }
      else if (next == '1') { keys.push_back('/'); j++; }
      else { q.key_code = QUERY_INVALID_JSON_POINTER; break; }
    }
    q.key_len = uint32_t(keys.size()) - keys_base - q.key_off;
    while (keys.size() & 7u) { keys.push_back(0); }
    // as an index
    if (tl == 1 && t[0] == '-' && end == L) { q.arr_code = QUERY_INDEX_OUT_OF_BOUNDS; }
    else {
      uint64_t index = 0;
      for (uint32_t j = 0; j < tl && !q.arr_code; j++) {
        const uint8_t digit = uint8_t(t[j] - '0');
        if (digit > 9) { q.arr_code = QUERY_INCORRECT_TYPE; }
        else if (j > 0 && t[0] == '0') { q.arr_code = QUERY_INVALID_JSON_POINTER; }
        else if (index > (~uint64_t(0) - digit) / 10) { q.arr_code = QUERY_INDEX_OUT_OF_BOUNDS; }
        else { index = index * 10 + digit; }
      }
      if (tl == 0) { q.arr_code = QUERY_INVALID_JSON_POINTER; }
      q.arr_index = q.arr_code ? 0 : index;
    }
    // by a scalar: the rest from this token's slash on
    q.scalar_code = QUERY_NO_SUCH_FIELD;
    for (uint32_t j = slash; j < L; j++) {
      if (p[j] != '~') { continue; }
      if (j + 1 == L || (p[j + 1] != '0' && p[j + 1] != '1')) { q.scalar_code = QUERY_INVALID_JSON_POINTER; }
      break;
    }
    toks->push_back(q);
    (*count)++;
    slash = end;
  }
  return true;
}

// -> false: K, a length or a token count beyond the limits
inline bool compile_query_program(const uint8_t *pointers, const uint32_t *lens, uint32_t K, query_program *out) {
  if (K > QUERY_MAX_POINTERS) { return false; }
  std::vector<query_pointer> ptrs(K);
  std::vector<query_token> toks;
  std::vector<uint8_t> keys;
  size_t at = 0;
  for (uint32_t k = 0; k < K; k++) {
    const uint32_t L = lens[k];
    if (L > QUERY_MAX_POINTER_BYTES) { return false; }
    const uint8_t *p = pointers + at;
    at += L;
    query_pointer &qp = ptrs[k];
    qp.first_token = uint32_t(toks.size());
    qp.tokens = 0;
    qp.code = 0;
    qp.keys_at = uint32_t(keys.size());
    if (L == 0) { continue; }
    if (p[0] != '/') { qp.code = QUERY_INVALID_JSON_POINTER; continue; }
    if (!append_pointer_tokens(p, L, qp.keys_at, QUERY_MAX_TOKENS, &toks, &keys, &qp.tokens)) { return false; }
  }
  out->tokens_at = uint32_t(K * sizeof(query_pointer));
  out->keys_at = uint32_t(out->tokens_at + toks.size() * sizeof(query_token));
  out->bytes.assign(size_t(out->keys_at) + keys.size() + 8, 0);
  if (K) { memcpy(out->bytes.data(), ptrs.data(), K * sizeof(query_pointer)); }
  if (!toks.empty()) { memcpy(out->bytes.data() + out->tokens_at, toks.data(), toks.size() * sizeof(query_token)); }
  if (!keys.empty()) { memcpy(out->bytes.data() + out->keys_at, keys.data(), keys.size()); }
  return true;
}

} // namespace sjgpu
#endif
