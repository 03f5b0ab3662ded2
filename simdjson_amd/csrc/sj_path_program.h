// simdjson_amd/csrc/sj_path_program.h -- JSONPath strings with wildcards compiled ONCE per call, on the host, into the LEVEL program the walk of
// k_at_paths (sjgpu_query.hip) runs per cell.
// The reference's at_path_with_wildcard parses the path while it recurses (dom/object-inl.h:155-244, dom/array-inl.h:129-214,
// dom/element-inl.h:448-459, jsonpathutil.h:58-161): every invocation looks at the string r that is left, does one thing and hands a SUFFIX of r to
// the invocations on the children.  Which suffix that is depends on r alone -- never on the document --, so the string left at recursion depth i is
// a function of the path, and so is what the invocation at that depth does with a container (a scalar contributes nothing at any depth,
// element-inl.h:456-457).  One level per depth:
//   ERR22      r is empty; or, behind an optional `$`, its next byte is neither `.` nor `[`; or r holds a `*` and get_next_key_and_json_path gives an
//              empty key (`[0]...`, an unterminated `['k`, `..`): INVALID_JSON_POINTER
//   WILD_LAST  r holds a `*` and is, behind the optional `$`, exactly `[*]` or `.*`: every child value is a match
//   WILD       r holds a `*` and its key is `*`: every child value goes on to the next level with the suffix
//   PTR        r holds a `*` and its key is anything else: at_pointer("/" + key) -- the key's bytes raw, so a `~` in it is read by the pointer's
//              rules and a `/` makes two tokens --; an error means no match, the element found goes on to the next level
//   TAIL       r holds no `*`: at_pointer(json_path_to_pointer_conversion(r)); one match or the pointer's code.  (The sentinel "-1" -- an unclosed
//              bracket -- is ERR22.)
// ERR22, WILD_LAST and TAIL end the program.  A code is the cell's status only at level 0; every deeper invocation's error is swallowed by the
// loop over the children (process_json_path_of_child_elements).
// The pointers of PTR and TAIL are compiled by sj_query_program.h's append_pointer_tokens, each as a pointer of its own: their lazy rules are
// those of sjgpu_at_pointers_device.  Plain C++ (no HIP): shared by the C-ABI and by the CPU-tier driver of the kernels.
#ifndef SJ_PATH_PROGRAM_H
#define SJ_PATH_PROGRAM_H

#include "sj_query_program.h"

#include <string>

namespace sjgpu {

constexpr uint32_t PATH_MAX_PATHS = 64, PATH_MAX_BYTES = 1024, PATH_MAX_LEVELS = 32, PATH_MAX_TOKENS = QUERY_MAX_TOKENS, PATH_MAX_WILDS = 8;
enum : uint32_t { PATH_ERR22 = 0, PATH_WILD_LAST = 1, PATH_WILD = 2, PATH_PTR = 3, PATH_TAIL = 4 };
// A path's key bytes: a key byte is a byte of the path (`~0` / `~1` only shrink), every token's key padded to a multiple of 8
static_assert(PATH_MAX_BYTES + 8 * PATH_MAX_TOKENS <= QUERY_KEY_AREA, "the key area of a pointer holds a path's keys");

struct alignas(8) path_level { // 16 bytes
  uint32_t kind;
  uint32_t first_token; // PTR, TAIL: index into the PATH's tokens
  uint32_t tokens;
  uint32_t pad;
};
struct alignas(8) path_header { // 32 bytes
  uint32_t first_level; // index into the levels of the program
  uint32_t levels;      // 1 .. PATH_MAX_LEVELS
  uint32_t first_token; // index into the tokens of the program
  uint32_t tokens;
  uint32_t keys_at;     // where the path's key area begins in the program's key bytes (a multiple of 8)
  uint32_t pad[3];
};
// [path_header x K][path_level x levels][query_token x tokens][key bytes]
struct path_program {
  std::vector<uint8_t> bytes;
  uint32_t levels_at = 0, tokens_at = 0, keys_at = 0;
};

namespace path_detail {
// get_next_key_and_json_path (jsonpathutil.h:109-161): -> the key (empty: none) and, in *rest, what is left behind it
inline std::string next_key(const std::string &r, std::string *rest) {
  std::string key;
  size_t i = (!r.empty() && r[0] == '$') ? 1 : 0;
  if (i < r.size() && r[i] == '.') {
    i++;
    const size_t start = i;
    while (i < r.size() && r[i] != '[' && r[i] != '.') { i++; }
    key = r.substr(start, i - start);
  } else if (i + 1 < r.size() && r[i] == '[' && (r[i + 1] == '\'' || r[i + 1] == '"')) {
    const char quote = r[i + 1];
    i += 2;
    const size_t start = i;
    while (i < r.size() && r[i] != quote) { i++; }
    if (i >= r.size() || i + 1 >= r.size() || r[i + 1] != ']') { *rest = r; return std::string(); }
    key = r.substr(start, i - start);
    i += 2;
  } else if (i + 2 < r.size() && r[i] == '[' && r[i + 1] == '*' && r[i + 2] == ']') {
    key = "*";
    i += 3;
  }
  *rest = r.substr(i);
  return key;
}
// json_path_to_pointer_conversion (jsonpathutil.h:58-107) of a string whose first byte behind the optional `$` is `.` or `[`; -> false: the sentinel
inline bool to_pointer(const std::string &r, std::string *out) {
  size_t i = (!r.empty() && r[0] == '$') ? 1 : 0;
  out->clear();
  auto put = [out](char c) {
    if (c == '~') { *out += "~0"; } else if (c == '/') { *out += "~1"; } else { *out += c; }
  };
  while (i < r.size()) {
    if (r[i] == '.') { *out += '/'; }
    else if (r[i] == '[') {
      *out += '/';
      i++;
      while (i < r.size() && r[i] != ']') { put(r[i]); i++; }
      if (i == r.size()) { return false; }
    } else { put(r[i]); }
    i++;
  }
  return true;
}
} // namespace path_detail

// -> false: K, a length, the levels, the tokens or the wildcards of a path beyond the limits (WILD and WILD_LAST both count as wildcards: at most
// PATH_MAX_WILDS of them, so the walk's stack -- one frame per WILD level -- never holds more than that)
inline bool compile_path_program(const uint8_t *paths, const uint32_t *lens, uint32_t K, path_program *out) {
  if (K > PATH_MAX_PATHS) { return false; }
  std::vector<path_header> heads(K);
  std::vector<path_level> levels;
  std::vector<query_token> toks;
  std::vector<uint8_t> keys;
  size_t at = 0;
  for (uint32_t k = 0; k < K; k++) {
    if (lens[k] > PATH_MAX_BYTES) { return false; }
    std::string r(reinterpret_cast<const char *>(paths + at), lens[k]);
    at += lens[k];
    path_header &h = heads[k];
    memset(&h, 0, sizeof h);
    h.first_level = uint32_t(levels.size());
    h.first_token = uint32_t(toks.size());
    h.keys_at = uint32_t(keys.size());
    uint32_t wilds = 0;
    for (bool done = false; !done;) {
      if (h.levels == PATH_MAX_LEVELS) { return false; }
      path_level lv;
      memset(&lv, 0, sizeof lv);
      lv.first_token = h.tokens;
      std::string pointer;
      const size_t i = (!r.empty() && r[0] == '$') ? 1 : 0;
      if (i >= r.size() || (r[i] != '.' && r[i] != '[')) {
        lv.kind = PATH_ERR22;
        done = true;
      } else if (r.find('*') == std::string::npos) {
        lv.kind = path_detail::to_pointer(r, &pointer) ? PATH_TAIL : PATH_ERR22;
        done = true;
      } else if (r.compare(i, std::string::npos, "[*]") == 0 || r.compare(i, std::string::npos, ".*") == 0) {
        lv.kind = PATH_WILD_LAST;
        if (++wilds > PATH_MAX_WILDS) { return false; }
        done = true;
      } else {
        std::string rest;
        const std::string key = path_detail::next_key(r, &rest);
        if (key.empty()) {
          lv.kind = PATH_ERR22;
          done = true;
        } else if (key == "*") {
          lv.kind = PATH_WILD;
          if (++wilds > PATH_MAX_WILDS) { return false; }
        } else {
          lv.kind = PATH_PTR;
          pointer = "/" + key;
        }
        r = rest;
      }
      if (lv.kind == PATH_PTR || lv.kind == PATH_TAIL) {
        if (!append_pointer_tokens(reinterpret_cast<const uint8_t *>(pointer.data()), uint32_t(pointer.size()), h.keys_at, PATH_MAX_TOKENS, &toks, &keys, &h.tokens)) { return false; }
        lv.tokens = h.tokens - lv.first_token;
      }
      levels.push_back(lv);
      h.levels++;
    }
  }
  out->levels_at = uint32_t(K * sizeof(path_header));
  out->tokens_at = uint32_t(out->levels_at + levels.size() * sizeof(path_level));
  out->keys_at = uint32_t(out->tokens_at + toks.size() * sizeof(query_token));
  out->bytes.assign(size_t(out->keys_at) + keys.size() + 8, 0);
  if (K) { memcpy(out->bytes.data(), heads.data(), K * sizeof(path_header)); }
  if (!levels.empty()) { memcpy(out->bytes.data() + out->levels_at, levels.data(), levels.size() * sizeof(path_level)); }
  if (!toks.empty()) { memcpy(out->bytes.data() + out->tokens_at, toks.data(), toks.size() * sizeof(query_token)); }
  if (!keys.empty()) { memcpy(out->bytes.data() + out->keys_at, keys.data(), keys.size()); }
  return true;
}

} // namespace sjgpu
#endif
