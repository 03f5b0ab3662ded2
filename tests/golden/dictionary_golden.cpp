// tests/golden/dictionary_golden.cpp -- asks the REAL reference for the dictionary of a column: the elements e of doc.at_path_with_wildcard(p), and for each either
// e.get_string() (mode 0: a column of values; an element that is no string is a null) or `for (dom::key_value_pair f : dom::object(e))` with f.key (mode 1: the keys
// of a set of records; an element that is no object has no field), entered into a std::unordered_map<std::string_view, entry> in the order they are met -- equality is
// std::string_view == on the unescaped bytes.  Built and run by tests/golden/make_dictionary_golden.py only (against the reference's public headers and
// oracle/_ref/libsjref.so); its binary is never committed.
// stdin:  [u32 documents] then every document as [u32 length][bytes]; [u32 cases] then every case as [u32 document][u32 mode][u32 length][path]
// stdout: per case
//   C E <code> | C <cells> <nulls> <distinct>     the path failed, or that many cells (mode 0: elements, mode 1: fields), nulls among them, distinct strings
//   <distinct> lines  <string as hex, - for the empty one> <first cell> <count> <ten counts: the values under the key that are { [ " l u d t f n and negative l>
//                     (mode 0: the ten counts are those of the cells themselves: all strings)
//   one line          the codes of the cells, -1 for a null, separated by blanks (`.` when there is no cell)
#include "simdjson.h"

#include <cstdint>
#include <cstdio>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

using namespace simdjson;

static bool read_u32(uint32_t *v) { return fread(v, 4, 1, stdin) == 1; }
static bool read_blob(std::string *s) {
  uint32_t n;
  if (!read_u32(&n)) { return false; }
  s->resize(n);
  return n == 0 || fread(&(*s)[0], 1, n, stdin) == n;
}

struct entry {
  std::string_view text;
  size_t first, count;
  size_t kinds[10];
};

static void count_kind(entry *d, dom::element v) {
  switch (v.type()) {
    case dom::element_type::OBJECT: d->kinds[0]++; break;
    case dom::element_type::ARRAY: d->kinds[1]++; break;
    case dom::element_type::STRING: d->kinds[2]++; break;
    case dom::element_type::INT64: d->kinds[3]++; if (int64_t(v) < 0) { d->kinds[9]++; } break;
    case dom::element_type::UINT64: d->kinds[4]++; break;
    case dom::element_type::DOUBLE: d->kinds[5]++; break;
    case dom::element_type::BOOL: d->kinds[bool(v) ? 6 : 7]++; break;
    case dom::element_type::NULL_VALUE: d->kinds[8]++; break;
    default: break;
  }
}

int main() {
  uint32_t ndocs, ncases;
  if (!read_u32(&ndocs)) { return 2; }
  std::vector<std::string> docs(ndocs);
  for (std::string &d : docs) { if (!read_blob(&d)) { return 2; } }
  if (!read_u32(&ncases)) { return 2; }
  for (uint32_t c = 0; c < ncases; c++) {
    uint32_t which, mode;
    std::string path;
    if (!read_u32(&which) || !read_u32(&mode) || !read_blob(&path) || which >= ndocs) { return 2; }
    dom::parser parser;
    dom::element root;
    const error_code pe = parser.parse(padded_string(docs[which])).get(root);
    if (pe) { fprintf(stderr, "the reference rejects document %u (%d)\n", which, int(pe)); return 1; }
    std::vector<dom::element> rows;
    const error_code re = root.at_path_with_wildcard(std::string_view(path.data(), path.size())).get(rows);
    if (re) { printf("C E %d\n", int(re)); continue; }
    std::unordered_map<std::string_view, size_t> index;
    std::vector<entry> dict;
    std::vector<long> codes;
    size_t nulls = 0;
    auto enter = [&](std::string_view s, dom::element counted) {
      auto found = index.find(s);
      if (found == index.end()) {
        found = index.emplace(s, dict.size()).first;
        dict.push_back(entry{s, codes.size(), 0, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}});
      }
      entry &d = dict[found->second];
      d.count++;
      count_kind(&d, counted);
      codes.push_back(long(found->second));
    };
    for (dom::element e : rows) {
      if (mode == 0) {
        std::string_view s;
        if (e.get_string().get(s) == SUCCESS) { enter(s, e); } else { nulls++; codes.push_back(-1); }
      } else {
        dom::object obj;
        if (e.get_object().get(obj) != SUCCESS) { continue; }
        for (dom::key_value_pair f : obj) { enter(f.key, f.value); }
      }
    }
    printf("C %zu %zu %zu\n", codes.size(), nulls, dict.size());
    for (const entry &d : dict) {
      if (d.text.empty()) { printf("-"); }
      for (unsigned char ch : d.text) { printf("%02x", ch); }
      printf(" %zu %zu", d.first, d.count);
      for (size_t k : d.kinds) { printf(" %zu", k); }
      printf("\n");
    }
    if (codes.empty()) { printf("."); }
    for (size_t i = 0; i < codes.size(); i++) { printf(i ? " %ld" : "%ld", codes[i]); }
    printf("\n");
  }
  return 0;
}
