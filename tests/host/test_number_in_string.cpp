// tests/host/test_number_in_string.cpp -- CPU tier: the rules header simdjson_amd/csrc/sj_number_in_string.h, as the host compiler sees it.
//   test_number_in_string answers          stdin: [u32 contents] then [u32 length][bytes] each; stdout: per content `int64;uint64;double`, each `E <code>` or
//                                          16 hex digits -- the line format of tests/golden/in_string.json, which tests/test_in_string_model.py compares with
//   test_number_in_string random N SEED    N random decimals of every length and shape against strtoll, strtoull and strtod (glibc's strtod rounds correctly);
//                                          the grammar is restated here, independently of the header.  Exit code 1 and the first differences on stderr.
// Every content is copied into a heap block of exactly its length: a read at or beyond the end is the sanitizers' to find (tests/test_in_string_model.py builds
// this file with -fsanitize=address,undefined too).
#include "sj_number_in_string.h"

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>

using namespace sjgpu;

struct exact_bytes {
  const uint8_t *p;
  u32 byte(u32 i) const { return p[i]; }
};

struct answers { in_string_number a[3]; };

static answers ask(const std::string &c) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[c.size() ? c.size() : 1]);
  memcpy(copy.get(), c.data(), c.size());
  const exact_bytes src{copy.get()};
  static bigint big[2];
  answers r;
  r.a[0] = parse_integer_in_string(src, u32(c.size()), false);
  r.a[1] = parse_integer_in_string(src, u32(c.size()), true);
  r.a[2] = parse_double_in_string<true>(src, u32(c.size()), big);
  // the road the first kernel takes: everything but the value of a text of more than 19 significant digits is decided without big integers
  const in_string_number quick = parse_double_in_string<false>(src, u32(c.size()), static_cast<bigint *>(nullptr));
  if (!quick.slow && (quick.code != r.a[2].code || quick.value != r.a[2].value)) {
    fprintf(stderr, "the two roads differ for %s\n", c.c_str());
    exit(1);
  }
  return r;
}

static void print(const in_string_number &v) {
  if (v.code) { printf("E %u", v.code); } else { printf("%016llx", (unsigned long long)v.value); }
}

// ---- the expectation, from the C library -------------------------------------------------------------------------------------------------
static bool is_digit(char c) { return c >= '0' && c <= '9'; }

static in_string_number want_integer(const std::string &c, bool is_unsigned) {
  in_string_number r{17, 0, false};
  size_t p = (!is_unsigned && !c.empty() && c[0] == '-') ? 1 : 0;
  const size_t start = p;
  while (p < c.size() && is_digit(c[p])) { p++; }
  const size_t count = p - start;
  if (count == 0 || count > (is_unsigned ? 20u : 19u)) { return r; }
  r.code = 9;
  if (c[start] == '0' && count > 1) { return r; }
  if (p != c.size()) { return r; }
  r.code = 17;
  errno = 0;
  if (is_unsigned) {
    const unsigned long long v = strtoull(c.c_str(), nullptr, 10);
    if (errno == ERANGE) { return r; }
    r.value = v;
  } else {
    const long long v = strtoll(c.c_str(), nullptr, 10);
    if (errno == ERANGE) { return r; }
    r.value = u64(v);
  }
  r.code = 0;
  return r;
}

static in_string_number want_double(const std::string &c) {
  in_string_number r{17, 0, false};
  size_t p = (!c.empty() && c[0] == '-') ? 1 : 0;
  const size_t start = p;
  while (p < c.size() && is_digit(c[p])) { p++; }
  if (p == start) { return r; }
  r.code = 9;
  if (c[start] == '0' && p - start > 1) { return r; }
  if (p < c.size() && c[p] == '.') {
    const size_t frac = ++p;
    while (p < c.size() && is_digit(c[p])) { p++; }
    if (p == frac) { return r; }
  }
  if (p < c.size() && (c[p] == 'e' || c[p] == 'E')) {
    p++;
    if (p < c.size() && (c[p] == '-' || c[p] == '+')) { p++; }
    const size_t exp = p;
    while (p < c.size() && is_digit(c[p])) { p++; }
    if (p == exp || p - exp > 19) { return r; }
  }
  if (p != c.size()) { return r; }
  const double d = strtod(c.c_str(), nullptr);
  if (std::isinf(d)) { return r; }
  memcpy(&r.value, &d, 8);
  r.code = 0;
  return r;
}

static std::string random_content(std::mt19937_64 &rng) {
  auto pick = [&](u64 n) { return u64(rng() % n); };
  auto digits = [&](size_t n, bool may_lead_zero) {
    std::string s;
    for (size_t k = 0; k < n; k++) { s += char('0' + pick(10)); }
    if (n && !may_lead_zero && s[0] == '0') { s[0] = char('1' + pick(9)); }
    return s;
  };
  static const size_t lengths[] = {0, 1, 1, 2, 3, 5, 8, 15, 16, 17, 18, 19, 19, 20, 20, 21, 22, 25, 30, 40, 120, 400, 790, 810};
  std::string s;
  if (pick(3) == 0) { s += '-'; }
  const u64 shape = pick(16);
  if (shape == 0) { // the integers' edges
    static const char *edges[] = {"9223372036854775807", "9223372036854775808", "18446744073709551615", "18446744073709551616", "9007199254740993", "0"};
    s += edges[pick(6)];
    if (pick(4) == 0) { s.back() = char('0' + pick(10)); }
    return s;
  }
  size_t n = lengths[pick(sizeof lengths / sizeof lengths[0])];
  if (shape < 6 && n > 22) { n = 17 + pick(6); }
  s += pick(12) == 0 ? "0" + digits(pick(3), true) : digits(n, pick(10) == 0);
  if (shape >= 4 && pick(3)) {
    s += '.';
    if (pick(20)) { s += std::string(pick(4) ? 0 : pick(30), '0') + digits(pick(8) ? 1 + pick(20) : lengths[pick(sizeof lengths / sizeof lengths[0])], true); }
  }
  if (shape >= 4 && pick(2)) {
    s += pick(2) ? 'e' : 'E';
    const u64 sg = pick(3);
    if (sg) { s += sg == 1 ? '-' : '+'; }
    const u64 kind = pick(10);
    if (kind < 6) { s += std::to_string(pick(400)); }
    else if (kind == 6) { s += std::string(pick(19), '0') + std::to_string(pick(330)); }
    else if (kind == 7) { s += digits(17 + pick(5), true); }
    else if (kind == 8) { s += std::to_string(300 + pick(50)); }
  }
  if (pick(25) == 0) { // something that does not belong
    static const char junk[] = {' ', 'x', '"', '\\', '+', '-', '.', 'e', ',', '\0', char(0xC3)};
    s.insert(s.begin() + long(pick(s.size() + 1)), junk[pick(sizeof junk)]);
  }
  return s;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "answers")) {
    uint32_t n;
    if (fread(&n, 4, 1, stdin) != 1) { return 2; }
    for (uint32_t k = 0; k < n; k++) {
      uint32_t len;
      if (fread(&len, 4, 1, stdin) != 1) { return 2; }
      std::string c(len, '\0');
      if (len && fread(&c[0], 1, len, stdin) != len) { return 2; }
      const answers r = ask(c);
      print(r.a[0]);
      printf(";");
      print(r.a[1]);
      printf(";");
      print(r.a[2]);
      printf("\n");
    }
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "random")) {
    const unsigned long n = strtoul(argv[2], nullptr, 10);
    std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
    unsigned long bad = 0, per_code[3][3] = {};
    for (unsigned long k = 0; k < n; k++) {
      const std::string c = random_content(rng);
      const answers got = ask(c);
      const in_string_number want[3] = {want_integer(c, false), want_integer(c, true), want_double(c)};
      for (int g = 0; g < 3; g++) {
        per_code[g][want[g].code == 0 ? 0 : want[g].code == 9 ? 1 : 2]++;
        if (got.a[g].code != want[g].code || got.a[g].value != want[g].value) {
          if (bad++ < 20) {
            fprintf(stderr, "getter %d of `%s`: code %u value %016llx, wanted code %u value %016llx\n", g, c.c_str(), got.a[g].code, (unsigned long long)got.a[g].value,
                    want[g].code, (unsigned long long)want[g].value);
          }
        }
      }
    }
    for (int g = 0; g < 3; g++) { printf("getter %d: %lu values, %lu NUMBER_ERROR, %lu INCORRECT_TYPE\n", g, per_code[g][0], per_code[g][1], per_code[g][2]); }
    printf("%lu contents, %lu differences\n", n, bad);
    return bad ? 1 : 0;
  }
  fprintf(stderr, "usage: %s answers | random N SEED\n", argv[0]);
  return 2;
}
