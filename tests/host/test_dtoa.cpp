// tests/host/test_dtoa.cpp -- CPU tier: simdjson_amd/csrc/sj_dtoa.h (the shortest digits of a double and their layout) and the integer printers of
// simdjson_amd/csrc/sj_json_text.h on the host, the same code the kernels of sjgpu_json.hip run.  tests/test_dtoa.py builds and drives it.
//   test_dtoa table          stdin: one double per line as 16 hex digits of its bits -> stdout: "<bits> <text>" per line
//   test_dtoa integers       stdin: "<l|u> <16 hex digits>" per line               -> stdout: "<tag> <bits> <text>" per line
//   test_dtoa live <seed> <count>   (built with -DSJ_DTOA_LIVE and linked with the reference) `count` seeded random bit patterns and all 2 046 powers of two against
//                                   simdjson::internal::to_chars, declared by hand below; prints every difference
// Every text is checked here before it is printed: it lies in a buffer of exactly its length between poisoned guards, dtoa_length says that length, it is at most
// 24 bytes, and strtod reads it back to the same bits.  Exit code 1 on any failure.
#include "sj_dtoa.h"
#include "sj_json_text.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace sjgpu;

#ifdef SJ_DTOA_LIVE
namespace simdjson {
namespace internal {
char *to_chars(char *first, const char *last, double value);
}
} // namespace simdjson
#endif

constexpr uint8_t POISON = 0x5A;

// the text of `bits` through dtoa_length + dtoa_write, in a buffer of exactly that length
static bool text_of(uint64_t bits, std::string *out) {
  const uint32_t want = dtoa_length(bits);
  if (want < 3 || want > DTOA_MAX_BYTES) { fprintf(stderr, "%016llx: length %u\n", (unsigned long long)bits, want); return false; }
  uint8_t buf[64 + DTOA_MAX_BYTES + 64];
  memset(buf, POISON, sizeof buf);
  const uint32_t got = dtoa_write(bits, buf + 64);
  if (got != want) { fprintf(stderr, "%016llx: wrote %u, counted %u\n", (unsigned long long)bits, got, want); return false; }
  for (size_t i = 0; i < sizeof buf; i++) {
    const bool inside = i >= 64 && i < 64 + want;
    if (!inside && buf[i] != POISON) { fprintf(stderr, "%016llx: a byte outside the text was written\n", (unsigned long long)bits); return false; }
  }
  out->assign(reinterpret_cast<const char *>(buf + 64), want);
  double back = strtod(out->c_str(), nullptr);
  uint64_t back_bits;
  memcpy(&back_bits, &back, 8);
  if (back_bits != bits) { fprintf(stderr, "%016llx: %s reads back as %016llx\n", (unsigned long long)bits, out->c_str(), (unsigned long long)back_bits); return false; }
  return true;
}

static uint64_t splitmix64(uint64_t *state) {
  uint64_t z = (*state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  char line[256];
  if (mode == "table") {
    while (fgets(line, sizeof line, stdin)) {
      const uint64_t bits = strtoull(line, nullptr, 16);
      std::string text;
      if (!dtoa_is_finite(bits) || !text_of(bits, &text)) { return 1; }
      printf("%016llx %s\n", (unsigned long long)bits, text.c_str());
    }
    return 0;
  }
  if (mode == "integers") {
    while (fgets(line, sizeof line, stdin)) {
      const char tag = line[0];
      const uint64_t bits = strtoull(line + 2, nullptr, 16);
      uint8_t buf[64 + 20 + 64];
      memset(buf, POISON, sizeof buf);
      const uint32_t want = tag == 'l' ? int64_text_length(bits) : decimal_digits(bits);
      const uint32_t got = tag == 'l' ? int64_text_write(bits, buf + 64) : (write_decimal(buf + 64, bits, want), want);
      if (got != want || want > 20) { return 1; }
      for (size_t i = 0; i < sizeof buf; i++) {
        if (!(i >= 64 && i < 64 + want) && buf[i] != POISON) { return 1; }
      }
      printf("%c %016llx %.*s\n", tag, (unsigned long long)bits, int(want), reinterpret_cast<const char *>(buf + 64));
    }
    return 0;
  }
#ifdef SJ_DTOA_LIVE
  if (mode == "live" && argc == 4) {
    uint64_t state = strtoull(argv[2], nullptr, 0);
    const unsigned long long count = strtoull(argv[3], nullptr, 0);
    unsigned long long differences = 0, done = 0;
    auto check = [&](uint64_t bits) {
      std::string text;
      if (!text_of(bits, &text)) { differences++; return; }
      char ref[64];
      double value;
      memcpy(&value, &bits, 8);
      const char *end = simdjson::internal::to_chars(ref, ref + sizeof ref, value);
      if (size_t(end - ref) != text.size() || memcmp(ref, text.data(), text.size()) != 0) {
        if (differences++ < 20) { fprintf(stderr, "%016llx: %s, the reference says %.*s\n", (unsigned long long)bits, text.c_str(), int(end - ref), ref); }
      }
      done++;
    };
    for (uint64_t e = 1; e <= 2046; e++) { check(e << 52); }
    for (unsigned long long i = 0; i < count;) {
      const uint64_t bits = splitmix64(&state);
      if (!dtoa_is_finite(bits)) { continue; }
      check(bits);
      i++;
    }
    printf("%llu compared, %llu differences\n", done, differences);
    return differences ? 1 : 0;
  }
#endif
  fprintf(stderr, "usage: test_dtoa table | integers | live <seed> <count>\n");
  return 2;
}
