// Stand-alone host check of ops/hip/dbl2dec.h: reads binary64 bit patterns,
// 16 hex digits a line, and prints dn_js_number of each, a line each.
//
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined \
//       -I dragnet_amd/ops/hip tools_dev/dbl2dec_host_check.cpp \
//       -o /tmp/dbl2dec_host_check && echo 3ff8000000000000 | \
//       /tmp/dbl2dec_host_check
//
// Every string is written through the storing sink into a buffer of exactly
// the length the counting sink measured, allocated for it alone, so a byte
// more than measured is an AddressSanitizer report; a string longer than
// DN_JS_MAX, or a shortest form that dn_dbl2dec's own contract rules out
// (no digit, more than 17, a trailing zero), ends the program with status 1.
// tests/test_dbl2dec_host.py compares the output with an independent
// Number::toString and with strings recorded from V8.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dbl2dec.h"

int main() {
  char line[64];
  while (std::fgets(line, sizeof line, stdin)) {
    const uint64_t bits = std::strtoull(line, nullptr, 16);
    dn::DnCount cnt = {0};
    dn::dn_js_number(bits, cnt);
    if (cnt.n < 1 || cnt.n > (uint32_t)dn::DN_JS_MAX) {
      std::fprintf(stderr, "%016llx: %u bytes\n", (unsigned long long)bits,
                   cnt.n);
      return 1;
    }
    const uint64_t mag = bits & ~(1ull << 63);
    if (mag != 0 && mag < 0x7FF0000000000000ull) {
      uint64_t digits;
      int exp10;
      dn::dn_dbl2dec(mag, digits, exp10);
      if (digits == 0 || digits >= 100000000000000000ull ||
          (digits % 10 == 0)) {
        std::fprintf(stderr, "%016llx: digits %llu e%d\n",
                     (unsigned long long)bits, (unsigned long long)digits,
                     exp10);
        return 1;
      }
    }
    uint8_t* buf = (uint8_t*)std::malloc(cnt.n);
    dn::DnStore w = {buf};
    dn::dn_js_number(bits, w);
    if (w.p != buf + cnt.n) {
      std::fprintf(stderr, "%016llx: measured %u, wrote %ld\n",
                   (unsigned long long)bits, cnt.n, (long)(w.p - buf));
      return 1;
    }
    std::fwrite(buf, 1, cnt.n, stdout);
    std::fputc('\n', stdout);
    std::free(buf);
  }
  return 0;
}
