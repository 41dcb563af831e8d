// Stand-alone host check of the two host-compilable routines of
// ops/hip/rank_strings.h: rank_key (the round key) and rank_compare (the
// from-depth comparison), against memcmp-with-length order.
//
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined \
//       -I dragnet_amd/ops/hip tools_dev/rank_host_check.cpp \
//       -o /tmp/rank_host_check && /tmp/rank_host_check
//
// Every dictionary is laid out at each of the 8 byte offsets and the blob
// is allocated at exactly round_up(bytes, 8), the padding the binding
// promises, so a read past it is an AddressSanitizer report.  Checked for
// every pair of strings: rank_compare's sign equals the truth's at every
// depth up to the common prefix, and the order of the round keys agrees
// with the truth on the chunk (key equal and low byte 8: equal chunks, both
// go on; key equal and low byte below 8: the same remainder).  Prints the
// counts and exits 0, or the first mismatch and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rank_strings.h"

namespace {

int truth(const std::string& a, const std::string& b) {
  const size_t n = std::min(a.size(), b.size());
  const int c = n ? std::memcmp(a.data(), b.data(), n) : 0;
  if (c) return c < 0 ? -1 : 1;
  return a.size() < b.size() ? -1 : a.size() > b.size() ? 1 : 0;
}

std::vector<std::string> dictionary() {
  std::vector<std::string> d = {
      "", "a", std::string("a\0", 2), std::string("a\0\0", 3),
      std::string("a\0b", 3), "ab", "abcdefg", "abcdefgh",
      std::string("abcdefg\0", 8), "\x80", "\x7f", "\xff\xff\xff\xff\xff\xff\xff",
      "\xff\xff\xff\xff\xff\xff\xff\xff"};
  uint64_t x = 0x9E3779B97F4A7C15ull;
  const unsigned char alphabet[] = {0x00, 0x01, 0x7f, 0x80, 0xff, 'a'};
  for (int i = 0; i < 160; i++) {
    std::string s;
    x = dn::mix64(x + i);
    const int len = (int)(x % 27);
    for (int k = 0; k < len; k++) {
      x = dn::mix64(x);
      s.push_back((char)alphabet[x % 6]);
    }
    d.push_back(s);
  }
  for (int i = 0; i < 24; i++)  // a long shared prefix
    d.push_back(std::string(50, 'p') + std::to_string(i * 37));
  return d;
}

}  // namespace

int main() {
  const std::vector<std::string> d = dictionary();
  long long compares = 0, keys = 0;
  for (int lead = 0; lead < 8; lead++) {
    std::vector<int64_t> offs = {lead};
    std::string bytes((size_t)lead, 'L');
    for (const auto& s : d) {
      bytes += s;
      offs.push_back((int64_t)bytes.size());
    }
    const size_t padded = (bytes.size() + 7) / 8 * 8;
    uint64_t* words = (uint64_t*)std::malloc(padded);  // 16-byte aligned
    std::memcpy(words, bytes.data(), bytes.size());
    for (size_t i = 0; i < d.size(); i++)
      for (size_t j = 0; j < d.size(); j++) {
        const std::string &a = d[i], &b = d[j];
        size_t common = 0;
        while (common < a.size() && common < b.size() &&
               a[common] == b[common])
          common++;
        for (size_t depth = 0; depth <= common; depth++) {
          const int got = dn::rank_compare(
              words, offs[i] + (int64_t)depth, offs[i + 1],
              offs[j] + (int64_t)depth, offs[j + 1]);
          compares++;
          if (got != truth(a, b)) {
            std::printf("rank_compare: strings %zu, %zu at depth %zu, lead "
                        "%d: %d, want %d\n", i, j, depth, lead, got,
                        truth(a, b));
            return 1;
          }
          const uint64_t ka = dn::rank_key(words, offs[i], offs[i + 1],
                                           (int64_t)depth) ^ dn::RANK_SIGN;
          const uint64_t kb = dn::rank_key(words, offs[j], offs[j + 1],
                                           (int64_t)depth) ^ dn::RANK_SIGN;
          keys++;
          const std::string ra = a.substr(depth), rb = b.substr(depth);
          const int want = truth(ra.substr(0, 7), rb.substr(0, 7));
          bool ok;
          if (ka != kb) {
            // differing keys order the strings, unless only the low bytes
            // differ as 7 against 8: then the one that ended is smaller
            ok = (ka < kb ? -1 : 1) == truth(ra, rb);
          } else if ((ka & 0xff) == 8) {
            ok = want == 0 && ra.size() >= 8 && rb.size() >= 8;
          } else {
            ok = ra == rb;
          }
          if (!ok) {
            std::printf("rank_key: strings %zu, %zu at depth %zu, lead %d: "
                        "keys %016llx %016llx\n", i, j, depth, lead,
                        (unsigned long long)ka, (unsigned long long)kb);
            return 1;
          }
        }
      }
    std::free(words);
  }
  std::printf("rank_host_check: %zu strings, 8 alignments, %lld comparisons "
              "and %lld key pairs agree with memcmp-with-length order\n",
              d.size(), compares, keys);
  return 0;
}
