// Stand-alone host check of dragnet_amd/ops/hip/dec2dbl.h.
//
//   c++ -O2 -std=c++17 -I dragnet_amd/ops/hip tools_dev/dec2dbl_check.cpp
//
// Reads "<mant> <exp10>" pairs (unsigned 64-bit decimal, signed
// decimal) from stdin and prints the 16-hex-digit bit pattern of
// dn_dec2dbl(mant, exp10) per line, so a driver (tests/
// test_numeric_cpu.py) can compare against a correctly rounded
// reference.  Plain host C++: the same header the device compiles.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "dec2dbl.h"

static const double P10[23] = {
    1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
    1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

int main() {
  unsigned long long mant;
  long ex;
  while (std::scanf("%llu %ld", &mant, &ex) == 2) {
    double v = dn::dn_dec2dbl((uint64_t)mant, ex, P10);
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    std::printf("%016" PRIx64 "\n", bits);
  }
  return 0;
}
