// Stand-alone host driver of the line routine of ops/hip/parse_points.h
// (pp_line and what it stands on), one request per stdin line, one answer
// per stdout line.
//
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -I dragnet_amd/ops/hip \
//       tools_dev/points_host_check.cpp -o /tmp/points_host_check
//
// Requests (HEX is the bytes in hexadecimal, `-` for none):
//   metric                 begins the next metric
//   col KIND STEP HEX      a column of it: kind 0..3, step, name
//   line HEX               one line, without its newline
// A line is answered through both sinks and must give the same class in
// both; the answer is
//   CLASS                  for skip, punt
//   drop METRIC
//   taken METRIC VALUE EL...   EL = i:<integer> or s:<hex of the span>
// Each line is copied into a buffer of exactly its length plus the 9 bytes
// `undefined` the op's caller puts behind the data, at a 16-byte boundary
// and again one byte further, so a read outside it is an AddressSanitizer
// report.  Exits 1 on a malformed request or when the sinks disagree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "parse_points.h"

namespace {

std::string unhex(const std::string& h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2)
    out.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return out;
}

std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string out;
  for (size_t i = 0; i < n; i++) {
    out.push_back(d[p[i] >> 4]);
    out.push_back(d[p[i] & 15]);
  }
  return out.empty() ? "-" : out;
}

std::string answer(const dn::PpSpecs& P, const std::string& line, int lead) {
  const size_t n = lead + line.size();
  uint8_t* text = (uint8_t*)std::malloc(n + dn::PP_TAIL);
  std::memset(text, ' ', (size_t)lead);
  std::memcpy(text + lead, line.data(), line.size());
  std::memcpy(text + n, "undefined", dn::PP_TAIL);
  const dn::PpGlobal S = {text};
  uint32_t lo = (uint32_t)lead, hi = (uint32_t)n;
  dn::pp_strip(S, lo, hi);
  int metric = -1, metric2 = -1;
  dn::PpCount cnt = {0};
  const uint8_t cls = dn::pp_line(S, lo, hi, P, (uint32_t)n, metric, cnt);
  const int kmax = dn::MAX_KEY;
  long long row[dn::MAX_KEY + 1] = {0};
  long long ss[dn::MAX_KEY] = {0}, sl[dn::MAX_KEY] = {0};
  int m_out = -1;
  double val = 0;
  dn::PpStore st = {&m_out, row, &val, ss, sl, 0, cnt.spans, kmax};
  const uint8_t cls2 = dn::pp_line(S, lo, hi, P, (uint32_t)n, metric2, st);
  if (cls != cls2 || metric != metric2) {
    std::fprintf(stderr, "sinks disagree: %d/%d\n", cls, cls2);
    std::exit(1);
  }
  std::ostringstream o;
  if (cls == dn::PP_SKIP) o << "skip";
  else if (cls == dn::PP_PUNT) o << "punt";
  else if (cls == dn::PP_DROP) o << "drop " << metric;
  else {
    o << "taken " << m_out << " " << (long long)val;
    for (int j = 0; j < P.nk[m_out]; j++) {
      if ((row[kmax] >> (2 * j)) & 3)
        o << " s:" << hex(text + ss[row[j]], (size_t)sl[row[j]]);
      else
        o << " i:" << row[j];
    }
  }
  std::free(text);
  return o.str();
}

}  // namespace

int main() {
  static dn::PpSpecs P;
  std::memset(&P, 0, sizeof(P));
  size_t used = 0;
  std::string req;
  while (std::getline(std::cin, req)) {
    std::istringstream in(req);
    std::string what;
    in >> what;
    if (what == "metric") {
      if (P.nm >= dn::PP_MAX_METRICS) return 1;
      P.nm++;
    } else if (what == "col") {
      int kind;
      double step;
      std::string h;
      in >> kind >> step >> h;
      const std::string name = unhex(h);
      const int m = P.nm - 1;
      if (m < 0 || P.nk[m] >= dn::MAX_KEY ||
          used + name.size() > (size_t)dn::PP_NAME_BYTES)
        return 1;
      const int j = P.nk[m]++;
      P.kind[m][j] = (uint8_t)kind;
      P.step[m][j] = step;
      P.name_off[m][j] = (uint16_t)used;
      P.name_len[m][j] = (uint16_t)name.size();
      std::memcpy(P.names + used, name.data(), name.size());
      used += name.size();
    } else if (what == "line") {
      std::string h;
      in >> h;
      const std::string line = unhex(h);
      const std::string a = answer(P, line, 0), b = answer(P, line, 1);
      if (a != b) {
        std::fprintf(stderr, "alignments disagree: %s | %s\n", a.c_str(),
                     b.c_str());
        return 1;
      }
      std::printf("%s\n", a.c_str());
    } else if (!what.empty()) {
      return 1;
    }
  }
  return 0;
}
