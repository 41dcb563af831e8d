// Stand-alone host check of the scan kernel's record semantics:
// dragnet_amd/ops/hip/{dec2dbl,scan_text,scan_record}.h compiled by a
// plain host C++ compiler — the same source the device compiles.
//
//   c++ -O2 -std=c++17 -I dragnet_amd/ops/hip -o kernel_host_check
//       tools_dev/kernel_host_check.cpp           (one command line)
//   kernel_host_check <bytes|x5|x6|x7> < requests > answers
//
// The argument picks the byte source every record-consuming request
// runs through: Bytes, or the wave-transposed XBytesT<5|6|7>.  One
// request per stdin line, one answer line per request (tests/
// test_kernel_host.py drives it; payload bytes are hex, "-" = empty):
//
//   dec2dbl <mant> <exp10>      -> <bits>
//   number <hex>                -> ok|invalid <bits> <consumed>
//        parse_json_number; ok only if it spans the whole literal
//   tonumber <hex>              -> <bits>          js_to_number (raw span)
//   date <hex>                  -> ok <ms> | invalid        parse_iso_ms
//   keysig <0|1> <hex>...       -> <sig> | invalid
//        scan_key_sig per key, each chained on the previous signature;
//        the flag is dot_splits
//   plan <dot_splits> <nf> <bloom> <fields_parent_sig>      (no answer)
//   field_sigs|prog_nodes|prog_bounds|const_meta|const_dvals|const_bytes
//        <values>... the plan's arrays as plan.compile_plan packs them
//        (no answer; u64 and doubles as hex bits)
//   record <hex>                -> 0 | 1 <top_type> <slot>... ; <prog>...
//        parse_record, then eval_predicate per program.  A slot is
//        "<type>" if missing/null/bool, "4:<bits>" for a number,
//        "<type>:<off>:<len>" for a string/object/array span.
//
// Buffers are heap blocks of EXACTLY the size the host engine promises
// the device, slack filled with '\n', so a sanitizer build checks the
// "may read up to 15 bytes past end" contract rather than hiding it:
//   Bytes     engine/chunks.py _pad(n + 1): record, its newline, slack
//   XBytesT   lane 0 of a one-wave layout as engine/gpu.py stage_xpose
//             sizes it: max(1, ceil(n / GRAN)) granule rows STRIDE
//             apart plus one STRIDE of slack
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "scan_record.h"

using namespace dn;

static uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

static std::string unhex(const std::string& h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2)
    out.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return out;
}

// One record laid out for byte source BS in an exact-size heap block.
template <class BS> struct Staged;

template <> struct Staged<Bytes> {
  uint8_t* buf;
  Bytes src;
  explicit Staged(const std::string& rec) {
    size_t n = rec.size() + 1;             // the record and its newline
    size_t padded = (n + 16 + 15) & ~(size_t)15;  // chunks.py _pad
    buf = (uint8_t*)std::malloc(padded);
    std::memset(buf, '\n', padded);
    std::memcpy(buf, rec.data(), rec.size());
    src.mem = buf;
    src.bias = 0;
  }
  ~Staged() { std::free(buf); }
};

template <int LG> struct Staged<XBytesT<LG>> {
  uint8_t* buf;
  XBytesT<LG> src;
  explicit Staged(const std::string& rec) {
    const size_t GRAN = XBytesT<LG>::GRAN, STRIDE = XBytesT<LG>::STRIDE;
    size_t rows = (rec.size() + GRAN - 1) / GRAN;
    if (rows == 0) rows = 1;
    size_t total = rows * STRIDE + STRIDE;  // gpu.py: + one stride slack
    buf = (uint8_t*)std::malloc(total);
    std::memset(buf, '\n', total);
    for (size_t p = 0; p < rec.size(); p++)
      buf[(p >> LG) * STRIDE + (p & (GRAN - 1))] = (uint8_t)rec[p];
    src.base = buf;  // wave base 0, lane 0
  }
  ~Staged() { std::free(buf); }
};

struct Plan {
  std::vector<uint64_t> field_sigs;
  std::vector<int32_t> prog_nodes, prog_bounds, const_meta;
  std::vector<double> const_dvals;
  std::vector<uint8_t> const_bytes;
  bool dot_splits = false;
  PlanView P;
  // what the kernel keeps in LDS, for lane 0 of one block
  std::vector<uint8_t> fv_type;
  std::vector<uint32_t> fv_soff, fv_slen;
  std::vector<uint64_t> sig_stack;

  void bind() {
    P.field_sigs = field_sigs.data();
    P.prog_nodes = prog_nodes.data();
    P.prog_bounds = prog_bounds.data();
    P.const_meta = const_meta.data();
    P.const_dvals = const_dvals.data();
    P.const_bytes = const_bytes.data();
    fv_type.assign((size_t)P.nf * BLOCK, T_MISSING);
    fv_soff.assign((size_t)P.nf * BLOCK, 0);
    fv_slen.assign((size_t)P.nf * BLOCK, 0);
    sig_stack.assign((size_t)SIG_DEPTH * BLOCK, 0);
  }
};

template <class BS>
static void do_record(Plan& pl, const std::string& rec) {
  Staged<BS> st(rec);
  pl.bind();
  FV fv;
  fv.type = pl.fv_type.data();
  fv.soff = pl.fv_soff.data();
  fv.slen = pl.fv_slen.data();
  fv.tid = 0;
  uint8_t top = T_MISSING;
  bool ok = parse_record(st.src, 0u, (uint32_t)rec.size(), pl.P, fv, top,
                         pl.sig_stack.data(), pl.dot_splits);
  if (!ok) { std::printf("0\n"); return; }
  std::printf("1 %d", (int)top);
  for (int f = 0; f < pl.P.nf; f++) {
    int t = fv.get_type(f);
    if (t == T_NUM)
      std::printf(" 4:%016" PRIx64, bits_of(fv.get_num(f)));
    else if (t == T_STR || t == T_OBJ || t == T_ARR)
      std::printf(" %d:%u:%u", t, fv.get_soff(f), fv.get_slen(f));
    else
      std::printf(" %d", t);
  }
  std::printf(" ;");
  int nprogs = (int)pl.prog_bounds.size() / 2;
  for (int p = 0; p < nprogs; p++)
    std::printf(" %d", eval_predicate(pl.P, st.src, fv, p));
  std::printf("\n");
}

template <class BS>
static int serve() {
  Plan pl;
  std::memset(&pl.P, 0, sizeof(pl.P));
  std::string line, mode, tok;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    if (!(in >> mode)) continue;
    if (mode == "dec2dbl") {
      unsigned long long mant; long ex;
      in >> mant >> ex;
      std::printf("%016" PRIx64 "\n",
                  bits_of(dn_dec2dbl((uint64_t)mant, ex, P10_TBL)));
    } else if (mode == "number") {
      in >> tok;
      std::string lit = unhex(tok);
      Staged<BS> st(lit);
      CursorT<BS> c;
      c.init(st.src, 0u, (uint32_t)lit.size());
      NumOut n = parse_json_number(c);
      std::printf("%s %016" PRIx64 " %u\n",
                  n.ok && c.pos == c.end ? "ok" : "invalid", bits_of(n.v),
                  c.pos);
    } else if (mode == "tonumber") {
      in >> tok;
      std::string s = unhex(tok);
      Staged<BS> st(s);
      std::printf("%016" PRIx64 "\n",
                  bits_of(js_to_number(st.src, 0u, (uint32_t)s.size())));
    } else if (mode == "date") {
      in >> tok;
      std::string s = unhex(tok);
      Staged<BS> st(s);
      DateOut d = parse_iso_ms(st.src, 0u, (uint32_t)s.size());
      if (d.ok) std::printf("ok %lld\n", d.ms);
      else std::printf("invalid\n");
    } else if (mode == "keysig") {
      int dot_splits;
      in >> dot_splits;
      uint64_t sig = FNV_OFFSET;
      bool ok = true;
      while (ok && (in >> tok)) {
        std::string key = unhex(tok) + "\"";  // cursor sits after the
        Staged<BS> st(key);                   // opening quote
        CursorT<BS> c;
        c.init(st.src, 0u, (uint32_t)key.size());
        uint64_t out = 0;
        ok = scan_key_sig(c, sig, out, dot_splits != 0) != 0;
        sig = out;
      }
      if (ok) std::printf("%016" PRIx64 "\n", sig);
      else std::printf("invalid\n");
    } else if (mode == "plan") {
      int ds;
      std::string bloom, fps;
      in >> ds >> pl.P.nf >> bloom >> fps;
      pl.dot_splits = ds != 0;
      pl.P.sig_bloom = std::stoull(bloom, nullptr, 16);
      pl.P.fields_parent_sig = std::stoull(fps, nullptr, 16);
    } else if (mode == "field_sigs") {
      pl.field_sigs.clear();
      while (in >> tok) pl.field_sigs.push_back(std::stoull(tok, nullptr, 16));
    } else if (mode == "const_dvals") {
      pl.const_dvals.clear();
      while (in >> tok) {
        uint64_t b = std::stoull(tok, nullptr, 16);
        double v;
        std::memcpy(&v, &b, 8);
        pl.const_dvals.push_back(v);
      }
    } else if (mode == "const_bytes") {
      in >> tok;
      std::string b = unhex(tok);
      pl.const_bytes.assign(b.begin(), b.end());
    } else if (mode == "prog_nodes" || mode == "prog_bounds" ||
               mode == "const_meta") {
      std::vector<int32_t>& v = mode == "prog_nodes" ? pl.prog_nodes
                              : mode == "prog_bounds" ? pl.prog_bounds
                                                      : pl.const_meta;
      v.clear();
      long x;
      while (in >> x) v.push_back((int32_t)x);
    } else if (mode == "record") {
      tok = "-";
      in >> tok;
      do_record<BS>(pl, unhex(tok));
    } else {
      std::fprintf(stderr, "unknown request: %s\n", mode.c_str());
      return 2;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  std::string src = argc > 1 ? argv[1] : "bytes";
  if (src == "bytes") return serve<Bytes>();
  if (src == "x5") return serve<XBytesT<5>>();
  if (src == "x6") return serve<XBytesT<6>>();
  if (src == "x7") return serve<XBytesT<7>>();
  std::fprintf(stderr, "usage: kernel_host_check <bytes|x5|x6|x7>\n");
  return 2;
}
