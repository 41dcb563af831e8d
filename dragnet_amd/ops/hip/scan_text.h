// Text layer of the scan engine: pure functions from record bytes to
// values.  Device code under hipcc and plain C++17 under a host compiler
// (tools_dev/kernel_host_check.cpp); device-only spellings are in hd.h.
#pragma once
#include "common.h"
#include "dec2dbl.h"

namespace dn {

// -------------------------------------------------------------------
// small utilities

DN_HD_INLINE uint64_t fnv1a_byte(uint64_t h, uint8_t b) {
  return (h ^ (uint64_t)b) * 0x100000001B3ull;
}
constexpr uint64_t FNV_OFFSET = 0xCBF29CE484222325ull;

DN_CONST_TABLE double P10_TBL[23] = {
  1e0,1e1,1e2,1e3,1e4,1e5,1e6,1e7,1e8,1e9,1e10,1e11,1e12,1e13,1e14,
  1e15,1e16,1e17,1e18,1e19,1e20,1e21,1e22};
DN_CONST_TABLE int DIM_TBL[12] = {
  31,28,31,30,31,30,31,31,30,31,30,31};

DN_HD_INLINE uint64_t mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33; return x;
}

// -------------------------------------------------------------------
// byte cursor: 16B-buffered reads from the chunk

// Record bytes are addressed by ABSOLUTE chunk offset through a Bytes
// view: either the global chunk pointer (bias 0) or a block's LDS
// staging tile (bias = tile base).  Parsing from LDS turns the 64-way
// divergent per-byte gathers of thread-per-record parsing into banked
// LDS reads.
struct Bytes {
  const uint8_t* mem;
  uint32_t bias;
  DN_HD_INLINE uint8_t at(uint32_t abs) const { return mem[abs - bias]; }
  // 8 little-endian bytes starting at abs (may read 7 past a span;
  // host padding guarantees slack)
  DN_HD_INLINE uint64_t load8(uint32_t abs) const {
    uint64_t w;
    __builtin_memcpy(&w, mem + (abs - bias), 8);
    return w;
  }
};

// Wave-transposed byte source (DRAGNET_XPOSE resident staging): the
// pool is re-laid out so granule g of the record owned by lane l of a
// wave sits at wave_base + g*(64*GRAN) + l*GRAN.  A wave's window
// refills for granule g then touch 64 *consecutive* GRAN-byte blocks
// — coalesced, several times fewer cache lines than the linear
// layout's 64 scattered records (the SQ_WAIT-bound gather profile in
// profiles/).  Positions are RECORD-RELATIVE (start=0); spans
// captured from this source are decoded through the same XBytesT.
template <int LG>  // log2 granule bytes (5/6/7 = 32/64/128B)
struct XBytesT {
  static constexpr uint32_t GRAN = 1u << LG;
  static constexpr uint32_t STRIDE = 64u << LG;  // wave granule row
  const uint8_t* base;  // pool + wave_base + lane*GRAN
  DN_HD_INLINE uint8_t at(uint32_t p) const {
    return base[(size_t)(p >> LG) * STRIDE + (p & (GRAN - 1u))];
  }
  DN_HD_INLINE uint64_t load8(uint32_t p) const {
    uint32_t o = p & (GRAN - 1u);
    const uint8_t* gp = base + (size_t)(p >> LG) * STRIDE;
    uint64_t w;
    if (o <= GRAN - 8) {
      __builtin_memcpy(&w, gp + o, 8);
      return w;
    }
    uint64_t lo, hi;
    __builtin_memcpy(&lo, gp + GRAN - 8, 8);
    __builtin_memcpy(&hi, gp + STRIDE, 8);
    uint32_t sh = (o - (GRAN - 8)) * 8;  // 8..56
    return (lo >> sh) | (hi << (64 - sh));
  }
};

template <class BS>
struct CursorT {
  BS B;
  uint32_t pos, end;
  uint64_t win, win2;  // 16 record bytes at [wbase, wbase+16)
  uint32_t wbase;

  DN_HD_INLINE void init(BS b, uint32_t p, uint32_t e) {
    B = b; pos = p; end = e;
    wbase = p;
    win = B.load8(p);
    win2 = B.load8(p + 8);
  }
  // NOTE: refill may read up to 15 bytes past `end`; the host pads
  // every chunk with >= 8 newline bytes and 16B alignment slack
  // (engine/chunks.py _pad()).
  DN_HD_INLINE uint8_t byte_at(uint32_t p) {
    uint32_t d = p - wbase;
    if (d >= 16u) {
      wbase = p;
      win = B.load8(p);
      win2 = B.load8(p + 8);
      d = 0;
    }
    uint64_t w = d < 8u ? win : win2;
    return (uint8_t)(w >> (8u * (d & 7u)));
  }
  DN_HD_INLINE bool eof() const { return pos >= end; }
  DN_HD_INLINE uint8_t peek() { return byte_at(pos); }
  DN_HD_INLINE uint8_t next() { return byte_at(pos++); }
  // 8 bytes starting at p, served from the 16B register window
  // (refills like byte_at; may read window slack past `end` — host
  // padding guarantees it)
  DN_HD_INLINE uint64_t word_at(uint32_t p) {
    uint32_t d = p - wbase;
    if (d > 8u) {
      wbase = p;
      win = B.load8(p);
      win2 = B.load8(p + 8);
      d = 0;
    }
    if (d == 0) return win;
    if (d == 8u) return win2;  // a 64-bit shift by 64 would be UB
    return (win >> (8u * d)) | (win2 << (64u - 8u * d));
  }
  DN_HD_INLINE void skip_ws() {
    while (pos < end) {
      uint8_t b = byte_at(pos);
      if (b == ' ' || b == '\t' || b == '\r' || b == '\n') pos++;
      else break;
    }
  }
};

// high bit set per zero byte; the FIRST flagged byte is always a true
// zero (false positives only occur above a real zero byte)
DN_HD_INLINE uint64_t hz8(uint64_t v) {
  return (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;
}

// bytes that end a bulk string run: '"', '\\', or a control char
DN_HD_INLINE uint64_t str_special_mask(uint64_t w) {
  uint64_t q = hz8(w ^ 0x2222222222222222ull);
  uint64_t b = hz8(w ^ 0x5C5C5C5C5C5C5C5Cull);
  uint64_t c = hz8(w & 0xE0E0E0E0E0E0E0E0ull);
  return q | b | c;
}

// Scan a JSON string body (cursor after the opening quote): SWAR over
// 8-byte windows, per-byte only at escapes.  Sets raw off/len.
template <class BS>
DN_HD_INLINE bool scan_string_fast(CursorT<BS>& c, uint32_t& off_out,
                                   uint32_t& len_out) {
  uint32_t off = c.pos, p = c.pos, end = c.end;
  while (true) {
    while (p + 8 <= end) {
      uint64_t w = c.B.load8(p);
      uint64_t m = str_special_mask(w);
      if (m == 0) { p += 8; continue; }
      p += ((uint32_t)DN_FFSLL((unsigned long long)m) - 1) >> 3;
      break;
    }
    if (p >= end) return false;
    uint8_t b = c.B.at(p);
    if (b == '"') {
      off_out = off; len_out = p - off; c.pos = p + 1;
      return true;
    }
    if (b == '\\') {
      p++;
      if (p >= end) return false;
      uint8_t e = c.B.at(p); p++;
      if (e == 'u') {
        if (p + 4 > end) return false;
        for (int k = 0; k < 4; k++) {
          uint8_t x = c.B.at(p + k);
          bool hex = (x >= '0' && x <= '9') || (x >= 'a' && x <= 'f') ||
                     (x >= 'A' && x <= 'F');
          if (!hex) return false;
        }
        p += 4;
      } else if (!(e == '"' || e == '\\' || e == '/' || e == 'b' ||
                   e == 'f' || e == 'n' || e == 'r' || e == 't')) {
        return false;
      }
      continue;
    }
    if (b < 0x20) return false;  // raw control char
    p++;  // SWAR tail (< 8 bytes left): plain byte, keep walking
  }
}

// Streamed signature chaining (mirrors plan.py comp_into): key bytes
// fold DIRECTLY into the path signature as zero-padded 8-byte words —
// one mix per word plus one length-finalization mix, with the words
// hashed inline during the key scan (no re-load pass, one mix fewer
// per component than the hash-then-chain scheme).
constexpr uint64_t SIG_LENK = 0xFF51AFD7ED558CCDull;

// 5-op bijective mix for the SIGNATURE chain only (dict/table hashing
// keeps the full murmur finalizer): xor-fold, odd-multiply, xor-fold.
// Bijective (hi recoverable, then lo), and the final fold feeds the
// bloom's low 6 bits from the whole state.  plan.py _sig_mix mirrors.
DN_HD_INLINE uint64_t sig_mix(uint64_t x) {
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  return x ^ (x >> 32);
}
// fields-root literal-dotted marker (plan.py SIG_LIT_MARK)
constexpr uint64_t SIG_LIT_MARK = 0xC2B2AE3D27D4EB4Full;

DN_HD_INLINE uint64_t sig_word(uint64_t sig, uint64_t w) {
  return sig_mix(sig ^ w);
}
DN_HD_INLINE uint64_t sig_fin(uint64_t sig, uint32_t len) {
  return sig_mix(sig ^ ((uint64_t)len * SIG_LENK));
}

// Fold the unhashed remainder [hashed, term) of the current component
// (8-byte strides stay aligned to comp_s), then finalize with the
// component length.
template <class BS>
DN_HD_INLINE uint64_t sig_comp_finish(BS B, uint64_t sig, uint32_t hashed,
                                      uint32_t comp_s, uint32_t term) {
  uint32_t k = hashed;
  while (k < term) {
    uint64_t w = B.load8(k);
    uint32_t rem = term - k;
    if (rem < 8) w &= (~0ull) >> (8 * (8 - rem));
    sig = sig_mix(sig ^ w);
    k += 8;
  }
  return sig_fin(sig, term - comp_s);
}

// Scan a KEY (cursor after the opening quote): SWAR windows to the
// next quote/dot/escape/control; chains component hashes into the
// path signature (mirrors plan.path_sig).  dot_splits is the mode
// switch: json-skinner reads point.fields[name] literally with
// dotted column names, so in-key '.' chains components there; json
// mode hashes the key as ONE component (dots are plain bytes), so a
// nested path matches its chained primary sig while a TOP-LEVEL
// literal "a.b" key matches the field's companion sig (the whole
// literal name as one component — plan.py lit_sig), which the
// aggregation readout consults first (points.lookup is literal-first)
// and krill pluck / synthetic sources never see.  Keys nested UNDER a
// literal dotted key chain from the literal sig and match nothing.
// Escaped keys are validated but get a sentinel signature.
template <class BS>
DN_HD_INLINE int scan_key_sig(CursorT<BS>& c, uint64_t parent,
                              uint64_t& sig_out, bool dot_splits) {
  uint32_t p = c.pos, end = c.end;
  uint32_t comp_s = p;   // current component start
  uint32_t hashed = p;   // bytes below this are already folded in
  uint64_t sig = parent;
  bool saw_dot = false;
  while (true) {
    while (p + 8 <= end) {
      uint64_t w = c.B.load8(p);
      // json mode hashes dots as plain component bytes, so they must
      // NOT break the window (alignment from comp_s is load-bearing)
      uint64_t m = str_special_mask(w);
      if (dot_splits) m |= hz8(w ^ 0x2E2E2E2E2E2E2E2Eull);
      if (m == 0) {
        if (p == hashed) {  // full window: fold inline
          sig = sig_word(sig, w);
          hashed = p + 8;
        }
        p += 8;
        continue;
      }
      p += ((uint32_t)DN_FFSLL((unsigned long long)m) - 1) >> 3;
      break;
    }
    if (p >= end) return 0;
    uint8_t b = c.B.at(p);
    if (b == '"') {
      sig_out = sig_comp_finish(c.B, sig, hashed, comp_s, p);
      c.pos = p + 1;
      return saw_dot ? 2 : 1;  // 2 = key contained a split dot
    }
    if (b == '.') {
      if (dot_splits) {
        sig = sig_comp_finish(c.B, sig, hashed, comp_s, p);
        comp_s = p + 1;
        hashed = p + 1;
        saw_dot = true;
      }
      p++;
      continue;
    }
    if (b == '\\') {
      c.pos = p;
      uint32_t o, l;
      if (!scan_string_fast(c, o, l)) return 0;
      sig_out = 0x1ull;  // never matches a compiled signature
      return 1;
    }
    if (b < 0x20) return 0;
    p++;  // near-record-end tail: plain byte
  }
}

// -------------------------------------------------------------------
// JSON number parsing (strict JSON grammar; value as double)

// mant * 10^ex, correctly rounded (dec2dbl.h: exact one-rounding fast
// path, Eisel-Lemire out of line behind it).  Shared by the JSON
// number parser and js_to_number.
DN_HD_INLINE double scale10(uint64_t mant, long ex) {
  return dn_dec2dbl(mant, ex, P10_TBL);
}

struct NumOut { double v; bool ok; };

// SWAR digit-run scan: consume the run of ASCII digits at c.pos,
// folding into mant (10^ndig positional, capped at 19 significant
// digits with the overflow counted in extra).  Leading zeros (mant
// still 0) are not significant: they leave ndig alone, so the cap
// never eats real digits of 0.000...0123.  Returns the number of
// digits consumed.  The classifier flags the FIRST non-digit exactly
// (carries out of a non-digit byte only corrupt LATER bytes, which
// are beyond the stop point by construction).
template <class BS>
DN_HD_INLINE int scan_digit_run(CursorT<BS>& c, uint64_t& mant, int& ndig,
                                int& extra) {
  int total = 0;
  while (!c.eof()) {
    uint64_t w = c.word_at(c.pos);
    uint64_t t = w ^ 0x3030303030303030ull;
    uint64_t nd = ((t + 0x7676767676767676ull) | t)
                  & 0x8080808080808080ull;
    uint32_t n = nd ? (((uint32_t)DN_FFSLL((long long)nd) - 1) >> 3)
                    : 8u;
    uint32_t avail = c.end - c.pos;
    if (n > avail) n = avail;
    if (n == 0) break;
    if (n == 8 && mant != 0 && ndig + 8 <= 19) {
      // 3-multiply 8-digit fold (first digit in the LOW byte = most
      // significant)
      uint64_t pairs = (t * ((10ull << 8) + 1)) >> 8;
      uint64_t quads = ((pairs & 0x00FF00FF00FF00FFull)
                        * ((100ull << 16) + 1)) >> 16;
      uint64_t v8 = ((quads & 0x0000FFFF0000FFFFull)
                     * ((10000ull << 32) + 1)) >> 32;
      mant = mant * 100000000ull + (uint32_t)v8;
      ndig += 8;
    } else {
      for (uint32_t k = 0; k < n; k++) {
        uint32_t d = (uint32_t)(w >> (8 * k)) & 0xFF;
        if (ndig < 19) {
          mant = mant * 10u + (d - '0');
          ndig += (mant != 0);
        } else extra++;
      }
    }
    c.pos += n;
    total += (int)n;
    if (n < 8) break;
  }
  return total;
}

template <class BS>
DN_HD_INLINE NumOut parse_json_number(CursorT<BS>& c) {
  NumOut out; out.ok = false; out.v = 0.0;
  bool neg = false;
  if (!c.eof() && c.peek() == '-') { neg = true; c.pos++; }
  if (c.eof()) return out;
  // integer part: 0 | [1-9][0-9]*
  uint64_t mant = 0;
  int ndig = 0, extra_exp = 0;
  uint8_t b = c.peek();
  if (b == '0') {
    c.pos++;
    if (!c.eof()) { uint8_t nb = c.peek(); if (nb >= '0' && nb <= '9') return out; }
  } else if (b >= '1' && b <= '9') {
    scan_digit_run(c, mant, ndig, extra_exp);
  } else {
    return out;
  }
  // fraction
  if (!c.eof() && c.peek() == '.') {
    c.pos++;
    int fdig = 0, fex = 0;
    fdig = scan_digit_run(c, mant, ndig, fex);
    // every fraction digit folded into mant shifts the exponent
    // (leading zeros included); truncated ones shift nothing
    extra_exp -= (fdig - fex);
    if (fdig == 0) return out;
  }
  // exponent
  int esign = 1; long e10 = 0;
  if (!c.eof() && (c.peek() == 'e' || c.peek() == 'E')) {
    c.pos++;
    if (!c.eof() && (c.peek() == '+' || c.peek() == '-')) {
      if (c.peek() == '-') esign = -1;
      c.pos++;
    }
    int edig = 0;
    while (!c.eof()) {
      uint8_t d = c.peek();
      if (d < '0' || d > '9') break;
      c.pos++;
      if (e10 < 100000) e10 = e10 * 10 + (d - '0');
      edig++;
    }
    if (edig == 0) return out;
  }
  long exp10 = esign * e10 + extra_exp;
  double v = scale10(mant, exp10);
  out.v = neg ? -v : v;
  out.ok = true;
  return out;
}

// Whitespace trim of a RAW (still JSON-escaped) string span, matching
// what the oracle trims after unescaping.  Raw bytes cover the plain
// space; every other ASCII whitespace can only appear in a JSON string
// as an escape (\t \n \r \f or \u00XX), which the cold helper below
// peels off both ends.  py_ws selects Python str.strip()'s ASCII set
// (U+001C..U+001F and U+0085, no U+FEFF: jsdate.parse_ms) over JS
// trim's (krill.to_number).  Non-ASCII whitespace spelled as raw
// UTF-8 bytes is not trimmed (COMPONENTS.md).
DN_HD_INLINE bool raw_ws(uint8_t b) {
  return b == ' ' || b == '\t' || b == '\r' || b == '\n' || b == '\f' ||
         b == '\v';
}

// length (2 or 6) of a whitespace escape starting at off+p, else 0
template <class BS>
DN_HD_INLINE uint32_t ws_escape_at(BS BV, uint32_t off, uint32_t p, uint32_t j,
                                   bool py_ws) {
  if (p + 2 > j || BV.at(off + p) != '\\') return 0;
  uint8_t e = BV.at(off + p + 1);
  if (e == 't' || e == 'n' || e == 'r' || e == 'f') return 2;
  if (e != 'u' || p + 6 > j) return 0;
  uint32_t cp = 0;
  for (int k = 2; k < 6; k++) {
    uint8_t x = BV.at(off + p + k);
    uint32_t d;
    if (x >= '0' && x <= '9') d = x - '0';
    else if (x >= 'a' && x <= 'f') d = x - 'a' + 10;
    else if (x >= 'A' && x <= 'F') d = x - 'A' + 10;
    else return 0;
    cp = cp * 16 + d;
  }
  bool ws = (cp >= 0x09 && cp <= 0x0D) || cp == 0x20 || cp == 0xA0 ||
            cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) ||
            cp == 0x2028 || cp == 0x2029 || cp == 0x202F ||
            cp == 0x205F || cp == 0x3000 ||
            (py_ws ? ((cp >= 0x1C && cp <= 0x1F) || cp == 0x85)
                   : cp == 0xFEFF);
  return ws ? 6u : 0u;
}

// (inlined, values in and packed i | j << 32 out: measured, an
// out-of-line copy costs every scan kernel 8+ bytes of scratch for
// its callee-saved registers, and reference parameters 24 more)
template <class BS>
DN_HD_INLINE uint64_t trim_escaped_ws(BS BV, uint32_t off, uint32_t i,
                                      uint32_t j, bool py_ws) {
  while (i < j) {
    if (raw_ws(BV.at(off + i))) { i++; continue; }
    uint32_t n = ws_escape_at(BV, off, i, j, py_ws);
    if (n == 0) break;
    i += n;
  }
  while (j > i) {
    if (raw_ws(BV.at(off + j - 1))) { j--; continue; }
    uint32_t n = 0;
    if (j - i >= 2 && ws_escape_at(BV, off, j - 2, j, py_ws) == 2) n = 2;
    else if (j - i >= 6 && ws_escape_at(BV, off, j - 6, j, py_ws) == 6) n = 6;
    if (n == 0) break;
    // the backslash starts an escape only if an even number of
    // backslashes precede it (else it is the tail of an escaped "\\")
    uint32_t run = 0;
    for (uint32_t k = j - n; k > i && BV.at(off + k - 1) == '\\'; k--) run++;
    if (run & 1) break;
    j -= n;
  }
  return (uint64_t)i | ((uint64_t)j << 32);
}

// trim [i, j) of the span at off: raw bytes first, escapes only when a
// backslash sits where an end-of-span escape would start
template <class BS>
DN_HD_INLINE void trim_ws(BS BV, uint32_t off, uint32_t& i, uint32_t& j,
                          bool py_ws) {
  while (i < j && raw_ws(BV.at(off + i))) i++;
  while (j > i && raw_ws(BV.at(off + j - 1))) j--;
  if (j - i >= 2 &&
      (BV.at(off + i) == '\\' || BV.at(off + j - 2) == '\\' ||
       (j - i >= 6 && BV.at(off + j - 6) == '\\')))
  {
    uint64_t ij = trim_escaped_ws(BV, off, i, j, py_ws);
    i = (uint32_t)ij;
    j = (uint32_t)(ij >> 32);
  }
}

// JavaScript ToNumber for record strings (mirrors krill.to_number):
// trim ws; "" -> 0; decimal/hex/Infinity; else NaN.
template <class BS>
DN_HD_INLINE double js_to_number(BS BV, uint32_t off, uint32_t len) {
  uint32_t i = 0, j = len;
  trim_ws(BV, off, i, j, false);
  if (i == j) return 0.0;
  const double NAN_ = __builtin_nan("");
  uint32_t p = i;
  bool neg = false;
  if (BV.at(off+p) == '+' || BV.at(off+p) == '-') { neg = BV.at(off+p) == '-'; p++; }
  if (p == j) return NAN_;
  // Infinity
  if (BV.at(off+p) == 'I') {
    const char* inf = "Infinity";
    if (j - p == 8) {
      for (int k = 0; k < 8; k++) if (BV.at(off+p+k) != (uint8_t)inf[k]) return NAN_;
      return neg ? -__builtin_inf() : __builtin_inf();
    }
    return NAN_;
  }
  // hex (unsigned form only: JS Number() rejects '-0x10'/'+0x10')
  if (j - p > 2 && BV.at(off+p) == '0' &&
      (BV.at(off+p+1) == 'x' || BV.at(off+p+1) == 'X')) {
    if (p != i) return NAN_;
    // accumulate 64 bits exactly; further digits only widen the value
    // (sticky bit keeps the rounding of the top 64 bits honest)
    uint64_t v = 0; int shift4 = 0; bool sticky = false;
    for (uint32_t k = p + 2; k < j; k++) {
      uint8_t b = BV.at(off+k);
      uint32_t d;
      if (b >= '0' && b <= '9') d = b - '0';
      else if (b >= 'a' && b <= 'f') d = b - 'a' + 10;
      else if (b >= 'A' && b <= 'F') d = b - 'A' + 10;
      else return NAN_;
      if (v >> 60) { shift4++; sticky |= (d != 0); }
      else v = v * 16u + d;
    }
    if (sticky) v |= 1;  // v >= 2^60 here: bit 0 is below the round bit
    double r = (double)v;
    for (; shift4 > 0 && r < __builtin_inf(); shift4--) r *= 16.0;
    return r;
  }
  // decimal (JS grammar: digits [. digits] [e[+-]digits], '.5' and '5.' OK)
  uint64_t mant = 0; int ndig = 0, extra = 0; bool any = false;
  while (p < j && BV.at(off+p) >= '0' && BV.at(off+p) <= '9') {
    if (ndig < 19) { mant = mant * 10 + (BV.at(off+p)-'0'); ndig += (mant != 0); }
    else extra++;
    p++; any = true;
  }
  if (p < j && BV.at(off+p) == '.') {
    p++;
    while (p < j && BV.at(off+p) >= '0' && BV.at(off+p) <= '9') {
      if (ndig < 19) { mant = mant * 10 + (BV.at(off+p)-'0'); ndig += (mant != 0); extra--; }
      p++; any = true;
    }
  }
  if (!any) return NAN_;
  long e10 = 0; int es = 1;
  if (p < j && (BV.at(off+p) == 'e' || BV.at(off+p) == 'E')) {
    p++;
    if (p < j && (BV.at(off+p) == '+' || BV.at(off+p) == '-')) {
      if (BV.at(off+p) == '-') es = -1;
      p++;
    }
    if (p >= j) return NAN_;
    while (p < j && BV.at(off+p) >= '0' && BV.at(off+p) <= '9') {
      if (e10 < 100000) e10 = e10 * 10 + (BV.at(off+p)-'0');
      p++;
    }
  }
  if (p != j) return NAN_;
  long ex = es * e10 + extra;
  double v = scale10(mant, ex);
  return neg ? -v : v;
}

// -------------------------------------------------------------------
// bucket ordinals (K4), shared by the scan and columnar kernels.  The
// ordinal stays a DOUBLE: floor(v/step) of 1e300 is far outside any
// integer type, and the oracle's int(floor(v/step)) is exactly that
// double.  Ordinals inside +-ORD_BIAS pack into the key code; the rest
// are interned as numbers (the host decodes both the same way).

DN_HD_INLINE bool finite_num(double v) {
  return __builtin_fabs(v) < __builtin_inf();  // false for NaN too
}

DN_HD_INLINE double bucket_ordinal(int kind, double num, double step) {
  if (kind == BUCKET_P2) {
    if (!(num >= 1.0)) return 0.0;
    // floor(log2(v)) + 1 via exponent field
    uint64_t bits = DN_DOUBLE_AS_LL(num);
    return (double)((int)((bits >> 52) & 0x7FF) - 1023 + 1);
  }
  return __builtin_floor(num / step);
}

DN_HD_INLINE bool ord_is_small(double ordf) {
  return ordf >= -(double)ORD_BIAS && ordf < (double)ORD_BIAS;
}

// -------------------------------------------------------------------
// ISO-8601 date parse (mirrors dragnet_amd/jsdate.parse_ms exactly)

DN_HD_INLINE long days_from_civil(long y, long m, long d) {
  y -= m <= 2;
  long era = (y >= 0 ? y : y - 399) / 400;
  long yoe = y - era * 400;
  long doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  long doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

struct DateOut { long long ms; bool ok; };

DN_HD_INLINE bool is_leap(long y) {
  return (y % 4 == 0) && ((y % 100 != 0) || (y % 400 == 0));
}

template <class BS>
DN_HD_INLINE DateOut parse_iso_ms(BS BV, uint32_t off, uint32_t len) {
  DateOut out; out.ok = false; out.ms = 0;
  // trim
  uint32_t i = 0, j = len;
  trim_ws(BV, off, i, j, true);
  uint32_t p = i;
  auto digits = [&](int n, long& v) -> bool {
    v = 0;
    for (int k = 0; k < n; k++) {
      if (p >= j) return false;
      uint8_t b = BV.at(off+p);
      if (b < '0' || b > '9') return false;
      v = v * 10 + (b - '0');
      p++;
    }
    return true;
  };
  long year, month = 1, day = 1, hh = 0, mm = 0, ss = 0, ms = 0;
  if (!digits(4, year)) return out;
  bool have_time = false;
  if (p < j && BV.at(off+p) == '-') {
    p++;
    if (!digits(2, month)) return out;
    if (p < j && BV.at(off+p) == '-') {
      p++;
      if (!digits(2, day)) return out;
      if (p < j && (BV.at(off+p) == 'T' || BV.at(off+p) == ' ')) {
        p++;
        if (!digits(2, hh)) return out;
        if (p >= j || BV.at(off+p) != ':') return out;
        p++;
        if (!digits(2, mm)) return out;
        have_time = true;
        if (p < j && BV.at(off+p) == ':') {
          p++;
          if (!digits(2, ss)) return out;
          if (p < j && BV.at(off+p) == '.') {
            p++;
            int nd = 0; long frac = 0;
            while (p < j && BV.at(off+p) >= '0' && BV.at(off+p) <= '9' && nd < 9) {
              if (nd < 3) frac = frac * 10 + (BV.at(off+p) - '0');
              nd++; p++;
            }
            if (nd == 0) return out;
            while (nd < 3) { frac *= 10; nd++; }
            ms = frac;
          }
        }
      }
    }
  }
  long tz_off_min = 0;
  if (have_time && p < j) {
    uint8_t b = BV.at(off+p);
    if (b == 'Z') { p++; }
    else if (b == '+' || b == '-') {
      int sign = (b == '+') ? 1 : -1;
      p++;
      long th, tm;
      if (!digits(2, th)) return out;
      if (p < j && BV.at(off+p) == ':') p++;
      if (!digits(2, tm)) return out;
      tz_off_min = sign * (th * 60 + tm);
    }
  }
  if (p != j) return out;
  if (month < 1 || month > 12) return out;
  long dim = DIM_TBL[month-1] + ((month == 2 && is_leap(year)) ? 1 : 0);
  if (day < 1 || day > dim) return out;
  if (hh > 24 || mm > 59 || ss > 59) return out;
  // V8 accepts hour 24 only as exactly 24:00:00.000
  if (hh == 24 && (mm || ss || ms)) return out;
  long days = days_from_civil(year, month, day);
  long long total = ((days * 24 + hh) * 60 + mm) * 60 + ss;
  out.ms = total * 1000 + ms - (long long)tz_off_min * 60000;
  out.ok = true;
  return out;
}

// -------------------------------------------------------------------
// decoded-string compare (cold path: only spans containing '\\').
// JSON-unescapes the field span on the fly and 3-way-compares it
// against the constant's raw (unescaped) UTF-8 bytes, mirroring the
// host-side decode (gpu._decode_json_string) that group keys get.
// Decoded bytes are packed into a u32 (no local array) so the hot
// kernel stays scratch-free.

DN_HD_INLINE int hexval4(uint8_t x) {
  if (x >= '0' && x <= '9') return x - '0';
  if (x >= 'a' && x <= 'f') return x - 'a' + 10;
  if (x >= 'A' && x <= 'F') return x - 'A' + 10;
  return -1;
}

// Decode one logical unit at i (a raw byte or a full escape, \uXXXX
// surrogate pairs included): packs 1-4 UTF-8 bytes little-endian into
// out, advances i, returns the byte count (0 = bad escape — cannot
// happen for spans the tokenizer accepted; defensive).
template <class BS>
DN_HD_INLINE int unesc_next(BS d, uint32_t fo, uint32_t fl,
                            uint32_t& i, uint32_t& out) {
  uint8_t b = d.at(fo + i);
  if (b != '\\') { i++; out = b; return 1; }
  if (i + 2 > fl) return 0;
  uint8_t e = d.at(fo + i + 1);
  i += 2;
  switch (e) {
    case '"':  out = '"';  return 1;
    case '\\': out = '\\'; return 1;
    case '/':  out = '/';  return 1;
    case 'b':  out = 8;    return 1;
    case 'f':  out = 12;   return 1;
    case 'n':  out = 10;   return 1;
    case 'r':  out = 13;   return 1;
    case 't':  out = 9;    return 1;
    case 'u':  break;
    default:   return 0;
  }
  if (i + 4 > fl) return 0;
  uint32_t cp = 0;
  for (int k = 0; k < 4; k++) {
    int h = hexval4(d.at(fo + i + k));
    if (h < 0) return 0;
    cp = cp * 16 + (uint32_t)h;
  }
  i += 4;
  if (cp >= 0xD800 && cp < 0xDC00 && i + 6 <= fl &&
      d.at(fo + i) == '\\' && d.at(fo + i + 1) == 'u') {
    uint32_t lo = 0;
    bool ok = true;
    for (int k = 0; k < 4; k++) {
      int h = hexval4(d.at(fo + i + 2 + k));
      if (h < 0) { ok = false; break; }
      lo = lo * 16 + (uint32_t)h;
    }
    if (ok && lo >= 0xDC00 && lo < 0xE000) {
      cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
      i += 6;
    }
  }
  if (cp < 0x80) { out = cp; return 1; }
  if (cp < 0x800) {
    out = (0xC0 | (cp >> 6)) | ((0x80u | (cp & 63)) << 8);
    return 2;
  }
  if (cp < 0x10000) {
    out = (0xE0 | (cp >> 12)) | ((0x80u | ((cp >> 6) & 63)) << 8)
          | ((0x80u | (cp & 63)) << 16);
    return 3;
  }
  out = (0xF0 | (cp >> 18)) | ((0x80u | ((cp >> 12) & 63)) << 8)
        | ((0x80u | ((cp >> 6) & 63)) << 16)
        | ((0x80u | (cp & 63)) << 24);
  return 4;
}

// 3-way compare of the DECODED field span vs const bytes; -2 on bad
// escape (defensive — the tokenizer already rejected those records).
template <class BS>
DN_HD_INLINE int unesc_cmp(BS d, uint32_t fo, uint32_t fl,
                           const uint8_t* cb, uint32_t cl) {
  uint32_t i = 0, j = 0;
  while (i < fl) {
    uint32_t pack;
    int n = unesc_next(d, fo, fl, i, pack);
    if (n == 0) return -2;
    for (int k = 0; k < n; k++) {
      uint8_t a = (uint8_t)(pack >> (8 * k));
      if (j >= cl) return 1;  // field longer than const
      uint8_t b = cb[j++];
      if (a != b) return a < b ? -1 : 1;
    }
  }
  return (j == cl) ? 0 : -1;
}

template <class BS>
DN_HD_INLINE bool span_has_backslash(BS d, uint32_t fo, uint32_t fl) {
  for (uint32_t k = 0; k < fl; k++)
    if (d.at(fo + k) == '\\') return true;
  return false;
}

}  // namespace dn
