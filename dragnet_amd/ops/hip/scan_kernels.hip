// dragnet_amd MI355X scan engine — fused CDNA4 kernel.
//
// One kernel pass implements the reference's entire per-record hot path
// (reference lib/stream-scan.js:40-94 pipeline):
// NDJSON tokenize + dotted-path field extraction (K1), krill predicate
// bytecode (K2), ISO-8601 date parse (K3), p2/linear bucketize (K4),
// string/number dictionary interning, and multi-metric hash aggregation
// (K5/K6) — one thread per record, grid-stride, with an LDS combining
// cache in front of the global tables so HBM atomics scale with the
// number of distinct keys per block, not with record count.
//
// Cross-workgroup table publication uses relaxed agent-scope atomic
// stores (write-through to the coherence point) with a vmcnt drain
// before the READY flag — the placement-independent protocol of the
// CDNA4 programming guide (§6 Guideline 16, form R1) — so no acquire
// fences (L1 invalidates) appear on the hot path.

#include "common.h"
#include <hip/hip_runtime.h>
#include "dec2dbl.h"

namespace dn {

#define DEV __device__ __forceinline__

constexpr int BLOCK = 256;
constexpr int SIG_DEPTH = 6;      // max dotted-path components
constexpr int LDS_CACHE = 128;    // per-block aggregation cache slots
// (halved from 256 in r2: the 7 KB buys a whole extra block of
// occupancy, which outweighs extra cache-miss fallthrough; misses
// go to the dense partial row / global table either way)

// -------------------------------------------------------------------
// small utilities

DEV uint64_t fnv1a_byte(uint64_t h, uint8_t b) {
  return (h ^ (uint64_t)b) * 0x100000001B3ull;
}
constexpr uint64_t FNV_OFFSET = 0xCBF29CE484222325ull;

__device__ __constant__ double P10_TBL[23] = {
  1e0,1e1,1e2,1e3,1e4,1e5,1e6,1e7,1e8,1e9,1e10,1e11,1e12,1e13,1e14,
  1e15,1e16,1e17,1e18,1e19,1e20,1e21,1e22};
__device__ __constant__ int DIM_TBL[12] = {
  31,28,31,30,31,30,31,31,30,31,30,31};

DEV uint64_t mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33; return x;
}

// Register-resident small "arrays": named scalar members with select
// chains, so dynamic indexing stays in VGPRs.  (A local ARRAY — even
// one indexed through an unrolled select chain — gets re-canonicalized
// by LLVM into scratch = HBM-backed private memory; measured as the
// scan kernel's dominant stall.)
#define DN_REGSEL6(T, NAME)                                            \
  struct NAME {                                                        \
    T a0, a1, a2, a3, a4, a5;                                          \
    DEV T get(int i) const {                                           \
      T r = a0;                                                        \
      r = (i == 1) ? a1 : r; r = (i == 2) ? a2 : r;                    \
      r = (i == 3) ? a3 : r; r = (i == 4) ? a4 : r;                    \
      r = (i == 5) ? a5 : r; return r;                                 \
    }                                                                  \
    DEV void set(int i, T x) {                                         \
      a0 = (i == 0) ? x : a0; a1 = (i == 1) ? x : a1;                  \
      a2 = (i == 2) ? x : a2; a3 = (i == 3) ? x : a3;                  \
      a4 = (i == 4) ? x : a4; a5 = (i == 5) ? x : a5;                  \
    }                                                                  \
  };
#define DN_REGSEL8(T, NAME)                                            \
  struct NAME {                                                        \
    T a0, a1, a2, a3, a4, a5, a6, a7;                                  \
    DEV T get(int i) const {                                           \
      T r = a0;                                                        \
      r = (i == 1) ? a1 : r; r = (i == 2) ? a2 : r;                    \
      r = (i == 3) ? a3 : r; r = (i == 4) ? a4 : r;                    \
      r = (i == 5) ? a5 : r; r = (i == 6) ? a6 : r;                    \
      r = (i == 7) ? a7 : r; return r;                                 \
    }                                                                  \
    DEV void set(int i, T x) {                                         \
      a0 = (i == 0) ? x : a0; a1 = (i == 1) ? x : a1;                  \
      a2 = (i == 2) ? x : a2; a3 = (i == 3) ? x : a3;                  \
      a4 = (i == 4) ? x : a4; a5 = (i == 5) ? x : a5;                  \
      a6 = (i == 6) ? x : a6; a7 = (i == 7) ? x : a7;                  \
    }                                                                  \
  };
DN_REGSEL6(uint64_t, Sig6)
DN_REGSEL8(uint64_t, U64x8)
DN_REGSEL8(double, F64x8)
DN_REGSEL8(uint32_t, U32x8)

template <typename T>
DEV T atomic_load_relaxed(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
DEV void atomic_store_relaxed(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV void drain_stores() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
  DEV uint8_t at(uint32_t abs) const { return mem[abs - bias]; }
  DEV const uint8_t* ptr(uint32_t abs) const { return mem + (abs - bias); }
  // 8 little-endian bytes starting at abs (may read 7 past a span;
  // host padding guarantees slack)
  DEV uint64_t load8(uint32_t abs) const {
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
  DEV uint8_t at(uint32_t p) const {
    return base[(size_t)(p >> LG) * STRIDE + (p & (GRAN - 1u))];
  }
  DEV uint64_t load8(uint32_t p) const {
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

  DEV void init(BS b, uint32_t p, uint32_t e) {
    B = b; pos = p; end = e;
    wbase = p;
    win = B.load8(p);
    win2 = B.load8(p + 8);
  }
  // NOTE: refill may read up to 15 bytes past `end`; the host pads
  // every chunk with >= 8 newline bytes and 16B alignment slack
  // (engine/gpu.py _pad()).
  DEV uint8_t byte_at(uint32_t p) {
#ifdef DN_DIRECT_BYTES
    return B.at(p);
#else
    uint32_t d = p - wbase;
    if (d >= 16u) {
      wbase = p;
      win = B.load8(p);
      win2 = B.load8(p + 8);
      d = 0;
    }
    uint64_t w = d < 8u ? win : win2;
    return (uint8_t)(w >> (8u * (d & 7u)));
#endif
  }
  DEV bool eof() const { return pos >= end; }
  DEV uint8_t peek() { return byte_at(pos); }
  DEV uint8_t next() { return byte_at(pos++); }
  // 8 bytes starting at p, served from the 16B register window
  // (refills like byte_at; may read window slack past `end` — host
  // padding guarantees it)
  DEV uint64_t word_at(uint32_t p) {
#ifdef DN_DIRECT_BYTES
    return B.load8(p);
#else
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
#endif
  }
  DEV void skip_ws() {
    while (pos < end) {
      uint8_t b = byte_at(pos);
      if (b == ' ' || b == '\t' || b == '\r' || b == '\n') pos++;
      else break;
    }
  }
};
using Cursor = CursorT<Bytes>;

// high bit set per zero byte; the FIRST flagged byte is always a true
// zero (false positives only occur above a real zero byte)
DEV uint64_t hz8(uint64_t v) {
  return (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;
}

// bytes that end a bulk string run: '"', '\\', or a control char
DEV uint64_t str_special_mask(uint64_t w) {
  uint64_t q = hz8(w ^ 0x2222222222222222ull);
  uint64_t b = hz8(w ^ 0x5C5C5C5C5C5C5C5Cull);
  uint64_t c = hz8(w & 0xE0E0E0E0E0E0E0E0ull);
  return q | b | c;
}

// Scan a JSON string body (cursor after the opening quote): SWAR over
// 8-byte windows, per-byte only at escapes.  Sets raw off/len.
template <class BS>
DEV bool scan_string_fast(CursorT<BS>& c, uint32_t& off_out,
                          uint32_t& len_out) {
  uint32_t off = c.pos, p = c.pos, end = c.end;
  while (true) {
    while (p + 8 <= end) {
      uint64_t w = c.B.load8(p);
      uint64_t m = str_special_mask(w);
      if (m == 0) { p += 8; continue; }
      p += ((uint32_t)__ffsll((unsigned long long)m) - 1) >> 3;
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
DEV inline uint64_t sig_mix(uint64_t x) {
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  return x ^ (x >> 32);
}
// fields-root literal-dotted marker (plan.py SIG_LIT_MARK)
constexpr uint64_t SIG_LIT_MARK = 0xC2B2AE3D27D4EB4Full;

DEV inline uint64_t sig_word(uint64_t sig, uint64_t w) {
  return sig_mix(sig ^ w);
}
DEV inline uint64_t sig_fin(uint64_t sig, uint32_t len) {
  return sig_mix(sig ^ ((uint64_t)len * SIG_LENK));
}

// Fold the unhashed remainder [hashed, term) of the current component
// (8-byte strides stay aligned to comp_s), then finalize with the
// component length.
template <class BS>
DEV uint64_t sig_comp_finish(BS B, uint64_t sig, uint32_t hashed,
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
DEV int scan_key_sig(CursorT<BS>& c, uint64_t parent, uint64_t& sig_out,
                     bool dot_splits) {
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
      p += ((uint32_t)__ffsll((unsigned long long)m) - 1) >> 3;
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
// per-record extracted field values, stored in LDS (SoA, [field][tid])

struct FV {
  // (soff, slen) double as the VALUE bits for T_NUM slots — a slot is
  // either a span (str/obj/arr) or a number, never both, and every
  // get_num consumer is type-gated.  The union halves the per-field
  // LDS footprint (9 B/field/thread), which buys occupancy: LDS is
  // the block-count limiter on this kernel.
  uint8_t* type;   // nf * BLOCK
  uint32_t* soff;  // nf * BLOCK; T_NUM: low 32 bits of the double
  uint32_t* slen;  // nf * BLOCK; T_NUM: high 32 bits
  int tid;
  DEV void set(int f, uint8_t t, uint32_t off, uint32_t len, double n) {
    type[f * BLOCK + tid] = t;
    if (t == T_NUM) {
      uint64_t b = (uint64_t)__double_as_longlong(n);
      soff[f * BLOCK + tid] = (uint32_t)b;
      slen[f * BLOCK + tid] = (uint32_t)(b >> 32);
    } else {
      soff[f * BLOCK + tid] = off;
      slen[f * BLOCK + tid] = len;
    }
  }
  DEV void set_len(int f, uint32_t len) { slen[f * BLOCK + tid] = len; }
  DEV uint8_t  get_type(int f) const { return type[f * BLOCK + tid]; }
  DEV uint32_t get_soff(int f) const { return soff[f * BLOCK + tid]; }
  DEV uint32_t get_slen(int f) const { return slen[f * BLOCK + tid]; }
  DEV double   get_num(int f) const {
    uint64_t b = (uint64_t)soff[f * BLOCK + tid]
               | ((uint64_t)slen[f * BLOCK + tid] << 32);
    return __longlong_as_double((long long)b);
  }
};

// -------------------------------------------------------------------
// JSON number parsing (strict JSON grammar; value as double)

// mant * 10^ex, correctly rounded (dec2dbl.h: exact one-rounding fast
// path, Eisel-Lemire out of line behind it).  Shared by the JSON
// number parser and js_to_number.
DEV double scale10(uint64_t mant, long ex) {
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
DEV int scan_digit_run(CursorT<BS>& c, uint64_t& mant, int& ndig,
                       int& extra) {
  int total = 0;
  while (!c.eof()) {
    uint64_t w = c.word_at(c.pos);
    uint64_t t = w ^ 0x3030303030303030ull;
    uint64_t nd = ((t + 0x7676767676767676ull) | t)
                  & 0x8080808080808080ull;
    uint32_t n = nd ? (((uint32_t)__ffsll((long long)nd) - 1) >> 3)
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
DEV NumOut parse_json_number(CursorT<BS>& c) {
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
DEV bool raw_ws(uint8_t b) {
  return b == ' ' || b == '\t' || b == '\r' || b == '\n' || b == '\f' ||
         b == '\v';
}

// length (2 or 6) of a whitespace escape starting at off+p, else 0
template <class BS>
DEV uint32_t ws_escape_at(BS BV, uint32_t off, uint32_t p, uint32_t j,
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
DEV uint64_t trim_escaped_ws(BS BV, uint32_t off, uint32_t i, uint32_t j,
                         bool py_ws) {
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
DEV void trim_ws(BS BV, uint32_t off, uint32_t& i, uint32_t& j, bool py_ws) {
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
DEV double js_to_number(BS BV, uint32_t off, uint32_t len) {
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

DEV bool finite_num(double v) {
  return __builtin_fabs(v) < __builtin_inf();  // false for NaN too
}

DEV double bucket_ordinal(int kind, double num, double step) {
  if (kind == BUCKET_P2) {
    if (!(num >= 1.0)) return 0.0;
    // floor(log2(v)) + 1 via exponent field
    uint64_t bits = __double_as_longlong(num);
    return (double)((int)((bits >> 52) & 0x7FF) - 1023 + 1);
  }
  return __builtin_floor(num / step);
}

DEV bool ord_is_small(double ordf) {
  return ordf >= -(double)ORD_BIAS && ordf < (double)ORD_BIAS;
}

// -------------------------------------------------------------------
// ISO-8601 date parse (mirrors dragnet_amd/jsdate.parse_ms exactly)

DEV long days_from_civil(long y, long m, long d) {
  y -= m <= 2;
  long era = (y >= 0 ? y : y - 399) / 400;
  long yoe = y - era * 400;
  long doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  long doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

struct DateOut { long long ms; bool ok; };

DEV bool is_leap(long y) {
  return (y % 4 == 0) && ((y % 100 != 0) || (y % 400 == 0));
}

template <class BS>
DEV DateOut parse_iso_ms(BS BV, uint32_t off, uint32_t len) {
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
// JSON record parser (K1): one pass, captures fields by path signature
// (PlanView layout: common.h)

// Parses one record (bytes [start,end)); fills fv (all slots must be
// preinitialized to T_MISSING by the caller).  Returns false on invalid
// JSON.  top_type receives the top-level value type.
template <class BS>
DEV bool parse_record(BS BV, uint32_t start, uint32_t end,
                      const PlanView& P, FV& fv, uint8_t& top_type,
                      uint64_t* sig_lds, bool dot_splits) {
  CursorT<BS> c; c.init(BV, start, end);
  // parent-signature stack in LDS: [depth * BLOCK + tid]
  #define sig_stack_at(d) sig_lds[(d) * BLOCK + (uint32_t)threadIdx.x]

  uint64_t cont_slot = ~0ull;  // 5 bits/depth: captured slot or 31
  uint64_t is_arr_bits = 0;       // bit d: container at depth d is array
  int depth = 0;                  // container depth (0 = at top value)
  int arr_depth = 0;              // number of array containers on stack
  uint64_t cur_sig = 0;           // path sig for the value being parsed
  bool cur_capture = false;       // does cur_sig match a slot?
  int cur_slot = -1;

  c.skip_ws();
  if (c.eof()) return false;

  // match cur sig against the field table
  auto match_slot = [&](uint64_t sig) -> int {
    if (!((P.sig_bloom >> ((uint32_t)sig & 63u)) & 1ull)) return -1;
    for (int f = 0; f < P.nf; f++)
      if (P.field_sigs[f] == sig) return f;
    return -1;
  };

  // scan a JSON string starting AFTER the opening quote; returns false
  // on bad escape/unterminated; sets len (raw bytes), computes fnv
  // parse the key of an object member (cursor at '"'), extending the
  // parent signature via chained component hashes (plan.path_sig)
  auto parse_key = [&](uint64_t parent, bool root, uint64_t& sig_out) -> bool {
    if (c.eof() || c.next() != '"') return false;
    int r = scan_key_sig(c, root ? FNV_OFFSET : parent, sig_out,
                         dot_splits);
    if (r == 0) return false;
    // skinner: a fields-ROOT key containing a dot is a LITERAL dotted
    // key — addressable by the aggregation lookup (literal-first) but
    // invisible to krill pluck; fold the marker so it captures into
    // the companion slot (plan.py SIG_LIT_MARK)
    if (r == 2 && !root && parent == P.fields_parent_sig)
      sig_out = sig_mix(sig_out ^ SIG_LIT_MARK);
    return true;
  };

  // Main loop: parse values iteratively.
  // expect_value: cursor sits at a value; otherwise we're closing
  // containers / consuming separators.
  bool expect_value = true;
  top_type = T_MISSING;

  while (true) {
    if (expect_value) {
      c.skip_ws();
      if (c.eof()) return false;
      uint8_t b = c.peek();
      uint8_t vtype = T_MISSING;
      uint32_t voff = 0, vlen = 0;
      double vnum = 0.0;

      if (b == '{') {
        uint32_t vstart = c.pos;
        c.pos++;
        // capture the object itself (presence + raw span)
        if (cur_capture && arr_depth == 0)
          fv.set(cur_slot, T_OBJ, vstart, 0, 0.0);
        if (depth == 0) top_type = T_OBJ;
        if (depth >= MAX_DEPTH) return false;
        c.skip_ws();
        if (!c.eof() && c.peek() == '}') {
          c.pos++;
          vtype = T_OBJ;  // empty object: treat as closed value
          voff = vstart; vlen = c.pos - vstart;
          // fall through to "after value"
        } else {
          // push object frame
          if (depth < SLOT_DEPTH) {
            uint64_t cs = (cur_capture && arr_depth == 0)
                              ? (uint64_t)cur_slot : 31ull;
            cont_slot = (cont_slot & ~(31ull << (5 * depth)))
                        | (cs << (5 * depth));
          }
          if (depth < SIG_DEPTH) sig_stack_at(depth) = cur_sig;
          is_arr_bits &= ~(1ull << depth);
          depth++;
          // parse first key
          uint64_t ksig;
          if (!parse_key(cur_sig, depth == 1, ksig)) return false;
          c.skip_ws();
          if (c.eof() || c.next() != ':') return false;
          cur_sig = ksig;
          cur_slot = (arr_depth == 0) ? match_slot(ksig) : -1;
          cur_capture = cur_slot >= 0;
          continue;  // parse the member value
        }
      } else if (b == '[') {
        uint32_t vstart = c.pos;
        c.pos++;
        if (cur_capture && arr_depth == 0)
          fv.set(cur_slot, T_ARR, vstart, 0, 0.0);
        if (depth == 0) top_type = T_ARR;
        if (depth >= MAX_DEPTH) return false;
        c.skip_ws();
        if (!c.eof() && c.peek() == ']') {
          c.pos++;
          vtype = T_ARR;
          voff = vstart; vlen = c.pos - vstart;
        } else {
          if (depth < SLOT_DEPTH) {
            uint64_t cs = (cur_capture && arr_depth == 0)
                              ? (uint64_t)cur_slot : 31ull;
            cont_slot = (cont_slot & ~(31ull << (5 * depth)))
                        | (cs << (5 * depth));
          }
          if (depth < SIG_DEPTH) sig_stack_at(depth) = cur_sig;
          is_arr_bits |= (1ull << depth);
          depth++;
          arr_depth++;
          cur_capture = false; cur_slot = -1;
          continue;  // parse first element
        }
      } else if (b == '"') {
        c.pos++;
        if (!scan_string_fast(c, voff, vlen)) return false;
        vtype = T_STR;
      } else if (b == 't') {
        if (c.end - c.pos < 4) return false;
        if (c.byte_at(c.pos+1)!='r'||c.byte_at(c.pos+2)!='u'||c.byte_at(c.pos+3)!='e') return false;
        c.pos += 4; vtype = T_TRUE;
      } else if (b == 'f') {
        if (c.end - c.pos < 5) return false;
        if (c.byte_at(c.pos+1)!='a'||c.byte_at(c.pos+2)!='l'||c.byte_at(c.pos+3)!='s'||c.byte_at(c.pos+4)!='e') return false;
        c.pos += 5; vtype = T_FALSE;
      } else if (b == 'n') {
        if (c.end - c.pos < 4) return false;
        if (c.byte_at(c.pos+1)!='u'||c.byte_at(c.pos+2)!='l'||c.byte_at(c.pos+3)!='l') return false;
        c.pos += 4; vtype = T_NULL;
      } else if (b == '-' || (b >= '0' && b <= '9')) {
        NumOut n = parse_json_number(c);
        if (!n.ok) return false;
        vtype = T_NUM; vnum = n.v;
      } else {
        return false;
      }

      // scalar (or empty-container) value completed
      if (vtype != T_MISSING) {
        if (cur_capture && arr_depth == 0)
          fv.set(cur_slot, vtype, voff, vlen, vnum);
        if (depth == 0) { top_type = (top_type == T_MISSING) ? vtype : top_type; }
      }
      expect_value = false;
      continue;
    }

    // after a value: close containers / separators
    if (depth == 0) {
      c.skip_ws();
      return c.eof();  // trailing garbage -> invalid
    }
    c.skip_ws();
    if (c.eof()) return false;
    uint8_t b = c.next();
    bool in_arr = (is_arr_bits >> (depth - 1)) & 1u;
    if (in_arr) {
      if (b == ',') { expect_value = true; cur_capture = false; cur_slot = -1; continue; }
      if (b == ']') {
        depth--; arr_depth--;
        {
          int cs = (depth < SLOT_DEPTH)
                       ? (int)((cont_slot >> (5 * depth)) & 31ull) : 31;
          if (cs != 31) fv.set_len(cs, c.pos - fv.get_soff(cs));
        }
        // restore parent sig (not needed for captures inside arrays)
        cur_sig = (depth < SIG_DEPTH) ? sig_stack_at(depth) : 0;
        continue;  // still "after value" for the parent
      }
      return false;
    } else {
      if (b == ',') {
        c.skip_ws();
        uint64_t parent = (depth - 1 < SIG_DEPTH) ? sig_stack_at(depth - 1) : 0;
        uint64_t ksig;
        if (!parse_key(parent, depth == 1, ksig)) return false;
        c.skip_ws();
        if (c.eof() || c.next() != ':') return false;
        cur_sig = ksig;
        cur_slot = (arr_depth == 0) ? match_slot(ksig) : -1;
        cur_capture = cur_slot >= 0;
        expect_value = true;
        continue;
      }
      if (b == '}') {
        depth--;
        {
          int cs = (depth < SLOT_DEPTH)
                       ? (int)((cont_slot >> (5 * depth)) & 31ull) : 31;
          if (cs != 31) fv.set_len(cs, c.pos - fv.get_soff(cs));
        }
        cur_sig = (depth < SIG_DEPTH) ? sig_stack_at(depth) : 0;
        continue;
      }
      return false;
    }
  }
}

// -------------------------------------------------------------------
// decoded-string compare (cold path: only spans containing '\\').
// JSON-unescapes the field span on the fly and 3-way-compares it
// against the constant's raw (unescaped) UTF-8 bytes, mirroring the
// host-side decode (gpu._decode_json_string) that group keys get.
// Decoded bytes are packed into a u32 (no local array) so the hot
// kernel stays scratch-free.

DEV int hexval4(uint8_t x) {
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
DEV int unesc_next(BS d, uint32_t fo, uint32_t fl,
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
DEV int unesc_cmp(BS d, uint32_t fo, uint32_t fl,
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
DEV bool span_has_backslash(BS d, uint32_t fo, uint32_t fl) {
  for (uint32_t k = 0; k < fl; k++)
    if (d.at(fo + k) == '\\') return true;
  return false;
}

// -------------------------------------------------------------------
// predicate evaluation (K2): -1 throw (missing field), 0 false, 1 true

template <class BS>
DEV int eval_leaf(const PlanView& P, BS BV, const FV& fv,
                  int op, int slot, int cidx) {
  uint8_t ft = fv.get_type(slot);
  if (ft == T_MISSING) return -1;  // krill: missing field -> throw

  int ckind = P.const_meta[cidx * 6 + 0];
  uint32_t coff = (uint32_t)P.const_meta[cidx * 6 + 1];
  uint32_t clen = (uint32_t)P.const_meta[cidx * 6 + 2];
  int cdvalid = P.const_meta[cidx * 6 + 3];
  double cdval = P.const_dvals[cidx];

  if (op == OP_EQ || op == OP_NE) {
    bool eq = false;
    if (ft == T_NULL) {
      eq = (ckind == CONST_NULL);
    } else if (ckind == CONST_NULL) {
      eq = false;
    } else if (ft == T_TRUE || ft == T_FALSE || ft == T_NUM) {
      double fnum = (ft == T_NUM) ? fv.get_num(slot) : (ft == T_TRUE ? 1.0 : 0.0);
      if (ckind == CONST_NUM) eq = (fnum == cdval);
      else eq = cdvalid && (fnum == cdval);  // number vs numeric string
    } else if (ft == T_STR) {
      if (ckind == CONST_STR) {
        uint32_t fo = fv.get_soff(slot), fl = fv.get_slen(slot);
        if (fl == clen) {
          eq = true;
          for (uint32_t k = 0; k < fl; k++)
            if (BV.at(fo + k) != P.const_bytes[coff + k]) { eq = false; break; }
        }
        // records may carry the constant in JSON-ESCAPED form: try
        // the canonical escaped rendering too (plan.py ConstPool)
        if (!eq) {
          uint32_t co2 = (uint32_t)P.const_meta[cidx * 6 + 4];
          uint32_t cl2 = (uint32_t)P.const_meta[cidx * 6 + 5];
          if (cl2 != 0 && fl == cl2) {
            eq = true;
            for (uint32_t k = 0; k < fl; k++)
              if (BV.at(fo + k) != P.const_bytes[co2 + k]) { eq = false; break; }
          }
        }
        // NON-canonical escapes in the data (GET, \/, surrogate
        // pairs): unescape-as-you-compare (cold; escaped spans only)
        if (!eq && span_has_backslash(BV, fo, fl))
          eq = unesc_cmp(BV, fo, fl, P.const_bytes + coff, clen) == 0;
      } else {  // string vs number: ToNumber(field)
        double fn = js_to_number(BV, fv.get_soff(slot), fv.get_slen(slot));
        eq = (fn == fn) && (fn == cdval);
      }
    } else {
      eq = false;  // object/array operands never equal scalars
    }
    return (op == OP_EQ) ? (eq ? 1 : 0) : (eq ? 0 : 1);
  }

  // relational
  if (ft == T_STR && ckind == CONST_STR) {
    uint32_t fo = fv.get_soff(slot), fl = fv.get_slen(slot);
    int cmp = 0;
    if (span_has_backslash(BV, fo, fl)) {
      cmp = unesc_cmp(BV, fo, fl, P.const_bytes + coff, clen);
      if (cmp == -2) cmp = 0;  // unreachable: tokenizer validated
    } else {
      uint32_t n = fl < clen ? fl : clen;
      for (uint32_t k = 0; k < n; k++) {
        uint8_t a = BV.at(fo + k), b = P.const_bytes[coff + k];
        if (a != b) { cmp = a < b ? -1 : 1; break; }
      }
      if (cmp == 0) cmp = (fl < clen) ? -1 : (fl > clen ? 1 : 0);
    }
    switch (op) {
      case OP_LT: return cmp < 0;
      case OP_LE: return cmp <= 0;
      case OP_GT: return cmp > 0;
      default:    return cmp >= 0;
    }
  }
  double x, y;
  if (ft == T_NUM) x = fv.get_num(slot);
  else if (ft == T_NULL) x = 0.0;
  else if (ft == T_TRUE) x = 1.0;
  else if (ft == T_FALSE) x = 0.0;
  else if (ft == T_STR) x = js_to_number(BV, fv.get_soff(slot), fv.get_slen(slot));
  else x = __builtin_nan("");  // object/array
  if (ckind == CONST_NUM) y = cdval;
  else if (ckind == CONST_NULL) y = 0.0;
  else y = cdvalid ? cdval : __builtin_nan("");
  if (x != x || y != y) return 0;
  switch (op) {
    case OP_LT: return x < y;
    case OP_LE: return x <= y;
    case OP_GT: return x > y;
    default:    return x >= y;
  }
}

template <class BS>
DEV int eval_predicate(const PlanView& P, BS BV,
                       const FV& fv, int prog_id) {
  int idx = P.prog_bounds[prog_id * 2 + 0];
  // frame packed into u64: op(1b) | remaining(23b) | end(32b), kept in
  // registers via RegArr (a plain array would spill to scratch)
  uint64_t stk[PRED_STACK];
  int sp = 0;
  int result;
  while (true) {
    int op = P.prog_nodes[idx * 4 + 0];
    if (op == OP_AND || op == OP_OR) {
      if (sp >= PRED_STACK) return -1;
      stk[sp] = ((uint64_t)(op == OP_OR)
                  | ((uint64_t)P.prog_nodes[idx * 4 + 1] << 1)
                  | ((uint64_t)P.prog_nodes[idx * 4 + 3] << 32));
      sp++;
      idx++;
      continue;
    }
    if (op == OP_TRUE) {
      result = 1;
      idx = P.prog_nodes[idx * 4 + 3];
    } else {
      result = eval_leaf(P, BV, fv, op,
                         P.prog_nodes[idx * 4 + 1],
                         P.prog_nodes[idx * 4 + 2]);
      idx = P.prog_nodes[idx * 4 + 3];
    }
    // unwind (short-circuit exactly like sequential evaluation)
    while (sp > 0) {
      if (result == -1) return -1;  // throw propagates
      uint64_t f = stk[sp - 1];
      bool is_or = f & 1;
      uint32_t remaining = (uint32_t)(f >> 1) & 0x7FFFFF;
      bool sc = (!is_or && result == 0) || (is_or && result == 1);
      remaining--;
      if (sc || remaining == 0) {
        idx = (int)(f >> 32);
        sp--;
      } else {
        stk[sp - 1] = (f & 0xFFFFFFFF00000001ull)
                      | ((uint64_t)remaining << 1);
        break;  // evaluate next child at idx
      }
    }
    if (sp == 0) return result;
  }
}

// -------------------------------------------------------------------
// dictionaries (string + number interning)

template <class BS>
DEV uint64_t hash_bytes(BS BV, uint32_t off, uint32_t len) {
  uint64_t h = FNV_OFFSET;
  for (uint32_t k = 0; k < len; k++) h = fnv1a_byte(h, BV.at(off + k));
  return mix64(h ^ len);
}

// Returns string id, or 0xFFFFFFFF on table/data overflow.
template <class BS>
DEV uint32_t intern_string(const StrDict& D, BS BV,
                           uint32_t off, uint32_t len) {
  uint64_t h = hash_bytes(BV, off, len);
  uint32_t mask = D.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes < D.nslots; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&D.state[s]);
      if (st == SLOT_READY) {
        if (atomic_load_relaxed(&D.hash[s]) != h) break;  // next probe
        // verify bytes
        uint32_t o2 = atomic_load_relaxed(&D.off[s]);
        uint32_t l2 = atomic_load_relaxed(&D.len[s]);
        if (l2 != len) break;
        bool same = true;
        for (uint32_t k = 0; k < len; k++)
          if (D.data[o2 + k] != BV.at(off + k)) { same = false; break; }
        if (same) return atomic_load_relaxed(&D.id[s]);
        break;
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&D.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
          // we own the slot: copy payload, publish
          uint32_t o = atomicAdd(D.data_used, (len + 7u) & ~7u);
          if (o + len > D.data_cap) return 0xFFFFFFFFu;  // overflow
          for (uint32_t k = 0; k < len; k++)
            atomic_store_relaxed(&D.data[o + k], BV.at(off + k));
          uint32_t myid = atomicAdd(D.next_id, 1u);
          atomic_store_relaxed(&D.hash[s], h);
          atomic_store_relaxed(&D.off[s], o);
          atomic_store_relaxed(&D.len[s], len);
          atomic_store_relaxed(&D.id[s], myid);
          drain_stores();
          atomic_store_relaxed(&D.state[s], SLOT_READY);
          return myid;
        }
        continue;  // lost the race: re-read state
      }
      // SLOT_CLAIMED by another lane: re-read (its publish completes
      // in its own loop iteration; no blocking spin)
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return 0xFFFFFFFFu;
}

DEV uint32_t intern_number(const NumDict& D, double v) {
  if (v == 0.0) v = 0.0;  // canonicalize -0
  uint64_t bits = __double_as_longlong(v);
  uint64_t h = mix64(bits ^ 0x9E3779B97F4A7C15ull);
  uint32_t mask = D.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes < D.nslots; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&D.state[s]);
      if (st == SLOT_READY) {
        if (atomic_load_relaxed(&D.bits[s]) != bits) break;
        return atomic_load_relaxed(&D.id[s]);
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&D.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
          uint32_t myid = atomicAdd(D.next_id, 1u);
          atomic_store_relaxed(&D.bits[s], bits);
          atomic_store_relaxed(&D.id[s], myid);
          drain_stores();
          atomic_store_relaxed(&D.state[s], SLOT_READY);
          return myid;
        }
        continue;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return 0xFFFFFFFFu;
}

// -------------------------------------------------------------------
// global aggregation insert (K5)

DEV bool agg_insert(const AggTable& T, const uint32_t* key, int nk,
                    double w) {
  uint64_t h = FNV_OFFSET;
  for (int k = 0; k < MAX_KEY; k++)
    h = mix64(h ^ (k < nk ? key[k] : 0u) ^ (uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull);
  uint32_t mask = T.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes < 4096u; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&T.state[s]);
      if (st == SLOT_READY) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < MAX_KEY; k++)
          if (k < nk &&
              atomic_load_relaxed(&T.keys[s * MAX_KEY + k]) != key[k])
            same = false;
        if (same) { atomicAdd(&T.count[s], w); return true; }
        break;
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&T.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
#pragma unroll
          for (int k = 0; k < MAX_KEY; k++)
            atomic_store_relaxed(&T.keys[s * MAX_KEY + k],
                                 k < nk ? key[k] : 0u);
          drain_stores();
          atomic_store_relaxed(&T.state[s], SLOT_READY);
          atomicAdd(&T.count[s], w);
          return true;
        }
        continue;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return false;  // pathological probe chain: table too full
}

// Directory variant for the dense-accumulation path: assign (or find)
// the key's stable slot WITHOUT touching count — counts accumulate in
// the caller's per-workgroup dense partial row and are folded by the
// MFMA reduce.  Returns the slot index or ~0u on probe exhaustion.
DEV uint32_t agg_insert_slot(const AggTable& T, const uint32_t* key,
                             int nk) {
  uint64_t h = FNV_OFFSET;
  for (int k = 0; k < MAX_KEY; k++)
    h = mix64(h ^ (k < nk ? key[k] : 0u) ^ (uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull);
  uint32_t mask = T.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  // TIGHT probe cap: once the directory saturates, every further
  // insert probe-scans to the cap before failing — with the old
  // nslots/4 cap a 5-field high-cardinality query measured 32 GB/s
  // (vs the 280 GB/s band) on its doomed first attempt; with the cap
  // + the global short-circuit it measures 150-256 GB/s.  256 probes
  // keeps the directory usable to ~85-90% load while keeping the
  // overflow attempt cheap; the engine restarts on the hash path.
  uint32_t max_probes = 256;
  for (uint32_t probes = 0; probes < max_probes; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&T.state[s]);
      if (st == SLOT_READY) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < MAX_KEY; k++)
          if (k < nk &&
              atomic_load_relaxed(&T.keys[s * MAX_KEY + k]) != key[k])
            same = false;
        if (same) return s;
        break;
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&T.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
#pragma unroll
          for (int k = 0; k < MAX_KEY; k++)
            atomic_store_relaxed(&T.keys[s * MAX_KEY + k],
                                 k < nk ? key[k] : 0u);
          drain_stores();
          atomic_store_relaxed(&T.state[s], SLOT_READY);
          return s;
        }
        continue;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return 0xFFFFFFFFu;
}

// Add one (key, weight) into a table: dense path (directory slot +
// this workgroup's partial row) or the atomic hash path.  gflag is
// the GLOBAL overflow counter: once any block overflows the dense
// directory the whole scan is doomed to restart, so later misses
// short-circuit instead of probe-scanning a saturated table.
DEV bool agg_add(const AggTable& T, const uint32_t* key, int nk,
                 double w, unsigned long long* gflag) {
  if (T.partial != nullptr) {
    if (atomic_load_relaxed(gflag) != 0ull) return false;
    uint32_t s = agg_insert_slot(T, key, nk);
    if (s == 0xFFFFFFFFu) {
      atomicAdd(gflag, 1ull);  // publish immediately (cross-block)
      return false;
    }
    atomicAdd(&T.partial[(size_t)(blockIdx.x % T.prows) * T.nslots + s],
              w);
    return true;
  }
  return agg_insert(T, key, nk, w);
}

// MFMA column-sum reduce: count[s] += sum_r partial[r][s], computed as
// ones[16,4] x partial-tile[4,16] on the f64 matrix core
// (v_mfma_f64_16x16x4_f64; A = all-ones so every accumulator row holds
// the column sum).  One wave per 16-slot tile x gridDim.y row splits.
typedef double dn_d4 __attribute__((ext_vector_type(4)));

__global__ void mfma_reduce_kernel(AggTable T, uint32_t rows_per_blk) {
  uint32_t slot0 = blockIdx.x * 16;
  uint32_t r0 = blockIdx.y * rows_per_blk;
  uint32_t r1 = r0 + rows_per_blk;
  if (r1 > T.prows) r1 = T.prows;
  int l = threadIdx.x;
  uint32_t n = slot0 + (l & 15);
  dn_d4 acc = {0.0, 0.0, 0.0, 0.0};
  const double* P = T.partial;
  size_t stride = T.nslots;
  for (uint32_t rt = r0; rt < r1; rt += 4) {
    uint32_t rr = rt + (uint32_t)(l >> 4);
    // B fragment: lane l holds B[k = l>>4][j = l&15]
    double b = (rr < r1 && n < T.nslots)
                   ? P[(size_t)rr * stride + n] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, b, acc, 0, 0, 0);
  }
  // C/D map: lane l holds D[(l>>4)*4 + reg, l&15]; rows identical
  // (A = ones), so lanes 0..15 publish their column's sum
  if (l < 16 && n < T.nslots) {
    double v = acc[0];
    if (v != 0.0) atomicAdd(&T.count[n], v);
  }
}

// -------------------------------------------------------------------
// the fused scan kernel

struct LdsCacheEntry {
  uint64_t hash;      // 0 = empty
  uint32_t metric;
  uint32_t key[MAX_KEY];
  double count;
};

// Dynamic-LDS layout of the scan and columnar kernels:
//   fv SoA | agg cache | counters [| synthetics | sig stack] | tile
// Defined ONCE: the kernels carve their LDS with it and the host sizes
// the launch (and checks the 160 KiB budget) from the same offsets.
// parse_state adds what only the NDJSON parser needs; the columnar
// kernel has neither synthetics nor a sig stack.
struct LdsLayout {
  size_t fv_soff, fv_slen, fv_type, cache, lcnt, synth, sig, tile, total;
  __host__ __device__ __forceinline__
  LdsLayout(int nf, int nm, int ns, bool parse_state) {
    size_t off = 0;
    fv_soff = off; off += (size_t)nf * BLOCK * sizeof(uint32_t);
    fv_slen = off; off += (size_t)nf * BLOCK * sizeof(uint32_t);
    fv_type = off; off += (size_t)nf * BLOCK * sizeof(uint8_t);
    off = (off + 15) & ~(size_t)15;
    cache = off; off += (size_t)LDS_CACHE * sizeof(LdsCacheEntry);
    lcnt = off;
    off += (size_t)(C_GLOBAL_N + nm * CM_N) * sizeof(unsigned long long);
    synth = sig = off;
    if (parse_state) {
      // sized by the ACTUAL synthetic count: the flagship plan has zero
      // synthetics and an unconditional MAX_SYNTH reservation (16 KB)
      // was costing a whole extra block of occupancy per CU
      off += (size_t)ns * BLOCK * sizeof(double);
      sig = off; off += (size_t)SIG_DEPTH * BLOCK * sizeof(uint64_t);
    }
    off = (off + 15) & ~(size_t)15;
    tile = off;         // optional staging tile: ScanArgs.tile_cap bytes
    total = off + 64;   // slack
  }
};

// -------------------------------------------------------------------
// aggregation tail shared by the scan and columnar kernels: key-column
// encoding, the LDS combining cache, and its block-level init / flush

// Encode one breakdown column (value type t: num, or the span so/sl)
// to its u32 key code (K4: bucketize; dict-intern).  Returns false
// with drop set (the record is nonnumeric for a bucketized column) or
// overflow set (a dictionary is full).
template <class BS>
DEV bool encode_key_col(const StrDict& sdict, const NumDict& ndict, BS BV,
                       uint8_t t, double num, uint32_t so, uint32_t sl,
                       int bucket, double step, uint32_t& code,
                        bool& drop, bool& overflow) {
  if (bucket != BUCKET_NONE) {
    if (t == T_STR) {
      // numeric STRINGS coerce for bucketized fields (JS arithmetic in
      // the reference's bucketizer: its own golden counts
      // {"latency": "26"} into the p2 histogram —
      // tests/data/2014/05-05/more.log:1); NaN / +-Infinity drop as
      // nonnumeric
      num = js_to_number(BV, so, sl);
      if (!(num == num) || num == __builtin_inf() ||
          num == -__builtin_inf())
        { drop = true; return false; }
      t = T_NUM;
    }
    // nonnumeric; an over-range literal (1e400) is +-Infinity and
    // drops like the Infinity strings above
    if (t != T_NUM || !finite_num(num)) { drop = true; return false; }
    double ordf = bucket_ordinal(bucket, num, step);
    if (ord_is_small(ordf)) {
      code = make_code(TAG_ORD, (uint32_t)((int)ordf + ORD_BIAS));
    } else {
      uint32_t id = intern_number(ndict, ordf);
      if (id == 0xFFFFFFFFu) { overflow = true; return false; }
      code = make_code(TAG_NUM, id);
    }
  } else if (t == T_MISSING) {
    code = make_code(TAG_SPECIAL, SPECIAL_UNDEF);
  } else if (t == T_NULL) {
    code = make_code(TAG_SPECIAL, SPECIAL_NULL);
  } else if (t == T_TRUE) {
    code = make_code(TAG_SPECIAL, SPECIAL_TRUE);
  } else if (t == T_FALSE) {
    code = make_code(TAG_SPECIAL, SPECIAL_FALSE);
  } else if (t == T_OBJ) {
    code = make_code(TAG_SPECIAL, SPECIAL_OBJECT);
  } else if (t == T_ARR) {
    // intern the raw JSON span; the host canonicalizes it with JS
    // Array.toString semantics (plan.decode_key)
    uint32_t id = intern_string(sdict, BV, so, sl);
    if (id == 0xFFFFFFFFu || id >= (1u << 27)) { overflow = true; return false; }
    code = make_code(TAG_SPECIAL, SPECIAL_ARRJSON | (id << 3));
  } else if (t == T_NUM) {
    uint32_t id = intern_number(ndict, num);
    if (id == 0xFFFFFFFFu) { overflow = true; return false; }
    code = make_code(TAG_NUM, id);
  } else {  // T_STR
    uint32_t id = intern_string(sdict, BV, so, sl);
    if (id == 0xFFFFFFFFu) { overflow = true; return false; }
    code = make_code(TAG_STR, id);
  }
  return true;
}

// LDS combining cache: hash of (metric, key); never 0 (0 = empty slot)
DEV uint64_t agg_key_hash(int m, const uint32_t* key) {
  uint64_t kh = mix64((uint64_t)m * 0x9E3779B97F4A7C15ull + 1);
  for (int k = 0; k < MAX_KEY; k++) kh = mix64(kh ^ key[k]);
  return kh == 0 ? 1 : kh;
}

// Add (metric m, key, weight) to the block's LDS cache, falling through
// to the global table when the probes are exhausted.
//
// NOTE on the LDS cache race: two lanes with DIFFERENT keys that
// collide on the same 64-bit kh would mis-combine.  kh is a 64-bit mix
// of the full key; a collision needs two distinct key tuples in one
// block with equal mix64 chains (~2^-64 per pair) — accepted and
// documented (SURVEY parity corners).  Identity (metric + key words)
// is nevertheless verified for the common same-slot case; the claim
// fill is racy only against lanes carrying the SAME kh.
//
// UNROLL is the probe loop's unroll count, fixed per kernel to the
// shape each compiled to before the loop was shared: rolled (1) in the
// scan kernels, where unrolling raises SGPR spills 226 -> 242 and
// measured 1.3% slower device-resident; fully unrolled (8) in the
// columnar kernel, where rolling raises them 165 -> 196.
template <int UNROLL>
DEV void lds_cache_add(LdsCacheEntry* cache, AggTable* tables,
                       unsigned long long* counters,
                       unsigned long long* lcnt, int m,
                       const uint32_t* key, int nk, uint64_t kh,
                       double weight) {
  bool cached = false;
  uint32_t ci = (uint32_t)kh & (LDS_CACHE - 1);
  // 8 probes: a hot key that loses every probe degrades to per-record
  // contended global inserts (measured 4x slower on low-cardinality
  // ordinal breakdowns with 2 probes)
#pragma unroll UNROLL
  for (int attempt = 0; attempt < 8; attempt++) {
    unsigned long long prev = atomicCAS(
        (unsigned long long*)&cache[ci].hash, 0ull,
        (unsigned long long)kh);
    if (prev == 0) {
      // claimed: fill identity (hash claim is the sync point;
      // same-key lanes re-check identity below)
      cache[ci].metric = m;
      for (int k = 0; k < MAX_KEY; k++) cache[ci].key[k] = key[k];
      atomicAdd(&cache[ci].count, weight);
      cached = true;
      break;
    }
    if (prev == (unsigned long long)kh && cache[ci].metric == m) {
      bool same = true;
      for (int k = 0; k < MAX_KEY; k++)
        if (cache[ci].key[k] != key[k]) { same = false; break; }
      if (same) {
        atomicAdd(&cache[ci].count, weight);
        cached = true;
        break;
      }
    }
    ci = (ci + 1) & (LDS_CACHE - 1);
  }
  if (!cached) {
    if (!agg_add(tables[m], key, nk, weight, &counters[C_OVERFLOW]))
      atomicAdd(&lcnt[C_OVERFLOW], 1ull);
  }
}

// Block start: empty the cache and zero the block-local counters.
DEV void block_agg_init(LdsCacheEntry* cache, unsigned long long* lcnt,
                        int ncnt) {
  for (int i = threadIdx.x; i < LDS_CACHE; i += BLOCK) {
    cache[i].hash = 0;
    cache[i].metric = 0;
    for (int k = 0; k < MAX_KEY; k++) cache[i].key[k] = 0;
    cache[i].count = 0.0;
  }
  for (int i = threadIdx.x; i < ncnt; i += BLOCK) lcnt[i] = 0;
  __syncthreads();
}

// Block end: flush the cache into the global tables, then the
// block-local counters into the global ones.
DEV void block_agg_flush(LdsCacheEntry* cache, unsigned long long* lcnt,
                         int ncnt, const PlanView& P, AggTable* tables,
                         unsigned long long* counters) {
  __syncthreads();
  for (int i = threadIdx.x; i < LDS_CACHE; i += BLOCK) {
    if (cache[i].hash != 0) {
      if (!agg_add(tables[cache[i].metric], cache[i].key,
                   P.metric_rows[cache[i].metric * 8 + 1],
                   cache[i].count, &counters[C_OVERFLOW]))
        atomicAdd(&lcnt[C_OVERFLOW], 1ull);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncnt; i += BLOCK) {
    if (lcnt[i]) atomicAdd(&counters[i], lcnt[i]);
  }
}

// ---- newline indexing (device-side, no host sync) ----
// Three passes over 2 KiB segments: count, exclusive-scan, write.
// Positions come out globally sorted because each segment writes its
// newlines in order at its scanned base offset.

constexpr uint32_t NL_SEG = 2048;

// SWAR newline mask: high bit set in each byte lane equal to '\n'.
// EXACT per-byte form: the classic (x-0x01..)&~x&0x80.. zero test is
// only exact as a boolean — a borrow out of a true-zero byte false-
// positives the next byte when it is 0x01 (i.e. the byte 0x0B right
// after a real '\n'; caught by the envelope-crossing fuzzer on binary
// garbage lines).  This form has no cross-byte carries.
DEV uint32_t nl_mask32(uint32_t w) {
  uint32_t x = w ^ 0x0A0A0A0Au;            // zero byte where '\n'
  uint32_t y = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;  // hi set iff low7!=0
  return ~(y | x | 0x7F7F7F7Fu);           // hi set iff byte==0
}

// byte-validity mask for a word at byte address wpos over [start, n)
DEV uint32_t range_mask32(uint32_t wpos, uint32_t start, uint32_t n) {
  uint32_t m = 0x80808080u;
  if (wpos >= start && wpos + 4 <= n) return m;  // interior fast path
  uint32_t out = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    uint32_t pos = wpos + b;
    if (pos >= start && pos < n) out |= 0x80u << (b * 8);
  }
  return out;
}

// One WAVE per 2 KiB segment: lane l reads 16 B at seg*2048 +
// half*1024 + l*16 — fully coalesced 1 KiB wave-lines.  (The previous
// thread-per-segment walk gathered 64 addresses 2 KiB apart per load
// and measured ~240 GB/s; this form is read-bandwidth-bound.)
__global__ void newline_count_kernel(const uint8_t* data,
                                     uint32_t start, uint32_t n,
                                     uint32_t* seg_counts,
                                     uint32_t nseg) {
  uint32_t seg = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  uint32_t lane = threadIdx.x & 63u;
  const uint4* p16 = reinterpret_cast<const uint4*>(data);
  uint32_t base0 = (start & ~15u) + seg * NL_SEG;
  uint32_t cnt = 0;
#pragma unroll
  for (int half = 0; half < 2; half++) {
    uint32_t base = base0 + half * 1024u + lane * 16u;
    if (base < n) {
      uint4 v = p16[base >> 4];
      uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int wi = 0; wi < 4; wi++)
        cnt += __popc(nl_mask32(w[wi]) &
                      range_mask32(base + wi * 4, start, n));
    }
  }
  for (int off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (lane == 0) seg_counts[seg] = cnt;
}

// single-block exclusive scan over seg_counts (nseg can be large; a
// 1024-thread block walks tiles with a running carry)
__global__ void newline_scan_kernel(uint32_t* seg_counts, uint32_t nseg,
                                    uint32_t* total_out) {
  __shared__ uint32_t tile[1024];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nseg; base += 1024) {
    uint32_t i = base + threadIdx.x;
    uint32_t v = (i < nseg) ? seg_counts[i] : 0;
    tile[threadIdx.x] = v;
    __syncthreads();
    // Hillis-Steele inclusive scan in LDS
    for (uint32_t d = 1; d < 1024; d <<= 1) {
      uint32_t t = (threadIdx.x >= d) ? tile[threadIdx.x - d] : 0;
      __syncthreads();
      tile[threadIdx.x] += t;
      __syncthreads();
    }
    uint32_t incl = tile[threadIdx.x];
    if (i < nseg) seg_counts[i] = carry + incl - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry += tile[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ void newline_write_kernel(const uint8_t* data,
                                     uint32_t start, uint32_t n,
                                     const uint32_t* seg_offsets,
                                     uint32_t nseg, uint32_t* out_pos,
                                     uint32_t cap) {
  // wave-per-segment, coalesced (see newline_count_kernel); per-half
  // lane-exclusive scan of newline counts keeps positions sorted:
  // lane l's bytes precede lane l+1's, half 0 precedes half 1
  uint32_t seg = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  uint32_t lane = threadIdx.x & 63u;
  const uint4* p16 = reinterpret_cast<const uint4*>(data);
  uint32_t base0 = (start & ~15u) + seg * NL_SEG;
  uint32_t w_at = seg_offsets[seg];
#pragma unroll
  for (int half = 0; half < 2; half++) {
    uint32_t base = base0 + half * 1024u + lane * 16u;
    uint32_t m[4] = {0, 0, 0, 0};
    uint32_t cnt = 0;
    if (base < n) {
      uint4 v = p16[base >> 4];
      uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int wi = 0; wi < 4; wi++) {
        m[wi] = nl_mask32(w[wi]) &
                range_mask32(base + wi * 4, start, n);
        cnt += __popc(m[wi]);
      }
    }
    // lane-exclusive scan of cnt
    uint32_t incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
      uint32_t t = __shfl_up(incl, off, 64);
      if ((int)lane >= off) incl += t;
    }
    uint32_t at = w_at + incl - cnt;
#pragma unroll
    for (int wi = 0; wi < 4; wi++) {
      uint32_t mm = m[wi];
      while (mm) {
        uint32_t b = ((uint32_t)__ffs(mm) - 1) >> 3;  // byte lane
        if (at < cap) out_pos[at] = base + wi * 4 + b;
        at++;
        mm &= mm - 1;
      }
    }
    w_at += __shfl(incl, 63, 64);  // wave total
  }
}

// -------------------------------------------------------------------
// Columnar index-query kernel (K7): evaluate a query directly over an
// index table's typed columns (reference lib/index-query.js:303-338
// runs SELECT ... WHERE pred GROUP BY; here the predicate + bucketize
// + hash-aggregate run over uploaded columns — no NDJSON round trip).
// Rows are weighted points: weight = the stored SUM(value).

struct ColDesc {
  int32_t kind;  // 0 = missing for every row, 1 = numeric, 2 = string
  int32_t pad_;
  const double* num;     // [nrows] (kind 1)
  const uint32_t* soff;  // [nrows] into the shared blob (kind 2)
  const uint32_t* slen;
};

struct ColArgs {
  uint32_t nrows;
  const double* values;  // [nrows] row weights
  const uint8_t* blob;   // concatenated string payloads
  const ColDesc* cols;   // [P.nf] per plan slot
  PlanView P;
  AggTable* tables;
  StrDict sdict;
  NumDict ndict;
  unsigned long long* counters;
};

// 5 waves/SIMD is what this kernel compiles to (91 VGPRs); holding the
// register allocator to it keeps the SGPR spill count at the level the
// kernel had before it shared the aggregation tail (157 vs 163; at a
// bound of 4 the allocator lands on 165).
__launch_bounds__(BLOCK, 5)
__global__ void columnar_query_kernel(ColArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smemc[];
  const PlanView& P = A.P;
  const int nf = P.nf;
  const LdsLayout L(nf, P.nm, 0, false);
  LdsCacheEntry* cache = reinterpret_cast<LdsCacheEntry*>(smemc + L.cache);
  unsigned long long* lcnt =
      reinterpret_cast<unsigned long long*>(smemc + L.lcnt);
  const int NCNT = C_GLOBAL_N + P.nm * CM_N;
  block_agg_init(cache, lcnt, NCNT);

  FV fv;
  fv.type = reinterpret_cast<uint8_t*>(smemc + L.fv_type);
  fv.soff = reinterpret_cast<uint32_t*>(smemc + L.fv_soff);
  fv.slen = reinterpret_cast<uint32_t*>(smemc + L.fv_slen);
  fv.tid = threadIdx.x;
  Bytes BV;
  BV.mem = A.blob;
  BV.bias = 0;

  const uint32_t stride = gridDim.x * BLOCK;
  for (uint32_t r = blockIdx.x * BLOCK + threadIdx.x; r < A.nrows;
       r += stride) {
    atomicAdd(&lcnt[C_LINES], 1ull);
    atomicAdd(&lcnt[C_PARSED], 1ull);
    for (int f = 0; f < nf; f++) {
      const ColDesc& c = A.cols[f];
      if (c.kind == 1)
        fv.set(f, T_NUM, 0, 0, c.num[r]);
      else if (c.kind == 2)
        fv.set(f, T_STR, c.soff[r], c.slen[r], 0.0);
      else
        fv.set(f, T_MISSING, 0, 0, 0.0);
    }
    // program 0: the combined (query ∧ time-bounds) filter
    {
      int keep = eval_predicate(P, BV, fv, 0);
      if (keep != 1) {
        if (keep == -1) atomicAdd(&lcnt[C_DS_FAILEDEVAL], 1ull);
        else atomicAdd(&lcnt[C_DS_FILTERED], 1ull);
        continue;
      }
    }
    double weight = A.values[r];
    for (int m = 0; m < P.nm; m++) {
      const int32_t* M = &P.metric_rows[m * 8];
      unsigned long long* mc = &lcnt[C_GLOBAL_N + m * CM_N];
      atomicAdd(&mc[CM_AGG_IN], 1ull);

      uint32_t key[MAX_KEY];
      int nk = M[1];
      bool drop = false, overflow = false;
      for (int bi = 0; bi < nk; bi++) {
        const int32_t* B = &P.bd_rows[(M[2] + bi) * 4];
        int slot = B[1];  // columnar plans use kind-0 refs only
        uint32_t code;
        if (!encode_key_col(A.sdict, A.ndict, BV, fv.get_type(slot),
                            fv.get_num(slot), fv.get_soff(slot),
                            fv.get_slen(slot), B[2],
                            P.bd_steps[M[2] + bi], code, drop, overflow))
          break;
#pragma unroll
        for (int kk = 0; kk < MAX_KEY; kk++)
          if (kk == bi) key[kk] = code;
      }
      if (overflow) { atomicAdd(&lcnt[C_OVERFLOW], 1ull); continue; }
      if (drop) { atomicAdd(&mc[CM_NONNUMERIC], 1ull); continue; }
#pragma unroll
      for (int k = 0; k < MAX_KEY; k++)
        if (k >= nk) key[k] = 0;

      lds_cache_add<8>(cache, A.tables, A.counters, lcnt, m, key, nk,
                    agg_key_hash(m, key), weight);
    }
  }

  block_agg_flush(cache, lcnt, NCNT, P, A.tables, A.counters);
}

// Device-side wave-transpose builder: scatter each (length-sorted)
// record's bytes into the granule-interleaved layout scan_kernel_x
// consumes (byte p of slot r -> wbase[r/64] + (p/gran)*(64*gran) +
// (r%64)*gran + p%gran).  One wave per 64-slot transposed wave: for a
// fixed granule g the 64 lanes write 64 CONSECUTIVE granules (fully
// coalesced 2 KiB stores); reads are per-record gathers (the cost the
// transpose exists to pay once instead of every scan pass).
__global__ void xpose_build_kernel(const uint8_t* __restrict__ data,
                                   const uint32_t* __restrict__ sstart,
                                   const uint32_t* __restrict__ slen,
                                   const unsigned long long* __restrict__ wbase,
                                   uint32_t n_slots, int gran_log,
                                   uint8_t* __restrict__ xb) {
  uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  uint32_t nw = n_slots >> 6;
  if (w >= nw) return;
  uint32_t lane = threadIdx.x & 63u;
  uint32_t r = (w << 6) + lane;
  uint32_t gran = 1u << gran_log;
  unsigned long long base = wbase[w];
  uint32_t gw = (uint32_t)((wbase[w + 1] - base) >> (6 + gran_log));
  uint32_t len = slen[r];
  if (len == 0xFFFFFFFFu) len = 0;  // padding slot
  uint32_t start = sstart[r];
  uint8_t* dst0 = xb + base + ((size_t)lane << gran_log);
  for (uint32_t g = 0; g < gw; g++) {
    uint8_t* dst = dst0 + ((size_t)g << (6 + gran_log));
    uint32_t off = g << gran_log;
    for (uint32_t k = 0; k < gran; k += 16) {
      uint8_t tmp[16];
#pragma unroll
      for (int t = 0; t < 16; t++) {
        uint32_t o = off + k + t;
        tmp[t] = (o < len) ? data[start + o] : (uint8_t)'\n';
      }
      uint4 vv;
      __builtin_memcpy(&vv, tmp, 16);
      *reinterpret_cast<uint4*>(dst + k) = vv;
    }
  }
}

template <int XP>
DEV void scan_kernel_body(char* smem, ScanArgs A);

__launch_bounds__(BLOCK)
__global__ void scan_kernel(ScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem0[];
  scan_kernel_body<0>(smem0, A);
}

// occupancy-capped variants (min waves per SIMD; constrains the
// register allocator) — selected at runtime for A/B measurement
template <int MW>
__launch_bounds__(BLOCK, MW)
__global__ void scan_kernel_mw(ScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem1[];
  scan_kernel_body<0>(smem1, A);
}
template __global__ void scan_kernel_mw<2>(ScanArgs);
template __global__ void scan_kernel_mw<3>(ScanArgs);
template __global__ void scan_kernel_mw<4>(ScanArgs);
template __global__ void scan_kernel_mw<5>(ScanArgs);
template __global__ void scan_kernel_mw<6>(ScanArgs);

// wave-transposed record staging (XBytesT; DRAGNET_XPOSE).
// second parameter = log2 granule bytes (DRAGNET_XGRAN)
template <int MW, int XLG>
__launch_bounds__(BLOCK, MW)
__global__ void scan_kernel_x(ScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem2[];
  scan_kernel_body<XLG>(smem2, A);
}
template __global__ void scan_kernel_x<2, 6>(ScanArgs);
template __global__ void scan_kernel_x<3, 6>(ScanArgs);
template __global__ void scan_kernel_x<4, 6>(ScanArgs);
template __global__ void scan_kernel_x<5, 6>(ScanArgs);
template __global__ void scan_kernel_x<4, 5>(ScanArgs);
template __global__ void scan_kernel_x<4, 7>(ScanArgs);

// Per-record pipeline (K1-K6) shared by the linear and the
// wave-transposed (XBytes) kernels: tokenize/extract, predicate,
// synthetics, per-metric filter + bucketize + intern + aggregate.
#define synth_val_at(si) synth_lds[(si) * BLOCK + threadIdx.x]

template <class BS>
DEV void process_record(BS BV, uint32_t start, uint32_t end,
                        const ScanArgs& A, const PlanView& P, FV& fv,
                        unsigned long long* lcnt, LdsCacheEntry* cache,
                        uint64_t* sig_lds, double* synth_lds) {
  const int nf = P.nf;
  uint32_t synth_ok = 0;
  atomicAdd(&lcnt[C_LINES], 1ull);
  // only the type lane needs initializing: soff/slen/num are read
  // only after a capture set them
  for (int f = 0; f < nf; f++)
    fv.type[f * BLOCK + fv.tid] = T_MISSING;

  uint8_t top_type;
  bool ok = (end > start) &&
            parse_record(BV, start, end, P, fv, top_type, sig_lds,
                         A.data_format_skinner);
  double weight = 1.0;
  if (ok && A.data_format_skinner) {
    // require: object top, a "fields" member, numeric "value"
    bool has_fields = P.fields_slot >= 0 &&
                      fv.get_type(P.fields_slot) != T_MISSING;
    bool val_num = P.value_slot >= 0 &&
                   fv.get_type(P.value_slot) == T_NUM;
    if (top_type != T_OBJ || !has_fields || !val_num) ok = false;
    else weight = fv.get_num(P.value_slot);
  }
  if (!ok) {
    atomicAdd(&lcnt[C_INVALID_JSON], 1ull);
  } else {
    atomicAdd(&lcnt[C_PARSED], 1ull);

    // datasource filter (program 0)
    int keep = eval_predicate(P, BV, fv, 0);
    if (keep == -1) atomicAdd(&lcnt[C_DS_FAILEDEVAL], 1ull);
    else if (keep == 0) atomicAdd(&lcnt[C_DS_FILTERED], 1ull);

    if (keep == 1) {
      // synthetic date fields (shared across metrics)
      synth_ok = 0;
      for (int si = 0; si < P.ns; si++) {
        int slot = P.synth_slots[si];
        uint8_t t = fv.get_type(slot);
        uint32_t ok;
        if (t == T_MISSING) ok = 2;                           // undef
        else if (t == T_NUM) {
          ok = 1; synth_val_at(si) = fv.get_num(slot);
        } else if (t == T_STR) {
          DateOut d = parse_iso_ms(BV, fv.get_soff(slot),
                                   fv.get_slen(slot));
          if (d.ok) {
            long long secs = d.ms >= 0 ? d.ms / 1000
                                       : (d.ms - 999) / 1000;
            ok = 1; synth_val_at(si) = (double)secs;
          } else ok = 3;                                      // baddate
        } else ok = 3;  // bool/null/obj/arr: Date.parse fails
        synth_ok |= ok << (2 * si);
      }

      // per-metric pipeline
      for (int m = 0; m < P.nm; m++) {
        const int32_t* M = &P.metric_rows[m * 8];
        unsigned long long* mc = &lcnt[C_GLOBAL_N + m * CM_N];
        atomicAdd(&mc[CM_FILTER_IN], 1ull);

        int res = eval_predicate(P, BV, fv, M[0]);
        if (res == -1) { atomicAdd(&mc[CM_FAILEDEVAL], 1ull); continue; }
        if (res == 0) { atomicAdd(&mc[CM_FILTERED], 1ull); continue; }

        // synthetic requirements (first failure counted; record
        // dropped on any failure — stream-synthetic.js:37-85)
        bool sok = true;
        for (int k = 0; k < M[3]; k++) {
          int si = P.synth_req[M[4] + k];
          uint32_t ok = (synth_ok >> (2 * si)) & 3u;
          if (ok != 1) {
            atomicAdd(&mc[ok == 2 ? CM_UNDEF : CM_BADDATE], 1ull);
            sok = false; break;
          }
        }
        if (!sok) continue;

        // time filter on dn_ts (= last synth req when present)
        if (M[5]) {
          int si = P.synth_req[M[4] + M[3] - 1];
          double ts = synth_val_at(si);
          if (!(ts >= (double)M[6] && ts < (double)M[7])) {
            atomicAdd(&mc[CM_TIME_OUT], 1ull); continue;
          }
        }

        atomicAdd(&mc[CM_AGG_IN], 1ull);

        // build the group key (K4: bucketize; dict-intern)
        uint32_t key[MAX_KEY];
        int nk = M[1];
        bool drop = false, overflow = false;
        for (int bi = 0; bi < nk; bi++) {
          const int32_t* B = &P.bd_rows[(M[2] + bi) * 4];
          double step = P.bd_steps[M[2] + bi];
          uint8_t t; double num = 0.0; uint32_t so = 0, sl = 0;
          if (B[0] == 1) {  // synthetic date value
            int si = B[1];
            if (((synth_ok >> (2 * si)) & 3u) == 1) {
              t = T_NUM; num = synth_val_at(si);
            } else t = T_MISSING;  // cannot happen: required above
          } else {
            int slot = B[1];
            // aggregation lookup is literal-first (points.lookup):
            // a top-level literal dotted key (companion slot)
            // shadows the plucked nested value
            int cs2 = P.comp_slot[slot];
            if (cs2 >= 0 && fv.get_type(cs2) != T_MISSING)
              slot = cs2;
            t = fv.get_type(slot);
            num = fv.get_num(slot);
            so = fv.get_soff(slot); sl = fv.get_slen(slot);
          }
          uint32_t code;
          if (!encode_key_col(A.sdict, A.ndict, BV, t, num, so, sl, B[2],
                              step, code, drop, overflow))
            break;
          // constant-index write keeps key[] in registers
#pragma unroll
          for (int kk = 0; kk < MAX_KEY; kk++)
            if (kk == bi) key[kk] = code;
        }
        if (overflow) { atomicAdd(&lcnt[C_OVERFLOW], 1ull); continue; }
        if (drop) { atomicAdd(&mc[CM_NONNUMERIC], 1ull); continue; }
#pragma unroll
        for (int k = 0; k < MAX_KEY; k++)
          if (k >= nk) key[k] = 0;

        uint64_t kh = agg_key_hash(m, key);

        // Wave-level pre-combining: lanes carrying the same key
        // elect one leader per distinct kh which adds the whole
        // group's weight — one LDS atomic per distinct key per
        // wavefront instead of one per record.  (Only when every
        // weight is 1: json format; skinner weights vary.)
        if (!A.data_format_skinner) {
          uint64_t unproc = __ballot(true);  // lanes still here
          bool leader = false;
          double wsum = 0.0;
          while (unproc) {
            int src = (int)(__ffsll((long long)unproc) - 1);
            uint64_t src_kh = __shfl(kh, src);
            bool same = (kh == src_kh);
            uint64_t grp = __ballot(same);
            if (same && __lane_id() == src) {
              leader = true;
              wsum = (double)__popcll(grp);
            }
            unproc &= ~grp;
          }
          if (!leader) continue;  // combined into the leader's add
          weight = wsum;
        }
        lds_cache_add<1>(cache, A.tables, A.counters, lcnt, m, key, nk, kh,
                      weight);
      }
    }
  }
}

template <int XP>
DEV void scan_kernel_body(char* smem, ScanArgs A) {
  const PlanView& P = A.P;
  const int nf = P.nf;

  const LdsLayout L(nf, P.nm, P.ns, true);
  LdsCacheEntry* cache = reinterpret_cast<LdsCacheEntry*>(smem + L.cache);
  unsigned long long* lcnt =
      reinterpret_cast<unsigned long long*>(smem + L.lcnt);
  const int NCNT = C_GLOBAL_N + P.nm * CM_N;
  double* synth_lds = reinterpret_cast<double*>(smem + L.synth);
  uint64_t* sig_lds = reinterpret_cast<uint64_t*>(smem + L.sig);
  uint8_t* tile = reinterpret_cast<uint8_t*>(smem + L.tile);  // staging
  block_agg_init(cache, lcnt, NCNT);

  FV fv;
  fv.type = reinterpret_cast<uint8_t*>(smem + L.fv_type);
  fv.soff = reinterpret_cast<uint32_t*>(smem + L.fv_soff);
  fv.slen = reinterpret_cast<uint32_t*>(smem + L.fv_slen);
  fv.tid = threadIdx.x;

  if constexpr (XP != 0) {
    // wave-transposed pool (XP = log2 granule bytes): slot r's bytes
    // live granule-interleaved at xwave_base[r/64] + (r%64)*GRAN; a
    // wave's refills are 64 consecutive granules (coalesced) instead
    // of 64 scattered records.  Record order is length-sorted by the
    // host — the aggregation is order-independent (associative
    // merge).
    const uint32_t stride_x = gridDim.x * BLOCK;
    for (uint32_t rbase = blockIdx.x * BLOCK; rbase < A.xn_slots;
         rbase += stride_x) {
      uint32_t r = rbase + threadIdx.x;
      if (r < A.xn_slots) {
        uint32_t len = A.xrec_len[r];
        if (len != 0xFFFFFFFFu) {
          XBytesT<XP> BV;
          BV.base = A.xdata + A.xwave_base[r >> 6]
                    + ((size_t)(r & 63u) << XP);
          process_record(BV, 0u, len, A, P, fv, lcnt, cache, sig_lds,
                         synth_lds);
        }
      }
    }
  } else {
  uint32_t nlines = *A.nlines_ptr;
  if (nlines > A.pos_cap) nlines = A.pos_cap;
  const uint32_t stride = gridDim.x * BLOCK;
  for (uint32_t rbase = blockIdx.x * BLOCK; rbase < nlines;
       rbase += stride) {
    uint32_t r = rbase + threadIdx.x;
    bool active = r < nlines;

    // Block-level LDS staging: copy the block's contiguous record
    // span into the tile with coalesced uint4 loads, then parse from
    // LDS (banked reads) instead of 64-way divergent global gathers.
    Bytes BV;
    BV.mem = A.data;
    BV.bias = 0;
    uint32_t t_start = rbase ? A.nl_pos[rbase - 1] + 1 : A.first_start;
    uint32_t r_last = rbase + BLOCK - 1;
    if (r_last >= nlines) r_last = nlines - 1;
    uint32_t t_end = A.nl_pos[r_last] + 1;
    uint32_t t_base = t_start & ~15u;
    uint32_t span = t_end - t_base;
    bool staged = A.tile_cap >= 16 && span <= A.tile_cap;
    if (staged) {
      const uint4* g16 = reinterpret_cast<const uint4*>(A.data + t_base);
      uint4* l16 = reinterpret_cast<uint4*>(tile);
      uint32_t n16 = (span + 15) >> 4;
      for (uint32_t i = threadIdx.x; i < n16; i += BLOCK)
        l16[i] = g16[i];
      __syncthreads();
      BV.mem = tile;
      BV.bias = t_base;
    }

    if (active) {
      uint32_t start = r ? A.nl_pos[r - 1] + 1 : A.first_start;
      uint32_t end = A.nl_pos[r];
      process_record(BV, start, end, A, P, fv, lcnt, cache, sig_lds,
                     synth_lds);
    }

    if (staged) __syncthreads();  // tile reused next iteration
  }
  }  // XP

  block_agg_flush(cache, lcnt, NCNT, P, A.tables, A.counters);
}

// -------------------------------------------------------------------
// extraction kernels

__global__ void extract_agg_kernel(AggTable T, uint32_t* out_keys,
                                   double* out_counts, uint32_t* out_n,
                                   uint32_t max_out) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= T.nslots) return;
  if (atomic_load_relaxed(&T.state[s]) != SLOT_READY) return;
  uint32_t i = atomicAdd(out_n, 1u);
  if (i >= max_out) return;
  for (int k = 0; k < MAX_KEY; k++)
    out_keys[i * MAX_KEY + k] = T.keys[s * MAX_KEY + k];
  out_counts[i] = T.count[s];
}

__global__ void extract_strdict_kernel(StrDict D, uint32_t* out_off,
                                       uint32_t* out_len, uint32_t max_ids) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= D.nslots) return;
  if (atomic_load_relaxed(&D.state[s]) != SLOT_READY) return;
  uint32_t id = D.id[s];
  if (id >= max_ids) return;
  out_off[id] = D.off[s];
  out_len[id] = D.len[s];
}

__global__ void extract_numdict_kernel(NumDict D, double* out_vals,
                                       uint32_t max_ids) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= D.nslots) return;
  if (atomic_load_relaxed(&D.state[s]) != SLOT_READY) return;
  uint32_t id = D.id[s];
  if (id >= max_ids) return;
  out_vals[id] = __longlong_as_double(
      (long long)atomic_load_relaxed(&D.bits[s]));
}

}  // namespace dn
