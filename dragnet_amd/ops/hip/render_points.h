// Receiving end of the merge, DEVICE ONLY: the merged table as merge_rows.h
// leaves it (distinct rows [g, nk + 1] of key codes and a tag pack, their
// f64 sums, the global string dictionary as a UTF-8 blob with offsets) to
// the bytes `dn scan --points` prints: one NDJSON line per row,
//   {"fields":{"a":"x","b":30},"value":5}\n
// byte for byte what output.point_json gives for the point that
// Aggregator.points() builds from merge._decode_rows of that row
// (dragnet_amd/merge.py, render_points).  Line i is row order[i]; no row
// becomes a Python object.
//
//   render_escape_measure_kernel  dictionary strings -> escaped lengths,
//                                 quotes included; validates offsets, UTF-8
//   sort_scan_kernel              } exclusive scan of those lengths: the
//   sort_scan_sums_kernel         } escaped dictionary's offsets (sort_rows.h)
//   render_measure_kernel         output lines -> lengths; validates order
//                                 entries, tags and string codes; refusals
//   sort_scan_kernel              line lengths, per 2048 lines
//   render_totals_kernel          the block sums -> int64 bases; totals -> meta
//   (the host reads meta: its one sync, and sizes esc_blob and text exactly)
//   render_escape_kernel          dictionary strings -> esc_blob
//   render_emit_kernel            rows -> text, line_off
//
//  * Escape once, compose by copying.  A dictionary string is escaped once
//    (json.dumps with ensure_ascii, i.e. c_encode_basestring_ascii; esc_json
//    of index/points_fast.cpp): `"` and `\` take a backslash, 08 09 0A 0C 0D
//    are \b \t \n \f \r, any other byte below 0x20 and 0x7F are \u00xx
//    (lowercase hex), a 2- or 3-byte sequence is \uxxxx, a 4-byte one its
//    surrogate pair; the quotes are part of the entry.  A line then only
//    copies: its constant pieces (rendered by the host once per call:
//    `{"fields":{"a":`, `,"b":`, ..., `},"value":`, `}\n`), the escaped
//    strings of its string elements, and decimal digits.  The escaped
//    dictionary's offsets are the scanned lengths in their two levels
//    (esc_scan + esc_sums), read by ren_esc_at; no third array holds them.
//  * One escape routine, one line routine.  ren_escape and ren_line are
//    templates over a sink that either counts or stores, so the measure and
//    the write of a string, and of a line, cannot disagree on a length: the
//    stores of the second pass fill exactly what the first pass measured.
//    ren_escape reads through unify_strings.h's 8-byte window; a word whose
//    bytes all lie in 0x20..0x7E with no `"` and no `\` (five SWAR tests)
//    goes out whole, any other word byte by byte through the UTF-8
//    automaton of encode_table.h (no overlong form, no surrogate, nothing
//    above U+10FFFF, no truncated sequence: what Python's decoder accepts).
//  * Staging.  A tile is 256 consecutive dictionary ids or 256 consecutive
//    output lines: its output is one contiguous range of esc_blob or text.
//    Escape: the tile's input bytes come into LDS by lane-consecutive
//    16-byte loads (unify_load16) when they are at most REN_IN_BYTES;
//    lanes escape into an output stage of REN_OUT_BYTES laid out as
//    esc_blob is, and the block stores that range by lane-consecutive
//    16-byte stores, the ragged first and last unit by bytes.  Emit: lanes
//    compose their lines into a stage of REN_STAGE_BYTES (48 KB: it assumes
//    lines of 191 bytes on average; the kernel's LDS holds nothing else) and
//    the block stores it the same way.  A tile that does not fit (one 4 KB
//    string beside others) runs the same routine straight to global
//    memory, lane per string or per line.  The choice is block-uniform.
//  * Numbers.  A plain or date element is its code; a quantize ordinal i is
//    0 for i <= 0, else 2^(i-1); an lquantize ordinal is i * step.  The value
//    is the sum when it is integral and below 2^63 in magnitude (f64 to int64
//    is exact there; -0.0 is 0).  Digits come 9 at a time: one 64-bit
//    division by 10^9, then 32-bit ones.  What does not fit int64 (i - 1 >=
//    63, an overflowing product), a fractional, NaN or infinite sum, an
//    F64-tagged element and a line of REN_MAX_LINE bytes or more set
//    REN_REFUSED: Python renders those as unbounded ints or floats, and the
//    caller takes the host path for the whole table.
//  * Bounds.  g, G < 2^31.  Every dictionary offset pair is checked against
//    the blob, every order entry against g, every tag to be INT, STR or F64,
//    every string code against G, the constant pieces' offsets against
//    their blob; a failure sets a status bit, the lane
//    reads nothing through the bad value, every later kernel returns at once
//    when the word is set, and the binding raises.  The escaped dictionary
//    is below 2^32 bytes (the binding bounds 6 * bytes + 2 * G); a line is
//    below REN_MAX_LINE = 2^20, so 2048 of them sum in u32; across blocks
//    the offsets are int64 (render_totals_kernel).  Within a tile u32.
//  * No atomics beyond the status OR.  All stores are vector stores.
#pragma once
#include "unify_strings.h"

namespace dn {

constexpr int REN_BLOCK = 256;               // ids / lines per tile = threads
constexpr int REN_IN_BYTES = 16 * 1024;      // escape: input stage
constexpr int REN_OUT_BYTES = 32 * 1024;     // escape: output stage
constexpr int REN_STAGE_BYTES = 48 * 1024;   // emit: 256 lines of <= 191 B
constexpr uint32_t REN_MAX_LINE = 1u << 20;

// column kinds (points.fast_reduce_spec)
constexpr int REN_COL_PLAIN = 0, REN_COL_DATE = 1, REN_COL_QUANTIZE = 2,
              REN_COL_LQUANTIZE = 3;

// wire tags (merge.py _EL_*)
constexpr long long REN_EL_INT = 0, REN_EL_STR = 1, REN_EL_F64 = 2;

// status word bits
constexpr uint32_t REN_BAD_DICT = 1;   // dictionary offsets outside the blob
constexpr uint32_t REN_BAD_UTF8 = 2;   // an ill-formed dictionary string
constexpr uint32_t REN_BAD_ORDER = 4;  // an order entry >= g
constexpr uint32_t REN_BAD_TAG = 8;    // a tag that is none of INT, STR, F64
constexpr uint32_t REN_BAD_CODE = 16;  // a string code outside 0..G-1
constexpr uint32_t REN_BAD_SEG = 32;   // seg_offs outside seg_blob
constexpr uint32_t REN_REFUSED = 64;   // what only Python renders

// meta words (u64), read by the host in one copy
enum RenMeta : int { REN_M_STATUS = 0, REN_M_ESC_BYTES, REN_M_TEXT_BYTES,
                     REN_M_WORDS };

struct RenArgs {
  const long long* rows;       // [g, nk + 1]
  const double* sums;          // [g]
  const uint32_t* order;       // [g] or null: line i is row i
  uint32_t g;
  int nk;
  const uint8_t* dict_blob;    // 16-byte aligned
  long long dict_len;
  const long long* dict_offs;  // [G + 1]
  uint32_t G;
  uint8_t col_kind[MAX_KEY];
  long long col_step[MAX_KEY];
  const uint8_t* seg_blob;     // the nk + 2 constant pieces
  long long seg_len;
  const long long* seg_offs;   // [nk + 3]
  uint32_t* esc_scan;          // [round8(G + 1)], zeros; lengths, scanned
  uint32_t* esc_sums;
  uint32_t* line_scan;         // [round8(g + 1)], zeros; lengths, scanned
  uint32_t* line_sums;         // [line_nsums]
  uint32_t line_nsums;
  long long* line_base;        // [line_nsums]
  unsigned long long* meta;    // [REN_M_WORDS]
  // allocated once the host has read meta
  uint8_t* esc_blob;           // 16-byte aligned
  long long esc_len;
  uint8_t* text;               // 16-byte aligned
  long long* line_off;         // [g + 1]
};

DEV uint32_t ren_status(const RenArgs& A) {
  return *reinterpret_cast<const uint32_t*>(A.meta);
}

// OR the lanes' bits into the status word; the whole wave calls it.
DEV void ren_fail(const RenArgs& A, uint32_t bad) {
#pragma unroll
  for (int off = 32; off; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if (bad && __lane_id() == 0)
    atomicOr(reinterpret_cast<uint32_t*>(A.meta), bad);
}

// Offset of escaped string c in esc_blob, c in 0..G.
DEV uint32_t ren_esc_at(const RenArgs& A, uint32_t c) {
  return A.esc_scan[c] + A.esc_sums[c / SORT_SCAN_TILE];
}

// Offset of line i in text, i in 0..g.
DEV long long ren_line_at(const RenArgs& A, uint32_t i) {
  return (long long)A.line_scan[i] + A.line_base[i / SORT_SCAN_TILE];
}

// ---- sinks: what the two passes do with a byte ---------------------------

struct RenCount {
  uint32_t n;
  DEV void put(uint8_t) { n++; }
  DEV void word(uint64_t, uint32_t m) { n += m; }
};

struct RenStore {
  uint8_t* p;
  DEV void put(uint8_t c) { *p++ = c; }
  DEV void word(uint64_t v, uint32_t m) {
    for (uint32_t b = 0; b < m; b++) *p++ = (uint8_t)(v >> (8 * b));
  }
};

// ---- one string, escaped ---------------------------------------------------

// Every byte of v in 0x20..0x7E and none of them `"` or `\`.
DEV bool ren_plain_word(uint64_t v) {
  constexpr uint64_t HI = 0x8080808080808080ull, ONES = 0x0101010101010101ull;
  const uint64_t q = v ^ (ONES * 0x22), s = v ^ (ONES * 0x5C),
                 d = v ^ (ONES * 0x7F);
  const uint64_t hit = v                        // a byte >= 0x80
                       | ((v - ONES * 0x20) & ~v)  // a byte < 0x20
                       | ((q - ONES) & ~q) | ((s - ONES) & ~s)
                       | ((d - ONES) & ~d);
  return !(hit & HI);
}

template <class Sink>
DEV void ren_hex4(Sink& out, uint32_t x) {
  out.put('\\');
  out.put('u');
#pragma unroll
  for (int sh = 12; sh >= 0; sh -= 4) {
    const uint32_t h = (x >> sh) & 15u;
    out.put((uint8_t)(h < 10 ? '0' + h : 'a' + (h - 10)));
  }
}

template <class Sink>
DEV void ren_ascii(Sink& out, uint32_t c) {
  if (c == 0x22 || c == 0x5C) {
    out.put('\\');
    out.put((uint8_t)c);
  } else if (c >= 0x20 && c != 0x7F) {
    out.put((uint8_t)c);
  } else {
    const uint8_t k = c == 8 ? 'b' : c == 9 ? 't' : c == 10 ? 'n'
                    : c == 12 ? 'f' : c == 13 ? 'r' : 0;
    if (k) {
      out.put('\\');
      out.put(k);
    } else {
      ren_hex4(out, c);
    }
  }
}

// The span (off, len) of W as a JSON string, quotes included; false when
// it is not UTF-8 that Python's decoder accepts (the output then is
// unspecified but no longer than 6 * len + 2).
template <class Words, class Sink>
DEV bool ren_escape(Words W, long long off, long long len, Sink& out) {
  constexpr uint64_t SPACES = 0x2020202020202020ull;
  out.put('"');
  UnifySpan<Words> span(W, off, len);
  uint32_t need = 0, lo = 0x80, hi = 0xBF, cp = 0;  // a sequence under way
  for (long long k = 0; k < len; k += 8) {
    const uint64_t v = span.next();
    const uint32_t m = (uint32_t)min(8ll, len - k);
    if (need == 0 && ren_plain_word(m < 8 ? v | (SPACES << (8 * m)) : v)) {
      out.word(v, m);
      continue;
    }
    for (uint32_t b = 0; b < m; b++) {
      const uint32_t c = (uint32_t)(v >> (8 * b)) & 0xffu;
      if (need) {
        if (c < lo || c > hi) return false;
        cp = (cp << 6) | (c & 0x3Fu);
        lo = 0x80; hi = 0xBF;
        if (--need == 0) {
          if (cp < 0x10000u) {
            ren_hex4(out, cp);
          } else {
            cp -= 0x10000u;
            ren_hex4(out, 0xD800u + (cp >> 10));
            ren_hex4(out, 0xDC00u + (cp & 0x3FFu));
          }
        }
      } else if (c < 0x80) {
        ren_ascii(out, c);
      } else if (c >= 0xC2 && c <= 0xDF) { need = 1; cp = c & 0x1Fu;
      } else if (c == 0xE0) { need = 2; cp = 0; lo = 0xA0;
      } else if (c == 0xED) { need = 2; cp = 0xD; hi = 0x9F;
      } else if (c >= 0xE1 && c <= 0xEF) { need = 2; cp = c & 0xFu;
      } else if (c == 0xF0) { need = 3; cp = 0; lo = 0x90;
      } else if (c == 0xF4) { need = 3; cp = 4; hi = 0x8F;
      } else if (c >= 0xF1 && c <= 0xF3) { need = 3; cp = c & 7u;
      } else { return false; }
    }
  }
  if (need) return false;
  out.put('"');
  return true;
}

// Bring [base, end) of the blob (base a multiple of 16, end <= blob_len)
// into the stage, 16 bytes per lane and step.
DEV void ren_stage_in(uint4* stage, const uint8_t* blob, long long blob_len,
                      long long base, long long end) {
  const uint32_t units = (uint32_t)((end - base + 15) >> 4);
  for (uint32_t u = threadIdx.x; u < units; u += REN_BLOCK)
    stage[u] = unify_load16(blob, blob_len, base + 16ll * u);
  __syncthreads();
}

// Store [lo, hi) of dst (16-byte aligned) out of the stage, whose byte 0
// is dst byte lo & ~15: lane-consecutive 16-byte stores, the ragged first
// and last unit by bytes.
DEV void ren_stage_out(uint8_t* dst, const uint4* stage, long long lo,
                       long long hi) {
  const long long base = lo & ~15ll;
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage);
  const uint32_t units = (uint32_t)((hi - base + 15) >> 4);
  for (uint32_t u = threadIdx.x; u < units; u += REN_BLOCK) {
    const long long at = base + 16ll * u;
    if (at >= lo && at + 16 <= hi) {
      *reinterpret_cast<uint4*>(dst + at) = stage[u];
    } else {
      for (uint32_t b = 0; b < 16u; b++)
        if (at + b >= lo && at + b < hi) dst[at + b] = bytes[16u * u + b];
    }
  }
}

__launch_bounds__(REN_BLOCK)
__global__ void render_escape_measure_kernel(RenArgs A) {
  __shared__ uint4 stage[REN_IN_BYTES / 16];
  const uint32_t row0 = blockIdx.x * REN_BLOCK, s = row0 + threadIdx.x;
  const uint32_t m = min((uint32_t)REN_BLOCK, A.G - row0);
  const bool live = threadIdx.x < m;
  long long off = 0, end = 0;
  bool ok = true;
  if (live) {
    off = A.dict_offs[s];
    end = A.dict_offs[s + 1];
    ok = off >= 0 && off <= end && end <= A.dict_len;
  }
  uint32_t bad = ok ? 0u : REN_BAD_DICT;
  long long lo = 0, hi = 0;
  if (__syncthreads_and(ok)) {  // block-uniform: the offsets ascend
    lo = A.dict_offs[row0];
    hi = A.dict_offs[row0 + m];
  }
  const long long base = lo & ~15ll;
  RenCount cnt = {0};
  bool well = true;
  if (hi > lo && hi - base <= REN_IN_BYTES) {
    ren_stage_in(stage, A.dict_blob, A.dict_len, base, hi);
    const UnifyLdsWords L = {reinterpret_cast<const uint64_t*>(stage),
                             base >> 3};
    if (live) well = ren_escape(L, off, end - off, cnt);
  } else if (live && ok) {
    const UnifyGlobalWords W = {A.dict_blob, A.dict_len};
    well = ren_escape(W, off, end - off, cnt);
  }
  if (live && ok) {
    if (!well) bad |= REN_BAD_UTF8;
    A.esc_scan[s] = cnt.n;
  }
  ren_fail(A, bad);
}

__launch_bounds__(REN_BLOCK)
__global__ void render_escape_kernel(RenArgs A) {
  __shared__ uint4 stage[REN_IN_BYTES / 16];
  __shared__ uint4 outb[REN_OUT_BYTES / 16];
  if (ren_status(A)) return;  // the offsets below are validated
  const uint32_t row0 = blockIdx.x * REN_BLOCK, s = row0 + threadIdx.x;
  const uint32_t m = min((uint32_t)REN_BLOCK, A.G - row0);
  const bool live = threadIdx.x < m;
  long long off = 0, end = 0, dst = 0;
  if (live) {
    off = A.dict_offs[s];
    end = A.dict_offs[s + 1];
    dst = ren_esc_at(A, s);
  }
  const long long lo = A.dict_offs[row0], hi = A.dict_offs[row0 + m];
  const long long dlo = ren_esc_at(A, row0), dhi = ren_esc_at(A, row0 + m);
  const long long base = lo & ~15ll, dbase = dlo & ~15ll;
  if (hi > lo && hi - base <= REN_IN_BYTES &&
      dhi - dbase <= REN_OUT_BYTES) {  // block-uniform
    ren_stage_in(stage, A.dict_blob, A.dict_len, base, hi);
    const UnifyLdsWords L = {reinterpret_cast<const uint64_t*>(stage),
                             base >> 3};
    // the tile's entries tile [dlo, dhi): one writer per byte
    RenStore w = {reinterpret_cast<uint8_t*>(outb) + (dst - dbase)};
    if (live) ren_escape(L, off, end - off, w);
    __syncthreads();
    ren_stage_out(A.esc_blob, outb, dlo, dhi);
  } else if (live) {
    const UnifyGlobalWords W = {A.dict_blob, A.dict_len};
    RenStore w = {A.esc_blob + dst};
    ren_escape(W, off, end - off, w);
  }
}

// ---- one line ----------------------------------------------------------------

// The integer a key element stands for, when int64 holds it.
DEV bool ren_int_value(int kind, long long step, long long c, long long& v) {
  if (kind == REN_COL_QUANTIZE) {
    if (c > 63) return false;
    v = c <= 0 ? 0 : 1ll << (c - 1);
    return true;
  }
  if (kind == REN_COL_LQUANTIZE) return !__builtin_mul_overflow(c, step, &v);
  v = c;
  return true;
}

// Decimal digits of u, at least one, at most 20.
DEV uint32_t ren_digits(uint64_t u) {
  uint32_t d = 1;
  for (uint64_t p = 10; d < 20 && u >= p; p *= 10) d++;
  return d;
}

struct RenLineCount {
  uint64_t n;
  DEV void seg(const RenArgs& A, int k) {
    n += (uint64_t)(A.seg_offs[k + 1] - A.seg_offs[k]);
  }
  DEV void str(const RenArgs& A, uint32_t c) {
    n += ren_esc_at(A, c + 1) - ren_esc_at(A, c);
  }
  DEV void num(long long v) {
    n += ren_digits(v < 0 ? 0ull - (uint64_t)v : (uint64_t)v) + (v < 0);
  }
};

struct RenLineStore {
  uint8_t* p;
  DEV void seg(const RenArgs& A, int k) {
    const long long end = A.seg_offs[k + 1];
    for (long long b = A.seg_offs[k]; b < end; b++) *p++ = A.seg_blob[b];
  }
  DEV void str(const RenArgs& A, uint32_t c) {
    const uint32_t at = ren_esc_at(A, c);
    const uint32_t len = ren_esc_at(A, c + 1) - at;
    const UnifyGlobalWords W = {A.esc_blob, A.esc_len};
    UnifySpan<UnifyGlobalWords> span(W, (long long)at, (long long)len);
    for (uint32_t k = 0; k < len; k += 8) {
      const uint64_t v = span.next();
      const uint32_t m = min(8u, len - k);
      for (uint32_t b = 0; b < m; b++) *p++ = (uint8_t)(v >> (8 * b));
    }
  }
  DEV void num(long long v) {
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    if (v < 0) *p++ = '-';
    const uint32_t d = ren_digits(u);
    uint32_t at = d;
    while (u >= 1000000000ull) {  // 9 digits per 64-bit division
      const uint64_t q = u / 1000000000ull;
      uint32_t low = (uint32_t)(u - q * 1000000000ull);
      for (int k = 0; k < 9; k++) {
        p[--at] = (uint8_t)('0' + low % 10u);
        low /= 10u;
      }
      u = q;
    }
    uint32_t low = (uint32_t)u;
    while (at) {
      p[--at] = (uint8_t)('0' + low % 10u);
      low /= 10u;
    }
    p += d;
  }
};

// Line of row r into the sink; the status bits of what stopped it, or 0.
template <class Sink>
DEV uint32_t ren_line(const RenArgs& A, uint32_t r, Sink& out) {
  const long long* row = A.rows + (size_t)r * (size_t)(A.nk + 1);
  const long long tp = row[A.nk];
#pragma unroll
  for (int j = 0; j < MAX_KEY; j++) {
    if (j >= A.nk) break;
    out.seg(A, j);
    const long long tag = (tp >> (2 * j)) & 3, c = row[j];
    if (tag == REN_EL_STR) {
      if ((unsigned long long)c >= (unsigned long long)A.G)
        return REN_BAD_CODE;
      out.str(A, (uint32_t)c);
    } else if (tag == REN_EL_INT) {
      long long v;
      if (!ren_int_value(A.col_kind[j], A.col_step[j], c, v))
        return REN_REFUSED;
      out.num(v);
    } else {
      return tag == REN_EL_F64 ? REN_REFUSED : REN_BAD_TAG;
    }
  }
  out.seg(A, A.nk);
  const double x = A.sums[r];
  if (!(x == trunc(x) && fabs(x) < 9223372036854775808.0))  // NaN: neither
    return REN_REFUSED;
  out.num((long long)x);
  out.seg(A, A.nk + 1);
  return 0;
}

__launch_bounds__(REN_BLOCK)
__global__ void render_measure_kernel(RenArgs A) {
  if (ren_status(A)) return;  // esc_scan holds no offsets then
  const uint32_t i = blockIdx.x * REN_BLOCK + threadIdx.x;
  // the constant pieces: every lane the same few words
  uint32_t bad = A.seg_offs[0] == 0 && A.seg_offs[A.nk + 2] == A.seg_len
                     ? 0u : REN_BAD_SEG;
  for (int k = 0; k < A.nk + 2; k++)
    if (A.seg_offs[k] > A.seg_offs[k + 1]) bad = REN_BAD_SEG;
  if (i < A.g && !bad) {
    const uint32_t r = A.order ? A.order[i] : i;
    if (r >= A.g) {
      bad = REN_BAD_ORDER;
    } else {
      RenLineCount cnt = {0};
      bad = ren_line(A, r, cnt);
      if (!bad && cnt.n >= REN_MAX_LINE) bad = REN_REFUSED;
      if (!bad) A.line_scan[i] = (uint32_t)cnt.n;
    }
  }
  ren_fail(A, bad);
}

// One block: exclusive scan of the line blocks' u32 sums into int64 bases,
// and the two byte totals for the host.
__launch_bounds__(SORT_BLOCK)
__global__ void render_totals_kernel(RenArgs A) {
  __shared__ unsigned long long wsum[SORT_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < A.line_nsums; base += SORT_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const unsigned long long v = i < A.line_nsums ? A.line_sums[i] : 0;
    unsigned long long incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long t = __shfl_up(incl, off, 64);
      if ((int)lane >= off) incl += t;
    }
    __syncthreads();  // the last round's readers of wsum
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned long long pre = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)SORT_WAVES; k++) {
      if (k < wave) pre += wsum[k];
      all += wsum[k];
    }
    if (i < A.line_nsums) A.line_base[i] = (long long)(carry + pre + incl - v);
    carry += all;
  }
  if (threadIdx.x == 0) {
    A.meta[REN_M_TEXT_BYTES] = carry;
    A.meta[REN_M_ESC_BYTES] = ren_status(A) ? 0ull : ren_esc_at(A, A.G);
  }
}

__launch_bounds__(REN_BLOCK)
__global__ void render_emit_kernel(RenArgs A) {
  __shared__ uint4 stage[REN_STAGE_BYTES / 16];
  if (ren_status(A)) return;  // order, tags and codes below are validated
  const uint32_t row0 = blockIdx.x * REN_BLOCK, i = row0 + threadIdx.x;
  const uint32_t m = min((uint32_t)REN_BLOCK, A.g - row0);
  const bool live = threadIdx.x < m;
  const long long lo = ren_line_at(A, row0), hi = ren_line_at(A, row0 + m);
  long long at = 0;
  uint32_t r = 0;
  if (live) {
    at = ren_line_at(A, i);
    r = A.order ? A.order[i] : i;
    A.line_off[i] = at;
    if (i == A.g - 1) A.line_off[A.g] = hi;
  }
  const long long base = lo & ~15ll;
  if (hi - base <= REN_STAGE_BYTES) {  // block-uniform
    // the tile's lines tile [lo, hi): one writer per byte
    RenLineStore w = {reinterpret_cast<uint8_t*>(stage) + (at - base)};
    if (live) ren_line(A, r, w);
    __syncthreads();
    ren_stage_out(A.text, stage, lo, hi);
  } else if (live) {
    RenLineStore w = {A.text + at};
    ren_line(A, r, w);
  }
}

}  // namespace dn
