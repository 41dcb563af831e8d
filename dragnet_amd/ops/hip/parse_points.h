// The reduce side's front door: NDJSON tagged point lines,
//   {"fields":{"__dn_metric":0,"a":"x","t":1400000000},"value":5}\n
// as `dn scan --points`, `dn index-scan` and render_points.h write them,
// to the rows merge_rows.h groups: the inverse of render_points.h.  Every
// line ends in one of four classes, as do_line of index/points_fast.cpp
// defines them after cli.cmd_index_read's loop over Aggregator.write:
//   SKIP   blank after stripping space, tab and CR; or a well-formed line
//          whose __dn_metric is absent, no integer literal or out of range
//   DROP   a bucketized column holds null, a bool, nothing or a number
//          that is not finite: ninputs and nonnumeric of the metric go up
//   TAKEN  one row is written, ninputs goes up
//   PUNT   the line goes back verbatim as a byte range; no counter moves
// Punting is always right (the caller runs the host reducer over the
// punts), so whatever is doubtful is punted.  The first part (the line
// routine pp_line and what it stands on) is plain C++17 under a host
// compiler (tools_dev/points_host_check.cpp); the kernels are DEVICE ONLY.
//
//   parse_nl_count_kernel  text -> newlines per 2 KiB segment
//   sort_scan_kernel       } exclusive scan of those counts (sort_rows.h)
//   sort_scan_sums_kernel  }
//   parse_lines_kernel     the totals -> meta   (host sync 1: line count)
//   parse_nl_write_kernel  text -> nl_pos, ascending
//   parse_measure_kernel   lines -> class, span count; the counters
//   parse_measure_global_kernel   the same for the tiles beyond the stage
//   sort_scan_kernel       } ONE scan over taken flags, span counts and
//   sort_scan_sums_kernel  } punt flags, three parts of one array
//   parse_totals_kernel    the three totals -> meta (host sync 2: sizes)
//   parse_emit_kernel      taken lines -> metric, rows, spans, vals;
//                          punted lines -> punts
//   parse_emit_global_kernel      the same for the tiles beyond the stage,
//                          launched only when the measure pass met one
//
//  * What is taken.  {"fields":{...},"value":V} or value first, space or
//    tab between tokens (json.dumps' ", " and ": ").  Names and strings
//    have no backslash and no byte below 0x20 and are well-formed UTF-8
//    by the automaton of render_points.h (no overlong form, no surrogate,
//    nothing above U+10FFFF).  A duplicate field name takes the last value.
//    V is an integer literal, 0 <= V < 2^53, without sign.  A field value
//    is a string, true, false, null or a json-strict number.  An integer
//    literal holds |v| <= 2^53.  In a plain column it is the span of its
//    own characters (so -0 is punted: Python prints 0), as are true, false
//    and null; a string is its span; a missing field is the span of the
//    constant `undefined` the caller put behind the data.  A date column
//    keeps an integer, truncates a fraction/exponent literal (dn_dec2dbl,
//    at most 19 significant digits, |t| < 2^62) and spans anything else.
//    A bucketized column takes both number forms through bucket_ordinal
//    (an lquantize ordinal at or beyond 2^62 is punted); a literal of
//    1e309 or more is infinite for float() and drops, one in [1e308,
//    1e309) is punted.
//  * What is punted: an escape anywhere, a nested value, a duplicate or
//    unknown top-level key, a missing value beside a valid metric, a value
//    that is no unsigned integer literal below 2^53, a fraction/exponent
//    literal or -0 in a plain column, more than 19 significant digits, an
//    integer beyond 2^53, trailing garbage, ill-formed UTF-8, a CR, FF or
//    VT inside the line, NaN and Infinity, a line above PP_MAX_LINE bytes,
//    a __dn_metric of true or false (Python counts a bool as an int) and
//    ANY STRING UNDER A BUCKETIZER: js_to_number is exact against
//    krill.to_number only on unescaped ASCII, and the host reducer punts
//    part of that itself; the device leaves all of it to the host.
//  * Two walks, one routine.  pp_walk checks the whole line against the
//    grammar and hands every field to a visitor.  The first walk's visitor
//    keeps the last __dn_metric and the value; the second, run only when
//    the metric is known, matches each name against that one metric's
//    columns and keeps a token (start, length, type) per column: MAX_KEY
//    tokens of lane state, no per-field table.  The columns are then
//    resolved in order, so the first bucketized column that is not
//    numeric drops the line whatever comes later, as Aggregator.write
//    returns there.  pp_line is a template over the byte source (the LDS
//    stage or global memory) and the sink (PpCount, PpStore), so the
//    measure and emit passes cannot disagree.
//  * Staging.  A tile is 256 consecutive lines, one contiguous byte range.
//    When [start & ~15, end) is at most PP_STAGE_BYTES it comes into LDS
//    by lane-consecutive 16-byte loads (unify_load16) and the lanes walk
//    their lines out of LDS.  Any other tile (one 60 KB line among short
//    ones, or lines of more than 191 bytes on average) runs the same
//    routine from global memory (PpGlobal, also the host checker's
//    source), a byte load per step: slower, and right.  The choice is
//    block-uniform, and each source has kernels of its own, so a kernel
//    holds one instantiation of pp_line and the staged ones carry no
//    second parser: both pairs are launched over all tiles and a block
//    whose tile is the other pair's returns at once (two index reads).
//    The global measure kernel ORs a word of meta when it meets a tile,
//    and the host launches the global emit kernel only then.  PpGlobal
//    reads through a volatile pointer: with plain loads this compiler's
//    reuse of loaded bytes gave fraction/exponent tokens the value of
//    their integer part on the GPU ("t":-1.5e3 became -1, "lat":1e999 was
//    taken as 1), in the global kernels only and in every build of them;
//    with each byte loaded where the source asks for it they agree with
//    the staged kernels and the host build (profiles/r16_parse_points.md).
//  * Order.  Rows, spans and punts are numbered by the exclusive scan of
//    the measure pass, so they come in line order whatever the execution
//    order; the spans of ascending rows ascend, apart from `undefined`,
//    and unify_hash_kernel's staging applies to them.
//  * Bounds.  data_len < 2^31; positions are u32.  A byte is read only at
//    pos < end of its line, and a line ends at or before data_len; the
//    tail is never read, only pointed at.  nl_pos is written by this
//    layer and clamped when read.  The specs are checked by the binding.
//    The store sink checks its row and span indices against the totals.
//  * The counters are atomicAdds of per-wave ballot counts, integers, so
//    their result has no order either.  No other atomics but the status
//    OR of PP_M_WIDE; all stores are vector stores.
//  * Caps (the Python side does not call the op beyond them):
//    PP_MAX_METRICS = 8 metrics, PP_NAME_BYTES = 2048 bytes of column
//    names in all, PP_MAX_LINE = 256 KiB per line (longer: punted).
#pragma once
#include "scan_text.h"
#if defined(__HIPCC__)
#include "unify_strings.h"
#endif

namespace dn {

constexpr int PP_BLOCK = 256;              // lines per tile = threads
constexpr int PP_STAGE_BYTES = 48 * 1024;  // 256 lines of <= 191 B
constexpr uint32_t PP_MAX_LINE = 1u << 18;
constexpr int PP_MAX_METRICS = 8;
constexpr int PP_NAME_BYTES = 2048;
constexpr uint32_t PP_TAIL = 9;            // strlen("undefined")
constexpr uint32_t PP_NL_SEG = 2048;       // bytes per newline segment
constexpr uint64_t PP_2_53 = 1ull << 53;
constexpr double PP_2_62 = 4611686018427387904.0;

enum PpClass : uint8_t { PP_SKIP = 0, PP_DROP = 1, PP_TAKEN = 2, PP_PUNT = 3 };

enum PpType : uint8_t { PP_T_MISSING = 0, PP_T_NULL, PP_T_FALSE, PP_T_TRUE,
                        PP_T_INT, PP_T_FLT, PP_T_STR };

// column kinds (points.fast_reduce_spec)
constexpr int PP_COL_PLAIN = 0, PP_COL_DATE = 1, PP_COL_QUANTIZE = 2,
              PP_COL_LQUANTIZE = 3;

// The metrics' columns, one struct in device memory, built by the binding.
struct PpSpecs {
  double step[PP_MAX_METRICS][MAX_KEY];
  uint16_t name_off[PP_MAX_METRICS][MAX_KEY];  // into names
  uint16_t name_len[PP_MAX_METRICS][MAX_KEY];
  uint8_t kind[PP_MAX_METRICS][MAX_KEY];
  uint8_t nk[PP_MAX_METRICS];
  int32_t nm;
  uint8_t names[PP_NAME_BYTES];
};

struct PpTok {
  uint32_t start, len;  // a string without its quotes; else the literal
  uint8_t type;
};

// What a taken line gives.
struct PpRow {
  long long el[MAX_KEY];   // INT elements; a STR element is its span
  uint32_t sstart[MAX_KEY], slen[MAX_KEY];
  uint32_t strmask;        // bit j: column j is a span
  int metric;
  double value;
};

// ---- byte sources: positions are offsets into the text ---------------------

struct PpGlobal {
  const volatile uint8_t* text;  // every byte is loaded where it is asked for
  DN_HD_INLINE uint8_t at(uint32_t p) const { return text[p]; }
};

struct PpStage {
  const uint8_t* stage;  // byte 0 is text byte `base`
  uint32_t base;
  DN_HD_INLINE uint8_t at(uint32_t p) const { return stage[p - base]; }
};

template <class Src>
struct PpCur {
  Src S;
  uint32_t pos, end;
  DN_HD_INLINE uint8_t peek() const { return pos < end ? S.at(pos) : 0; }
  DN_HD_INLINE void ws() {
    while (pos < end) {
      const uint8_t b = S.at(pos);
      if (b != ' ' && b != '\t') break;
      pos++;
    }
  }
  // skip blanks; is the next byte c?
  DN_HD_INLINE bool next_is(uint8_t c) {
    ws();
    return pos < end && S.at(pos) == c;
  }
  DN_HD_INLINE bool lit(uint8_t c) {
    if (!next_is(c)) return false;
    pos++;
    return true;
  }
};

// ---- tokens -------------------------------------------------------------------

// A string whose opening quote is consumed: its span, the cursor behind
// the closing quote.  False: an escape, a control byte, ill-formed UTF-8 or
// no closing quote.
template <class Src>
DN_HD_INLINE bool pp_string(PpCur<Src>& c, uint32_t& start, uint32_t& len) {
  start = c.pos;
  uint32_t need = 0, lo = 0x80, hi = 0xBF;  // a sequence under way
  while (c.pos < c.end) {
    const uint32_t b = c.S.at(c.pos);
    if (need) {
      if (b < lo || b > hi) return false;
      lo = 0x80; hi = 0xBF;
      need--;
    } else if (b == '"') {
      len = c.pos - start;
      c.pos++;
      return true;
    } else if (b == '\\' || b < 0x20) { return false;
    } else if (b < 0x80) {
    } else if (b >= 0xC2 && b <= 0xDF) { need = 1;
    } else if (b == 0xE0) { need = 2; lo = 0xA0;
    } else if (b == 0xED) { need = 2; hi = 0x9F;
    } else if (b >= 0xE1 && b <= 0xEF) { need = 2;
    } else if (b == 0xF0) { need = 3; lo = 0x90;
    } else if (b == 0xF4) { need = 3; hi = 0x8F;
    } else if (b >= 0xF1 && b <= 0xF3) { need = 3;
    } else { return false; }
    c.pos++;
  }
  return false;
}

// Bytes [at, at + n) of the source against w; the caller has at + n <= end.
template <class Src>
DN_HD_INLINE bool pp_same(Src S, uint32_t at, const uint8_t* w, uint32_t n) {
  for (uint32_t k = 0; k < n; k++)
    if (S.at(at + k) != w[k]) return false;
  return true;
}

template <class Src>
DN_HD_INLINE bool pp_word(PpCur<Src>& c, const char* w, uint32_t n) {
  if (c.end - c.pos < n ||
      !pp_same(c.S, c.pos, reinterpret_cast<const uint8_t*>(w), n))
    return false;
  c.pos += n;
  return true;
}

template <class Src>
DN_HD_INLINE bool pp_digits(PpCur<Src>& c) {
  const uint32_t p0 = c.pos;
  while (c.pos < c.end) {
    const uint8_t b = c.S.at(c.pos);
    if (b < '0' || b > '9') break;
    c.pos++;
  }
  return c.pos > p0;
}

// One scalar value by the JSON grammar; false for anything else.
template <class Src>
DN_HD_INLINE bool pp_value(PpCur<Src>& c, PpTok& t) {
  c.ws();
  t.start = c.pos;
  t.len = 0;
  const uint8_t b = c.peek();
  if (b == '"') {
    c.pos++;
    t.type = PP_T_STR;
    return pp_string(c, t.start, t.len);
  }
  if (b == 't') {
    t.type = PP_T_TRUE;
    if (!pp_word(c, "true", 4)) return false;
  } else if (b == 'f') {
    t.type = PP_T_FALSE;
    if (!pp_word(c, "false", 5)) return false;
  } else if (b == 'n') {
    t.type = PP_T_NULL;
    if (!pp_word(c, "null", 4)) return false;
  } else if (b == '-' || (b >= '0' && b <= '9')) {
    if (b == '-') c.pos++;
    const uint32_t d0 = c.pos;
    if (!pp_digits(c)) return false;
    if (c.S.at(d0) == '0' && c.pos - d0 > 1) return false;  // 01
    t.type = PP_T_INT;
    if (c.peek() == '.') {
      c.pos++;
      if (!pp_digits(c)) return false;
      t.type = PP_T_FLT;
    }
    if (c.peek() == 'e' || c.peek() == 'E') {
      c.pos++;
      if (c.peek() == '+' || c.peek() == '-') c.pos++;
      if (!pp_digits(c)) return false;
      t.type = PP_T_FLT;
    }
  } else {
    return false;  // nested, NaN, Infinity, garbage
  }
  t.len = c.pos - t.start;
  return true;
}

// An integer literal (PP_T_INT) as sign and magnitude; false when it has
// more than 19 digits.
template <class Src>
DN_HD_INLINE bool pp_int(Src S, const PpTok& t, bool& neg, uint64_t& mag) {
  uint32_t p = t.start;
  const uint32_t e = t.start + t.len;
  neg = S.at(p) == '-';
  if (neg) p++;
  mag = 0;
  if (e - p > 19) return false;
  for (; p < e; p++) mag = mag * 10u + (uint64_t)(S.at(p) - '0');
  return true;
}

// A number literal (PP_T_INT, PP_T_FLT) as the nearest double; false when
// it has more than 19 significant digits, or lies in [1e308, 1e309), where
// only the rounding tells whether float() overflows.  `inf`: the literal
// is 1e309 or more in magnitude, infinite for float(); this is decided on
// the decimal exponent, v is then 0 and no infinity ever enters the
// arithmetic.
template <class Src>
DN_HD_INLINE bool pp_double(Src S, const PpTok& t, double& v, bool& inf) {
  uint32_t p = t.start;
  const uint32_t e = t.start + t.len;
  const bool neg = S.at(p) == '-';
  if (neg) p++;
  uint64_t mant = 0;
  int ndig = 0;
  long ex = 0;
  bool frac = false;
  for (; p < e; p++) {
    const uint8_t b = S.at(p);
    if (b == '.') { frac = true; continue; }
    if (b < '0' || b > '9') break;
    if (ndig == 19) return false;
    mant = mant * 10u + (uint64_t)(b - '0');
    ndig += mant != 0;
    if (frac) ex--;
  }
  if (p < e) {  // e or E
    p++;
    bool eneg = false;
    if (S.at(p) == '+' || S.at(p) == '-') { eneg = S.at(p) == '-'; p++; }
    long e10 = 0;
    for (; p < e; p++)
      if (e10 < 100000) e10 = e10 * 10 + (S.at(p) - '0');
    ex += eneg ? -e10 : e10;
  }
  // mant has ndig digits: the value lies in [10^(top - 1), 10^top)
  const long top = ex + ndig;
  inf = mant != 0 && top > 309;
  v = 0.0;
  if (inf) return true;
  if (mant != 0 && top == 309) return false;
  v = scale10(mant, ex);
  if (neg) v = -v;
  return true;
}

// ---- the walk -----------------------------------------------------------------

// The whole stripped line against the grammar; every field of "fields"
// goes to V.field and the value to V.value.  False: punt.
template <class Src, class Visit>
DN_HD_INLINE bool pp_walk(PpCur<Src>& c, Visit& V) {
  if (!c.lit('{')) return false;
  bool have_fields = false, have_value = false;
  if (c.next_is('}')) {
    c.pos++;
  } else {
    for (;;) {
      uint32_t ks, kl;
      if (!c.lit('"') || !pp_string(c, ks, kl) || !c.lit(':')) return false;
      if (kl == 6 && pp_same(c.S, ks,
                             reinterpret_cast<const uint8_t*>("fields"), 6)) {
        if (have_fields) return false;
        have_fields = true;
        if (!c.lit('{')) return false;
        if (c.next_is('}')) {
          c.pos++;
        } else {
          for (;;) {
            uint32_t ns, nl;
            PpTok t;
            if (!c.lit('"') || !pp_string(c, ns, nl) || !c.lit(':') ||
                !pp_value(c, t))
              return false;
            V.field(c.S, ns, nl, t);
            if (c.next_is(',')) { c.pos++; continue; }
            if (!c.lit('}')) return false;
            break;
          }
        }
      } else if (kl == 5 &&
                 pp_same(c.S, ks,
                         reinterpret_cast<const uint8_t*>("value"), 5)) {
        if (have_value) return false;
        have_value = true;
        PpTok t;
        if (!pp_value(c, t)) return false;
        V.value(c.S, t);
      } else {
        return false;
      }
      if (c.next_is(',')) { c.pos++; continue; }
      if (!c.lit('}')) return false;
      break;
    }
  }
  c.ws();
  return c.pos == c.end;
}

// First walk: the last __dn_metric, and the value.
struct PpFindMetric {
  PpTok metric;
  bool have_value, value_ok;
  uint64_t vmag;
  template <class Src>
  DN_HD_INLINE void field(Src S, uint32_t ns, uint32_t nl, const PpTok& t) {
    if (nl == 11 &&
        pp_same(S, ns, reinterpret_cast<const uint8_t*>("__dn_metric"), 11))
      metric = t;
  }
  template <class Src>
  DN_HD_INLINE void value(Src S, const PpTok& t) {
    have_value = true;
    bool neg;
    value_ok = t.type == PP_T_INT && pp_int(S, t, neg, vmag) && !neg &&
               vmag < PP_2_53;
  }
};

// Second walk: a token per column of metric m, the last of a name.
struct PpMatch {
  const PpSpecs* P;
  int m;
  PpTok tok[MAX_KEY];
  template <class Src>
  DN_HD_INLINE void field(Src S, uint32_t ns, uint32_t nl, const PpTok& t) {
#pragma unroll
    for (int j = 0; j < MAX_KEY; j++)
      if (j < P->nk[m] && nl == P->name_len[m][j] &&
          pp_same(S, ns, P->names + P->name_off[m][j], nl))
        tok[j] = t;
  }
  template <class Src>
  DN_HD_INLINE void value(Src, const PpTok&) {}
};

// ---- sinks: what the two passes do with a taken line ------------------------

struct PpCount {
  uint32_t spans;
  DN_HD_INLINE void take(const PpRow& r) {
    spans = (uint32_t)__builtin_popcount(r.strmask);
  }
};

struct PpStore {
  int* metric;          // this row's
  long long* row;       // this row's kmax + 1 words
  double* val;          // this row's
  long long* span_start;
  long long* span_len;
  uint32_t span_base;   // this row's first span
  uint32_t n_spans;     // spans in all
  int kmax;
  DN_HD_INLINE void take(const PpRow& r) {
    uint32_t k = span_base;
    long long tags = 0;
#pragma unroll
    for (int j = 0; j < MAX_KEY; j++) {
      if (j >= kmax) break;
      long long v = r.el[j];
      if ((r.strmask >> j) & 1u) {
        if (k < n_spans) {
          span_start[k] = (long long)r.sstart[j];
          span_len[k] = (long long)r.slen[j];
        }
        v = (long long)k++;
        tags |= 1ll << (2 * j);  // _EL_STR
      }
      row[j] = v;
    }
    row[kmax] = tags;
    *metric = r.metric;
    *val = r.value;
  }
};

// ---- one line --------------------------------------------------------------------

// [lo, hi) without the space, tab and CR at its ends.
template <class Src>
DN_HD_INLINE void pp_strip(Src S, uint32_t& lo, uint32_t& hi) {
  while (lo < hi) {
    const uint8_t b = S.at(lo);
    if (b != ' ' && b != '\t' && b != '\r') break;
    lo++;
  }
  while (hi > lo) {
    const uint8_t b = S.at(hi - 1);
    if (b != ' ' && b != '\t' && b != '\r') break;
    hi--;
  }
}

// The class of line [lo, hi), already stripped; `metric` is set for DROP
// and TAKEN, and a TAKEN line goes to the sink.  tail is where the caller's
// `undefined` lies.
template <class Src, class Sink>
DN_HD_INLINE uint8_t pp_line(Src S, uint32_t lo, uint32_t hi,
                             const PpSpecs& P, uint32_t tail, int& metric,
                             Sink& out) {
  metric = -1;
  if (lo == hi) return PP_SKIP;
  if (hi - lo > PP_MAX_LINE) return PP_PUNT;
  PpFindMetric f;
  f.metric.type = PP_T_MISSING;
  f.metric.start = f.metric.len = 0;
  f.have_value = false;
  f.value_ok = true;
  f.vmag = 0;
  {
    PpCur<Src> c = {S, lo, hi};
    if (!pp_walk(c, f) || !f.value_ok) return PP_PUNT;
  }
  if (f.metric.type == PP_T_TRUE || f.metric.type == PP_T_FALSE)
    return PP_PUNT;  // isinstance(True, int)
  if (f.metric.type != PP_T_INT) return PP_SKIP;
  bool neg;
  uint64_t mag;
  if (!pp_int(S, f.metric, neg, mag)) return PP_SKIP;  // 20 digits: no metric
  if ((neg && mag) || mag >= (uint64_t)P.nm) return PP_SKIP;
  if (!f.have_value) return PP_PUNT;  // KeyError in Python
  const int m = (int)mag, nk = P.nk[m];
  PpMatch mt;
  mt.P = &P;
  mt.m = m;
#pragma unroll
  for (int j = 0; j < MAX_KEY; j++) {
    mt.tok[j].type = PP_T_MISSING;
    mt.tok[j].start = mt.tok[j].len = 0;
  }
  {
    PpCur<Src> c = {S, lo, hi};
    if (!pp_walk(c, mt)) return PP_PUNT;  // the same bytes: true again
  }
  PpRow r;
  r.metric = metric = m;
  r.value = (double)f.vmag;
  r.strmask = 0;
#pragma unroll
  for (int j = 0; j < MAX_KEY; j++) {
    r.el[j] = 0;
    r.sstart[j] = r.slen[j] = 0;
  }
#pragma unroll
  for (int j = 0; j < MAX_KEY; j++) {
    if (j >= nk) break;
    const PpTok t = mt.tok[j];
    const int kind = P.kind[m][j];
    const bool number = t.type == PP_T_INT || t.type == PP_T_FLT;
    double num = 0.0;
    bool inf = false;
    if (t.type == PP_T_INT) {
      if (!pp_int(S, t, neg, mag) || mag > PP_2_53) return PP_PUNT;
      num = neg ? -(double)mag : (double)mag;
    } else if (t.type == PP_T_FLT) {
      if (kind == PP_COL_PLAIN || !pp_double(S, t, num, inf)) return PP_PUNT;
      if (inf && kind == PP_COL_DATE) return PP_PUNT;  // int(inf) raises
    }
    if (kind >= PP_COL_QUANTIZE) {
      if (t.type == PP_T_STR) return PP_PUNT;  // krill.to_number: the host's
      if (!number || inf) return PP_DROP;
      const double q = bucket_ordinal(
          kind == PP_COL_QUANTIZE ? BUCKET_P2 : BUCKET_LIN, num, P.step[m][j]);
      if (!(__builtin_fabs(q) < PP_2_62)) return PP_PUNT;
      r.el[j] = (long long)q;
    } else if (number && kind == PP_COL_DATE) {
      const double q = __builtin_trunc(num);
      if (!(__builtin_fabs(q) < PP_2_62)) return PP_PUNT;  // NaN: neither
      r.el[j] = (long long)q;
    } else {
      if (number && neg && mag == 0) return PP_PUNT;  // -0 prints as 0
      r.strmask |= 1u << j;
      r.sstart[j] = t.type == PP_T_MISSING ? tail : t.start;
      r.slen[j] = t.type == PP_T_MISSING ? PP_TAIL : t.len;
    }
  }
  out.take(r);
  return PP_TAKEN;
}

#if defined(__HIPCC__)

// meta words (u64), read by the host
enum PpMeta : int { PP_M_NL = 0, PP_M_LINES, PP_M_TAKEN, PP_M_SPANS,
                    PP_M_PUNTS, PP_M_WIDE, PP_M_WORDS };

struct PpArgs {
  const uint8_t* text;   // 16-byte aligned; data, then `undefined`
  uint32_t data_len;
  const PpSpecs* specs;
  int kmax;
  uint32_t nseg;         // newline segments
  uint32_t* seg_scan;    // [round8(nseg + 1)], zeros; counts, scanned
  uint32_t* seg_sums;
  unsigned long long* meta;      // [PP_M_WORDS]
  unsigned long long* counters;  // [nm, 2], zeros
  // known after sync 1
  uint32_t n_nl, n_lines;
  uint32_t* nl_pos;      // [n_nl]
  uint8_t* cls;          // [n_lines]
  uint32_t n8;           // round8(n_lines + 1)
  uint32_t* scan;        // [3 * n8], zeros: taken, spans, punts
  uint32_t* sums;
  // known after sync 2
  uint32_t n_taken, n_spans, n_punts;
  int* metric;           // [n_taken]
  long long* rows;       // [n_taken, kmax + 1]
  double* vals;          // [n_taken]
  long long* span_start; // [n_spans]
  long long* span_len;
  long long* punts;      // [n_punts, 2]
};

// High bit of every byte of w that is '\n'; no carry crosses a byte.
DEV uint32_t pp_nl_mask(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t y = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return ~(y | x | 0x7F7F7F7Fu);
}

// The newline masks of the 16 bytes lane `lane` takes of half `half` of
// segment `seg`; bytes at or past data_len count as none.
DEV uint32_t pp_nl_unit(const PpArgs& A, uint32_t seg, int half,
                        uint32_t lane, uint32_t (&m)[4]) {
  const uint32_t at = seg * PP_NL_SEG + (uint32_t)half * 1024u + lane * 16u;
  m[0] = m[1] = m[2] = m[3] = 0;
  if (at < A.data_len) {
    const uint4 v = unify_load16(A.text, (long long)A.data_len, (long long)at);
    m[0] = pp_nl_mask(v.x);
    m[1] = pp_nl_mask(v.y);
    m[2] = pp_nl_mask(v.z);
    m[3] = pp_nl_mask(v.w);
  }
  return at;
}

// A wave per segment, lane-consecutive 16-byte loads.
__launch_bounds__(PP_BLOCK)
__global__ void parse_nl_count_kernel(PpArgs A) {
  const uint32_t seg = blockIdx.x * (PP_BLOCK / 64) + (threadIdx.x >> 6);
  if (seg >= A.nseg) return;  // wave-uniform
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t cnt = 0, m[4];
#pragma unroll
  for (int half = 0; half < 2; half++) {
    pp_nl_unit(A, seg, half, lane, m);
    cnt += __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0) A.seg_scan[seg] = cnt;
}

__global__ void parse_lines_kernel(PpArgs A) {
  if (threadIdx.x || blockIdx.x) return;
  const unsigned long long n_nl =
      A.seg_scan[A.nseg] + A.seg_sums[A.nseg / SORT_SCAN_TILE];
  A.meta[PP_M_NL] = n_nl;
  A.meta[PP_M_LINES] = n_nl + (A.text[A.data_len - 1] != '\n' ? 1u : 0u);
}

__launch_bounds__(PP_BLOCK)
__global__ void parse_nl_write_kernel(PpArgs A) {
  const uint32_t seg = blockIdx.x * (PP_BLOCK / 64) + (threadIdx.x >> 6);
  if (seg >= A.nseg) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t w_at = A.seg_scan[seg] + A.seg_sums[seg / SORT_SCAN_TILE];
#pragma unroll
  for (int half = 0; half < 2; half++) {
    uint32_t m[4];
    const uint32_t base = pp_nl_unit(A, seg, half, lane, m);
    const uint32_t cnt =
        __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = __shfl_up(incl, off, 64);
      if ((int)lane >= off) incl += t;
    }
    uint32_t at = w_at + incl - cnt;
#pragma unroll
    for (int wi = 0; wi < 4; wi++) {
      uint32_t mm = m[wi];
      while (mm) {
        const uint32_t b = ((uint32_t)__ffs(mm) - 1) >> 3;
        if (at < A.n_nl) A.nl_pos[at] = base + (uint32_t)wi * 4u + b;
        at++;
        mm &= mm - 1;
      }
    }
    w_at += __shfl(incl, 63, 64);
  }
}

// Line i is [pp_lo, pp_hi), i < n_lines; both within data_len, lo <= hi.
DEV uint32_t pp_hi(const PpArgs& A, uint32_t i) {
  return i < A.n_nl ? min(A.nl_pos[i], A.data_len) : A.data_len;
}
DEV uint32_t pp_lo(const PpArgs& A, uint32_t i) {
  return i ? min(A.nl_pos[i - 1] + 1u, pp_hi(A, i)) : 0u;
}

// Entry i of part k of the scan, relative to the part's first entry.
DEV uint32_t pp_at(const PpArgs& A, uint32_t k, uint32_t i) {
  const uint32_t a = k * A.n8, b = a + i;
  return A.scan[b] + A.sums[b / SORT_SCAN_TILE] -
         (A.scan[a] + A.sums[a / SORT_SCAN_TILE]);
}

// A block's tile: lines [row0, row0 + m), bytes [tlo, thi); this lane's
// line i is [lo, hi) within them.  `fits`: the bytes from the 16-byte
// boundary `base` at or below tlo fit the stage; block-uniform.
struct PpTile {
  uint32_t i, lo, hi, base, thi;
  bool live, fits;
};

DEV PpTile pp_tile(const PpArgs& A) {
  PpTile T;
  const uint32_t row0 = blockIdx.x * PP_BLOCK;
  const uint32_t m = min((uint32_t)PP_BLOCK, A.n_lines - row0);
  const uint32_t tlo = pp_lo(A, row0);
  T.i = row0 + threadIdx.x;
  T.live = threadIdx.x < m;
  T.thi = pp_hi(A, row0 + m - 1);
  T.base = tlo & ~15u;
  T.fits = T.thi - T.base <= (uint32_t)PP_STAGE_BYTES;
  T.lo = T.hi = 0;
  if (T.live) {
    T.lo = max(pp_lo(A, T.i), tlo);
    T.hi = min(pp_hi(A, T.i), T.thi);
    T.lo = min(T.lo, T.hi);
  }
  return T;
}

// The bytes [base, thi) of a tile that fits, lane-consecutive.
DEV void pp_stage_in(const PpArgs& A, uint4* stage, const PpTile& T) {
  const uint32_t units = (T.thi - T.base + 15u) >> 4;
  for (uint32_t u = threadIdx.x; u < units; u += PP_BLOCK)
    stage[u] = unify_load16(A.text, (long long)A.data_len,
                            (long long)T.base + 16ll * u);
  __syncthreads();
}

// The measure pass over one tile from source S: class, span count and
// the scan's three inputs per line, the metric counters per wave.
template <class Src>
DEV void pp_measure(const PpArgs& A, const PpTile& T, Src S) {
  uint8_t cls = PP_SKIP;
  int metric = -1;
  PpCount cnt = {0};
  if (T.live) {
    uint32_t lo = T.lo, hi = T.hi;
    pp_strip(S, lo, hi);
    cls = pp_line(S, lo, hi, *A.specs, A.data_len, metric, cnt);
    A.cls[T.i] = cls;
    A.scan[T.i] = cls == PP_TAKEN ? 1u : 0u;
    A.scan[A.n8 + T.i] = cnt.spans;
    A.scan[2 * A.n8 + T.i] = cls == PP_PUNT ? 1u : 0u;
  }
  const bool counted = T.live && (cls == PP_TAKEN || cls == PP_DROP);
  for (int k = 0; k < A.specs->nm; k++) {  // uniform
    const unsigned long long in = __ballot(counted && metric == k);
    const unsigned long long non =
        __ballot(counted && metric == k && cls == PP_DROP);
    if (__lane_id() == 0) {
      if (in) atomicAdd(&A.counters[2 * k], (unsigned long long)__popcll(in));
      if (non)
        atomicAdd(&A.counters[2 * k + 1], (unsigned long long)__popcll(non));
    }
  }
}

// The tiles that fit the stage; the others are parse_measure_global_kernel's.
__launch_bounds__(PP_BLOCK)
__global__ void parse_measure_kernel(PpArgs A) {
  __shared__ uint4 stage[PP_STAGE_BYTES / 16];
  const PpTile T = pp_tile(A);
  if (!T.fits) return;  // block-uniform
  pp_stage_in(A, stage, T);
  pp_measure(A, T, PpStage{reinterpret_cast<const uint8_t*>(stage), T.base});
}

// The tiles that do not fit, from global memory; says in meta that there
// are such tiles, so the host launches parse_emit_global_kernel.
__launch_bounds__(PP_BLOCK)
__global__ void parse_measure_global_kernel(PpArgs A) {
  const PpTile T = pp_tile(A);
  if (T.fits) return;  // block-uniform
  if (threadIdx.x == 0) atomicOr(&A.meta[PP_M_WIDE], 1ull);
  pp_measure(A, T, PpGlobal{A.text});
}

__global__ void parse_totals_kernel(PpArgs A) {
  if (threadIdx.x || blockIdx.x) return;
  A.meta[PP_M_TAKEN] = pp_at(A, 0, A.n_lines);
  A.meta[PP_M_SPANS] = pp_at(A, 1, A.n_lines);
  A.meta[PP_M_PUNTS] = pp_at(A, 2, A.n_lines);
}

// The emit pass over one tile from source S: a taken line is parsed again
// into the store sink, a punted line gives its stripped byte range.
template <class Src>
DEV void pp_emit(const PpArgs& A, const PpTile& T, Src S) {
  if (!T.live) return;
  const uint8_t cls = A.cls[T.i];
  uint32_t lo = T.lo, hi = T.hi;
  pp_strip(S, lo, hi);
  if (cls == PP_TAKEN) {
    const uint32_t t = pp_at(A, 0, T.i);
    if (t >= A.n_taken) return;
    PpStore st = {A.metric + t, A.rows + (size_t)t * (size_t)(A.kmax + 1),
                  A.vals + t, A.span_start, A.span_len, pp_at(A, 1, T.i),
                  A.n_spans, A.kmax};
    int metric;
    pp_line(S, lo, hi, *A.specs, A.data_len, metric, st);
  } else if (cls == PP_PUNT) {
    const uint32_t p = pp_at(A, 2, T.i);
    if (p < A.n_punts) {
      A.punts[2 * (size_t)p] = (long long)lo;
      A.punts[2 * (size_t)p + 1] = (long long)hi;
    }
  }
}

__launch_bounds__(PP_BLOCK)
__global__ void parse_emit_kernel(PpArgs A) {
  __shared__ uint4 stage[PP_STAGE_BYTES / 16];
  const PpTile T = pp_tile(A);
  if (!T.fits) return;  // block-uniform
  pp_stage_in(A, stage, T);
  pp_emit(A, T, PpStage{reinterpret_cast<const uint8_t*>(stage), T.base});
}

__launch_bounds__(PP_BLOCK)
__global__ void parse_emit_global_kernel(PpArgs A) {
  const PpTile T = pp_tile(A);
  if (T.fits) return;  // block-uniform
  pp_emit(A, T, PpGlobal{A.text});
}

#endif  // __HIPCC__

}  // namespace dn
