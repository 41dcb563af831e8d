// Number formatting layer, DEVICE ONLY: f64 values to their JavaScript
// strings (dbl2dec.h: ECMAScript Number::toString, what plan.number_key
// gives on the host) as one byte blob with offsets, the form a dictionary
// has on the wire.  String i is text[offs[i] : offs[i + 1]].
//
//   format_measure_kernel   a number per lane: dn_decimal_of once, the
//                           decimal form parked (12 bytes), its length
//   sort_scan_kernel        the lengths, per 2048 numbers (sort_rows.h)
//   format_totals_kernel    the block sums -> int64 bases; the total -> meta
//   (the host reads meta: its one sync, and sizes text exactly)
//   format_emit_kernel      parked forms -> text, offs
//
//  * Convert once.  The shortest-digits search (three 64x128-bit products
//    and the table entry) runs in the measuring pass only.  That pass
//    parks digits (u64) and exponent, sign and kind (one u32) per number,
//    and the emit pass lays the string out from those: dn_js_layout is the
//    one routine behind both the counted and the stored bytes, so the
//    stores fill exactly what was measured.
//  * Staging.  A tile is 256 consecutive numbers; its strings are one
//    contiguous range of text of at most 256 * DN_JS_MAX = 6400 bytes.
//    Lanes lay their strings out in an LDS stage placed as text is (byte 0
//    of the stage is text byte lo & ~15) and the block stores the range
//    with render_points.h's ren_stage_out: lane-consecutive 16-byte stores,
//    the ragged first and last unit by bytes.  Every tile fits the stage
//    (FMT_STAGE_BYTES = 6400 + 16), so there is no global-memory path.
//  * Variants, for measurements (tools_dev/ab_format_numbers.py; the
//    binding's `variant`, 0 in use).  FMT_RECOMPUTE: nothing is parked and
//    the emit pass converts again.  FMT_LDS_TABLE: each block first copies
//    the 9872-byte power table into LDS and multiplies from there.
//    profiles/r17_format_numbers.md has both comparisons.
//  * Bounds.  n < 2^31.  A string is at most 25 bytes, so 2048 lengths sum
//    in u32; across blocks the offsets are int64 (format_totals_kernel).
//    Every bit pattern of a double has a string: there is nothing to
//    refuse and no status word.  text is 16-byte aligned.
//  * No atomics.  All stores are vector stores.
#pragma once
#include "dbl2dec.h"
#include "render_points.h"

namespace dn {

constexpr int FMT_BLOCK = REN_BLOCK;  // numbers per tile = threads
constexpr int FMT_STAGE_BYTES = FMT_BLOCK * DN_JS_MAX + 16;
constexpr int FMT_RECOMPUTE = 1, FMT_LDS_TABLE = 2;  // variant bits
static_assert(FMT_STAGE_BYTES % 16 == 0, "the stage is whole 16-byte units");

struct FmtArgs {
  const double* x;            // [n]
  uint32_t n;
  unsigned long long* dig;    // [n] parked digits
  uint32_t* form;             // [n] parked dn_decimal_pack words
  uint32_t* len_scan;         // [round8(n + 1)], zeros; lengths, scanned
  uint32_t* len_sums;         // [nsums]
  uint32_t nsums;
  long long* base;            // [nsums]
  unsigned long long* meta;   // [1]: the bytes of text
  // allocated once the host has read meta
  uint8_t* text;              // 16-byte aligned
  long long* offs;            // [n + 1]
};

// Offset of string i in text, i in 0..n.
DEV long long fmt_at(const FmtArgs& A, uint32_t i) {
  return (long long)A.len_scan[i] + A.base[i / SORT_SCAN_TILE];
}

struct FmtLdsTable {
  const uint64_t* t;
  DEV void get(int k, uint64_t& hi, uint64_t& lo) const {
    const int at = 2 * (k - DN_POW10_KMIN);
    hi = t[at];
    lo = t[at + 1];
  }
};

// The decimal form of number i, through the table the variant names; tbl
// is the block's LDS copy (filled here, every lane of the block calling).
template <int V>
DEV DnDecimal fmt_decimal(const FmtArgs& A, uint32_t i, bool live,
                          uint64_t* tbl) {
  if (V & FMT_LDS_TABLE) {
    for (uint32_t w = threadIdx.x; w < (uint32_t)DN_POW10_WORDS;
         w += FMT_BLOCK)
      tbl[w] = DN_POW10_128[w];
    __syncthreads();
  }
  const uint64_t bits = live ? (uint64_t)__double_as_longlong(A.x[i]) : 0;
  if (V & FMT_LDS_TABLE) return dn_decimal_of(bits, FmtLdsTable{tbl});
  return dn_decimal_of(bits, DnGlobalTable());
}

template <int V>
__launch_bounds__(FMT_BLOCK)
__global__ void format_measure_kernel(FmtArgs A) {
  __shared__ uint64_t tbl[(V & FMT_LDS_TABLE) ? DN_POW10_WORDS : 1];
  const uint32_t i = blockIdx.x * FMT_BLOCK + threadIdx.x;
  const bool live = i < A.n;
  const DnDecimal d = fmt_decimal<V>(A, i, live, tbl);
  if (!live) return;
  if (!(V & FMT_RECOMPUTE)) {
    A.dig[i] = d.digits;
    A.form[i] = dn_decimal_pack(d);
  }
  DnCount cnt = {0};
  dn_js_layout(d, cnt);
  A.len_scan[i] = cnt.n;
}

// One block: exclusive scan of the scan blocks' u32 sums into int64 bases,
// and the byte total for the host.
__launch_bounds__(SORT_BLOCK)
__global__ void format_totals_kernel(FmtArgs A) {
  __shared__ unsigned long long wsum[SORT_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint32_t b0 = 0; b0 < A.nsums; b0 += SORT_BLOCK) {
    const uint32_t i = b0 + threadIdx.x;
    const unsigned long long v = i < A.nsums ? A.len_sums[i] : 0;
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
    if (i < A.nsums) A.base[i] = (long long)(carry + pre + incl - v);
    carry += all;
  }
  if (threadIdx.x == 0) A.meta[0] = carry;
}

template <int V>
__launch_bounds__(FMT_BLOCK)
__global__ void format_emit_kernel(FmtArgs A) {
  __shared__ uint4 stage[FMT_STAGE_BYTES / 16];
  __shared__ uint64_t tbl[(V & FMT_LDS_TABLE) && (V & FMT_RECOMPUTE)
                              ? DN_POW10_WORDS : 1];
  const uint32_t row0 = blockIdx.x * FMT_BLOCK, i = row0 + threadIdx.x;
  const uint32_t m = min((uint32_t)FMT_BLOCK, A.n - row0);
  const bool live = threadIdx.x < m;
  const long long lo = fmt_at(A, row0), hi = fmt_at(A, row0 + m);
  const long long base = lo & ~15ll;
  DnDecimal d = {0, 0, DN_NUM_ZERO, false};
  if (V & FMT_RECOMPUTE)
    d = fmt_decimal<V>(A, i, live, tbl);
  else if (live)
    d = dn_decimal_unpack(A.dig[i], A.form[i]);
  if (live) {
    const long long at = fmt_at(A, i);
    A.offs[i] = at;
    if (i == A.n - 1) A.offs[A.n] = hi;
    // the tile's strings tile [lo, hi): one writer per byte, and
    // hi - base <= 15 + 256 * DN_JS_MAX < FMT_STAGE_BYTES
    DnStore w = {reinterpret_cast<uint8_t*>(stage) + (at - base)};
    dn_js_layout(d, w);
  }
  __syncthreads();
  ren_stage_out(A.text, stage, lo, hi);
}

}  // namespace dn
