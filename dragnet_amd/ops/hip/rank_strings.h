// String ranking layer: the rank of every dictionary string in byte
// order, a most-significant-first sort of variable-length byte strings on
// top of the fixed-width row sort (sort_rows.h).  render_points' lines come
// out in Aggregator.points()'s order, strings by code point, which is
// UTF-8 byte order; this layer gives sort_rows the rank of each string in
// that order without the dictionary leaving the device.  The first part
// (rank_load8, rank_key, rank_compare) is plain C++17 under a host
// compiler (tools_dev/rank_host_check.cpp); the kernels are DEVICE ONLY.
//
//   rank_key_kernel     active strings -> rows (group, key of 7 bytes)
//   rank_bound_kernel   sorted rows -> run-head and still-tied flags
//   rank_heads_kernel   scanned head flags -> the position of every head
//   rank_assign_kernel  ranks of the resolved, the next round's active list
//   rank_finish_kernel  small tied groups: each member counts its smaller
//
// between them sort_span_kernel, the passes of sort_rows.h (sort_passes in
// the binding, w = 2) and sort_scan_kernel / sort_scan_sums_kernel, all
// used as they are.
//
//  * Contract.  blob uint8 [bytes] and offs int64 [G + 1] are a dictionary
//    in wire form; rank[i] = the number of strings smaller than string i,
//    bytes compared unsigned, a proper prefix before the longer string:
//    sorted(range(G), key=items.__getitem__) inverted.  One string twice
//    sets RANK_DUPLICATE and leaves the ranks unspecified.  offs that do
//    not start at 0, descend, or end beyond the blob set RANK_BAD_DICT; a
//    string whose span is bad is not read.
//  * Rounds.  Round d looks at bytes [7d, 7d + 7) of the strings still
//    tied after round d - 1 (the active list; all G in round 0).  A tie
//    group is the set of active strings equal so far; its members are
//    contiguous in the active list, groups ascend, and `group` is the
//    final rank of the group's first member, 0 in round 0.
//  * Key.  A string with r = len - 7d bytes left gets the 64-bit key whose
//    high 56 bits are its next 7 bytes, big-endian, zero-padded, and whose
//    low byte is min(r, 8).  Unsigned order of the key is byte order on
//    the chunk: the low byte tells "a" < "a\0" < "a\0\0" apart, puts a
//    string that ends with the chunk (7) before one that goes on (8), and
//    an empty remainder is key 0.  Equal keys with low byte 8 are still
//    tied; with a low byte below 8 they are one string twice.  The passes
//    order signed words, so the key is stored with bit 63 flipped
//    (SORT_SIGN): a leading byte of 0x80 or above sorts after ASCII.
//  * Loading.  The 7 bytes sit at any byte offset.  The blob is taken as
//    aligned 64-bit words from its 16-byte-aligned base: the word that
//    holds the first byte, the next one when the chunk reaches into it, a
//    funnel shift, a byte swap and a mask of the bytes at or past the
//    string's end.  A word is read only when it holds a byte below the
//    string's end, hence below `bytes`: nothing at or past blob +
//    round_up(bytes, 8) is ever read.  The binding guarantees that much
//    memory: a blob that is not 16-byte aligned, or whose length is no
//    multiple of 8, is copied into a buffer of round_up(bytes, 8) bytes.
//  * One round.  rank_key_kernel writes the row (group, key) of each
//    active string into an int64 [m, 2] array, the layout the row sort
//    takes: sort_span_kernel finds the bytes that vary, sort_passes
//    returns the stable permutation; a constant group column (round 0)
//    costs no pass, a round of m <= SORT_TILE strings is one block.
//    Sorting by (group, key) leaves every group in the places it had, so
//    place p of the sorted order has the group of active entry p.
//    rank_bound_kernel takes the sorted rows, neighbours by shuffle: the
//    head flag of p is "differs from p - 1", the tied flag is "equals a
//    neighbour and low byte 8"; equal to p - 1 with a low byte below 8
//    raises RANK_DUPLICATE.  Both flag arrays are one array of 2 * m8
//    counts (m8 = m + 1 rounded up to 8), scanned in one go by the scan
//    kernels of sort_rows.h; the tied half is read relative to its first
//    entry.  rank_heads_kernel writes headpos[run] = p for every head and
//    m behind the last.  rank_assign_kernel: place p in run `run` with
//    head h; h - gstart (gstart: where p's group starts in the active
//    list) is the head's place among the group's rows, and group + that is
//    the final rank of the run's first member: the rank of a resolved
//    string (a run of one, or an ended string), and the new group of a
//    tied one, which goes, stably, to entry scan(tied)[p] of the next
//    active list with gstart = scan(tied)[h].
//  * One sync a round.  The next count, the longest tied run, the status
//    word and the span words of the NEXT round's rows share one small meta
//    array: rank_key_kernel and sort_span_kernel of the next round are
//    enqueued behind rank_assign_kernel, sized for m and reading the true
//    count on the device, and one D2H copy brings all of it.
//  * Finish.  A long shared prefix (URL paths, host names) would cost a
//    round per 7 bytes.  Once no tied group has more than RANK_FINISH_MAX
//    strings, rank_finish_kernel ends the sort in one launch: a thread per
//    active entry q compares its string, from the current depth, 8 bytes a
//    step to the end of the shorter, with every member of its group, and
//    its rank is group + the members smaller; an equal member raises
//    RANK_DUPLICATE.  The group is the run of entries with q's gstart: it
//    starts at gstart[q] and ends before the first j with gstart[j] !=
//    gstart[q] (or the list's end), so the thread walks j up from
//    gstart[q] and needs no length.  Thread q is entry q: the lanes of a
//    wave are neighbouring members of a run, walk the same j and load the
//    same other string (one broadcast), each comparing it with its own.
//    Groups above the cutoff go on in global rounds, however many their
//    common prefix takes: slow (a sync and a dozen launches per 7 bytes)
//    but correct.
//
// G < 2^31 - 16 (2 * m8 counts are indexed in u32); blob offsets are
// 64-bit.
#pragma once
#include "dev_util.h"
#if defined(__HIPCC__)
#include "sort_rows.h"
#endif

namespace dn {

constexpr int RANK_CHUNK = 7;         // string bytes per round
constexpr int RANK_FINISH_MAX = 64;   // largest tied group the finish takes
constexpr uint32_t RANK_BAD_DICT = 1u, RANK_DUPLICATE = 2u;
constexpr uint64_t RANK_SIGN = 1ull << 63;  // = SORT_SIGN

// meta words (u64): the span of the rows (AND c0, AND c1, OR c0, OR c1),
// the active count, the status bits, the longest tied run
enum RankMeta : int {
  RANK_M_SPAN = 0, RANK_M_COUNT = 4, RANK_M_STATUS = 5, RANK_M_MAXRUN = 6,
  RANK_M_WORDS = 8,
};

// The 8 bytes of the blob from byte `at`, the first one highest; bytes at
// or past `end` are 0.  words is the blob as aligned little-endian 64-bit
// words; only words that hold a byte of [at, end) are read.
DN_HD_INLINE uint64_t rank_load8(const uint64_t* words, int64_t at,
                                 int64_t end) {
  if (at >= end) return 0;
  const int64_t w = at >> 3;
  const int sh = (int)(at & 7) * 8;
  uint64_t v = words[w] >> sh;
  if (sh && (w + 1) * 8 < end) v |= words[w + 1] << (64 - sh);
  v = __builtin_bswap64(v);
  const int64_t n = end - at;
  if (n < 8) v &= ~0ull << (8 * (8 - n));
  return v;
}

// The round key of the string [start, end) at `depth` bytes, bit 63
// flipped for the signed passes.
DN_HD_INLINE uint64_t rank_key(const uint64_t* words, int64_t start,
                               int64_t end, int64_t depth) {
  const int64_t at = start + depth;
  const int64_t r = end > at ? end - at : 0;
  const uint64_t v = rank_load8(words, at, end);
  return ((v & ~0xffull) | (uint64_t)(r < 8 ? r : 8)) ^ RANK_SIGN;
}

// Byte order of [a, a_end) against [b, b_end): -1, 0 or 1.
DN_HD_INLINE int rank_compare(const uint64_t* words, int64_t a, int64_t a_end,
                              int64_t b, int64_t b_end) {
  for (;;) {
    const uint64_t va = rank_load8(words, a, a_end);
    const uint64_t vb = rank_load8(words, b, b_end);
    if (va != vb) return va < vb ? -1 : 1;
    // equal with the padding: the one that ends first is the prefix
    const int64_t na = a_end - a < 8 ? a_end - a : 8;
    const int64_t nb = b_end - b < 8 ? b_end - b : 8;
    if (na != nb) return na < nb ? -1 : 1;
    if (na < 8) return 0;
    a += 8;
    b += 8;
  }
}

#if defined(__HIPCC__)

constexpr int RANK_BLOCK = 256;

// entry i of a scanned array: the block's scan plus the block's base
DEV uint32_t rank_scanned(const uint32_t* scan, const uint32_t* sums,
                          uint32_t i) {
  return scan[i] + sums[i / SORT_SCAN_TILE];
}

// The span of string s, or false (and RANK_BAD_DICT) when offs is bad
// there: the string is then not read.
DEV bool rank_span(const long long* offs, long long bytes, uint32_t s,
                   long long& a, long long& b, unsigned long long* meta) {
  a = offs[s];
  b = offs[s + 1];
  const bool ok = a >= 0 && a <= b && b <= bytes && (s != 0 || a == 0);
  if (!ok) atomicOr(&meta[RANK_M_STATUS], (unsigned long long)RANK_BAD_DICT);
  return ok;
}

// rows[i] = (group, key at depth) of active entry i, for i below the
// count in meta (capped by n_cap).  act == nullptr: round 0, entry i is
// string i and every group is 0.
__launch_bounds__(RANK_BLOCK)
__global__ void rank_key_kernel(const uint64_t* words, long long bytes,
                                const long long* offs, const uint32_t* act,
                                const uint32_t* grp, uint32_t n_cap,
                                long long depth, longlong2* rows,
                                unsigned long long* meta) {
  const uint32_t n = min(n_cap, (uint32_t)meta[RANK_M_COUNT]);
  const uint32_t i = blockIdx.x * RANK_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = act ? act[i] : i;
  long long a, b;
  longlong2 row;
  row.x = grp ? (long long)grp[i] : 0;
  row.y = (long long)RANK_SIGN;  // key 0
  if (rank_span(offs, bytes, s, a, b, meta))
    row.y = (long long)rank_key(words, a, b, depth);
  rows[i] = row;
}

// Place p of the sorted order, p < m8: scan[p] = 1 at the head of a run of
// equal rows, scan[m8 + p] = 1 where p goes to the next round; both 0 from
// m up.  sid[p] = the string at place p.  Resets the span words and the
// longest run for the round to come.
__launch_bounds__(RANK_BLOCK)
__global__ void rank_bound_kernel(const longlong2* rows,
                                  const uint32_t* perm, const uint32_t* act,
                                  uint32_t m, uint32_t m8, uint32_t* scan,
                                  uint32_t* sid, unsigned long long* meta) {
  const uint32_t p = blockIdx.x * RANK_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  if (p == 0) {
    meta[RANK_M_SPAN + 0] = ~0ull;
    meta[RANK_M_SPAN + 1] = ~0ull;
    meta[RANK_M_SPAN + 2] = 0;
    meta[RANK_M_SPAN + 3] = 0;
    meta[RANK_M_MAXRUN] = 0;
  }
  longlong2 me = {0, 0};
  uint32_t src = 0;
  if (p < m) {
    src = perm[p];
    me = rows[src];
  }
  longlong2 prev, next;  // of the neighbouring lanes; the wave's ends load
  prev.x = __shfl_up(me.x, 1, 64);
  prev.y = __shfl_up(me.y, 1, 64);
  next.x = __shfl_down(me.x, 1, 64);
  next.y = __shfl_down(me.y, 1, 64);
  if (p >= m8) return;
  if (p >= m) {
    scan[p] = 0;
    scan[m8 + p] = 0;
    return;
  }
  if (lane == 0 && p > 0) prev = rows[perm[p - 1]];
  if (lane == 63 && p + 1 < m) next = rows[perm[p + 1]];
  const bool eqp = p > 0 && prev.x == me.x && prev.y == me.y;
  const bool eqn = p + 1 < m && next.x == me.x && next.y == me.y;
  const bool goes_on = ((unsigned long long)me.y & 0xffull) == 8;
  scan[p] = eqp ? 0u : 1u;
  scan[m8 + p] = ((eqp || eqn) && goes_on) ? 1u : 0u;
  sid[p] = act ? act[src] : src;
  if (eqp && !goes_on)
    atomicOr(&meta[RANK_M_STATUS], (unsigned long long)RANK_DUPLICATE);
}

// headpos[run] = the place of the run's head; headpos[runs] = m.
__launch_bounds__(RANK_BLOCK)
__global__ void rank_heads_kernel(const uint32_t* scan, const uint32_t* sums,
                                  uint32_t m, uint32_t* headpos) {
  const uint32_t p = blockIdx.x * RANK_BLOCK + threadIdx.x;
  if (p >= m) return;
  const uint32_t v0 = rank_scanned(scan, sums, p);
  const uint32_t v1 = rank_scanned(scan, sums, p + 1);
  if (v1 != v0) headpos[v0] = p;
  if (p == m - 1) headpos[v1] = m;
}

// Place p < m: the rank of its string if it is resolved, else its entry
// of the next active list (nact, ngrp, ngstart).  grp / gstart ==
// nullptr: round 0, one group from 0.  Leaves the next count and the
// longest tied run in meta.
__launch_bounds__(RANK_BLOCK)
__global__ void rank_assign_kernel(const uint32_t* scan, const uint32_t* sums,
                                   const uint32_t* headpos,
                                   const uint32_t* sid, const uint32_t* grp,
                                   const uint32_t* gstart, uint32_t m,
                                   uint32_t m8, long long* rank,
                                   uint32_t* nact, uint32_t* ngrp,
                                   uint32_t* ngstart,
                                   unsigned long long* meta) {
  const uint32_t p = blockIdx.x * RANK_BLOCK + threadIdx.x;
  if (p >= m) return;
  const uint32_t t0 = rank_scanned(scan, sums, m8);
  if (p == 0)
    meta[RANK_M_COUNT] = rank_scanned(scan, sums, m8 + m) - t0;
  const uint32_t run = rank_scanned(scan, sums, p + 1) - 1;
  const uint32_t h = headpos[run];
  const uint32_t first = (grp ? grp[p] : 0u) + (h - (gstart ? gstart[p] : 0u));
  const uint32_t tq = rank_scanned(scan, sums, m8 + p);
  if (rank_scanned(scan, sums, m8 + p + 1) == tq) {
    rank[sid[p]] = (long long)first;
    return;
  }
  const uint32_t q = tq - t0;
  nact[q] = sid[p];
  ngrp[q] = first;
  ngstart[q] = rank_scanned(scan, sums, m8 + h) - t0;
  if (p == h)
    atomicMax(&meta[RANK_M_MAXRUN],
              (unsigned long long)(headpos[run + 1] - h));
}

// Active entry q, below the count in meta (capped by n_cap): rank = group
// + the members of its group smaller than it from `depth` on.
__launch_bounds__(RANK_BLOCK)
__global__ void rank_finish_kernel(const uint64_t* words, long long bytes,
                                   const long long* offs,
                                   const uint32_t* act, const uint32_t* grp,
                                   const uint32_t* gstart, uint32_t n_cap,
                                   long long depth, long long* rank,
                                   unsigned long long* meta) {
  const uint32_t n = min(n_cap, (uint32_t)meta[RANK_M_COUNT]);
  const uint32_t q = blockIdx.x * RANK_BLOCK + threadIdx.x;
  if (q >= n) return;
  const uint32_t s = act[q];
  long long a, a_end;
  if (!rank_span(offs, bytes, s, a, a_end, meta)) return;
  const uint32_t gs = gstart[q];
  uint32_t smaller = 0;
  bool twice = false;
  for (uint32_t j = gs; j < n && gstart[j] == gs; j++) {
    if (j == q) continue;
    long long b, b_end;
    if (!rank_span(offs, bytes, act[j], b, b_end, meta)) continue;
    const int c = rank_compare(words, b + depth, b_end, a + depth, a_end);
    smaller += c < 0 ? 1u : 0u;
    twice |= c == 0;
  }
  rank[s] = (long long)(grp[q] + smaller);
  if (twice)
    atomicOr(&meta[RANK_M_STATUS], (unsigned long long)RANK_DUPLICATE);
}

#endif  // __HIPCC__

}  // namespace dn
