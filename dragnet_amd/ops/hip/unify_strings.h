// Dictionary unification layer, DEVICE ONLY: number the distinct byte
// strings among N spans (start[i], length[i]) of one blob in order of
// first occurrence.  This is the step in front of merge_rows.h: after the
// multi-GPU gather every rank holds the ranks' string dictionaries as
// blobs and offsets, and needs one global dictionary ("first seen first,
// in rank order") and, per rank, the table from its codes to the global
// ones (dragnet_amd/merge.py, unify_dictionaries).
//
//   unify_hash_kernel    spans -> one 64-bit hash each; validates spans
//   unify_insert_kernel  find-or-insert into one open-addressing table
//   unify_flag_kernel    is_first[i] = (i is the lowest index of its class)
//   sort_scan_kernel     } exclusive scan of is_first (sort_rows.h)
//   sort_scan_sums_kernel}
//   unify_emit_kernel    remap[i] = id of i's class, first[id] = i
//
// remap is int64 [N]; first is int64 [G], strictly increasing, with
// remap[first[g]] == g.  The result is what a Python dict loop over the
// strings gives, whatever order the device executes in.
//
//  * Hash, 256 threads, grid-stride over tiles of UNIFY_TILE consecutive
//    strings, one string per lane.  A string is consumed 8 bytes per step
//    through an 8-byte window (UnifySpan): aligned 8-byte words, two of
//    them funnelled by the span's misalignment, the tail zeroed beyond
//    the span's end.  h = (h ^ word) * K, folded by h >> 32, per step;
//    the length goes into the seed and mix64 finishes.  The table is
//    private to one call, so the hash is nobody else's.
//  * Staging.  Lanes reading variable-length spans straight from global
//    memory is the 64-way divergent gather of DESIGN.md's ladder.  Both
//    callers hand over packed, ascending spans, so a tile whose spans are
//    valid and ascending (start[i] >= start[i-1] + length[i-1]) and whose
//    byte range [start[first] & ~15, end[last]) is at most
//    UNIFY_STAGE_BYTES is brought into LDS once, by lane-consecutive
//    16-byte loads, and the lanes hash out of LDS.  Any other tile
//    (descending or overlapping spans, a range beyond the stage, an
//    invalid span) reads global memory through the same window; both
//    sources give the same words, so both paths give the same hash.  The
//    choice is per tile and block-uniform (__syncthreads_and).
//  * Bounds.  A negative start or length, or an end beyond the blob, sets
//    UNIFY_BAD_SPAN and the lane reads nothing.  The blob is 16-byte
//    aligned (the binding sees to it), so an aligned 8- or 16-byte unit
//    lies inside the blob when its end does; the one unit that straddles
//    the blob's end is assembled from byte loads below blob_len.  Nothing
//    outside [blob, blob + blob_len) is read.  The later kernels return at
//    once when the status word is set: they index by what this one
//    validated.
//  * hash_mask is ANDed into the hash before it is stored, so a narrow
//    mask (tests) makes true equal-hash collisions, not only shared home
//    slots.
//  * Insert.  table is u32[slots], a power of two >= 2N, all UNIFY_EMPTY.
//    A slot holds the INDEX OF A REPRESENTATIVE of one class of equal
//    strings.  Lane i probes linearly from hash[i] & (slots - 1): an empty
//    slot is claimed with atomicCAS(slot, EMPTY, i); a slot holding j
//    matches iff hash[j] == hash[i], the lengths are equal and the bytes
//    are equal (word-wise from global memory, only on a hash match); on a
//    match atomicMin(slot, i) (skipped when j < i: a slot only goes
//    down, so 25 hot strings do not take an atomic per row), otherwise
//    the next slot.
//    No claim-and-publish protocol (agg_insert_slot's CLAIMED / READY) is
//    needed: the payload is the kernel's read-only input, written before
//    the launch, so any index read from a slot can be compared against at
//    once.  A slot's class never changes: it is set from EMPTY by one CAS
//    and afterwards only lowered by lanes that have just compared equal to
//    its holder.  Hence whichever index a reader sees in a slot, the
//    outcome of its comparison is the same; two lanes of a class walk the
//    same probe sequence past the same foreign classes and meet in the
//    same slot, one by CAS and the other by comparison.  slots >= 2N, so
//    a free slot always exists and the walk is bounded.
//  * Order.  After the kernel every class's slot holds the class's lowest
//    index (atomicMin over all its members), which no execution order can
//    change.  is_first marks those; the exclusive scan of is_first at a
//    first occurrence is its id; remap[i] is the id of table[slot_of[i]].
//    The scan is sort_rows.h's: is_first is padded with zeros to a
//    multiple of 8, each block of SORT_SCAN_TILE is scanned in place, the
//    block sums are scanned beside it, and the emit kernel adds the two,
//    being their only reader.  It also leaves G in meta[0], which the
//    host reads with the status word in one copy.
//
// N < 2^31; indices and slots are u32, starts and lengths int64.
#pragma once
#include "sort_rows.h"

namespace dn {

constexpr int UNIFY_TILE = 256;              // strings per tile = threads
constexpr int UNIFY_STAGE_BYTES = 32 * 1024; // LDS stage of one tile
constexpr uint32_t UNIFY_EMPTY = 0xFFFFFFFFu;
constexpr uint64_t UNIFY_K1 = 0x9E3779B97F4A7C15ull;
constexpr uint64_t UNIFY_K2 = 0xFF51AFD7ED558CCDull;

// status word bits
constexpr uint32_t UNIFY_BAD_SPAN = 1;  // a span outside the blob
constexpr uint32_t UNIFY_FULL = 2;      // no free slot (slots < n: a bug)

struct UnifyArgs {
  const uint8_t* blob;       // 16-byte aligned
  long long blob_len;
  const long long* start;    // [n]
  const long long* length;   // [n]
  uint32_t n;
  uint64_t hash_mask;
  unsigned long long* hash;  // [n]
  uint32_t* table;           // [slot_mask + 1], UNIFY_EMPTY
  uint32_t slot_mask;
  uint32_t* slot_of;         // [n]
  uint32_t* status;
};

// Aligned 8-byte word j of the blob; bytes at or beyond blob_len are 0
// and are not read.
struct UnifyGlobalWords {
  const uint8_t* blob;
  long long blob_len;
  DEV uint64_t word(long long j) const {
    const long long at = j * 8;
    if (at + 8 <= blob_len)
      return *reinterpret_cast<const uint64_t*>(blob + at);
    uint64_t v = 0;
    for (int b = 0; b < 8; b++)
      if (at + b < blob_len) v |= (uint64_t)blob[at + b] << (8 * b);
    return v;
  }
};

// The same words out of the LDS stage, which starts at word base_word.
struct UnifyLdsWords {
  const uint64_t* stage;
  long long base_word;
  DEV uint64_t word(long long j) const { return stage[j - base_word]; }
};

// The 8-byte window over one span: next() gives its next 8 bytes, little
// end first, zero beyond the span's end.  A word is fetched only when it
// holds a byte of the span.
template <class Words>
struct UnifySpan {
  Words W;
  long long j, end, left;
  uint32_t sh;
  uint64_t a0;
  DEV UnifySpan(Words W_, long long s, long long l)
      : W(W_), j(s >> 3), end(s + l), left(l),
        sh((uint32_t)(s & 7) * 8u), a0(0) {
    if (l > 0) a0 = W.word(j);
  }
  DEV uint64_t next() {
    const uint64_t a1 = (j + 1) * 8 < end ? W.word(j + 1) : 0;
    uint64_t v = sh ? (a0 >> sh) | (a1 << (64u - sh)) : a0;
    if (left < 8) v &= (1ull << (8 * (uint32_t)left)) - 1;
    left -= 8;
    j++;
    a0 = a1;
    return v;
  }
};

template <class Words>
DEV uint64_t unify_hash_span(Words W, long long s, long long l) {
  uint64_t h = FNV_OFFSET ^ ((uint64_t)l * UNIFY_K1);
  UnifySpan<Words> span(W, s, l);
  for (long long k = 0; k < l; k += 8) {
    h = (h ^ span.next()) * UNIFY_K2;
    h ^= h >> 32;
  }
  return mix64(h);
}

// Two spans of one length, byte for byte.
DEV bool unify_same_bytes(UnifyGlobalWords W, long long sa, long long sb,
                          long long l) {
  UnifySpan<UnifyGlobalWords> a(W, sa, l), b(W, sb, l);
  for (long long k = 0; k < l; k += 8)
    if (a.next() != b.next()) return false;
  return true;
}

// The 16 bytes at `at` (a multiple of 16, below blob_len); bytes at or
// beyond blob_len are 0 and are not read.
DEV uint4 unify_load16(const uint8_t* blob, long long blob_len,
                       long long at) {
  if (at + 16 <= blob_len) return *reinterpret_cast<const uint4*>(blob + at);
  const UnifyGlobalWords W = {blob, blob_len};
  const uint64_t lo = W.word(at >> 3);
  const uint64_t hi = at + 8 < blob_len ? W.word((at >> 3) + 1) : 0;
  uint4 v;
  v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32);
  v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
  return v;
}

__launch_bounds__(UNIFY_TILE)
__global__ void unify_hash_kernel(UnifyArgs A) {
  __shared__ uint4 stage[UNIFY_STAGE_BYTES / 16];
  const uint32_t tid = threadIdx.x;
  const UnifyGlobalWords G = {A.blob, A.blob_len};
  bool bad = false;
  const uint32_t ntiles = (A.n + UNIFY_TILE - 1) / UNIFY_TILE;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t row0 = t * UNIFY_TILE;
    const uint32_t m = min((uint32_t)UNIFY_TILE, A.n - row0);
    const uint32_t i = row0 + tid;
    const bool live = tid < m;
    long long s = 0, l = 0;
    bool ok = true;  // this lane lets the tile be staged
    if (live) {
      s = A.start[i];
      l = A.length[i];
      if (s < 0 || l < 0 || s > A.blob_len || l > A.blob_len - s) {
        bad = true;
        ok = false;
        s = 0;
        l = 0;
      } else if (tid > 0) {
        const long long ps = A.start[i - 1], pl = A.length[i - 1];
        ok = ps >= 0 && pl >= 0 && ps <= s && pl <= s - ps;
      }
    }
    // also the barrier behind the last tile's readers of the stage
    bool staged = __syncthreads_and(ok);
    long long base = 0, bytes = 0;
    if (staged) {  // block-uniform; every span of the tile is valid
      base = A.start[row0] & ~15ll;
      bytes = A.start[row0 + m - 1] + A.length[row0 + m - 1] - base;
      staged = bytes <= UNIFY_STAGE_BYTES;
    }
    uint64_t h;
    if (staged) {
      const uint32_t units = (uint32_t)((bytes + 15) >> 4);
      for (uint32_t u = tid; u < units; u += UNIFY_TILE)
        stage[u] = unify_load16(A.blob, A.blob_len, base + 16ll * u);
      __syncthreads();
      const UnifyLdsWords L = {reinterpret_cast<const uint64_t*>(stage),
                               base >> 3};
      h = unify_hash_span(L, s, l);
    } else {
      h = unify_hash_span(G, s, l);
    }
    if (live) A.hash[i] = h & A.hash_mask;
  }
  if (__ballot(bad) && __lane_id() == 0) atomicOr(A.status, UNIFY_BAD_SPAN);
}

__launch_bounds__(UNIFY_TILE)
__global__ void unify_insert_kernel(UnifyArgs A) {
  if (atomic_load_relaxed(A.status) & UNIFY_BAD_SPAN) return;
  const UnifyGlobalWords G = {A.blob, A.blob_len};
  const uint32_t mask = A.slot_mask;
  bool full = false;
  const uint32_t stride = gridDim.x * UNIFY_TILE;
  for (uint32_t i = blockIdx.x * UNIFY_TILE + threadIdx.x; i < A.n;
       i += stride) {
    const unsigned long long h = A.hash[i];
    const long long s = A.start[i], l = A.length[i];
    uint32_t slot = (uint32_t)h & mask;
    bool found = false;
    for (uint32_t probes = 0; probes <= mask; probes++) {
      uint32_t j = atomic_load_relaxed(&A.table[slot]);
      if (j == UNIFY_EMPTY) {
        j = atomicCAS(&A.table[slot], UNIFY_EMPTY, i);
        if (j == UNIFY_EMPTY) { found = true; break; }
      }
      // j is an index of the slot's class, now and ever after
      if (A.hash[j] == h && A.length[j] == l &&
          unify_same_bytes(G, s, A.start[j], l)) {
        // a slot only ever goes down: below i already, it stays there
        if (i < j) atomicMin(&A.table[slot], i);
        found = true;
        break;
      }
      slot = (slot + 1) & mask;
    }
    if (!found) { full = true; slot = 0; }
    A.slot_of[i] = slot;
  }
  if (__ballot(full) && __lane_id() == 0) atomicOr(A.status, UNIFY_FULL);
}

// is_first[i] for i < n, 0 for n <= i < n8 (n rounded up to 8).
__launch_bounds__(UNIFY_TILE)
__global__ void unify_flag_kernel(const uint32_t* table,
                                  const uint32_t* slot_of, uint32_t n,
                                  uint32_t n8, const uint32_t* status,
                                  uint32_t* is_first) {
  if (*status) return;
  const uint32_t i = blockIdx.x * UNIFY_TILE + threadIdx.x;
  if (i >= n8) return;
  is_first[i] = (i < n && table[slot_of[i]] == i) ? 1u : 0u;
}

// scan / sums: what the two scan kernels left of is_first.  meta[0] = G.
__launch_bounds__(UNIFY_TILE)
__global__ void unify_emit_kernel(const uint32_t* table,
                                  const uint32_t* slot_of, uint32_t n,
                                  const uint32_t* scan, const uint32_t* sums,
                                  const uint32_t* status, long long* remap,
                                  long long* first, uint32_t* meta) {
  if (*status) return;
  const uint32_t i = blockIdx.x * UNIFY_TILE + threadIdx.x;
  if (i >= n) return;
  const uint32_t rep = table[slot_of[i]];
  const uint32_t id = scan[rep] + sums[rep / SORT_SCAN_TILE];
  remap[i] = (long long)id;
  if (rep == i) first[id] = (long long)i;
  if (i == n - 1)
    meta[0] = scan[i] + sums[i / SORT_SCAN_TILE] + (rep == i ? 1u : 0u);
}

}  // namespace dn
