// Row re-aggregation layer, DEVICE ONLY: group identical int64 rows and
// sum their f64 values.  This is the step after the multi-GPU gather
// (dragnet_amd/merge.py, reaggregate): every rank holds the union
// of the per-rank aggregate tables as dense rows [codes..., tagpack] and
// needs the distinct rows with the sum of the values over each.
//
//   merge_insert_kernel   rows -> one global open-addressing table
//   merge_compact_kernel  table -> dense (row, sum) arrays, any order
//
// A row is w = nk + 1 words of 64 bits, nk <= MAX_KEY; the last word is
// the tag pack, 2 bits per key element.  Rows may arrive in segments,
// one per sending rank, each with its own string dictionary: an element
// tagged MERGE_EL_STR is then an index into its segment's slice of
// `remap` and is replaced by the global code before it is hashed or
// stored.  A code outside the slice is never used as an index: the row
// is left out and MERGE_BAD_CODE is set in the status word.
//
// Insert kernel, 256 threads, grid-stride over tiles of 256 rows:
//
//  * Staging.  A tile is 256*w*8 contiguous bytes, 16-byte aligned (the
//    binding checks the base).  Lane-consecutive 16-byte global loads
//    bring it in; each 16 bytes is two row words, stored to LDS as two
//    8-byte writes because a pair may straddle two rows.  A partial last
//    tile of m rows holds m*w words; when that is odd its last word is
//    half a 16-byte unit and is loaded on its own, 8 bytes, so nothing
//    past the array is read.
//    LDS row stride S = w | 1 words (w if odd, w + 1 if even).  When
//    thread t then reads word k of row t, a wave touches the 8-byte
//    words t*S + k.  An LDS pass serves 256 bytes = 32 such words, a
//    64-lane b64 read is two passes of 32 lanes, and t*S mod 32 is a
//    permutation of 0..31 over 32 consecutive t exactly when S is odd.
//    An even S = 8 would put the 32 lanes on 4 words' banks (8-way).
//    The staging writes have word stride 2 (2-way), once per tile word.
//  * Each thread takes its row into registers (9 words at most; the
//    loops are unrolled to MERGE_W with a k < w guard so that key[]
//    never becomes an indexed stack array), remaps, hashes (mix64
//    chained over the w words, then & hash_mask) and finds or claims its
//    slot: state u32[slots], keys i64[slots*w], sum f64[slots], with the
//    claim-and-publish protocol of agg_insert_slot (scan_tables.h).  A
//    hit compares all w words, 64 bits each.  slots >= 2n, so a free
//    slot always exists and the probe loop is bounded by slots.
//  * Combining is keyed by the SLOT INDEX, which names a key exactly, so
//    no stage in front of the table can mix two keys up.  First a wave
//    elects one leader per distinct slot (ballot/shuffle loop); a group
//    of more than one lane sums its values with a shuffle butterfly, a
//    group of one skips it, so an all-distinct wave pays only the
//    election.  The leader adds the group's sum into a per-block LDS
//    table of (slot, partial sum), MERGE_CACHE entries, 4 probes, LDS
//    f64 adds.  The table lives across all the block's tiles and is
//    flushed with one global f64 atomicAdd per live entry at block end.
//    A full or conflicting entry falls through to a direct global add:
//    at high cardinality most rows do, and the table costs them 4 LDS
//    probes each.
//  * Exactness.  Device adds come in no fixed order.  A sum is
//    independent of the order exactly when every partial sum is exact,
//    which holds when all values are non-negative integers and the total
//    stays below 2^53.  A value that is negative, fractional, NaN or
//    >= 2^53 sets MERGE_INEXACT (one atomic per wave, by ballot, at the
//    end of the kernel); so does a slot total >= 2^53 in the compact
//    kernel.  With non-negative terms no partial sum can exceed 2^53
//    and then come back under it unseen.  The caller discards an inexact
//    result.
#pragma once
#include "common.h"
#include "dev_util.h"

namespace dn {

constexpr int MERGE_W = MAX_KEY + 1;     // most words of a row
constexpr int MERGE_TILE = 256;          // rows per tile = threads
constexpr int MERGE_CACHE = 1024;        // per-block (slot, sum) entries
constexpr int MERGE_CACHE_PROBES = 4;
constexpr uint32_t MERGE_NO_SLOT = 0xFFFFFFFFu;
constexpr long long MERGE_EL_STR = 1;    // merge.py _EL_STR

// status word bits
constexpr uint32_t MERGE_BAD_CODE = 1;   // string code outside its remap
constexpr uint32_t MERGE_INEXACT = 2;    // sums may depend on add order
constexpr uint32_t MERGE_FULL = 4;       // no free slot (slots < n: a bug)

constexpr double MERGE_EXACT_LIMIT = 9007199254740992.0;  // 2^53

struct MergeTable {
  uint32_t* state;   // [slots]
  long long* keys;   // [slots * w]
  double* sum;       // [slots]
  uint32_t slots;    // power of two, >= 2n
  int w;
};

struct MergeArgs {
  const long long* rows;       // [n * w], 16-byte aligned
  const double* vals;          // [n]
  uint32_t n;
  uint32_t nseg;               // 0: no segments, nothing is remapped
  const uint32_t* seg_start;   // [nseg + 1] first row of each segment
  const long long* remap;      // the segments' tables, concatenated
  const long long* remap_off;  // [nseg + 1] start of each table
  uint64_t hash_mask;
  MergeTable T;
  uint32_t* status;
};

// LDS row stride in words: odd (header comment)
DEV int merge_row_stride(int w) { return w | 1; }

// Find the row's slot or claim a free one; MERGE_NO_SLOT when the probe
// has gone round the whole table.
DEV uint32_t merge_find_or_insert(const MergeTable& T,
                                  const long long (&key)[MERGE_W],
                                  uint64_t hash_mask) {
  const int w = T.w;
  uint64_t h = FNV_OFFSET;
#pragma unroll
  for (int k = 0; k < MERGE_W; k++)
    if (k < w) h = mix64(h ^ (uint64_t)key[k]);
  const uint32_t mask = T.slots - 1;
  uint32_t s = (uint32_t)(h & hash_mask) & mask;
  for (uint32_t probes = 0; probes < T.slots; probes++, s = (s + 1) & mask) {
    long long* slot_keys = T.keys + (size_t)s * w;
    while (true) {
      uint32_t st = atomic_load_relaxed(&T.state[s]);
      if (st == SLOT_READY) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < MERGE_W; k++)
          if (k < w && atomic_load_relaxed(&slot_keys[k]) != key[k])
            same = false;
        if (same) return s;
        break;  // another key's slot: next probe
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&T.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
#pragma unroll
          for (int k = 0; k < MERGE_W; k++)
            if (k < w) atomic_store_relaxed(&slot_keys[k], key[k]);
          drain_stores();
          atomic_store_relaxed(&T.state[s], SLOT_READY);
          return s;
        }
        continue;  // lost the race: re-read state
      }
      // claimed by another lane, which publishes without waiting
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return MERGE_NO_SLOT;
}

// Sum of v over the lanes of the wave where in_group holds.
DEV double merge_group_sum(bool in_group, double v) {
  double x = in_group ? v : 0.0;
#pragma unroll
  for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__launch_bounds__(MERGE_TILE)
__global__ void merge_insert_kernel(MergeArgs A) {
  __shared__ long long tile[MERGE_TILE * MERGE_W];
  __shared__ uint32_t cache_slot[MERGE_CACHE];
  __shared__ double cache_sum[MERGE_CACHE];

  const int w = A.T.w;
  const int nk = w - 1;
  const int S = merge_row_stride(w);
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < (uint32_t)MERGE_CACHE; i += MERGE_TILE) {
    cache_slot[i] = MERGE_NO_SLOT;
    cache_sum[i] = 0.0;
  }

  bool inexact = false, bad_code = false, full = false;
  const uint32_t ntiles = (A.n + MERGE_TILE - 1) / MERGE_TILE;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t row0 = t * MERGE_TILE;
    const uint32_t m = min((uint32_t)MERGE_TILE, A.n - row0);
    const uint32_t nw = m * (uint32_t)w;  // words of this tile
    const long long* src = A.rows + (size_t)row0 * w;
    __syncthreads();  // the last tile's readers (and the cache init)
    const longlong2* src2 = reinterpret_cast<const longlong2*>(src);
    for (uint32_t c = tid; c < nw / 2; c += MERGE_TILE) {
      longlong2 v = src2[c];
      uint32_t r = (2 * c) / (uint32_t)w, k = 2 * c - r * (uint32_t)w;
      tile[r * S + k] = v.x;
      if (++k == (uint32_t)w) { k = 0; r++; }
      tile[r * S + k] = v.y;
    }
    if ((nw & 1u) && tid == 0) tile[(m - 1) * S + nk] = src[nw - 1];
    __syncthreads();

    bool valid = tid < m;
    long long key[MERGE_W];
#pragma unroll
    for (int k = 0; k < MERGE_W; k++)
      key[k] = (valid && k < w) ? tile[tid * S + k] : 0;
    double v = valid ? A.vals[row0 + tid] : 0.0;

    if (valid && A.nseg != 0) {
      bool bad = false;
      long long tags = 0;
#pragma unroll
      for (int k = 0; k < MERGE_W; k++)
        if (k == nk) tags = key[k];
      uint32_t seg = file_ordinal(A.seg_start, A.nseg, row0 + tid);
      long long base = A.remap_off[seg];
      long long len = A.remap_off[seg + 1] - base;
#pragma unroll
      for (int k = 0; k < MAX_KEY; k++) {
        if (k < nk && ((tags >> (2 * k)) & 3) == MERGE_EL_STR) {
          long long code = key[k];
          if (code >= 0 && code < len) key[k] = A.remap[base + code];
          else bad = true;
        }
      }
      if (bad) { bad_code = true; valid = false; }
    }

    uint32_t slot = MERGE_NO_SLOT;
    if (valid) {
      if (!(v >= 0.0 && v < MERGE_EXACT_LIMIT && v == trunc(v)))
        inexact = true;
      slot = merge_find_or_insert(A.T, key, A.hash_mask);
      if (slot == MERGE_NO_SLOT) { full = true; valid = false; }
    }

    // one leader per distinct slot of the wave, carrying the group's sum
    bool leader = false;
    uint64_t unproc = __ballot(valid);
    while (unproc) {
      int src_lane = (int)(__ffsll((long long)unproc) - 1);
      uint32_t src_slot = __shfl(slot, src_lane, 64);
      bool same = valid && slot == src_slot;
      uint64_t grp = __ballot(same);
      if (__popcll(grp) > 1) {  // wave-uniform
        double gsum = merge_group_sum(same, v);
        if (same) v = gsum;
      }
      if ((int)__lane_id() == src_lane) leader = true;
      unproc &= ~grp;
    }

    if (leader) {
      bool cached = false;
      uint32_t ci = (uint32_t)mix64(slot) & (MERGE_CACHE - 1);
#pragma unroll 1
      for (int p = 0; p < MERGE_CACHE_PROBES; p++) {
        uint32_t prev = atomicCAS(&cache_slot[ci], MERGE_NO_SLOT, slot);
        if (prev == MERGE_NO_SLOT || prev == slot) {
          atomicAdd(&cache_sum[ci], v);
          cached = true;
          break;
        }
        ci = (ci + 1) & (MERGE_CACHE - 1);
      }
      if (!cached) atomicAdd(&A.T.sum[slot], v);
    }
  }

  __syncthreads();
  for (uint32_t i = tid; i < (uint32_t)MERGE_CACHE; i += MERGE_TILE) {
    uint32_t s = cache_slot[i];
    if (s != MERGE_NO_SLOT) atomicAdd(&A.T.sum[s], cache_sum[i]);
  }

  uint32_t bits = 0;
  if (__ballot(bad_code)) bits |= MERGE_BAD_CODE;
  if (__ballot(inexact)) bits |= MERGE_INEXACT;
  if (__ballot(full)) bits |= MERGE_FULL;
  if (bits && __lane_id() == 0) atomicOr(A.status, bits);
}

// One thread per slot: READY slots are written densely to out_rows /
// out_sums.  A wave reserves its rows with one atomicAdd on out_n[0];
// a lane's place among them is the count of READY lanes below it.
__global__ void merge_compact_kernel(MergeTable T, long long* out_rows,
                                     double* out_sums, uint32_t* out_n,
                                     uint32_t* status) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const int w = T.w;
  const bool ready = s < T.slots && T.state[s] == SLOT_READY;
  const uint64_t mask = __ballot(ready);
  if (mask == 0) return;
  const uint32_t lane = __lane_id();
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(out_n, (uint32_t)__popcll(mask));
  base = __shfl(base, 0, 64);
  bool inexact = false;
  if (ready) {
    const uint32_t i = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
    const long long* k_in = T.keys + (size_t)s * w;
    long long* k_out = out_rows + (size_t)i * w;
    for (int k = 0; k < w; k++) k_out[k] = k_in[k];
    double sum = T.sum[s];
    out_sums[i] = sum;
    inexact = !(sum >= 0.0 && sum < MERGE_EXACT_LIMIT);
  }
  if (__ballot(inexact) && lane == 0) atomicOr(status, MERGE_INEXACT);
}

}  // namespace dn
