// Row ordering layer, DEVICE ONLY: a stable LSD radix sort of a row
// permutation.  Rows are w <= MERGE_W int64 words; they compare column 0
// first, each word as a signed int64, which is np.lexsort(rows.T[::-1])
// and, on distinct rows, np.unique(axis=0)'s order.  merge_rows.h hands
// its distinct rows back in table order; this layer puts them in that
// order without a trip to the host.
//
//   sort_span_kernel     rows -> per-column AND and OR (which bytes vary)
//   sort_small_kernel    n <= SORT_TILE: every pass in one block's LDS
//   sort_key_kernel      (key, idx)[i] = (rows[perm[i]][c], perm[i])
//   sort_hist_kernel     per-tile digit counts, bin-major
//   sort_scan_kernel     } exclusive scan of the counts: per 2048 counts,
//   sort_scan_sums_kernel} then over the block sums
//   sort_scatter_kernel  stable scatter of the (key, idx) pairs
//   sort_gather_kernel   out_rows[i] = rows[perm[i]], out_sums likewise
//
// Digits are 8 bits, so the 256 bins map onto the 256 threads of a block.
//
//  * Span.  Byte b of column c needs a pass only when the column's OR
//    and AND differ in it: ((or ^ and) >> 8b) & 0xff != 0.  Dictionary
//    codes are small and the tag pack is nearly constant, so a real merge
//    takes a handful of passes, not 8w.  A digit is taken from key ^ 2^63,
//    which orders signed words and changes no span.  Each thread folds
//    its rows, a wave reduces by shuffles, and one lane per wave issues
//    one atomicAnd and one atomicOr per column on span[0..w) (AND, set to
//    ~0 by the host) and span[w..2w) (OR, zeroed).
//  * Column at a time, last to first.  A column with a varying byte is
//    gathered once, key[i] = rows[perm[i] * w + c] (the one random read of
//    the rows per column); the (key u64, idx u32) pairs then go through
//    that column's varying bytes, low to high, between two buffers, every
//    pass streaming.  Stable passes over the columns last to first leave
//    the lexicographic order.
//  * Tile.  SORT_TILE = 2048 rows per 256-thread block, 8 per thread,
//    taken in rounds of 256 consecutive rows, so tile order is row order:
//    round, then wave, then lane.
//  * Rank (sort_tile_positions, shared by the scatter and the single-tile
//    kernel).  In each round the lanes of a wave find the lanes with their
//    digit by 8 ballots, one per digit bit; a lane's rank in the wave is
//    the popcount of those peers below it, and the lowest peer writes the
//    group's size to cnt[round][wave][digit] (u16, 16 KB).  After one
//    barrier thread d turns column d of cnt into running sums over
//    (round, wave), which is tile order, and the 256 bin totals are
//    scanned across the block.  A row's place among the tile's rows is
//    binstart[digit] + cnt[round][wave][digit] + rank: no LDS atomic, and
//    a skewed digit costs what a uniform one does.
//  * Scatter.  The pairs are written to LDS at that place, so the tile
//    is grouped by bin; position p of the grouped tile then goes to
//    base[bin][tile] + (p - binstart[bin]): consecutive lanes write
//    consecutive destinations within a bin, runs instead of 64 scattered
//    addresses.  base is the exclusive scan of hist[bin * ntiles + tile]
//    over the flat bin-major array.  The scan leaves each 2048-count block
//    scanned in place and the block sums scanned beside it; the scatter
//    adds the two when it reads a base (the "add" pass of a three-pass
//    scan, folded into its one consumer).  A destination is checked
//    against n before it is written.
//  * The histogram kernel counts in wave-private LDS histograms (LDS
//    atomics), so a skewed digit is not one address for four waves.
//  * Single tile.  With n <= SORT_TILE one block keeps its 8 pairs per
//    thread in registers, reads the span from device memory and runs
//    every pass through LDS: place, write, read back in row order.  One
//    launch instead of three per pass, and no host knowledge of the span.
//  * Gather.  A block takes 256 output rows: the source rows are read
//    word-consecutive (a row's w words by neighbouring lanes) into an LDS
//    tile at merge_row_stride(w), and leave as lane-consecutive 16-byte
//    stores, two words each, the mirror of merge_insert_kernel's staging.
//    An odd last word is stored on its own, 8 bytes.
//
// n < 2^31; the permutation is u32.  Flat histogram indices stay below
// 256 * 2^20 = 2^28.
#pragma once
#include "merge_rows.h"

namespace dn {

constexpr int SORT_BLOCK = 256;               // threads = bins
constexpr int SORT_ROUNDS = 8;                // rows per thread
constexpr int SORT_TILE = SORT_BLOCK * SORT_ROUNDS;
constexpr int SORT_WAVES = SORT_BLOCK / 64;
constexpr int SORT_BINS = 256;
constexpr int SORT_GROUPS = SORT_ROUNDS * SORT_WAVES;  // (round, wave)
constexpr int SORT_SCAN_TILE = 2048;          // counts per scan block
constexpr unsigned long long SORT_SIGN = 1ull << 63;

typedef unsigned long long sort_key_t;

struct SortLds {
  sort_key_t key[SORT_TILE];
  uint32_t idx[SORT_TILE];
  uint16_t cnt[SORT_GROUPS * SORT_BINS];
  uint32_t binstart[SORT_BINS];
  uint32_t gofs[SORT_BINS];
  uint32_t wsum[SORT_WAVES];
};

DEV uint32_t sort_digit(sort_key_t key, int shift) {
  return (uint32_t)((key ^ SORT_SIGN) >> shift) & 0xffu;
}

// Exclusive prefix of v over the 256 threads of the block; wsum is LDS.
// Thread 255's result plus its v is the block total.
DEV uint32_t sort_block_scan(uint32_t v, uint32_t* wsum) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    uint32_t t = __shfl_up(incl, off, 64);
    if ((int)lane >= off) incl += t;
  }
  __syncthreads();  // the last scan's readers of wsum
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t pre = 0;
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)SORT_WAVES; k++)
    if (k < wave) pre += wsum[k];
  return pre + incl - v;
}

// pos[r] = the stable place of the thread's row r (tile row r * 256 +
// tid, one of m) among the tile's rows ordered by the digit at `shift`.
// Leaves L.binstart: the first place of each bin.
DEV void sort_tile_positions(SortLds& L,
                             const sort_key_t (&key)[SORT_ROUNDS],
                             uint32_t m, int shift,
                             uint32_t (&pos)[SORT_ROUNDS]) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  // (round, wave) groups that hold rows: a short tile pays for those
  const uint32_t groups =
      (m + SORT_BLOCK - 1) / SORT_BLOCK * (uint32_t)SORT_WAVES;
  __syncthreads();  // the last pass's readers of cnt and binstart
  uint32_t* zero = reinterpret_cast<uint32_t*>(L.cnt);
  for (uint32_t i = tid; i < groups * (SORT_BINS / 2); i += SORT_BLOCK)
    zero[i] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    pos[r] = 0;
    if ((uint32_t)r * SORT_BLOCK >= m) continue;  // block-uniform
    const bool valid = (uint32_t)r * SORT_BLOCK + tid < m;
    const uint32_t d = sort_digit(key[r], shift);
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t with = __ballot(valid && bit);
      peers &= bit ? with : ~with;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
    if (valid && rank == 0)
      L.cnt[(r * SORT_WAVES + wave) * SORT_BINS + d] =
          (uint16_t)__popcll(peers);
    pos[r] = rank;
  }
  __syncthreads();
  uint32_t run = 0;  // thread = bin
#pragma unroll 4
  for (uint32_t j = 0; j < groups; j++) {
    const uint32_t c = L.cnt[j * SORT_BINS + tid];
    L.cnt[j * SORT_BINS + tid] = (uint16_t)run;
    run += c;
  }
  L.binstart[tid] = sort_block_scan(run, L.wsum);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint32_t d = sort_digit(key[r], shift);
    if ((uint32_t)r * SORT_BLOCK + tid < m)
      pos[r] += L.binstart[d] +
                L.cnt[(r * SORT_WAVES + wave) * SORT_BINS + d];
  }
}

// span[c] &= rows[i][c], span[w + c] |= rows[i][c] over the first n rows;
// n is *n_ptr (capped by n_cap) when n_ptr is given, else n_cap.
__launch_bounds__(SORT_BLOCK)
__global__ void sort_span_kernel(const long long* rows, uint32_t n_cap,
                                 const uint32_t* n_ptr, int w,
                                 unsigned long long* span) {
  uint32_t n = n_cap;
  if (n_ptr) n = min(n, *n_ptr);
  if (blockIdx.x * SORT_BLOCK >= n) return;
  unsigned long long a[MERGE_W], o[MERGE_W];
#pragma unroll
  for (int k = 0; k < MERGE_W; k++) { a[k] = ~0ull; o[k] = 0; }
  const uint32_t stride = gridDim.x * SORT_BLOCK;
  for (uint32_t i = blockIdx.x * SORT_BLOCK + threadIdx.x; i < n;
       i += stride) {
    const long long* row = rows + (size_t)i * w;
#pragma unroll
    for (int k = 0; k < MERGE_W; k++)
      if (k < w) {
        const unsigned long long v = (unsigned long long)row[k];
        a[k] &= v;
        o[k] |= v;
      }
  }
#pragma unroll
  for (int k = 0; k < MERGE_W; k++) {
    if (k < w) {  // wave-uniform
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        a[k] &= __shfl_xor(a[k], off, 64);
        o[k] |= __shfl_xor(o[k], off, 64);
      }
      if (__lane_id() == 0) {
        atomicAnd(&span[k], a[k]);
        atomicOr(&span[w + k], o[k]);
      }
    }
  }
}

// The whole sort of n <= SORT_TILE rows in one block.
__launch_bounds__(SORT_BLOCK)
__global__ void sort_small_kernel(const long long* rows, uint32_t n, int w,
                                  const unsigned long long* span,
                                  uint32_t* perm) {
  __shared__ SortLds L;
  const uint32_t tid = threadIdx.x;
  sort_key_t key[SORT_ROUNDS];
  uint32_t idx[SORT_ROUNDS], pos[SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    idx[r] = (uint32_t)r * SORT_BLOCK + tid;
    key[r] = 0;
  }
  for (int c = w - 1; c >= 0; c--) {
    const unsigned long long diff = span[w + c] ^ span[c];
    if (diff == 0) continue;  // block-uniform, as is every skip below
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; r++)
      if ((uint32_t)r * SORT_BLOCK + tid < n)
        key[r] = (sort_key_t)rows[(size_t)idx[r] * w + c];
    for (int shift = 0; shift < 64; shift += 8) {
      if (((diff >> shift) & 0xffull) == 0) continue;
      sort_tile_positions(L, key, n, shift, pos);
#pragma unroll
      for (int r = 0; r < SORT_ROUNDS; r++)
        if ((uint32_t)r * SORT_BLOCK + tid < n) {
          L.key[pos[r]] = key[r];
          L.idx[pos[r]] = idx[r];
        }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < SORT_ROUNDS; r++) {
        const uint32_t p = (uint32_t)r * SORT_BLOCK + tid;
        if (p < n) {
          key[r] = L.key[p];
          idx[r] = L.idx[p];
        }
      }
      // the next pass writes L.key only after sort_tile_positions'
      // barriers
    }
  }
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint32_t p = (uint32_t)r * SORT_BLOCK + tid;
    if (p < n) perm[p] = idx[r];
  }
}

// Column c through the permutation so far: idx_in == nullptr is the
// identity (the first column sorted).  idx_out may be idx_in.
__launch_bounds__(SORT_BLOCK)
__global__ void sort_key_kernel(const long long* rows, uint32_t n, int w,
                                int c, const uint32_t* idx_in,
                                sort_key_t* key_out, uint32_t* idx_out) {
  const uint32_t i = blockIdx.x * SORT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t src = idx_in ? idx_in[i] : i;
  key_out[i] = (sort_key_t)rows[(size_t)src * w + c];
  idx_out[i] = src;
}

// hist[bin * ntiles + tile] = rows of the tile with that digit
__launch_bounds__(SORT_BLOCK)
__global__ void sort_hist_kernel(const sort_key_t* key, uint32_t n,
                                 int shift, uint32_t* hist,
                                 uint32_t ntiles) {
  __shared__ uint32_t wh[SORT_WAVES][SORT_BINS];
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  const uint32_t tile = blockIdx.x;
  if (tile >= ntiles) return;
#pragma unroll
  for (int k = 0; k < SORT_WAVES; k++) wh[k][tid] = 0;
  __syncthreads();
  const uint32_t row0 = tile * SORT_TILE;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint32_t p = row0 + (uint32_t)r * SORT_BLOCK + tid;
    if (p < n) atomicAdd(&wh[wave][sort_digit(key[p], shift)], 1u);
  }
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int k = 0; k < SORT_WAVES; k++) total += wh[k][tid];
  hist[(size_t)tid * ntiles + tile] = total;
}

// Exclusive scan of a[0..total) in blocks of SORT_SCAN_TILE, in place;
// sums[block] = the block's total.  total is a multiple of 8 (it is
// 256 * ntiles) and a is 16-byte aligned: a thread's 8 counts are two
// 16-byte words, all inside or all outside.
__launch_bounds__(SORT_BLOCK)
__global__ void sort_scan_kernel(uint32_t* a, uint32_t total,
                                 uint32_t* sums) {
  __shared__ uint32_t wsum[SORT_WAVES];
  const uint32_t base = blockIdx.x * SORT_SCAN_TILE + threadIdx.x * 8;
  const bool in = base < total;
  uint4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
  if (in) {
    lo = *reinterpret_cast<const uint4*>(a + base);
    hi = *reinterpret_cast<const uint4*>(a + base + 4);
  }
  const uint32_t s =
      lo.x + lo.y + lo.z + lo.w + hi.x + hi.y + hi.z + hi.w;
  uint32_t at = sort_block_scan(s, wsum);
  if (threadIdx.x == SORT_BLOCK - 1) sums[blockIdx.x] = at + s;
  if (in) {
    uint4 xl, xh;
    xl.x = at; at += lo.x;
    xl.y = at; at += lo.y;
    xl.z = at; at += lo.z;
    xl.w = at; at += lo.w;
    xh.x = at; at += hi.x;
    xh.y = at; at += hi.y;
    xh.z = at; at += hi.z;
    xh.w = at;
    *reinterpret_cast<uint4*>(a + base) = xl;
    *reinterpret_cast<uint4*>(a + base + 4) = xh;
  }
}

// Exclusive scan of the block sums, one block with a running carry.
__launch_bounds__(SORT_BLOCK)
__global__ void sort_scan_sums_kernel(uint32_t* sums, uint32_t nsums) {
  __shared__ uint32_t wsum[SORT_WAVES];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nsums; base += SORT_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nsums ? sums[i] : 0;
    const uint32_t excl = sort_block_scan(v, wsum);
    if (i < nsums) sums[i] = carry + excl;
#pragma unroll
    for (int k = 0; k < SORT_WAVES; k++) carry += wsum[k];
  }
}

// One stable pass: tile `blockIdx.x` of (key_in, idx_in) to its places
// in (key_out, idx_out) by the digit at `shift`.  hist and sums are the
// two levels of the scanned histogram.
__launch_bounds__(SORT_BLOCK)
__global__ void sort_scatter_kernel(const sort_key_t* key_in,
                                    const uint32_t* idx_in,
                                    sort_key_t* key_out, uint32_t* idx_out,
                                    uint32_t n, int shift,
                                    const uint32_t* hist,
                                    const uint32_t* sums,
                                    uint32_t ntiles) {
  __shared__ SortLds L;
  const uint32_t tid = threadIdx.x;
  const uint32_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  const uint32_t row0 = tile * SORT_TILE;
  const uint32_t m = min((uint32_t)SORT_TILE, n - row0);
  sort_key_t key[SORT_ROUNDS];
  uint32_t idx[SORT_ROUNDS], pos[SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint32_t p = (uint32_t)r * SORT_BLOCK + tid;
    key[r] = p < m ? key_in[row0 + p] : 0;
    idx[r] = p < m ? idx_in[row0 + p] : 0;
  }
  sort_tile_positions(L, key, m, shift, pos);
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++)
    if ((uint32_t)r * SORT_BLOCK + tid < m) {
      L.key[pos[r]] = key[r];
      L.idx[pos[r]] = idx[r];
    }
  const uint32_t e = tid * ntiles + tile;  // thread = bin
  // place p of the grouped tile goes to gofs[bin] + p (mod 2^32)
  L.gofs[tid] = hist[e] + sums[e / SORT_SCAN_TILE] - L.binstart[tid];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    const uint32_t p = (uint32_t)r * SORT_BLOCK + tid;
    if (p < m) {
      const sort_key_t k = L.key[p];
      const uint32_t dst = L.gofs[sort_digit(k, shift)] + p;
      if (dst < n) {
        key_out[dst] = k;
        idx_out[dst] = L.idx[p];
      }
    }
  }
}

// out_rows[i] = rows[perm[i]], out_sums[i] = sums[perm[i]] for i < n.
// out_rows is 16-byte aligned.
__launch_bounds__(MERGE_TILE)
__global__ void sort_gather_kernel(const long long* rows,
                                   const double* sums,
                                   const uint32_t* perm, uint32_t n, int w,
                                   long long* out_rows, double* out_sums) {
  __shared__ long long tile[MERGE_TILE * MERGE_W];
  __shared__ uint32_t src_row[MERGE_TILE];
  const uint32_t tid = threadIdx.x;
  const uint32_t row0 = blockIdx.x * MERGE_TILE;
  if (row0 >= n) return;
  const uint32_t m = min((uint32_t)MERGE_TILE, n - row0);
  const uint32_t S = (uint32_t)merge_row_stride(w);
  const uint32_t nw = m * (uint32_t)w;  // words of this tile
  if (tid < m) {
    const uint32_t s = perm[row0 + tid];
    src_row[tid] = s;
    out_sums[row0 + tid] = sums[s];
  }
  __syncthreads();
  for (uint32_t j = tid; j < nw; j += MERGE_TILE) {
    const uint32_t r = j / (uint32_t)w, k = j - r * (uint32_t)w;
    tile[r * S + k] = rows[(size_t)src_row[r] * w + k];
  }
  __syncthreads();
  long long* dst = out_rows + (size_t)row0 * w;
  longlong2* dst2 = reinterpret_cast<longlong2*>(dst);
  for (uint32_t c = tid; c < nw / 2; c += MERGE_TILE) {
    uint32_t r = (2 * c) / (uint32_t)w, k = 2 * c - r * (uint32_t)w;
    longlong2 v;
    v.x = tile[r * S + k];
    if (++k == (uint32_t)w) { k = 0; r++; }
    v.y = tile[r * S + k];
    dst2[c] = v;
  }
  if ((nw & 1u) && tid == 0)
    dst[nw - 1] = tile[(m - 1) * S + (uint32_t)w - 1];
}

}  // namespace dn
