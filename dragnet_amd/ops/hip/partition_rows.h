// Row partition layer, DEVICE ONLY: a stable multi-split of the rows of
// one rank by the rank that will merge them.  This is the step between
// unify_strings.h and the all_to_all of the high-cardinality merge
// (dragnet_amd/merge.py, partition_rows): every rank remaps its
// string-tagged codes to global ones, hashes each row, and sends row i to
// rank hash % world, so the send buffer must hold the rows grouped by
// destination, each group in input order.
//
//   partition_hist_kernel     rows -> per-tile bin counts, bin-major
//   sort_scan_kernel          } exclusive scan of the counts (sort_rows.h)
//   sort_scan_sums_kernel     }
//   partition_scatter_kernel  rows, vals -> wire rows in bin order; counts
//
// A row is w = nk + 1 words of 64 bits (key codes, then the tag pack); a
// wire row is W = nk + 2 words: the remapped codes, the tag pack and the
// bits of the row's f64 value.  world <= 256 bins, one per thread of a
// block where a thread stands for a bin.
//
//  * Per row, in both passes (nothing is kept between them but the
//    counts): a code whose tag (tagpack >> 2j) & 3 is MERGE_EL_STR becomes
//    remap[code]; a code outside [0, m) is never used as an index, it
//    stays as it is and PART_BAD_CODE is set in the status word (the
//    binding raises, so where such a row lands does not matter, only that
//    both passes agree, which they do).  Then h = 0; h = (h ^ code_j) *
//    0x100000001B3 over the columns, h ^= tagpack, all in unsigned 64-bit
//    arithmetic, and bin = h % world.  The modulo is taken in 32-bit
//    pieces: (hi % world * (2^32 % world) + lo % world) % world, whose
//    terms stay below 2^16 + 2^8.
//  * Tile.  sort_rows.h's: SORT_TILE = 2048 rows per 256-thread block in
//    rounds of 256 consecutive rows, so tile order is row order.  Both
//    kernels stride over the tiles, so a capped grid (tests) gives the
//    same result.
//  * Reading.  A round is 256 * w * 8 contiguous bytes, 16-byte aligned
//    (the binding checks the base).  It is staged as merge_insert_kernel
//    stages its tile: lane-consecutive 16-byte loads into LDS rows of odd
//    stride merge_row_stride(w), an odd last word on its own; thread t
//    then reads row t out of LDS without bank conflicts.
//  * Rank (partition_peers, partition_tile_positions: siblings of
//    sort_tile_positions for at most 256 bins).  The lanes of a wave find
//    the lanes with their bin by one ballot per bit of world - 1 (three
//    for world = 8, none for world = 1), not eight.  The histogram kernel
//    lets the lowest lane of each group add the group's size to its
//    wave's private LDS histogram: a plain add, since one wave's LDS
//    operations are ordered and no other wave touches that histogram.  No
//    LDS atomic anywhere, so a table whose rows all go to one rank costs
//    what a uniform one does.  The scatter kernel writes the group sizes
//    to cnt[round][wave][bin] (u16), thread b turns column b into running
//    sums over (round, wave), the bin totals are scanned across the block
//    (sort_block_scan), and a row's place in the tile grouped by bin is
//    binstart[bin] + cnt[round][wave][bin] + rank.
//  * Scan.  hist[bin * ntiles + tile] is padded with zeros to a multiple
//    of 8 counts (the scan kernels' contract; block 0 of the histogram
//    kernel writes the pad) and scanned in place by sort_rows.h's two
//    kernels; the scatter adds the two levels when it reads a base.  The
//    flat index stays below 256 * 2^20 = 2^28.
//  * Scatter.  A whole tile of wire rows is 2048 * 10 * 8 bytes, all 160
//    KB of a CU's LDS, so the tile is grouped by INDEX: place p of the
//    grouped tile gets the tile-local source row (u16) and the bin (u8),
//    6 KB.  The rows themselves then go through LDS a sub-tile of 256
//    places at a time: the sub-tile's source rows are gathered
//    word-consecutive (a row's w words by neighbouring lanes, as
//    sort_gather_kernel reads; the tile was read a moment ago and is in
//    L2), thread t remaps row t in LDS and puts the value's bits behind
//    it, and the sub-tile leaves for wire row base[bin][tile] + (p -
//    binstart[bin]) with neighbouring lanes writing neighbouring 16-byte
//    units of a wire row and neighbouring places neighbouring rows: runs
//    of whole rows, not 64 scattered addresses.  With W even every wire
//    row starts on a 16-byte boundary and is W / 2 units.  With W odd an
//    odd destination row starts 8 bytes past one: its first word is stored
//    on its own and words 1..W-1 are the units; an even row has its last
//    word on its own.  A destination is checked against n, and a source
//    index against the tile's rows, before either is used.
//  * Counts.  counts[b] is the difference of the scanned starts of bins b
//    and b + 1 (n behind the last); block 0 of the scatter writes them, no
//    further kernel.
//  * LDS.  Scatter: 22.0 KB stage (256 rows at stride W | 1 <= 11 words,
//    also the read stage of a round), 16 KB cnt, 4 + 2 KB grouped indices
//    and bins, 3.5 KB binstart, offsets and the sub-tile's sources and
//    destinations: 47.5 KB, three blocks per CU.  Histogram: 18 KB stage
//    + 4 KB wave histograms.
//
// n < 2^31; a tile index is below 2^20.
#pragma once
#include "sort_rows.h"

namespace dn {

constexpr unsigned long long PART_PRIME = 0x100000001B3ull;
constexpr int PART_MAX_WORLD = SORT_BINS;     // a thread per bin
constexpr int PART_WIRE_W = MAX_KEY + 2;      // most words of a wire row
constexpr uint32_t PART_BAD_CODE = 1;         // status: code outside remap

struct PartArgs {
  const long long* rows;   // [n * (nk + 1)], 16-byte aligned
  const long long* remap;  // [m]; read only when remapped
  long long m;
  uint32_t n;
  int nk;
  uint32_t world;          // 1..PART_MAX_WORLD
  uint32_t nbits;          // bits of world - 1
  uint32_t c32;            // 2^32 % world
  bool remapped;
};

// LDS row stride of a wire row in words: odd, as merge_row_stride
DEV uint32_t partition_wire_stride(uint32_t W) { return W | 1u; }

struct PartLds {
  long long stage[SORT_BLOCK * (PART_WIRE_W | 1)];
  uint16_t cnt[SORT_GROUPS * SORT_BINS];
  uint16_t idx[SORT_TILE];   // place -> tile-local source row
  uint8_t bin[SORT_TILE];    // place -> bin
  uint32_t binstart[SORT_BINS];
  uint32_t gofs[SORT_BINS];
  uint32_t dst[SORT_BLOCK];  // of the sub-tile's rows
  uint16_t src[SORT_BLOCK];
  uint32_t wsum[SORT_WAVES];
};

// Rows [0, mm) of src, mm <= 256 rows of w words, 16-byte aligned, into
// LDS rows of stride S.  Barriers before (the stage's last readers) and
// after.
DEV void partition_stage_round(long long* stage, const long long* src,
                               uint32_t mm, uint32_t w, uint32_t S) {
  const uint32_t tid = threadIdx.x;
  const uint32_t nw = mm * w;
  __syncthreads();
  const longlong2* src2 = reinterpret_cast<const longlong2*>(src);
  for (uint32_t c = tid; c < nw / 2; c += SORT_BLOCK) {
    const longlong2 v = src2[c];
    uint32_t r = (2 * c) / w, k = 2 * c - r * w;
    stage[r * S + k] = v.x;
    if (++k == w) { k = 0; r++; }
    stage[r * S + k] = v.y;
  }
  if ((nw & 1u) && tid == 0) stage[(mm - 1) * S + w - 1] = src[nw - 1];
  __syncthreads();
}

// remap[code] of a string-tagged code; the code itself, and bad, when it
// lies outside the table.
DEV long long partition_remap(const PartArgs& A, long long code, bool& bad) {
  if (code >= 0 && code < A.m) return A.remap[code];
  bad = true;
  return code;
}

// The bin of the row at `row` (LDS, nk codes and the tag pack).
DEV uint32_t partition_row_bin(const PartArgs& A, const long long* row,
                               bool& bad) {
  const long long tags = row[A.nk];
  unsigned long long h = 0;
#pragma unroll
  for (int j = 0; j < MAX_KEY; j++) {
    if (j < A.nk) {
      long long code = row[j];
      if (A.remapped && ((tags >> (2 * j)) & 3) == MERGE_EL_STR)
        code = partition_remap(A, code, bad);
      h = (h ^ (unsigned long long)code) * PART_PRIME;
    }
  }
  h ^= (unsigned long long)tags;
  const uint32_t hi = (uint32_t)(h >> 32), lo = (uint32_t)h;
  return ((hi % A.world) * A.c32 + lo % A.world) % A.world;
}

// The valid lanes of the wave whose bin equals this lane's.
DEV uint64_t partition_peers(bool valid, uint32_t bin, uint32_t nbits) {
  uint64_t peers = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < 8; b++) {
    if (b < nbits) {  // uniform
      const bool bit = (bin >> b) & 1u;
      const uint64_t with = __ballot(valid && bit);
      peers &= bit ? with : ~with;
    }
  }
  return peers;
}

// pos[r] = the stable place of the thread's row r (tile row r * 256 +
// tid, one of m) among the tile's rows ordered by bin[r] < 256.  Leaves
// L.binstart: the first place of each bin.
DEV void partition_tile_positions(PartLds& L,
                                  const uint32_t (&bin)[SORT_ROUNDS],
                                  uint32_t m, uint32_t nbits,
                                  uint32_t (&pos)[SORT_ROUNDS]) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t groups =
      (m + SORT_BLOCK - 1) / SORT_BLOCK * (uint32_t)SORT_WAVES;
  __syncthreads();  // the last tile's readers of cnt and binstart
  uint32_t* zero = reinterpret_cast<uint32_t*>(L.cnt);
  for (uint32_t i = tid; i < groups * (SORT_BINS / 2); i += SORT_BLOCK)
    zero[i] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; r++) {
    pos[r] = 0;
    if ((uint32_t)r * SORT_BLOCK >= m) continue;  // block-uniform
    const bool valid = (uint32_t)r * SORT_BLOCK + tid < m;
    const uint64_t peers = partition_peers(valid, bin[r], nbits);
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
    if (valid && rank == 0)
      L.cnt[(r * SORT_WAVES + wave) * SORT_BINS + bin[r]] =
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
  for (int r = 0; r < SORT_ROUNDS; r++)
    if ((uint32_t)r * SORT_BLOCK + tid < m)
      pos[r] += L.binstart[bin[r]] +
                L.cnt[(r * SORT_WAVES + wave) * SORT_BINS + bin[r]];
}

// hist[bin * ntiles + tile] = rows of the tile that go to that bin, and
// `pad` zeros behind the world * ntiles counts.
__launch_bounds__(SORT_BLOCK)
__global__ void partition_hist_kernel(PartArgs A, uint32_t* hist,
                                      uint32_t ntiles, uint32_t pad,
                                      uint32_t* status) {
  __shared__ long long stage[SORT_BLOCK * MERGE_W];
  __shared__ uint32_t wh[SORT_WAVES][SORT_BINS];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t w = (uint32_t)A.nk + 1;
  const uint32_t S = (uint32_t)merge_row_stride((int)w);
  if (blockIdx.x == 0 && tid < pad) hist[(size_t)A.world * ntiles + tid] = 0;
  bool bad = false;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t row0 = tile * SORT_TILE;
    const uint32_t m = min((uint32_t)SORT_TILE, A.n - row0);
    __syncthreads();  // the last tile's readers of wh
#pragma unroll
    for (int k = 0; k < SORT_WAVES; k++) wh[k][tid] = 0;
    for (uint32_t at = 0; at < m; at += SORT_BLOCK) {
      const uint32_t mm = min((uint32_t)SORT_BLOCK, m - at);
      partition_stage_round(stage, A.rows + (size_t)(row0 + at) * w, mm, w,
                            S);
      const bool valid = tid < mm;
      const uint32_t bin =
          valid ? partition_row_bin(A, stage + tid * S, bad) : 0;
      const uint64_t peers = partition_peers(valid, bin, A.nbits);
      if (valid && (peers & ((1ull << lane) - 1)) == 0)
        wh[wave][bin] += (uint32_t)__popcll(peers);
    }
    __syncthreads();
    if (tid < A.world) {
      uint32_t total = 0;
#pragma unroll
      for (int k = 0; k < SORT_WAVES; k++) total += wh[k][tid];
      hist[(size_t)tid * ntiles + tile] = total;
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(status, PART_BAD_CODE);
}

// The first wire row of (bin, tile) out of the two levels of the scanned
// histogram.
DEV uint32_t partition_base(const uint32_t* hist, const uint32_t* sums,
                            uint32_t e) {
  return hist[e] + sums[e / SORT_SCAN_TILE];
}

// Tile by tile: the rows, remapped, with their values' bits, to their
// places in wire [n * (nk + 2)], 16-byte aligned; counts [world] from
// block 0.  hist and sums are the two levels of the scanned histogram.
__launch_bounds__(SORT_BLOCK)
__global__ void partition_scatter_kernel(PartArgs A, const long long* vals,
                                         const uint32_t* hist,
                                         const uint32_t* sums,
                                         uint32_t ntiles, long long* wire,
                                         long long* counts) {
  __shared__ PartLds L;
  const uint32_t tid = threadIdx.x;
  const uint32_t w = (uint32_t)A.nk + 1, W = w + 1;
  const uint32_t S = (uint32_t)merge_row_stride((int)w);
  const uint32_t SW = partition_wire_stride(W);
  const uint32_t npairs = W / 2, units = (W + 1) / 2;
  if (blockIdx.x == 0 && tid < A.world) {
    const uint32_t e = tid * ntiles;
    const uint32_t end =
        tid + 1 < A.world ? partition_base(hist, sums, e + ntiles) : A.n;
    counts[tid] = (long long)(end - partition_base(hist, sums, e));
  }
  bool bad = false;  // reported by the histogram kernel
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t row0 = tile * SORT_TILE;
    const uint32_t m = min((uint32_t)SORT_TILE, A.n - row0);
    uint32_t bin[SORT_ROUNDS], pos[SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; r++) {
      bin[r] = 0;
      const uint32_t at = (uint32_t)r * SORT_BLOCK;
      if (at >= m) continue;  // block-uniform
      const uint32_t mm = min((uint32_t)SORT_BLOCK, m - at);
      partition_stage_round(L.stage, A.rows + (size_t)(row0 + at) * w, mm,
                            w, S);
      if (tid < mm) bin[r] = partition_row_bin(A, L.stage + tid * S, bad);
    }
    partition_tile_positions(L, bin, m, A.nbits, pos);
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; r++) {
      const uint32_t i = (uint32_t)r * SORT_BLOCK + tid;
      if (i < m) {
        L.idx[pos[r]] = (uint16_t)i;
        L.bin[pos[r]] = (uint8_t)bin[r];
      }
    }
    // place p of the grouped tile goes to gofs[bin] + p (mod 2^32)
    if (tid < A.world)
      L.gofs[tid] = partition_base(hist, sums, tid * ntiles + tile) -
                    L.binstart[tid];
    for (uint32_t at = 0; at < m; at += SORT_BLOCK) {
      const uint32_t mm = min((uint32_t)SORT_BLOCK, m - at);
      __syncthreads();  // idx, bin, gofs; the last sub-tile's readers
      if (tid < mm) {
        uint32_t s = L.idx[at + tid];
        uint32_t d = L.gofs[L.bin[at + tid]] + at + tid;
        if (s >= m) { s = 0; d = A.n; }  // never: nothing is read outside
        L.src[tid] = (uint16_t)s;
        L.dst[tid] = d;
        L.stage[tid * SW + w] = vals[row0 + s];
      }
      __syncthreads();
      for (uint32_t j = tid; j < mm * w; j += SORT_BLOCK) {
        const uint32_t r = j / w, k = j - r * w;
        L.stage[r * SW + k] = A.rows[(size_t)(row0 + L.src[r]) * w + k];
      }
      __syncthreads();
      if (A.remapped && tid < mm) {
        long long* row = L.stage + tid * SW;
        const long long tags = row[A.nk];
#pragma unroll
        for (int j = 0; j < MAX_KEY; j++)
          if (j < A.nk && ((tags >> (2 * j)) & 3) == MERGE_EL_STR)
            row[j] = partition_remap(A, row[j], bad);
      }
      __syncthreads();
      for (uint32_t c = tid; c < mm * units; c += SORT_BLOCK) {
        const uint32_t r = c / units, u = c - r * units;
        const uint32_t d = L.dst[r];
        if (d >= A.n) continue;
        const long long* in = L.stage + r * SW;
        long long* out = wire + (size_t)d * W;
        // an odd row of an odd width starts 8 bytes past a 16-byte unit
        const uint32_t off = W & d & 1u;
        if (u < npairs) {
          const uint32_t k = off + 2 * u;
          longlong2 v;
          v.x = in[k];
          v.y = in[k + 1];
          *reinterpret_cast<longlong2*>(out + k) = v;
        } else {
          const uint32_t k = off ? 0 : W - 1;
          out[k] = in[k];
        }
      }
    }
  }
}

}  // namespace dn
