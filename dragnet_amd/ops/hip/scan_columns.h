// Column-query layer, DEVICE ONLY: answer an index query over typed
// columns instead of NDJSON records.  Rows are weighted points (weight =
// the stored SUM(value)); the predicate, bucketize and aggregation tail
// are the record kernels' own (scan_record.h, scan_tables.h).  One row
// body serves two kernels:
//
//   columnar_query_kernel (K7): the columns of ONE index file's metric
//     table, extracted out of SQLite (reference lib/index-query.js:
//     303-338 runs SELECT ... WHERE pred GROUP BY).  Strings are spans
//     of one blob.  ScanState::columnar_query binds it.
//   coded_query_kernel: the merged columnar sidecars of a whole index
//     tree in one launch (index/columnar.py builds the input;
//     ScanState::coded_query binds it).  String columns arrive as u32
//     codes into ONE launch-wide dictionary (doff / dlen spans into a
//     blob of the distinct values).  The dictionary is interned once,
//     one thread per distinct string (dict_intern_kernel -> code2id), so
//     a row's string breakdown is a table lookup: no per-row hash, probe
//     or payload copy.  The row's file ordinal (binary search of
//     seg_start) rides in the plan's reserved trailing key column, so
//     the host can hand every file its own partial rows, as the
//     per-file SQLite GROUP BY does.
#pragma once
#include "scan_tables.h"

namespace dn {

// ColDesc kinds
constexpr int32_t COL_MISSING = 0;  // missing for every row
constexpr int32_t COL_NUM = 1;      // num[r]
constexpr int32_t COL_STR = 2;      // the span soff[r], slen[r] of blob
// a dictionary-coded string (coded_query_kernel only): soff[r] is the
// row's code, slen is unused
constexpr int32_t COL_CODED = 3;

struct ColDesc {
  int32_t kind;
  int32_t pad_;
  const double* num;     // [nrows] (COL_NUM)
  const uint32_t* soff;  // [nrows] (COL_STR, COL_CODED)
  const uint32_t* slen;  // [nrows] (COL_STR)
};

// What both kernels take (ScanState::bind_columns fills it).
struct ColArgs {
  uint32_t nrows;
  const double* values;  // [nrows] row weights
  const uint8_t* blob;   // string payloads / the dictionary's values
  const ColDesc* cols;   // [P.nf] per plan slot
  PlanView P;
  AggTable* tables;
  StrDict sdict;
  NumDict ndict;
  unsigned long long* counters;
};

// The launch dictionary and file segments of a coded query.
struct CodedArgs {
  uint32_t ndict;             // entries of doff / dlen / code2id
  uint32_t nfiles;            // seg_start has nfiles + 1 entries
  const uint32_t* doff;       // [ndict] span of each value in blob
  const uint32_t* dlen;
  const uint32_t* code2id;    // [ndict] StrDict id (dict_intern_kernel)
  const uint32_t* seg_start;  // [nfiles + 1] first row of each file
};

// One thread per distinct string of the launch dictionary: intern it
// and record its id.  A full dictionary leaves 0xFFFFFFFF in code2id
// and bumps overflow[0] (the C_OVERFLOW counter).
__global__ void dict_intern_kernel(StrDict D, const uint8_t* blob,
                                   const uint32_t* doff,
                                   const uint32_t* dlen, uint32_t ndict,
                                   uint32_t* code2id,
                                   unsigned long long* overflow) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ndict) return;
  Bytes BV;
  BV.mem = blob;
  BV.bias = 0;
  uint32_t id = intern_string(D, BV, doff[i], dlen[i]);
  if (id == 0xFFFFFFFFu) atomicAdd(overflow, 1ull);
  code2id[i] = id;
}

// Ordinal of the file that row r belongs to: the last f with
// seg_start[f] <= r.  Empty files repeat a value and are never chosen
// (their successor starts at the same row).  seg_start is a few KB at
// most, shared by every row: it stays in L2.
DEV uint32_t file_ordinal(const uint32_t* seg_start, uint32_t nfiles,
                          uint32_t r) {
  uint32_t lo = 0, hi = nfiles;  // seg_start[lo] <= r < seg_start[hi]
  while (hi - lo > 1) {
    uint32_t mid = lo + ((hi - lo) >> 1);
    if (seg_start[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// Grid-stride over rows.  CODED: string columns are COL_CODED, not
// COL_STR; the last breakdown of every metric is the reserved file
// column; an unbucketed string key is code2id's.  X is read only then.
template <bool CODED>
DEV void column_rows(char* smem, const ColArgs& A, const CodedArgs& X) {
  const PlanView& P = A.P;
  const int nf = P.nf;
  const LdsLayout L(nf, P.nm, 0, false);
  LdsCacheEntry* cache = reinterpret_cast<LdsCacheEntry*>(smem + L.cache);
  unsigned long long* lcnt =
      reinterpret_cast<unsigned long long*>(smem + L.lcnt);
  const int NCNT = C_GLOBAL_N + P.nm * CM_N;
  block_agg_init(cache, lcnt, NCNT);

  FV fv;
  fv.type = reinterpret_cast<uint8_t*>(smem + L.fv_type);
  fv.soff = reinterpret_cast<uint32_t*>(smem + L.fv_soff);
  fv.slen = reinterpret_cast<uint32_t*>(smem + L.fv_slen);
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
      if (c.kind == COL_NUM) {
        fv.set(f, T_NUM, 0, 0, c.num[r]);
      } else if (!CODED && c.kind == COL_STR) {
        fv.set(f, T_STR, c.soff[r], c.slen[r], 0.0);
      } else if (CODED && c.kind == COL_CODED) {
        // the host validated every code; a code past the dictionary
        // reads nothing and counts as a missing field
        uint32_t code = c.soff[r];
        if (code < X.ndict)
          fv.set(f, T_STR, X.doff[code], X.dlen[code], 0.0);
        else
          fv.set(f, T_MISSING, 0, 0, 0.0);
      } else {
        fv.set(f, T_MISSING, 0, 0, 0.0);
      }
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
    uint32_t file_code = 0;
    if constexpr (CODED)
      file_code = make_code(
          TAG_ORD, file_ordinal(X.seg_start, X.nfiles, r) + ORD_BIAS);
    for (int m = 0; m < P.nm; m++) {
      const int32_t* M = &P.metric_rows[m * 8];
      unsigned long long* mc = &lcnt[C_GLOBAL_N + m * CM_N];
      atomicAdd(&mc[CM_AGG_IN], 1ull);

      uint32_t key[MAX_KEY];
      int nk = M[1];  // CODED: the query's breakdowns + the file column
      if (CODED && nk < 1) continue;
      bool drop = false, overflow = false;
      for (int bi = 0; bi < nk; bi++) {
        const int32_t* B = &P.bd_rows[(M[2] + bi) * 4];
        int slot = B[1];  // column plans use kind-0 refs only
        uint32_t code;
        if (CODED && bi == nk - 1) {
          code = file_code;
        } else if (CODED && B[2] == BUCKET_NONE &&
                   fv.get_type(slot) == T_STR) {
          // T_STR comes from a coded column alone, its code in range
          uint32_t id = X.code2id[A.cols[slot].soff[r]];
          if (id == 0xFFFFFFFFu) { overflow = true; break; }
          code = make_code(TAG_STR, id);
        } else if (!encode_key_col(A.sdict, A.ndict, BV,
                                   fv.get_type(slot), fv.get_num(slot),
                                   fv.get_soff(slot), fv.get_slen(slot),
                                   B[2], P.bd_steps[M[2] + bi], code, drop,
                                   overflow)) {
          break;
        }
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

      lds_cache_add<8>(cache, A.tables, A.counters, lcnt, m, key, nk,
                       agg_key_hash(m, key), weight);
    }
  }

  block_agg_flush(cache, lcnt, NCNT, P, A.tables, A.counters);
}

// 5 waves/SIMD is what these kernels compile to (91 / 89 VGPRs);
// holding the register allocator to it keeps the K7 kernel's SGPR spill
// count at the level it had before it shared the aggregation tail (157
// vs 163; at a bound of 4 the allocator lands on 165).
__launch_bounds__(BLOCK, 5)
__global__ void columnar_query_kernel(ColArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smemc[];
  column_rows<false>(smemc, A, CodedArgs{});
}

__launch_bounds__(BLOCK, 5)
__global__ void coded_query_kernel(ColArgs A, CodedArgs X) {
  extern __shared__ __attribute__((aligned(16))) char smemd[];
  column_rows<true>(smemd, A, X);
}

}  // namespace dn
