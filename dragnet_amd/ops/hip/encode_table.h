// Wire-form export layer, DEVICE ONLY: one metric's table, as a scan's
// extraction leaves it (u32 key codes, f64 counts, the scan's string and
// number dictionaries), to the wire form of dragnet_amd/merge.py: int64
// codes [n, nk], a tag pack and the values per row, and a string
// dictionary as a byte blob with offsets.  It is the step in front of
// unify_strings.h, merge_rows.h and partition_rows.h; with it a table
// reaches them without becoming Python objects.  Output row i is
// extraction row i; the result is plan.decode_key followed by
// merge._encode_table, element by element.
//
//   encode_mark_kernel      rows -> which string / number ids and which
//                           constants are referenced; validates the codes
//   encode_classify_kernel  used strings -> plain or exception, lengths
//   encode_numbers_kernel   used numbers -> integral or exception, lengths
//   sort_scan_kernel        } one exclusive scan over every flag and
//   sort_scan_sums_kernel   } length array at once (sort_rows.h)
//   encode_totals_kernel    segment bases, counts and byte totals -> meta
//   (the host reads meta: its one sync, and sizes the outputs exactly)
//   encode_strings_kernel   plain strings -> dict_blob, exceptions' raw
//                           bytes -> exc_blob, with their offsets
//   encode_digits_kernel    integral numbers -> decimal digits; constants
//   encode_emit_kernel      rows -> codes, tagpack, vals
//
//  * Dictionary.  Only what a ready row references enters it, each scan
//    id, number id and constant once, in an order the snapshot fixes:
//    used constants by code, plain strings by id, integral numbers by
//    id, then the exceptions by (kind, id).  A plain string is a
//    dictionary string without a backslash that Python's UTF-8 decoder
//    accepts (no overlong form, no surrogate, nothing above U+10FFFF, no
//    truncated sequence): its bytes are its wire bytes.  A number with an
//    integral value below 2^53 in magnitude is its decimal digits, 1 to
//    16 of them by integer division, "-" in front of a negative one, -0
//    as "0".  Everything else (ENC_X_STR: an escaped or ill-formed
//    string, ENC_X_ARR: an array's JSON text, ENC_X_NUM: any other
//    number) is an exception: its raw bytes (a number's 8) go to
//    exc_blob in (kind, id) order, the host renders those E entries with
//    the functions the host path uses and appends them, and their wire
//    codes are S_dev + position.  The dictionary may name one string
//    twice; every consumer unifies first.
//  * One scan.  Ten u32 arrays, indexed by string id or number id, lie
//    end to end in one array (EncSeg), each padded to a multiple of 8:
//    plain flag and bytes; the three exception flags; the three
//    exceptions' byte counts; integral flag and bytes.  One exclusive scan
//    runs over all of it; a value inside segment k is scan - base[k],
//    base[k] being the scan at the segment's first entry.  The three
//    exception flag segments are neighbours, so scan - base[ENC_X_STR
//    flags] is the position by (kind, id) directly; likewise their bytes.
//    Sums wrap mod 2^32 across segments and the differences are exact
//    (the binding bounds every segment's own total).
//  * Variable-length spans: staged through LDS.  Dictionary strings are
//    tens of bytes and lie packed in the payload; a lane per string
//    reading them from global memory is the 64-way divergent gather of
//    DESIGN.md's ladder.  A tile is 256 consecutive ids.  The byte range
//    from the lowest start to the highest end of its used strings, when
//    it is at most ENC_STAGE_BYTES, comes into LDS by lane-consecutive
//    16-byte loads (unify_strings.h's unify_load16) and the lanes
//    classify out of LDS through UnifySpan's 8-byte window: a word with
//    no byte >= 0x80 and no backslash, outside a sequence, is accepted
//    whole; only other words go through the byte-wise UTF-8 automaton.
//    The copy stages twice: lanes move their strings from the input
//    stage to an output stage laid out as dict_blob is (plain strings of
//    ascending ids are neighbours there: the tile's output is one
//    range), and the block stores that range by lane-consecutive 16-byte
//    stores, the ragged first and last unit by bytes.  A tile whose range
//    does not fit (a 4 KB string beside others, ids far apart in the
//    payload) takes the same code over global memory, lane per string.
//    Staging rather than balancing by bytes: the common tile fits, the
//    classify needs a sequential automaton per string anyway, and both
//    paths share one window.  Exceptions are rare and copied by their
//    lane from global memory.
//  * Bounds.  n, n_str, n_num and used are read on the device (the
//    extraction hands them out there) and clamped to the tensors' sizes.
//    The mark kernel checks every tag against its column's kind and
//    every id against n_str / n_num; the classify kernel checks every
//    used span against used.  A failure sets a status bit; every later
//    kernel returns at once when the word is set, and the binding raises.
//    The payload is 16-byte aligned and read as unify_strings.h reads a
//    blob of `used` bytes: nothing outside [blob, blob + used).
//  * Refusal.  A bucketized or date column holding a NaN or infinite
//    number is where the host's int() raises; ENC_REFUSED tells the
//    caller to take the host path.
//  * Emit.  One thread per row reads its 32-byte key row in two 16-byte
//    loads; tagpack and vals leave lane-consecutive; the nk code words
//    go through an LDS tile at an odd stride and leave as
//    lane-consecutive 16-byte stores (sort_gather_kernel's way out).
//  * No atomics beyond the constants-mask and status ORs; the flag
//    stores are plain byte stores of 1.  All stores are vector stores.
//
// n < 2^31 rows; ids, offsets and byte totals are u32.
#pragma once
#include "unify_strings.h"

namespace dn {

constexpr int ENC_BLOCK = 256;               // rows / ids per tile = threads
constexpr int ENC_STAGE_BYTES = 16 * 1024;   // each of the two LDS stages

// column kinds (merge.py col_kinds)
constexpr int ENC_COL_PLAIN = 0, ENC_COL_DATE = 1, ENC_COL_BUCKET = 2;

// wire tags (merge.py _EL_*)
constexpr long long ENC_EL_INT = 0, ENC_EL_STR = 1, ENC_EL_F64 = 2;

// exception kinds, the order of the exceptions in the dictionary
constexpr int ENC_X_STR = 0, ENC_X_ARR = 1, ENC_X_NUM = 2;

// status word bits
constexpr uint32_t ENC_BAD_TAG = 1;   // a code its column cannot hold
constexpr uint32_t ENC_BAD_ID = 2;    // a string / number id out of range
constexpr uint32_t ENC_BAD_SPAN = 4;  // a used string beyond `used`
constexpr uint32_t ENC_REFUSED = 8;   // NaN / inf in an integer column

// per-id classes (str_cls, num_cls)
constexpr uint8_t ENC_S_PLAIN = 1, ENC_S_EXC = 2, ENC_S_ARR = 4;
constexpr uint8_t ENC_N_INT = 1, ENC_N_EXC = 2;

// segments of the scanned array, by string id (S) or number id (N)
enum EncSeg : int {
  ENC_PLAIN_F = 0,  // S: plain string flag
  ENC_PLAIN_B,      // S: its bytes
  ENC_XSTR_F,       // S: exception string flag  } positions by
  ENC_XARR_F,       // S: array text flag        } (kind, id)
  ENC_XNUM_F,       // N: exception number flag  }
  ENC_XSTR_B,       // S: raw bytes              } exc_blob offsets
  ENC_XARR_B,       // S: raw bytes              }
  ENC_XNUM_B,       // N: 8                      }
  ENC_INT_F,        // N: integral number flag
  ENC_INT_B,        // N: digits and sign
  ENC_SEGS
};

// meta words, read by the host in one copy
enum EncMeta : int {
  ENC_M_STATUS = 0, ENC_M_MASK, ENC_M_N, ENC_M_SDEV, ENC_M_E, ENC_M_DBYTES,
  ENC_M_EBYTES, ENC_M_NCONST, ENC_M_CBYTES, ENC_M_P, ENC_M_PBYTES,
  ENC_M_BASE = 12,                      // ENC_SEGS bases
  ENC_M_CONST = ENC_M_BASE + ENC_SEGS,  // wire code of each constant
  ENC_M_WORDS = ENC_M_CONST + 6
};

struct EncArgs {
  const uint32_t* keys;       // [cap, MAX_KEY], 16-byte aligned
  const double* counts;       // [cap]
  const uint32_t* n_ptr;
  uint32_t cap;
  const uint32_t* str_off;    // [str_cap]
  const uint32_t* str_len;
  const uint32_t* n_str_ptr;
  uint32_t str_cap;
  const uint8_t* blob;        // 16-byte aligned
  const uint32_t* used_ptr;
  uint32_t blob_cap;
  const double* numbers;      // [num_cap]
  const uint32_t* n_num_ptr;
  uint32_t num_cap;
  int nk;
  uint8_t col_kind[MAX_KEY];
  uint8_t* str_used;          // [str_cap] referenced as a string
  uint8_t* arr_used;          // [str_cap] referenced as an array's text
  uint8_t* num_used;          // [num_cap] referenced from a plain column
  uint8_t* str_cls;           // [str_cap]
  uint8_t* num_cls;           // [num_cap]
  uint32_t* scan;             // [seg[ENC_SEGS] + 8]
  uint32_t* sums;
  uint32_t seg[ENC_SEGS + 1]; // first entry of each segment; the end
  uint32_t* meta;             // [ENC_M_WORDS]
  // outputs, allocated once the host has read meta
  long long* codes;           // [n, nk], 16-byte aligned
  long long* tagpack;
  double* vals;
  uint8_t* dict_blob;         // 16-byte aligned
  long long* dict_offs;       // [S_dev + 1]
  int* exc_kind;              // [E]
  int* exc_id;
  uint8_t* exc_blob;
  long long* exc_offs;        // [E + 1]
};

DEV uint32_t enc_n(const EncArgs& A) { return min(*A.n_ptr, A.cap); }
DEV uint32_t enc_n_str(const EncArgs& A) {
  return min(*A.n_str_ptr, A.str_cap);
}
DEV uint32_t enc_n_num(const EncArgs& A) {
  return min(*A.n_num_ptr, A.num_cap);
}
DEV uint32_t enc_used(const EncArgs& A) {
  return min(*A.used_ptr, A.blob_cap);
}

// The scanned value of entry i of segment k, less nothing.
DEV uint32_t enc_at(const EncArgs& A, int k, uint32_t i) {
  const uint32_t e = A.seg[k] + i;
  return A.scan[e] + A.sums[e / SORT_SCAN_TILE];
}

DEV void enc_key_row(const EncArgs& A, uint32_t i,
                     uint32_t (&code)[MAX_KEY]) {
  const uint4* row =
      reinterpret_cast<const uint4*>(A.keys + (size_t)i * MAX_KEY);
  const uint4 lo = row[0], hi = row[1];
  code[0] = lo.x; code[1] = lo.y; code[2] = lo.z; code[3] = lo.w;
  code[4] = hi.x; code[5] = hi.y; code[6] = hi.z; code[7] = hi.w;
}

__launch_bounds__(ENC_BLOCK)
__global__ void encode_mark_kernel(EncArgs A) {
  const uint32_t n = enc_n(A), n_str = enc_n_str(A), n_num = enc_n_num(A);
  uint32_t bad = 0, mask = 0;
  const uint32_t stride = gridDim.x * ENC_BLOCK;
  for (uint32_t i = blockIdx.x * ENC_BLOCK + threadIdx.x; i < n;
       i += stride) {
    uint32_t code[MAX_KEY];
    enc_key_row(A, i, code);
#pragma unroll
    for (int j = 0; j < MAX_KEY; j++) {
      if (j >= A.nk) break;
      const uint32_t tag = code[j] >> 30, val = code[j] & 0x3FFFFFFFu;
      const int kind = A.col_kind[j];
      if (tag == TAG_ORD) {
        if (kind != ENC_COL_BUCKET) bad |= ENC_BAD_TAG;
      } else if (tag == TAG_NUM) {
        if (val >= n_num) {
          bad |= ENC_BAD_ID;
        } else if (kind == ENC_COL_PLAIN) {
          A.num_used[val] = 1;
        } else if (!(fabs(A.numbers[val]) < __builtin_inf())) {
          bad |= ENC_REFUSED;
        }
      } else if (kind == ENC_COL_BUCKET) {
        bad |= ENC_BAD_TAG;
      } else if (tag == TAG_STR) {
        if (val >= n_str) bad |= ENC_BAD_ID; else A.str_used[val] = 1;
      } else if ((val & 7u) == SPECIAL_ARRJSON) {
        if ((val >> 3) >= n_str) bad |= ENC_BAD_ID;
        else A.arr_used[val >> 3] = 1;
      } else if (val <= SPECIAL_ARRAY) {
        mask |= 1u << val;
      } else {
        bad |= ENC_BAD_TAG;
      }
    }
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    bad |= __shfl_xor(bad, off, 64);
    mask |= __shfl_xor(mask, off, 64);
  }
  if (__lane_id() == 0) {
    if (bad) atomicOr(&A.meta[ENC_M_STATUS], bad);
    if (mask) atomicOr(&A.meta[ENC_M_MASK], mask);
  }
}

// Lowest lo and highest hi over the block; red is LDS, 2 * waves words.
DEV void enc_block_range(uint32_t& lo, uint32_t& hi, uint32_t* red) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor(lo, off, 64));
    hi = max(hi, (uint32_t)__shfl_xor(hi, off, 64));
  }
  constexpr int waves = ENC_BLOCK / 64;
  __syncthreads();  // the last tile's readers of red and of the stages
  if (__lane_id() == 0) {
    red[threadIdx.x >> 6] = lo;
    red[waves + (threadIdx.x >> 6)] = hi;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < waves; k++) {
    lo = min(lo, red[k]);
    hi = max(hi, red[waves + k]);
  }
}

// Bring [base, end) of the payload (base a multiple of 16, end <= used)
// into the stage, 16 bytes per lane and step.
DEV void enc_stage_in(uint4* stage, const uint8_t* blob, uint32_t used,
                      uint32_t base, uint32_t end) {
  const uint32_t units = (end - base + 15u) >> 4;
  for (uint32_t u = threadIdx.x; u < units; u += ENC_BLOCK)
    stage[u] = unify_load16(blob, (long long)used, (long long)base + 16ll * u);
  __syncthreads();
}

// No backslash, and UTF-8 that Python's decoder accepts.
template <class Words>
DEV bool enc_is_plain(Words W, uint32_t off, uint32_t len) {
  constexpr uint64_t HI = 0x8080808080808080ull, ONES = 0x0101010101010101ull;
  UnifySpan<Words> span(W, (long long)off, (long long)len);
  uint32_t need = 0, lo = 0x80, hi = 0xBF;  // of a sequence under way
  for (uint32_t k = 0; k < len; k += 8) {
    const uint64_t v = span.next();
    if (need == 0 && !(v & HI)) {
      const uint64_t x = v ^ (ONES * 0x5C);  // a zero byte: a backslash
      if ((x - ONES) & ~x & HI) return false;
      continue;
    }
    const uint32_t m = min(8u, len - k);
    for (uint32_t b = 0; b < m; b++) {
      const uint32_t c = (uint32_t)(v >> (8 * b)) & 0xffu;
      if (need) {
        if (c < lo || c > hi) return false;
        need--; lo = 0x80; hi = 0xBF;
      } else if (c < 0x80) {
        if (c == 0x5C) return false;
      } else if (c >= 0xC2 && c <= 0xDF) { need = 1;
      } else if (c == 0xE0) { need = 2; lo = 0xA0;
      } else if (c == 0xED) { need = 2; hi = 0x9F;
      } else if (c >= 0xE1 && c <= 0xEF) { need = 2;
      } else if (c == 0xF0) { need = 3; lo = 0x90;
      } else if (c == 0xF4) { need = 3; hi = 0x8F;
      } else if (c >= 0xF1 && c <= 0xF3) { need = 3;
      } else { return false; }
    }
  }
  return need == 0;
}

__launch_bounds__(ENC_BLOCK)
__global__ void encode_classify_kernel(EncArgs A) {
  __shared__ uint4 stage[ENC_STAGE_BYTES / 16];
  __shared__ uint32_t red[2 * ENC_BLOCK / 64];
  if (A.meta[ENC_M_STATUS]) return;
  const uint32_t n_str = enc_n_str(A), used = enc_used(A);
  const UnifyGlobalWords G = {A.blob, (long long)used};
  bool bad = false;
  const uint32_t ntiles = (n_str + ENC_BLOCK - 1) / ENC_BLOCK;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t s = t * ENC_BLOCK + threadIdx.x;
    bool su = false, au = false;
    uint32_t off = 0, len = 0;
    if (s < n_str && (A.str_used[s] | A.arr_used[s])) {
      off = A.str_off[s];
      len = A.str_len[s];
      if (off > used || len > used - off) {
        bad = true;
      } else {
        su = A.str_used[s];
        au = A.arr_used[s];
      }
    }
    uint32_t lo = su ? off : 0xFFFFFFFFu, hi = su ? off + len : 0u;
    enc_block_range(lo, hi, red);
    const uint32_t base = lo & ~15u;
    bool plain = false;
    if (hi > lo && hi - base <= (uint32_t)ENC_STAGE_BYTES) {  // block-uniform
      enc_stage_in(stage, A.blob, used, base, hi);
      const UnifyLdsWords L = {reinterpret_cast<const uint64_t*>(stage),
                               (long long)(base >> 3)};
      if (su) plain = enc_is_plain(L, off, len);
    } else if (su) {
      plain = enc_is_plain(G, off, len);
    }
    uint8_t cls = 0;
    if (su) {
      cls = plain ? ENC_S_PLAIN : ENC_S_EXC;
      A.scan[A.seg[plain ? ENC_PLAIN_F : ENC_XSTR_F] + s] = 1;
      A.scan[A.seg[plain ? ENC_PLAIN_B : ENC_XSTR_B] + s] = len;
    }
    if (au) {
      cls |= ENC_S_ARR;
      A.scan[A.seg[ENC_XARR_F] + s] = 1;
      A.scan[A.seg[ENC_XARR_B] + s] = len;
    }
    if (cls) A.str_cls[s] = cls;
  }
  if (__ballot(bad) && __lane_id() == 0)
    atomicOr(&A.meta[ENC_M_STATUS], ENC_BAD_SPAN);
}

// Decimal digits of u < 2^53, at least one.
DEV uint32_t enc_digits(uint64_t u) {
  uint32_t d = 1;
  while (u >= 10) { u /= 10; d++; }
  return d;
}

DEV bool enc_integral(double x) {
  return x == trunc(x) && fabs(x) < 9007199254740992.0;  // NaN: neither
}

__launch_bounds__(ENC_BLOCK)
__global__ void encode_numbers_kernel(EncArgs A) {
  if (A.meta[ENC_M_STATUS]) return;
  const uint32_t k = blockIdx.x * ENC_BLOCK + threadIdx.x;
  if (k >= enc_n_num(A) || !A.num_used[k]) return;
  const double x = A.numbers[k];
  if (enc_integral(x)) {
    A.num_cls[k] = ENC_N_INT;
    A.scan[A.seg[ENC_INT_F] + k] = 1;
    A.scan[A.seg[ENC_INT_B] + k] =
        enc_digits((uint64_t)fabs(x)) + (x < 0 ? 1u : 0u);
  } else {
    A.num_cls[k] = ENC_N_EXC;
    A.scan[A.seg[ENC_XNUM_F] + k] = 1;
    A.scan[A.seg[ENC_XNUM_B] + k] = 8;
  }
}

__device__ const char ENC_CONST_TEXT[6][16] = {
    "null", "undefined", "true", "false", "[object Object]", "<array>"};
__device__ const uint32_t ENC_CONST_LEN[6] = {4, 9, 4, 5, 15, 7};

// One block: the bases of the scanned segments and what follows from
// them, for the host and for the kernels behind it.
__launch_bounds__(64)
__global__ void encode_totals_kernel(EncArgs A) {
  __shared__ uint32_t base[ENC_SEGS + 1];
  A.meta[ENC_M_N] = enc_n(A);  // every lane the same word
  if (A.meta[ENC_M_STATUS]) return;
  if (threadIdx.x <= ENC_SEGS) {
    const uint32_t e = A.seg[threadIdx.x];  // the end is scanned too
    base[threadIdx.x] = A.scan[e] + A.sums[e / SORT_SCAN_TILE];
  }
  __syncthreads();
  if (threadIdx.x < ENC_SEGS)
    A.meta[ENC_M_BASE + threadIdx.x] = base[threadIdx.x];
  if (threadIdx.x != 0) return;
  const uint32_t mask = A.meta[ENC_M_MASK];
  uint32_t nconst = 0, cbytes = 0;
  for (uint32_t c = 0; c < 6; c++) {
    A.meta[ENC_M_CONST + c] = nconst;
    if (mask & (1u << c)) { nconst++; cbytes += ENC_CONST_LEN[c]; }
  }
  const uint32_t P = base[ENC_PLAIN_B] - base[ENC_PLAIN_F];
  const uint32_t PB = base[ENC_XSTR_F] - base[ENC_PLAIN_B];
  const uint32_t I = base[ENC_INT_B] - base[ENC_INT_F];
  const uint32_t IB = base[ENC_SEGS] - base[ENC_INT_B];
  A.meta[ENC_M_NCONST] = nconst;
  A.meta[ENC_M_CBYTES] = cbytes;
  A.meta[ENC_M_P] = P;
  A.meta[ENC_M_PBYTES] = PB;
  A.meta[ENC_M_SDEV] = nconst + P + I;
  A.meta[ENC_M_DBYTES] = cbytes + PB + IB;
  A.meta[ENC_M_E] = base[ENC_XSTR_B] - base[ENC_XSTR_F];
  A.meta[ENC_M_EBYTES] = base[ENC_INT_F] - base[ENC_XSTR_B];
}

// Exception (kind, id) of len raw bytes at src: its entry and its bytes.
DEV void enc_put_exception(const EncArgs& A, int kind, uint32_t id,
                           int flag_seg, int byte_seg, const uint8_t* src,
                           uint32_t len) {
  const uint32_t pos =
      enc_at(A, flag_seg, id) - A.meta[ENC_M_BASE + ENC_XSTR_F];
  const uint32_t at =
      enc_at(A, byte_seg, id) - A.meta[ENC_M_BASE + ENC_XSTR_B];
  A.exc_kind[pos] = kind;
  A.exc_id[pos] = (int)id;
  A.exc_offs[pos] = (long long)at;
  for (uint32_t b = 0; b < len; b++) A.exc_blob[at + b] = src[b];
}

__launch_bounds__(ENC_BLOCK)
__global__ void encode_strings_kernel(EncArgs A) {
  __shared__ uint4 stage[ENC_STAGE_BYTES / 16];
  __shared__ uint4 outb[ENC_STAGE_BYTES / 16];
  __shared__ uint32_t red[2 * ENC_BLOCK / 64];
  if (A.meta[ENC_M_STATUS]) return;
  const uint32_t n_str = enc_n_str(A), used = enc_used(A);
  const uint32_t nconst = A.meta[ENC_M_NCONST];
  const uint32_t cbytes = A.meta[ENC_M_CBYTES];
  const uint32_t base_f = A.meta[ENC_M_BASE + ENC_PLAIN_F];
  const uint32_t base_b = A.meta[ENC_M_BASE + ENC_PLAIN_B];
  const uint32_t ntiles = (n_str + ENC_BLOCK - 1) / ENC_BLOCK;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t s = t * ENC_BLOCK + threadIdx.x;
    const uint8_t cls = s < n_str ? A.str_cls[s] : (uint8_t)0;
    const bool plain = cls & ENC_S_PLAIN;
    uint32_t off = 0, len = 0, dst = 0;
    if (cls) {  // validated by the classify kernel
      off = A.str_off[s];
      len = A.str_len[s];
    }
    if (plain) {
      dst = cbytes + (enc_at(A, ENC_PLAIN_B, s) - base_b);
      A.dict_offs[nconst + (enc_at(A, ENC_PLAIN_F, s) - base_f)] =
          (long long)dst;
    }
    uint32_t lo = plain ? off : 0xFFFFFFFFu, hi = plain ? off + len : 0u;
    enc_block_range(lo, hi, red);
    uint32_t dlo = plain ? dst : 0xFFFFFFFFu, dhi = plain ? dst + len : 0u;
    enc_block_range(dlo, dhi, red);
    const uint32_t base = lo & ~15u, dbase = dlo & ~15u;
    if (hi > lo && hi - base <= (uint32_t)ENC_STAGE_BYTES &&
        dhi - dbase <= (uint32_t)ENC_STAGE_BYTES) {  // block-uniform
      enc_stage_in(stage, A.blob, used, base, hi);
      // the plain strings of a tile tile [dlo, dhi): one writer per byte
      const uint8_t* in = reinterpret_cast<const uint8_t*>(stage);
      uint8_t* out = reinterpret_cast<uint8_t*>(outb);
      if (plain)
        for (uint32_t b = 0; b < len; b++)
          out[dst - dbase + b] = in[off - base + b];
      __syncthreads();
      const uint32_t units = (dhi - dbase + 15u) >> 4;
      for (uint32_t u = threadIdx.x; u < units; u += ENC_BLOCK) {
        const uint32_t at = dbase + 16u * u;
        if (at >= dlo && at + 16u <= dhi) {
          *reinterpret_cast<uint4*>(A.dict_blob + at) = outb[u];
        } else {
          for (uint32_t b = 0; b < 16u; b++)
            if (at + b >= dlo && at + b < dhi)
              A.dict_blob[at + b] = out[16u * u + b];
        }
      }
    } else if (plain) {
      for (uint32_t b = 0; b < len; b++)
        A.dict_blob[dst + b] = A.blob[off + b];
    }
    if (cls & ENC_S_EXC)
      enc_put_exception(A, ENC_X_STR, s, ENC_XSTR_F, ENC_XSTR_B,
                        A.blob + off, len);
    if (cls & ENC_S_ARR)
      enc_put_exception(A, ENC_X_ARR, s, ENC_XARR_F, ENC_XARR_B,
                        A.blob + off, len);
  }
}

// Integral numbers as digits, exception numbers as their 8 bytes; block
// 0 also writes the constants and closes both offset arrays.
__launch_bounds__(ENC_BLOCK)
__global__ void encode_digits_kernel(EncArgs A) {
  if (A.meta[ENC_M_STATUS]) return;
  const uint32_t nconst = A.meta[ENC_M_NCONST];
  const uint32_t k = blockIdx.x * ENC_BLOCK + threadIdx.x;
  if (k == 0) {
    const uint32_t mask = A.meta[ENC_M_MASK];
    uint32_t at = 0;
    for (uint32_t c = 0; c < 6; c++)
      if (mask & (1u << c)) {
        A.dict_offs[A.meta[ENC_M_CONST + c]] = (long long)at;
        for (uint32_t b = 0; b < ENC_CONST_LEN[c]; b++)
          A.dict_blob[at++] = (uint8_t)ENC_CONST_TEXT[c][b];
      }
    A.dict_offs[A.meta[ENC_M_SDEV]] = (long long)A.meta[ENC_M_DBYTES];
    A.exc_offs[A.meta[ENC_M_E]] = (long long)A.meta[ENC_M_EBYTES];
  }
  if (k >= enc_n_num(A)) return;
  const uint8_t cls = A.num_cls[k];
  const double x = A.numbers[k];
  if (cls == ENC_N_INT) {
    const uint32_t rank =
        enc_at(A, ENC_INT_F, k) - A.meta[ENC_M_BASE + ENC_INT_F];
    uint32_t at = A.meta[ENC_M_CBYTES] + A.meta[ENC_M_PBYTES] +
                  (enc_at(A, ENC_INT_B, k) - A.meta[ENC_M_BASE + ENC_INT_B]);
    A.dict_offs[nconst + A.meta[ENC_M_P] + rank] = (long long)at;
    uint64_t u = (uint64_t)fabs(x);
    if (x < 0) A.dict_blob[at++] = '-';
    const uint32_t d = enc_digits(u);
    for (uint32_t p = d; p-- > 0;) {
      A.dict_blob[at + p] = (uint8_t)('0' + (uint32_t)(u % 10));
      u /= 10;
    }
  } else if (cls == ENC_N_EXC) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    uint8_t raw[8];
    for (int b = 0; b < 8; b++) raw[b] = (uint8_t)(bits >> (8 * b));
    enc_put_exception(A, ENC_X_NUM, k, ENC_XNUM_F, ENC_XNUM_B, raw, 8);
  }
}

__launch_bounds__(ENC_BLOCK)
__global__ void encode_emit_kernel(EncArgs A) {
  __shared__ long long tile[ENC_BLOCK * (MAX_KEY | 1)];
  if (A.meta[ENC_M_STATUS]) return;
  const uint32_t n = enc_n(A);
  const uint32_t tid = threadIdx.x;
  const uint32_t row0 = blockIdx.x * ENC_BLOCK;
  if (row0 >= n) return;
  const uint32_t m = min((uint32_t)ENC_BLOCK, n - row0);
  const uint32_t nk = (uint32_t)A.nk, S = nk | 1u;
  if (tid < m) {
    const uint32_t i = row0 + tid;
    const uint32_t nconst = A.meta[ENC_M_NCONST];
    const uint32_t sdev = A.meta[ENC_M_SDEV];
    const uint32_t xbase = A.meta[ENC_M_BASE + ENC_XSTR_F];
    uint32_t code[MAX_KEY];
    enc_key_row(A, i, code);
    long long tp = 0;
#pragma unroll
    for (int j = 0; j < MAX_KEY; j++) {
      if (j >= A.nk) break;
      const uint32_t tag = code[j] >> 30, val = code[j] & 0x3FFFFFFFu;
      long long el = ENC_EL_STR, out;
      if (tag == TAG_ORD) {
        el = ENC_EL_INT;
        out = (long long)val - (long long)ORD_BIAS;
      } else if (tag == TAG_NUM && A.col_kind[j] != ENC_COL_PLAIN) {
        const double x = A.numbers[val];  // finite: the mark kernel
        if (x >= -9223372036854775808.0 && x < 9223372036854775808.0) {
          el = ENC_EL_INT;
          out = (long long)x;  // toward zero
        } else {
          el = ENC_EL_F64;
          out = __double_as_longlong(x);
        }
      } else if (tag == TAG_NUM) {
        out = A.num_cls[val] == ENC_N_INT
            ? nconst + A.meta[ENC_M_P] +
                  (enc_at(A, ENC_INT_F, val) - A.meta[ENC_M_BASE + ENC_INT_F])
            : sdev + (enc_at(A, ENC_XNUM_F, val) - xbase);
      } else if (tag == TAG_STR) {
        out = (A.str_cls[val] & ENC_S_PLAIN)
            ? nconst + (enc_at(A, ENC_PLAIN_F, val) -
                        A.meta[ENC_M_BASE + ENC_PLAIN_F])
            : sdev + (enc_at(A, ENC_XSTR_F, val) - xbase);
      } else if ((val & 7u) == SPECIAL_ARRJSON) {
        out = sdev + (enc_at(A, ENC_XARR_F, val >> 3) - xbase);
      } else {
        out = A.meta[ENC_M_CONST + val];
      }
      tile[tid * S + j] = out;
      tp |= el << (2 * j);
    }
    A.tagpack[i] = tp;
    A.vals[i] = A.counts[i];
  }
  __syncthreads();
  const uint32_t nw = m * nk;  // words of this tile
  long long* dst = A.codes + (size_t)row0 * nk;
  longlong2* dst2 = reinterpret_cast<longlong2*>(dst);
  for (uint32_t c = tid; c < nw / 2; c += ENC_BLOCK) {
    uint32_t r = (2 * c) / nk, k = 2 * c - r * nk;
    longlong2 v;
    v.x = tile[r * S + k];
    if (++k == nk) { k = 0; r++; }
    v.y = tile[r * S + k];
    dst2[c] = v;
  }
  if ((nw & 1u) && tid == 0) dst[nw - 1] = tile[(m - 1) * S + nk - 1];
}

}  // namespace dn
