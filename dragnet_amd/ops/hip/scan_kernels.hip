// dragnet_amd MI355X scan engine — fused CDNA4 kernel.
//
// One kernel pass implements the reference's entire per-record hot path
// (reference lib/stream-scan.js:40-94 pipeline):
// NDJSON tokenize + dotted-path field extraction (K1), krill predicate
// bytecode (K2), ISO-8601 date parse (K3), p2/linear bucketize (K4),
// string/number dictionary interning, and multi-metric hash aggregation
// (K5/K6) — one thread per record, grid-stride, with an LDS combining
// cache in front of the global tables so HBM atomics scale with the
// number of distinct keys per block, not with record count.
//
// Cross-workgroup table publication uses relaxed agent-scope atomic
// stores (write-through to the coherence point) with a vmcnt drain
// before the READY flag — the placement-independent protocol of the
// CDNA4 programming guide (§6 Guideline 16, form R1) — so no acquire
// fences (L1 invalidates) appear on the hot path.
//
// Layers (docs/DESIGN.md): scan_text.h, scan_record.h (record semantics,
// host-compilable too), scan_tables.h (device only), the kernels here,
// scan_rehash.h (device only: table growth between launches),
// scan_columns.h (device only: the index queries over typed columns).

#include "common.h"
#include <hip/hip_runtime.h>

// ONE top-level declaration around the layers and the kernels: clang
// emits deferred globals (P10_TBL, DIM_TBL) at the end of each, and
// their place in the module's order shows in the assembly.  The block
// keeps the device assembly byte-identical to the single-file form.
extern "C++" {
#include "scan_text.h"
#include "scan_record.h"
#include "scan_tables.h"

namespace dn {

// MFMA column-sum reduce: count[s] += sum_r partial[r][s], computed as
// ones[16,4] x partial-tile[4,16] on the f64 matrix core
// (v_mfma_f64_16x16x4_f64; A = all-ones so every accumulator row holds
// the column sum).  One wave per 16-slot tile x gridDim.y row splits.
typedef double dn_d4 __attribute__((ext_vector_type(4)));

__global__ void mfma_reduce_kernel(AggTable T, uint32_t rows_per_blk) {
  uint32_t slot0 = blockIdx.x * 16;
  uint32_t r0 = blockIdx.y * rows_per_blk;
  uint32_t r1 = r0 + rows_per_blk;
  if (r1 > T.prows) r1 = T.prows;
  int l = threadIdx.x;
  uint32_t n = slot0 + (l & 15);
  dn_d4 acc = {0.0, 0.0, 0.0, 0.0};
  const double* P = T.partial;
  size_t stride = T.nslots;
  for (uint32_t rt = r0; rt < r1; rt += 4) {
    uint32_t rr = rt + (uint32_t)(l >> 4);
    // B fragment: lane l holds B[k = l>>4][j = l&15]
    double b = (rr < r1 && n < T.nslots)
                   ? P[(size_t)rr * stride + n] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, b, acc, 0, 0, 0);
  }
  // C/D map: lane l holds D[(l>>4)*4 + reg, l&15]; rows identical
  // (A = ones), so lanes 0..15 publish their column's sum
  if (l < 16 && n < T.nslots) {
    double v = acc[0];
    if (v != 0.0) atomicAdd(&T.count[n], v);
  }
}

// ---- newline indexing (device-side, no host sync) ----
// Three passes over 2 KiB segments: count, exclusive-scan, write.
// Positions come out globally sorted because each segment writes its
// newlines in order at its scanned base offset.

constexpr uint32_t NL_SEG = 2048;

// SWAR newline mask: high bit set in each byte lane equal to '\n'.
// EXACT per-byte form: the classic (x-0x01..)&~x&0x80.. zero test is
// only exact as a boolean — a borrow out of a true-zero byte false-
// positives the next byte when it is 0x01 (i.e. the byte 0x0B right
// after a real '\n'; caught by the envelope-crossing fuzzer on binary
// garbage lines).  This form has no cross-byte carries.
DEV uint32_t nl_mask32(uint32_t w) {
  uint32_t x = w ^ 0x0A0A0A0Au;            // zero byte where '\n'
  uint32_t y = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;  // hi set iff low7!=0
  return ~(y | x | 0x7F7F7F7Fu);           // hi set iff byte==0
}

// byte-validity mask for a word at byte address wpos over [start, n)
DEV uint32_t range_mask32(uint32_t wpos, uint32_t start, uint32_t n) {
  uint32_t m = 0x80808080u;
  if (wpos >= start && wpos + 4 <= n) return m;  // interior fast path
  uint32_t out = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    uint32_t pos = wpos + b;
    if (pos >= start && pos < n) out |= 0x80u << (b * 8);
  }
  return out;
}

// One WAVE per 2 KiB segment: lane l reads 16 B at seg*2048 +
// half*1024 + l*16 — fully coalesced 1 KiB wave-lines.  (The previous
// thread-per-segment walk gathered 64 addresses 2 KiB apart per load
// and measured ~240 GB/s; this form is read-bandwidth-bound.)
__global__ void newline_count_kernel(const uint8_t* data,
                                     uint32_t start, uint32_t n,
                                     uint32_t* seg_counts,
                                     uint32_t nseg) {
  uint32_t seg = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  uint32_t lane = threadIdx.x & 63u;
  const uint4* p16 = reinterpret_cast<const uint4*>(data);
  uint32_t base0 = (start & ~15u) + seg * NL_SEG;
  uint32_t cnt = 0;
#pragma unroll
  for (int half = 0; half < 2; half++) {
    uint32_t base = base0 + half * 1024u + lane * 16u;
    if (base < n) {
      uint4 v = p16[base >> 4];
      uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int wi = 0; wi < 4; wi++)
        cnt += __popc(nl_mask32(w[wi]) &
                      range_mask32(base + wi * 4, start, n));
    }
  }
  for (int off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (lane == 0) seg_counts[seg] = cnt;
}

// single-block exclusive scan over seg_counts (nseg can be large; a
// 1024-thread block walks tiles with a running carry)
__global__ void newline_scan_kernel(uint32_t* seg_counts, uint32_t nseg,
                                    uint32_t* total_out) {
  __shared__ uint32_t tile[1024];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nseg; base += 1024) {
    uint32_t i = base + threadIdx.x;
    uint32_t v = (i < nseg) ? seg_counts[i] : 0;
    tile[threadIdx.x] = v;
    __syncthreads();
    // Hillis-Steele inclusive scan in LDS
    for (uint32_t d = 1; d < 1024; d <<= 1) {
      uint32_t t = (threadIdx.x >= d) ? tile[threadIdx.x - d] : 0;
      __syncthreads();
      tile[threadIdx.x] += t;
      __syncthreads();
    }
    uint32_t incl = tile[threadIdx.x];
    if (i < nseg) seg_counts[i] = carry + incl - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry += tile[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ void newline_write_kernel(const uint8_t* data,
                                     uint32_t start, uint32_t n,
                                     const uint32_t* seg_offsets,
                                     uint32_t nseg, uint32_t* out_pos,
                                     uint32_t cap) {
  // wave-per-segment, coalesced (see newline_count_kernel); per-half
  // lane-exclusive scan of newline counts keeps positions sorted:
  // lane l's bytes precede lane l+1's, half 0 precedes half 1
  uint32_t seg = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  uint32_t lane = threadIdx.x & 63u;
  const uint4* p16 = reinterpret_cast<const uint4*>(data);
  uint32_t base0 = (start & ~15u) + seg * NL_SEG;
  uint32_t w_at = seg_offsets[seg];
#pragma unroll
  for (int half = 0; half < 2; half++) {
    uint32_t base = base0 + half * 1024u + lane * 16u;
    uint32_t m[4] = {0, 0, 0, 0};
    uint32_t cnt = 0;
    if (base < n) {
      uint4 v = p16[base >> 4];
      uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int wi = 0; wi < 4; wi++) {
        m[wi] = nl_mask32(w[wi]) &
                range_mask32(base + wi * 4, start, n);
        cnt += __popc(m[wi]);
      }
    }
    // lane-exclusive scan of cnt
    uint32_t incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
      uint32_t t = __shfl_up(incl, off, 64);
      if ((int)lane >= off) incl += t;
    }
    uint32_t at = w_at + incl - cnt;
#pragma unroll
    for (int wi = 0; wi < 4; wi++) {
      uint32_t mm = m[wi];
      while (mm) {
        uint32_t b = ((uint32_t)__ffs(mm) - 1) >> 3;  // byte lane
        if (at < cap) out_pos[at] = base + wi * 4 + b;
        at++;
        mm &= mm - 1;
      }
    }
    w_at += __shfl(incl, 63, 64);  // wave total
  }
}

// Device-side wave-transpose builder: scatter each (length-sorted)
// record's bytes into the granule-interleaved layout scan_kernel_x
// consumes (byte p of slot r -> wbase[r/64] + (p/gran)*(64*gran) +
// (r%64)*gran + p%gran).  One wave per 64-slot transposed wave: for a
// fixed granule g the 64 lanes write 64 CONSECUTIVE granules (fully
// coalesced 2 KiB stores); reads are per-record gathers (the cost the
// transpose exists to pay once instead of every scan pass).
__global__ void xpose_build_kernel(const uint8_t* __restrict__ data,
                                   const uint32_t* __restrict__ sstart,
                                   const uint32_t* __restrict__ slen,
                                   const unsigned long long* __restrict__ wbase,
                                   uint32_t n_slots, int gran_log,
                                   uint8_t* __restrict__ xb) {
  uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  uint32_t nw = n_slots >> 6;
  if (w >= nw) return;
  uint32_t lane = threadIdx.x & 63u;
  uint32_t r = (w << 6) + lane;
  uint32_t gran = 1u << gran_log;
  unsigned long long base = wbase[w];
  uint32_t gw = (uint32_t)((wbase[w + 1] - base) >> (6 + gran_log));
  uint32_t len = slen[r];
  if (len == 0xFFFFFFFFu) len = 0;  // padding slot
  uint32_t start = sstart[r];
  uint8_t* dst0 = xb + base + ((size_t)lane << gran_log);
  for (uint32_t g = 0; g < gw; g++) {
    uint8_t* dst = dst0 + ((size_t)g << (6 + gran_log));
    uint32_t off = g << gran_log;
    for (uint32_t k = 0; k < gran; k += 16) {
      uint8_t tmp[16];
#pragma unroll
      for (int t = 0; t < 16; t++) {
        uint32_t o = off + k + t;
        tmp[t] = (o < len) ? data[start + o] : (uint8_t)'\n';
      }
      uint4 vv;
      __builtin_memcpy(&vv, tmp, 16);
      *reinterpret_cast<uint4*>(dst + k) = vv;
    }
  }
}

template <int XP>
DEV void scan_kernel_body(char* smem, ScanArgs A);

__launch_bounds__(BLOCK)
__global__ void scan_kernel(ScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem0[];
  scan_kernel_body<0>(smem0, A);
}

// occupancy-capped variants (min waves per SIMD; constrains the
// register allocator) — selected at runtime for A/B measurement
template <int MW>
__launch_bounds__(BLOCK, MW)
__global__ void scan_kernel_mw(ScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem1[];
  scan_kernel_body<0>(smem1, A);
}
template __global__ void scan_kernel_mw<2>(ScanArgs);
template __global__ void scan_kernel_mw<3>(ScanArgs);
template __global__ void scan_kernel_mw<4>(ScanArgs);
template __global__ void scan_kernel_mw<5>(ScanArgs);
template __global__ void scan_kernel_mw<6>(ScanArgs);

// wave-transposed record staging (XBytesT; DRAGNET_XPOSE).
// second parameter = log2 granule bytes (DRAGNET_XGRAN)
template <int MW, int XLG>
__launch_bounds__(BLOCK, MW)
__global__ void scan_kernel_x(ScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem2[];
  scan_kernel_body<XLG>(smem2, A);
}
template __global__ void scan_kernel_x<2, 6>(ScanArgs);
template __global__ void scan_kernel_x<3, 6>(ScanArgs);
template __global__ void scan_kernel_x<4, 6>(ScanArgs);
template __global__ void scan_kernel_x<5, 6>(ScanArgs);
template __global__ void scan_kernel_x<4, 5>(ScanArgs);
template __global__ void scan_kernel_x<4, 7>(ScanArgs);

// Per-record pipeline (K1-K6) shared by the linear and the
// wave-transposed (XBytes) kernels: tokenize/extract, predicate,
// synthetics, per-metric filter + bucketize + intern + aggregate.
#define synth_val_at(si) synth_lds[(si) * BLOCK + threadIdx.x]

template <class BS>
DEV void process_record(BS BV, uint32_t start, uint32_t end,
                        const ScanArgs& A, const PlanView& P, FV& fv,
                        unsigned long long* lcnt, LdsCacheEntry* cache,
                        uint64_t* sig_lds, double* synth_lds) {
  const int nf = P.nf;
  uint32_t synth_ok = 0;
  atomicAdd(&lcnt[C_LINES], 1ull);
  // only the type lane needs initializing: soff/slen/num are read
  // only after a capture set them
  for (int f = 0; f < nf; f++)
    fv.type[f * BLOCK + fv.tid] = T_MISSING;

  uint8_t top_type;
  bool ok = (end > start) &&
            parse_record(BV, start, end, P, fv, top_type, sig_lds,
                         A.data_format_skinner);
  double weight = 1.0;
  if (ok && A.data_format_skinner) {
    // require: object top, a "fields" member, numeric "value"
    bool has_fields = P.fields_slot >= 0 &&
                      fv.get_type(P.fields_slot) != T_MISSING;
    bool val_num = P.value_slot >= 0 &&
                   fv.get_type(P.value_slot) == T_NUM;
    if (top_type != T_OBJ || !has_fields || !val_num) ok = false;
    else weight = fv.get_num(P.value_slot);
  }
  if (!ok) {
    atomicAdd(&lcnt[C_INVALID_JSON], 1ull);
  } else {
    atomicAdd(&lcnt[C_PARSED], 1ull);

    // datasource filter (program 0)
    int keep = eval_predicate(P, BV, fv, 0);
    if (keep == -1) atomicAdd(&lcnt[C_DS_FAILEDEVAL], 1ull);
    else if (keep == 0) atomicAdd(&lcnt[C_DS_FILTERED], 1ull);

    if (keep == 1) {
      // synthetic date fields (shared across metrics)
      synth_ok = 0;
      for (int si = 0; si < P.ns; si++) {
        int slot = P.synth_slots[si];
        uint8_t t = fv.get_type(slot);
        uint32_t ok;
        if (t == T_MISSING) ok = 2;                           // undef
        else if (t == T_NUM) {
          ok = 1; synth_val_at(si) = fv.get_num(slot);
        } else if (t == T_STR) {
          DateOut d = parse_iso_ms(BV, fv.get_soff(slot),
                                   fv.get_slen(slot));
          if (d.ok) {
            long long secs = d.ms >= 0 ? d.ms / 1000
                                       : (d.ms - 999) / 1000;
            ok = 1; synth_val_at(si) = (double)secs;
          } else ok = 3;                                      // baddate
        } else ok = 3;  // bool/null/obj/arr: Date.parse fails
        synth_ok |= ok << (2 * si);
      }

      // per-metric pipeline
      for (int m = 0; m < P.nm; m++) {
        const int32_t* M = &P.metric_rows[m * 8];
        unsigned long long* mc = &lcnt[C_GLOBAL_N + m * CM_N];
        atomicAdd(&mc[CM_FILTER_IN], 1ull);

        int res = eval_predicate(P, BV, fv, M[0]);
        if (res == -1) { atomicAdd(&mc[CM_FAILEDEVAL], 1ull); continue; }
        if (res == 0) { atomicAdd(&mc[CM_FILTERED], 1ull); continue; }

        // synthetic requirements (first failure counted; record
        // dropped on any failure — stream-synthetic.js:37-85)
        bool sok = true;
        for (int k = 0; k < M[3]; k++) {
          int si = P.synth_req[M[4] + k];
          uint32_t ok = (synth_ok >> (2 * si)) & 3u;
          if (ok != 1) {
            atomicAdd(&mc[ok == 2 ? CM_UNDEF : CM_BADDATE], 1ull);
            sok = false; break;
          }
        }
        if (!sok) continue;

        // time filter on dn_ts (= last synth req when present)
        if (M[5]) {
          int si = P.synth_req[M[4] + M[3] - 1];
          double ts = synth_val_at(si);
          if (!(ts >= (double)M[6] && ts < (double)M[7])) {
            atomicAdd(&mc[CM_TIME_OUT], 1ull); continue;
          }
        }

        atomicAdd(&mc[CM_AGG_IN], 1ull);

        // build the group key (K4: bucketize; dict-intern)
        uint32_t key[MAX_KEY];
        int nk = M[1];
        bool drop = false, overflow = false;
        for (int bi = 0; bi < nk; bi++) {
          const int32_t* B = &P.bd_rows[(M[2] + bi) * 4];
          double step = P.bd_steps[M[2] + bi];
          uint8_t t; double num = 0.0; uint32_t so = 0, sl = 0;
          if (B[0] == 1) {  // synthetic date value
            int si = B[1];
            if (((synth_ok >> (2 * si)) & 3u) == 1) {
              t = T_NUM; num = synth_val_at(si);
            } else t = T_MISSING;  // cannot happen: required above
          } else {
            int slot = B[1];
            // aggregation lookup is literal-first (points.lookup):
            // a top-level literal dotted key (companion slot)
            // shadows the plucked nested value
            int cs2 = P.comp_slot[slot];
            if (cs2 >= 0 && fv.get_type(cs2) != T_MISSING)
              slot = cs2;
            t = fv.get_type(slot);
            num = fv.get_num(slot);
            so = fv.get_soff(slot); sl = fv.get_slen(slot);
          }
          uint32_t code;
          if (!encode_key_col(A.sdict, A.ndict, BV, t, num, so, sl, B[2],
                              step, code, drop, overflow))
            break;
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

        uint64_t kh = agg_key_hash(m, key);

        // Wave-level pre-combining: lanes carrying the same key
        // elect one leader per distinct kh which adds the whole
        // group's weight — one LDS atomic per distinct key per
        // wavefront instead of one per record.  (Only when every
        // weight is 1: json format; skinner weights vary.)
        if (!A.data_format_skinner) {
          uint64_t unproc = __ballot(true);  // lanes still here
          bool leader = false;
          double wsum = 0.0;
          while (unproc) {
            int src = (int)(__ffsll((long long)unproc) - 1);
            uint64_t src_kh = __shfl(kh, src);
            bool same = (kh == src_kh);
            uint64_t grp = __ballot(same);
            if (same && __lane_id() == src) {
              leader = true;
              wsum = (double)__popcll(grp);
            }
            unproc &= ~grp;
          }
          if (!leader) continue;  // combined into the leader's add
          weight = wsum;
        }
        lds_cache_add<1>(cache, A.tables, A.counters, lcnt, m, key, nk, kh,
                      weight);
      }
    }
  }
}

template <int XP>
DEV void scan_kernel_body(char* smem, ScanArgs A) {
  const PlanView& P = A.P;
  const int nf = P.nf;

  const LdsLayout L(nf, P.nm, P.ns, true);
  LdsCacheEntry* cache = reinterpret_cast<LdsCacheEntry*>(smem + L.cache);
  unsigned long long* lcnt =
      reinterpret_cast<unsigned long long*>(smem + L.lcnt);
  const int NCNT = C_GLOBAL_N + P.nm * CM_N;
  double* synth_lds = reinterpret_cast<double*>(smem + L.synth);
  uint64_t* sig_lds = reinterpret_cast<uint64_t*>(smem + L.sig);
  uint8_t* tile = reinterpret_cast<uint8_t*>(smem + L.tile);  // staging
  block_agg_init(cache, lcnt, NCNT);

  FV fv;
  fv.type = reinterpret_cast<uint8_t*>(smem + L.fv_type);
  fv.soff = reinterpret_cast<uint32_t*>(smem + L.fv_soff);
  fv.slen = reinterpret_cast<uint32_t*>(smem + L.fv_slen);
  fv.tid = threadIdx.x;

  if constexpr (XP != 0) {
    // wave-transposed pool (XP = log2 granule bytes): slot r's bytes
    // live granule-interleaved at xwave_base[r/64] + (r%64)*GRAN; a
    // wave's refills are 64 consecutive granules (coalesced) instead
    // of 64 scattered records.  Record order is length-sorted by the
    // host — the aggregation is order-independent (associative
    // merge).
    const uint32_t stride_x = gridDim.x * BLOCK;
    for (uint32_t rbase = blockIdx.x * BLOCK; rbase < A.xn_slots;
         rbase += stride_x) {
      uint32_t r = rbase + threadIdx.x;
      if (r < A.xn_slots) {
        uint32_t len = A.xrec_len[r];
        if (len != 0xFFFFFFFFu) {
          XBytesT<XP> BV;
          BV.base = A.xdata + A.xwave_base[r >> 6]
                    + ((size_t)(r & 63u) << XP);
          process_record(BV, 0u, len, A, P, fv, lcnt, cache, sig_lds,
                         synth_lds);
        }
      }
    }
  } else {
  uint32_t nlines = *A.nlines_ptr;
  if (nlines > A.pos_cap) nlines = A.pos_cap;
  const uint32_t stride = gridDim.x * BLOCK;
  for (uint32_t rbase = blockIdx.x * BLOCK; rbase < nlines;
       rbase += stride) {
    uint32_t r = rbase + threadIdx.x;
    bool active = r < nlines;

    // Block-level LDS staging: copy the block's contiguous record
    // span into the tile with coalesced uint4 loads, then parse from
    // LDS (banked reads) instead of 64-way divergent global gathers.
    Bytes BV;
    BV.mem = A.data;
    BV.bias = 0;
    uint32_t t_start = rbase ? A.nl_pos[rbase - 1] + 1 : A.first_start;
    uint32_t r_last = rbase + BLOCK - 1;
    if (r_last >= nlines) r_last = nlines - 1;
    uint32_t t_end = A.nl_pos[r_last] + 1;
    uint32_t t_base = t_start & ~15u;
    uint32_t span = t_end - t_base;
    bool staged = A.tile_cap >= 16 && span <= A.tile_cap;
    if (staged) {
      const uint4* g16 = reinterpret_cast<const uint4*>(A.data + t_base);
      uint4* l16 = reinterpret_cast<uint4*>(tile);
      uint32_t n16 = (span + 15) >> 4;
      for (uint32_t i = threadIdx.x; i < n16; i += BLOCK)
        l16[i] = g16[i];
      __syncthreads();
      BV.mem = tile;
      BV.bias = t_base;
    }

    if (active) {
      uint32_t start = r ? A.nl_pos[r - 1] + 1 : A.first_start;
      uint32_t end = A.nl_pos[r];
      process_record(BV, start, end, A, P, fv, lcnt, cache, sig_lds,
                     synth_lds);
    }

    if (staged) __syncthreads();  // tile reused next iteration
  }
  }  // XP

  block_agg_flush(cache, lcnt, NCNT, P, A.tables, A.counters);
}

// -------------------------------------------------------------------
// extraction kernels

__global__ void extract_agg_kernel(AggTable T, uint32_t* out_keys,
                                   double* out_counts, uint32_t* out_n,
                                   uint32_t max_out) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= T.nslots) return;
  if (atomic_load_relaxed(&T.state[s]) != SLOT_READY) return;
  uint32_t i = atomicAdd(out_n, 1u);
  if (i >= max_out) return;
  for (int k = 0; k < MAX_KEY; k++)
    out_keys[i * MAX_KEY + k] = T.keys[s * MAX_KEY + k];
  out_counts[i] = T.count[s];
}

__global__ void extract_strdict_kernel(StrDict D, uint32_t* out_off,
                                       uint32_t* out_len, uint32_t max_ids) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= D.nslots) return;
  if (atomic_load_relaxed(&D.state[s]) != SLOT_READY) return;
  uint32_t id = D.id[s];
  if (id >= max_ids) return;
  out_off[id] = D.off[s];
  out_len[id] = D.len[s];
}

__global__ void extract_numdict_kernel(NumDict D, double* out_vals,
                                       uint32_t max_ids) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= D.nslots) return;
  if (atomic_load_relaxed(&D.state[s]) != SLOT_READY) return;
  uint32_t id = D.id[s];
  if (id >= max_ids) return;
  out_vals[id] = __longlong_as_double(
      (long long)atomic_load_relaxed(&D.bits[s]));
}

}  // namespace dn

// in-place table growth (the rehash kernels); last, so the kernels
// above keep their place in the module
#include "scan_rehash.h"

// index queries over typed columns (K7 and the columnar sidecars);
// after everything else, for the same reason
#include "scan_columns.h"

}  // extern "C++"
