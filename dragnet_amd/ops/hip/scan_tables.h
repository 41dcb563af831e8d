// Concurrent table layer of the scan engine, DEVICE ONLY: relaxed
// atomics, dictionaries, aggregation insert, the per-block LDS cache.
#pragma once
#include "scan_record.h"

namespace dn {

#define DEV __device__ __forceinline__

constexpr int LDS_CACHE = 128;    // per-block aggregation cache slots
// (halved from 256 in r2: the 7 KB buys a whole extra block of
// occupancy, which outweighs extra cache-miss fallthrough; misses
// go to the dense partial row / global table either way)

template <typename T>
DEV T atomic_load_relaxed(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
DEV void atomic_store_relaxed(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV void drain_stores() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// -------------------------------------------------------------------
// dictionaries (string + number interning)

template <class BS>
DEV uint64_t hash_bytes(BS BV, uint32_t off, uint32_t len) {
  uint64_t h = FNV_OFFSET;
  for (uint32_t k = 0; k < len; k++) h = fnv1a_byte(h, BV.at(off + k));
  return mix64(h ^ len);
}

// Returns string id, or 0xFFFFFFFF on table/data overflow.
template <class BS>
DEV uint32_t intern_string(const StrDict& D, BS BV,
                           uint32_t off, uint32_t len) {
  uint64_t h = hash_bytes(BV, off, len);
  uint32_t mask = D.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes < D.nslots; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&D.state[s]);
      if (st == SLOT_READY) {
        if (atomic_load_relaxed(&D.hash[s]) != h) break;  // next probe
        // verify bytes
        uint32_t o2 = atomic_load_relaxed(&D.off[s]);
        uint32_t l2 = atomic_load_relaxed(&D.len[s]);
        if (l2 != len) break;
        bool same = true;
        for (uint32_t k = 0; k < len; k++)
          if (D.data[o2 + k] != BV.at(off + k)) { same = false; break; }
        if (same) return atomic_load_relaxed(&D.id[s]);
        break;
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&D.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
          // we own the slot: copy payload, publish
          uint32_t o = atomicAdd(D.data_used, (len + 7u) & ~7u);
          if (o + len > D.data_cap) return 0xFFFFFFFFu;  // overflow
          for (uint32_t k = 0; k < len; k++)
            atomic_store_relaxed(&D.data[o + k], BV.at(off + k));
          uint32_t myid = atomicAdd(D.next_id, 1u);
          atomic_store_relaxed(&D.hash[s], h);
          atomic_store_relaxed(&D.off[s], o);
          atomic_store_relaxed(&D.len[s], len);
          atomic_store_relaxed(&D.id[s], myid);
          drain_stores();
          atomic_store_relaxed(&D.state[s], SLOT_READY);
          return myid;
        }
        continue;  // lost the race: re-read state
      }
      // SLOT_CLAIMED by another lane: re-read (its publish completes
      // in its own loop iteration; no blocking spin)
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return 0xFFFFFFFFu;
}

// Home-slot hash of a number-dictionary entry (canonical double bits).
DEV uint64_t number_hash(uint64_t bits) {
  return mix64(bits ^ 0x9E3779B97F4A7C15ull);
}

DEV uint32_t intern_number(const NumDict& D, double v) {
  if (v == 0.0) v = 0.0;  // canonicalize -0
  uint64_t bits = __double_as_longlong(v);
  uint64_t h = number_hash(bits);
  uint32_t mask = D.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes < D.nslots; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&D.state[s]);
      if (st == SLOT_READY) {
        if (atomic_load_relaxed(&D.bits[s]) != bits) break;
        return atomic_load_relaxed(&D.id[s]);
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&D.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
          uint32_t myid = atomicAdd(D.next_id, 1u);
          atomic_store_relaxed(&D.bits[s], bits);
          atomic_store_relaxed(&D.id[s], myid);
          drain_stores();
          atomic_store_relaxed(&D.state[s], SLOT_READY);
          return myid;
        }
        continue;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return 0xFFFFFFFFu;
}

// -------------------------------------------------------------------
// global aggregation insert (K5)

// Home-slot hash of a group key: columns past nk hash as 0, which is
// also how they are stored, so hashing a stored key with nk = MAX_KEY
// (the table rehash, scan_rehash.h) gives the inserting scan's value.
DEV uint64_t agg_table_hash(const uint32_t* key, int nk) {
  uint64_t h = FNV_OFFSET;
  for (int k = 0; k < MAX_KEY; k++)
    h = mix64(h ^ (k < nk ? key[k] : 0u) ^ (uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull);
  return h;
}

// agg_insert gives up after this many probes (C_OVERFLOW)
constexpr uint32_t AGG_MAX_PROBES = 4096u;

DEV bool agg_insert(const AggTable& T, const uint32_t* key, int nk,
                    double w) {
  uint64_t h = agg_table_hash(key, nk);
  uint32_t mask = T.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes < AGG_MAX_PROBES; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&T.state[s]);
      if (st == SLOT_READY) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < MAX_KEY; k++)
          if (k < nk &&
              atomic_load_relaxed(&T.keys[s * MAX_KEY + k]) != key[k])
            same = false;
        if (same) { atomicAdd(&T.count[s], w); return true; }
        break;
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&T.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
#pragma unroll
          for (int k = 0; k < MAX_KEY; k++)
            atomic_store_relaxed(&T.keys[s * MAX_KEY + k],
                                 k < nk ? key[k] : 0u);
          drain_stores();
          atomic_store_relaxed(&T.state[s], SLOT_READY);
          atomicAdd(&T.count[s], w);
          return true;
        }
        continue;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return false;  // pathological probe chain: table too full
}

// Directory variant for the dense-accumulation path: assign (or find)
// the key's stable slot WITHOUT touching count — counts accumulate in
// the caller's per-workgroup dense partial row and are folded by the
// MFMA reduce.  Returns the slot index or ~0u on probe exhaustion.
DEV uint32_t agg_insert_slot(const AggTable& T, const uint32_t* key,
                             int nk) {
  uint64_t h = agg_table_hash(key, nk);
  uint32_t mask = T.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  // TIGHT probe cap: once the directory saturates, every further
  // insert probe-scans to the cap before failing — with the old
  // nslots/4 cap a 5-field high-cardinality query measured 32 GB/s
  // (vs the 280 GB/s band) on its doomed first attempt; with the cap
  // + the global short-circuit it measures 150-256 GB/s.  256 probes
  // keeps the directory usable to ~85-90% load while keeping the
  // overflow attempt cheap; the engine restarts on the hash path.
  uint32_t max_probes = 256;
  for (uint32_t probes = 0; probes < max_probes; probes++, s = (s + 1) & mask) {
    while (true) {
      uint32_t st = atomic_load_relaxed(&T.state[s]);
      if (st == SLOT_READY) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < MAX_KEY; k++)
          if (k < nk &&
              atomic_load_relaxed(&T.keys[s * MAX_KEY + k]) != key[k])
            same = false;
        if (same) return s;
        break;
      }
      if (st == SLOT_EMPTY) {
        uint32_t prev = atomicCAS(&T.state[s], SLOT_EMPTY, SLOT_CLAIMED);
        if (prev == SLOT_EMPTY) {
#pragma unroll
          for (int k = 0; k < MAX_KEY; k++)
            atomic_store_relaxed(&T.keys[s * MAX_KEY + k],
                                 k < nk ? key[k] : 0u);
          drain_stores();
          atomic_store_relaxed(&T.state[s], SLOT_READY);
          return s;
        }
        continue;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return 0xFFFFFFFFu;
}

// Add one (key, weight) into a table: dense path (directory slot +
// this workgroup's partial row) or the atomic hash path.  gflag is
// the GLOBAL overflow counter: once any block overflows the dense
// directory the whole scan is doomed to restart, so later misses
// short-circuit instead of probe-scanning a saturated table.
DEV bool agg_add(const AggTable& T, const uint32_t* key, int nk,
                 double w, unsigned long long* gflag) {
  if (T.partial != nullptr) {
    if (atomic_load_relaxed(gflag) != 0ull) return false;
    uint32_t s = agg_insert_slot(T, key, nk);
    if (s == 0xFFFFFFFFu) {
      atomicAdd(gflag, 1ull);  // publish immediately (cross-block)
      return false;
    }
    atomicAdd(&T.partial[(size_t)(blockIdx.x % T.prows) * T.nslots + s],
              w);
    return true;
  }
  return agg_insert(T, key, nk, w);
}

// -------------------------------------------------------------------
// per-block LDS state of the scan and columnar kernels

struct LdsCacheEntry {
  uint64_t hash;      // 0 = empty
  uint32_t metric;
  uint32_t key[MAX_KEY];
  double count;
};

// Dynamic-LDS layout of the scan and columnar kernels:
//   fv SoA | agg cache | counters [| synthetics | sig stack] | tile
// Defined ONCE: the kernels carve their LDS with it and the host sizes
// the launch (and checks the 160 KiB budget) from the same offsets.
// parse_state adds what only the NDJSON parser needs; the columnar
// kernel has neither synthetics nor a sig stack.
struct LdsLayout {
  size_t fv_soff, fv_slen, fv_type, cache, lcnt, synth, sig, tile, total;
  __host__ __device__ __forceinline__
  LdsLayout(int nf, int nm, int ns, bool parse_state) {
    size_t off = 0;
    fv_soff = off; off += (size_t)nf * BLOCK * sizeof(uint32_t);
    fv_slen = off; off += (size_t)nf * BLOCK * sizeof(uint32_t);
    fv_type = off; off += (size_t)nf * BLOCK * sizeof(uint8_t);
    off = (off + 15) & ~(size_t)15;
    cache = off; off += (size_t)LDS_CACHE * sizeof(LdsCacheEntry);
    lcnt = off;
    off += (size_t)(C_GLOBAL_N + nm * CM_N) * sizeof(unsigned long long);
    synth = sig = off;
    if (parse_state) {
      // sized by the ACTUAL synthetic count: the flagship plan has zero
      // synthetics and an unconditional MAX_SYNTH reservation (16 KB)
      // was costing a whole extra block of occupancy per CU
      off += (size_t)ns * BLOCK * sizeof(double);
      sig = off; off += (size_t)SIG_DEPTH * BLOCK * sizeof(uint64_t);
    }
    off = (off + 15) & ~(size_t)15;
    tile = off;         // optional staging tile: ScanArgs.tile_cap bytes
    total = off + 64;   // slack
  }
};

// -------------------------------------------------------------------
// aggregation tail shared by the scan and columnar kernels: key-column
// encoding, the LDS combining cache, and its block-level init / flush

// Encode one breakdown column (value type t: num, or the span so/sl)
// to its u32 key code (K4: bucketize; dict-intern).  Returns false
// with drop set (the record is nonnumeric for a bucketized column) or
// overflow set (a dictionary is full).
template <class BS>
DEV bool encode_key_col(const StrDict& sdict, const NumDict& ndict, BS BV,
                       uint8_t t, double num, uint32_t so, uint32_t sl,
                       int bucket, double step, uint32_t& code,
                        bool& drop, bool& overflow) {
  if (bucket != BUCKET_NONE) {
    if (t == T_STR) {
      // numeric STRINGS coerce for bucketized fields (JS arithmetic in
      // the reference's bucketizer: its own golden counts
      // {"latency": "26"} into the p2 histogram —
      // tests/data/2014/05-05/more.log:1); NaN / +-Infinity drop as
      // nonnumeric
      num = js_to_number(BV, so, sl);
      if (!(num == num) || num == __builtin_inf() ||
          num == -__builtin_inf())
        { drop = true; return false; }
      t = T_NUM;
    }
    // nonnumeric; an over-range literal (1e400) is +-Infinity and
    // drops like the Infinity strings above
    if (t != T_NUM || !finite_num(num)) { drop = true; return false; }
    double ordf = bucket_ordinal(bucket, num, step);
    if (ord_is_small(ordf)) {
      code = make_code(TAG_ORD, (uint32_t)((int)ordf + ORD_BIAS));
    } else {
      uint32_t id = intern_number(ndict, ordf);
      if (id == 0xFFFFFFFFu) { overflow = true; return false; }
      code = make_code(TAG_NUM, id);
    }
  } else if (t == T_MISSING) {
    code = make_code(TAG_SPECIAL, SPECIAL_UNDEF);
  } else if (t == T_NULL) {
    code = make_code(TAG_SPECIAL, SPECIAL_NULL);
  } else if (t == T_TRUE) {
    code = make_code(TAG_SPECIAL, SPECIAL_TRUE);
  } else if (t == T_FALSE) {
    code = make_code(TAG_SPECIAL, SPECIAL_FALSE);
  } else if (t == T_OBJ) {
    code = make_code(TAG_SPECIAL, SPECIAL_OBJECT);
  } else if (t == T_ARR) {
    // intern the raw JSON span; the host canonicalizes it with JS
    // Array.toString semantics (plan.decode_key)
    uint32_t id = intern_string(sdict, BV, so, sl);
    if (id == 0xFFFFFFFFu || id >= (1u << 27)) { overflow = true; return false; }
    code = make_code(TAG_SPECIAL, SPECIAL_ARRJSON | (id << 3));
  } else if (t == T_NUM) {
    uint32_t id = intern_number(ndict, num);
    if (id == 0xFFFFFFFFu) { overflow = true; return false; }
    code = make_code(TAG_NUM, id);
  } else {  // T_STR
    uint32_t id = intern_string(sdict, BV, so, sl);
    if (id == 0xFFFFFFFFu) { overflow = true; return false; }
    code = make_code(TAG_STR, id);
  }
  return true;
}

// LDS combining cache: hash of (metric, key); never 0 (0 = empty slot)
DEV uint64_t agg_key_hash(int m, const uint32_t* key) {
  uint64_t kh = mix64((uint64_t)m * 0x9E3779B97F4A7C15ull + 1);
  for (int k = 0; k < MAX_KEY; k++) kh = mix64(kh ^ key[k]);
  return kh == 0 ? 1 : kh;
}

// Add (metric m, key, weight) to the block's LDS cache, falling through
// to the global table when the probes are exhausted.
//
// NOTE on the LDS cache race: two lanes with DIFFERENT keys that
// collide on the same 64-bit kh would mis-combine.  kh is a 64-bit mix
// of the full key; a collision needs two distinct key tuples in one
// block with equal mix64 chains (~2^-64 per pair) — accepted and
// documented (SURVEY parity corners).  Identity (metric + key words)
// is nevertheless verified for the common same-slot case; the claim
// fill is racy only against lanes carrying the SAME kh.
//
// UNROLL is the probe loop's unroll count, fixed per kernel to the
// shape each compiled to before the loop was shared: rolled (1) in the
// scan kernels, where unrolling raises SGPR spills 226 -> 242 and
// measured 1.3% slower device-resident; fully unrolled (8) in the
// columnar kernel, where rolling raises them 165 -> 196.
template <int UNROLL>
DEV void lds_cache_add(LdsCacheEntry* cache, AggTable* tables,
                       unsigned long long* counters,
                       unsigned long long* lcnt, int m,
                       const uint32_t* key, int nk, uint64_t kh,
                       double weight) {
  bool cached = false;
  uint32_t ci = (uint32_t)kh & (LDS_CACHE - 1);
  // 8 probes: a hot key that loses every probe degrades to per-record
  // contended global inserts (measured 4x slower on low-cardinality
  // ordinal breakdowns with 2 probes)
#pragma unroll UNROLL
  for (int attempt = 0; attempt < 8; attempt++) {
    unsigned long long prev = atomicCAS(
        (unsigned long long*)&cache[ci].hash, 0ull,
        (unsigned long long)kh);
    if (prev == 0) {
      // claimed: fill identity (hash claim is the sync point;
      // same-key lanes re-check identity below)
      cache[ci].metric = m;
      for (int k = 0; k < MAX_KEY; k++) cache[ci].key[k] = key[k];
      atomicAdd(&cache[ci].count, weight);
      cached = true;
      break;
    }
    if (prev == (unsigned long long)kh && cache[ci].metric == m) {
      bool same = true;
      for (int k = 0; k < MAX_KEY; k++)
        if (cache[ci].key[k] != key[k]) { same = false; break; }
      if (same) {
        atomicAdd(&cache[ci].count, weight);
        cached = true;
        break;
      }
    }
    ci = (ci + 1) & (LDS_CACHE - 1);
  }
  if (!cached) {
    if (!agg_add(tables[m], key, nk, weight, &counters[C_OVERFLOW]))
      atomicAdd(&lcnt[C_OVERFLOW], 1ull);
  }
}

// Block start: empty the cache and zero the block-local counters.
DEV void block_agg_init(LdsCacheEntry* cache, unsigned long long* lcnt,
                        int ncnt) {
  for (int i = threadIdx.x; i < LDS_CACHE; i += BLOCK) {
    cache[i].hash = 0;
    cache[i].metric = 0;
    for (int k = 0; k < MAX_KEY; k++) cache[i].key[k] = 0;
    cache[i].count = 0.0;
  }
  for (int i = threadIdx.x; i < ncnt; i += BLOCK) lcnt[i] = 0;
  __syncthreads();
}

// Block end: flush the cache into the global tables, then the
// block-local counters into the global ones.
DEV void block_agg_flush(LdsCacheEntry* cache, unsigned long long* lcnt,
                         int ncnt, const PlanView& P, AggTable* tables,
                         unsigned long long* counters) {
  __syncthreads();
  for (int i = threadIdx.x; i < LDS_CACHE; i += BLOCK) {
    if (cache[i].hash != 0) {
      if (!agg_add(tables[cache[i].metric], cache[i].key,
                   P.metric_rows[cache[i].metric * 8 + 1],
                   cache[i].count, &counters[C_OVERFLOW]))
        atomicAdd(&lcnt[C_OVERFLOW], 1ull);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncnt; i += BLOCK) {
    if (lcnt[i]) atomicAdd(&counters[i], lcnt[i]);
  }
}

}  // namespace dn
