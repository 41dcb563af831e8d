// In-place growth of the scan tables, DEVICE ONLY: move every ready
// slot of a populated table into a larger, zeroed one between two scan
// launches (engine/capacity.py decides when; ScanState::grow_* binds the
// result).  One thread per OLD slot.  Every entry of a table is
// distinct, so a re-insert never compares keys: it claims the first
// empty slot on the entry's probe chain, with the scan's own hash, so a
// later scan probe finds it where it looks.
#pragma once
#include "scan_tables.h"

namespace dn {

// Claim the first empty slot of h's probe chain -> slot, or ~0u after
// max_probes.  A slot another thread holds (claimed or ready) belongs
// to a different entry and is ready by the end of the kernel, so
// walking past it keeps the chain free of holes.
DEV uint32_t rehash_claim(uint32_t* state, uint32_t nslots, uint64_t h,
                          uint32_t max_probes) {
  uint32_t mask = nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes < max_probes;
       probes++, s = (s + 1) & mask) {
    if (atomic_load_relaxed(&state[s]) != SLOT_EMPTY) continue;
    if (atomicCAS(&state[s], SLOT_EMPTY, SLOT_CLAIMED) == SLOT_EMPTY)
      return s;
  }
  return 0xFFFFFFFFu;
}

// Aggregation table: same MAX_KEY key words, same count.  Each key is
// inserted once, so the count is a store, not an accumulation.  The
// probe cap is the scan's (AGG_MAX_PROBES): an entry placed further out
// would be invisible to agg_insert.  A failed placement raises
// overflow[0] (the C_OVERFLOW counter): the engine then fails loudly.
__global__ void rehash_agg_kernel(AggTable Old, AggTable New,
                                  unsigned long long* overflow) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= Old.nslots) return;
  if (Old.state[s] != SLOT_READY) return;
  uint32_t key[MAX_KEY];
#pragma unroll
  for (int k = 0; k < MAX_KEY; k++) key[k] = Old.keys[s * MAX_KEY + k];
  uint32_t d = rehash_claim(New.state, New.nslots,
                            agg_table_hash(key, MAX_KEY), AGG_MAX_PROBES);
  if (d == 0xFFFFFFFFu) { atomicAdd(overflow, 1ull); return; }
#pragma unroll
  for (int k = 0; k < MAX_KEY; k++)
    atomic_store_relaxed(&New.keys[d * MAX_KEY + k], key[k]);
  atomic_store_relaxed(&New.count[d], Old.count[s]);
  drain_stores();
  atomic_store_relaxed(&New.state[d], SLOT_READY);
}

// String dictionary: re-insert by the STORED hash; hash, id, off and
// len move unchanged (ids are what the aggregation keys hold, offsets
// point into the payload blob, which the host copies to the same
// offsets).  data_used / next_id are not touched.
__global__ void rehash_strdict_kernel(StrDict Old, StrDict New,
                                      unsigned long long* overflow) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= Old.nslots) return;
  if (Old.state[s] != SLOT_READY) return;
  uint64_t h = Old.hash[s];
  uint32_t d = rehash_claim(New.state, New.nslots, h, New.nslots);
  if (d == 0xFFFFFFFFu) { atomicAdd(overflow, 1ull); return; }
  atomic_store_relaxed(&New.hash[d], h);
  atomic_store_relaxed(&New.id[d], Old.id[s]);
  atomic_store_relaxed(&New.off[d], Old.off[s]);
  atomic_store_relaxed(&New.len[d], Old.len[s]);
  drain_stores();
  atomic_store_relaxed(&New.state[d], SLOT_READY);
}

// Number dictionary: re-insert by intern_number's hash of the stored
// bits; ids unchanged, next_id not touched.
__global__ void rehash_numdict_kernel(NumDict Old, NumDict New,
                                      unsigned long long* overflow) {
  uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= Old.nslots) return;
  if (Old.state[s] != SLOT_READY) return;
  uint64_t bits = Old.bits[s];
  uint32_t d = rehash_claim(New.state, New.nslots, number_hash(bits),
                            New.nslots);
  if (d == 0xFFFFFFFFu) { atomicAdd(overflow, 1ull); return; }
  atomic_store_relaxed(&New.bits[d], bits);
  atomic_store_relaxed(&New.id[d], Old.id[s]);
  drain_stores();
  atomic_store_relaxed(&New.state[d], SLOT_READY);
}

}  // namespace dn
