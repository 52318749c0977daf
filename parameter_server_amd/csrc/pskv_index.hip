// pskv_index.hip — CDNA4 (gfx950) kernels of a sparse shard's hash index
// (pskv_shard_create_sparse): uint32 keys -> slots of the row
// arrays, so that the row kernels (pskv_rows.hip) run unchanged on slot ids.
//
//   k_index_insert     writing calls only: every key of the call without an
//                      entry claims one (one 64-bit atomicCAS, 0 -> key + 1);
//                      the lane that wins the CAS, and only that lane, takes a
//                      slot (atomicAdd on the counter), then stores the
//                      complete entry and slot_keys[slot]
//   k_index_translate  every call, next in stream order: one uint32 slot id per
//                      key position (SparseIndex, pskv_internal.h)
//   k_index_rebuild    growth and erase (pskv_sparse_reserve, automatic growth,
//                      pskv_sparse_erase): a new table and a new
//                      slot_keys from the old slot_keys alone, on an idle shard
//   k_index_mark_dead  erase: the slot ids of the erase list set their flags
//
// Two launches, so that no lane ever waits for another: a lane that finds its
// key claimed by another lane needs the slot only in the second kernel, which
// starts after every store of the first.  Inside k_index_insert an entry is
// only ever compared by its key part, which never changes once written, so a
// stale read of an entry is either 0 (the CAS then returns the truth) or
// right.  Every probe loop ends after mask + 1 entries.
//
// A full shard (the counter at capacity): a lane that reaches an empty entry
// does not claim it, so a burst of new keys cannot fill the table with
// slotless claims.  That check races with other claimers; a lane that claims
// and then finds no slot left gives the counter back, leaves its entry
// slotless (the key stays dropped until pskv_clear or a rebuild, which leaves
// slotless entries behind: they are not in slot_keys) and sets kErrSparseFull.
//
// Work split: virtual workgroups of kGeneralChunk keys of one batch, as the row
// kernels; lane t takes the chunk's keys t, t + kBlock, ...
#include "pskv_internal.h"

namespace pskv {
namespace {

constexpr int kIndexPerLane = kGeneralChunk / kBlock;
constexpr unsigned long long kIndexKeyMask = (1ull << kIndexKeyBits) - 1ull;

// (pskv_kernels.hip's hash of the overflow table)
__device__ __forceinline__ uint32_t index_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ int index_batch_of(const GroupArgs& ga, uint32_t wg) {
  int lo = 0, hi = ga.nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ga.wg_prefix[mid] <= wg)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void index_insert_one(const SparseIndex& x, uint32_t key) {
  const unsigned long long want = (unsigned long long)key + 1ull;
  uint64_t h = index_fmix32(key) & x.mask;
  for (uint64_t probe = 0; probe <= x.mask; ++probe, h = (h + 1) & x.mask) {
    unsigned long long e = __hip_atomic_load(x.table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e == 0ull) {
      // absent so far.  Full: do not claim (the check may race; the claimer
      // below covers a lost race)
      if (__hip_atomic_load(x.stat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= x.capacity) {
        atomicOr(x.stat + 1, kErrSparseFull);
        return;
      }
      e = atomicCAS(x.table + h, 0ull, want);
      if (e == 0ull) {  // this lane claimed the entry: it alone takes the key's slot
        const uint32_t slot = atomicAdd(x.stat, 1u);
        if (slot < x.capacity) {
          __hip_atomic_store(x.table + h, want | ((unsigned long long)(slot + 1u) << kIndexKeyBits), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          x.slot_keys[slot] = key;
        } else {
          (void)atomicSub(x.stat, 1u);  // (slots below capacity are each handed out once all the same)
          atomicOr(x.stat + 1, kErrSparseFull);
        }
        return;
      }
    }
    if ((e & kIndexKeyMask) == want) return;  // claimed by another lane, or stored by an earlier call
  }
  atomicOr(x.stat + 1, kErrSparseFull);  // walked the whole table
}

// The key's slot, or 0xFFFFFFFF when it has none (absent, or claimed slotless).
__device__ __forceinline__ uint32_t index_find(const SparseIndex& x, uint32_t key, unsigned long long e) {
  const unsigned long long want = (unsigned long long)key + 1ull;
  uint64_t h = index_fmix32(key) & x.mask;
  for (uint64_t probe = 0;;) {
    if (e == 0ull) return 0xFFFFFFFFu;
    if ((e & kIndexKeyMask) == want) return (uint32_t)(e >> kIndexKeyBits) - 1u;  // slotless: 0 - 1
    if (++probe > x.mask) return 0xFFFFFFFFu;
    h = (h + 1) & x.mask;
    e = x.table[h];
  }
}

__global__ __launch_bounds__(kBlock) void k_index_insert(GroupArgs ga, SparseIndex x) {
  const uint32_t nvwg = ga.wg_prefix[ga.nb];
  for (uint32_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const int j = index_batch_of(ga, wg);
    const uint32_t* __restrict__ keys = ga.b[j].keys;
    const uint64_t n = ga.b[j].n;
    const uint64_t base = (uint64_t)(wg - ga.wg_prefix[j]) * kGeneralChunk;
    uint32_t k[kIndexPerLane];
    bool live[kIndexPerLane];
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r) {
      const uint64_t i = base + threadIdx.x + (uint32_t)r * kBlock;
      live[r] = i < n;
      k[r] = live[r] ? keys[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r)
      if (live[r]) index_insert_one(x, k[r]);
  }
}

// `out` may be the keys themselves (a host call's keys in the device staging):
// a position is read and written by one lane, read first.
template <bool WRITING>
__global__ __launch_bounds__(kBlock) void k_index_translate(GroupArgs ga, SparseIndex x) {
  const uint32_t nvwg = ga.wg_prefix[ga.nb];
  for (uint32_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const int j = index_batch_of(ga, wg);
    const uint32_t* keys = ga.b[j].keys;
    uint32_t* out = reinterpret_cast<uint32_t*>(const_cast<void*>(ga.b[j].vals));
    const uint64_t n = ga.b[j].n;
    const uint64_t base = (uint64_t)(wg - ga.wg_prefix[j]) * kGeneralChunk;
    uint32_t k[kIndexPerLane];
    bool live[kIndexPerLane];
    unsigned long long e[kIndexPerLane];
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r) {
      const uint64_t i = base + threadIdx.x + (uint32_t)r * kBlock;
      live[r] = i < n;
      k[r] = live[r] ? keys[i] : 0u;
    }
    // every key's first probe is in flight before the first is looked at
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r) e[r] = live[r] ? x.table[index_fmix32(k[r]) & x.mask] : 0ull;
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r) {
      if (!live[r]) continue;
      uint32_t id = index_find(x, k[r], e[r]);
      if (id >= x.capacity) {  // no slot
        if (WRITING) {
          id = 0xFFFFFFFFu;
          atomicOr(x.stat + 1, kErrSparseFull);
        } else {
          id = x.capacity;  // the zero row
        }
      }
      out[base + threadIdx.x + (uint32_t)r * kBlock] = id;
    }
  }
}

// One flag per slot id of an erase list (the reading translate's: an absent key
// carries `capacity`, whose flag nobody reads).  Plain stores of the same value:
// a key listed twice needs no atomic.  `dead` holds capacity + 1 flags.
__global__ __launch_bounds__(kBlock) void k_index_mark_dead(const uint32_t* __restrict__ ids, uint64_t n,
                                                            uint32_t capacity, uint8_t* __restrict__ dead) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t id = ids[i];
    if (id <= capacity) dead[id] = 1;
  }
}

// The whole index again from old_keys[0 .. count), the keys of the old slots,
// into the EMPTY table of `x` (the caller zeroed it; nothing else runs on the
// shard).  COMPACT (erase): a slot whose dead flag is set is left out and the
// live ones take new numbers from x.stat[0], which the caller zeroed -- one
// returning atomicAdd per chunk, the lanes' shares by a workgroup scan; the
// order among chunks is unspecified.  Otherwise (growth) a slot keeps its
// number and the counter is not touched.  For new slot ns: x.slot_keys[ns],
// survivors[ns] = the old slot (COMPACT only) and the complete entry, placed by
// one 64-bit CAS on an empty entry.  The keys are distinct, so no two lanes
// place the same key; no lane waits for another, and every probe loop ends
// after mask + 1 entries.  The first lane also clears the full bits of stat[1].
template <bool COMPACT>
__global__ __launch_bounds__(kBlock) void k_index_rebuild(const uint32_t* __restrict__ old_keys, uint32_t count,
                                                          const uint8_t* __restrict__ dead, SparseIndex x,
                                                          uint32_t* __restrict__ survivors) {
  __shared__ uint32_t wave_total[kBlock / 64];
  __shared__ uint32_t chunk_base;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAnd(x.stat + 1, ~(kErrSparseFull | kErrRowOutOfRange));
  const uint32_t nchunks = (count + (uint32_t)kGeneralChunk - 1u) / (uint32_t)kGeneralChunk;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // lane t takes kIndexPerLane CONSECUTIVE old slots of the chunk, so that a
    // compaction keeps the chunk's order
    const uint32_t first = c * (uint32_t)kGeneralChunk + threadIdx.x * (uint32_t)kIndexPerLane;
    uint32_t k[kIndexPerLane];
    bool live[kIndexPerLane];
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r) {
      const uint32_t i = first + (uint32_t)r;
      live[r] = i < count && !(COMPACT && dead[i]);
      k[r] = live[r] ? old_keys[i] : 0u;
      mine += live[r] ? 1u : 0u;
    }
    // every key's first probe is in flight before the first is looked at
    unsigned long long e[kIndexPerLane];
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r)
      e[r] = live[r] ? __hip_atomic_load(x.table + (index_fmix32(k[r]) & x.mask), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT)
                     : 0ull;
    uint32_t ns = first;
    if (COMPACT) {
      // exclusive scan of `mine` over the workgroup: inside the wave by shuffles,
      // across the four waves through LDS
      const uint32_t wl = threadIdx.x & 63u, wv = threadIdx.x >> 6;
      uint32_t incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (wl >= (uint32_t)d) incl += up;
      }
      if (wl == 63u) wave_total[wv] = incl;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < kBlock / 64; ++w) total += wave_total[w];
        chunk_base = total ? atomicAdd(x.stat, total) : 0u;
      }
      __syncthreads();
      ns = chunk_base + incl - mine;
      for (uint32_t w = 0; w < wv; ++w) ns += wave_total[w];
      __syncthreads();  // (the next chunk writes wave_total and chunk_base again)
    }
#pragma unroll
    for (int r = 0; r < kIndexPerLane; ++r) {
      if (!live[r]) {
        if (!COMPACT) ++ns;
        continue;
      }
      const uint32_t slot = ns++;
      if (slot >= x.capacity) continue;  // (cannot happen: at most `count` <= capacity slots are handed out)
      x.slot_keys[slot] = k[r];
      if (COMPACT) survivors[slot] = first + (uint32_t)r;
      const unsigned long long entry =
          ((unsigned long long)k[r] + 1ull) | ((unsigned long long)(slot + 1u) << kIndexKeyBits);
      uint64_t h = index_fmix32(k[r]) & x.mask;
      unsigned long long seen = e[r];
      for (uint64_t probe = 0; probe <= x.mask; ++probe) {
        // (a stale 0 only costs a failed CAS; entries are never emptied here)
        if (seen == 0ull && atomicCAS(x.table + h, 0ull, entry) == 0ull) break;
        h = (h + 1) & x.mask;
        seen = __hip_atomic_load(x.table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

uint32_t index_grid(uint32_t nwg) { return nwg < 4096u ? nwg : 4096u; }

}  // namespace

hipError_t launch_index_insert(const GroupArgs& ga, uint32_t nwg, const SparseIndex& x, hipStream_t st) {
  if (nwg == 0) return hipSuccess;
  k_index_insert<<<index_grid(nwg), kBlock, 0, st>>>(ga, x);
  return hipGetLastError();
}

hipError_t launch_index_translate(bool writing, const GroupArgs& ga, uint32_t nwg, const SparseIndex& x,
                                  hipStream_t st) {
  if (nwg == 0) return hipSuccess;
  if (writing)
    k_index_translate<true><<<index_grid(nwg), kBlock, 0, st>>>(ga, x);
  else
    k_index_translate<false><<<index_grid(nwg), kBlock, 0, st>>>(ga, x);
  return hipGetLastError();
}

hipError_t launch_index_mark_dead(const uint32_t* ids, uint64_t n, uint32_t capacity, uint8_t* dead, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const uint64_t nwg = (n + kBlock - 1) / kBlock;
  k_index_mark_dead<<<nwg < 4096u ? (uint32_t)nwg : 4096u, kBlock, 0, st>>>(ids, n, capacity, dead);
  return hipGetLastError();
}

hipError_t launch_index_rebuild(const uint32_t* old_keys, uint32_t count, const uint8_t* dead, const SparseIndex& x,
                                uint32_t* survivors, hipStream_t st) {
  // (count == 0: one workgroup still clears the full bits)
  const uint32_t nchunks = (count + (uint32_t)kGeneralChunk - 1u) / (uint32_t)kGeneralChunk;
  const uint32_t grid = index_grid(nchunks ? nchunks : 1u);
  if (dead)
    k_index_rebuild<true><<<grid, kBlock, 0, st>>>(old_keys, count, dead, x, survivors);
  else
    k_index_rebuild<false><<<grid, kBlock, 0, st>>>(old_keys, count, nullptr, x, nullptr);
  return hipGetLastError();
}

}  // namespace pskv
