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
// slotless (the key stays dropped until pskv_clear) and sets kErrSparseFull.
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

}  // namespace pskv
