// pskv_plan.h — the host planner: the pure arithmetic of a shard's host paths
// (pskv_shard.cpp).  How a call's batches are cut into pieces, launch groups
// and DMA windows, where each batch lies in a staging buffer, the vectorised
// key check of host inputs, K5's bucket rule, the bags, chunks and windows
// of a pooled pull, the bag of a position of a pooled push, and the launch
// groups, descriptors and staging of a grouped pooled push (the part the
// kernels share is marked PSKV_HD), the optimizer's state slots and a sparse
// shard's sizes and growth rule.  No HIP and
// no shard state: everything here is a function of its arguments, so it is
// tested on the CPU (tests/cpp/host_plan_test.cpp, tests/cpp/pooled_plan_test.cpp,
// tests/cpp/pooled_push_plan_test.cpp, tests/cpp/pooled_push_group_plan_test.cpp,
// tests/cpp/sparse_plan_test.cpp).  Internal linkage throughout: libpskv.so
// exports nothing from this header (the types the kernels do not share are in
// an unnamed namespace, so that no instantiation over them is exported either).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "pskv.h"

namespace pskv {

constexpr int kMaxBatches = 64;      // batches per grouped launch (kernarg budget)
constexpr int kRbMaxBuckets = 2064;  // key buckets incl. the out-of-range bucket (>= 2049)
constexpr uint64_t kMaxGroupElems = 1ull << 32;  // a launch group holds fewer (32-bit stamp index and counts)

constexpr size_t kPieceBytes = 1 << 20;         // one pool task
constexpr size_t kCheckPieceBytes = 256 << 10;  // one pool task of a check without copy
constexpr size_t kWindowBytes = 8 << 20;  // one H2D / D2H DMA while the next window is copied

namespace {

static inline size_t round16(size_t x) { return (x + 15) & ~size_t(15); }

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline uint64_t next_pow2(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// ------------------------------------------------------ pieces and groups
// Append batch b to v as consecutive pieces of at most kMaxPiece elements
// (empty batches are dropped).  A batch applied piece by piece in order is the
// same Add (last-wins / sums follow index order) and the same Get, and every
// launch group then stays below 2^32 elements (the stamp index and the
// per-launch element counts are 32 bits).  vb: bytes per key of the value
// side (a row shard: width * value bytes).
constexpr uint64_t kMaxPiece = 1ull << 31;
static inline void push_pieces(std::vector<pskv_batch>& v, const pskv_batch& b, size_t vb) {
  for (uint64_t off = 0; off < b.n; off += kMaxPiece)
    v.push_back(pskv_batch{b.keys + off, static_cast<char*>(b.vals) + off * vb, std::min(kMaxPiece, b.n - off)});
}

using Span = std::pair<size_t, size_t>;  // [first, end) of a batch or piece list

// Split a batch list into launch groups: <= max_batches batches and fewer than
// max_elems elements each.  Every batch holds at most kMaxPiece elements
// (push_pieces), so every group takes at least one batch.
static inline std::vector<Span> split_groups(const std::vector<pskv_batch>& v, size_t max_batches = kMaxBatches,
                                             uint64_t max_elems = kMaxGroupElems) {
  std::vector<Span> out;
  size_t b = 0;
  while (b < v.size()) {
    size_t e = b;
    uint64_t el = 0;
    while (e < v.size() && e - b < max_batches && el + v[e].n < max_elems) {
      el += v[e].n;
      ++e;
    }
    out.emplace_back(b, e);
    b = e;
  }
  return out;
}

// Batches into K1 / DMA windows of a page-locked Get: each window takes
// batches until it holds at least min_key_bytes of keys, and is one launch
// group (split_groups' limits).  A window always takes its first batch.
static inline std::vector<Span> batch_windows(const std::vector<pskv_batch>& v, size_t min_key_bytes = kWindowBytes,
                                              size_t max_batches = kMaxBatches,
                                              uint64_t max_elems = kMaxGroupElems) {
  std::vector<Span> wins;
  for (size_t i = 0; i < v.size();) {
    size_t j = i, kb = 0;
    uint64_t el = 0;
    while (j < v.size() &&
           (j == i || (kb < min_key_bytes && j - i < max_batches && el + v[j].n < max_elems))) {
      kb += v[j].n * 4;
      el += v[j].n;
      ++j;
    }
    wins.emplace_back(i, j);
    i = j;
  }
  return wins;
}

// ------------------------------------------------------------ staging layout
// Where each batch's keys and values lie in a staging buffer: every range
// starts on a 16-byte boundary (16 B vector accesses, DMA alignment).
enum class StageOrder {
  kInterleaved,  // keys of batch 0, values of batch 0, keys of batch 1, ...
  kKeysFirst,    // every batch's keys, then every batch's values
};
struct StageSlot {
  size_t keys, vals;  // byte offsets from the staging's start
};
struct StageLayout {
  std::vector<StageSlot> at;  // per batch
  size_t key_bytes = 0;       // all key ranges (kKeysFirst: the values start here)
  size_t total = 0;
  // The batches as views into a staging buffer at `base`.
  std::vector<pskv_batch> views(const std::vector<pskv_batch>& v, char* base) const {
    std::vector<pskv_batch> out(v.size());
    for (size_t i = 0; i < v.size(); ++i)
      out[i] = pskv_batch{reinterpret_cast<const uint32_t*>(base + at[i].keys), base + at[i].vals, v[i].n};
    return out;
  }
};

// Staging bytes of the batches (either order); vb: value-side bytes per key.
static inline size_t staged_bytes(const std::vector<pskv_batch>& v, size_t vb) {
  size_t bytes = 0;
  for (const auto& b : v) bytes += round16(b.n * 4) + round16(b.n * vb);
  return bytes;
}

static inline StageLayout stage_layout(const std::vector<pskv_batch>& v, size_t vb, StageOrder order) {
  StageLayout l;
  l.at.resize(v.size());
  for (const auto& b : v) l.key_bytes += round16(b.n * 4);
  size_t ko = 0, vo = order == StageOrder::kKeysFirst ? l.key_bytes : 0;
  for (size_t i = 0; i < v.size(); ++i) {
    const size_t kb = round16(v[i].n * 4), vbytes = round16(v[i].n * vb);
    if (order == StageOrder::kInterleaved) {
      l.at[i] = StageSlot{ko, ko + kb};
      ko += kb + vbytes;
    } else {
      l.at[i] = StageSlot{ko, vo};
      ko += kb;
      vo += vbytes;
    }
  }
  l.total = order == StageOrder::kInterleaved ? ko : vo;
  return l;
}

// -------------------------------------------------- host copies and checks
// One contiguous piece of a host->pinned (or pinned->host) copy.
struct Piece {
  const char* src;
  char* dst;
  size_t bytes;
  int key_batch;  // >= 0: keys of that batch (checked while copied), -1: values
  // results of the key check
  bool sorted;
  bool dense;  // every key is its predecessor + 1
  uint32_t first, last;
  uint64_t outside;
};

// The key check, written so the compiler vectorises it (no loop-carried
// state but the or / sum reductions): 2-4x the rate of the sequential form.
static inline void check_keys(Piece& p, const uint32_t* k, size_t n, uint32_t key_begin, uint64_t range) {
  p.sorted = p.dense = true;
  p.first = p.last = 0;
  p.outside = 0;
  if (!n) return;
  const uint32_t rmax = range ? (uint32_t)(range - 1) : 0u;  // in range: (x - key_begin) <= rmax
  uint32_t unsorted = 0, gap = 0, out = (uint32_t)(k[0] - key_begin) > rmax;
  for (size_t i = 1; i < n; ++i) {
    const uint32_t a = k[i - 1], x = k[i];
    unsorted |= (uint32_t)(a > x);
    gap |= (uint32_t)(x != a + 1u);
    out += (uint32_t)((uint32_t)(x - key_begin) > rmax);
  }
  p.sorted = unsorted == 0;
  p.dense = gap == 0;
  p.first = k[0];
  p.last = k[n - 1];
  p.outside = range ? out : n;  // pieces hold < 2^32 keys
}

// The first key of these batches outside [key_begin, key_begin + range), or
// null: the vectorised count per batch, and the scan for the key itself only
// in a batch that holds one.
static inline const uint32_t* first_key_outside(const std::vector<pskv_batch>& v, uint32_t key_begin,
                                                uint64_t range) {
  for (const auto& b : v) {
    Piece p{};
    check_keys(p, b.keys, b.n, key_begin, range);
    if (!p.outside) continue;
    for (uint64_t i = 0; i < b.n; ++i)
      if ((uint64_t)(uint32_t)(b.keys[i] - key_begin) >= range) return b.keys + i;
  }
  return nullptr;
}

static inline void copy_piece(Piece& p, uint32_t key_begin, uint64_t range) {
  if (p.key_batch < 0) {
    std::memcpy(p.dst, p.src, p.bytes);
    return;
  }
  if (p.dst) std::memcpy(p.dst, p.src, p.bytes);  // else a page-locked caller buffer: check only
  check_keys(p, reinterpret_cast<const uint32_t*>(p.src), p.bytes / 4, key_begin, range);
}

// Cut [src, src+bytes) into pieces appended to `out`; check-only pieces
// (dst null) are smaller, so a pool spreads a medium batch's check wider.
static inline void add_pieces(std::vector<Piece>& out, const void* src, char* dst, size_t bytes, int key_batch) {
  const char* s = static_cast<const char*>(src);
  const size_t piece = dst ? kPieceBytes : kCheckPieceBytes;
  for (size_t off = 0; off < bytes; off += piece) {
    Piece p{};
    p.src = s + off;
    p.dst = dst ? dst + off : nullptr;
    p.bytes = std::min(piece, bytes - off);
    p.key_batch = key_batch;
    p.sorted = true;
    p.dense = true;
    out.push_back(p);
  }
}

// Combine the per-piece key checks: every piece sorted, and each piece's first
// key not below the previous piece's last key within the same batch.
static inline void combine_checks(const std::vector<Piece>& pieces, bool* all_sorted_in_range,
                                  bool* all_dense_in_range) {
  bool ok = true, dense = true;
  uint64_t outside = 0;
  int prev_batch = -1;
  uint32_t prev_last = 0;
  for (const auto& p : pieces) {
    if (p.key_batch < 0) continue;
    outside += p.outside;
    ok &= p.sorted;
    dense &= p.dense;
    if (p.key_batch == prev_batch) {
      ok &= prev_last <= p.first;
      dense &= p.first == prev_last + 1u;
    }
    prev_batch = p.key_batch;
    prev_last = p.last;
  }
  *all_sorted_in_range = ok && outside == 0;
  if (all_dense_in_range) *all_dense_in_range = dense && outside == 0;
}

// Pieces into copy windows: each window takes pieces until it holds at least
// `window` bytes (one DMA while the pool copies the next window).
static inline std::vector<Span> piece_windows(const std::vector<Piece>& pieces, size_t window = kWindowBytes) {
  std::vector<Span> wins;
  for (size_t i = 0; i < pieces.size();) {
    size_t j = i, win = 0;
    while (j < pieces.size() && (win < window || j == i)) win += pieces[j++].bytes;
    wins.emplace_back(i, j);
    i = j;
  }
  return wins;
}

// ------------------------------------------------------------ pooled pulls
// pskv_get_pooled (pskv.h "Pooled pulls"): bag b of a call is
// keys [offsets[b], offsets[b+1]).  Everything below is a function of its
// arguments and is shared, where marked PSKV_HD, by k_row_pooled and the CPU
// test of it (tests/cpp/pooled_plan_test.cpp).
#if defined(__HIP__)
#define PSKV_HD __host__ __device__
#else
#define PSKV_HD
#endif

constexpr uint64_t kPoolChunk = 256;      // keys per chunk of a long bag (a bag of more than kPoolChunk keys)
// Bags per virtual workgroup.  Few, so that a call of few, long bags still
// spreads over the CUs (1 Mi keys in bags of 64 are 512 workgroups); a row of
// at most 4 units leaves part of such a workgroup's 256 / L lane groups idle.
constexpr uint32_t kPoolBagsPerWg = 32;
constexpr uint64_t kPoolNone = ~0ull;

// The keys of a bag as the kernel takes them: device offsets cannot be checked
// by the library, so every bag is clamped to
// [min(o_b, n), min(max(o_b+1, o_b), n)): begin <= end <= n whatever the offsets hold.
struct PoolBag {
  uint64_t begin, end;
};
PSKV_HD static inline PoolBag pool_clamp(uint64_t o0, uint64_t o1, uint64_t n) {
  PoolBag b;
  b.begin = o0 < n ? o0 : n;
  const uint64_t e = o1 > o0 ? o1 : o0;
  b.end = e < n ? e : n;
  return b;
}

// The order of a bag's additions, a function of its length m alone:
//   m <= kPoolChunk  t_0, then + t_1, + t_2, ... in key order (t_i = w_i * row_i;
//                    the sum of no term is +0, the sum of one term is that term)
//   m >  kPoolChunk  chunk c = keys [c * kPoolChunk, min((c+1) * kPoolChunk, m)) of the
//                    bag is summed as above into a partial row s_c; the result is
//                    s_0, then + s_1, + s_2, ... in chunk order.
PSKV_HD static inline uint64_t pool_chunks(uint64_t m) { return m <= kPoolChunk ? 1 : (m + kPoolChunk - 1) / kPoolChunk; }

// Long bags' chunks are summed by a launch of their own whose work items are
// the WINDOWS of the call's key array: window q = key positions [q * kPoolChunk,
// (q+1) * kPoolChunk).  A chunk belongs to the window its first key lies in.
// A long bag covers more than a window's worth of positions, so it holds the
// first or the last position of every window one of its chunks starts in: at
// most two chunks start in a window, one of a bag that holds the window's
// first position (slot 0) and one of a bag that begins inside it (slot 1).
// pool_window_chunk: the chunk of the bag [b0, b1) that starts in window q, or
// kPoolNone (none does, or the bag is not long).
PSKV_HD static inline uint64_t pool_window_chunk(uint64_t b0, uint64_t b1, uint64_t q) {
  if (b1 < b0 || b1 - b0 <= kPoolChunk) return kPoolNone;
  const uint64_t lo = q * kPoolChunk;
  const uint64_t c = b0 >= lo ? 0 : (lo - b0 + kPoolChunk - 1) / kPoolChunk;
  const uint64_t p = b0 + c * kPoolChunk;
  return (p >= lo && p - lo < kPoolChunk && p < b1) ? c : kPoolNone;
}
// The partial row of chunk c of the bag that begins at b0: two slots per window.
PSKV_HD static inline uint64_t pool_slot(uint64_t b0, uint64_t c) {
  const uint64_t q = (b0 + c * kPoolChunk) / kPoolChunk;
  return 2 * q + (b0 > q * kPoolChunk ? 1u : 0u);
}
// Partial rows a call of n keys needs at most (every slot index is below it).
PSKV_HD static inline uint64_t pool_slots(uint64_t n) { return 2 * ((n + kPoolChunk - 1) / kPoolChunk); }

// The last index i of off[0 .. cnt) with off[i] <= x (0 when there is none):
// the bag that holds key position x when the offsets are well formed.
PSKV_HD static inline uint64_t pool_bag_of(const uint64_t* off, uint64_t cnt, uint64_t x) {
  uint64_t lo = 0, hi = cnt;
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// Pooled pushes (pskv_apply_pooled) work position-major: the
// kernels need the bag of a key position, not the positions of a bag.  A
// virtual workgroup of consecutive positions [first, last] finds the bags of
// its two ends once (pool_bag_span); every position in between then searches
// only off[lo .. hi] by pool_bag_of's rule (pool_bags_in), and not at all when
// one bag covers the workgroup (lo == hi).  With well-formed offsets the result
// is pool_bag_of's, the true bag, empty bags skipped (pool_bag_of does not
// decrease in x, so lo <= pool_bag_of(x) <= hi); with any offsets it lies in
// [lo, hi], so below nbags (nbags >= 1).
struct PoolSpan {
  uint64_t lo, hi;  // lo <= hi < nbags
};
PSKV_HD static inline PoolSpan pool_bag_span(const uint64_t* off, uint64_t nbags, uint64_t first, uint64_t last) {
  PoolSpan sp;
  sp.lo = pool_bag_of(off, nbags, first);
  sp.hi = pool_bag_of(off, nbags, last);
  if (sp.hi < sp.lo) sp.hi = sp.lo;  // (malformed offsets only)
  return sp;
}
// bag[r] = the last index i of [sp.lo, sp.hi] with off[i] <= x[r] (sp.lo when
// there is none), for every r with want[r]; the others get sp.lo unsearched.
// The R searches are independent and advance in step, so their loads are
// issued together and a round costs one memory latency, not R.
template <int R>
PSKV_HD static inline void pool_bags_in(const uint64_t* off, const PoolSpan& sp, const uint64_t (&x)[R],
                                        const bool (&want)[R], uint64_t (&bag)[R]) {
  uint64_t hi[R];
  bool more = false;
  for (int r = 0; r < R; ++r) {
    bag[r] = sp.lo;
    hi[r] = want[r] ? sp.hi + 1 : sp.lo + 1;
    more |= hi[r] - bag[r] > 1;
  }
  while (more) {
    more = false;
    for (int r = 0; r < R; ++r) {
      if (hi[r] - bag[r] <= 1) continue;
      const uint64_t mid = bag[r] + ((hi[r] - bag[r]) >> 1);
      if (off[mid] <= x[r])
        bag[r] = mid;
      else
        hi[r] = mid;
      more |= hi[r] - bag[r] > 1;
    }
  }
}

// A host call's offsets: nbags + 1 values, offsets[0] == 0, non-decreasing,
// offsets[nbags] == n.  Null when they hold (nbags == 0: nothing to check),
// else what is wrong, with the first bad bag in *bad.
static inline const char* pool_offsets_error(const uint64_t* off, uint64_t nbags, uint64_t n, uint64_t* bad) {
  if (nbags == 0) return nullptr;
  *bad = 0;
  if (off[0] != 0) return "offsets[0] must be 0";
  for (uint64_t b = 0; b < nbags; ++b) {
    *bad = b;
    if (off[b + 1] < off[b]) return "offsets must not decrease";
    if (off[b + 1] > n) return "the bag ends past the n keys";
  }
  *bad = nbags - 1;
  if (off[nbags] != n) return "offsets[nbags] must equal n";
  return nullptr;
}

}  // namespace

// ---------------------------------------------------- grouped pooled pushes
// pskv_apply_pooled_grouped (pskv.h "Grouped pooled pushes"): the pooled
// pushes of several workers as ONE step.  The live batches (n > 0 and nbags >
// 0) of a call are cut into launch groups of at most kMaxPoolBatches batches
// and fewer than kMaxGroupElems keys; a launch group's descriptors travel by
// value in the kernel arguments, cut into virtual workgroups of `chunk`
// positions as a GroupArgs of the same batches is, so that K4a, given that
// GroupArgs (keys and n only), stamps the tags the pooled kernels compare.
constexpr int kMaxPoolBatches = 32;  // batches per launch group of a grouped pooled push (kernarg budget)

struct PoolBatchDesc {
  const uint32_t* keys;     // n
  const void* weights;      // n values, or null: this batch's terms are its bag rows themselves
  const uint64_t* offsets;  // nbags + 1 (the kernels read [0, nbags))
  const void* bag_grads;    // nbags rows
  uint64_t n, nbags;        // both > 0
};
struct PoolGroupArgs {
  int nb;
  uint32_t wg_prefix[kMaxPoolBatches + 1];  // first virtual workgroup of each batch
  PoolBatchDesc b[kMaxPoolBatches];
};
static_assert(sizeof(PoolBatchDesc) == 48, "six 8-byte words per batch");
// beside it in the 4 KiB kernarg segment: DenseView (32), five pointers, the
// epoch, RowShape (16), OptArgs<double> (88) and the hidden arguments (~300)
static_assert(sizeof(PoolGroupArgs) <= 1800, "a pooled group plus the other arguments fit the 4 KiB kernarg segment");

namespace {

// The live batches of a call, in call order (a batch without a key or without
// a bag contributes nothing), and each one's index in the call.
static inline std::vector<pskv_pool_batch> pool_live_batches(const pskv_pool_batch* b, uint64_t nb,
                                                             std::vector<uint64_t>* index = nullptr) {
  std::vector<pskv_pool_batch> out;
  for (uint64_t i = 0; i < nb; ++i) {
    if (b[i].n == 0 || b[i].nbags == 0) continue;
    out.push_back(b[i]);
    if (index) index->push_back(i);
  }
  return out;
}

// The batches as the mark takes them: keys and n (the bag rows stand in for
// the values, which the mark does not read).
static inline std::vector<pskv_batch> pool_mark_batches(const std::vector<pskv_pool_batch>& v) {
  std::vector<pskv_batch> out;
  for (const auto& b : v) out.push_back(pskv_batch{b.keys, const_cast<void*>(b.bag_grads), b.n});
  return out;
}

// Launch groups of live batches (each of at most kMaxPiece keys): split_groups
// with the pooled limit.
static inline std::vector<Span> pool_split_groups(const std::vector<pskv_pool_batch>& v,
                                                  size_t max_batches = kMaxPoolBatches,
                                                  uint64_t max_elems = kMaxGroupElems) {
  return split_groups(pool_mark_batches(v), max_batches, max_elems);
}

// The descriptor of batches [b, e) of a list (e - b <= kMaxPoolBatches), cut
// into virtual workgroups of `chunk` positions; *nwg: their number.
static inline PoolGroupArgs make_pool_group(const std::vector<pskv_pool_batch>& v, size_t b, size_t e, uint64_t chunk,
                                            uint32_t* nwg, uint64_t* elems) {
  PoolGroupArgs g;
  std::memset(&g, 0, sizeof(g));
  g.nb = (int)(e - b);
  uint64_t wg = 0, el = 0;
  for (size_t i = b; i < e; ++i) {
    const size_t j = i - b;
    g.wg_prefix[j] = (uint32_t)wg;
    g.b[j] = PoolBatchDesc{v[i].keys, v[i].weights, v[i].offsets, v[i].bag_grads, v[i].n, v[i].nbags};
    wg += (v[i].n + chunk - 1) / chunk;
    el += v[i].n;
  }
  g.wg_prefix[e - b] = (uint32_t)wg;
  *nwg = (uint32_t)wg;
  *elems = el;
  return g;
}

// The batch of virtual workgroup wg: the last batch whose first workgroup is
// at or before it (live batches hold at least one workgroup each, so the
// prefix increases strictly).
PSKV_HD static inline int pool_group_batch_of(const PoolGroupArgs& ga, uint32_t wg) {
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
// Group-wide index of batch j's first position: K4a's elem_prefix over the
// same batches.  A position's tag is epoch << 32 | (this + the position).
PSKV_HD static inline uint64_t pool_group_elem_prefix(const PoolGroupArgs& ga, int j) {
  uint64_t e = 0;
  for (int i = 0; i < j; ++i) e += ga.b[i].n;
  return e;
}

// A host call's staging: every live batch's keys, weights (where it has
// them), offsets and bag rows, each range on a 16-byte boundary, batch after
// batch.  vb: bytes per value; rb: bytes per row.
struct PoolStageSlot {
  size_t keys, weights, offsets, rows;  // byte offsets from the staging's start (weights: unused without weights)
};
struct PoolStageLayout {
  std::vector<PoolStageSlot> at;  // per live batch
  size_t total = 0;
};
static inline PoolStageLayout pool_stage_layout(const std::vector<pskv_pool_batch>& v, size_t vb, size_t rb) {
  PoolStageLayout l;
  l.at.resize(v.size());
  size_t o = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    PoolStageSlot& s = l.at[i];
    s.keys = o;
    o += round16(v[i].n * 4);
    s.weights = o;
    if (v[i].weights) o += round16(v[i].n * vb);
    s.offsets = o;
    o += round16((v[i].nbags + 1) * sizeof(uint64_t));
    s.rows = o;
    o += round16(v[i].nbags * rb);
  }
  l.total = o;
  return l;
}

// ------------------------------------- optimizer state slots, sparse shards
// State slots per kind (pskv_optimizer_kind), and whether a slot starts at
// init_accum (Adagrad's h, FTRL's n) or, as every other slot, at zero.
static inline int opt_slots(int kind) {
  return (kind == PSKV_OPT_ADAM || kind == PSKV_OPT_FTRL) ? 2
         : (kind == PSKV_OPT_ADAGRAD || kind == PSKV_OPT_MOMENTUM) ? 1 : 0;
}
static inline bool opt_slot_is_accum(int kind, int slot) {
  return (kind == PSKV_OPT_ADAGRAD && slot == 0) || (kind == PSKV_OPT_FTRL && slot == 1);
}

// A sparse shard's limits (pskv.h "Sparse shards"): slot + 1
// fits an index entry's 31 bits and 0xFFFFFFFF stays free as the id the row
// kernels drop; the index has at least two entries per slot.
constexpr uint64_t kSparseMaxCapacity = (1ull << 31) - 2;
static inline uint64_t sparse_table_slots(uint64_t capacity) { return std::max<uint64_t>(16, next_pow2(2 * capacity)); }

// The capacity behind a writing call of n key positions at `capacity` slots
// holding `count` keys, growth limit `max` (0: off): grown iff count + n >
// capacity, to min(max, max(2 * capacity, count + n)).
static inline uint64_t sparse_grown_capacity(uint64_t capacity, uint64_t count, uint64_t n, uint64_t max) {
  if (capacity >= max || count + n <= capacity) return capacity;
  return std::min(max, std::max(2 * capacity, count + n));
}
// Must the count be read to decide?  Not while this is false for a bound >= count.
static inline bool sparse_may_grow(uint64_t bound, uint64_t n, uint64_t capacity, uint64_t max) {
  return capacity < max && bound + n > capacity;
}

// What is wrong with `capacity` as the capacity or growth limit of a sparse
// shard of `current` slots and rows of row_bytes, or null.
static inline const char* sparse_capacity_error(uint64_t current, uint64_t capacity, uint64_t row_bytes) {
  if (capacity < current) return "capacity is below the shard's current capacity (a sparse shard does not shrink)";
  if ((capacity + 1) * row_bytes > (1ull << 46)) return "(capacity + 1) * width * value bytes exceeds 2^46 bytes";
  return nullptr;
}

}  // namespace

// ------------------------------------------------------------ K5 bucket rule
// K5 key buckets: windows of 2^wbits keys of the owned range, window w in
// bucket w % nbd (1 <= nbd < 2^12, windows < 2^21: wbits >= 11 or a range
// below 2^32); magic = ceil(2^32 / nbd); span = keys per bucket at most
// (ceil(windows / nbd) << wbits), the extent of a bucket's local index.
struct RbMap {
  uint32_t wbits;
  uint32_t nbd;
  uint32_t magic;
  uint32_t span;
  int32_t nlog;  // log2(nbd) when nbd is a power of two (then magic is unused), else -1
};
namespace {

struct RbPlan {
  RbMap bm;
  int apply_log2;  // log2 of the resolve workgroup's LDS table slots
};

// The buckets of one K5 launch of `elems` keys into a shard of `range` keys.
// bucket = key offset >> bshift (more buckets: longer loff rows, shorter
// runs).  Per mode: assign takes one bucket per 2 Ki pushed keys, at most
// 2^11 bucket bits; accumulate, whose resolve also reads the parameters, one
// per 4 Ki, at most 2^10.  The sweep behind the rule (tools/zipf_probe.py,
// 4/8/16 x 1M Zipf keys) and its timings: DESIGN.md §7 "K5 bucket count",
// logs in profiles/r01_probes/probe_tb*.log and probe_new_*.log.
// The resolve workgroup uses a 2^13-slot LDS table while buckets average
// <= 2 Ki pushed keys, else 2^14.
// tb, wbits, nbd: options RB_TB, RB_WBITS, RB_NBD (0 = by the rule).
static inline RbPlan rb_plan(uint64_t range, uint64_t elems, int mode, uint32_t tb_opt, uint32_t wbits_opt,
                             uint32_t nbd_opt) {
  uint32_t bits = 0;
  while (bits < 32 && ((range - 1) >> bits) != 0) ++bits;
  const uint32_t per = mode == PSKV_ASSIGN ? 11 : 12, tmax = mode == PSKV_ASSIGN ? 11 : 10;
  uint32_t tb = 6;
  while (tb < tmax && (elems >> (per + tb)) != 0) ++tb;
  if (tb_opt) tb = tb_opt;
  const uint32_t bshift = bits > tb ? bits - tb : 0;
  uint32_t nbd = (uint32_t)(((range - 1) >> bshift) + 1);
  if (nbd_opt) nbd = nbd_opt;
  // The buckets own windows of 2^wbits keys dealt round-robin (window w ->
  // bucket w % nbd); wbits = bshift is one contiguous window per bucket.
  RbPlan p;
  RbMap& bm = p.bm;
  bm.wbits = std::min<uint32_t>(bshift, wbits_opt ? wbits_opt : 11u);
  bm.nbd = nbd;
  bm.nlog = -1;
  for (int l = 0; l < 12; ++l)
    if (nbd == (1u << l)) bm.nlog = l;
  bm.magic = nbd > 1 ? (uint32_t)(((1ull << 32) + nbd - 1) / nbd) : 0u;  // nbd = 1 takes the shift path
  const uint64_t nwin = ((range - 1) >> bm.wbits) + 1;  // < 2^21: wbits = 11, or wbits = bshift and nwin = nbd
  bm.span = (uint32_t)std::min<uint64_t>(((nwin + nbd - 1) / nbd) << bm.wbits, 0xFFFFFFFFull);
  p.apply_log2 = elems / nbd <= 2048 ? 13 : 14;
  return p;
}

}  // namespace
}  // namespace pskv
