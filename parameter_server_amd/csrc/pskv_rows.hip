// pskv_rows.hip — CDNA4 (gfx950) kernels of row-valued shards: a fixed-width
// vector of W values per key (DESIGN.md "Row-valued shards").
//
//   k_row_gather      Get: out[i] = row(keys[i]), zeros for a key outside the range
//   k_row_commit      assign Add: the stamped winner of each key copies its whole row
//   k_row_accumulate  accumulate Add: one no-return atomic add per element
//   k_row_step_losers optimizer step: gradient rows of non-winners summed into gsum
//   k_row_step_apply  optimizer step: each key's winner applies SGD / Adagrad / momentum / Adam / FTRL once
//                     (both over GroupArgs: rows given; PoolPushArgs, PoolGroupArgs: a pooled push's
//                     or a group of pooled pushes' rows weight * bag_grads[bag], formed in registers)
//   k_row_pooled      pooled pull: out[b] = sum over bag b's keys of weight * row(key)
//   k_row_pooled_chunks  pooled pull: the chunks of bags longer than kPoolChunk, into partial rows
//
// Lane mapping (all of them).  A row is U units long (RowShape); a group of
// L = min(64, next_pow2(U)) consecutive lanes owns one row at a time, lane l
// of the group taking units l, l + L, ...  A wave therefore covers 64 / L
// rows per instruction, each as one contiguous segment, and every lane of a
// group reads the same key (one broadcast load).  The copy kernels take
// 16-byte units when the row size and the pointers allow, else one element;
// the accumulate always takes one element per lane, so that an atomic
// wave-instruction covers contiguous bytes of each row (a lane holding four
// consecutive elements would spread each instruction over 64 rows' worth of
// 16-byte strides).  kRowsInFlight rows per group are loaded before the first
// is stored.
//
// Work split: as K4 (pskv_kernels.hip): virtual workgroups of kGeneralChunk
// keys of one batch (GroupArgs / build_group), grid-stride.  Within a chunk,
// group g of the workgroup's G = kBlock / L groups takes the chunk's elements
// g, g + G, ...; `li` below is the element's index inside the chunk, the same
// number K4a folds into its stamps.
#include <type_traits>

#include "pskv_internal.h"

namespace pskv {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowsInFlight = 4;
static_assert(kGeneralChunk % (kRowsInFlight * kBlock) == 0, "every group's row index stays inside the chunk");

// (the same search as pskv_kernels.hip's: the last batch whose first virtual
// workgroup is at or before `wg`)
__device__ __forceinline__ int row_batch_of(const GroupArgs& ga, uint32_t wg) {
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

// Group-wide index of batch j's first element: must equal K4a's elem_prefix,
// or no element's tag would match its stamp.
__device__ __forceinline__ uint64_t row_elem_prefix(const GroupArgs& ga, int j) {
  uint64_t e = 0;
  for (int i = 0; i < j; ++i) e += ga.b[i].n;
  return e;
}

// The tag K4a stamped for an element: epoch<<32 | (group-wide index of the element).
__device__ __forceinline__ unsigned long long row_tag(uint32_t epoch, uint64_t index) {
  return ((unsigned long long)epoch << 32) | index;
}

template <typename UT>
__device__ __forceinline__ UT zero_unit() {
  return UT(0);
}
template <>
__device__ __forceinline__ u32x4 zero_unit<u32x4>() {
  return u32x4{0u, 0u, 0u, 0u};
}

template <bool NT, typename UT>
__device__ __forceinline__ void store_unit(UT* p, UT v) {
  if (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// The rows one lane group handles in one step: kRowsInFlight elements of the
// chunk, G apart.  live: the element exists; in: its key is owned.
struct RowStep {
  uint64_t i[kRowsInFlight];    // element index in the batch
  uint32_t off[kRowsInFlight];  // key - key_begin
  bool live[kRowsInFlight];
  bool in[kRowsInFlight];
};

__device__ __forceinline__ void load_step(RowStep& s, const uint32_t* __restrict__ keys, uint64_t n,
                                          uint64_t base, uint32_t r0, uint32_t G, const DenseView& d) {
#pragma unroll
  for (int r = 0; r < kRowsInFlight; ++r) {
    s.i[r] = base + r0 + (uint32_t)r * G;
    s.live[r] = s.i[r] < n;
    const uint32_t k = s.live[r] ? keys[s.i[r]] : 0u;
    s.off[r] = k - d.key_begin;
    s.in[r] = s.live[r] && (uint64_t)s.off[r] < d.range;
  }
}

template <typename UT, bool NT>
__global__ __launch_bounds__(kBlock) void k_row_gather(GroupArgs ga, DenseView d, RowShape rs) {
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  const uint32_t U = rs.units;
  const UT* __restrict__ param = reinterpret_cast<const UT*>(d.param);
  const uint32_t nvwg = ga.wg_prefix[ga.nb];
  for (uint32_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const int j = row_batch_of(ga, wg);
    const uint32_t* __restrict__ keys = ga.b[j].keys;
    UT* __restrict__ out = reinterpret_cast<UT*>(const_cast<void*>(ga.b[j].vals));
    const uint64_t n = ga.b[j].n;
    const uint64_t base = (uint64_t)(wg - ga.wg_prefix[j]) * kGeneralChunk;
    for (uint32_t r0 = grp; r0 < (uint32_t)kGeneralChunk; r0 += kRowsInFlight * G) {
      if (base + r0 >= n) break;  // (r0 grows: the later rows of the step are past the end too)
      RowStep s;
      load_step(s, keys, n, base, r0, G, d);
      for (uint32_t u = lane; u < U; u += rs.lanes) {
        UT v[kRowsInFlight];
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          v[r] = s.in[r] ? param[(uint64_t)s.off[r] * U + u] : zero_unit<UT>();
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          if (s.live[r]) store_unit<NT>(out + s.i[r] * U + u, v[r]);
      }
    }
  }
}

// `err`: the shard's sticky error word (OvfCtl::stat[1]).  A row whose key
// lies outside the owned range is dropped, and one lane of its group sets
// kErrRowOutOfRange there (pskv_sync reports it).
template <typename UT>
__global__ __launch_bounds__(kBlock) void k_row_commit(GroupArgs ga, DenseView d,
                                                       const unsigned long long* __restrict__ owner,
                                                       uint32_t* err, uint32_t epoch, RowShape rs) {
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  const uint32_t U = rs.units;
  UT* __restrict__ param = reinterpret_cast<UT*>(d.param);
  const uint32_t nvwg = ga.wg_prefix[ga.nb];
  for (uint32_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const int j = row_batch_of(ga, wg);
    const uint32_t* __restrict__ keys = ga.b[j].keys;
    const UT* __restrict__ vals = reinterpret_cast<const UT*>(ga.b[j].vals);
    const uint64_t n = ga.b[j].n;
    const uint64_t base = (uint64_t)(wg - ga.wg_prefix[j]) * kGeneralChunk;
    const uint64_t gbase = row_elem_prefix(ga, j) + base;
    for (uint32_t r0 = grp; r0 < (uint32_t)kGeneralChunk; r0 += kRowsInFlight * G) {
      if (base + r0 >= n) break;
      RowStep s;
      load_step(s, keys, n, base, r0, G, d);
      bool win[kRowsInFlight];
#pragma unroll
      for (int r = 0; r < kRowsInFlight; ++r) {
        const unsigned long long tag = row_tag(epoch, gbase + r0 + (uint32_t)r * G);
        win[r] = s.in[r] && owner[s.off[r]] == tag;
        if (s.live[r] && !s.in[r] && lane == 0) atomicOr(err, kErrRowOutOfRange);
      }
      for (uint32_t u = lane; u < U; u += rs.lanes) {
        UT v[kRowsInFlight];
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          v[r] = win[r] ? vals[s.i[r] * U + u] : zero_unit<UT>();
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          if (win[r]) param[(uint64_t)s.off[r] * U + u] = v[r];
      }
    }
  }
}

// One element per lane (rs.units = the width).  The adds are no-return device
// atomics: any order, so float sums meet the recursive-summation bound.
template <typename AT>
__global__ __launch_bounds__(kBlock) void k_row_accumulate(GroupArgs ga, DenseView d, uint32_t* err,
                                                           RowShape rs) {
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  const uint32_t U = rs.units;
  AT* __restrict__ param = reinterpret_cast<AT*>(d.param);
  const uint32_t nvwg = ga.wg_prefix[ga.nb];
  for (uint32_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const int j = row_batch_of(ga, wg);
    const uint32_t* __restrict__ keys = ga.b[j].keys;
    const AT* __restrict__ vals = reinterpret_cast<const AT*>(ga.b[j].vals);
    const uint64_t n = ga.b[j].n;
    const uint64_t base = (uint64_t)(wg - ga.wg_prefix[j]) * kGeneralChunk;
    for (uint32_t r0 = grp; r0 < (uint32_t)kGeneralChunk; r0 += kRowsInFlight * G) {
      if (base + r0 >= n) break;
      RowStep s;
      load_step(s, keys, n, base, r0, G, d);
#pragma unroll
      for (int r = 0; r < kRowsInFlight; ++r)
        if (s.live[r] && !s.in[r] && lane == 0) atomicOr(err, kErrRowOutOfRange);
      for (uint32_t u = lane; u < U; u += rs.lanes) {
        AT v[kRowsInFlight];
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r) v[r] = s.in[r] ? vals[s.i[r] * U + u] : AT(0);
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          if (s.in[r]) (void)atomicAdd(param + (uint64_t)s.off[r] * U + u, v[r]);
      }
    }
  }
}

// ------------------------------------------------------- optimizer steps
// One call is one step: behind K4a's stamps, k_row_step_losers
// sums the gradient row of every position that is not its key's winner into
// `gsum` (zero between calls), then k_row_step_apply lets each winner apply the
// rule once to its key's row and put the gsum row back to zero.  Both are
// written once over the argument block, which says where a virtual workgroup's
// batch and a position's gradient row come from:
//   GroupArgs      pskv_apply[_grouped]: a launch group of batches; position
//                  i's row is vals[i].
//   PoolPushArgs   pskv_apply_pooled: one batch, so a position
//                  is its own stamp index; its row is formed here, weights[i] *
//                  bag_grads[bag(i)] (the bag of a position: pskv_plan.h).
//   PoolGroupArgs  pskv_apply_pooled_grouped: a launch group of
//                  pooled batches.  A virtual workgroup of kGeneralChunk
//                  positions belongs to ONE batch (the wg_prefix search); its
//                  bags are looked up in that batch's offsets, its span ends
//                  at that batch's last position, and its tags carry the keys
//                  of the batches before it: the index K4a stamped when given
//                  the same batches as a GroupArgs.
// WEIGHTED (pooled blocks): the batch has weights; for a group, some batch of
// it has, and one without them (uniform over the workgroup) adds its bag rows
// unmultiplied.

// A unit of V consecutive elements: V = 1, or 16 bytes' worth.
template <typename T, int V>
struct OptUnit {
  T e[V];
};

template <typename T, int V>
__device__ __forceinline__ OptUnit<T, V> load_opt_unit(const T* p, uint64_t unit) {
  OptUnit<T, V> r;
  if constexpr (V == 1) {
    r.e[0] = p[unit];
  } else {
    typedef T vt __attribute__((ext_vector_type(V)));
    const vt v = *reinterpret_cast<const vt*>(p + unit * V);
#pragma unroll
    for (int i = 0; i < V; ++i) r.e[i] = v[i];
  }
  return r;
}

template <typename T, int V>
__device__ __forceinline__ void store_opt_unit(T* p, uint64_t unit, const OptUnit<T, V>& r) {
  if constexpr (V == 1) {
    p[unit] = r.e[0];
  } else {
    typedef T vt __attribute__((ext_vector_type(V)));
    vt v;
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = r.e[i];
    *reinterpret_cast<vt*>(p + unit * V) = v;
  }
}

__device__ __forceinline__ bool nonzero_bits(float x) { return __float_as_uint(x) != 0u; }
__device__ __forceinline__ bool nonzero_bits(double x) { return __double_as_longlong(x) != 0ll; }

// One multiplication rounded to T: the empty statement keeps the product out
// of a contraction with the addition that follows, so a weighted term is the
// same value in gsum, in a winner's step and in a host-expanded pskv_apply.
__device__ __forceinline__ float rounded_mul(float w, float x) {
  float r = w * x;
  asm("" : "+v"(r));
  return r;
}
__device__ __forceinline__ double rounded_mul(double w, double x) {
  double r = w * x;
  asm("" : "+v"(r));
  return r;
}

// A wave-uniform value held in vector registers from here on (PIN), or left
// to the compiler.
template <bool PIN, typename X>
__device__ __forceinline__ X in_vgprs(X x) {
  if constexpr (PIN) asm("" : "+v"(x));
  return x;
}

// The argument blocks: virtual workgroups, the batch of one (its index j, the
// batch, its first workgroup, the group-wide index of its first position: must
// equal K4a's elem_prefix) and where the batch's gradient rows lie.
template <typename Args>
constexpr bool kStepPooled = !std::is_same<Args, GroupArgs>::value;
template <typename Args>
constexpr bool kStepPoolGroup = std::is_same<Args, PoolGroupArgs>::value;

template <typename GA>
__device__ __forceinline__ uint32_t step_nvwg(const GA& ga) { return ga.wg_prefix[ga.nb]; }
__device__ __forceinline__ uint32_t step_nvwg(const PoolPushArgs& a) {
  return (uint32_t)((a.n + kGeneralChunk - 1) / kGeneralChunk);
}
__device__ __forceinline__ int step_batch_of(const GroupArgs& ga, uint32_t wg) { return row_batch_of(ga, wg); }
__device__ __forceinline__ int step_batch_of(const PoolGroupArgs& ga, uint32_t wg) {
  return pool_group_batch_of(ga, wg);
}
__device__ __forceinline__ int step_batch_of(const PoolPushArgs&, uint32_t) { return 0; }
__device__ __forceinline__ DevBatch step_batch(const GroupArgs& ga, int j) { return ga.b[j]; }
__device__ __forceinline__ const PoolBatchDesc& step_batch(const PoolGroupArgs& ga, int j) { return ga.b[j]; }
__device__ __forceinline__ const PoolPushArgs& step_batch(const PoolPushArgs& a, int) { return a; }
template <typename GA>
__device__ __forceinline__ uint32_t step_first_wg(const GA& ga, int j) { return ga.wg_prefix[j]; }
__device__ __forceinline__ uint32_t step_first_wg(const PoolPushArgs&, int) { return 0; }
__device__ __forceinline__ uint64_t step_elem_prefix(const GroupArgs& ga, int j) { return row_elem_prefix(ga, j); }
__device__ __forceinline__ uint64_t step_elem_prefix(const PoolGroupArgs& ga, int j) {
  return pool_group_elem_prefix(ga, j);
}
__device__ __forceinline__ uint64_t step_elem_prefix(const PoolPushArgs&, int) { return 0; }
template <typename B>
__device__ __forceinline__ const void* step_rows(const B& b) { return b.bag_grads; }
__device__ __forceinline__ const void* step_rows(const DevBatch& b) { return b.vals; }

// The span of the bags of the workgroup at position `base` of pooled batch
// `a` (LOOKUP; else none yet), held in vector registers (PIN) or not.
template <bool LOOKUP, bool PIN, typename B>
__device__ __forceinline__ PoolSpan step_span(const B& a, uint64_t base) {
  PoolSpan sp{0, 0};
  if constexpr (LOOKUP) {
    const uint64_t end = base + kGeneralChunk < a.n ? base + kGeneralChunk : a.n;  // base < n of THIS batch
    sp = pool_bag_span(a.offsets, a.nbags, base, end - 1);
    sp.lo = in_vgprs<PIN>(sp.lo);
    sp.hi = in_vgprs<PIN>(sp.hi);
  }
  return sp;
}

// The bags of a step's wanted rows in pooled batch `a`; the workgroup's span
// is looked up at the first step that wants one (`have`), so a lane group of
// winners only (k_row_step_losers, distinct keys) reads no offset.
template <typename B>
__device__ __forceinline__ void step_bags(const B& a, const uint64_t* offsets, uint64_t base, PoolSpan& sp, bool& have,
                                          const RowStep& s, const bool (&want)[kRowsInFlight],
                                          uint64_t (&bag)[kRowsInFlight]) {
  if (!have) {
    sp = step_span<true, false>(a, base);
    have = true;
  }
  pool_bags_in<kRowsInFlight>(offsets, sp, s.i, want, bag);
}

// One element per lane, as k_row_accumulate.  `tag` of a position as in
// k_row_commit; an in-range position whose tag is not its key's stamp is a loser.
template <typename AT, typename Args, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_row_step_losers(Args ga, DenseView d, AT* __restrict__ gsum,
                                                            const unsigned long long* __restrict__ owner,
                                                            uint32_t* err, uint32_t epoch, RowShape rs) {
  static_assert(kStepPooled<Args> || !WEIGHTED, "only bag rows are weighted");
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  const uint32_t U = rs.units;
  const uint32_t nvwg = step_nvwg(ga);
  for (uint32_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const int j = step_batch_of(ga, wg);
    decltype(auto) a = step_batch(ga, j);  // (by value or by reference: k_row_step_apply)
    const AT* __restrict__ weights = nullptr;
    if constexpr (kStepPooled<Args>) weights = reinterpret_cast<const AT*>(a.weights);
    const AT* __restrict__ rows = reinterpret_cast<const AT*>(step_rows(a));
    const bool mul = WEIGHTED && (!kStepPoolGroup<Args> || weights != nullptr);
    const uint64_t base = (uint64_t)(wg - step_first_wg(ga, j)) * kGeneralChunk;
    const uint64_t gbase = step_elem_prefix(ga, j) + base;
    PoolSpan sp{0, 0};
    bool have = false;
    for (uint32_t r0 = grp; r0 < (uint32_t)kGeneralChunk; r0 += kRowsInFlight * G) {
      if (base + r0 >= a.n) break;
      RowStep s;
      load_step(s, a.keys, a.n, base, r0, G, d);
      bool lose[kRowsInFlight];
      bool any = false;
#pragma unroll
      for (int r = 0; r < kRowsInFlight; ++r) {
        const unsigned long long tag = row_tag(epoch, gbase + r0 + (uint32_t)r * G);
        lose[r] = s.in[r] && owner[s.off[r]] != tag;
        any |= lose[r];
        if (s.live[r] && !s.in[r] && lane == 0) atomicOr(err, kErrRowOutOfRange);
      }
      if (!any) continue;  // distinct keys: only keys and stamps were read
      // a position's gradient row: its own of `rows`, or its bag's times w[r] where mul
      uint64_t bag[kRowsInFlight];
      AT w[kRowsInFlight];
      if constexpr (kStepPooled<Args>) {
        step_bags(a, a.offsets, base, sp, have, s, lose, bag);
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r) w[r] = (mul && lose[r]) ? weights[s.i[r]] : AT(1);
      }
      for (uint32_t u = lane; u < U; u += rs.lanes) {
        AT v[kRowsInFlight];
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          v[r] = lose[r] ? rows[(kStepPooled<Args> ? bag[r] : s.i[r]) * U + u] : AT(0);
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          if (lose[r]) (void)atomicAdd(gsum + (uint64_t)s.off[r] * U + u, mul ? rounded_mul(w[r], v[r]) : v[r]);
      }
    }
  }
}

// The rule on one unit: g the winner's own gradient unit, gs the key's gsum
// unit (set to zero), p and the state units h (slot 0), h2 (slot 1) stepped in
// place.  Returns whether gs held a non-zero bit (then its zeros are to be
// written back).
template <typename T, int KIND, int V>
__device__ __forceinline__ bool opt_step_unit(const OptUnit<T, V>& g, OptUnit<T, V>& gs, OptUnit<T, V>& p,
                                              OptUnit<T, V>& h, OptUnit<T, V>& h2, const OptArgs<T>& o) {
  bool dirty = false;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    dirty |= nonzero_bits(gs.e[i]);
    const T dd = (g.e[i] + gs.e[i]) + o.wd * p.e[i];
    if (KIND == 2) {
      h.e[i] = h.e[i] + dd * dd;
      p.e[i] = p.e[i] - o.lr * (dd / (sqrt(h.e[i]) + o.eps));
    } else if (KIND == 3) {
      h.e[i] = o.mu * h.e[i] + dd;
      const T step = o.nesterov ? dd + o.mu * h.e[i] : h.e[i];
      p.e[i] = p.e[i] - o.lr * step;
    } else if (KIND == 4) {
      h.e[i] = o.beta1 * h.e[i] + o.omb1 * dd;
      h2.e[i] = o.beta2 * h2.e[i] + o.omb2 * (dd * dd);
      p.e[i] = p.e[i] - o.a * (h.e[i] / (sqrt(h2.e[i]) * o.b + o.eps));
    } else if (KIND == 5) {  // h is z, h2 is n
      const T n0 = h2.e[i];
      const T n1 = n0 + dd * dd;
      const T r = sqrt(n1);
      const T s = (r - sqrt(n0)) * o.inv_lr;
      const T z1 = (h.e[i] + dd) - s * p.e[i];
      h2.e[i] = n1;
      h.e[i] = z1;
      // a NaN z1 fails the comparison and goes on through the closed form
      p.e[i] = fabs(z1) <= o.l1 ? T(0) : (copysign(o.l1, z1) - z1) / ((o.fbeta + r) * o.inv_lr + o.l2);
    } else {
      p.e[i] = p.e[i] - o.lr * dd;
    }
    gs.e[i] = T(0);
  }
  return dirty;
}

// KIND: 1 = SGD, 2 = Adagrad, 3 = momentum, 4 = Adam, 5 = FTRL-Proximal
// (pskv_optimizer_kind).  Winners only, one writer per row.  `state` is slot 0
// (h / v / m / z), `state2` slot 1 (Adam's v, FTRL's n).  No instantiation
// spills with kRowsInFlight rows in flight (DESIGN.md §8d, §8h and §8i have
// the resource tables), Adam's and FTRL's five units per row included.
template <typename T, int KIND, int V, typename Args, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_row_step_apply(Args ga, DenseView d, T* __restrict__ gsum,
                                                           T* __restrict__ state, T* __restrict__ state2,
                                                           const unsigned long long* __restrict__ owner,
                                                           uint32_t epoch, RowShape rs, OptArgs<T> o) {
  static_assert(kStepPooled<Args> || !WEIGHTED, "only bag rows are weighted");
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  const uint32_t U = rs.units;
  T* __restrict__ param = reinterpret_cast<T*>(d.param);
  const uint32_t nvwg = step_nvwg(ga);
  for (uint32_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const int j = step_batch_of(ga, wg);
    decltype(auto) a = step_batch(ga, j);
    // (a plain batch is copied, so its three words are loaded here, up front; a
    // pooled descriptor is read where it is used.  This and the order of the
    // reads below are what the compiler's schedule hangs on: DESIGN.md §8j)
    //
    // A pooled group:
    // The descriptor's fields come from a computed place in the kernel
    // arguments, so unlike the single-batch kernel's they cannot be loaded
    // again where they are used, and held in scalar registers across the unit
    // loop they would be spilled (Adam: up to 13 of them).
    // Where that happens -- every kind with state, but for float rows taken
    // one element at a time -- what only the per-lane arithmetic in front of
    // the unit loop reads is kept in vector registers instead.
    constexpr bool kPin = kStepPoolGroup<Args> && KIND >= 2 && (V > 1 || sizeof(T) > 4);
    const uint32_t* keys = in_vgprs<kPin>(a.keys);
    const T* weights = nullptr;
    const uint64_t* offsets = nullptr;
    if constexpr (kStepPooled<Args>) {
      weights = reinterpret_cast<const T*>(a.weights);
      offsets = in_vgprs<kPin>(a.offsets);
    }
    const T* __restrict__ rows = reinterpret_cast<const T*>(step_rows(a));
    const uint64_t n = a.n;
    const uint64_t base = (uint64_t)(wg - step_first_wg(ga, j)) * kGeneralChunk;
    const uint64_t gbase = step_elem_prefix(ga, j) + base;
    // A pooled group: the tag of the workgroup's first position; a group holds fewer than 2^32
    // keys, so adding a position's offset never carries into the epoch
    const unsigned long long tag0 = kStepPoolGroup<Args> ? in_vgprs<kPin>(row_tag(epoch, gbase)) : 0;
    // nearly every workgroup holds a winner: the span is looked up at once
    // (in its declaration: assigned in a block of its own it is scheduled otherwise)
    bool have = kStepPoolGroup<Args>;
    PoolSpan sp = step_span<kStepPoolGroup<Args>, kPin>(a, base);
    for (uint32_t r0 = grp; r0 < (uint32_t)kGeneralChunk; r0 += kRowsInFlight * G) {
      if (base + r0 >= n) break;
      RowStep s;
      load_step(s, keys, n, base, r0, G, d);
      bool win[kRowsInFlight];
      bool any = false;
#pragma unroll
      for (int r = 0; r < kRowsInFlight; ++r) {
        const unsigned long long tag =
            kStepPoolGroup<Args> ? tag0 + (r0 + (uint32_t)r * G) : row_tag(epoch, gbase + r0 + (uint32_t)r * G);
        win[r] = s.in[r] && owner[s.off[r]] == tag;
        any |= win[r];
      }
      if (!any) continue;
      // the winner's gradient row: its own of `rows`, or its bag's times w[r] where WEIGHTED
      uint64_t bag[kRowsInFlight];
      T w[kRowsInFlight];
      if constexpr (kStepPooled<Args>) {
        step_bags(a, offsets, base, sp, have, s, win, bag);
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r)
          w[r] = (WEIGHTED && (kStepPoolGroup<Args> ? weights != nullptr : true) && win[r]) ? weights[s.i[r]] : T(1);
      }
      for (uint32_t u = lane; u < U; u += rs.lanes) {
        OptUnit<T, V> g[kRowsInFlight], gs[kRowsInFlight], p[kRowsInFlight], h[kRowsInFlight], h2[kRowsInFlight];
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r) {
          if (!win[r]) continue;
          const uint64_t at = (uint64_t)s.off[r] * U + u;
          g[r] = load_opt_unit<T, V>(rows, (kStepPooled<Args> ? bag[r] : s.i[r]) * U + u);
          gs[r] = load_opt_unit<T, V>(gsum, at);
          p[r] = load_opt_unit<T, V>(param, at);
          if (KIND >= 2) h[r] = load_opt_unit<T, V>(state, at);
          if (KIND >= 4) h2[r] = load_opt_unit<T, V>(state2, at);
        }
#pragma unroll
        for (int r = 0; r < kRowsInFlight; ++r) {
          if (!win[r]) continue;
          const uint64_t at = (uint64_t)s.off[r] * U + u;
          if (WEIGHTED) {  // (a batch of a group without weights: times one, exact)
#pragma unroll
            for (int i = 0; i < V; ++i) g[r].e[i] = rounded_mul(w[r], g[r].e[i]);
          }
          const bool dirty = opt_step_unit<T, KIND, V>(g[r], gs[r], p[r], h[r], h2[r], o);
          store_opt_unit<T, V>(param, at, p[r]);
          if (KIND >= 2) store_opt_unit<T, V>(state, at, h[r]);
          if (KIND >= 4) store_opt_unit<T, V>(state2, at, h2[r]);
          if (dirty) store_opt_unit<T, V>(gsum, at, gs[r]);
        }
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_fill(T* __restrict__ p, uint64_t n, T v) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) p[i] = v;
}

uint32_t row_grid(uint32_t nwg) { return nwg < 4096u ? nwg : 4096u; }

// f(T()) with T the shard's float type (dtype: 1 float, 2 double), then the
// launch's error; any other dtype is refused.
template <typename F>
hipError_t with_float_type(int dtype, F&& f) {
  if (dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  dtype == 1 ? f(float()) : f(double());
  return hipGetLastError();
}

// f(UT()) with UT the unit of a copy kernel: 16 bytes, or one element of vb bytes.
template <typename F>
hipError_t with_unit_type(const RowShape& rs, int vb, F&& f) {
  if (rs.unit_bytes == 16)
    f(u32x4());
  else if (vb == 4)
    f(uint32_t());
  else
    f((unsigned long long)0);
  return hipGetLastError();
}

template <typename T>
OptArgs<T> round_opt_args(const OptArgs<double>& h) {
  // (mu to b: FTRL's l1, l2, fbeta and inv_lr lie in the same places)
  OptArgs<T> o;
  o.lr = (T)h.lr, o.wd = (T)h.wd, o.eps = (T)h.eps;
  o.mu = (T)h.mu, o.beta1 = (T)h.beta1, o.omb1 = (T)h.omb1, o.beta2 = (T)h.beta2, o.omb2 = (T)h.omb2;
  o.a = (T)h.a, o.b = (T)h.b;
  o.nesterov = h.nesterov;
  return o;
}

// f(K) with K the std::integral_constant of optimizer kind `kind` (1 to 5:
// opt_kind_ok), so that a kind reaches the kernels as a template argument in
// one place.
template <typename F>
void with_opt_kind(int kind, F&& f) {
  if (kind == 5)
    f(std::integral_constant<int, 5>());
  else if (kind == 4)
    f(std::integral_constant<int, 4>());
  else if (kind == 3)
    f(std::integral_constant<int, 3>());
  else if (kind == 2)
    f(std::integral_constant<int, 2>());
  else
    f(std::integral_constant<int, 1>());
}

// A known kind with the state slots it steps.
bool opt_kind_ok(int kind, void* const state[2]) {
  return kind >= 1 && kind <= 5 && (kind < 2 || state[0]) && (kind < 4 || state[1]);
}

// f(W) with W whether the block's kernels multiply by weights: for a group,
// some batch of it has them.  Rows given by value have none.
template <typename F>
void with_step_weights(const GroupArgs&, F&& f) {
  f(std::false_type());
}
template <typename F>
void with_step_weights(const PoolPushArgs& a, F&& f) {
  a.weights ? f(std::true_type()) : f(std::false_type());
}
template <typename F>
void with_step_weights(const PoolGroupArgs& ga, F&& f) {
  bool weighted = false;
  for (int j = 0; j < ga.nb; ++j) weighted |= ga.b[j].weights != nullptr;
  weighted ? f(std::true_type()) : f(std::false_type());
}

// An argument block as the step kernels assume it, nwg its virtual workgroups
// (> 0).  GroupArgs: as make_group built it.  PoolPushArgs: one batch of 1 to
// kMaxPiece keys and at least one bag.  PoolGroupArgs: 1 to kMaxPoolBatches
// such batches.
bool step_args_ok(const GroupArgs&, uint32_t) { return true; }
bool step_args_ok(const PoolPushArgs& a, uint32_t nwg) {
  return a.n != 0 && a.n <= kMaxPiece && a.nbags != 0 && nwg == (a.n + kGeneralChunk - 1) / kGeneralChunk;
}
bool step_args_ok(const PoolGroupArgs& ga, uint32_t nwg) {
  if (ga.nb < 1 || ga.nb > kMaxPoolBatches || ga.wg_prefix[ga.nb] != nwg) return false;
  for (int j = 0; j < ga.nb; ++j)
    if (ga.b[j].n == 0 || ga.b[j].n > kMaxPiece || ga.b[j].nbags == 0 ||
        ga.wg_prefix[j + 1] - ga.wg_prefix[j] != (ga.b[j].n + kGeneralChunk - 1) / kGeneralChunk)
      return false;
  return true;
}

// ----------------------------------------------------------- pooled pulls
// pskv_get_pooled: a lane group owns a BAG at a time and keeps
// one accumulator unit per lane: the unit strips of a row wider than the
// group are the outer loop, the bag's keys the inner one (the keys are re-read
// from cache), so a 4096-wide row costs the registers of a 64-unit one.  The
// additions are a dependent chain, the row loads in front of them are not: R
// rows are loaded before the first is added.  T is the shard's value type
// (int32 as uint32_t: exact with wrap); the multiply-add is always one fma, in
// every instantiation, so the unit-16 and the element path return the same bits.
// Order of the additions, the clamp of device offsets and the chunks of bags
// longer than kPoolChunk: pskv_plan.h.
constexpr int kPoolChunkRowsInFlight = 16;  // k_row_pooled_chunks: a chunk is one lane group's chain
constexpr int kPoolPartsInFlight = 8;       // partial rows of a long bag, read back by k_row_pooled

__device__ __forceinline__ float pool_fma(float w, float p, float a) { return __builtin_fmaf(w, p, a); }
__device__ __forceinline__ double pool_fma(double w, double p, double a) { return __builtin_fma(w, p, a); }
__device__ __forceinline__ uint32_t pool_fma(uint32_t w, uint32_t p, uint32_t a) { return a + w * p; }

template <typename T, int V>
__device__ __forceinline__ OptUnit<T, V> zero_opt_unit() {
  OptUnit<T, V> r;
#pragma unroll
  for (int i = 0; i < V; ++i) r.e[i] = T(0);
  return r;
}

template <typename T, int V, bool NT>
__device__ __forceinline__ void store_pool_unit(T* p, uint64_t unit, const OptUnit<T, V>& r) {
  if constexpr (V == 1) {
    store_unit<NT>(p + unit, r.e[0]);
  } else {
    typedef T vt __attribute__((ext_vector_type(V)));
    vt v;
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = r.e[i];
    store_unit<NT>(reinterpret_cast<vt*>(p + unit * V), v);
  }
}

// acc = t when it is the first term (the sum of one term is that term, bit
// for bit), else acc + t.
template <typename T, int V>
__device__ __forceinline__ void pool_add_unit(OptUnit<T, V>& acc, bool& have, const OptUnit<T, V>& t) {
#pragma unroll
  for (int i = 0; i < V; ++i) acc.e[i] = have ? acc.e[i] + t.e[i] : t.e[i];
  have = true;
}

// Unit u of the sum over key positions [b, e), in key order, R rows in flight.
// The keys (and weights) of the next R positions are loaded before the rows
// of this round are added, so a long bag's chain costs one memory latency per
// round, not a key's and then a row's.
// oor: some key lay outside the range (it counted as a zero row).
template <typename T, int V, int R, bool WEIGHTED>
__device__ __forceinline__ OptUnit<T, V> pool_sum(const uint32_t* __restrict__ keys, const T* __restrict__ weights,
                                                  uint64_t b, uint64_t e, const T* __restrict__ param,
                                                  const DenseView& d, uint32_t U, uint32_t u, bool& oor) {
  OptUnit<T, V> acc = zero_opt_unit<T, V>();
  bool have = false;
  uint32_t k[R];
  T w[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    k[r] = b + r < e ? keys[b + r] : 0u;
    w[r] = (WEIGHTED && b + r < e) ? weights[b + r] : T(0);
  }
  for (uint64_t i = b; i < e; i += R) {
    OptUnit<T, V> p[R];
    T wc[R];
    bool live[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      live[r] = i + r < e;
      const uint32_t off = k[r] - d.key_begin;
      const bool in = live[r] && (uint64_t)off < d.range;
      oor |= live[r] && !in;
      wc[r] = w[r];
      p[r] = in ? load_opt_unit<T, V>(param, (uint64_t)off * U + u) : zero_opt_unit<T, V>();
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t nx = i + R + r;
      k[r] = nx < e ? keys[nx] : 0u;
      w[r] = (WEIGHTED && nx < e) ? weights[nx] : T(0);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!live[r]) continue;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (WEIGHTED)
          acc.e[j] = have ? pool_fma(wc[r], p[r].e[j], acc.e[j]) : wc[r] * p[r].e[j];
        else
          acc.e[j] = have ? acc.e[j] + p[r].e[j] : p[r].e[j];
      }
      have = true;
    }
  }
  return acc;
}

// Work items: the windows of the key array (pskv_plan.h), one lane group per
// window.  Each sums the at most two long-bag chunks that start in its window
// into their partial rows.
template <typename T, int V, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_row_pooled_chunks(PoolArgs a, DenseView d, uint32_t* err, RowShape rs) {
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  const uint32_t U = rs.units;
  const T* __restrict__ param = reinterpret_cast<const T*>(d.param);
  const T* __restrict__ weights = reinterpret_cast<const T*>(a.weights);
  T* __restrict__ part = reinterpret_cast<T*>(a.part);
  const uint64_t nwin = (a.n + kPoolChunk - 1) / kPoolChunk;
  for (uint64_t q = (uint64_t)blockIdx.x * G + grp; q < nwin; q += (uint64_t)gridDim.x * G) {
    const uint64_t lo = q * kPoolChunk;
    const uint64_t hi = (lo + kPoolChunk < a.n ? lo + kPoolChunk : a.n) - 1;
    const uint64_t ba = pool_bag_of(a.offsets, a.nbags, lo);
    const uint64_t bb = pool_bag_of(a.offsets, a.nbags, hi);
    for (int cand = 0; cand < 2; ++cand) {
      if (cand == 1 && bb == ba) break;
      const uint64_t bag = cand ? bb : ba;  // < nbags
      const PoolBag bg = pool_clamp(a.offsets[bag], a.offsets[bag + 1], a.n);
      const uint64_t c = pool_window_chunk(bg.begin, bg.end, q);
      if (c == kPoolNone) continue;
      const uint64_t p0 = bg.begin + c * kPoolChunk;  // in the window, below bg.end <= n
      const uint64_t p1 = p0 + kPoolChunk < bg.end ? p0 + kPoolChunk : bg.end;
      const uint64_t slot = pool_slot(bg.begin, c);  // < pool_slots(n), as p0 < n
      bool oor = false;
      for (uint32_t u = lane; u < U; u += rs.lanes) {
        const OptUnit<T, V> acc =
            pool_sum<T, V, kPoolChunkRowsInFlight, WEIGHTED>(a.keys, weights, p0, p1, param, d, U, u, oor);
        store_opt_unit<T, V>(part, slot * U + u, acc);
      }
      if (oor && lane == 0) atomicOr(err, kErrRowOutOfRange);
    }
  }
}

// Work items: bags, in virtual workgroups of kPoolBagsPerWg, grid-stride; group
// g of the workgroup's G takes the workgroup's bags g, g + G, ...  A bag of at
// most kPoolChunk keys is summed here; a longer one adds up its chunks'
// partial rows (k_row_pooled_chunks ran first) in chunk order.
template <typename T, int V, bool NT, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_row_pooled(PoolArgs a, DenseView d, uint32_t* err, RowShape rs) {
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  const uint32_t U = rs.units;
  const T* __restrict__ param = reinterpret_cast<const T*>(d.param);
  const T* __restrict__ weights = reinterpret_cast<const T*>(a.weights);
  const T* __restrict__ part = reinterpret_cast<const T*>(a.part);
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  const uint64_t nvwg = (a.nbags + kPoolBagsPerWg - 1) / kPoolBagsPerWg;
  for (uint64_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    for (uint32_t g = grp; g < kPoolBagsPerWg; g += G) {
      const uint64_t bag = wg * kPoolBagsPerWg + g;
      if (bag >= a.nbags) break;
      const PoolBag bg = pool_clamp(a.offsets[bag], a.offsets[bag + 1], a.n);
      const uint64_t m = bg.end - bg.begin;
      bool oor = false;
      for (uint32_t u = lane; u < U; u += rs.lanes) {
        OptUnit<T, V> acc;
        if (m > kPoolChunk) {
          const uint64_t nc = pool_chunks(m);
          bool have = false;
          acc = zero_opt_unit<T, V>();
          for (uint64_t c = 0; c < nc; c += kPoolPartsInFlight) {
            OptUnit<T, V> s[kPoolPartsInFlight];
#pragma unroll
            for (int r = 0; r < kPoolPartsInFlight; ++r)
              if (c + r < nc) s[r] = load_opt_unit<T, V>(part, pool_slot(bg.begin, c + r) * U + u);
#pragma unroll
            for (int r = 0; r < kPoolPartsInFlight; ++r)
              if (c + r < nc) pool_add_unit<T, V>(acc, have, s[r]);
          }
        } else {
          acc = pool_sum<T, V, kRowsInFlight, WEIGHTED>(a.keys, weights, bg.begin, bg.end, param, d, U, u, oor);
        }
        store_pool_unit<T, V, NT>(out, bag * U + u, acc);
      }
      if (oor && lane == 0) atomicOr(err, kErrRowOutOfRange);
    }
  }
}

// f(T()) with T the arithmetic type of a pooled pull (dtype 0: int32 summed as
// uint32_t, 1: float, 2: double), then the launch's error.
template <typename F>
hipError_t with_pool_type(int dtype, F&& f) {
  if (dtype == 0)
    f(uint32_t());
  else if (dtype == 1)
    f(float());
  else if (dtype == 2)
    f(double());
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

template <typename T, int V>
void launch_row_pooled_v(uint32_t grid, bool nt, const PoolArgs& a, const DenseView& d, uint32_t* err,
                         const RowShape& rs, hipStream_t st) {
  if (a.weights) {
    if (nt)
      k_row_pooled<T, V, true, true><<<grid, kBlock, 0, st>>>(a, d, err, rs);
    else
      k_row_pooled<T, V, false, true><<<grid, kBlock, 0, st>>>(a, d, err, rs);
  } else {
    if (nt)
      k_row_pooled<T, V, true, false><<<grid, kBlock, 0, st>>>(a, d, err, rs);
    else
      k_row_pooled<T, V, false, false><<<grid, kBlock, 0, st>>>(a, d, err, rs);
  }
}

template <typename T, int V>
void launch_row_pooled_chunks_v(uint32_t grid, const PoolArgs& a, const DenseView& d, uint32_t* err,
                                const RowShape& rs, hipStream_t st) {
  if (a.weights)
    k_row_pooled_chunks<T, V, true><<<grid, kBlock, 0, st>>>(a, d, err, rs);
  else
    k_row_pooled_chunks<T, V, false><<<grid, kBlock, 0, st>>>(a, d, err, rs);
}

}  // namespace

RowShape row_shape(uint32_t width, int vb, bool unit16) {
  RowShape rs;
  rs.unit_bytes = unit16 ? 16u : (uint32_t)vb;
  rs.units = (uint32_t)((uint64_t)width * (uint32_t)vb / rs.unit_bytes);
  rs.lanes = 1;
  rs.lshift = 0;
  while (rs.lanes < 64u && rs.lanes < rs.units) {
    rs.lanes <<= 1;
    ++rs.lshift;
  }
  return rs;
}

hipError_t launch_row_gather(int vb, bool nt, const GroupArgs& ga, uint32_t nwg, const DenseView& d,
                             const RowShape& rs, hipStream_t st) {
  if (nwg == 0) return hipSuccess;
  const uint32_t grid = row_grid(nwg);
  return with_unit_type(rs, vb, [&](auto u) {
    using UT = decltype(u);
    if (nt)
      k_row_gather<UT, true><<<grid, kBlock, 0, st>>>(ga, d, rs);
    else
      k_row_gather<UT, false><<<grid, kBlock, 0, st>>>(ga, d, rs);
  });
}

hipError_t launch_row_commit(int vb, const GroupArgs& ga, uint32_t nwg, const DenseView& d,
                             const unsigned long long* owner, const Ovf& o, uint32_t epoch,
                             const RowShape& rs, hipStream_t st) {
  if (nwg == 0) return hipSuccess;
  const uint32_t grid = row_grid(nwg);
  uint32_t* err = &o.c->stat[1];
  return with_unit_type(rs, vb, [&](auto u) {
    k_row_commit<decltype(u)><<<grid, kBlock, 0, st>>>(ga, d, owner, err, epoch, rs);
  });
}

hipError_t launch_row_accumulate(int dtype, const GroupArgs& ga, uint32_t nwg, const DenseView& d,
                                 const Ovf& o, const RowShape& rs, hipStream_t st) {
  if (nwg == 0) return hipSuccess;
  const uint32_t grid = row_grid(nwg);
  uint32_t* err = &o.c->stat[1];
  if (dtype == 0)
    k_row_accumulate<int><<<grid, kBlock, 0, st>>>(ga, d, err, rs);
  else if (dtype == 1)
    k_row_accumulate<float><<<grid, kBlock, 0, st>>>(ga, d, err, rs);
  else
    k_row_accumulate<double><<<grid, kBlock, 0, st>>>(ga, d, err, rs);
  return hipGetLastError();
}

template <typename Args>
hipError_t launch_row_step_losers(int dtype, const Args& a, uint32_t nwg, const DenseView& d, void* gsum,
                                  const unsigned long long* owner, const Ovf& o, uint32_t epoch, const RowShape& rs,
                                  hipStream_t st) {
  if (nwg == 0) return hipSuccess;
  if (!step_args_ok(a, nwg)) return hipErrorInvalidValue;
  const uint32_t grid = row_grid(nwg);
  uint32_t* err = &o.c->stat[1];
  return with_float_type(dtype, [&](auto z) {
    using T = decltype(z);
    with_step_weights(a, [&](auto w) {
      k_row_step_losers<T, Args, decltype(w)::value>
          <<<grid, kBlock, 0, st>>>(a, d, static_cast<T*>(gsum), owner, err, epoch, rs);
    });
  });
}

template <typename Args>
hipError_t launch_row_step_apply(int dtype, int kind, const Args& a, uint32_t nwg, const DenseView& d, void* gsum,
                                 void* const state[2], const unsigned long long* owner, uint32_t epoch,
                                 const RowShape& rs, const OptArgs<double>& hy, hipStream_t st) {
  if (nwg == 0) return hipSuccess;
  if (!step_args_ok(a, nwg) || !opt_kind_ok(kind, state)) return hipErrorInvalidValue;
  const uint32_t grid = row_grid(nwg);
  return with_float_type(dtype, [&](auto z) {
    using T = decltype(z);
    const OptArgs<T> o = round_opt_args<T>(hy);
    T* g = static_cast<T*>(gsum);
    T* s1 = static_cast<T*>(state[0]);
    T* s2 = static_cast<T*>(state[1]);
    with_opt_kind(kind, [&](auto k) {
      with_step_weights(a, [&](auto w) {
        constexpr int K = decltype(k)::value;
        constexpr bool W = decltype(w)::value;
        constexpr int V16 = 16 / sizeof(T);
        if (rs.unit_bytes == 16)
          k_row_step_apply<T, K, V16, Args, W><<<grid, kBlock, 0, st>>>(a, d, g, s1, s2, owner, epoch, rs, o);
        else
          k_row_step_apply<T, K, 1, Args, W><<<grid, kBlock, 0, st>>>(a, d, g, s1, s2, owner, epoch, rs, o);
      });
    });
  });
}

#define PSKV_STEP_LAUNCHERS(Args)                                                                                \
  template hipError_t launch_row_step_losers<Args>(int, const Args&, uint32_t, const DenseView&, void*,         \
                                                   const unsigned long long*, const Ovf&, uint32_t,             \
                                                   const RowShape&, hipStream_t);                               \
  template hipError_t launch_row_step_apply<Args>(int, int, const Args&, uint32_t, const DenseView&, void*,     \
                                                  void* const[2], const unsigned long long*, uint32_t,          \
                                                  const RowShape&, const OptArgs<double>&, hipStream_t)
PSKV_STEP_LAUNCHERS(GroupArgs);
PSKV_STEP_LAUNCHERS(PoolPushArgs);
PSKV_STEP_LAUNCHERS(PoolGroupArgs);
#undef PSKV_STEP_LAUNCHERS

hipError_t launch_fill(int dtype, void* p, uint64_t n, double v, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const uint64_t nwg = (n + kBlock - 1) / kBlock;
  const uint32_t grid = (uint32_t)(nwg < 65536u ? nwg : 65536u);
  return with_float_type(dtype, [&](auto z) {
    using T = decltype(z);
    k_fill<T><<<grid, kBlock, 0, st>>>(static_cast<T*>(p), n, (T)v);
  });
}

hipError_t launch_row_pooled_chunks(int dtype, const PoolArgs& a, const DenseView& d, const Ovf& o,
                                    const RowShape& rs, hipStream_t st) {
  if (a.nbags == 0 || a.n <= kPoolChunk) return hipSuccess;  // no bag can be long
  if (!a.part) return hipErrorInvalidValue;
  const uint64_t G = (uint64_t)kBlock >> rs.lshift;
  const uint64_t nwg = ((a.n + kPoolChunk - 1) / kPoolChunk + G - 1) / G;
  const uint32_t grid = row_grid((uint32_t)std::min<uint64_t>(nwg, 4096));
  uint32_t* err = &o.c->stat[1];
  return with_pool_type(dtype, [&](auto z) {
    using T = decltype(z);
    if (rs.unit_bytes == 16)
      launch_row_pooled_chunks_v<T, 16 / sizeof(T)>(grid, a, d, err, rs, st);
    else
      launch_row_pooled_chunks_v<T, 1>(grid, a, d, err, rs, st);
  });
}

hipError_t launch_row_pooled(int dtype, bool nt, const PoolArgs& a, const DenseView& d, const Ovf& o,
                             const RowShape& rs, hipStream_t st) {
  if (a.nbags == 0) return hipSuccess;
  const uint64_t nwg = (a.nbags + kPoolBagsPerWg - 1) / kPoolBagsPerWg;
  const uint32_t grid = row_grid((uint32_t)std::min<uint64_t>(nwg, 4096));
  uint32_t* err = &o.c->stat[1];
  return with_pool_type(dtype, [&](auto z) {
    using T = decltype(z);
    if (rs.unit_bytes == 16)
      launch_row_pooled_v<T, 16 / sizeof(T)>(grid, nt, a, d, err, rs, st);
    else
      launch_row_pooled_v<T, 1>(grid, nt, a, d, err, rs, st);
  });
}

}  // namespace pskv
