// pskv_init.hip — CDNA4 (gfx950) kernels of a shard's row initializer
// (pskv_shard_set_initializer; pskv.h "Row initializers"): the
// value of a row that was never written, a pure function of (seed, key,
// element, dtype, kind, a, b).
//
//   k_row_init_range  a dense row shard's clear: row r = init(key_begin + r)
//   k_row_init_new    a sparse shard's writing call, between k_index_insert and
//                     k_index_translate: the slots handed out since the last
//                     fill, [mark, min(stat[0], capacity)), each from the key
//                     in slot_keys; the last workgroup to finish moves the mark
//   k_init_eval       pskv_get_init: out row i = init(keys[i])
//
// The generator.  One Philox4x32-10 block, counter (key, q, 0, 0) and key
// (seed low word, seed high word), makes the 16-byte unit q of a key's row: four
// floats or two doubles.  A lane makes whole units, so no block is computed
// twice, and a row of width 8 is the prefix of the same key's row of width 16.
// Philox is ten rounds of two 32 x 32 -> 64 multiplications (v_mul_lo_u32 and
// v_mul_hi_u32: gfx950 has no 64-bit integer multiply), unrolled, all in
// registers: no table, no LDS, no scratch.
//
// Lane mapping.  k_row_init_range: consecutive lanes take consecutive units of
// the array (the units of a row lie side by side), so a wave's stores are one
// contiguous 1 KiB segment when the row size is a multiple of 16 bytes.
// k_row_init_new and k_init_eval: the row kernels' mapping (pskv_rows.hip): a
// group of L = min(64, next_pow2(U)) lanes owns one row at a time, lane l
// taking units l, l + L, ... (wide rows are walked in strips of L units), and
// every lane of a group reads the same key.  A row whose size is no multiple
// of 16 bytes (or whose array is not 16-byte aligned) is stored element by
// element, the last unit cut at the width.
//
// The normal kind is evaluated in double for both value types (log, sqrt, sin
// and cos of the device library) and rounded to the value type once.
#include <algorithm>
#include <type_traits>

#include "pskv_internal.h"

namespace pskv {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct Philox4 {
  uint32_t x[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
    const uint32_t hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kW0;
    k1 += kW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

template <typename T>
struct InitUnit {
  static constexpr int kPer = 16 / (int)sizeof(T);
  T e[kPer];
};

// 53 bits of two words as an integer-valued double (exact).
__device__ __forceinline__ double bits53(uint32_t hi, uint32_t lo) {
  return (double)(hi >> 5) * 67108864.0 + (double)(lo >> 6);
}

// Box-Muller in double: z[0] = rad cos(ang), z[1] = rad sin(ang), rad = sqrt(-2
// log u1), ang = 2 pi u2; u1 in (0, 1], u2 in [0, 1).  Every product is rounded
// on its own, so the device's contraction rules are not part of the value.
__device__ __forceinline__ void box_muller(double u1, double u2, double z[2]) {
  const double rad = sqrt(-2.0 * log(u1));
  const double ang = rounded_mul(6.283185307179586476925286766559, u2);
  double sn, cs;
  sincos(ang, &sn, &cs);
  z[0] = rounded_mul(rad, cs);
  z[1] = rounded_mul(rad, sn);
}

__device__ __forceinline__ double normal_value(const InitRule& r, double z) { return r.a + rounded_mul(r.b, z); }

// Unit q of key's row.
template <typename T>
__device__ __forceinline__ InitUnit<T> init_unit(const InitRule& r, uint32_t key, uint32_t q) {
  InitUnit<T> out;
  constexpr int P = InitUnit<T>::kPer;
  if (r.kind == 1) {  // PSKV_INIT_CONSTANT
#pragma unroll
    for (int i = 0; i < P; ++i) out.e[i] = (T)r.a;
    return out;
  }
  const Philox4 px = philox4x32_10(key, q, r.seed_lo, r.seed_hi);
  if (r.kind == 2) {  // PSKV_INIT_UNIFORM: rounded(u * d) + lo, two roundings
    const T lo = (T)r.a, d = (T)(r.b - r.a);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      T u;
      if constexpr (sizeof(T) == 4)
        u = (T)(px.x[i] >> 8) * (T)5.9604644775390625e-8;  // 2^-24: exact
      else
        u = (T)(bits53(px.x[2 * i], px.x[2 * i + 1]) * 1.1102230246251565404e-16);  // 2^-53: exact
      out.e[i] = rounded_mul(u, d) + lo;
    }
    return out;
  }
  // PSKV_INIT_NORMAL
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double u1 = (double)((px.x[2 * h] >> 8) + 1u) * 5.9604644775390625e-8;
      const double u2 = (double)(px.x[2 * h + 1] >> 8) * 5.9604644775390625e-8;
      double z[2];
      box_muller(u1, u2, z);
      out.e[2 * h] = (T)normal_value(r, z[0]);
      out.e[2 * h + 1] = (T)normal_value(r, z[1]);
    }
  } else {
    const double u1 = (bits53(px.x[0], px.x[1]) + 1.0) * 1.1102230246251565404e-16;
    const double u2 = bits53(px.x[2], px.x[3]) * 1.1102230246251565404e-16;
    double z[2];
    box_muller(u1, u2, z);
    out.e[0] = (T)normal_value(r, z[0]);
    out.e[1] = (T)normal_value(r, z[1]);
  }
  return out;
}

// Unit q of a row of `width` values at `row`.  VEC: one 16-byte store (the row
// size is a multiple of 16 bytes and `row` is aligned); else the unit's
// elements below the width, one store each.
template <typename T, bool VEC>
__device__ __forceinline__ void store_init_unit(T* row, uint32_t q, uint32_t width, const InitUnit<T>& v) {
  constexpr int P = InitUnit<T>::kPer;
  if constexpr (VEC) {
    u32x4 w;
    if constexpr (sizeof(T) == 4) {
      w = u32x4{__float_as_uint(v.e[0]), __float_as_uint(v.e[1]), __float_as_uint(v.e[2]), __float_as_uint(v.e[3])};
    } else {
      const unsigned long long b0 = (unsigned long long)__double_as_longlong(v.e[0]);
      const unsigned long long b1 = (unsigned long long)__double_as_longlong(v.e[1]);
      w = u32x4{(uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32)};
    }
    reinterpret_cast<u32x4*>(row)[q] = w;
  } else {
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (q * (uint32_t)P + (uint32_t)i < width) row[q * (uint32_t)P + (uint32_t)i] = v.e[i];
  }
}

// The body k_row_init_new and k_init_eval share: the lane's strips of one row.
template <typename T, bool VEC>
__device__ __forceinline__ void init_row(const InitRule& r, uint32_t key, T* row, uint32_t width, uint32_t units,
                                         uint32_t lane, uint32_t lanes) {
  for (uint32_t q = lane; q < units; q += lanes) store_init_unit<T, VEC>(row, q, width, init_unit<T>(r, key, q));
}

constexpr uint32_t kInitChunk = kBlock;  // units per virtual workgroup of k_row_init_range

// total = rows * units.  A virtual workgroup takes kInitChunk consecutive units
// of the array; its first unit's row and place in the row come from one 64-bit
// division (uniform over the workgroup), a lane's own from a 32-bit one.
template <typename T, bool VEC>
__global__ PSKV_NO_PK_F32 __launch_bounds__(kBlock) void k_row_init_range(InitRule r, T* __restrict__ param,
                                                                         uint32_t key_begin, uint64_t total,
                                                                         uint32_t width, uint32_t units) {
  const uint64_t nvwg = (total + kInitChunk - 1) / kInitChunk;
  for (uint64_t wg = blockIdx.x; wg < nvwg; wg += gridDim.x) {
    const uint64_t first = wg * kInitChunk;
    if (first + threadIdx.x >= total) continue;
    const uint64_t row0 = first / units;
    const uint32_t at = (uint32_t)(first - row0 * units) + threadIdx.x;  // < units + kBlock
    const uint32_t up = at / units;
    const uint64_t row = row0 + up;
    const uint32_t q = at - up * units;
    store_init_unit<T, VEC>(param + row * width, q, width, init_unit<T>(r, key_begin + (uint32_t)row, q));
  }
}

// mark[0]: the first slot not yet filled; mark[1]: the ticket.  Every workgroup
// reads the same two words -- the mark moves only after every workgroup has
// drawn its ticket, and the slot counter only in k_index_insert -- so either
// all leave at once (no new key: two loads) or all fill their share and draw.
template <typename T, bool VEC>
__global__ PSKV_NO_PK_F32 __launch_bounds__(kBlock) void k_row_init_new(InitRule r, T* __restrict__ param,
                                                                       SparseIndex x, uint32_t* mark, uint32_t width,
                                                                       RowShape rs) {
  const uint32_t from = __hip_atomic_load(mark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t end = __hip_atomic_load(x.stat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  end = end < x.capacity ? end : x.capacity;
  if (from >= end) return;
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  for (uint64_t slot = (uint64_t)from + (uint64_t)blockIdx.x * G + grp; slot < end; slot += (uint64_t)gridDim.x * G)
    init_row<T, VEC>(r, x.slot_keys[slot], param + slot * width, width, rs.units, lane, rs.lanes);
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(mark + 1, 1u) == gridDim.x - 1u) {
      __hip_atomic_store(mark + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(mark, end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <typename T, bool VEC>
__global__ PSKV_NO_PK_F32 __launch_bounds__(kBlock) void k_init_eval(InitRule r, const uint32_t* __restrict__ keys,
                                                                    uint64_t n, T* __restrict__ out, uint32_t width,
                                                                    RowShape rs) {
  const uint32_t lane = threadIdx.x & (rs.lanes - 1u);
  const uint32_t grp = threadIdx.x >> rs.lshift;
  const uint32_t G = (uint32_t)kBlock >> rs.lshift;
  for (uint64_t i = (uint64_t)blockIdx.x * G + grp; i < n; i += (uint64_t)gridDim.x * G)
    init_row<T, VEC>(r, keys[i], out + i * width, width, rs.units, lane, rs.lanes);
}

// Units of 16 bytes per row, the last one cut at the width where the row size
// is no multiple of 16; the lane group of the row kernels over them.
RowShape init_shape(uint32_t width, int vb) {
  const uint32_t per = 16u / (uint32_t)vb;
  return row_shape((width + per - 1u) / per * per, vb, /*unit16=*/true);
}

bool init_vec(const void* p, uint32_t width, int vb) {
  return ((uint64_t)width * (uint32_t)vb) % 16 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

constexpr uint64_t kInitGridCap = 4096;

// f(T(), vec) with T the shard's float type (dtype: 1 float, 2 double).
template <typename F>
hipError_t with_init_type(int dtype, bool vec, F&& f) {
  if (dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  if (dtype == 1)
    vec ? f(float(), std::true_type()) : f(float(), std::false_type());
  else
    vec ? f(double(), std::true_type()) : f(double(), std::false_type());
  return hipGetLastError();
}

}  // namespace

hipError_t launch_row_init_range(int dtype, const InitRule& r, void* param, uint32_t key_begin, uint64_t rows,
                                 uint32_t width, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  const int vb = dtype == 1 ? 4 : 8;
  const RowShape rs = init_shape(width, vb);
  const uint64_t total = rows * rs.units;
  const uint64_t nvwg = (total + kInitChunk - 1) / kInitChunk;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(nvwg, 65536);
  return with_init_type(dtype, init_vec(param, width, vb), [&](auto z, auto vec) {
    using T = decltype(z);
    k_row_init_range<T, decltype(vec)::value>
        <<<grid, kBlock, 0, st>>>(r, static_cast<T*>(param), key_begin, total, width, rs.units);
  });
}

hipError_t launch_row_init_new(int dtype, const InitRule& r, void* param, const SparseIndex& x, uint32_t* mark,
                               uint32_t width, uint64_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const int vb = dtype == 1 ? 4 : 8;
  const RowShape rs = init_shape(width, vb);
  const uint64_t G = (uint64_t)kBlock >> rs.lshift;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + G - 1) / G, kInitGridCap);
  return with_init_type(dtype, init_vec(param, width, vb), [&](auto z, auto vec) {
    using T = decltype(z);
    k_row_init_new<T, decltype(vec)::value><<<grid, kBlock, 0, st>>>(r, static_cast<T*>(param), x, mark, width, rs);
  });
}

hipError_t launch_init_eval(int dtype, const InitRule& r, const uint32_t* keys, uint64_t n, void* out, uint32_t width,
                            hipStream_t st) {
  if (n == 0) return hipSuccess;
  const int vb = dtype == 1 ? 4 : 8;
  const RowShape rs = init_shape(width, vb);
  const uint64_t G = (uint64_t)kBlock >> rs.lshift;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + G - 1) / G, kInitGridCap);
  return with_init_type(dtype, init_vec(out, width, vb), [&](auto z, auto vec) {
    using T = decltype(z);
    k_init_eval<T, decltype(vec)::value><<<grid, kBlock, 0, st>>>(r, keys, n, static_cast<T*>(out), width, rs);
  });
}

}  // namespace pskv
