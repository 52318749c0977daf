// pskv_matrix.hip — CDNA4 (gfx950) kernel of the score matrix pull
// (pskv_get_score_matrix; pskv.h "Score matrix pulls"):
//
//   k_row_score_matrix   out[b * out_stride + i] = queries[b] . row(keys[i]) for every query b and every key
//                        position i, on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64
//
// Work split (mat_split, pskv_plan.h).  A virtual workgroup (grid-stride) owns
// one window of kMatKeys = 64 key positions and one group of consecutive query
// blocks of kMatQueries = 64 queries.  Neighbouring workgroups share a window,
// so the groups of one window find its rows in L2.
//
// LDS (mat_lds, pskv_plan.h): the window's 64 rows, a block's 64 query rows
// one k-chunk (kMatChunk = 32 elements) at a time, and the window's row
// offsets.  While 64 padded rows fit kMatRowsLds the rows are gathered once per
// workgroup, in the 16-byte units of the other row kernels (RowShape), and
// stay for every query block; wider rows are gathered a k-chunk at a time,
// again for every block (from L2 after the first).  Dead positions (past n, or
// a key outside the range), dead queries (past nq) and the elements between
// the width and the next multiple of 4 are zeros in LDS: no lane ever loads
// outside keys[0, n), queries[0, nq * W) or the dense array.
//
// MFMA.  Wave w of the four owns queries 16w .. 16w + 15 of the block against
// all 64 keys: four 16 x 16 accumulator tiles.  Queries are the A operand,
// rows the B operand: lane l supplies element k0 + l / 16 of query 16w + l % 16
// and of row 16t + l % 16, so tile t's four accumulator values of lane l belong
// to key column 16t + l % 16 and the 16 lanes of a group hold 16 consecutive
// key positions of one query's row of `out` (64 or 128 contiguous bytes per
// store instruction and lane group).  The four tiles of a k-step are
// independent instructions; each waits only for its own tile's last k-step.
//
// The order of one score's sum: k ascending in steps of 4 from an accumulator
// of +0, each step one MFMA -- the same for every tile, lane, window, group,
// path and alignment; zero padding adds fma(0, 0, acc).  The bits of a score
// depend on the row, the query and the width alone.
#include <type_traits>

#include "pskv_internal.h"

namespace pskv {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kMatInFlight = 4;  // loads a thread issues before its first LDS store

__device__ __forceinline__ f32x4 mat_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f64x4 mat_mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// The query (of the wave's 16) that accumulator value r of a lane in group g
// belongs to: the f32 instruction keeps four consecutive rows per group, the
// f64 one rows 4 apart.
template <typename T>
__device__ __forceinline__ uint32_t mat_acc_row(uint32_t g, uint32_t r) {
  return std::is_same<T, float>::value ? 4u * g + r : 4u * r + g;
}

template <bool NT, typename T>
__device__ __forceinline__ void mat_store(T* p, T v) {
  if (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// `cnt` copies of UT from src(t) to dst(t), t = tid, tid + kBlock, ...,
// kMatInFlight loads in flight; src returns null for a zero.
template <typename UT, typename Src, typename Dst>
__device__ __forceinline__ void mat_copy(uint32_t tid, uint32_t cnt, Src&& src, Dst&& dst) {
  for (uint32_t t0 = tid; t0 < cnt; t0 += kMatInFlight * kBlock) {
    UT v[kMatInFlight];
#pragma unroll
    for (int j = 0; j < kMatInFlight; ++j) {
      const uint32_t t = t0 + (uint32_t)j * kBlock;
      const UT* p = t < cnt ? src(t) : nullptr;
      v[j] = p ? *p : UT{};
    }
#pragma unroll
    for (int j = 0; j < kMatInFlight; ++j) {
      const uint32_t t = t0 + (uint32_t)j * kBlock;
      if (t < cnt) *dst(t) = v[j];
    }
  }
}

template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void k_row_score_matrix(ScoreMatArgs a, DenseView d, uint32_t* err, RowShape rs,
                                                             MatSplit ms, MatLds ml) {
  typedef typename std::conditional<std::is_same<T, float>::value, f32x4, f64x4>::type acc_t;
  constexpr uint32_t V16 = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char mat_lds_bytes[];
  T* const rowsL = reinterpret_cast<T*>(mat_lds_bytes);
  T* const qL = rowsL + kMatKeys * ml.rstride;
  uint32_t* const koff = reinterpret_cast<uint32_t*>(qL + kMatQueries * ml.qstride);  // [64] offsets, [64] in-range flags
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6, l16 = tid & 15u, grp = (tid >> 4) & 3u;
  const uint32_t U = rs.units;
  const uint32_t V = rs.unit_bytes / (uint32_t)sizeof(T);  // elements of a unit: 1 or V16
  const uint32_t W = U * V;
  const uint32_t rstride = ml.rstride, qstride = ml.qstride;
  const bool resident = ml.resident != 0;
  const T* __restrict__ param = reinterpret_cast<const T*>(d.param);
  const T* __restrict__ queries = reinterpret_cast<const T*>(a.queries);
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  // 16-byte query loads: every row of every chunk then starts on a 16-byte boundary
  const bool qvec = (reinterpret_cast<uintptr_t>(queries) & 15u) == 0 && (W % V16) == 0;

  // rows [k0, k0 + k4) of the window -> columns [0, k4) of rowsL (k0, k4 multiples of 4)
  auto gather = [&](uint32_t k0, uint32_t k4) {
    const uint32_t cu = k4 / V, u0 = k0 / V;  // units of the piece, its first unit
    auto dst_col = [&](uint32_t t) { return (t / cu) * rstride + (t % cu) * V; };
    if (rs.unit_bytes == 16) {
      const u32x4* __restrict__ pu = reinterpret_cast<const u32x4*>(param);
      mat_copy<u32x4>(
          tid, kMatKeys * cu,
          [&](uint32_t t) -> const u32x4* {
            const uint32_t r = t / cu, u = u0 + t % cu;
            return (koff[kMatKeys + r] && u < U) ? pu + ((uint64_t)koff[r] * U + u) : nullptr;
          },
          [&](uint32_t t) { return reinterpret_cast<u32x4*>(rowsL + dst_col(t)); });
    } else {
      mat_copy<T>(
          tid, kMatKeys * cu,
          [&](uint32_t t) -> const T* {
            const uint32_t r = t / cu, u = u0 + t % cu;
            return (koff[kMatKeys + r] && u < U) ? param + ((uint64_t)koff[r] * U + u) : nullptr;
          },
          [&](uint32_t t) { return rowsL + dst_col(t); });
    }
  };
  // elements [k0, k0 + kc) of the block's queries -> columns [0, k4) of qL, zeros from kc on
  auto stage = [&](uint64_t q0, uint32_t k0, uint32_t kc, uint32_t k4) {
    if (qvec) {
      typedef T vt __attribute__((ext_vector_type(V16)));
      const uint32_t cv = k4 / V16;
      mat_copy<vt>(
          tid, kMatQueries * cv,
          [&](uint32_t t) -> const vt* {
            const uint32_t r = t / cv, c = (t % cv) * V16;
            return (q0 + r < a.nq && c < kc) ? reinterpret_cast<const vt*>(queries + ((q0 + r) * W + k0 + c)) : nullptr;
          },
          [&](uint32_t t) { return reinterpret_cast<vt*>(qL + (t / cv) * qstride + (t % cv) * V16); });
    } else {
      mat_copy<T>(
          tid, kMatQueries * k4,
          [&](uint32_t t) -> const T* {
            const uint32_t r = t / k4, c = t % k4;
            return (q0 + r < a.nq && c < kc) ? queries + ((q0 + r) * W + k0 + c) : nullptr;
          },
          [&](uint32_t t) { return qL + (t / k4) * qstride + t % k4; });
    }
  };

  const uint64_t nvwg = ms.nwin * ms.groups;
  for (uint64_t vwg = blockIdx.x; vwg < nvwg; vwg += gridDim.x) {
    const uint64_t win = vwg / ms.groups, qg = vwg - win * ms.groups;
    const uint64_t wb = win * kMatKeys;
    const uint64_t qb0 = qg * ms.per, qb1 = qb0 + ms.per < ms.nqb ? qb0 + ms.per : ms.nqb;
    __syncthreads();  // the last window's rows and offsets are read
    if (tid < kMatKeys) {
      const bool live = wb + tid < a.n;
      const uint32_t ko = (live ? a.keys[wb + tid] : 0u) - d.key_begin;
      const bool in = live && (uint64_t)ko < d.range;
      koff[tid] = ko;
      koff[kMatKeys + tid] = in;
      if (live && !in) atomicOr(err, kErrRowOutOfRange);
    }
    __syncthreads();
    if (resident) gather(0, (W + 3u) & ~3u);
    for (uint64_t qb = qb0; qb < qb1; ++qb) {
      const uint64_t q0 = qb * kMatQueries;
      acc_t acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
      for (uint32_t k0 = 0; k0 < W; k0 += kMatChunk) {
        const uint32_t kc = W - k0 < kMatChunk ? W - k0 : kMatChunk;
        const uint32_t k4 = (kc + 3u) & ~3u;
        __syncthreads();  // the last chunk is read
        if (!resident) gather(k0, k4);
        stage(q0, k0, kc, k4);
        __syncthreads();  // rows and queries of the chunk lie in LDS
        const T* ap = qL + (16u * wave + l16) * qstride + grp;
        const T* bp = rowsL + l16 * rstride + (resident ? k0 : 0u) + grp;
        for (uint32_t ks = 0; ks < k4; ks += 4) {
          const T qa = ap[ks];
          T rb[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) rb[t] = bp[(uint32_t)t * 16u * rstride + ks];
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = mat_mfma(qa, rb[t], acc[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint64_t key = wb + 16u * (uint32_t)t + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint64_t q = q0 + 16u * wave + mat_acc_row<T>(grp, (uint32_t)r);
          if (key < a.n && q < a.nq) mat_store<NT>(out + (q * a.out_stride + key), acc[t][r]);
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_row_score_matrix(int dtype, bool nt, const ScoreMatArgs& a, const DenseView& d, const Ovf& o,
                                   const RowShape& rs, hipStream_t st) {
  if (a.n == 0 || a.nq == 0) return hipSuccess;
  if (!a.keys || !a.queries || !a.out || a.out_stride < a.n || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  const int vb = dtype == 1 ? 4 : 8;
  const uint32_t width = rs.units * (rs.unit_bytes / (uint32_t)vb);
  const MatSplit ms = mat_split(a.n, a.nq);
  const MatLds ml = mat_lds(width, vb);
  const uint64_t nvwg = ms.nwin * ms.groups;
  const uint32_t grid = (uint32_t)(nvwg < (1u << 20) ? nvwg : (1u << 20));
  uint32_t* err = &o.c->stat[1];
  auto go = [&](auto kernel) {
    if (ml.bytes > 65536u) {  // past 64 KiB of dynamic LDS the runtime wants to be told
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)ml.bytes);
      if (e != hipSuccess) return e;
    }
    kernel<<<grid, kBlock, ml.bytes, st>>>(a, d, err, rs, ms, ml);
    return hipGetLastError();
  };
  if (dtype == 1) return nt ? go(k_row_score_matrix<float, true>) : go(k_row_score_matrix<float, false>);
  return nt ? go(k_row_score_matrix<double, true>) : go(k_row_score_matrix<double, false>);
}

}  // namespace pskv
