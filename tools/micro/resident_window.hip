// resident_window.hip — does a cache-sized window of the parameters stay in the
// 256 MiB Infinity Cache across steps while everything else streams past it?
// (DESIGN.md §7 "Resident window": the measurement behind option RESIDENT_BYTES.)
//
// One loop "step" is two launches, shaped like the dense step's K2g and K1
// (256-thread workgroups, one 32 KiB chunk each, 16 bytes per lane, 8 accesses
// per lane in flight).  Between them they
//   write  the window, R bytes at the start of a 400 MiB parameter array
//          (launch 1), and read it back (launch 2), under the policy swept;
//   move   400 MiB - R bytes of "outside" parameter traffic, non-temporal:
//          one half of the rest of the array written in launch 1, the other
//          half read in launch 2, the halves swapping every step;
//   move   S = 860 MB of non-temporal copy streams (read one chunk, write
//          another) that are never reused: chunks of a 16 GiB pool taken in
//          turn, so a chunk recurs only after 16 GiB of other traffic.
// The three kinds of chunk are interleaved over each launch's workgroups.
//
// Sweep: R in {0, 128, 160, 192, 224, 256 MiB} x the window's policy
//   plain/plain   plain stores, plain loads        (the resident window)
//   nt-st/plain   non-temporal stores, plain loads (today's NTP = 1)
//   nt/nt         everything non-temporal          (nothing may stay)
// Output: time per step (median) and effective TB/s over every byte moved
// (2 R + 400 MiB - R + S).  If dirty lines written with plain stores stay in
// the cache and non-temporal traffic does not displace them, plain/plain gets
// faster with R up to the cache's capacity and the other two do not.
// Not part of libpskv: a measurement.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/micro/resident_window.hip -o tools/micro/resident_window
//   tools/micro/resident_window [steps=30]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

namespace {

constexpr int kBlock = 256;
constexpr int U = 8;
constexpr uint64_t CH = kBlock * 4 * U;  // elements per chunk
constexpr uint64_t CHB = CH * 4;         // bytes per chunk (32 KiB)
constexpr uint32_t kWindow = 0, kOutside = 1, kStream = 2;  // a work item: kind << 30 | index
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ u32x4 ld(const uint32_t* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return *reinterpret_cast<const u32x4*>(p);
}
template <bool NT>
__device__ __forceinline__ void st(uint32_t* p, u32x4 v) {
  if (NT)
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  else
    *reinterpret_cast<u32x4*>(p) = v;
}

struct Step {
  uint32_t* param;       // the parameter array
  uint32_t* pool;        // the stream pool, npool chunks
  const uint32_t* work;  // one item per workgroup
  uint64_t npool;        // even
  uint64_t cursor;       // this launch's first pool chunk (even)
  uint64_t outside0;     // first chunk of the outside half this launch works on
};

template <bool NT, bool WRITE>
__device__ __forceinline__ void chunk(uint32_t* c, uint32_t* sink) {
  const uint64_t o = (uint64_t)threadIdx.x * 4;
  if (WRITE) {
    const u32x4 v = {blockIdx.x, threadIdx.x, 0x9e3779b9u, 1u};
#pragma unroll
    for (int u = 0; u < U; ++u) st<NT>(c + o + (uint64_t)u * kBlock * 4, v);
  } else {
    u32x4 v[U], s = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld<NT>(c + o + (uint64_t)u * kBlock * 4);
#pragma unroll
    for (int u = 0; u < U; ++u) s ^= v[u];
    if ((s.x ^ s.y ^ s.z ^ s.w) == 0x12345678u) sink[blockIdx.x & 1023u] = s.x;  // never in practice
  }
}

// NTW: the window's accesses are non-temporal.  WRITE: launch 1 (stores to the
// parameters), else launch 2 (loads).
template <bool NTW, bool WRITE>
__global__ __launch_bounds__(kBlock) void k_step(Step a, uint32_t* sink) {
  const uint32_t w = a.work[blockIdx.x];
  const uint32_t kind = w >> 30;
  const uint64_t idx = w & 0x3FFFFFFFu;
  if (kind == kWindow) {
    chunk<NTW, WRITE>(a.param + idx * CH, sink);
  } else if (kind == kOutside) {
    chunk<true, WRITE>(a.param + (a.outside0 + idx) * CH, sink);
  } else {
    const uint32_t* src = a.pool + ((a.cursor + 2 * idx) % a.npool) * CH;
    uint32_t* dst = a.pool + ((a.cursor + 2 * idx + 1) % a.npool) * CH;
    const uint64_t o = (uint64_t)threadIdx.x * 4;
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld<true>(src + o + (uint64_t)u * kBlock * 4);
#pragma unroll
    for (int u = 0; u < U; ++u) st<true>(dst + o + (uint64_t)u * kBlock * 4, v[u]);
  }
}

// n_w window chunks, n_o outside chunks and n_s stream pairs, evenly interleaved
std::vector<uint32_t> interleave(uint64_t n_w, uint64_t n_o, uint64_t n_s) {
  std::vector<std::pair<double, uint32_t>> it;
  const uint64_t n[3] = {n_w, n_o, n_s};
  for (uint32_t k = 0; k < 3; ++k)
    for (uint64_t i = 0; i < n[k]; ++i) it.push_back({(i + 0.5) / (double)n[k], (k << 30) | (uint32_t)i});
  std::sort(it.begin(), it.end());
  std::vector<uint32_t> out;
  for (const auto& p : it) out.push_back(p.second);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 30;
  const int warm = 4;  // steps before the timed ones (the window has to get into the cache first)
  const uint64_t MiB = 1ull << 20;
  const uint64_t param_bytes = 400 * MiB;
  const uint64_t pool_bytes = 16ull << 30;
  const uint64_t stream_bytes = 860000000ull;
  const uint64_t npool = pool_bytes / CHB;                  // even
  const uint64_t pairs = stream_bytes / (2 * CHB) / 2;      // copy pairs per launch
  uint32_t *param = nullptr, *pool = nullptr, *sink = nullptr, *work = nullptr;
  CHECK(hipMalloc(&param, param_bytes));
  CHECK(hipMalloc(&pool, pool_bytes));
  CHECK(hipMalloc(&sink, 4096));
  CHECK(hipMemset(param, 0, param_bytes));
  CHECK(hipMemset(pool, 0, pool_bytes));
  CHECK(hipMemset(sink, 0, 4096));
  const uint64_t max_items = param_bytes / CHB + pairs;
  CHECK(hipMalloc(&work, max_items * 4));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  uint64_t cursor = 0;
  std::printf("%-8s %-12s %10s %10s %9s\n", "R MiB", "policy", "us/step", "bytes MB", "TB/s");
  const uint64_t sweep[] = {0, 128, 160, 192, 224, 256};
  const char* const pol_name[3] = {"plain/plain", "nt-st/plain", "nt/nt"};
  for (uint64_t r_mib : sweep) {
    const uint64_t n_w = r_mib * MiB / CHB;
    const uint64_t n_o = (param_bytes / CHB - n_w) / 2;  // one outside half
    const std::vector<uint32_t> items = interleave(n_w, n_o, pairs);
    if (items.size() > max_items || n_w + 2 * n_o > param_bytes / CHB) {
      std::fprintf(stderr, "work list out of bounds\n");
      return 2;
    }
    CHECK(hipMemcpy(work, items.data(), items.size() * 4, hipMemcpyHostToDevice));
    const uint32_t grid = (uint32_t)items.size();
    const double bytes = (double)(2 * n_w + 2 * n_o + 4 * pairs) * CHB;
    for (int pol = 0; pol < 3; ++pol) {
      if (r_mib == 0 && pol) continue;  // no window: the policies are one
      std::vector<float> ms;
      for (int s = 0; s < warm + steps; ++s) {
        Step a{param, pool, work, npool, 0, 0};
        const uint64_t first = n_w + (s & 1 ? n_o : 0), second = n_w + (s & 1 ? 0 : n_o);
        CHECK(hipEventRecord(e0));
        a.cursor = cursor;
        a.outside0 = first;
        if (pol == 0)
          k_step<false, true><<<grid, kBlock>>>(a, sink);
        else
          k_step<true, true><<<grid, kBlock>>>(a, sink);
        cursor = (cursor + 2 * pairs) % npool;
        a.cursor = cursor;
        a.outside0 = second;
        if (pol == 2)
          k_step<true, false><<<grid, kBlock>>>(a, sink);
        else
          k_step<false, false><<<grid, kBlock>>>(a, sink);
        cursor = (cursor + 2 * pairs) % npool;
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float t = 0;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (s >= warm) ms.push_back(t);
      }
      CHECK(hipGetLastError());
      std::sort(ms.begin(), ms.end());
      const float med = ms[ms.size() / 2];
      std::printf("%-8llu %-12s %10.1f %10.1f %9.3f   (min %.1f max %.1f us)\n", (unsigned long long)r_mib,
                  pol_name[pol], med * 1e3, bytes / 1e6, bytes / (med * 1e-3) / 1e12, ms.front() * 1e3,
                  ms.back() * 1e3);
      std::fflush(stdout);
    }
  }
  CHECK(hipDeviceSynchronize());
  CHECK(hipFree(param));
  CHECK(hipFree(pool));
  CHECK(hipFree(sink));
  CHECK(hipFree(work));
  return 0;
}
