// hip_storage_pooled_test.cpp — HipStorage<Val>::SubGetPooled against SubGet of
// the same keys plus a host sum, for float, double and int.
//
//   float / double   |pooled - ref64| <= 1.01 (m + 1) u sum|w_i||p_i| per element
//                    (m the bag's length, u the unit roundoff: the accumulate
//                    bound, which holds for any order of the additions)
//   int              exact, two's complement with wrap
// Bags: empty ones, one key, a few keys, one longer than the kernel's chunk of
// 256 keys; keys repeat; weighted and with null weights.
//
// Needs a GPU (run by tests/test_pooled_gpu.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <type_traits>
#include <vector>

#include "ps/hip_storage.hpp"

using namespace csci5570;

static int g_fail = 0, g_pass = 0;
#define EXPECT(cond)                                                            \
  do {                                                                          \
    if (cond) {                                                                 \
      ++g_pass;                                                                 \
    } else {                                                                    \
      ++g_fail;                                                                 \
      std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);             \
    }                                                                           \
  } while (0)

template <typename V>
static V Draw(std::mt19937& rng) {
  if (std::is_same<V, int>::value) return (V)(int32_t)rng();
  return (V)(((double)(rng() % 20001) - 10000.0) / 1000.0);
}

template <typename V>
static void Pooled(const char* name, uint32_t width) {
  std::printf("[ RUN ] %s width %u\n", name, width);
  const uint32_t kb = 100, ke = 1100;
  HipStorage<V> s(0, kb, ke, PSKV_ASSIGN, 0, width);
  std::mt19937 rng(17 + width);
  {
    std::vector<Key> k;
    std::vector<V> v;
    for (uint32_t key = kb; key < ke; ++key) {
      k.push_back(key);
      for (uint32_t j = 0; j < width; ++j) v.push_back(Draw<V>(rng));
    }
    s.SubAdd(third_party::SArray<Key>(k), third_party::SArray<char>(third_party::SArray<V>(v)));
  }
  const std::vector<uint64_t> lens = {0, 1, 5, 300, 0, 4, 2, 0};
  std::vector<uint64_t> off(1, 0);
  std::vector<Key> keys;
  for (uint64_t m : lens) {
    for (uint64_t i = 0; i < m; ++i) keys.push_back(i % 3 == 2 ? keys.back() : kb + rng() % (ke - kb));
    off.push_back(keys.size());
  }
  keys[1] = kb;
  keys[2] = ke - 1;
  std::vector<V> wts;
  for (size_t i = 0; i < keys.size(); ++i) wts.push_back(Draw<V>(rng));
  third_party::SArray<Key> s_keys(keys);
  third_party::SArray<V> s_wts(wts);
  third_party::SArray<uint64_t> s_off(off);
  auto rows = third_party::SArray<V>(s.SubGet(s_keys));
  EXPECT(rows.size() == keys.size() * width);
  const double u = std::is_same<V, float>::value ? std::ldexp(1.0, -24) : std::ldexp(1.0, -53);
  for (int weighted = 0; weighted < 2; ++weighted) {
    auto got = third_party::SArray<V>(s.SubGetPooled(s_keys, weighted ? &s_wts : nullptr, s_off));
    EXPECT(got.size() == lens.size() * width);
    if (got.size() != lens.size() * width || rows.size() != keys.size() * width) continue;
    for (size_t b = 0; b < lens.size(); ++b)
      for (uint32_t j = 0; j < width; ++j) {
        const V g = got[b * width + j];
        if (std::is_same<V, int>::value) {
          uint32_t want = 0;
          for (uint64_t i = off[b]; i < off[b + 1]; ++i)
            want += (uint32_t)rows[i * width + j] * (weighted ? (uint32_t)wts[i] : 1u);
          EXPECT((uint32_t)g == want);
        } else {
          double ref = 0, mag = 0;
          for (uint64_t i = off[b]; i < off[b + 1]; ++i) {
            const double t = (double)rows[i * width + j] * (weighted ? (double)wts[i] : 1.0);
            ref += t;
            mag += std::fabs(t);
          }
          EXPECT(std::fabs((double)g - ref) <= 1.01 * (double)(lens[b] + 1) * u * mag);
        }
      }
  }
  s.FinishIter();
}

int main() {
  for (uint32_t width : {1u, 4u, 5u}) {
    Pooled<float>("PooledFloat", width);
    Pooled<double>("PooledDouble", width);
    Pooled<int>("PooledInt", width);
  }
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
