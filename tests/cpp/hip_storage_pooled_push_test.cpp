// hip_storage_pooled_push_test.cpp — one training step as two calls through
// HipStorage<Val> with an Adagrad optimizer: SubGetPooled (the margins), then
// SubApplyPooled (one gradient row per bag), then SubGet, against a loop
// written out here in long double from the rows SubGet returned before the step.
//
//   g[k]  = sum over the occurrences i of key k of x_i * err[bag(i)]
//   h'    = h + g g            (h = init_accum before the first step)
//   p'    = p - lr g / (sqrt(h') + eps)
// Bound per element, m the occurrences of the key, G = sum |x_i err|, u the
// unit roundoff (tests/pooled_push_util.py: opt_util's Adagrad tolerance with
// m + 1 for m, one more rounding per term):
//   dd = 1.01 (m + 4) u G
//   |p_got - p'| <= 1.01 u |p'| + lr (dd / (sqrt(h + max(|g| - dd, 0)^2) + eps) + 8 * 1.01 u |g| / (sqrt(h') + eps))
// Keys outside the call keep their bits.
//
// Needs a GPU (run by tests/test_pooled_push_gpu.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
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
  return (V)(((double)(rng() % 20001) - 10000.0) / 1000.0);
}

template <typename V>
static void Step(const char* name, uint32_t width, bool weighted) {
  std::printf("[ RUN ] %s width %u weighted %d\n", name, width, (int)weighted);
  const uint32_t kb = 100, ke = 1100;
  const double lr = 0.05, eps = 1e-8, h0 = 0.1;
  pskv_optimizer opt{PSKV_OPT_ADAGRAD, lr, 0.0, eps, h0};
  HipStorage<V> s(0, kb, ke, PSKV_ASSIGN, 0, width);
  std::mt19937 rng(29 + width);
  std::vector<Key> all;
  {
    std::vector<V> v;
    for (uint32_t key = kb; key < ke; ++key) {
      all.push_back(key);
      for (uint32_t j = 0; j < width; ++j) v.push_back(Draw<V>(rng));
    }
    s.SubAdd(third_party::SArray<Key>(all), third_party::SArray<char>(third_party::SArray<V>(v)));
  }
  pskv_check(pskv_shard_set_optimizer(s.shard(), &opt), "pskv_shard_set_optimizer");
  const std::vector<uint64_t> lens = {0, 1, 5, 300, 0, 4, 2, 0};
  std::vector<uint64_t> off(1, 0);
  std::vector<Key> keys;
  for (uint64_t m : lens) {
    for (uint64_t i = 0; i < m; ++i) keys.push_back(i % 3 == 2 ? keys.back() : kb + rng() % (ke - kb));
    off.push_back(keys.size());
  }
  keys[1] = kb;
  keys[2] = ke - 1;
  std::vector<V> x;
  for (size_t i = 0; i < keys.size(); ++i) x.push_back(Draw<V>(rng));
  third_party::SArray<Key> s_all(all), s_keys(keys);
  third_party::SArray<V> s_x(x);
  third_party::SArray<uint64_t> s_off(off);
  auto before = third_party::SArray<V>(s.SubGet(s_all));
  // forward: one pooled row per bag; backward: err = tanh(margin) - 0.25 per element
  auto margins = third_party::SArray<V>(s.SubGetPooled(s_keys, weighted ? &s_x : nullptr, s_off));
  EXPECT(margins.size() == lens.size() * width);
  std::vector<V> err(lens.size() * width);
  for (size_t i = 0; i < err.size() && i < margins.size(); ++i) err[i] = (V)(std::tanh((double)margins[i]) - 0.25);
  third_party::SArray<V> s_err(err);
  s.SubApplyPooled(s_keys, weighted ? &s_x : nullptr, s_off, s_err);
  auto after = third_party::SArray<V>(s.SubGet(s_all));
  uint64_t t = 0;
  EXPECT(pskv_get_step(s.shard(), &t) == PSKV_OK && t == 1);
  EXPECT(before.size() == all.size() * width && after.size() == before.size());
  if (before.size() != all.size() * width || after.size() != before.size()) return;
  // the loop, per key and column
  const double u = std::is_same<V, float>::value ? std::ldexp(1.0, -24) : std::ldexp(1.0, -53);
  std::map<Key, std::vector<size_t>> occ;
  for (size_t b = 0; b < lens.size(); ++b)
    for (uint64_t i = off[b]; i < off[b + 1]; ++i) occ[keys[i]].push_back(i);
  std::vector<size_t> bag_of(keys.size());
  for (size_t b = 0; b < lens.size(); ++b)
    for (uint64_t i = off[b]; i < off[b + 1]; ++i) bag_of[i] = b;
  for (uint32_t key = kb; key < ke; ++key) {
    const size_t row = (size_t)(key - kb) * width;
    auto it = occ.find(key);
    for (uint32_t j = 0; j < width; ++j) {
      const V p0 = before[row + j], got = after[row + j];
      if (it == occ.end()) {
        EXPECT(std::memcmp(&p0, &got, sizeof(V)) == 0);
        continue;
      }
      long double g = 0, G = 0;
      for (size_t i : it->second) {
        const long double term = (weighted ? (long double)x[i] : 1.0L) * (long double)err[bag_of[i] * width + j];
        g += term;
        G += std::fabs(term);
      }
      const long double m = (long double)it->second.size();
      const long double hn = h0 + g * g;
      const long double pn = (long double)p0 - lr * g / (std::sqrt(hn) + eps);
      const long double dd = 1.01L * (m + 4) * u * G;
      const long double lo = std::max(std::fabs(g) - dd, (long double)0);
      const long double tol = 1.01 * u * std::fabs(pn) +
                         lr * (dd / (std::sqrt(h0 + lo * lo) + eps) + 8 * 1.01 * u * std::fabs(g) / (std::sqrt(hn) + eps));
      EXPECT(std::fabs((long double)got - pn) <= tol);
    }
  }
  s.FinishIter();
}

int main() {
  for (uint32_t width : {1u, 4u, 5u})
    for (int weighted = 0; weighted < 2; ++weighted) {
      Step<float>("PooledPushFloat", width, weighted != 0);
      Step<double>("PooledPushDouble", width, weighted != 0);
    }
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
