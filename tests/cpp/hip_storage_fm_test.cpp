// hip_storage_fm_test.cpp — one matrix-factorisation step through HipStorage<Val>:
// SubGetPooledFm over the bags {user, item} (the predictions u . v), then
// SubApplyPooledFm with c = -(label - predict) under SGD with weight decay,
// against the host formula in long double from the rows before the step:
//   u' = u - lr (c v + beta u),   v' = v - lr (c u + beta v)   (u, not u')
// Bounds, u_r the unit roundoff: the prediction, the pull's at m = 2; a step,
// four roundings over at most 2 |c| (|u_j| + |v_j|) in the gradient element,
// four more over |g| + beta |p| in the rule, lr times that, and p' itself.
// Needs a GPU (run by tests/test_fm_gpu.py).
#include <cmath>
#include <cstdio>
#include <random>
#include <type_traits>
#include <vector>

#include "ps/hip_storage.hpp"

using namespace csci5570;

static int g_fail = 0, g_pass = 0;
#define EXPECT(cond) \
  ((cond) ? (void)++g_pass : (void)(++g_fail, std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond)))

template <typename V>
static void MfStep(const char* name, uint32_t width) {
  std::printf("[ RUN ] %s width %u\n", name, width);
  const uint32_t users = 40, items = 60, kb = 10, ke = kb + users + items;  // items behind the users, as mf.cpp keys them
  const double lr = 0.05, beta = 0.02;
  const long double ur = std::is_same<V, float>::value ? std::ldexp(1.0L, -24) : std::ldexp(1.0L, -53);
  HipStorage<V> s(0, kb, ke, PSKV_ASSIGN, 0, width);
  std::mt19937 rng(7 + width);
  std::vector<Key> all;
  std::vector<V> init;
  for (uint32_t key = kb; key < ke; ++key) {
    all.push_back(key);
    for (uint32_t j = 0; j < width; ++j) init.push_back((V)(((double)(rng() % 2001) - 1000.0) / 1000.0));
  }
  s.SubAdd(third_party::SArray<Key>(all), third_party::SArray<char>(third_party::SArray<V>(init)));
  pskv_optimizer opt{PSKV_OPT_SGD, lr, beta, 0.0, 0.0};
  pskv_check(pskv_shard_set_optimizer(s.shard(), &opt), "pskv_shard_set_optimizer");
  // one rating per user, every item at most once: the keys of the step are distinct
  const uint32_t nr = 30;
  std::vector<Key> keys;
  std::vector<uint64_t> off(1, 0);
  std::vector<V> label;
  for (uint32_t r = 0; r < nr; ++r) {
    keys.push_back(kb + r);
    keys.push_back(kb + users + (r * 7) % items);
    off.push_back(keys.size());
    label.push_back((V)(1 + rng() % 5));
  }
  third_party::SArray<Key> s_all(all), s_keys(keys);
  third_party::SArray<uint64_t> s_off(off);
  auto before = third_party::SArray<V>(s.SubGet(s_all));
  third_party::SArray<V> predict;
  auto sums = third_party::SArray<V>(s.SubGetPooledFm(s_keys, nullptr, s_off, &predict, /*want_sum=*/false));
  EXPECT(sums.size() == 0 && predict.size() == nr && before.size() == all.size() * width);
  if (predict.size() != nr || before.size() != all.size() * width) return;
  std::vector<V> c(nr);
  for (uint32_t r = 0; r < nr; ++r) {
    const V* u = &before[(size_t)(keys[2 * r] - kb) * width];
    const V* v = &before[(size_t)(keys[2 * r + 1] - kb) * width];
    long double dot = 0, mag = 0;
    for (uint32_t j = 0; j < width; ++j) {
      dot += (long double)u[j] * v[j];
      const long double a = std::fabs((long double)u[j]) + std::fabs((long double)v[j]);
      mag += a * a + (long double)u[j] * u[j] + (long double)v[j] * v[j];
    }
    EXPECT(std::fabs((long double)predict[r] - dot) <= 0.5L * 1.01L * (2 * 2 + width + 4) * ur * mag);
    c[r] = -(label[r] - predict[r]);
  }
  s.SubApplyPooledFm(s_keys, nullptr, s_off, third_party::SArray<V>(c));
  auto after = third_party::SArray<V>(s.SubGet(s_all));
  EXPECT(after.size() == before.size());
  if (after.size() != before.size()) return;
  std::vector<int> partner(all.size(), -1), rating(all.size(), -1);
  for (uint32_t r = 0; r < nr; ++r) {
    partner[keys[2 * r] - kb] = (int)(keys[2 * r + 1] - kb), partner[keys[2 * r + 1] - kb] = (int)(keys[2 * r] - kb);
    rating[keys[2 * r] - kb] = rating[keys[2 * r + 1] - kb] = (int)r;
  }
  for (size_t k = 0; k < all.size(); ++k)
    for (uint32_t j = 0; j < width; ++j) {
      const long double p = before[k * width + j], got = after[k * width + j];
      if (partner[k] < 0) {
        EXPECT(got == p);  // a key outside the step keeps its row
        continue;
      }
      const long double q = before[(size_t)partner[k] * width + j], cc = c[rating[k]];
      const long double g = cc * q, want = p - lr * (g + beta * p);
      const long double gerr = 4 * ur * 2 * std::fabs(cc) * (std::fabs(p) + std::fabs(q));
      const long double tol = 1.01L * (lr * (gerr + 4 * ur * (std::fabs(g) + beta * std::fabs(p))) + ur * std::fabs(want));
      EXPECT(std::fabs(got - want) <= tol);
    }
  uint64_t t = 0;
  EXPECT(pskv_get_step(s.shard(), &t) == PSKV_OK && t == 1);
  s.FinishIter();
}

int main() {
  for (uint32_t width : {1u, 8u, 10u}) {
    MfStep<float>("MfStepFloat", width);
    MfStep<double>("MfStepDouble", width);
  }
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
