// hip_storage_scores_test.cpp — HipStorage<Val>::SubGetScores against a host
// loop in long double: a candidate list (one bag), an empty bag, then bags of
// one.  Once as the method's host call, once as a device call of
// pskv_get_scores on frames (page-locked and mapped: read and written in place).
// Bound: |got - ref| <= gamma_W * sum_j |q_j p_j|, gamma_W = W u / (1 - W u).
// Needs a GPU (run by tests/test_scores_gpu.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <type_traits>
#include <vector>

#include "ps/hip_storage.hpp"

using namespace csci5570;

static int g_fail = 0, g_pass = 0;
#define EXPECT(cond) \
  ((cond) ? (void)++g_pass : (void)(++g_fail, std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond)))

template <typename V>
static void Scores(const char* name, uint32_t width) {
  std::printf("[ RUN ] %s width %u\n", name, width);
  const uint32_t rows = 50, kb = 10, ke = kb + rows, cand = 37, pairs = 9;
  const long double ur = std::is_same<V, float>::value ? std::ldexp(1.0L, -24) : std::ldexp(1.0L, -53);
  HipStorage<V> s(0, kb, ke, PSKV_ASSIGN, 0, width);
  std::mt19937 rng(11 + width);
  auto draw = [&] { return (V)(((double)(rng() % 2001) - 1000.0) / 1000.0); };
  std::vector<Key> all;
  std::vector<V> init;
  for (uint32_t key = kb; key < ke - 1; ++key) {  // the last key is never written: a row of zeros
    all.push_back(key);
    for (uint32_t j = 0; j < width; ++j) init.push_back(draw());
  }
  s.SubAdd(third_party::SArray<Key>(all), third_party::SArray<char>(third_party::SArray<V>(init)));
  init.resize((size_t)rows * width, (V)0);
  std::vector<Key> keys;
  std::vector<uint64_t> off(1, 0);
  for (uint32_t i = 0; i < cand; ++i) keys.push_back(kb + (i * 7) % rows);
  off.push_back(keys.size());
  off.push_back(keys.size());  // an empty bag
  for (uint32_t i = 0; i < pairs; ++i) {
    keys.push_back(ke - 1 - i);
    off.push_back(keys.size());
  }
  const size_t nbags = off.size() - 1;
  std::vector<V> q(nbags * width);
  for (auto& x : q) x = draw();
  auto got = third_party::SArray<V>(s.SubGetScores(third_party::SArray<Key>(keys), third_party::SArray<uint64_t>(off),
                                                   third_party::SArray<V>(q)));
  EXPECT(got.size() == keys.size());
  if (got.size() != keys.size()) return;
  auto d_keys = FrameArray<Key>(keys.size());
  auto d_off = FrameArray<uint64_t>(off.size());
  auto d_q = FrameArray<V>(q.size());
  auto d_out = FrameArray<V>(keys.size());
  std::memcpy(d_keys.data(), keys.data(), keys.size() * sizeof(Key));
  std::memcpy(d_off.data(), off.data(), off.size() * sizeof(uint64_t));
  std::memcpy(d_q.data(), q.data(), q.size() * sizeof(V));
  pskv_check(pskv_get_scores(s.shard(), d_keys.data(), keys.size(), d_q.data(), d_off.data(), nbags, d_out.data(),
                             PSKV_DEVICE),
             "pskv_get_scores");
  pskv_check(pskv_sync(s.shard()), "pskv_sync");
  EXPECT(std::memcmp(d_out.data(), got.data(), keys.size() * sizeof(V)) == 0);
  size_t bag = 0;
  for (size_t i = 0; i < keys.size(); ++i) {
    while (off[bag + 1] <= i) ++bag;
    const V* p = &init[(size_t)(keys[i] - kb) * width];
    long double dot = 0, mag = 0;
    for (uint32_t j = 0; j < width; ++j) {
      dot += (long double)q[bag * width + j] * p[j];
      mag += std::fabs((long double)q[bag * width + j] * p[j]);
    }
    const long double gamma = width * ur / (1 - width * ur);
    EXPECT(std::fabs((long double)got[i] - dot) <= gamma * mag);
    if (keys[i] == ke - 1) EXPECT(got[i] == 0 && !std::signbit(got[i]));
  }
  s.FinishIter();
}

int main() {
  for (uint32_t width : {1u, 8u, 10u, 100u}) {
    Scores<float>("ScoresFloat", width);
    Scores<double>("ScoresDouble", width);
  }
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
