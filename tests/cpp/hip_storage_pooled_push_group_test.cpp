// hip_storage_pooled_push_group_test.cpp — a BSP server's flush of two
// workers' pooled pushes as ONE optimizer step, through HipStorage<Val> with
// an Adagrad optimizer: SubApplyPooledGrouped on one storage, and on a twin
// the same two pushes expanded on the host (rows fl(x_i * err[bag(i)]), one
// rounding each) and applied as one AddGrouped.  The two workers' keys are
// distinct over the whole call, so p must be equal bit for bit (pskv.h
// "Grouped pooled pushes"), Adagrad's h too, and the step counter stands at 1
// on both.  A third storage takes the two pushes one by one: its counter
// stands at 2, what the grouped call is there to avoid.
//
// Needs a GPU (run by tests/test_pooled_push_grouped_gpu.py).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
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
struct Worker {
  std::vector<Key> keys;
  std::vector<V> x;
  std::vector<uint64_t> off;
  std::vector<V> err;
};

template <typename V>
static void Flush(const char* name, uint32_t width, bool weighted) {
  std::printf("[ RUN ] %s width %u weighted %d\n", name, width, (int)weighted);
  const uint32_t kb = 100, ke = 5100;
  pskv_optimizer opt{PSKV_OPT_ADAGRAD, 0.05, 0.01, 1e-8, 0.1};
  // (constructed with the optimizer: AddGrouped is then pskv_apply_grouped, one step)
  HipStorage<V> grouped(0, kb, ke, PSKV_ASSIGN, 0, width, &opt), twin(0, kb, ke, PSKV_ASSIGN, 0, width, &opt),
      serial(0, kb, ke, PSKV_ASSIGN, 0, width, &opt);
  std::mt19937 rng(41 + width);
  std::vector<Key> all;
  std::vector<V> p0;
  for (uint32_t key = kb; key < ke; ++key) {
    all.push_back(key);
    for (uint32_t j = 0; j < width; ++j) p0.push_back(Draw<V>(rng));
  }
  third_party::SArray<Key> s_all(all);
  for (HipStorage<V>* s : {&grouped, &twin, &serial})  // the parameters: a plain Add (SubAdd would be a step)
    pskv_check(pskv_add(s->shard(), all.data(), p0.data(), all.size(), PSKV_HOST), "pskv_add");
  // two workers; their keys are distinct over both: a shuffle of the range, dealt out
  std::vector<Key> deck(all);
  std::shuffle(deck.begin(), deck.end(), rng);
  const std::vector<std::vector<uint64_t>> lens = {{0, 1, 5, 2100, 0, 4, 2, 0}, {300, 0, 1, 17}};
  std::vector<Worker<V>> workers(2);
  size_t dealt = 0;
  for (size_t wk = 0; wk < 2; ++wk) {
    Worker<V>& w = workers[wk];
    w.off.push_back(0);
    for (uint64_t m : lens[wk]) {
      for (uint64_t i = 0; i < m; ++i) w.keys.push_back(deck[dealt++]);
      w.off.push_back(w.keys.size());
    }
    for (size_t i = 0; i < w.keys.size(); ++i) w.x.push_back(Draw<V>(rng));
    for (size_t i = 0; i < lens[wk].size() * width; ++i) w.err.push_back(Draw<V>(rng));
  }
  // the grouped flush
  std::vector<third_party::SArray<V>> s_x;
  for (const Worker<V>& w : workers) s_x.emplace_back(w.x);
  std::vector<typename HipStorage<V>::PooledPush> pushes;
  for (size_t wk = 0; wk < 2; ++wk) {
    const Worker<V>& w = workers[wk];
    pushes.push_back(typename HipStorage<V>::PooledPush{third_party::SArray<Key>(w.keys),
                                                        weighted ? s_x[wk] : third_party::SArray<V>(), weighted,
                                                        third_party::SArray<uint64_t>(w.off),
                                                        third_party::SArray<V>(w.err)});
  }
  grouped.SubApplyPooledGrouped(pushes);
  // the twin: the expanded rows of both workers as one AddGrouped
  std::vector<Message> msgs(2);
  for (size_t wk = 0; wk < 2; ++wk) {
    const Worker<V>& w = workers[wk];
    std::vector<V> rows;
    for (size_t b = 0; b + 1 < w.off.size(); ++b)
      for (uint64_t i = w.off[b]; i < w.off[b + 1]; ++i)
        for (uint32_t j = 0; j < width; ++j) {
          const V e = w.err[b * width + j];
          rows.push_back(weighted ? (V)(w.x[i] * e) : e);  // one multiplication rounded to V
        }
    msgs[wk].AddData(third_party::SArray<Key>(w.keys));
    msgs[wk].AddData(third_party::SArray<V>(rows));
  }
  twin.AddGrouped(msgs);
  // one by one: two steps
  for (size_t wk = 0; wk < 2; ++wk)
    serial.SubApplyPooled(pushes[wk].keys, weighted ? &pushes[wk].weights : nullptr, pushes[wk].offsets,
                          pushes[wk].bag_grads);
  uint64_t tg = 0, tt = 0, ts = 0;
  EXPECT(pskv_get_step(grouped.shard(), &tg) == PSKV_OK && tg == 1);
  EXPECT(pskv_get_step(twin.shard(), &tt) == PSKV_OK && tt == 1);
  EXPECT(pskv_get_step(serial.shard(), &ts) == PSKV_OK && ts == 2);
  auto got = third_party::SArray<V>(grouped.SubGet(s_all));
  auto want = third_party::SArray<V>(twin.SubGet(s_all));
  EXPECT(got.size() == p0.size() && want.size() == p0.size());
  if (got.size() != p0.size() || want.size() != p0.size()) return;
  size_t differ = 0, moved = 0;
  for (size_t i = 0; i < p0.size(); ++i) {
    differ += std::memcmp(&got[i], &want[i], sizeof(V)) != 0;
    moved += std::memcmp(&got[i], &p0[i], sizeof(V)) != 0;
  }
  EXPECT(differ == 0);
  // the keys of the call moved, the others kept their bits (weight decay alone moves a key with a zero term)
  std::vector<char> in_call(ke - kb, 0);
  for (const Worker<V>& w : workers)
    for (Key k : w.keys) in_call[k - kb] = 1;
  size_t kept = 0, outside = 0;
  for (uint32_t key = kb; key < ke; ++key) {
    if (in_call[key - kb]) continue;
    ++outside;
    kept += std::memcmp(&got[(size_t)(key - kb) * width], &p0[(size_t)(key - kb) * width], sizeof(V) * width) == 0;
  }
  EXPECT(kept == outside && outside > 0);
  EXPECT(moved > 0);
  // the optimizer state too: Adagrad's h through pskv_get_state
  std::vector<V> hg(p0.size()), ht(p0.size());
  EXPECT(pskv_get_state(grouped.shard(), all.data(), all.size(), hg.data(), PSKV_HOST) == PSKV_OK);
  EXPECT(pskv_get_state(twin.shard(), all.data(), all.size(), ht.data(), PSKV_HOST) == PSKV_OK);
  EXPECT(std::memcmp(hg.data(), ht.data(), hg.size() * sizeof(V)) == 0);
  for (HipStorage<V>* s : {&grouped, &twin, &serial}) s->FinishIter();
}

int main() {
  for (uint32_t width : {1u, 4u, 5u})
    for (int weighted = 0; weighted < 2; ++weighted) {
      Flush<float>("PooledPushGroupFloat", width, weighted != 0);
      Flush<double>("PooledPushGroupDouble", width, weighted != 0);
    }
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
