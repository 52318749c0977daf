// hip_storage_sparse_test.cpp — sparse storages behind consistent hashing:
// HipStorage<Val>::Sparse and CreateTable's sparse_capacity.
//
//   SparseAddGet        the reference's three-key storage case (server/
//                       map_storage_test.cpp:19-75) at width 4 on keys from the
//                       ends of the key space, held as std::unique_ptr<AbstractStorage>
//   SparseStep          HipStorage::Sparse with an optimizer: SubAdd is an SGD step,
//                       a new key starts from zeros
//   HashedSparseTable   two servers under jump hashing, sparse_capacity = 4096:
//                       4000 hashed ids pushed and pulled through the models; every
//                       storage ends up holding exactly the keys the hash sends it,
//                       its memory follows the capacity (not the 2^32-key space),
//                       and the replies are those of a std::map (the CPU map
//                       storage: last write wins, 0 for a key never written)
//
// Needs a GPU (run by tests/test_sparse_gpu.py).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "ps/storage_factory.hpp"

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

static void SparseAddGet() {
  std::printf("[ RUN ] SparseAddGet\n");
  const uint32_t W = 4;
  std::unique_ptr<AbstractStorage> s = HipStorage<float>::Sparse(0, 8, PSKV_ASSIGN, W);
  const std::vector<uint32_t> keys = {0xFFFFFFFFu, 0u, 0x80000000u};
  std::vector<float> vals;
  for (size_t i = 0; i < keys.size(); ++i)
    for (uint32_t j = 0; j < W; ++j) vals.push_back(float(i + 1) + float(j) / 8);
  Message m;
  m.AddData(third_party::SArray<Key>(keys));
  m.AddData(third_party::SArray<float>(vals));
  s->Add(m);
  Message g;
  g.AddData(third_party::SArray<Key>(std::vector<uint32_t>{0u, 77u, 0x80000000u, 0xFFFFFFFFu}));
  Message rep = s->Get(g);
  auto got = third_party::SArray<float>(rep.data[1]);
  EXPECT(got.size() == 4 * W);
  const int row_of[4] = {1, -1, 2, 0};  // 77 was never written: zeros
  for (size_t i = 0; i < 4 && got.size() == 4 * W; ++i)
    for (uint32_t j = 0; j < W; ++j)
      EXPECT(got[i * W + j] == (row_of[i] < 0 ? 0.f : vals[row_of[i] * W + j]));
  s->FinishIter();
  auto* hs = dynamic_cast<HipStorage<float>*>(s.get());
  EXPECT(hs != nullptr);
  pskv_sparse_info si;
  si.size = sizeof(si);
  EXPECT(pskv_sparse_info_get(hs->shard(), &si) == PSKV_OK);
  EXPECT(si.capacity == 8 && si.count == 3 && si.table_slots == 16);  // the Get of 77 stored nothing
}

static void SparseStep() {
  std::printf("[ RUN ] SparseStep\n");
  pskv_optimizer opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.kind = PSKV_OPT_SGD;
  opt.lr = 0.5;
  auto s = HipStorage<float>::Sparse(0, 100, PSKV_ASSIGN, 2, &opt);
  const std::vector<uint32_t> keys = {4000000000u, 9u, 4000000000u};
  const std::vector<float> grads = {1.f, 2.f, 4.f, 8.f, 0.5f, 0.25f};
  s->SubAdd(third_party::SArray<Key>(keys), third_party::SArray<char>(third_party::SArray<float>(grads)));
  auto got = third_party::SArray<float>(s->SubGet(third_party::SArray<Key>(std::vector<uint32_t>{9u, 4000000000u, 10u})));
  EXPECT(got.size() == 6);
  const float want[6] = {-2.f, -4.f, -0.75f, -1.125f, 0.f, 0.f};  // p = 0 - lr * sum of the key's rows
  for (size_t i = 0; i < 6 && got.size() == 6; ++i) EXPECT(got[i] == want[i]);
  uint64_t t = 0;
  EXPECT(pskv_get_step(s->shard(), &t) == PSKV_OK && t == 1);
  s->FinishIter();
}

static void HashedSparseTable() {
  std::printf("[ RUN ] HashedSparseTable\n");
  const uint32_t model_id = 3;
  const uint64_t capacity = 4096;  // about 2000 of the 4000 ids reach each server
  ConsistentHashShardMap map({0, 1});
  std::vector<std::unique_ptr<ServerThread>> threads;
  for (uint32_t i = 0; i < 2; ++i) threads.emplace_back(new ServerThread(i));
  ReplyQueue replies;
  auto st = CreateTable<float>(threads, map, 1ull << 32, model_id, ModelType::ASP, StorageType::Hip, 0, &replies,
                               PSKV_ASSIGN, nullptr, 1, capacity);
  EXPECT(st.size() == 2);
  std::mt19937 rng(5);
  std::map<uint32_t, float> want;
  std::set<uint32_t> owned[2];
  std::vector<uint32_t> pushed;
  for (int round = 0; round < 3; ++round) {
    // rounds 0 and 1: fresh hashed ids; round 2: earlier ids again, some twice
    std::vector<uint32_t> ks(2000);
    for (auto& k : ks) k = round == 2 ? pushed[rng() % pushed.size()] : (uint32_t)rng();
    ks[0] = 0u;
    ks[1] = 0xFFFFFFFFu;
    ks[2] = 0x80000000u;
    pushed.insert(pushed.end(), ks.begin(), ks.end());
    third_party::SArray<uint32_t> ka(ks);
    std::vector<std::pair<int, AbstractPartitionManager::Keys>> sl;
    map.Slice(ka, &sl);
    for (auto& s : sl) {
      std::vector<float> vs(s.second.size());
      for (size_t i = 0; i < vs.size(); ++i) {
        vs[i] = float((s.second[i] % 4093u) + 1u) + float(round) / 4;
        want[s.second[i]] = vs[i];  // (within a slice the last occurrence wins, as in the map)
        owned[s.first].insert(s.second[i]);
      }
      Message m;
      m.meta.flag = Flag::kAdd;
      m.meta.model_id = model_id;
      m.AddData(s.second);
      m.AddData(third_party::SArray<float>(vs));
      threads[s.first]->GetModel(model_id)->Add(m);
    }
  }
  // pull every key written and as many that were not, through the map
  std::vector<uint32_t> q;
  for (auto& kv : want) q.push_back(kv.first);
  for (size_t i = 0, n = q.size(); i < n; ++i)
    if (!want.count(q[i] + 1u)) q.push_back(q[i] + 1u);
  third_party::SArray<uint32_t> qa(q);
  std::vector<std::pair<int, AbstractPartitionManager::Keys>> sl;
  map.Slice(qa, &sl);
  size_t bad = 0, seen = 0;
  for (auto& s : sl) {
    Message m;
    m.meta.flag = Flag::kGet;
    m.meta.model_id = model_id;
    m.meta.recver = s.first;
    m.AddData(s.second);
    threads[s.first]->GetModel(model_id)->Get(m);
    Message r;
    EXPECT(replies.Pop(&r));
    auto v = third_party::SArray<float>(r.data[1]);
    EXPECT(v.size() == s.second.size());
    for (size_t i = 0; i < s.second.size() && i < v.size(); ++i, ++seen) {
      auto it = want.find(s.second[i]);
      bad += v[i] != (it == want.end() ? 0.f : it->second);
    }
  }
  EXPECT(seen == q.size() && bad == 0);
  EXPECT(owned[0].size() + owned[1].size() == want.size() && !owned[0].empty() && !owned[1].empty());
  for (size_t i = 0; i < 2; ++i) {
    st[i]->FinishIter();
    auto* hs = dynamic_cast<HipStorage<float>*>(st[i]);
    EXPECT(hs != nullptr);
    pskv_sparse_info si;
    si.size = sizeof(si);
    EXPECT(pskv_sparse_info_get(hs->shard(), &si) == PSKV_OK);
    EXPECT(si.capacity == capacity && si.count == owned[i].size());  // its own keys only; the Gets stored nothing
    std::vector<uint32_t> held(capacity);
    uint64_t n = 0;
    EXPECT(pskv_sparse_keys(hs->shard(), held.data(), held.size(), &n, PSKV_HOST) == PSKV_OK);
    EXPECT(n == owned[i].size());
    EXPECT(std::set<uint32_t>(held.begin(), held.begin() + std::min<uint64_t>(n, capacity)) == owned[i]);
    pskv_info info;
    EXPECT(pskv_shard_info(hs->shard(), &info) == PSKV_OK);
    EXPECT(info.key_begin == 0 && info.key_end == (1ull << 32));
    EXPECT(info.dense_bytes == (capacity + 1) * sizeof(float));  // not 2^32 * 4 bytes
    uint64_t two = 0;
    EXPECT(pskv_sparse_keys(hs->shard(), held.data(), 2, &two, PSKV_HOST) == PSKV_OK && two == n);  // n may exceed cap
  }
}

int main() {
  SparseAddGet();
  SparseStep();
  HashedSparseTable();
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
