// hip_storage_sparse_grow_test.cpp — sparse storages that grow and forget:
// CreateTable's sparse_max_capacity, HipStorage::Reserve / SetGrowth / Erase.
//
//   GrowingHashedTable  two servers under jump hashing, sparse storages of
//                       capacity 8 that may grow to 4096: a few hundred hashed
//                       ids pushed in three rounds through the models; the
//                       replies are those of a std::map, no push is dropped, and
//                       each storage holds exactly the keys the hash sent it.
//                       Then Erase of every third key: the replies are those of
//                       the map after erase, and erased keys read 0
//   ReserveKeeps        HipStorage::Reserve on a full capacity-8 storage: rows
//                       kept, room for more
//
// Needs a GPU (run by tests/test_sparse_grow_gpu.py).
#include <algorithm>
#include <cstdio>
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

typedef std::vector<std::pair<int, AbstractPartitionManager::Keys>> Slices;

// Pull `q` through the map and count the replies that differ from `want` (0 for a key it lacks).
static size_t Mismatches(ConsistentHashShardMap& map, std::vector<std::unique_ptr<ServerThread>>& threads,
                         ReplyQueue& replies, uint32_t model_id, const std::vector<uint32_t>& q,
                         const std::map<uint32_t, float>& want) {
  third_party::SArray<uint32_t> qa(q);
  Slices sl;
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
    if (!replies.Pop(&r)) return q.size();
    auto v = third_party::SArray<float>(r.data[1]);
    if (v.size() != s.second.size()) return q.size();
    for (size_t i = 0; i < s.second.size(); ++i, ++seen) {
      auto it = want.find(s.second[i]);
      bad += v[i] != (it == want.end() ? 0.f : it->second);
    }
  }
  return bad + (seen == q.size() ? 0 : q.size());
}

static void GrowingHashedTable() {
  std::printf("[ RUN ] GrowingHashedTable\n");
  const uint32_t model_id = 4;
  ConsistentHashShardMap map({0, 1});
  std::vector<std::unique_ptr<ServerThread>> threads;
  for (uint32_t i = 0; i < 2; ++i) threads.emplace_back(new ServerThread(i));
  ReplyQueue replies;
  auto st = CreateTable<float>(threads, map, 1ull << 32, model_id, ModelType::ASP, StorageType::Hip, 0, &replies,
                               PSKV_ASSIGN, nullptr, 1, /*sparse_capacity=*/8, /*sparse_max_capacity=*/4096);
  EXPECT(st.size() == 2);
  std::mt19937 rng(11);
  std::map<uint32_t, float> want;
  std::set<uint32_t> owned[2];
  std::vector<uint32_t> pushed;
  for (int round = 0; round < 3; ++round) {
    // rounds 0 and 1: fresh hashed ids; round 2: earlier ids again, some twice
    std::vector<uint32_t> ks(150);
    for (auto& k : ks) k = round == 2 ? pushed[rng() % pushed.size()] : (uint32_t)rng();
    ks[0] = 0u;
    ks[1] = 0xFFFFFFFFu;
    ks[2] = 0x80000000u;
    pushed.insert(pushed.end(), ks.begin(), ks.end());
    third_party::SArray<uint32_t> ka(ks);
    Slices sl;
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
  std::vector<uint32_t> q;
  for (auto& kv : want) q.push_back(kv.first);
  for (size_t i = 0, n = q.size(); i < n; ++i)
    if (!want.count(q[i] + 1u)) q.push_back(q[i] + 1u);
  EXPECT(Mismatches(map, threads, replies, model_id, q, want) == 0);
  EXPECT(!owned[0].empty() && !owned[1].empty() && owned[0].size() > 8 && owned[1].size() > 8);
  for (size_t i = 0; i < 2; ++i) {
    st[i]->FinishIter();  // (aborts had a key been dropped)
    auto* hs = dynamic_cast<HipStorage<float>*>(st[i]);
    EXPECT(hs != nullptr);
    pskv_sparse_info si;
    si.size = sizeof(si);
    EXPECT(pskv_sparse_info_get(hs->shard(), &si) == PSKV_OK);
    EXPECT(si.count == owned[i].size() && si.capacity >= si.count && si.capacity <= 4096 && si.capacity > 8);
    uint64_t limit = 0, rebuilds = 0;
    EXPECT(pskv_sparse_get_growth(hs->shard(), &limit, &rebuilds) == PSKV_OK && limit == 4096 && rebuilds >= 1);
  }
  // std::map::erase of every third key (and of keys nobody holds), through each storage
  std::vector<uint32_t> gone[2];
  size_t at = 0;
  for (auto it = want.begin(); it != want.end(); ++at) {
    if (at % 3 == 0) {
      const int srv = owned[0].count(it->first) ? 0 : 1;
      gone[srv].push_back(it->first);
      owned[srv].erase(it->first);
      it = want.erase(it);
    } else {
      ++it;
    }
  }
  for (size_t i = 0; i < 2; ++i) {
    gone[i].push_back(gone[i][0]);          // listed twice
    gone[i].push_back(gone[1 - i].back());  // the other server's key: not stored here
    auto* hs = dynamic_cast<HipStorage<float>*>(st[i]);
    hs->Erase(third_party::SArray<Key>(gone[i]));
    st[i]->FinishIter();
    pskv_sparse_info si;
    si.size = sizeof(si);
    EXPECT(pskv_sparse_info_get(hs->shard(), &si) == PSKV_OK && si.count == owned[i].size());
    std::vector<uint32_t> held(si.capacity);
    uint64_t n = 0;
    EXPECT(pskv_sparse_keys(hs->shard(), held.data(), held.size(), &n, PSKV_HOST) == PSKV_OK && n == owned[i].size());
    EXPECT(std::set<uint32_t>(held.begin(), held.begin() + std::min<uint64_t>(n, held.size())) == owned[i]);
  }
  EXPECT(Mismatches(map, threads, replies, model_id, q, want) == 0);  // (q still names the erased keys: they read 0)
}

static void ReserveKeeps() {
  std::printf("[ RUN ] ReserveKeeps\n");
  auto s = HipStorage<float>::Sparse(0, 8, PSKV_ASSIGN, 3);
  std::vector<uint32_t> keys;
  std::vector<float> vals;
  for (uint32_t i = 0; i < 8; ++i) {
    keys.push_back(i * 0x20000001u);
    for (uint32_t j = 0; j < 3; ++j) vals.push_back(float(i) + float(j) / 4 + 1.f);
  }
  s->SubAdd(third_party::SArray<Key>(keys), third_party::SArray<char>(third_party::SArray<float>(vals)));
  s->Reserve(20);
  auto got = third_party::SArray<float>(s->SubGet(third_party::SArray<Key>(keys)));
  EXPECT(got.size() == vals.size());
  for (size_t i = 0; i < vals.size() && i < got.size(); ++i) EXPECT(got[i] == vals[i]);
  const std::vector<uint32_t> more = {7u, 8u, 9u};
  s->SubAdd(third_party::SArray<Key>(more),
            third_party::SArray<char>(third_party::SArray<float>(std::vector<float>(9, 2.5f))));
  s->FinishIter();
  pskv_sparse_info si;
  si.size = sizeof(si);
  EXPECT(pskv_sparse_info_get(s->shard(), &si) == PSKV_OK);
  EXPECT(si.capacity == 20 && si.count == 11 && si.table_slots == 64);
}

int main() {
  GrowingHashedTable();
  ReserveKeeps();
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
