// hip_storage_rows_test.cpp — the reference's three-key storage cases at row
// width 4: HipStorage<Val>(..., width) held as std::unique_ptr<AbstractStorage>,
// the way a consistency model holds it (server/consistency/ssp_model.hpp:42).
//
//   AddGetRows         server/map_storage_test.cpp:19-75 with a row of 4 values per key
//   LastWriteWinsRows  SURVEY.md §0.1: Add{5:r1,5:r2,7:r3}; Add{7:r10}; Get{5,7,9} -> {r2,r10,0}
//   SizeCheckAborts    SubAdd with keys * width != values aborts (the reference's
//                      CHECK_EQ, map_storage.hpp:20), observed in a child process
//
// Needs a GPU (run by tests/test_rows_gpu.py).
#include <spawn.h>
#include <sys/wait.h>

#include <csignal>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "ps/hip_storage.hpp"

extern char** environ;

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

constexpr uint32_t kWidth = 4;

// row r of a test: kWidth distinct values derived from `seed`
template <typename V>
static std::vector<V> Rows(std::initializer_list<int> seeds) {
  std::vector<V> v;
  for (int s : seeds)
    for (uint32_t j = 0; j < kWidth; ++j) v.push_back(V(s) + V(j) / V(8));
  return v;
}

template <typename V>
static void AddGetRows(const char* name) {
  std::printf("[ RUN ] %s\n", name);
  std::unique_ptr<AbstractStorage> s(new HipStorage<V>(0, 0, 1 << 10, PSKV_ASSIGN, 0, kWidth));
  Message m;
  third_party::SArray<Key> s_keys({13, 14, 15});
  third_party::SArray<V> s_vals(Rows<V>({1, 2, 3}));
  m.AddData(s_keys);
  m.AddData(s_vals);
  s->Add(m);
  Message m2;
  m2.meta.sender = 7;
  m2.meta.recver = 1000;
  m2.meta.flag = Flag::kGet;
  m2.meta.model_id = 3;
  m2.AddData(s_keys);
  Message rep = s->Get(m2);
  EXPECT(rep.data.size() == 2);
  EXPECT(rep.meta.sender == 1000 && rep.meta.recver == 7);
  EXPECT(rep.meta.flag == Flag::kGet && rep.meta.model_id == 3);
  auto rep_keys = third_party::SArray<Key>(rep.data[0]);
  auto rep_vals = third_party::SArray<V>(rep.data[1]);
  EXPECT(rep_keys.size() == 3 && rep_vals.size() == 3 * kWidth);
  EXPECT(rep_keys.data() == s_keys.data());  // reply keys alias the request (abstract_storage.hpp:27)
  EXPECT(rep_vals.size() == s_vals.size() &&
         std::memcmp(rep_vals.data(), s_vals.data(), s_vals.size() * sizeof(V)) == 0);
  s->FinishIter();
}

template <typename V>
static void LastWriteWinsRows(const char* name) {
  std::printf("[ RUN ] %s\n", name);
  std::unique_ptr<AbstractStorage> s(new HipStorage<V>(0, 2, 1 << 10, PSKV_ASSIGN, 0, kWidth));
  {
    Message m;
    m.AddData(third_party::SArray<Key>({5, 5, 7}));
    m.AddData(third_party::SArray<V>(Rows<V>({1, 2, 3})));
    s->Add(m);
  }
  {
    Message m;
    m.AddData(third_party::SArray<Key>({7}));
    m.AddData(third_party::SArray<V>(Rows<V>({10})));
    s->Add(m);
  }
  Message g;
  g.AddData(third_party::SArray<Key>({5, 7, 9}));
  Message rep = s->Get(g);
  auto v = third_party::SArray<V>(rep.data[1]);
  const std::vector<V> want2 = Rows<V>({2}), want10 = Rows<V>({10});
  EXPECT(v.size() == 3 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 3 * kWidth; ++j) {
    EXPECT(v[j] == want2[j]);
    EXPECT(v[kWidth + j] == want10[j]);
    EXPECT(v[2 * kWidth + j] == V(0));
  }
  s->FinishIter();
}

// the child: 3 keys with 3 * kWidth - 1 values
static int SizeCheckChild() {
  HipStorage<float> s(0, 0, 1 << 10, PSKV_ASSIGN, 0, kWidth);
  third_party::SArray<Key> keys({13, 14, 15});
  third_party::SArray<float> vals(std::vector<float>(3 * kWidth - 1, 1.f));
  s.SubAdd(keys, third_party::SArray<char>(vals));  // aborts
  return 0;
}

static void SizeCheckAborts(const char* self) {
  std::printf("[ RUN ] SizeCheckAborts\n");
  std::fflush(stdout);
  char arg0[4096], arg1[] = "--size-check-child";
  std::snprintf(arg0, sizeof(arg0), "%s", self);
  char* const argv[] = {arg0, arg1, nullptr};
  pid_t pid = 0;
  EXPECT(posix_spawn(&pid, self, nullptr, nullptr, argv, environ) == 0);
  int status = 0;
  EXPECT(waitpid(pid, &status, 0) == pid);
  EXPECT(WIFSIGNALED(status) && WTERMSIG(status) == SIGABRT);
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--size-check-child") == 0) return SizeCheckChild();
  // first: this process has not touched the GPU yet
  SizeCheckAborts(argv[0]);
  AddGetRows<float>("AddGetRowsFloat");
  AddGetRows<double>("AddGetRowsDouble");
  LastWriteWinsRows<float>("LastWriteWinsRowsFloat");
  LastWriteWinsRows<double>("LastWriteWinsRowsDouble");
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
