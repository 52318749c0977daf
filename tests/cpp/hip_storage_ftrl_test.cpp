// hip_storage_ftrl_test.cpp — HipStorage<float> with an FTRL-Proximal optimizer
// (the pskv_optimizer_cfg constructor), held as std::unique_ptr<AbstractStorage>.
//
//   TwoAddsAreTwoSteps   two Add messages on one key are two FTRL steps
//   AddGroupedIsOneStep  AddGrouped of the same two messages is ONE step on the
//                        summed gradients
//   LargeL1GivesPlusZero with l1 above |z'| the weights are the bit pattern +0
//
// lr = 1, ftrl_beta = l1 = l2 = 0, n from 0, gradients 3 (j + 1) then 4 (j + 1)
// on column j: every square, root, sum and product is exact in float, so n and
// z are: (n, z, p) goes to (9, 3, -1) (j + 1)^{2, 1, 0}, then (25, 9, -1.8);
// one step on the sum gives (49, 7, -1).  -1.8 is one division, compared to
// two units in the last place (a build may divide without correct rounding).
//
// Needs a GPU (run by tests/test_ftrl_gpu.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
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

constexpr uint32_t kWidth = 4;

static std::vector<float> Row(float scale) {
  std::vector<float> v;
  for (uint32_t j = 0; j < kWidth; ++j) v.push_back(scale * float(j + 1));
  return v;
}

static std::unique_ptr<AbstractStorage> MakeStorage(double l1) {
  pskv_optimizer_cfg opt{};
  opt.size = sizeof(opt);
  opt.kind = PSKV_OPT_FTRL;
  opt.lr = 1.0;
  opt.l1 = l1;
  return std::unique_ptr<AbstractStorage>(new HipStorage<float>(0, 2, 1 << 10, PSKV_ASSIGN, 0, kWidth, &opt));
}

static Message AddMsg(Key k, const std::vector<float>& g) {
  Message m;
  m.AddData(third_party::SArray<Key>({k}));
  m.AddData(third_party::SArray<float>(g));
  return m;
}

static third_party::SArray<float> Pull(AbstractStorage* s, std::initializer_list<Key> keys) {
  Message g;
  g.meta.flag = Flag::kGet;
  g.AddData(third_party::SArray<Key>(keys));
  Message rep = s->Get(g);
  return third_party::SArray<float>(rep.data[1]);
}

static bool Near(float got, float want) { return std::fabs(got - want) <= 2.f * 1.1920929e-7f * std::fabs(want); }

static void TwoAddsAreTwoSteps() {
  std::printf("[ RUN ] TwoAddsAreTwoSteps\n");
  auto s = MakeStorage(0.0);
  {
    Message m = AddMsg(5, Row(3.f));
    s->Add(m);
  }
  auto v = Pull(s.get(), {5, 7});
  EXPECT(v.size() == 2 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 2 * kWidth; ++j) EXPECT(v[j] == -1.f);  // -3 (j+1) / (3 (j+1)): exact
  {
    Message m = AddMsg(5, Row(4.f));
    s->Add(m);
  }
  v = Pull(s.get(), {5, 7});
  EXPECT(v.size() == 2 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 2 * kWidth; ++j) {
    EXPECT(Near(v[j], -1.8f));
    EXPECT(v[kWidth + j] == 0.f);  // key 7: untouched
  }
  s->FinishIter();
}

static void AddGroupedIsOneStep() {
  std::printf("[ RUN ] AddGroupedIsOneStep\n");
  auto s = MakeStorage(0.0);
  std::vector<Message> msgs;
  msgs.push_back(AddMsg(5, Row(3.f)));
  msgs.push_back(AddMsg(5, Row(4.f)));
  s->AddGrouped(msgs);
  auto v = Pull(s.get(), {5, 7});
  EXPECT(v.size() == 2 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 2 * kWidth; ++j) {
    EXPECT(v[j] == -1.f);  // ONE step on the sum 7 (j+1): -7 / 7, not -1.8
    EXPECT(v[kWidth + j] == 0.f);
  }
  s->FinishIter();
}

static void LargeL1GivesPlusZero() {
  std::printf("[ RUN ] LargeL1GivesPlusZero\n");
  auto s = MakeStorage(64.0);  // |z'| is at most 7 * 4
  std::vector<Message> msgs;
  msgs.push_back(AddMsg(5, Row(-3.f)));
  msgs.push_back(AddMsg(5, Row(-4.f)));
  s->AddGrouped(msgs);
  auto v = Pull(s.get(), {5});
  EXPECT(v.size() == kWidth);
  const uint32_t zero = 0;
  for (uint32_t j = 0; j < kWidth && v.size() == kWidth; ++j) EXPECT(std::memcmp(&v[j], &zero, sizeof(float)) == 0);
  s->FinishIter();
}

int main() {
  TwoAddsAreTwoSteps();
  AddGroupedIsOneStep();
  LargeL1GivesPlusZero();
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
