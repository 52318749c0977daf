// hip_storage_opt2_test.cpp — HipStorage<float> with a momentum optimizer (the
// pskv_optimizer_ex constructor), held as std::unique_ptr<AbstractStorage>.
//
//   TwoAddsAreTwoSteps   two Add messages on one key are two momentum steps:
//                        the second sees the velocity the first left
//   AddGroupedIsOneStep  AddGrouped of the same two messages is ONE step on
//                        the summed gradients
//
// momentum = 0.5, lr = 2^-3, no weight decay, gradients multiples of 2^-2:
// every product, sum and difference is exact in float, so the results are
// compared bit for bit (v1 = g1, p1 = -lr g1; v2 = g1 / 2 + g2,
// p2 = p1 - lr v2; one step: v = g1 + g2, p = -lr v).
//
// Needs a GPU (run by tests/test_opt2_gpu.py).
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
constexpr float kLr = 0.125f, kMu = 0.5f;

static std::vector<float> Row(int seed) {
  std::vector<float> v;
  for (uint32_t j = 0; j < kWidth; ++j) v.push_back(float(seed) + float(j) / 4.f);
  return v;
}

static std::unique_ptr<AbstractStorage> MakeStorage(int nesterov) {
  pskv_optimizer_ex opt{};
  opt.size = sizeof(opt);
  opt.kind = PSKV_OPT_MOMENTUM;
  opt.lr = kLr;
  opt.momentum = kMu;
  opt.nesterov = nesterov;
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

// one momentum step of one value: the new (p, v)
static void Step(float& p, float& v, float g, int nesterov) {
  v = kMu * v + g;
  p = p - kLr * (nesterov ? g + kMu * v : v);
}

static void TwoAddsAreTwoSteps(int nesterov) {
  std::printf("[ RUN ] TwoAddsAreTwoSteps nesterov=%d\n", nesterov);
  auto s = MakeStorage(nesterov);
  const std::vector<float> g1 = Row(1), g2 = Row(6);
  {
    Message m = AddMsg(5, g1);
    s->Add(m);
  }
  {
    Message m = AddMsg(5, g2);
    s->Add(m);
  }
  auto v = Pull(s.get(), {5, 7});
  EXPECT(v.size() == 2 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 2 * kWidth; ++j) {
    float p = 0.f, vel = 0.f;
    Step(p, vel, g1[j], nesterov);
    Step(p, vel, g2[j], nesterov);
    EXPECT(std::memcmp(&v[j], &p, sizeof(float)) == 0);
    EXPECT(v[kWidth + j] == 0.f);  // key 7: untouched
  }
  s->FinishIter();
}

static void AddGroupedIsOneStep(int nesterov) {
  std::printf("[ RUN ] AddGroupedIsOneStep nesterov=%d\n", nesterov);
  auto s = MakeStorage(nesterov);
  const std::vector<float> g1 = Row(1), g2 = Row(6);
  std::vector<Message> msgs;
  msgs.push_back(AddMsg(5, g1));
  msgs.push_back(AddMsg(5, g2));
  s->AddGrouped(msgs);
  auto v = Pull(s.get(), {5, 7});
  EXPECT(v.size() == 2 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 2 * kWidth; ++j) {
    float p = 0.f, vel = 0.f;
    Step(p, vel, g1[j] + g2[j], nesterov);  // ONE step on the sum
    float p2 = 0.f, vel2 = 0.f;
    Step(p2, vel2, g1[j], nesterov);
    Step(p2, vel2, g2[j], nesterov);
    EXPECT(p != p2);
    EXPECT(std::memcmp(&v[j], &p, sizeof(float)) == 0);
    EXPECT(v[kWidth + j] == 0.f);
  }
  s->FinishIter();
}

int main() {
  for (int nesterov = 0; nesterov < 2; ++nesterov) {
    TwoAddsAreTwoSteps(nesterov);
    AddGroupedIsOneStep(nesterov);
  }
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
