// hip_storage_opt_test.cpp — HipStorage<float> with an optimizer (the last
// constructor argument), held as std::unique_ptr<AbstractStorage> the way a
// consistency model holds it (server/consistency/ssp_model.hpp:42): an Add
// message carries gradients.
//
//   SubAddIsAStep        Add{5:g1,5:g2,7:g3} is ONE step: key 5 steps once, on g1 + g2
//   AddGroupedIsOneStep  AddGrouped of two messages on overlapping keys (the BSP
//                        flush, bsp_model.cpp:14-31) is one step on the summed
//                        gradients, not two steps
//
// SGD with lr = 2^-3 and weight decay 2^-2 on multiples of 2^-2: every product,
// sum and difference is exact in float, so the results are compared bit for
// bit, and the weight decay makes two steps differ from one step on the sum.
//
// Needs a GPU (run by tests/test_opt_gpu.py).
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
constexpr float kLr = 0.125f, kWd = 0.25f;

// gradient row of a test: kWidth multiples of 2^-2 derived from `seed`
static std::vector<float> Rows(std::initializer_list<int> seeds) {
  std::vector<float> v;
  for (int s : seeds)
    for (uint32_t j = 0; j < kWidth; ++j) v.push_back(float(s) + float(j) / 4.f);
  return v;
}

// one SGD step of one value from the summed gradient g
static float Step(float p, float g) { return p - kLr * (g + kWd * p); }

static std::unique_ptr<AbstractStorage> MakeStorage() {
  pskv_optimizer opt{};
  opt.kind = PSKV_OPT_SGD;
  opt.lr = kLr;
  opt.weight_decay = kWd;
  return std::unique_ptr<AbstractStorage>(new HipStorage<float>(0, 2, 1 << 10, PSKV_ASSIGN, 0, kWidth, &opt));
}

static third_party::SArray<float> Pull(AbstractStorage* s, std::initializer_list<Key> keys) {
  Message g;
  g.meta.flag = Flag::kGet;
  g.AddData(third_party::SArray<Key>(keys));
  Message rep = s->Get(g);
  return third_party::SArray<float>(rep.data[1]);
}

static void SubAddIsAStep() {
  std::printf("[ RUN ] SubAddIsAStep\n");
  auto s = MakeStorage();
  const std::vector<float> g = Rows({1, 2, 3});
  {
    Message m;
    m.AddData(third_party::SArray<Key>({5, 5, 7}));
    m.AddData(third_party::SArray<float>(g));
    s->Add(m);
  }
  auto v = Pull(s.get(), {5, 7, 9});
  EXPECT(v.size() == 3 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 3 * kWidth; ++j) {
    const float want5 = Step(0.f, g[j] + g[kWidth + j]), want7 = Step(0.f, g[2 * kWidth + j]);
    EXPECT(std::memcmp(&v[j], &want5, sizeof(float)) == 0);
    EXPECT(std::memcmp(&v[kWidth + j], &want7, sizeof(float)) == 0);
    EXPECT(v[2 * kWidth + j] == 0.f);
  }
  // a second message is a second step, from the parameters the first left
  {
    Message m;
    m.AddData(third_party::SArray<Key>({7}));
    m.AddData(third_party::SArray<float>(Rows({10})));
    s->Add(m);
  }
  auto v2 = Pull(s.get(), {5, 7});
  const std::vector<float> g10 = Rows({10});
  for (uint32_t j = 0; j < kWidth && v2.size() == 2 * kWidth; ++j) {
    const float want7 = Step(Step(0.f, g[2 * kWidth + j]), g10[j]);
    EXPECT(std::memcmp(&v2[j], &v[j], sizeof(float)) == 0);  // key 5: untouched
    EXPECT(std::memcmp(&v2[kWidth + j], &want7, sizeof(float)) == 0);
  }
  s->FinishIter();
}

static void AddGroupedIsOneStep() {
  std::printf("[ RUN ] AddGroupedIsOneStep\n");
  auto s = MakeStorage();
  const std::vector<float> ga = Rows({1, 2}), gb = Rows({4, 8});
  std::vector<Message> msgs(2);
  msgs[0].AddData(third_party::SArray<Key>({5, 7}));
  msgs[0].AddData(third_party::SArray<float>(ga));
  msgs[1].AddData(third_party::SArray<Key>({7, 9}));
  msgs[1].AddData(third_party::SArray<float>(gb));
  s->AddGrouped(msgs);
  auto v = Pull(s.get(), {5, 7, 9});
  EXPECT(v.size() == 3 * kWidth);
  for (uint32_t j = 0; j < kWidth && v.size() == 3 * kWidth; ++j) {
    const float want5 = Step(0.f, ga[j]);
    const float want7 = Step(0.f, ga[kWidth + j] + gb[j]);  // ONE step on the sum
    const float two7 = Step(Step(0.f, ga[kWidth + j]), gb[j]);
    const float want9 = Step(0.f, gb[kWidth + j]);
    EXPECT(want7 != two7);
    EXPECT(std::memcmp(&v[j], &want5, sizeof(float)) == 0);
    EXPECT(std::memcmp(&v[kWidth + j], &want7, sizeof(float)) == 0);
    EXPECT(std::memcmp(&v[2 * kWidth + j], &want9, sizeof(float)) == 0);
  }
  s->FinishIter();
}

int main() {
  SubAddIsAStep();
  AddGroupedIsOneStep();
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
