// hip_storage_score_matrix_test.cpp — HipStorage<Val>::SubGetScoreMatrix
// against a host loop in long double: 70 keys (a whole window and a short one,
// repeats, a never-written row) by 19 queries.  Once as the method's host
// call, once as a device call of pskv_get_score_matrix on frames (page-locked
// and mapped) into a column block of a wider matrix.
// Bound: |got - ref| <= gamma_W * sum_j |q_j p_j|, gamma_W = W u / (1 - W u).
// Needs a GPU (run by tests/test_score_matrix_gpu.py).
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
static void Matrix(const char* name, uint32_t width) {
  std::printf("[ RUN ] %s width %u\n", name, width);
  const uint32_t rows = 50, kb = 10, ke = kb + rows, n = 70, nq = 19, stride = n + 6, col = 3;
  const long double ur = std::is_same<V, float>::value ? std::ldexp(1.0L, -24) : std::ldexp(1.0L, -53);
  HipStorage<V> s(0, kb, ke, PSKV_ASSIGN, 0, width);
  std::mt19937 rng(23 + width);
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
  for (uint32_t i = 0; i < n; ++i) keys.push_back(i == 5 ? ke - 1 : kb + (i * 7) % rows);
  std::vector<V> q((size_t)nq * width);
  for (auto& x : q) x = draw();
  auto got = third_party::SArray<V>(s.SubGetScoreMatrix(third_party::SArray<Key>(keys), third_party::SArray<V>(q)));
  EXPECT(got.size() == (size_t)nq * n);
  if (got.size() != (size_t)nq * n) return;
  auto d_keys = FrameArray<Key>(n);
  auto d_q = FrameArray<V>(q.size());
  auto d_out = FrameArray<V>((size_t)nq * stride);
  std::memcpy(d_keys.data(), keys.data(), n * sizeof(Key));
  std::memcpy(d_q.data(), q.data(), q.size() * sizeof(V));
  for (size_t i = 0; i < (size_t)nq * stride; ++i) d_out.data()[i] = (V)77;
  pskv_check(pskv_get_score_matrix(s.shard(), d_keys.data(), n, d_q.data(), nq, d_out.data() + col, stride, PSKV_DEVICE),
             "pskv_get_score_matrix");
  pskv_check(pskv_sync(s.shard()), "pskv_sync");
  const long double gamma = width * ur / (1 - width * ur);
  for (uint32_t b = 0; b < nq; ++b) {
    const V* dev = d_out.data() + (size_t)b * stride;
    EXPECT(std::memcmp(dev + col, &got[(size_t)b * n], n * sizeof(V)) == 0);
    for (uint32_t i = 0; i < stride; ++i)
      if (i < col || i >= col + n) EXPECT(dev[i] == (V)77);
    for (uint32_t i = 0; i < n; ++i) {
      const V* p = &init[(size_t)(keys[i] - kb) * width];
      long double dot = 0, mag = 0;
      for (uint32_t j = 0; j < width; ++j) {
        dot += (long double)q[(size_t)b * width + j] * p[j];
        mag += std::fabs((long double)q[(size_t)b * width + j] * p[j]);
      }
      const V x = got[(size_t)b * n + i];
      EXPECT(std::fabs((long double)x - dot) <= gamma * mag);
      if (keys[i] == ke - 1) EXPECT(x == 0 && !std::signbit(x));
    }
  }
  s.FinishIter();
}

int main() {
  for (uint32_t width : {1u, 8u, 10u, 100u}) {
    Matrix<float>("ScoreMatrixFloat", width);
    Matrix<double>("ScoreMatrixDouble", width);
  }
  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  (void)pskv_host_pool_trim();
  return g_fail ? 1 : 0;
}
