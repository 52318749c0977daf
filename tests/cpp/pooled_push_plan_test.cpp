// CPU unit test of the pooled push's bag lookup (parameter_server_amd/csrc/pskv_plan.h):
// the kernels' two steps replayed on the host -- per virtual workgroup of
// kChunk consecutive key positions the bags of its two ends (pool_bag_span),
// then per position the bounded search (pool_bags_in), kRows positions in step
// as a lane group takes them.  With well-formed offsets every position gets
// its true bag, empty bags skipped; with any offsets the result is below
// nbags.  Host-only: no HIP, no GPU.
#include <cstdio>
#include <random>
#include <vector>

#include "pskv_plan.h"

using namespace pskv;

static int failed = 0, passed = 0;
#define EXPECT(c)                                                      \
  do {                                                                 \
    if (c) {                                                           \
      ++passed;                                                        \
    } else {                                                           \
      ++failed;                                                        \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
    }                                                                  \
  } while (0)

static const uint64_t kChunk = 2048;  // kGeneralChunk (pskv_internal.h, a HIP header)
static const int kRows = 4;           // kRowsInFlight (pskv_rows.hip)
static const uint64_t C = kPoolChunk;

// The lookup as k_row_step_losers / k_row_step_apply run it for a pooled push: bag of
// every position of [0, n), `stride` apart inside a step (a lane group's rows
// in flight are G positions apart), every other row of a step unwanted.
static std::vector<uint64_t> lookup(const std::vector<uint64_t>& off, uint64_t n, uint64_t stride, bool skip_odd) {
  const uint64_t nbags = off.size() - 1;
  std::vector<uint64_t> out(n, ~0ull);
  for (uint64_t base = 0; base < n; base += kChunk) {
    const uint64_t end = base + kChunk < n ? base + kChunk : n;
    const PoolSpan sp = pool_bag_span(off.data(), nbags, base, end - 1);
    EXPECT(sp.lo <= sp.hi && sp.hi < nbags);
    for (uint64_t r0 = 0; r0 < stride; ++r0)
      for (uint64_t q = base + r0; q < end; q += kRows * stride) {
        uint64_t x[kRows], bag[kRows];
        bool want[kRows];
        for (int r = 0; r < kRows; ++r) {
          x[r] = q + (uint64_t)r * stride;
          want[r] = x[r] < end && !(skip_odd && (r & 1));
        }
        pool_bags_in<kRows>(off.data(), sp, x, want, bag);
        for (int r = 0; r < kRows; ++r) {
          EXPECT(bag[r] >= sp.lo && bag[r] <= sp.hi);
          if (want[r]) out[x[r]] = bag[r];
          if (!want[r]) EXPECT(bag[r] == sp.lo);
        }
      }
  }
  return out;
}

static std::vector<uint64_t> offsets_of(const std::vector<uint64_t>& lens) {
  std::vector<uint64_t> off(1, 0);
  for (uint64_t m : lens) off.push_back(off.back() + m);
  return off;
}

static void test_true_bags() {
  std::vector<std::vector<uint64_t>> patterns;
  patterns.push_back(std::vector<uint64_t>(4100, 1));                       // bags of 1
  patterns.push_back(std::vector<uint64_t>(513, 8));                        // bags of 8
  patterns.push_back({0, 1, 5, C + 1, 0, 3 * C + 2, 17, C, 2, 1, 5, C + 1, 0, 3 * C + 2, 17, C, 2, 0});  // mixed
  patterns.push_back({4100});                                               // one bag: lo == hi in every workgroup
  {
    std::vector<uint64_t> b(682, 3);                                        // a boundary exactly at position 2048
    b.push_back(2);
    b.insert(b.end(), {0, 0, 1000, 1052});
    patterns.push_back(b);
  }
  patterns.push_back({0, 0, 0, 1, 0, 0});                                   // one key among empty bags
  patterns.push_back({2048, 2048, 1});                                      // bags equal to workgroups
  patterns.push_back({1, 2047, 0, 0, 2049, 0});
  for (const auto& lens : patterns) {
    const std::vector<uint64_t> off = offsets_of(lens);
    const uint64_t n = off.back();
    EXPECT(n > 0);
    std::vector<uint64_t> truth;
    for (size_t b = 0; b < lens.size(); ++b) truth.insert(truth.end(), lens[b], (uint64_t)b);
    for (uint64_t stride : {1ull, 4ull, 64ull, 256ull}) {
      const std::vector<uint64_t> got = lookup(off, n, stride, false);
      bool same = got == truth;
      EXPECT(same);
      for (uint64_t i = 0; i < n; ++i) EXPECT(pool_bag_of(off.data(), lens.size(), i) == truth[i]);
      const std::vector<uint64_t> half = lookup(off, n, stride, true);
      for (uint64_t i = 0; i < n; ++i) EXPECT(half[i] == ~0ull || half[i] == truth[i]);
    }
  }
}

static void test_malformed_offsets_stay_below_nbags() {
  std::mt19937_64 rng(7);
  const uint64_t n = 5000;
  for (int round = 0; round < 40; ++round) {
    const uint64_t nbags = 1 + rng() % 700;
    std::vector<uint64_t> off(nbags + 1);
    const int form = round % 5;
    for (uint64_t b = 0; b <= nbags; ++b) {
      if (form == 0) off[b] = rng() % (2 * n);            // random
      if (form == 1) off[b] = (nbags - b) * 7;            // decreasing
      if (form == 2) off[b] = n + 1 + b * 1000;           // all past n
      if (form == 3) off[b] = 17;                         // all equal
      if (form == 4) off[b] = (b & 1) ? ~0ull - b : rng() % 64;  // huge values between small ones
    }
    for (uint64_t stride : {1ull, 64ull}) {
      const std::vector<uint64_t> got = lookup(off, n, stride, false);  // (lookup checks lo <= bag <= hi < nbags)
      for (uint64_t i = 0; i < n; ++i) EXPECT(got[i] < nbags);
    }
  }
}

int main() {
  test_true_bags();
  test_malformed_offsets_stay_below_nbags();
  std::printf("%d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
