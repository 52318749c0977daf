// CPU unit test of the sparse shard's host rules (parameter_server_amd/csrc/pskv_plan.h):
// the index size of a capacity, the growth rule of a writing call and the
// host-side test that decides whether the count must be read for it, the
// refusal of a capacity, and the optimizer's state slots with their start
// values.  Host-only: no HIP, no GPU.
//   sparse_plan_test                            the checks; ends "N passed, 0 failed"
//   sparse_plan_test --grid CAP_LO CAP_HI N_HI  prints, for every capacity c of the range,
//       "slots c <sparse_table_slots>" and, for count 0..c, n 0..N_HI and max in
//       {c, c + 1, 2c - 1, 2c, 4c}, "grow c count n max <sparse_grown_capacity>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

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

static const uint64_t M = kSparseMaxCapacity;

static void test_table_slots() {
  EXPECT(M == (1ull << 31) - 2);
  EXPECT(sparse_table_slots(1) == 16 && sparse_table_slots(8) == 16 && sparse_table_slots(9) == 32);
  EXPECT(sparse_table_slots(20) == 64 && sparse_table_slots(4100) == 16384);
  EXPECT(sparse_table_slots(1ull << 30) == 1ull << 31 && sparse_table_slots((1ull << 30) + 1) == 1ull << 32);
  EXPECT(sparse_table_slots(M) == 1ull << 32);
  for (uint64_t c = 1; c <= 5000; ++c) {  // a power of two, at least two entries per slot, the smallest such
    const uint64_t t = sparse_table_slots(c);
    EXPECT((t & (t - 1)) == 0 && t >= 16 && t >= 2 * c && (t == 16 || t / 2 < 2 * c));
  }
}

static void test_growth_rule() {
  // growth off, and a shard at its limit
  EXPECT(sparse_grown_capacity(8, 0, 8, 0) == 8 && sparse_grown_capacity(8, 8, 100, 0) == 8);
  EXPECT(!sparse_may_grow(8, 100, 8, 0) && !sparse_may_grow(8, 100, 8, 8));
  EXPECT(sparse_grown_capacity(4100, 4100, 37, 4100) == 4100);
  // count + n == capacity fits; one more grows
  EXPECT(sparse_grown_capacity(8, 0, 8, 4100) == 8 && sparse_grown_capacity(8, 7, 1, 4100) == 8);
  EXPECT(sparse_grown_capacity(8, 0, 9, 4100) == 16 && sparse_grown_capacity(8, 8, 1, 4100) == 16);
  EXPECT(sparse_grown_capacity(8, 8, 0, 4100) == 8);  // a call without keys does not grow
  // doubling against count + n, both clamped by the limit
  EXPECT(sparse_grown_capacity(8, 3, 14, 4100) == 17 && sparse_grown_capacity(8, 3, 13, 4100) == 16);
  EXPECT(sparse_grown_capacity(8, 0, 4100, 4100) == 4100 && sparse_grown_capacity(8, 0, 5000, 4100) == 4100);
  EXPECT(sparse_grown_capacity(100, 100, 1, 150) == 150 && sparse_grown_capacity(100, 60, 41, 101) == 101);
  EXPECT(sparse_grown_capacity(16, 16, 600, 20) == 20);  // n larger than max
  // capacity 1
  EXPECT(sparse_grown_capacity(1, 0, 1, 5) == 1 && sparse_grown_capacity(1, 1, 1, 5) == 2);
  EXPECT(sparse_grown_capacity(1, 1, 9, 5) == 5 && sparse_grown_capacity(1, 1, 1, 1) == 1);
  // around the largest capacity
  EXPECT(sparse_grown_capacity(1ull << 30, 1ull << 30, 1, M) == M);
  EXPECT(sparse_grown_capacity(M - 1, M - 1, 1, M) == M && sparse_grown_capacity(M - 1, M - 2, 1, M) == M - 1);
  EXPECT(sparse_grown_capacity(M, M, 1ull << 31, M) == M && !sparse_may_grow(M, 1ull << 31, M, M));
  EXPECT(sparse_grown_capacity(M / 2, M / 2, 1, M) == M && sparse_grown_capacity(M / 2 + 1, 0, M, M) == M);
  EXPECT(sparse_grown_capacity(M / 2 - 1, M / 2 - 1, 1, M) == M - 2);  // doubling just below the limit
}

// While bound + n <= capacity the count need not be read: for every count <=
// bound the rule leaves the capacity alone.  And where the rule fires for some
// count <= bound, sparse_may_grow says so.
static void test_bound_agrees_with_count() {
  const uint64_t caps[] = {1, 2, 7, 8, 33, M - 2, M - 1, M};
  for (uint64_t cap : caps) {
    const uint64_t maxes[] = {0, cap, cap + 1, 2 * cap - 1, 2 * cap, 4 * cap, M};
    for (uint64_t max : maxes) {
      if (max > M) continue;
      const uint64_t ns[] = {0, 1, 2, cap - 1, cap, cap + 1, max, max + 1, 1ull << 31};
      const uint64_t bounds[] = {0, 1, cap / 2, cap - 1, cap};
      for (uint64_t n : ns)
        for (uint64_t bound : bounds) {
          const bool may = sparse_may_grow(bound, n, cap, max);
          const uint64_t lows[] = {0, bound / 2, bound ? bound - 1 : 0, bound};
          for (uint64_t count : lows) {
            const uint64_t to = sparse_grown_capacity(cap, count, n, max);
            EXPECT(to >= cap && (to == cap || (to <= max && to >= std::min(max, count + n))));
            if (!may) EXPECT(to == cap);
            if (to != cap) EXPECT(may);
          }
        }
    }
  }
}

// The same walked in full for the small capacities: every bound <= capacity,
// every count <= bound, n 0..70.  The test is also tight: it says "read the
// count" exactly where the count, were it the bound itself, would grow the shard.
static void test_bound_walked_for_small_capacities() {
  EXPECT(!sparse_may_grow(0, 8, 8, 64) && sparse_may_grow(0, 9, 8, 64) && sparse_may_grow(8, 1, 8, 64));
  EXPECT(!sparse_may_grow(7, 1, 8, 64) && !sparse_may_grow(8, 0, 8, 64) && !sparse_may_grow(8, 100, 8, 8));
  EXPECT(!sparse_may_grow(8, 100, 8, 0) && sparse_may_grow(1, 1, 1, 2) && !sparse_may_grow(0, 1, 1, 2));
  for (uint64_t cap = 1; cap <= 33; ++cap) {
    const uint64_t maxes[] = {0, cap, cap + 1, 2 * cap - 1, 2 * cap, 4 * cap};
    for (uint64_t max : maxes)
      for (uint64_t n = 0; n <= 70; ++n)
        for (uint64_t bound = 0; bound <= cap; ++bound) {
          const bool may = sparse_may_grow(bound, n, cap, max);
          bool all_stay = true;
          for (uint64_t count = 0; count <= bound; ++count)
            all_stay = all_stay && sparse_grown_capacity(cap, count, n, max) == cap;
          if (!may) EXPECT(all_stay);
          EXPECT(may == (sparse_grown_capacity(cap, bound, n, max) != cap));
        }
  }
}

static void test_capacity_refusal() {
  EXPECT(sparse_capacity_error(8, 8, 4) == nullptr && sparse_capacity_error(8, M, 4) == nullptr);
  const char* why = sparse_capacity_error(8, 7, 4);
  EXPECT(why && std::strstr(why, "does not shrink"));
  // (capacity + 1) rows of 2^15 bytes: 2^31 - 1 rows are 2^46 - 2^15 bytes, 2^31 rows are 2^46
  EXPECT(sparse_capacity_error(8, (1ull << 31) - 2, 1ull << 15) == nullptr);
  EXPECT(sparse_capacity_error(8, (1ull << 31) - 1, 1ull << 15) == nullptr);
  why = sparse_capacity_error(8, 1ull << 31, 1ull << 15);
  EXPECT(why && std::strstr(why, "2^46"));
  why = sparse_capacity_error(8, M, 1ull << 16);
  EXPECT(why && std::strstr(why, "2^46"));
  why = sparse_capacity_error(M, M - 1, 1ull << 16);  // shrinking is named first
  EXPECT(why && std::strstr(why, "does not shrink"));
}

static void test_opt_slots() {
  const int kinds[] = {PSKV_OPT_NONE, PSKV_OPT_SGD, PSKV_OPT_ADAGRAD, PSKV_OPT_MOMENTUM, PSKV_OPT_ADAM, PSKV_OPT_FTRL};
  const int slots[] = {0, 0, 1, 1, 2, 2};
  for (int i = 0; i < 6; ++i) {
    EXPECT(opt_slots(kinds[i]) == slots[i]);
    for (int slot = 0; slot < 2; ++slot) {
      const bool accum = (kinds[i] == PSKV_OPT_ADAGRAD && slot == 0) || (kinds[i] == PSKV_OPT_FTRL && slot == 1);
      EXPECT(opt_slot_is_accum(kinds[i], slot) == accum);
      if (opt_slot_is_accum(kinds[i], slot)) EXPECT(slot < opt_slots(kinds[i]));  // only a slot the kind has
    }
  }
}

static int print_grid(uint64_t cap_lo, uint64_t cap_hi, uint64_t n_hi) {
  for (uint64_t c = cap_lo; c <= cap_hi; ++c) {
    std::printf("slots %llu %llu\n", (unsigned long long)c, (unsigned long long)sparse_table_slots(c));
    const uint64_t maxes[] = {c, c + 1, 2 * c - 1, 2 * c, 4 * c};
    for (uint64_t count = 0; count <= c; ++count)
      for (uint64_t n = 0; n <= n_hi; ++n)
        for (uint64_t max : maxes)
          std::printf("grow %llu %llu %llu %llu %llu\n", (unsigned long long)c, (unsigned long long)count,
                      (unsigned long long)n, (unsigned long long)max,
                      (unsigned long long)sparse_grown_capacity(c, count, n, max));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && std::string(argv[1]) == "--grid")
    return print_grid(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10),
                      std::strtoull(argv[4], nullptr, 10));
  if (argc != 1) {
    std::printf("usage: sparse_plan_test [--grid CAP_LO CAP_HI N_HI]\n");
    return 2;
  }
  test_table_slots();
  test_growth_rule();
  test_bound_agrees_with_count();
  test_bound_walked_for_small_capacities();
  test_capacity_refusal();
  test_opt_slots();
  std::printf("sparse_plan_test: %d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
