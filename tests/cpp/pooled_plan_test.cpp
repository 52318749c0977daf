// CPU unit test of the pooled pull's planner (parameter_server_amd/csrc/pskv_plan.h):
// the check of a host call's offsets, the clamp the kernels apply to device
// offsets, the chunks of a long bag as a function of its length, and the
// window / slot rule by which k_row_pooled_chunks finds every chunk exactly
// once without the host reading the offsets.  Host-only: no HIP, no GPU.
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>
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

static const uint64_t C = kPoolChunk;

// (reason or "", first bad bag)
static std::pair<std::string, uint64_t> check(const std::vector<uint64_t>& off, uint64_t n) {
  uint64_t bad = ~0ull;
  const char* why = pool_offsets_error(off.empty() ? nullptr : off.data(), off.empty() ? 0 : off.size() - 1, n, &bad);
  return {why ? why : "", bad};
}

static void test_offsets_check() {
  EXPECT(check({}, 0).first.empty());              // nbags == 0: nothing to check, null offsets
  EXPECT(check({}, 17).first.empty());
  EXPECT(check({0}, 0).first.empty());             // one value is nbags == 0 too
  EXPECT(check({0, 0, 0, 0}, 0).first.empty());    // all bags empty
  EXPECT(check({0, 3, 3, 7}, 7).first.empty());
  EXPECT(check({0, 7}, 7).first.empty());
  auto r = check({1, 3, 7}, 7);                    // first element non-zero
  EXPECT(r.first.find("offsets[0]") != std::string::npos && r.second == 0);
  r = check({0, 5, 4, 7}, 7);                      // a decrease: bag 1 is [5, 4)
  EXPECT(r.first.find("decrease") != std::string::npos && r.second == 1);
  r = check({0, 3, 6}, 7);                         // last element below n
  EXPECT(r.first.find("offsets[nbags]") != std::string::npos && r.second == 1);
  r = check({0, 3, 9}, 7);                         // last element above n: bag 1 ends past the keys
  EXPECT(!r.first.empty() && r.second == 1);
  r = check({0, 9, 9, 9}, 7);                      // the FIRST bad bag is named
  EXPECT(!r.first.empty() && r.second == 0);
  r = check({0, 0, 0}, 1);                         // all empty but n > 0
  EXPECT(r.first.find("offsets[nbags]") != std::string::npos && r.second == 1);
  r = check({0, ~0ull, 0}, 0);
  EXPECT(!r.first.empty() && r.second == 0);
}

// Every ordering of o_b, o_b+1 and n around each other, with the values that
// wrap a careless o + 1 or o1 - o0.
static void test_clamp() {
  const uint64_t vals[] = {0, 1, 2, 5, 6, 7, 1000, (1ull << 63), ~0ull - 1, ~0ull};
  for (uint64_t o0 : vals)
    for (uint64_t o1 : vals)
      for (uint64_t n : vals) {
        const PoolBag b = pool_clamp(o0, o1, n);
        EXPECT(b.begin <= b.end && b.end <= n);
        EXPECT(b.begin == std::min(o0, n));
        EXPECT(b.end == std::min(std::max(o1, o0), n));
        if (o0 <= o1 && o1 <= n) EXPECT(b.begin == o0 && b.end == o1);  // well formed: untouched
        if (o1 < o0) EXPECT(b.begin == b.end);                         // a decrease: an empty bag
      }
}

// The chunks of a bag: a function of its length alone; they tile [0, m) in
// order, every chunk but the last is kPoolChunk long, none is empty.
static void test_chunks() {
  EXPECT(pool_chunks(0) == 1 && pool_chunks(1) == 1 && pool_chunks(C - 1) == 1 && pool_chunks(C) == 1);
  EXPECT(pool_chunks(C + 1) == 2 && pool_chunks(2 * C) == 2 && pool_chunks(2 * C + 1) == 3);
  EXPECT(pool_chunks(100000) == (100000 + C - 1) / C);
  for (uint64_t m : {C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 7 * C + 5, (uint64_t)50000}) {
    // the same chunks wherever the bag begins: chunk c of a bag at b0 covers
    // positions b0 + [c C, min((c+1) C, m))
    for (uint64_t b0 : {(uint64_t)0, (uint64_t)1, C - 1, C, C + 1, 12345 * C + 77}) {
      uint64_t covered = 0;
      for (uint64_t c = 0; c < pool_chunks(m); ++c) {
        const uint64_t p0 = b0 + c * C, p1 = std::min(p0 + C, b0 + m);
        EXPECT(p0 - b0 == covered && p1 > p0);
        EXPECT(p1 - p0 == C || c + 1 == pool_chunks(m));
        covered += p1 - p0;
        // the window the chunk starts in finds it, no other window does
        const uint64_t q = p0 / C;
        EXPECT(pool_window_chunk(b0, b0 + m, q) == c);
        if (q > 0) EXPECT(pool_window_chunk(b0, b0 + m, q - 1) != c);
        EXPECT(pool_window_chunk(b0, b0 + m, q + 1) != c);
      }
      EXPECT(covered == m);
    }
  }
  // not long: no chunk in any window
  for (uint64_t m : {(uint64_t)0, (uint64_t)1, C - 1, C})
    for (uint64_t q = 0; q < 4; ++q) EXPECT(pool_window_chunk(C / 2, C / 2 + m, q) == kPoolNone);
  EXPECT(pool_window_chunk(10, 5, 0) == kPoolNone);  // (never produced by the clamp)
}

// What k_row_pooled_chunks does, on the host: per window, the bags that hold
// its first and its last position.  Every chunk of every long bag is found
// exactly once, in its own slot below pool_slots(n).
static void simulate(const std::vector<uint64_t>& lens) {
  std::vector<uint64_t> off(1, 0);
  for (uint64_t m : lens) off.push_back(off.back() + m);
  const uint64_t n = off.back(), nbags = lens.size();
  uint64_t bad = 0;
  EXPECT(pool_offsets_error(off.data(), nbags, n, &bad) == nullptr);
  std::set<std::pair<uint64_t, uint64_t>> found;  // (bag, chunk)
  std::set<uint64_t> slots;
  const uint64_t nwin = (n + C - 1) / C;
  for (uint64_t q = 0; q < nwin; ++q) {
    const uint64_t lo = q * C, hi = std::min(lo + C, n) - 1;
    const uint64_t ba = pool_bag_of(off.data(), nbags, lo), bb = pool_bag_of(off.data(), nbags, hi);
    EXPECT(ba < nbags && bb < nbags);
    EXPECT(off[ba] <= lo && lo < off[ba + 1] && off[bb] <= hi && hi < off[bb + 1]);
    for (int cand = 0; cand < 2; ++cand) {
      if (cand == 1 && bb == ba) break;
      const uint64_t bag = cand ? bb : ba;
      const PoolBag bg = pool_clamp(off[bag], off[bag + 1], n);
      const uint64_t c = pool_window_chunk(bg.begin, bg.end, q);
      if (c == kPoolNone) continue;
      EXPECT(found.insert({bag, c}).second);
      const uint64_t slot = pool_slot(bg.begin, c);
      EXPECT(slot < pool_slots(n) && slot / 2 == q && slot % 2 == (uint64_t)cand);
      EXPECT(slots.insert(slot).second);
    }
  }
  size_t want = 0;
  for (uint64_t b = 0; b < nbags; ++b) {
    if (lens[b] <= C) continue;
    for (uint64_t c = 0; c < pool_chunks(lens[b]); ++c) {
      ++want;
      EXPECT(found.count({b, c}) == 1);
    }
  }
  EXPECT(found.size() == want);
}

static void test_windows() {
  simulate({C + 1});
  simulate({C, C + 1, C - 1, 2 * C + 1});
  simulate({0, 0, 3 * C, 0, 0, C + 1, 0});
  simulate({1, C + 1, C + 1, C + 1});                   // a long bag ends and another begins in one window
  simulate({C - 1, 2, C + 1, 1, 4 * C});
  simulate({5, 50000, 7, 0, 50000, 3});
  std::mt19937_64 rng(7);
  for (int it = 0; it < 200; ++it) {
    std::vector<uint64_t> lens;
    const int nb = 1 + (int)(rng() % 12);
    for (int i = 0; i < nb; ++i) {
      const uint64_t kind = rng() % 5;
      lens.push_back(kind == 0 ? 0 : kind == 1 ? rng() % 9 : kind == 2 ? C - 2 + rng() % 5 : rng() % (5 * C));
    }
    uint64_t n = 0;
    for (uint64_t m : lens) n += m;
    if (n) simulate(lens);
  }
}

// Malformed (device) offsets: whatever they hold, the bag the search returns
// is a bag, and every position and slot the kernels would touch is in bounds.
static void test_malformed() {
  std::mt19937_64 rng(11);
  for (int it = 0; it < 300; ++it) {
    const uint64_t nbags = 1 + rng() % 10, n = rng() % (6 * C);
    std::vector<uint64_t> off(nbags + 1);
    for (auto& o : off) o = (rng() % 4 == 0) ? rng() : rng() % (8 * C);
    const uint64_t nwin = (n + C - 1) / C;
    for (uint64_t q = 0; q < nwin; ++q) {
      const uint64_t lo = q * C, hi = std::min(lo + C, n) - 1;
      for (uint64_t x : {lo, hi}) {
        const uint64_t bag = pool_bag_of(off.data(), nbags, x);
        EXPECT(bag < nbags);
        const PoolBag bg = pool_clamp(off[bag], off[bag + 1], n);
        const uint64_t c = pool_window_chunk(bg.begin, bg.end, q);
        if (c == kPoolNone) continue;
        const uint64_t p0 = bg.begin + c * C, p1 = std::min(p0 + C, bg.end);
        EXPECT(p0 < p1 && p1 <= n && pool_slot(bg.begin, c) < pool_slots(n));
      }
    }
    for (uint64_t b = 0; b < nbags; ++b) {
      const PoolBag bg = pool_clamp(off[b], off[b + 1], n);
      EXPECT(bg.begin <= bg.end && bg.end <= n);
      if (bg.end - bg.begin > C)
        for (uint64_t c = 0; c < pool_chunks(bg.end - bg.begin); ++c)
          EXPECT(pool_slot(bg.begin, c) < pool_slots(n));
    }
  }
}

int main() {
  test_offsets_check();
  test_clamp();
  test_chunks();
  test_windows();
  test_malformed();
  std::printf("pooled_plan_test: %d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
