// CPU unit test of the grouped pooled push's planner (parameter_server_amd/csrc/pskv_plan.h):
// the live batches of a call, their split into launch groups, the staging
// layout of a host call, and the kernels' per-position work replayed on the
// host -- the batch of a virtual workgroup (pool_group_batch_of), the bag of a
// position inside THAT batch (pool_bag_span over the batch's own last position,
// pool_bags_in), and the position's group-wide tag index, which must be the
// one K4a stamps when it is given the same batches as a plain group (keys and
// n only).  Host-only: no HIP, no GPU.
#include <cstdio>
#include <random>
#include <vector>

#include "../../parameter_server_amd/csrc/pskv_plan.h"

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

// One worker's push with real arrays behind it.
struct Push {
  std::vector<uint32_t> keys;
  std::vector<float> weights;  // empty: no weights
  std::vector<uint64_t> off;
  std::vector<float> rows;
  pskv_pool_batch view() const {
    return pskv_pool_batch{keys.data(), weights.empty() ? nullptr : weights.data(), off.data(), rows.data(),
                           (uint64_t)keys.size(), (uint64_t)off.size() - 1};
  }
};

static Push make_push(std::mt19937_64& rng, uint64_t n, uint64_t bag, bool weighted, uint32_t width) {
  Push p;
  p.off.push_back(0);
  for (uint64_t i = 0; i < n; ++i) p.keys.push_back((uint32_t)(rng() % 100000));
  if (n) p.off.push_back(0);  // an empty first bag
  for (uint64_t i = 0; i < n; i += bag) p.off.push_back(i + bag < n ? i + bag : n);
  if (weighted) p.weights.assign(n, 0.5f);
  p.rows.assign((p.off.size() - 1) * width + 1, 1.0f);  // (+ 1: data() of an empty vector may be null)
  return p;
}

static std::vector<pskv_pool_batch> views(const std::vector<Push>& pushes) {
  std::vector<pskv_pool_batch> v;
  for (const Push& p : pushes) v.push_back(p.view());
  return v;
}

// ------------------------------------------------------------ launch groups
static void test_split(size_t live_count) {
  std::mt19937_64 rng(live_count);
  std::vector<Push> pushes;
  // empty batches (no key; keys but no bag) in front of, between and behind the live ones
  for (size_t i = 0; i < live_count; ++i) {
    if (i % 3 == 0) pushes.push_back(make_push(rng, 0, 1, false, 4));
    pushes.push_back(make_push(rng, 1 + rng() % 40, 1 + rng() % 5, i % 2 == 0, 4));
    if (i % 5 == 4) {
      Push nobag = make_push(rng, 3, 1, false, 4);
      nobag.off.assign(1, 0);
      pushes.push_back(nobag);
    }
  }
  pushes.push_back(make_push(rng, 0, 1, true, 4));
  const std::vector<pskv_pool_batch> all = views(pushes);
  std::vector<uint64_t> index;
  const std::vector<pskv_pool_batch> live = pool_live_batches(all.data(), all.size(), &index);
  EXPECT(live.size() == live_count && index.size() == live_count);
  for (size_t i = 0; i < live.size(); ++i) {
    EXPECT(live[i].n > 0 && live[i].nbags > 0);
    EXPECT(all[index[i]].keys == live[i].keys);
    EXPECT(i == 0 || index[i] > index[i - 1]);
  }
  const std::vector<Span> spans = pool_split_groups(live);
  const size_t want = (live_count + kMaxPoolBatches - 1) / kMaxPoolBatches;
  EXPECT(spans.size() == want);
  size_t next = 0;
  for (const Span& sp : spans) {
    EXPECT(sp.first == next && sp.second > sp.first && sp.second - sp.first <= (size_t)kMaxPoolBatches);
    next = sp.second;
  }
  EXPECT(next == live.size());
  // every group but the last is full
  for (size_t g = 0; g + 1 < spans.size(); ++g) EXPECT(spans[g].second - spans[g].first == (size_t)kMaxPoolBatches);
}

static void test_split_by_elements() {
  // three batches of 2^31 keys: the first group takes one (2 x 2^31 is not below 2^32)
  std::vector<pskv_pool_batch> v(3, pskv_pool_batch{nullptr, nullptr, nullptr, nullptr, kMaxPiece, 1});
  const std::vector<Span> spans = pool_split_groups(v);
  EXPECT(spans.size() == 3);
  v[1].n = kMaxPiece - 1;
  const std::vector<Span> two = pool_split_groups(v);
  EXPECT(two.size() == 2 && two[0].second == 2);
  EXPECT(pool_split_groups(std::vector<pskv_pool_batch>()).empty());
}

// ----------------------------------------------------------------- staging
static void test_staging() {
  std::mt19937_64 rng(3);
  for (size_t vb : {4u, 8u})
    for (uint32_t width : {1u, 3u, 4u, 33u}) {
      std::vector<Push> pushes;
      for (int i = 0; i < 7; ++i) pushes.push_back(make_push(rng, 1 + rng() % 3000, 1 + rng() % 9, i % 2 == 1, width));
      const std::vector<pskv_pool_batch> v = views(pushes);
      const size_t rb = width * vb;
      const PoolStageLayout lay = pool_stage_layout(v, vb, rb);
      EXPECT(lay.at.size() == v.size());
      size_t end = 0;  // the ranges in staging order: each starts aligned, at or behind the previous one's end
      for (size_t i = 0; i < v.size(); ++i) {
        const PoolStageSlot& s = lay.at[i];
        EXPECT(s.keys % 16 == 0 && s.offsets % 16 == 0 && s.rows % 16 == 0);
        EXPECT(s.keys >= end);
        end = s.keys + v[i].n * 4;
        if (v[i].weights) {
          EXPECT(s.weights % 16 == 0 && s.weights >= end);
          end = s.weights + v[i].n * vb;
        }
        EXPECT(s.offsets >= end);
        end = s.offsets + (v[i].nbags + 1) * 8;
        EXPECT(s.rows >= end);
        end = s.rows + v[i].nbags * rb;
      }
      EXPECT(lay.total >= end && lay.total % 16 == 0 && lay.total < end + 16);
    }
  EXPECT(pool_stage_layout(std::vector<pskv_pool_batch>(), 4, 16).total == 0);
}

// One batch: the layout a single pooled push and a pooled pull stage by, which
// was once computed by hand in their host paths.  Those formulas are the
// expectation: keys at 0, then weights (where present), offsets of nbags + 1,
// rows of nbags * rb, each range rounded up to 16 bytes.
static void test_staging_one_batch() {
  for (uint64_t n : {1u, 3u, 4u, 5u})
    for (uint64_t nbags : {1u, 2u})
      for (bool weighted : {false, true})
        for (size_t vb : {4u, 8u})
          for (size_t rb : {4u, 12u, 16u, 24u}) {
            const float w = 0;
            const pskv_pool_batch call{nullptr, weighted ? &w : nullptr, nullptr, nullptr, n, nbags};
            const size_t wo = round16(call.n * 4);
            const size_t oo = wo + (call.weights ? round16(call.n * vb) : 0);
            const size_t ro = oo + round16((call.nbags + 1) * sizeof(uint64_t));
            const size_t total = ro + round16(call.nbags * rb);
            const PoolStageLayout lay = pool_stage_layout(std::vector<pskv_pool_batch>(1, call), vb, rb);
            EXPECT(lay.at.size() == 1);
            EXPECT(lay.at[0].keys == 0);
            EXPECT(!weighted || lay.at[0].weights == wo);
            EXPECT(lay.at[0].offsets == oo);
            EXPECT(lay.at[0].rows == ro);
            EXPECT(lay.total == total);
          }
}

// ------------------------------------- the kernels' lookup, on the host
// K4a's index of element i of batch j of a plain group over the same batches.
static uint64_t mark_index(const std::vector<pskv_batch>& marks, size_t b, size_t j, uint64_t i) {
  uint64_t e = 0;
  for (size_t q = b; q < b + j; ++q) e += marks[q].n;
  return e + i;
}

static void test_lookup(size_t live_count, uint64_t stride) {
  std::mt19937_64 rng(17 * live_count + stride);
  const uint64_t sizes[] = {1, 7, 2049, 4100, 2048, 40};
  std::vector<Push> pushes;
  for (size_t i = 0; i < live_count; ++i)
    pushes.push_back(make_push(rng, sizes[(i + live_count) % 6], 1 + rng() % 70, i % 2 == 0, 1));
  const std::vector<pskv_pool_batch> v = views(pushes);
  const std::vector<pskv_batch> marks = pool_mark_batches(v);
  for (const Span& span : pool_split_groups(v)) {
    uint32_t nwg = 0;
    uint64_t elems = 0;
    const PoolGroupArgs ga = make_pool_group(v, span.first, span.second, kChunk, &nwg, &elems);
    EXPECT(ga.nb == (int)(span.second - span.first) && ga.wg_prefix[ga.nb] == nwg);
    std::vector<std::vector<int>> seen(ga.nb);
    uint64_t total = 0;
    for (int j = 0; j < ga.nb; ++j) {
      seen[j].assign(ga.b[j].n, 0);
      total += ga.b[j].n;
      EXPECT(ga.b[j].keys == v[span.first + j].keys && ga.b[j].offsets == v[span.first + j].offsets);
      EXPECT(ga.b[j].weights == v[span.first + j].weights && ga.b[j].bag_grads == v[span.first + j].bag_grads);
    }
    EXPECT(total == elems);
    std::vector<int> tags(elems, 0);
    for (uint32_t wg = 0; wg < nwg; ++wg) {
      const int j = pool_group_batch_of(ga, wg);
      EXPECT(j >= 0 && j < ga.nb && ga.wg_prefix[j] <= wg && wg < ga.wg_prefix[j + 1]);
      const PoolBatchDesc& a = ga.b[j];
      const uint64_t base = (uint64_t)(wg - ga.wg_prefix[j]) * kChunk;
      EXPECT(base < a.n);
      const uint64_t gbase = pool_group_elem_prefix(ga, j) + base;
      const uint64_t end = base + kChunk < a.n ? base + kChunk : a.n;  // the BATCH's n bounds the span
      const PoolSpan sp = pool_bag_span(a.offsets, a.nbags, base, end - 1);
      EXPECT(sp.lo <= sp.hi && sp.hi < a.nbags);
      for (uint64_t r0 = 0; r0 < stride; ++r0)
        for (uint64_t q = base + r0; q < end; q += kRows * stride) {
          uint64_t x[kRows], bag[kRows];
          bool want[kRows];
          for (int r = 0; r < kRows; ++r) {
            x[r] = q + (uint64_t)r * stride;
            want[r] = x[r] < end;
          }
          pool_bags_in<kRows>(a.offsets, sp, x, want, bag);
          for (int r = 0; r < kRows; ++r) {
            if (!want[r]) continue;
            EXPECT(bag[r] < a.nbags && a.offsets[bag[r]] <= x[r] && x[r] < a.offsets[bag[r] + 1]);  // the true bag
            ++seen[j][x[r]];
            // the tag index: K4a's over the same batches
            const uint64_t tag = gbase + (x[r] - base);
            EXPECT(tag == mark_index(marks, span.first, (size_t)j, x[r]));
            EXPECT(tag < elems);
            if (tag < elems) ++tags[tag];
          }
        }
    }
    // every position of every batch exactly once, every tag index exactly once
    for (int j = 0; j < ga.nb; ++j)
      for (int c : seen[j]) EXPECT(c == 1);
    for (int c : tags) EXPECT(c == 1);
    // a tag without the prefix would collide with batch 0's (the hazard the prefix is there for)
    if (ga.nb > 1) EXPECT(pool_group_elem_prefix(ga, 1) == ga.b[0].n && pool_group_elem_prefix(ga, 0) == 0);
  }
}

int main() {
  for (size_t n : {(size_t)1, (size_t)kMaxPoolBatches, (size_t)kMaxPoolBatches + 1, (size_t)3 * kMaxPoolBatches})
    test_split(n);
  test_split_by_elements();
  test_staging();
  test_staging_one_batch();
  for (size_t n : {(size_t)1, (size_t)3, (size_t)5, (size_t)kMaxPoolBatches + 1})
    for (uint64_t stride : {1ull, 64ull, 256ull}) test_lookup(n, stride);
  std::printf("%d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
