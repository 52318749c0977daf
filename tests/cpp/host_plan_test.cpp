// CPU unit test of the host planner (parameter_server_amd/csrc/pskv_plan.h):
// pieces, launch groups, staging layouts, DMA / copy windows, the vectorised
// key check with its combination across pieces, and K5's bucket rule -- the
// places where an off-by-one at 64 batches, 2^31 or 2^32 elements or a 16-byte
// boundary would hide.  Host-only: no HIP, no GPU.  Batches with fake pointers
// are never dereferenced.
#include <cstdio>
#include <initializer_list>
#include <random>
#include <set>
#include <utility>
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

static const uintptr_t kFakeKeys = 0x100000000000ull, kFakeVals = 0x400000000000ull;
static pskv_batch fake(uint64_t n, uint64_t i = 0) {
  return pskv_batch{reinterpret_cast<const uint32_t*>(kFakeKeys + (i << 36)),
                    reinterpret_cast<void*>(kFakeVals + (i << 40)), n};
}
static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

static void test_push_pieces() {
  for (size_t vb : {size_t(4), size_t(8), size_t(3 * 4), size_t(5 * 8)}) {
    for (uint64_t n : {0ull, 1ull, 1ull << 31, (1ull << 31) + 1, (1ull << 32) + (1ull << 20)}) {
      const pskv_batch b = fake(n);
      std::vector<pskv_batch> v;
      push_pieces(v, b, vb);
      EXPECT(v.size() == (n + kMaxPiece - 1) / kMaxPiece);
      uint64_t off = 0;
      for (const auto& p : v) {
        EXPECT(p.n >= 1 && p.n <= kMaxPiece);
        EXPECT(addr(p.keys) == addr(b.keys) + off * 4);
        EXPECT(addr(p.vals) == addr(b.vals) + off * vb);
        off += p.n;
      }
      EXPECT(off == n);
    }
  }
}

// Groups / windows are consecutive, non-empty and cover [0, n).
static bool covers(const std::vector<Span>& g, size_t n) {
  size_t at = 0;
  for (const auto& s : g) {
    if (s.first != at || s.second <= s.first) return false;
    at = s.second;
  }
  return at == n;
}
static uint64_t elems_of(const std::vector<pskv_batch>& v, const Span& s) {
  uint64_t el = 0;
  for (size_t i = s.first; i < s.second; ++i) el += v[i].n;
  return el;
}

static void check_groups(const std::vector<pskv_batch>& v, size_t want_groups) {
  const std::vector<Span> g = split_groups(v);
  EXPECT(covers(g, v.size()));
  EXPECT(g.size() == want_groups);
  for (size_t k = 0; k < g.size(); ++k) {
    EXPECT(g[k].second - g[k].first <= 64);
    EXPECT(elems_of(v, g[k]) < (1ull << 32));
    // greedy: the next batch did not fit
    if (g[k].second < v.size())
      EXPECT(g[k].second - g[k].first == 64 || elems_of(v, g[k]) + v[g[k].second].n >= (1ull << 32));
  }
}

static void test_split_groups() {
  EXPECT(kMaxBatches == 64);
  EXPECT(split_groups({}).empty());
  for (size_t nb : {size_t(1), size_t(64), size_t(65), size_t(150)}) {
    std::vector<pskv_batch> v;
    for (size_t i = 0; i < nb; ++i) v.push_back(fake(1, i));
    check_groups(v, (nb + 63) / 64);
  }
  {
    std::vector<pskv_batch> v(5, fake(1ull << 31));  // 2^31 + 2^31 = 2^32 does not fit
    check_groups(v, 5);
  }
  {
    std::vector<pskv_batch> v = {fake(1ull << 31), fake((1ull << 31) - 1), fake(1), fake(1ull << 31)};
    check_groups(v, 2);  // 2^32 - 1 fits; the next key does not
  }
  // the limits as parameters
  std::vector<pskv_batch> v(10, fake(7));
  const std::vector<Span> g = split_groups(v, 3, 15);
  EXPECT(covers(g, v.size()) && g.size() == 5);
  for (const auto& s : g) EXPECT(s.second - s.first == 2);
}

static void test_layout() {
  const uint64_t ns[] = {0, 1, 3, 4, 5};
  std::vector<std::vector<pskv_batch>> lists;
  lists.push_back({});
  for (uint64_t n : ns) lists.push_back({fake(n)});
  {
    std::vector<pskv_batch> all, rev;
    for (uint64_t n : ns) all.push_back(fake(n));
    for (int i = 4; i >= 0; --i) rev.push_back(fake(ns[i]));
    lists.push_back(all);
    lists.push_back(rev);
    for (uint64_t a : ns)
      for (uint64_t b : ns) lists.push_back({fake(a), fake(b), fake(a)});
  }
  for (size_t vb : {size_t(4), size_t(8), size_t(12), size_t(40)}) {
    for (const auto& v : lists) {
      for (StageOrder order : {StageOrder::kInterleaved, StageOrder::kKeysFirst}) {
        const StageLayout l = stage_layout(v, vb, order);
        EXPECT(l.at.size() == v.size());
        // every range as [start, padded end): aligned, disjoint, ending at total
        std::vector<std::pair<size_t, size_t>> r;
        size_t kb = 0;
        for (size_t i = 0; i < v.size(); ++i) {
          r.emplace_back(l.at[i].keys, l.at[i].keys + round16(v[i].n * 4));
          r.emplace_back(l.at[i].vals, l.at[i].vals + round16(v[i].n * vb));
          kb += round16(v[i].n * 4);
          EXPECT(v[i].n * 4 <= round16(v[i].n * 4) && v[i].n * vb <= round16(v[i].n * vb));
        }
        size_t end = 0;
        for (size_t a = 0; a < r.size(); ++a) {
          EXPECT(r[a].first % 16 == 0);
          end = std::max(end, r[a].second);
          for (size_t b = a + 1; b < r.size(); ++b)
            EXPECT(r[a].second <= r[b].first || r[b].second <= r[a].first);
        }
        EXPECT(l.total == end);
        EXPECT(l.key_bytes == kb);
        EXPECT(l.total == staged_bytes(v, vb));
        // today's formulas
        size_t off = 0, ko = 0, vo = kb;
        for (size_t i = 0; i < v.size(); ++i) {
          if (order == StageOrder::kInterleaved) {
            EXPECT(l.at[i].keys == off);
            off += round16(v[i].n * 4);
            EXPECT(l.at[i].vals == off);
            off += round16(v[i].n * vb);
          } else {
            EXPECT(l.at[i].keys == ko && l.at[i].vals == vo);
            ko += round16(v[i].n * 4);
            vo += round16(v[i].n * vb);
          }
        }
        char* base = reinterpret_cast<char*>(0x7000000000ull);
        const std::vector<pskv_batch> views = l.views(v, base);
        EXPECT(views.size() == v.size());
        for (size_t i = 0; i < v.size(); ++i)
          EXPECT(addr(views[i].keys) == addr(base) + l.at[i].keys && addr(views[i].vals) == addr(base) + l.at[i].vals &&
                 views[i].n == v[i].n);
      }
    }
  }
  EXPECT(round16(0) == 0 && round16(1) == 16 && round16(16) == 16 && round16(17) == 32);
  EXPECT(aligned16(reinterpret_cast<void*>(32)) && !aligned16(reinterpret_cast<void*>(40)));
  EXPECT(next_pow2(0) == 1 && next_pow2(1) == 1 && next_pow2(3) == 4 && next_pow2(64) == 64 && next_pow2(65) == 128);
}

// batch_windows against its three limits.
static void check_batch_windows(const std::vector<pskv_batch>& v, size_t min_key_bytes, size_t max_batches,
                                uint64_t max_elems, bool defaults) {
  const std::vector<Span> w =
      defaults ? batch_windows(v) : batch_windows(v, min_key_bytes, max_batches, max_elems);
  EXPECT(covers(w, v.size()));
  for (const auto& s : w) {
    const size_t nb = s.second - s.first;
    EXPECT(nb <= max_batches);
    EXPECT(nb == 1 || elems_of(v, s) < max_elems);
    // no batch beyond the first was taken once the keys reached the window size
    EXPECT(nb == 1 || (elems_of(v, s) - v[s.second - 1].n) * 4 < min_key_bytes);
    // closed for a reason
    if (s.second < v.size())
      EXPECT(elems_of(v, s) * 4 >= min_key_bytes || nb == max_batches ||
             elems_of(v, s) + v[s.second].n >= max_elems);
  }
}

static void test_windows() {
  EXPECT(kWindowBytes == (8u << 20));
  EXPECT(batch_windows({}).empty());
  const size_t W = kWindowBytes, B = kMaxBatches;
  const uint64_t E = 1ull << 32;
  check_batch_windows(std::vector<pskv_batch>(200, fake(1)), W, B, E, true);       // the 64-batch limit
  check_batch_windows(std::vector<pskv_batch>(65, fake(3)), W, B, E, true);
  check_batch_windows(std::vector<pskv_batch>(9, fake(1u << 20)), W, B, E, true);   // 4 MiB of keys each: pairs
  check_batch_windows(std::vector<pskv_batch>(3, fake((2u << 20) - 1)), W, B, E, true);  // one key short: 2 + 1
  check_batch_windows(std::vector<pskv_batch>(4, fake(1ull << 31)), W, B, E, true);  // alone each (also by size)
  EXPECT(batch_windows(std::vector<pskv_batch>(9, fake(1u << 20))).size() == 5);
  EXPECT(batch_windows(std::vector<pskv_batch>(3, fake((2u << 20) - 1))).size() == 2);
  EXPECT(batch_windows(std::vector<pskv_batch>(200, fake(1))).size() == 4);
  // the element limit with the byte limit out of the way
  check_batch_windows({fake(1ull << 31), fake((1ull << 31) - 1), fake(1), fake(5)}, ~size_t(0), B, E, false);
  EXPECT(batch_windows({fake(1ull << 31), fake((1ull << 31) - 1), fake(1), fake(5)}, ~size_t(0)).size() == 2);
  std::mt19937 rng(7);
  for (int t = 0; t < 200; ++t) {
    std::vector<pskv_batch> v;
    const size_t nb = 1 + rng() % 40;
    for (size_t i = 0; i < nb; ++i) v.push_back(fake(rng() % 30));
    const size_t min_key_bytes = 4 * (1 + rng() % 50), max_batches = 1 + rng() % 6;
    const uint64_t max_elems = 20 + rng() % 60;
    check_batch_windows(v, min_key_bytes, max_batches, max_elems, false);
  }
  // pieces into copy windows
  EXPECT(piece_windows({}).empty());
  for (int t = 0; t < 200; ++t) {
    std::vector<Piece> p(1 + rng() % 50);
    for (auto& x : p) {
      x = Piece{};
      x.bytes = t < 20 ? kPieceBytes : 1 + rng() % 4096;
    }
    if (t < 20) p.back().bytes = 1 + rng() % kPieceBytes;
    const size_t win = t < 20 ? kWindowBytes : 1 + rng() % 20000;
    const std::vector<Span> w = t < 20 ? piece_windows(p) : piece_windows(p, win);
    EXPECT(covers(w, p.size()));
    for (const auto& s : w) {
      size_t bytes = 0;
      for (size_t i = s.first; i < s.second; ++i) bytes += p[i].bytes;
      EXPECT(bytes - p[s.second - 1].bytes < win);          // no piece taken beyond the window size
      EXPECT(s.second == p.size() || bytes >= win);         // closed only once full
    }
    if (t < 20) EXPECT(w.size() == (p.size() + 7) / 8);
  }
}

// The plain sequential restatement of the key check over whole batches.
struct SeqCheck {
  bool sorted = true, dense = true;
  uint64_t outside = 0;
};
static SeqCheck seq_check(const std::vector<std::vector<uint32_t>>& batches, uint32_t key_begin, uint64_t range) {
  SeqCheck c;
  for (const auto& k : batches)
    for (size_t i = 0; i < k.size(); ++i) {
      if ((uint64_t)(uint32_t)(k[i] - key_begin) >= range) ++c.outside;
      if (i && k[i - 1] > k[i]) c.sorted = false;
      if (i && k[i] != (uint32_t)(k[i - 1] + 1u)) c.dense = false;
    }
  return c;
}

// Cut every batch into pieces of `cut` keys, check them (copying when `copy`)
// and compare the combination with the restatement.
static void check_against_seq(const std::vector<std::vector<uint32_t>>& batches, uint32_t key_begin, uint64_t range,
                              size_t cut, bool copy) {
  std::vector<std::vector<uint32_t>> dst(batches.size());
  std::vector<Piece> pieces;
  for (size_t j = 0; j < batches.size(); ++j) {
    dst[j].assign(batches[j].size(), 0xDEADBEEFu);
    for (size_t off = 0; off < batches[j].size(); off += cut) {
      Piece p{};
      p.src = reinterpret_cast<const char*>(batches[j].data() + off);
      p.dst = copy ? reinterpret_cast<char*>(dst[j].data() + off) : nullptr;
      p.bytes = std::min(cut, batches[j].size() - off) * 4;
      p.key_batch = (int)j;
      p.sorted = p.dense = true;
      pieces.push_back(p);
    }
    if (j % 2 == 0) {  // a values piece between the batches is skipped by the combination
      Piece p{};
      p.key_batch = -1;
      p.sorted = p.dense = false;
      p.outside = 99;
      pieces.push_back(p);
    }
  }
  uint64_t outside = 0;
  for (auto& p : pieces)
    if (p.key_batch >= 0) {
      copy_piece(p, key_begin, range);
      outside += p.outside;
    }
  bool ok = false, dense = false;
  combine_checks(pieces, &ok, &dense);
  const SeqCheck c = seq_check(batches, key_begin, range);
  EXPECT(outside == c.outside);
  EXPECT(ok == (c.sorted && c.outside == 0));
  EXPECT(dense == (c.dense && c.outside == 0));
  bool ok2 = false;
  combine_checks(pieces, &ok2, nullptr);
  EXPECT(ok2 == ok);
  if (copy) EXPECT(dst == batches);
}

static void check_all_cuts(const std::vector<std::vector<uint32_t>>& batches, uint32_t key_begin, uint64_t range) {
  for (size_t cut : {size_t(1), size_t(2), size_t(3), size_t(7), size_t(64), size_t(1000), size_t(5000)})
    check_against_seq(batches, key_begin, range, cut, cut % 2 == 0);
}

static void test_key_check() {
  // hand cases
  check_all_cuts({{5, 6, 6, 8}}, 0, 100);                 // sorted, spans n - 1 keys, not dense
  check_all_cuts({{5, 6, 6, 8}}, 5, 4);
  check_all_cuts({{5, 6, 7, 8}}, 5, 4);
  check_all_cuts({{5, 6, 7, 8}}, 5, 3);                   // the last key outside
  check_all_cuts({{5, 6, 7, 8}}, 6, 100);                 // a key equal to key_begin - 1
  check_all_cuts({{99, 100}, {100, 101}}, 100, 10);
  {
    std::vector<uint32_t> run(4000);
    for (size_t i = 0; i < run.size(); ++i) run[i] = 1000 + (uint32_t)i;  // a dense run split across pieces
    check_all_cuts({run}, 1000, 4000);
    check_all_cuts({run}, 1000, 3999);
    check_all_cuts({run, run}, 0, 1ull << 32);
    run[2000] = run[1999];  // one repeat at a piece boundary of the 1000-key cut
    check_all_cuts({run}, 1000, 4000);
    run[2000] = run[1999] + 2;
    check_all_cuts({run}, 1000, 4002);
    run[2000] = 0;
    check_all_cuts({run}, 0, 1ull << 32);
  }
  {
    // key_begin near 2^32 with a wrapping range: 0xFFFFFFF0 .. 2^32 - 1, 0 .. 15
    std::vector<uint32_t> k;
    for (uint32_t i = 0; i < 32; ++i) k.push_back(0xFFFFFFF0u + i);
    check_all_cuts({k}, 0xFFFFFFF0u, 32);
    check_all_cuts({k}, 0xFFFFFFF0u, 31);
    check_all_cuts({k}, 0xFFFFFFF1u, 32);
    check_all_cuts({{0xFFFFFFFEu, 0xFFFFFFFFu}, {0u, 1u}}, 0xFFFFFFF0u, 32);
  }
  check_all_cuts({{0u, 1u, 0xFFFFFFFFu}, {7u}}, 0, 1ull << 32);  // range = 2^32: every key inside
  check_all_cuts({{0xFFFFFFFFu, 0u}}, 12345, 1ull << 32);
  check_all_cuts({{42u}}, 42, 1);                                // range = 1
  check_all_cuts({{42u, 42u, 42u}}, 42, 1);
  check_all_cuts({{41u, 42u, 43u}}, 42, 1);
  check_all_cuts({{}, {3u}, {}}, 0, 10);
  // seeded random batches of 1 to 5000 keys
  std::mt19937 rng(12345);
  for (int t = 0; t < 120; ++t) {
    const uint32_t key_begin = t % 3 == 0 ? 0u : (uint32_t)rng();
    const uint64_t range = t % 5 == 0 ? (1ull << 32) : 1 + rng() % 20000;
    std::vector<std::vector<uint32_t>> batches(1 + rng() % 3);
    for (auto& k : batches) {
      k.resize(1 + rng() % 5000);
      const int kind = rng() % 4;  // dense window, sorted, sorted with strays, random
      uint32_t x = key_begin + (uint32_t)(rng() % range);
      for (auto& e : k) {
        if (kind == 0) e = x++;
        else if (kind == 3) e = key_begin + (uint32_t)(rng() % (2 * range));
        else e = (x += rng() % 3);
      }
      if (kind == 2) k[rng() % k.size()] = (uint32_t)rng();
    }
    const size_t cuts[] = {1, 7, 64, 1000, 5000};
    check_against_seq(batches, key_begin, range, cuts[t % 5], t % 2 == 0);
  }
  // add_pieces: copy pieces of kPieceBytes, check-only pieces of kCheckPieceBytes
  for (bool copy : {true, false}) {
    std::vector<Piece> p;
    const size_t bytes = (5u << 19) + 12;  // 2.5 MiB + 12
    const char* src = reinterpret_cast<const char*>(kFakeKeys);
    char* dst = copy ? reinterpret_cast<char*>(kFakeVals) : nullptr;
    add_pieces(p, src, dst, bytes, 3);
    add_pieces(p, src, dst, 0, 4);  // nothing
    const size_t piece = copy ? kPieceBytes : kCheckPieceBytes;
    EXPECT(p.size() == (bytes + piece - 1) / piece);
    size_t off = 0;
    for (const auto& x : p) {
      EXPECT(x.src == src + off && x.dst == (copy ? dst + off : nullptr) && x.key_batch == 3);
      EXPECT(x.bytes >= 1 && x.bytes <= piece);
      off += x.bytes;
    }
    EXPECT(off == bytes);
  }
}

static void test_bucket_rule() {
  const uint64_t ranges[] = {1, 2, 3, 2048, 2049, 500000, 100000000ull, 1000000000ull, (1ull << 31) + 5,
                             (1ull << 32) - 1, 1ull << 32};
  const uint64_t counts[] = {1, 1ull << 11, 1ull << 17, 1ull << 20, (1ull << 22) + 1, 1ull << 24, 1ull << 28,
                             (1ull << 32) - 1};
  std::set<std::pair<uint32_t, uint64_t>> seen;  // (nbd, windows) whose division was checked
  uint32_t max_nbd = 0;
  uint64_t max_win = 0;
  for (int mode : {(int)PSKV_ASSIGN, (int)PSKV_ACCUMULATE})
    for (uint64_t range : ranges)
      for (uint64_t elems : counts) {
        const RbPlan p = rb_plan(range, elems, mode, 0, 0, 0);
        const RbMap& m = p.bm;
        EXPECT(m.nbd >= 1);
        EXPECT(m.nbd + 1 <= (uint32_t)kRbMaxBuckets);
        EXPECT(m.nbd <= (mode == PSKV_ASSIGN ? 2048u : 1024u));
        EXPECT(m.wbits <= 11);
        const uint64_t windows = ((range - 1) >> m.wbits) + 1;
        EXPECT(windows <= (1ull << 21));
        EXPECT(windows >= m.nbd);  // no empty bucket by construction
        EXPECT(m.span == (uint32_t)std::min<uint64_t>(((windows + m.nbd - 1) / m.nbd) << m.wbits, 0xFFFFFFFFull));
        EXPECT(m.magic == (uint32_t)(((1ull << 32) + m.nbd - 1) / m.nbd));
        int nlog = -1;
        for (int l = 0; l < 32; ++l)
          if (m.nbd == (1u << l)) nlog = l;
        EXPECT(m.nlog == nlog);
        EXPECT(p.apply_log2 == (elems / m.nbd <= 2048 ? 13 : 14));
        // every key's local index fits the span
        EXPECT((uint64_t)m.span >= std::min<uint64_t>(((windows - 1) / m.nbd + 1) << m.wbits, 0xFFFFFFFFull));
        max_nbd = std::max(max_nbd, m.nbd);
        max_win = std::max(max_win, windows);
        if (nlog < 0 && seen.insert({m.nbd, windows}).second) {
          uint64_t bad = 0;
          for (uint64_t w = 0; w < windows; ++w) bad += ((w * m.magic) >> 32) != w / m.nbd;
          EXPECT(bad == 0);
        }
      }
  EXPECT(max_nbd == 2048 && max_win == (1ull << 21));
  EXPECT(!seen.empty());
  // the overrides (options RB_TB, RB_WBITS, RB_NBD)
  const RbPlan o = rb_plan(1ull << 20, 1ull << 20, PSKV_ASSIGN, 8, 13, 0);
  EXPECT(o.bm.nbd == 256 && o.bm.wbits == 12 && o.bm.nlog == 8);  // wbits capped by the bucket shift
  const RbPlan n = rb_plan(1ull << 20, 1ull << 20, PSKV_ASSIGN, 0, 0, 100);
  EXPECT(n.bm.nbd == 100 && n.bm.nlog == -1 && n.bm.magic == (uint32_t)(((1ull << 32) + 99) / 100));
}

// first_key_outside: the key a host row call names when it refuses its input.
static void test_first_key_outside() {
  auto first = [](const std::vector<std::vector<uint32_t>>& keys, uint32_t key_begin, uint64_t range) -> long {
    std::vector<pskv_batch> v;
    for (const auto& k : keys) v.push_back(pskv_batch{k.data(), nullptr, k.size()});
    const uint32_t* at = first_key_outside(v, key_begin, range);
    if (!at) return -1;
    // the pointer lies in one of the batches: report (batch << 16) | index
    for (size_t b = 0; b < keys.size(); ++b)
      if (!keys[b].empty() && at >= keys[b].data() && at < keys[b].data() + keys[b].size())
        return (long)((b << 16) | (size_t)(at - keys[b].data()));
    return -2;
  };
  EXPECT(first({}, 0, 10) == -1);
  EXPECT(first({{0u, 9u, 5u}, {3u}}, 0, 10) == -1);                           // no such key
  EXPECT(first({{10u, 19u}, {12u}}, 10, 10) == -1);
  EXPECT(first({{1u, 2u}, {3u, 10u, 4u, 11u}, {12u}}, 0, 10) == ((1 << 16) | 1));  // the first of several
  EXPECT(first({{9u, 20u, 21u}}, 10, 10) == 0);                               // a key equal to key_begin - 1
  EXPECT(first({{10u, 20u}}, 10, 10) == 1);                                   // a key equal to key_end
  EXPECT(first({{5u, 0x80000000u, 0xFFFFFFFFu}}, 0, 1ull << 31) == 1);        // a key >= 2^31
  EXPECT(first({{5u, 0x80000000u, 0xFFFFFFFFu}}, 0, (1ull << 31) + 1) == 2);
  EXPECT(first({{0u, 0x80000000u, 0xFFFFFFFFu}}, 0, 1ull << 32) == -1);       // range = 2^32: every key inside
  // a wrapped range whose key_begin > 0: 0xFFFFFFF0 .. 2^32 - 1, 0 .. 15
  EXPECT(first({{0xFFFFFFF0u, 0xFFFFFFFFu, 0u, 15u}}, 0xFFFFFFF0u, 32) == -1);
  EXPECT(first({{0xFFFFFFF0u, 0u, 15u, 16u, 0xFFFFFFEFu}}, 0xFFFFFFF0u, 32) == 3);
  EXPECT(first({{0xFFFFFFFFu}, {0xFFFFFFEFu}}, 0xFFFFFFF0u, 32) == (1 << 16));
  EXPECT(first({{1u}, {}, {2u, 77u}}, 0, 10) == ((2 << 16) | 1));             // an empty batch between two others
  EXPECT(first({{}, {77u}, {}}, 0, 10) == (1 << 16));
  EXPECT(first({{3u, 4u}}, 3, 0) == 0);                                       // an empty range owns nothing
}

int main() {
  test_push_pieces();
  test_split_groups();
  test_layout();
  test_windows();
  test_key_check();
  test_first_key_outside();
  test_bucket_rule();
  std::printf("host_plan_test: %d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
