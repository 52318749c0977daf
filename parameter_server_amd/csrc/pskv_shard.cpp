// pskv_shard.cpp — host side of the C ABI declared in include/pskv.h.
//
// One pskv_shard is what the reference calls a storage: the object
// Engine::CreateTable builds per server thread (driver/engine.hpp:100-109) and
// the consistency model drives through AbstractStorage::Add/Get
// (server/abstract_storage.hpp:14-32).  Here it owns a dense HBM array for its
// key range, an overflow hash table for every other key, a stream, and
// pinned/device staging for host (zmq-buffer) inputs.
//
// Call flow of an assign-mode Add:
//   small host messages → K8 (kernarg-carried) or the K9 request server.
//   host inputs   → copy into pinned staging (or DMA / read in place when
//                   page-locked) while checking "sorted and in range" on the
//                   CPU → K2 / K2g if verified, else K5.
//   device inputs → PSKV_SORTED_HINT: K2 (one batch) or K2g (group), each
//                   verifying on device, followed by the one-workgroup K4r
//                   replay, which exits at once unless the verification
//                   tagged the call.  No hint: K5 (key buckets).
// Accumulate-mode Add: K6 density proof + K7 for dense windows, else K5.
// Get: K1 (one launch per group of <= 64 batches), K8 for small messages.
//
// This file is the policy: which path a call takes, what it queues and in
// which order, and what it waits for.  The arithmetic underneath -- pieces,
// launch groups, staging layout, DMA windows, the key check, K5's bucket rule
// -- is the host planner, pskv_plan.h (no HIP, tested on the CPU).  The hold
// on the pinned staging buffer is a scope guard (HstageHold), not a call on
// each error exit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pskv.h"
#include "pskv_frames.h"
#include "pskv_internal.h"
#include "pskv_plan.h"
#include "pskv_queues.h"

using namespace pskv;

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define PSKV_HIP(call)                                                                     \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(PSKV_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
  } while (0)

int value_bytes(int dtype) {
  switch (dtype) {
    case PSKV_I32:
    case PSKV_F32:
      return 4;
    case PSKV_F64:
      return 8;
    default:
      return 0;
  }
}

constexpr uint64_t kDefaultOverflowSlots = 1ull << 16;
// see tune_dma_min_bytes: measured per call (tools/micro/small_latency.cpp,
// f64): Add via the pinned copy 6-7 us up to 4 Ki keys, 338 us at 1 Mi keys
// (direct DMA 48 / 366 us), DMA ahead from ~4 Mi keys; Get via the copy 18 us
// up to 2 Ki keys (DMA 26), DMA ahead from 4 Ki keys
constexpr size_t kDefaultDmaMinBytes = 32ull << 20;
constexpr size_t kDefaultDmaMinBytesGet = 32ull << 10;
// Option RESIDENT_BYTES (DESIGN.md §7 "Resident window").  kResidentAutoBytes:
// what auto (-1) keeps resident of a dense array larger than itself.  The
// headline sweep (profiles/resident_window/sweep.txt): 128 MiB and less lose or
// gain nothing, 224-256 MiB gain 2.3 %, 288 MiB loses 1 %; 224 leaves the
// 256 MiB cache some room for what else runs.
constexpr uint64_t kResidentAutoBytes = 224ull << 20;
constexpr int64_t kResidentDefault = -1;

struct TimedLaunch {
  int kernel;
  hipEvent_t a, b;
  uint64_t elems;
  uint64_t count = 1;  // operations the bracket stands for (an optimizer step: its launch groups)
};

// Timing slots: the kernels of enum pskv_kernel, then one slot for a whole
// optimizer step (pskv_apply_time; PSKV_TIME_APPLY is its mask bit) and one for
// a whole pooled pull (pskv_pooled_time; PSKV_TIME_POOLED).
constexpr int kTimeApply = PSKV_K_COUNT;
constexpr int kTimePooled = PSKV_K_COUNT + 1;
constexpr int kTimeIndex = PSKV_K_COUNT + 2;  // a sparse shard's index launches of one call (pskv_index_time)
constexpr int kTimeSlots = PSKV_K_COUNT + 3;
static_assert(PSKV_TIME_APPLY == (1u << kTimeApply), "the apply slot follows the kernel ids");
static_assert(PSKV_TIME_APPLY == (1u << 14), "the apply slot's bit is part of the interface");
static_assert(PSKV_TIME_POOLED == (1u << kTimePooled), "the pooled slot follows the apply slot");
static_assert(PSKV_TIME_INDEX == (1u << kTimeIndex), "the index slot follows the pooled slot");

// ---------------------------------------------------------------- host pool
// A small persistent pool for the host side of the path: copying zmq-buffer
// inputs into pinned staging (with the sorted/in-range check) and pinned
// outputs back to the caller.  One parallel section at a time; the caller
// thread works too.  Size: PSKV_HOST_THREADS (default min(8, cores)).
class HostPool {
 public:
  static HostPool& get() {
    static HostPool p;
    return p;
  }
  size_t size() const { return workers_.size() + 1; }
  // Runs fn(0..n-1), blocking until all are done.
  void run(size_t n, const std::function<void(size_t)>& fn) {
    if (n == 0) return;
    if (n == 1 || workers_.empty()) {
      for (size_t i = 0; i < n; ++i) fn(i);
      return;
    }
    std::lock_guard<std::mutex> section(section_);
    Job job(&fn, n);
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = &job;
      ++gen_;
    }
    cv_.notify_all();
    work(job);
    std::unique_lock<std::mutex> lk(m_);
    // a worker that joined late may still hold the job: wait for it to let go
    done_.wait(lk, [&] { return job.left == 0 && job.refs == 0; });
    job_ = nullptr;
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
      ++gen_;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }

 private:
  // One parallel section; lives on the stack of run() until every index is
  // done and no worker references it.
  struct Job {
    Job(const std::function<void(size_t)>* f, size_t count) : fn(f), n(count), left(count) {}
    const std::function<void(size_t)>* fn;
    size_t n;
    std::atomic<size_t> next{0};
    size_t left;  // guarded by m_
    int refs = 0;  // workers inside work(*this), guarded by m_
  };
  HostPool() {
    unsigned hw = std::thread::hardware_concurrency();
    unsigned n = std::min(8u, hw ? hw : 1u);
    if (const char* e = std::getenv("PSKV_HOST_THREADS")) n = (unsigned)std::max(1, std::atoi(e));
    for (unsigned i = 1; i < n; ++i) workers_.emplace_back([this] { loop(); });
  }
  void work(Job& j) {
    for (;;) {
      const size_t i = j.next.fetch_add(1);
      if (i >= j.n) return;
      (*j.fn)(i);
      std::lock_guard<std::mutex> lk(m_);
      if (--j.left == 0) done_.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      Job* j;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
        j = job_;
        if (!j) continue;
        ++j->refs;
      }
      work(*j);
      std::lock_guard<std::mutex> lk(m_);
      if (--j->refs == 0 && j->left == 0) done_.notify_all();
    }
  }
  std::vector<std::thread> workers_;
  std::mutex section_, m_;
  std::condition_variable cv_, done_;
  Job* job_ = nullptr;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

constexpr size_t kInlineCopyBytes = 256 << 10;  // smaller windows are copied by the calling thread

// Run fn over pieces [b, e) of `pieces`: on the calling thread when they are
// small (waking the pool costs more than copying a few hundred KiB), on the
// pool otherwise.
template <typename PieceT, typename Fn>
void run_pieces(std::vector<PieceT>& pieces, size_t b, size_t e, const Fn& fn) {
  size_t bytes = 0;
  for (size_t i = b; i < e; ++i) bytes += pieces[i].bytes;
  if (bytes < kInlineCopyBytes) {
    for (size_t i = b; i < e; ++i) fn(pieces[i]);
    return;
  }
  HostPool::get().run(e - b, [&](size_t t) { fn(pieces[b + t]); });
}

}  // namespace

struct pskv_shard {
  int device = 0;
  int dtype = PSKV_F32;
  int mode = PSKV_ASSIGN;
  int vb = 4;
  uint32_t width = 1;  // values per key; > 1: a row shard (the rows_* paths below, pskv_rows.hip)
  uint32_t key_begin = 0;
  uint64_t range = 0;
  void* dense = nullptr;
  unsigned long long* owner = nullptr;  // u64 stamps, allocated on first general-path use
  // overflow table: the control block (device memory; the kernels' argument),
  // its growth mailbox (coherent page-locked), the table as of the last
  // adoption (read_overflow_stat) and every table array set allocated for this
  // shard, by the host or by the grow service (freed once superseded and the
  // stream is idle).  tab_m guards `tables` (the service appends to it).
  Ovf ovf{};
  OvfMbox* mbox = nullptr;
  OvfTab cur{};
  std::mutex tab_m;
  std::vector<OvfTab> tables;
  uint32_t mbox_served = 0;  // grow service: number of the last request answered
  uint64_t ocap = 0;
  uint64_t ocount_known = 0;
  // device words: [0] verification tag
  uint32_t* flag = nullptr;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  uint32_t epoch = 0;
  // staging for host inputs/outputs
  void* hstage = nullptr;
  size_t hstage_bytes = 0;
  hipEvent_t hstage_free = nullptr;
  bool hstage_pending = false;
  hipEvent_t h2d_done = nullptr;  // pinned caller buffers: their DMA has completed
  void* dstage = nullptr;
  size_t dstage_bytes = 0;
  std::vector<hipEvent_t> win_events;  // per-window D2H completion (pull to host)
  // page-locked Get: values DMA'd out on their own stream, window by window
  hipStream_t out_stream = nullptr;
  std::vector<hipEvent_t> out_events;
  // timing
  uint32_t timing_mask = 0;  // bit k: bracket kernel k with events
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> event_pool;
  uint64_t t_launches[kTimeSlots] = {};
  double t_ms[kTimeSlots] = {};
  uint64_t t_elems[kTimeSlots] = {};
  // stats
  uint64_t n_add = 0, n_get = 0, n_sorted = 0, n_general = 0;
  // K5 radix-bucket scratch (grown on demand)
  uint16_t* rb_loff = nullptr;
  size_t rb_loff_bytes = 0;
  void* rb_ent = nullptr;
  size_t rb_ent_bytes = 0;
  // pooled pulls: the partial rows of long bags' chunks (grown on demand, as
  // the K5 scratch: a steady workload allocates nothing)
  void* pool_part = nullptr;
  size_t pool_part_bytes = 0;
  int general_path = 1;  // PSKV_GENERAL: stamps = 0 (K4 always), auto = 1, radix = 2 (K5 always)
  // tuning knobs (environment, read at creation): PSKV_TILE_SHIFT, PSKV_TILE_GRID
  uint32_t tune_tile_shift = 0;
  // grid cap of K2g / K7: one workgroup per dense-mode chunk up to 512 Mi keys
  // (round 4: at 4096 a workgroup took two of cfg 2's 8192 chunks, K2g 112.7
  // against 111.4 us; 2048 / 1024: 116.5 / 117.3; profiles/r04_probes/k2g_tune/)
  uint32_t tune_tile_grid = 65536;
  int tune_unroll = 8;   // PSKV_UNROLL: 4 or 8 (8: measured +5 % on the dense Add)
  int tune_get_unroll = 0;  // PSKV_GET_UNROLL: K1's keys per lane, 4 or 8, 0 = by launch size
  bool tune_nt = true;   // PSKV_NT: non-temporal streams (measured +12-15 % on K1 / K2g)
  // PSKV_NTP: non-temporal parameter stores in the dense Add (K2g).  On
  // since round 4: cached stores leave the Add's parameter lines dirty in the
  // Infinity Cache, and the next Get pays their write-back; the headline step
  // 5.74-5.86 -> 6.11-6.22 TB/s, its Get (K1) 114-116 -> 91 us
  // (profiles/r04_probes/ntp_ab/)
  bool tune_ntp = true;
  int tune_early = 2;    // PSKV_EARLY: K2g early loads (0 never, 1 always, 2 when the group's keys cover < 1/4 of the range)
  // PSKV_PAGEABLE_DMA: DMA pageable host buffers directly (the runtime moves
  // them at the PCIe rate, measured 55 GB/s) instead of copying them into
  // pinned staging first; 0 selects the staging path.  cfg-2-shaped Add of
  // 8 x 1M keys: 1.43 ms against 1.75 ms staged, Get 1.37 against 1.44 ms.
  bool tune_pageable_dma = true;
  // PSKV_DMA_MIN_BYTES / PSKV_DMA_MIN_BYTES_GET: pageable host Adds / Gets of
  // at least this many bytes (keys + values) take the direct DMA; smaller ones
  // the pinned staging copy
  size_t tune_dma_min_bytes = kDefaultDmaMinBytes;
  size_t tune_dma_min_bytes_get = kDefaultDmaMinBytesGet;
  // PSKV_DMA_MIN_BYTES_PINNED: page-locked host Adds of at least this many
  // bytes are DMA'd straight from the caller's buffers (and wait for it);
  // smaller ones take the pinned staging copy, which returns before its DMA.
  // Measured (tools/micro/small_latency.cpp, f64): 16 Ki keys 9 us copied
  // against 29 us DMA'd, 256 Ki keys 95 against 90
  size_t tune_dma_min_bytes_pinned = 2ull << 20;
  // PSKV_ZC_MAX_BYTES: pageable host Gets of at most this many bytes (keys +
  // values) past the inline size go zero-copy through pinned staging (0: off).
  // Measured (tools/micro/small_latency.cpp, f64): 4 Ki keys 18 us, 16 Ki 23,
  // 64 Ki 43 against 28 / 40 / 63 us by DMA; DMA ahead at 256 Ki (101 vs 152)
  size_t tune_zc_max_bytes = 1ull << 20;
  // PSKV_FRAME_ZC_MAX_BYTES: PSKV_HOST_FRAME Adds and page-locked Gets of at
  // most this many bytes (keys + values) run the kernels on the host buffers
  // in place; larger ones DMA
  size_t tune_frame_zc_max_bytes = 8ull << 20;
  uint32_t tune_rb_tb = 0; // PSKV_RB_TB: K5 bucket bits (0 = by element count)
  uint32_t tune_rb_wbits = 0; // PSKV_RB_WBITS: K5 window bits (0 = 11; >= bucket shift: contiguous buckets)
  uint32_t tune_rb_nbd = 0;   // PSKV_RB_NBD: K5 dense bucket count (0 = by the rule; tuning)
  // PSKV_INLINE: host calls of <= kInlineMax (Add) / kInlineGetMax (Get) keys in
  // all travel inside the kernel arguments (K8); 0 sends them through staging
  bool tune_inline = true;
  // PSKV_INLINE_ADD_CHUNKS / PSKV_INLINE_GET_CHUNKS: K8 launches per call at
  // most (1..kInlineMaxChunks).  Measured (tools/micro/small_latency.cpp): an
  // Add launch costs ~3-7 us of enqueue, and the pinned staging copy returns
  // in 6-8 us up to 4 Ki keys (its DMA and kernels run on), so one launch;
  // a Get launch beyond the first ~4-12 us against ~20 us through the copy
  // (1024 keys: 16 us), so up to 2 (1024 keys).
  int tune_inline_add_chunks = 1;
  int tune_inline_get_chunks = 2;
  void* ireply = nullptr;  // page-locked reply buffer of inline Gets (kInlineGetMax values)
  bool tune_ispin = true;  // PSKV_ISPIN: poll the reply's sequence word instead of a stream wait
  unsigned int ireply_seq = 0;
  int tune_rb_apply_log2 = 0; // PSKV_RB_APPLY_LOG2: 13 or 14 (0 = by bucket size)
  int tune_rb_bin_block = kRbBinBlockDefault;  // PSKV_RB_BIN_BLOCK: K5a workgroup, 512 or 1024
  // K9 request server (PSKV_SERVE=1): the inline-size messages go to a ring in
  // coherent page-locked memory that one resident workgroup polls
  // (PSKV_SERVE_IDLE_US: it leaves after this long without a request)
  bool tune_serve = false;
  uint32_t tune_serve_idle_us = 20000;
  SrvRing* srv = nullptr;
  uint32_t srv_gen = 0;  // launch generation (the kernel stores it in ring->started on entry)
  hipStream_t srv_stream = nullptr;
  hipEvent_t srv_dep = nullptr;  // the shard's stream up to the server's launch
  bool srv_running = false;
  uint32_t srv_posted = 0;
  unsigned long long srv_idle_ticks = 0;
  bool counted = false;  // in g_queues (pskv_queues.h)
  bool add_chunks_set = false;  // INLINE_ADD_CHUNKS chosen explicitly
  int wall_khz = 0;             // device wall-clock rate (the server's idle timer)
  // bounded host waits (round 5): PSKV_SYNC_TIMEOUT_MS, 0 = unbounded.  A wait
  // for the shard's stream, an event or the request server that outlasts it
  // fails the call with PSKV_ESTATE naming what it waited for; nothing is
  // restarted.  The longest legitimate wait measured (one 2^32 + 2^20-key
  // unhinted batch) is ~1.4 s.
  uint32_t tune_sync_timeout_ms = 120000;
  int last_kernel = -1;           // the last kernel this shard queued (PSKV_K_*), for the report
  uint64_t launches = 0;          // kernels this shard queued
  hipEvent_t sync_ev = nullptr;   // marks the end of a stream for a bounded wait
  uint32_t* stat_host = nullptr;  // page-locked read-back of the overflow table's {count, err}
  // pskv_add_get_grouped (round 5): the Add's last conditional replay (K4r)
  // held back and folded into the Get's first K1 launch (K1r) instead of a
  // launch of its own; option FOLD_REPLAY
  int tune_fold_replay = 1;
  bool defer_replay = false;  // inside add_get: replay() holds the group instead of launching
  bool pend_replay = false;   // a held replay: pend_rg, pend_epoch, pend_elems
  ReplayGroup pend_rg{};
  uint32_t pend_epoch = 0;
  uint64_t pend_elems = 0;
  // optimizer (pskv_shard_set_optimizer): the configuration, the gradient
  // scratch (shaped as the dense array, zero between calls) and the kind's
  // state slots (Adagrad h; momentum v; Adam m, v); all allocated when the
  // optimizer is set.  opt_step: steps since creation, clear or a kind change.
  pskv_optimizer_cfg opt{};  // (its first 72 bytes are a pskv_optimizer_ex)
  void* opt_gsum = nullptr;
  void* opt_slot[2] = {nullptr, nullptr};  // the first opt_slots(opt.kind) are allocated
  uint64_t opt_step = 0;

  // A sparse shard (pskv_shard_create_sparse): the row shard
  // [0, range) over SLOT numbers, range = the capacity, behind a hash index
  // from keys to slots (pskv_index.hip).  Every row-shaped array holds one row
  // more than `range`: row `range` stays zero and is what an absent key reads.
  // The slot counter and the full bit live in ovf.c->stat (SparseIndex).
  bool sparse = false;
  unsigned long long* sp_table = nullptr;
  uint32_t* sp_slot_keys = nullptr;
  uint64_t sp_table_slots = 0;
  void* sp_ids = nullptr;  // a device call's slot ids (grown on demand, as the K5 scratch)
  size_t sp_ids_bytes = 0;
  // Growth (pskv_sparse_set_growth).  sp_max_capacity: writing
  // calls may grow the shard up to it (0: fixed).  sp_bound: an upper bound of
  // the keys stored after everything queued -- the count at the last read-back
  // plus the key positions of every writing call since (kept while growth is on).
  uint64_t sp_max_capacity = 0;
  uint64_t sp_bound = 0;
  uint64_t sp_rebuilds = 0;  // rebuilds of the index done (reserve, automatic growth, erase)
  uint64_t rows_held() const { return range + (sparse ? 1u : 0u); }  // rows of every row-shaped array
  // The row-shaped arrays, described once: the parameters, the two state
  // slots, the gradient scratch.  `used`: the current kind has the array;
  // `start`: the value a fresh row of it holds.
  struct RowArray { void** p; bool used; double start; };
  static constexpr int kRowArrays = 4;
  RowArray row_array(int a) {
    if (a == 0) return RowArray{&dense, true, 0.0};
    if (a == 3) return RowArray{&opt_gsum, opt.kind != PSKV_OPT_NONE, 0.0};
    return RowArray{&opt_slot[a - 1], a - 1 < opt_slots(opt.kind),
                    opt_slot_is_accum(opt.kind, a - 1) ? opt.init_accum : 0.0};
  }
  RowArray row_array(int a) const { return const_cast<pskv_shard*>(this)->row_array(a); }  // (for readers of used / start)
  SparseIndex sindex() const {
    return SparseIndex{sp_table, sp_slot_keys, ovf.c->stat, sp_table_slots - 1, (uint32_t)range};
  }
  // The array `arr` (the dense array or a state array) as a reading call sees
  // it: a sparse shard's translate pass sends absent keys to the zero row.
  DenseView read_view(void* arr) const {
    return DenseView{arr, key_begin, rows_held(), arr == dense ? resident_bytes() / (uint64_t)vb : 0};
  }

  // PSKV_RESIDENT_BYTES: the resident window, bytes of the dense
  // array from its start that K2g's dense mode and K1 / K1r keep in the
  // Infinity Cache (plain stores and loads inside, non-temporal ones outside).
  // -1 = auto (resident_bytes() below), 0 = off, else bytes (clamped to the
  // array).  The budget is this shard's alone: shards busy on one device at
  // the same time share the cache and should have the option set explicitly.
  int64_t tune_resident_bytes = kResidentDefault;

  // The effective window in bytes.  Auto: none for an array the cache holds
  // anyway (at most the budget), else the budget.  Row shards have none (the
  // row kernels do not look at it).
  uint64_t resident_bytes() const {
    if (width != 1 || sparse) return 0;
    const uint64_t bytes = range * (uint64_t)vb;
    if (tune_resident_bytes < 0) return bytes <= kResidentAutoBytes ? 0 : kResidentAutoBytes;
    return std::min<uint64_t>((uint64_t)tune_resident_bytes, bytes);
  }
  DenseView dview() const { return DenseView{dense, key_begin, range, resident_bytes() / (uint64_t)vb}; }
};

namespace {

// K1's keys per lane (8 x 4 or 4 x 4, i.e. 8 Ki- or 4 Ki-key chunks) for a
// launch of `elems` keys.  Option GET_UNROLL: 4 or 8, or 0 = by size (round 5):
// a launch of under kGetSmallKeys keys takes 4 x 4 -- a cfg-4 rank's Get at
// N = 8 (~8 M keys) ran K1 in 17.5 against 18.4 us with the smaller chunks
// (ranks 0 and 1 emulated, twice each, profiles/r05_probes/emu_u48/), where
// the dense Add's K2g lost with them (22.0 against 21.2 us), so the two are
// chosen apart; UNROLL = 4 still forces 4 x 4 on both.
constexpr uint64_t kGetSmallKeys = 24ull << 20;
int gather_unroll(const pskv_shard* s, uint64_t elems) {
  if (s->tune_get_unroll) return s->tune_get_unroll;
  if (s->tune_unroll == 4) return 4;
  return elems < kGetSmallKeys ? 4 : 8;
}

int use_device(pskv_shard* s) {
  PSKV_HIP(hipSetDevice(s->device));
  return PSKV_OK;
}

hipEvent_t take_event(pskv_shard* s) {
  if (!s->event_pool.empty()) {
    hipEvent_t e = s->event_pool.back();
    s->event_pool.pop_back();
    return e;
  }
  // timing-only events: no system-scope release fence (an L2 writeback + invalidate
  // per record, measured at ~4 us each between the cfg-2 kernels)
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
  return e;
}

// Bracket one kernel launch with events when timing is on.
struct LaunchTimer {
  pskv_shard* s;
  int kernel;
  uint64_t elems;
  uint64_t count = 1;
  hipEvent_t a = nullptr, b = nullptr;
  LaunchTimer(pskv_shard* s_, int k, uint64_t e) : s(s_), kernel(k), elems(e) {
    s->last_kernel = k;
    ++s->launches;
    if (s->timing_mask & (1u << k)) {
      a = take_event(s);
      b = take_event(s);
      if (a && b) (void)hipEventRecord(a, s->stream);
    }
  }
  void done() {
    if (a && b) {
      (void)hipEventRecord(b, s->stream);
      s->pending.push_back(TimedLaunch{kernel, a, b, elems, count});
    }
    a = b = nullptr;
  }
};

// ------------------------------------------------------ bounded host waits
// Every host wait of the library polls a HIP event instead of blocking in
// hipStreamSynchronize / hipEventSynchronize, so that work which never
// completes -- a kernel that does not finish, a stream held behind another
// process's queue -- fails the call after PSKV_SYNC_TIMEOUT_MS with
// PSKV_ESTATE and a message naming the stream or event, the device and the
// last kernel the shard queued, instead of hanging its caller (VERDICT r4
// item 1).  Nothing is restarted or cancelled: the work stays queued.  Polls
// spin for the first millisecond (a small call's latency), then yield, then
// sleep 100 us between polls after 50 ms.
const char* const kKernelNames[kTimeSlots] = {
    "k_gather (K1 Get)",          "k_assign_sorted (K2)",          "k_assign_group (K2g)",
    "k_general_mark (K4a)",       "k_general_commit (K4b)",        "k_rb_bin + k_rb_resolve (K5 Add)",
    "k_dense_check (K6)",         "k_acc_dense (K7)",              "k_inline_add (K8)",
    "k_inline_get (K8)",          "k_replay (K4r)",                "k_row_gather (row Get)",
    "k_general_mark + k_row_commit (row assign Add)",              "k_row_accumulate (row accumulate Add)",
    "k_general_mark + k_row_grad_losers + k_row_apply (optimizer step)",
    "k_row_pooled_chunks + k_row_pooled (pooled pull)",
    "k_index_insert + k_index_translate (sparse index)"};

std::string wait_report(const pskv_shard* s, const char* what, const void* handle, double ms) {
  char buf[384];
  std::snprintf(buf, sizeof(buf),
                "%s (%p) on device %d not complete after %.0f ms (PSKV_SYNC_TIMEOUT_MS); last kernel this shard "
                "queued: %s (%llu launches); the work stays queued",
                what, handle, s->device, ms,
                s->last_kernel >= 0 && s->last_kernel < kTimeSlots ? kKernelNames[s->last_kernel] : "none",
                (unsigned long long)s->launches);
  return buf;
}

int wait_event(pskv_shard* s, hipEvent_t ev, const char* what, const void* handle) {
  if (!s->tune_sync_timeout_ms) {  // unbounded: the runtime's own blocking wait
    const hipError_t e = hipEventSynchronize(ev);
    return e == hipSuccess ? PSKV_OK : fail(PSKV_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  using Clock = std::chrono::steady_clock;
  const auto t0 = Clock::now();
  for (uint64_t it = 0;; ++it) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return PSKV_OK;
    if (e != hipErrorNotReady) return fail(PSKV_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    if ((it & 15u) != 15u) continue;
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    if (s->tune_sync_timeout_ms && ms > (double)s->tune_sync_timeout_ms)
      return fail(PSKV_ESTATE, wait_report(s, what, handle ? handle : ev, ms));
    if (ms > 50.0)
      std::this_thread::sleep_for(std::chrono::microseconds(100));
    else if (ms > 1.0)
      std::this_thread::yield();
  }
}

// Wait for everything queued on `st` so far (hipStreamSynchronize, bounded).
// The marker event keeps the default system-scope release, as the stream
// synchronisation it replaces: host reads of pinned results see the writes.
int wait_stream(pskv_shard* s, hipStream_t st, const char* what) {
  if (!s->tune_sync_timeout_ms) {  // unbounded: the runtime's own blocking wait
    const hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? PSKV_OK : fail(PSKV_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  if (!s->sync_ev) PSKV_HIP(hipEventCreateWithFlags(&s->sync_ev, hipEventDisableTiming));
  PSKV_HIP(hipEventRecord(s->sync_ev, st));
  return wait_event(s, s->sync_ev, what, st);
}

int drain_timing(pskv_shard* s) {
  for (auto& t : s->pending) {
    if (int rc = wait_event(s, t.b, "timing event of the shard's stream", t.b)) return rc;
    float ms = 0.f;
    PSKV_HIP(hipEventElapsedTime(&ms, t.a, t.b));
    s->t_launches[t.kernel] += t.count;
    s->t_ms[t.kernel] += ms;
    s->t_elems[t.kernel] += t.elems;
    s->event_pool.push_back(t.a);
    s->event_pool.push_back(t.b);
  }
  s->pending.clear();
  return PSKV_OK;
}

// ------------------------------------------------------- K9 request server
// Protocol (host side).  Requests are numbered 1, 2, ...; the host fills slot
// q % kSrvSlots, then publishes q in req_seq (release).  The kernel applies
// requests in order and publishes each number in done_seq after it (a Get
// after its reply is released).  The kernel runs ALONE on the shard: before
// any other work is queued on the shard's stream (srv_stop: every posted
// request applied, then `stop`, then the kernel's end, which releases its
// stores), and it starts behind everything already queued on that stream
// (srv_launch: stream wait on an event), so stream order is kept both ways.
// A kernel that left on its idle timer is restarted from done_seq (srv_wait).

// A resident server holds the hardware queue its stream maps to (the
// accounting per device, pskv_queues.h): the server engages on a device only
// while 2 * shards + 1 + extra streams fit its GPU_MAX_HW_QUEUES queues (one
// shard at the default 4) — it then holds a queue of its own, provided the
// process creates no further streams on the device (torch's default stream is
// the null stream).  Beyond that the K8 launches serve.  A launch that is
// nevertheless queued behind other work does not hang its caller: srv_wait
// bounds the wait for it to start (kSrvStartTimeoutMs) and fails the call.
DeviceQueues g_queues;

bool serve_on(const pskv_shard* s) {
  if (!s->tune_serve) return false;
  static const int queues = hw_queues_from_env(std::getenv("GPU_MAX_HW_QUEUES"));
  return g_queues.serve_fits(s->device, queues);
}

constexpr int kSrvStartTimeoutMs = 2000;

int ensure_ireply(pskv_shard* s, size_t cap) {
  if (s->ireply) return PSKV_OK;
  // the reply values, then the K8 reply's sequence word on its own line.
  // Coherent (fine-grained) memory: the kernel's stores go straight to the
  // host.  Measured alternatives (tools/micro/small_latency.cpp):
  // non-coherent pinned memory the same, a device reply + D2H copy 3 us slower.
  if (hipHostMalloc(&s->ireply, cap + 128, hipHostMallocCoherent) != hipSuccess) {
    s->ireply = nullptr;
    return fail(PSKV_ENOMEM, "inline reply buffer allocation failed");
  }
  // the sequence word the host polls (ireply_seq counts from 1): page-locked
  // memory may come back holding a former owner's bytes, so clear it
  std::memset(static_cast<char*>(s->ireply) + cap, 0, 128);
  s->ireply_seq = 0;
  return PSKV_OK;
}

int srv_launch(pskv_shard* s) {
  SrvRing* r = s->srv;
  const uint32_t start = __atomic_load_n(&r->done_seq, __ATOMIC_ACQUIRE);
  __atomic_store_n(&r->stop, 0u, __ATOMIC_RELAXED);
  __atomic_store_n(&r->alive, 1u, __ATOMIC_RELEASE);
  ++s->srv_gen;
  // SERVE_IDLE_US may change between launches (pskv_set_option)
  s->srv_idle_ticks =
      (unsigned long long)s->tune_serve_idle_us * (unsigned long long)std::max(s->wall_khz, 1) / 1000ull;
  PSKV_HIP(hipEventRecord(s->srv_dep, s->stream));
  PSKV_HIP(hipStreamWaitEvent(s->srv_stream, s->srv_dep, 0));
  PSKV_HIP(launch_serve(s->dtype, s->mode, r, s->dview(), s->ovf, s->ireply, start, s->srv_idle_ticks,
                        s->srv_gen, s->srv_stream));
  s->srv_running = true;
  return PSKV_OK;
}

// The kernel has left (or is leaving) its loop: wait for its end.
int srv_reap(pskv_shard* s) {
  s->srv_running = false;
  if (int rc = wait_stream(s, s->srv_stream, "request-server stream (K9 end)")) return rc;
  return PSKV_OK;
}

// Wait until request `seq` has been applied.
int srv_wait(pskv_shard* s, uint32_t seq) {
  SrvRing* r = s->srv;
  // The start clock runs only once the server's own dependency (everything
  // queued on the shard's stream before its launch, srv_dep) has completed: a
  // launch still waiting for that work -- e.g. a long replay of a broken sorted
  // hint -- is not stuck, however long the work takes.
  auto t_start = std::chrono::steady_clock::now();
  const auto t_entry = t_start;
  bool dep_done = false;
  for (uint32_t it = 1;; ++it) {
    if ((int32_t)(__atomic_load_n(&r->done_seq, __ATOMIC_ACQUIRE) - seq) >= 0) return PSKV_OK;
    if ((it & 255u) == 0 && __atomic_load_n(&r->alive, __ATOMIC_ACQUIRE) == 0u) {
      // it left on its idle timer as requests were being posted: restart it
      if (int rc = srv_reap(s)) return rc;
      if ((int32_t)(__atomic_load_n(&r->done_seq, __ATOMIC_ACQUIRE) - seq) >= 0) return PSKV_OK;
      if (int rc = srv_launch(s)) return rc;
      dep_done = false;
      t_start = std::chrono::steady_clock::now();
    }
    if ((it & 65535u) == 0) {  // a faulted kernel never publishes: surface the error
      const hipError_t e = hipStreamQuery(s->srv_stream);
      if (e != hipSuccess && e != hipErrorNotReady) PSKV_HIP(e);
      // the overall bound (PSKV_SYNC_TIMEOUT_MS): a dependency that never
      // completes -- a kernel that does not finish, or work held behind
      // another queue -- fails the call instead of spinning without end
      const double ms =
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
      if (s->tune_sync_timeout_ms && ms > (double)s->tune_sync_timeout_ms)
        return fail(PSKV_ESTATE, wait_report(s, dep_done ? "request-server request (server launched, request not "
                                                            "applied)"
                                                          : "request-server dependency (the shard's stream before "
                                                            "the server's launch)",
                                             dep_done ? static_cast<const void*>(s->srv_stream)
                                                      : static_cast<const void*>(s->srv_dep),
                                             ms));
      if (!dep_done) {
        const hipError_t d = hipEventQuery(s->srv_dep);
        if (d != hipSuccess && d != hipErrorNotReady) PSKV_HIP(d);
        dep_done = d == hipSuccess;
        t_start = std::chrono::steady_clock::now();  // re-armed while the dependency runs
        continue;
      }
      // the dependency is done and the launch has still not started: it is
      // queued behind other work on its hardware queue -- fail the call rather
      // than wait without bound
      if (__atomic_load_n(&r->started, __ATOMIC_ACQUIRE) != s->srv_gen &&
          std::chrono::steady_clock::now() - t_start > std::chrono::milliseconds(kSrvStartTimeoutMs))
        return fail(PSKV_ESTATE,
                    "request server did not start within 2 s: its hardware queue is held by other work "
                    "(more streams on the device than GPU_MAX_HW_QUEUES); run without PSKV_SERVE");
    }
  }
}

// Every posted request applied and the kernel ended (before any other work).
int srv_stop(pskv_shard* s) {
  if (!s->srv_running) return PSKV_OK;
  if (int rc = srv_wait(s, s->srv_posted)) return rc;
  __atomic_store_n(&s->srv->stop, 1u, __ATOMIC_RELEASE);
  return srv_reap(s);
}

int srv_ensure(pskv_shard* s) {
  if (!s->srv) {
    int rc = ensure_ireply(s, (size_t)kInlineGetMax * kInlineMaxChunks * 8);
    if (rc) return rc;
    void* p = nullptr;
    if (hipHostMalloc(&p, sizeof(SrvRing), hipHostMallocCoherent) != hipSuccess)
      return fail(PSKV_ENOMEM, "request ring allocation failed");
    std::memset(p, 0, sizeof(SrvRing));
    s->srv = static_cast<SrvRing*>(p);
    PSKV_HIP(hipStreamCreateWithFlags(&s->srv_stream, hipStreamNonBlocking));
    PSKV_HIP(hipEventCreateWithFlags(&s->srv_dep, hipEventDisableTiming | hipEventDisableSystemFence));
    PSKV_HIP(hipDeviceGetAttribute(&s->wall_khz, hipDeviceAttributeWallClockRate, s->device));
  }
  if (s->srv_running && __atomic_load_n(&s->srv->alive, __ATOMIC_ACQUIRE) == 0u)
    if (int rc = srv_reap(s)) return rc;
  if (!s->srv_running) return srv_launch(s);
  return PSKV_OK;
}

// The slot of the next request (waits while the ring is full).
int srv_slot(pskv_shard* s, SrvSlot** slot) {
  const uint32_t q = s->srv_posted + 1;
  if ((int32_t)(q - __atomic_load_n(&s->srv->done_seq, __ATOMIC_ACQUIRE)) > kSrvSlots)
    if (int rc = srv_wait(s, q - kSrvSlots)) return rc;
  *slot = &s->srv->slot[q % kSrvSlots];
  return PSKV_OK;
}

void srv_publish(pskv_shard* s) {
  const uint32_t q = ++s->srv_posted;
  __atomic_store_n(&s->srv->req_seq, q, __ATOMIC_RELEASE);
}

// ------------------------------------------------------- overflow table
// One array set of the table: keys EMPTY, values 0 (stream-ordered), tracked
// in s->tables.
int alloc_tab(pskv_shard* s, uint64_t cap, OvfTab* out) {
  OvfTab t{};
  if (hipMalloc(&t.keys, cap * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc(&t.vals, cap * (size_t)s->vb) != hipSuccess) {
    if (t.keys) (void)hipFree(t.keys);
    return fail(PSKV_ENOMEM, "overflow table allocation failed");
  }
  t.mask = cap - 1;
  {
    std::lock_guard<std::mutex> g(s->tab_m);
    s->tables.push_back(t);
  }
  PSKV_HIP(hipMemsetAsync(t.keys, 0xFF, cap * sizeof(unsigned long long), s->stream));
  PSKV_HIP(hipMemsetAsync(t.vals, 0, cap * (size_t)s->vb, s->stream));
  *out = t;
  return PSKV_OK;
}

// Free every array set but the current one.  Only with the shard's stream
// idle (no kernel can still hold a superseded table).
void free_stale_tables(pskv_shard* s) {
  std::lock_guard<std::mutex> g(s->tab_m);
  std::vector<OvfTab> keep;
  for (const auto& t : s->tables) {
    if (t.keys == s->cur.keys) {
      keep.push_back(t);
      continue;
    }
    (void)hipFree(t.keys);
    (void)hipFree(t.vals);
  }
  s->tables.swap(keep);
}

// Read the control block back (synchronises the stream): {count, err}, and
// adopt the table it names -- a device-side inserter may have grown it
// (ovf_reserve) -- freeing the superseded arrays.
int read_overflow_stat(pskv_shard* s, uint32_t* count, uint32_t* err) {
  if (int rc = srv_stop(s)) return rc;
  // into page-locked memory the shard owns: the copy is truly asynchronous (a
  // pageable destination would block inside the runtime, unbounded), and a
  // wait that times out leaves it writing into live memory, not a dead frame
  static_assert(sizeof(OvfCtl) <= 64, "the control block fits the read-back buffer");
  if (!s->stat_host) {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocDefault) != hipSuccess)
      return fail(PSKV_ENOMEM, "overflow-stat read-back buffer allocation failed");
    s->stat_host = static_cast<uint32_t*>(p);
  }
  OvfCtl* st = reinterpret_cast<OvfCtl*>(s->stat_host);
  std::memset(st, 0, sizeof(OvfCtl));
  PSKV_HIP(hipMemcpyAsync(st, s->ovf.c, sizeof(OvfCtl), hipMemcpyDeviceToHost, s->stream));
  if (int rc = wait_stream(s, s->stream, "shard stream (overflow count read-back)")) return rc;
  const uint32_t cnt = *count = st->stat[0];
  *err = st->stat[1];
  s->ocount_known = cnt;
  // a sparse shard: stat[0] is the slot counter, which an overfull call runs
  // past the capacity; the stream is idle, so this is the true count, and
  // sp_bound, the host's upper bound of it, is refreshed here and nowhere else
  if (s->sparse) s->sp_bound = std::min<uint64_t>(cnt, s->range);
  if (st->t.keys && st->t.keys != s->cur.keys) {
    s->cur = st->t;
    s->ocap = st->t.mask + 1;
  }
  free_stale_tables(s);
  return PSKV_OK;
}

// The keys a sparse shard holds: one read-back (a bounded stream wait), which
// clamps the slot counter to the capacity and leaves the result in sp_bound.
int sparse_count(pskv_shard* s, uint64_t* count) {
  uint32_t cnt = 0, err = 0;
  if (int rc = read_overflow_stat(s, &cnt, &err)) return rc;
  *count = s->sp_bound;
  return PSKV_OK;
}

// Grow the overflow table to at least `need` occupied slots at load <= 1/2
// (after read_overflow_stat: the stream is idle and s->cur current).
int grow_overflow(pskv_shard* s, uint64_t need) {
  if (int rc = srv_stop(s)) return rc;
  uint64_t cap = s->ocap;
  while (cap < 2 * need) cap <<= 1;
  if (cap == s->ocap) return PSKV_OK;
  OvfTab n{};
  if (int rc = alloc_tab(s, cap, &n)) return rc;
  // rehash, then the control block names the new arrays (its counts and
  // sticky bits stay where they are)
  PSKV_HIP(launch_ovf_rehash(s->vb, s->ovf, s->ocap, n, s->stream));
  if (int rc = wait_stream(s, s->stream, "shard stream (overflow table growth)")) return rc;
  s->cur = n;
  s->ocap = cap;
  free_stale_tables(s);
  return PSKV_OK;
}

// Device wait bound of a growth request (SYNC_TIMEOUT_MS in device wall-clock
// ticks; 0 = unbounded host waits still bounds the device at 10 minutes, so a
// grow service that is gone cannot hold a workgroup forever).
void refresh_grow_wait(pskv_shard* s) {
  if (!s->mbox) return;
  const uint64_t ms = s->tune_sync_timeout_ms ? s->tune_sync_timeout_ms : 600000u;
  const uint64_t ticks = ms * (uint64_t)std::max(s->wall_khz, 1);
  __atomic_store_n(&s->mbox->wait_ticks, ticks, __ATOMIC_RELEASE);
}

// The grow service: ONE host thread per process that answers the growth
// requests device-side inserters post to their shard's mailbox (ovf_reserve in
// pskv_kernels.hip).  It polls every registered mailbox (100 us apart while
// requests come, backing off to 1 ms after a quiet second), allocates arrays of
// the asked capacity on the shard's device -- only allocation: the requesting
// workgroup fills them and rehashes the table itself, so nothing here waits for
// a queue the requester may be blocking -- records them in the shard's table
// list, and answers.  A shard unregisters (under the service's lock) before its
// mailbox goes.
class GrowService {
 public:
  static GrowService& get() {
    static GrowService g;
    return g;
  }
  void add(pskv_shard* s) {
    std::lock_guard<std::mutex> g(m_);
    shards_.push_back(s);
    if (!th_.joinable()) th_ = std::thread([this] { loop(); });
    cv_.notify_all();
  }
  void remove(pskv_shard* s) {
    std::lock_guard<std::mutex> g(m_);
    shards_.erase(std::remove(shards_.begin(), shards_.end(), s), shards_.end());
  }
  ~GrowService() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    if (th_.joinable()) th_.join();
  }

 private:
  GrowService() = default;
  void serve(pskv_shard* s) {
    OvfMbox* m = s->mbox;
    const uint32_t seq = __atomic_load_n(&m->req_seq, __ATOMIC_ACQUIRE);
    if (seq == s->mbox_served) return;
    const uint64_t cap = __atomic_load_n(&m->req_cap, __ATOMIC_RELAXED);
    OvfTab t{};
    uint32_t ok = 0;
    if (cap >= 2 && (cap & (cap - 1)) == 0 && hipSetDevice(s->device) == hipSuccess &&
        hipMalloc(&t.keys, cap * sizeof(unsigned long long)) == hipSuccess) {
      if (hipMalloc(&t.vals, cap * (size_t)s->vb) == hipSuccess) {
        t.mask = cap - 1;
        ok = 1;
        std::lock_guard<std::mutex> g(s->tab_m);
        s->tables.push_back(t);
      } else {
        (void)hipFree(t.keys);
        t = OvfTab{};
      }
    }
    (void)hipGetLastError();
    m->resp_tab = t;
    m->resp_ok = ok;
    __atomic_store_n(&m->resp_seq, seq, __ATOMIC_RELEASE);
    s->mbox_served = seq;
    ++served_;
  }
  void loop() {
    auto quiet_since = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      cv_.wait(lk, [&] { return stop_ || !shards_.empty(); });
      if (stop_) return;
      const uint64_t before = served_;
      for (pskv_shard* s : shards_) serve(s);
      const auto now = std::chrono::steady_clock::now();
      if (served_ != before) quiet_since = now;
      const bool busy = now - quiet_since < std::chrono::seconds(1);
      cv_.wait_for(lk, std::chrono::microseconds(busy ? 100 : 1000), [&] { return stop_; });
      if (stop_) return;
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::vector<pskv_shard*> shards_;
  std::thread th_;
  bool stop_ = false;
  uint64_t served_ = 0;
};

// The hold on the pinned staging buffer, as a scope guard.  The rule: once
// anything queued reads or writes the buffer (H2D from it, D2H or K1 stores
// into it), no exit may leave without marking it busy until the stream's
// current end, so the next host call waits (bounded) before its CPU copy
// touches the buffer or a regrowth frees it -- a call that gives
// up on a wait (PSKV_ESTATE) or fails midway included.  A path arms the guard
// before it queues the first such operation; every exit from the guard's
// scope then records hstage_free.  A Get that has waited for all of its copies
// dismisses it (no event record on a successful Get); a staged Add, which
// returns before its DMA, leaves it armed.
struct HstageHold {
  pskv_shard* s;
  bool armed = false;
  explicit HstageHold(pskv_shard* s_) : s(s_) {}
  HstageHold(const HstageHold&) = delete;
  HstageHold& operator=(const HstageHold&) = delete;
  void arm() { armed = true; }
  void dismiss() { armed = false; }
  ~HstageHold() {
    if (armed && hipEventRecord(s->hstage_free, s->stream) == hipSuccess) s->hstage_pending = true;
  }
};

int ensure_hstage(pskv_shard* s, size_t bytes) {
  if (s->hstage_pending) {
    if (int rc = wait_event(s, s->hstage_free, "pinned staging release event", s->hstage_free)) return rc;
    s->hstage_pending = false;
  }
  if (s->hstage_bytes >= bytes) return PSKV_OK;
  if (s->hstage) (void)hipHostFree(s->hstage);
  s->hstage = nullptr;
  size_t nb = std::max<size_t>(bytes + bytes / 2, 1 << 20);
  if (hipHostMalloc(&s->hstage, nb, hipHostMallocDefault) != hipSuccess) {
    s->hstage_bytes = 0;
    return fail(PSKV_ENOMEM, "pinned staging allocation failed");
  }
  s->hstage_bytes = nb;
  return PSKV_OK;
}

int ensure_dstage(pskv_shard* s, size_t bytes) {
  if (s->dstage_bytes >= bytes) return PSKV_OK;
  if (s->dstage) {
    // stream-ordered free: the buffer may still be read by queued kernels
    if (int rc = wait_stream(s, s->stream, "shard stream (device staging regrowth)")) return rc;
    (void)hipFree(s->dstage);
  }
  s->dstage = nullptr;
  size_t nb = std::max<size_t>(bytes + bytes / 2, 1 << 20);
  if (hipMalloc(&s->dstage, nb) != hipSuccess) {
    s->dstage_bytes = 0;
    return fail(PSKV_ENOMEM, "device staging allocation failed");
  }
  s->dstage_bytes = nb;
  return PSKV_OK;
}

// One launch group: the kernarg descriptor of batches [b, e) of a list, cut
// into chunks of `chunk` elements per workgroup, with its workgroup and
// element counts.
struct LaunchGroup {
  GroupArgs ga;
  uint32_t nwg;
  uint64_t elems;
};

// chunk_of(elems): the chunk, for a kernel that chooses it by the launch's size.
template <typename ChunkOf>
LaunchGroup make_group_by(const std::vector<pskv_batch>& v, size_t b, size_t e, const ChunkOf& chunk_of) {
  LaunchGroup g;
  std::memset(&g.ga, 0, sizeof(g.ga));
  g.ga.nb = (int)(e - b);
  g.elems = 0;
  for (size_t i = b; i < e; ++i) g.elems += v[i].n;
  const uint64_t chunk = chunk_of(g.elems);
  uint64_t wg = 0;
  for (size_t i = b; i < e; ++i) {
    const int j = (int)(i - b);
    g.ga.wg_prefix[j] = (uint32_t)wg;
    g.ga.b[j] = DevBatch{v[i].keys, v[i].vals, v[i].n};
    wg += (v[i].n + chunk - 1) / chunk;
  }
  g.ga.wg_prefix[e - b] = (uint32_t)wg;
  g.nwg = (uint32_t)wg;
  return g;
}

LaunchGroup make_group(const std::vector<pskv_batch>& v, size_t b, size_t e, uint64_t chunk) {
  return make_group_by(v, b, e, [chunk](uint64_t) { return chunk; });
}

// Every keys and values pointer 16-byte aligned: the kernels' `vec` argument.
bool all_aligned16(const std::vector<pskv_batch>& v) {
  bool vec = true;
  for (auto& b : v) vec &= aligned16(b.keys) & aligned16(b.vals);
  return vec;
}

// The stamp array is only needed once a stamp-mode Add can run: allocate it on
// first use (8 B per owned KEY, also in a row shard).
int ensure_owner(pskv_shard* s) {
  if (s->owner) return PSKV_OK;
  const size_t bytes = s->range * sizeof(unsigned long long);
  if (hipMalloc(&s->owner, bytes) != hipSuccess) {
    s->owner = nullptr;
    return fail(PSKV_ENOMEM, "stamp array allocation failed");
  }
  PSKV_HIP(hipMemsetAsync(s->owner, 0, bytes, s->stream));
  return PSKV_OK;
}

uint32_t next_epoch(pskv_shard* s) {
  // Stamps are epoch<<32|index; on wrap-around the stamp arrays are reset so
  // that every old stamp still loses to the new epoch 1.
  if (s->epoch == 0xFFFFFFFFu) {
    if (s->owner) (void)hipMemsetAsync(s->owner, 0, s->range * sizeof(unsigned long long), s->stream);
    (void)hipMemsetAsync(s->flag, 0, 2 * sizeof(uint32_t), s->stream);  // both tags
    s->epoch = 0;
  }
  return ++s->epoch;
}

// Grow a device scratch buffer (stream-ordered: queued kernels may still use
// the old one, so synchronise before freeing it).
int ensure_scratch(pskv_shard* s, void** p, size_t* have, size_t need) {
  if (*have >= need) return PSKV_OK;
  if (*p) {
    if (int rc = wait_stream(s, s->stream, "shard stream (scratch regrowth)")) return rc;
    (void)hipFree(*p);
  }
  *p = nullptr;
  const size_t nb = std::max<size_t>(need + need / 4, 1 << 16);
  if (hipMalloc(p, nb) != hipSuccess) {
    *p = nullptr;
    *have = 0;
    return fail(PSKV_ENOMEM, "scratch allocation failed");
  }
  *have = nb;
  return PSKV_OK;
}

// K5: radix-bucket general Add (no random global atomics), one launch pair
// per <= kRbMaxSc super-chunks; a longer group is cut into consecutive pieces
// (a batch may be split), which run in stream order, so call order holds.
int radix_launch(pskv_shard* s, const std::vector<pskv_batch>& v, size_t b, size_t e) {
  const LaunchGroup g = make_group(v, b, e, rb_superchunk(s->vb, s->tune_rb_bin_block));
  const uint32_t nsc = g.nwg;
  const RbPlan p = rb_plan(s->range, g.elems, s->mode, s->tune_rb_tb, s->tune_rb_wbits, s->tune_rb_nbd);
  const int apply_log2 = s->tune_rb_apply_log2 ? s->tune_rb_apply_log2 : p.apply_log2;
  const uint32_t nbk = p.bm.nbd + 1;
  if (nbk > (uint32_t)kRbMaxBuckets) return fail(PSKV_EINVAL, "radix path: too many buckets");
  if (nsc > kRbMaxSc) return fail(PSKV_EINVAL, "radix path: launch piece too large");
  const size_t eb = rb_entry_bytes(s->vb);
  int rc = ensure_scratch(s, reinterpret_cast<void**>(&s->rb_loff), &s->rb_loff_bytes,
                          (size_t)nsc * (nbk + 1) * sizeof(uint16_t));
  if (!rc)
    rc = ensure_scratch(s, &s->rb_ent, &s->rb_ent_bytes,
                        (size_t)nsc * rb_superchunk(s->vb, s->tune_rb_bin_block) * eb + kRbTmpPad);
  if (rc) return rc;
  LaunchTimer t(s, PSKV_K_RADIX, g.elems);
  PSKV_HIP(launch_rb_add(s->dtype, s->mode, g.ga, nsc, s->dview(), s->ovf, p.bm, apply_log2,
                         s->tune_rb_bin_block, s->rb_loff, s->rb_ent, s->stream));
  t.done();
  s->n_general += 2;
  return PSKV_OK;
}

int radix_add(pskv_shard* s, const std::vector<pskv_batch>& v, size_t b, size_t e) {
  const uint64_t sc = rb_superchunk(s->vb, s->tune_rb_bin_block);
  uint64_t nsc = 0;
  for (size_t i = b; i < e; ++i) nsc += (v[i].n + sc - 1) / sc;
  const uint64_t max_sc = kRbMaxSc;
  if (nsc <= max_sc) return radix_launch(s, v, b, e);
  // pieces of whole super-chunks, each <= max_sc of them
  std::vector<pskv_batch> piece;
  uint64_t used = 0;  // super-chunks in `piece`
  auto flush = [&]() -> int {
    if (piece.empty()) return PSKV_OK;
    const int rc = radix_launch(s, piece, 0, piece.size());
    piece.clear();
    used = 0;
    return rc;
  };
  for (size_t i = b; i < e; ++i) {
    uint64_t off = 0;
    while (off < v[i].n) {
      if (used == max_sc || piece.size() == (size_t)kMaxBatches) {
        if (int rc = flush()) return rc;
      }
      const uint64_t room = (max_sc - used) * sc;
      const uint64_t n = std::min<uint64_t>(v[i].n - off, room);
      piece.push_back(pskv_batch{v[i].keys + off,
                                 static_cast<char*>(v[i].vals) + off * (uint64_t)s->vb, n});
      used += (n + sc - 1) / sc;
      off += n;
    }
  }
  return flush();
}

// The general (any order) Add over one launch group: K5, or K4 (stamps) under
// GENERAL = 0.
int general_add(pskv_shard* s, const std::vector<pskv_batch>& v, size_t b, size_t e, uint32_t epoch) {
  if (s->general_path != 0) return radix_add(s, v, b, e);
  if (s->mode == PSKV_ASSIGN)
    if (int rc = ensure_owner(s)) return rc;
  const LaunchGroup g = make_group(v, b, e, kGeneralChunk);
  {
    LaunchTimer t(s, PSKV_K_GENERAL_MARK, g.elems);
    PSKV_HIP(launch_general_mark(s->dtype, s->mode, g.ga, g.nwg, s->dview(), s->flag + 1, s->owner, nullptr,
                                 epoch, s->stream));
    t.done();
  }
  s->n_general++;
  if (s->mode == PSKV_ASSIGN) {
    LaunchTimer t(s, PSKV_K_GENERAL_COMMIT, g.elems);
    PSKV_HIP(launch_general_commit(s->vb, g.ga, g.nwg, s->dview(), s->owner, nullptr, epoch, s->stream));
    t.done();
    s->n_general++;
  }
  // the group's out-of-range keys, which K4a only tagged (flag[1]): one
  // workgroup applies them in call order, growing the table as it goes
  {
    LaunchTimer t(s, PSKV_K_REPLAY, g.elems);
    PSKV_HIP(launch_replay(s->dtype, s->mode, g.ga, s->dview(), s->ovf, s->flag + 1, epoch, s->stream,
                           /*oor_only=*/true));
    t.done();
    s->n_general++;
  }
  return PSKV_OK;
}

// A held replay (see replay) launched as K4r, its own launch.
int flush_replay(pskv_shard* s) {
  if (!s->pend_replay) return PSKV_OK;
  GroupArgs ga;
  ga.nb = s->pend_rg.nb;
  for (int i = 0; i < ga.nb; ++i) ga.b[i] = s->pend_rg.b[i];
  LaunchTimer t(s, PSKV_K_REPLAY, s->pend_elems);
  PSKV_HIP(launch_replay(s->dtype, s->mode, ga, s->dview(), s->ovf, s->flag, s->pend_epoch, s->stream));
  s->pend_replay = false;  // (held until its launch is queued)
  t.done();
  s->n_general++;
  return PSKV_OK;
}

// The safety net behind a verifying sorted-path launch group: K4r replays the
// group in call order iff the verification tagged s->flag with `epoch` (one
// single-workgroup launch that exits at once otherwise).
// Inside pskv_add_get_grouped (s->defer_replay) the replay of an assign group
// with 4-byte values is held instead (pend_*): the Get's first K1 launch takes
// it (K1r), or flush_replay launches it as K4r before anything else is queued.
int replay(pskv_shard* s, const std::vector<pskv_batch>& v, size_t b, size_t e, uint32_t epoch) {
  const LaunchGroup g = make_group(v, b, e, kGeneralChunk);
  if (s->defer_replay && s->mode == PSKV_ASSIGN && s->vb == 4) {
    if (int rc = flush_replay(s)) return rc;  // (add_impl flushed it already: the order holds either way)
    s->pend_rg.nb = g.ga.nb;
    for (int i = 0; i < g.ga.nb; ++i) s->pend_rg.b[i] = g.ga.b[i];
    s->pend_epoch = epoch;
    s->pend_elems = g.elems;
    s->pend_replay = true;
    return PSKV_OK;
  }
  LaunchTimer t(s, PSKV_K_REPLAY, g.elems);
  PSKV_HIP(launch_replay(s->dtype, s->mode, g.ga, s->dview(), s->ovf, s->flag, epoch, s->stream));
  t.done();
  s->n_general++;
  return PSKV_OK;
}

// Sorted path over one launch group of device-resident batches (verifying);
// `repair` adds the conditional replay launch behind it; `maybe_windows` false
// (a host group proven sorted but not all windows) keeps K2g out of early mode.
int sorted_add(pskv_shard* s, const std::vector<pskv_batch>& v, size_t b, size_t e, bool vec,
               uint32_t epoch, bool repair, bool maybe_windows) {
  if (e - b == 1) {
    LaunchTimer t(s, PSKV_K_ASSIGN_SORTED, v[b].n);
    PSKV_HIP(launch_assign_sorted(s->vb, vec, v[b].keys, v[b].vals, v[b].n, s->dview(), s->flag,
                                  epoch, s->stream));
    t.done();
  } else {
    const LaunchGroup g = make_group(v, b, e, stream_chunk(s->tune_unroll));
    const uint32_t nchunks = g.nwg;
    const uint64_t elems = g.elems;
    // Tile (tile mode): enough tiles for several workgroups per CU, 4 Ki..64 Ki keys.
    uint32_t shift = 16;
    while (shift > 12 && (elems >> shift) < 2048) --shift;
    if (s->tune_tile_shift) shift = s->tune_tile_shift;
    const uint64_t ntiles = (s->range + (1ull << shift) - 1) >> shift;
    // grid: one workgroup per dense-mode chunk (the common case: every batch a
    // window), at least 1024 for the tile mode's grid-stride over the tiles;
    // a workgroup beyond the chunks only runs the prologue (two dependent key
    // loads per batch) and leaves
    const uint32_t grid = (uint32_t)std::min<uint64_t>(
        std::max<uint64_t>(std::min<uint64_t>(ntiles, 1024), nchunks), s->tune_tile_grid);
    // Early mode (K2g's whole-chunk loads issued before its prologue, its
    // chunks storing their own elements): for launches whose windows are
    // unlikely to overlap — the pushed keys cover under a quarter of the
    // shard's range, e.g. a rank's share of cfg 4 — since it cannot skip the
    // values of a chunk a later window covers.  Results are the same either way.
    // A host group the CPU found sorted but not all windows goes to the tile
    // mode, where early loads would only be read again (maybe_windows false).
    const bool early = s->tune_early == 1 || (s->tune_early == 2 && maybe_windows && elems * 4 < s->range);
    LaunchTimer t(s, PSKV_K_ASSIGN_TILES, elems);
    PSKV_HIP(launch_assign_group(s->vb, vec, s->tune_unroll, s->tune_nt, s->tune_ntp, early, g.ga, s->dview(),
                                 shift, ntiles, grid, s->flag, epoch, s->stream));
    t.done();
  }
  s->n_sorted++;
  if (repair) return replay(s, v, b, e, epoch);
  return PSKV_OK;
}

// Accumulate over dense windows (K7), one launch group.  `verify`: device
// inputs under PSKV_SORTED_HINT are first proven dense by K6; if not, K7 skips
// and the conditional K4a accumulate takes the group.  Host inputs come
// proven by the CPU check (verify = false).
int dense_accumulate(pskv_shard* s, const std::vector<pskv_batch>& v, size_t b, size_t e,
                     uint32_t epoch, bool verify) {
  const LaunchGroup g = make_group(v, b, e, stream_chunk(8));
  if (verify) {
    LaunchTimer t(s, PSKV_K_DENSE_CHECK, g.elems);
    PSKV_HIP(launch_dense_check(g.ga, g.nwg, s->dview(), s->flag, epoch, s->stream));
    t.done();
  }
  {
    const uint32_t grid = std::min<uint32_t>(g.nwg, s->tune_tile_grid);
    LaunchTimer t(s, PSKV_K_ACC_DENSE, g.elems);
    PSKV_HIP(launch_acc_dense(s->dtype, g.ga, grid, s->dview(), s->flag, epoch, s->stream));
    t.done();
  }
  s->n_sorted++;
  if (verify) return replay(s, v, b, e, epoch);
  return PSKV_OK;
}

void run_copies(pskv_shard* s, std::vector<Piece>& pieces, size_t b, size_t e) {
  run_pieces(pieces, b, e, [&](Piece& p) { copy_piece(p, s->key_begin, s->range); });
}

// Copy pieces window by window (pool in parallel) and DMA each window to the
// device as soon as it is staged, so the copy of window w+1 overlaps the H2D
// of window w.  Pieces must be in increasing staging order.  `hold` is armed
// once a window's H2D from the staging is queued.
int pipelined_h2d(pskv_shard* s, std::vector<Piece>& pieces, char* h, char* d, HstageHold& hold) {
  for (const Span& w : piece_windows(pieces)) {
    run_copies(s, pieces, w.first, w.second);
    char* lo = pieces[w.first].dst;
    char* hi = pieces[w.second - 1].dst + pieces[w.second - 1].bytes;
    PSKV_HIP(hipMemcpyAsync(d + (lo - h), lo, (size_t)(hi - lo), hipMemcpyHostToDevice, s->stream));
    hold.arm();
  }
  return PSKV_OK;
}

// Host batches -> device staging through pinned staging, every batch's keys
// then every batch's values (`lay`, kKeysFirst): the keys -- and, for an Add,
// the values -- are copied in and queued for DMA; a Get's values get room
// behind them.  Returns the device views in `dv`; the pinned copy of a range
// lies at the same offset of hstage.
int stage_keys_first(pskv_shard* s, const std::vector<pskv_batch>& v, const StageLayout& lay, size_t vb,
                     bool with_values, HstageHold& hold, std::vector<pskv_batch>* dv) {
  int rc = ensure_hstage(s, lay.total);
  if (rc) return rc;
  rc = ensure_dstage(s, lay.total);
  if (rc) return rc;
  char* h = static_cast<char*>(s->hstage);
  std::vector<Piece> pieces;
  for (size_t i = 0; i < v.size(); ++i) add_pieces(pieces, v[i].keys, h + lay.at[i].keys, v[i].n * 4, -1);
  if (with_values)
    for (size_t i = 0; i < v.size(); ++i) add_pieces(pieces, v[i].vals, h + lay.at[i].vals, v[i].n * vb, -1);
  *dv = lay.views(v, static_cast<char*>(s->dstage));
  return pipelined_h2d(s, pieces, h, static_cast<char*>(s->dstage), hold);
}

// Page-locked (hipHostMalloc'd / registered) host memory: the DMA engine can
// read or write it directly, so no staging copy is needed.
bool is_pinned(const void* p, void** dev = nullptr) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (dev) *dev = a.devicePointer;
  return a.type == hipMemoryTypeHost && (!dev || a.devicePointer);
}

// Device view of [p, p + bytes) when the whole range lies in ONE page-locked
// allocation (hipHostMalloc'd or registered), else null: a kernel reads and
// writes through the view, so a range that runs past its registration (a
// sub-range registration, a slice across two) must take the DMA path instead.
void* pinned_range_view(const void* p, size_t bytes) {
  void* dev = nullptr;
  if (!is_pinned(p, &dev)) return nullptr;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, reinterpret_cast<hipDeviceptr_t>(dev)) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  const uintptr_t b = reinterpret_cast<uintptr_t>(base), d = reinterpret_cast<uintptr_t>(dev);
  if (d < b || d + bytes > b + size) return nullptr;
  // in place only through the unified address (valid on every device; see
  // pskv_frames.cpp): a device-specific view would tie the buffer to the
  // device that was current when the attributes were read
  if (dev != p) return nullptr;
  return dev;
}

// Device views of page-locked host batches (frames or any other pinned
// memory), or false.
bool pinned_views(const std::vector<pskv_batch>& in, size_t vb, std::vector<pskv_batch>* out) {
  out->clear();
  for (const auto& b : in) {
    pskv_batch d = b;
    void* k = pinned_range_view(b.keys, b.n * 4);
    void* v = pinned_range_view(b.vals, b.n * vb);
    if (!k || !v) return false;
    d.keys = static_cast<const uint32_t*>(k);
    d.vals = v;
    out->push_back(d);
  }
  return true;
}

// Queue the DMA of host batches straight from the caller's buffers to their
// device views `dv`.
hipError_t dma_batches(pskv_shard* s, const std::vector<pskv_batch>& in, const std::vector<pskv_batch>& dv) {
  for (size_t j = 0; j < in.size(); ++j) {
    hipError_t e = hipMemcpyAsync(const_cast<uint32_t*>(dv[j].keys), in[j].keys, in[j].n * 4,
                                  hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dv[j].vals, in[j].vals, in[j].n * (size_t)s->vb, hipMemcpyHostToDevice, s->stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Stage host batches into one device buffer (keys then values per batch,
// 16-byte aligned) through pinned memory, checking on the way whether every
// batch is sorted and inside the dense range.  Returns device batch views.
int stage_host_batches(pskv_shard* s, const std::vector<pskv_batch>& in, std::vector<pskv_batch>* out,
                       bool* all_sorted_in_range, bool* all_dense_in_range) {
  const StageLayout lay = stage_layout(in, (size_t)s->vb, StageOrder::kInterleaved);
  bool locked = true;
  for (const auto& b : in) locked = locked && is_pinned(b.keys) && is_pinned(b.vals);
  // page-locked buffers: DMA'd directly from tune_dma_min_bytes_pinned on
  // (below it the copy, which returns before the DMA, is ahead); pageable
  // buffers only when large (the runtime's pageable copy has a high fixed cost
  // and blocks until done).  Smaller ones are copied into pinned staging and
  // DMA'd asynchronously (the call returns after the host copy).
  locked = locked && lay.total >= s->tune_dma_min_bytes_pinned;
  const bool pinned = locked || (s->tune_pageable_dma && lay.total >= s->tune_dma_min_bytes);
  int rc = pinned ? PSKV_OK : ensure_hstage(s, lay.total);
  if (rc) return rc;
  rc = ensure_dstage(s, lay.total);
  if (rc) return rc;
  char* h = static_cast<char*>(s->hstage);
  *out = lay.views(in, static_cast<char*>(s->dstage));
  // direct DMA: the CPU only checks the keys (dst null)
  std::vector<Piece> pieces;
  for (size_t j = 0; j < in.size(); ++j) {
    add_pieces(pieces, in[j].keys, pinned ? nullptr : h + lay.at[j].keys, in[j].n * 4, (int)j);
    if (!pinned) add_pieces(pieces, in[j].vals, h + lay.at[j].vals, in[j].n * (size_t)s->vb, -1);
  }
  if (pinned) {
    auto issue = [&]() -> hipError_t {
      const hipError_t e = dma_batches(s, in, *out);
      return e == hipSuccess ? hipEventRecord(s->h2d_done, s->stream) : e;
    };
    auto check = [&]() {
      HostPool::get().run(pieces.size(),
                          [&](size_t t) { copy_piece(pieces[t], s->key_begin, s->range); });
    };
    hipError_t e = hipSuccess;
    if (locked) {  // page-locked: the copies are queued at once
      e = issue();
      check();
    } else {
      // pageable (PSKV_PAGEABLE_DMA): the runtime's copies block the issuing
      // thread, so they are issued from a helper while the pool checks
      std::thread t;
      try {
        t = std::thread([&]() {
          (void)hipSetDevice(s->device);
          e = issue();
        });
      } catch (...) {  // no helper thread: issue, then check
      }
      if (!t.joinable()) e = issue();
      check();
      if (t.joinable()) t.join();
    }
    if (e != hipSuccess) {
      // copies queued before the failure may still read the caller's buffers
      (void)wait_stream(s, s->stream, "shard stream (failed host copy)");
      PSKV_HIP(e);
    }
    // the caller may reuse its buffers once this returns
    if (int rc2 = wait_event(s, s->h2d_done, "host-buffer DMA completion event", s->h2d_done)) return rc2;
  } else {
    // the call returns before its DMA: the hold stays armed
    HstageHold hold(s);
    rc = pipelined_h2d(s, pieces, h, static_cast<char*>(s->dstage), hold);
    if (rc) return rc;
  }
  combine_checks(pieces, all_sorted_in_range, all_dense_in_range);
  return PSKV_OK;
}

// Device views of host batches that lie in pskv_host_alloc frames (every
// keys and values range inside one live frame), or false.
bool frame_views(const std::vector<pskv_batch>& in, size_t vb, std::vector<pskv_batch>* out) {
  out->clear();
  for (const auto& b : in) {
    pskv_batch d = b;
    d.keys = static_cast<const uint32_t*>(frames::device_view(b.keys, b.n * 4));
    d.vals = frames::device_view(b.vals, b.n * vb);
    if (!d.keys || !d.vals) return false;
    out->push_back(d);
  }
  return true;
}

// Host Add batches in borrowed frames (PSKV_HOST_FRAME): the CPU checks the
// keys (sorted / dense / in range, as for staged inputs) without copying
// anything; the kernels then read the frames in place across PCIe when the
// call is at most tune_frame_zc_max_bytes, otherwise the frames are DMA'd
// into device staging.  Either way nothing waits: the frames stay unmodified
// until freed, and pskv_host_free holds them until this call's work has run
// (note_frame_uses).
int frame_batches(pskv_shard* s, const std::vector<pskv_batch>& in, const std::vector<pskv_batch>& views,
                  std::vector<pskv_batch>* out, bool* all_sorted_in_range, bool* all_dense_in_range) {
  std::vector<Piece> pieces;
  for (size_t j = 0; j < in.size(); ++j) add_pieces(pieces, in[j].keys, nullptr, in[j].n * 4, (int)j);
  if (staged_bytes(in, (size_t)s->vb) <= s->tune_frame_zc_max_bytes) {
    *out = views;
  } else {
    const StageLayout lay = stage_layout(in, (size_t)s->vb, StageOrder::kInterleaved);
    int rc = ensure_dstage(s, lay.total);
    if (rc) return rc;
    *out = lay.views(in, static_cast<char*>(s->dstage));
    PSKV_HIP(dma_batches(s, in, *out));
  }
  run_copies(s, pieces, 0, pieces.size());
  combine_checks(pieces, all_sorted_in_range, all_dense_in_range);
  return PSKV_OK;
}

// The work queued so far reads the frames of `v` (host pointers).
int note_frame_uses(pskv_shard* s, const std::vector<pskv_batch>& v) {
  std::string err;
  for (const auto& b : v) {
    int rc = frames::note_use(b.keys, s->device, s->stream, &err);
    if (!rc && b.vals != static_cast<const void*>(b.keys))
      rc = frames::note_use(b.vals, s->device, s->stream, &err);
    if (rc) return fail(rc, err);
  }
  return PSKV_OK;
}

// K8: a host Add of at most kInlineMax keys per launch (the reference's
// per-sample messages), up to tune_inline_chunks launches per call.  The
// grouped form equals the concatenation of its batches in order (last-wins /
// sums follow index order across batches), and so does a sequence of launches
// over consecutive pieces of it, so the batches are packed into kernel-argument
// messages of kInlineMax keys; the caller's buffers are free once the launches
// are enqueued (the runtime copies the arguments).
int inline_add(pskv_shard* s, const std::vector<pskv_batch>& v) {
  // (out-of-range keys need no host step: K8 / K9 reserve room in the
  // overflow table on the device, ovf_reserve)
  const bool serve = serve_on(s);
  if (int rc = serve ? srv_ensure(s) : srv_stop(s)) return rc;
  InlineAdd a;
  a.n = 0;
  auto flush = [&]() -> int {
    if (a.n == 0) return PSKV_OK;
    if (serve) {  // K9: one ring slot instead of a launch
      SrvSlot* sl = nullptr;
      if (int rc = srv_slot(s, &sl)) return rc;
      sl->kind = kSrvAdd;
      sl->n = a.n;
      std::memcpy(sl->keys, a.keys, a.n * sizeof(uint32_t));
      std::memcpy(sl->vals, a.vals, a.n * sizeof(unsigned long long));
      srv_publish(s);
      a.n = 0;
      return PSKV_OK;
    }
    LaunchTimer t(s, PSKV_K_INLINE_ADD, a.n);
    PSKV_HIP(launch_inline_add(s->dtype, s->mode, a, s->dview(), s->ovf, s->stream));
    t.done();
    a.n = 0;
    return PSKV_OK;
  };
  for (const auto& b : v) {
    for (uint64_t e = 0; e < b.n; ++e) {
      const uint32_t i = a.n++;
      a.keys[i] = b.keys[e];
      if (s->vb == 8) {
        std::memcpy(&a.vals[i], static_cast<const char*>(b.vals) + e * 8, 8);
      } else {
        uint32_t w;
        std::memcpy(&w, static_cast<const char*>(b.vals) + e * 4, 4);
        a.vals[i] = w;
      }
      if (a.n == (uint32_t)kInlineMax)
        if (int rc = flush()) return rc;
    }
  }
  return flush();
}

// K8 Get: keys in the kernel arguments (kInlineGetMax per launch), the reply
// written by the kernels into a page-locked buffer, copied out to the caller
// once the LAST launch has published (stream order: the earlier ones are done).
int inline_get(pskv_shard* s, const std::vector<pskv_batch>& v, uint64_t total) {
  const size_t cap = (size_t)kInlineGetMax * kInlineMaxChunks * 8;
  if (int rc = ensure_ireply(s, cap)) return rc;
  if (serve_on(s)) {  // K9: ring slots of kInlineGetMax keys, then wait for the last
    if (int rc = srv_ensure(s)) return rc;
    uint64_t off = 0;
    SrvSlot* sl = nullptr;
    for (const auto& b : v) {
      for (uint64_t e = 0; e < b.n; ++e) {
        if (!sl) {
          if (int rc = srv_slot(s, &sl)) return rc;
          sl->kind = kSrvGet;
          sl->n = 0;
          sl->reply_off = (uint32_t)off;
        }
        sl->keys[sl->n++] = b.keys[e];
        ++off;
        if (sl->n == (uint32_t)kInlineGetMax) {
          srv_publish(s);
          sl = nullptr;
        }
      }
    }
    if (sl) srv_publish(s);
    if (int rc = srv_wait(s, s->srv_posted)) return rc;
    const char* r = static_cast<const char*>(s->ireply);
    for (const auto& b : v) {
      std::memcpy(b.vals, r, b.n * (size_t)s->vb);
      r += b.n * (size_t)s->vb;
    }
    return PSKV_OK;
  }
  if (int rc = srv_stop(s)) return rc;  // the K8 launches run on the shard's stream
  unsigned int* done = reinterpret_cast<unsigned int*>(static_cast<char*>(s->ireply) + cap);
  const unsigned int seq = ++s->ireply_seq;
  InlineGet a;
  a.n = 0;
  uint64_t issued = 0;  // values requested by earlier launches
  bool spin = false;
  auto flush = [&](bool last) -> int {
    if (a.n == 0) return PSKV_OK;
    LaunchTimer t(s, PSKV_K_INLINE_GET, a.n);
    // spin-wait reply (coherent host buffer, no timing events to drain): the
    // last kernel publishes a sequence number after the values; the host polls it
    spin = last && s->tune_ispin && !t.a;
    PSKV_HIP(launch_inline_get(s->vb, a, s->dview(), s->ovf,
                               static_cast<char*>(s->ireply) + issued * (size_t)s->vb,
                               spin ? done : nullptr, seq, s->stream));
    t.done();
    issued += a.n;
    a.n = 0;
    return PSKV_OK;
  };
  uint64_t seen = 0;
  for (const auto& b : v) {
    for (uint64_t e = 0; e < b.n; ++e) {
      a.keys[a.n++] = b.keys[e];
      ++seen;
      if (a.n == (uint32_t)kInlineGetMax)
        if (int rc = flush(seen == total)) return rc;
    }
  }
  if (int rc = flush(true)) return rc;
  if (spin) {
    // poll the sequence word; every 1024 polls ask the stream whether it
    // finished (or failed) without publishing, so a fault cannot hang the host
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t it = 1;; ++it) {
      if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == seq) break;
      if ((it & 1023u) == 0) {
        const hipError_t e = hipStreamQuery(s->stream);
        if (e == hipSuccess) {
          if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == seq) break;
          return fail(PSKV_EHIP, "inline get: kernel finished without publishing its reply");
        }
        if (e != hipErrorNotReady) PSKV_HIP(e);
        // bounded like every other host wait (PSKV_SYNC_TIMEOUT_MS)
        const double ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (s->tune_sync_timeout_ms && ms > (double)s->tune_sync_timeout_ms)
          return fail(PSKV_ESTATE, wait_report(s, "shard stream (inline Get reply)", s->stream, ms));
        if (ms > 50.0) std::this_thread::sleep_for(std::chrono::microseconds(100));
      }
    }
  } else {
    if (int rc = wait_stream(s, s->stream, "shard stream (inline Get)")) return rc;
  }
  const char* r = static_cast<const char*>(s->ireply);
  for (const auto& b : v) {
    std::memcpy(b.vals, r, b.n * (size_t)s->vb);
    r += b.n * (size_t)s->vb;
  }
  return PSKV_OK;
}

// ------------------------------------------------------------- row shards
// A shard of width W > 1 (pskv_shard_create_rows): W values per key, row-major
// in the batches and in the dense array.  It takes none of the scalar paths
// above: add_impl / get_impl / add_get_impl dispatch here at their top.
//   Get         k_row_gather
//   assign Add  K4a (k_general_mark, stamp mode, unchanged: it reads keys only)
//               then k_row_commit: the element whose tag equals its key's stamp
//               copies its whole row; timed together as PSKV_K_ROW_COMMIT
//   accumulate  k_row_accumulate
// Host buffers are staged through the pinned and device staging buffers
// (stage_keys_first: every batch's keys, then every batch's rows, 16-byte
// aligned); the row D2H of a Get is one copy and one wait.  Keys outside the
// owned range are not stored (pskv.h): a host Add refuses them before anything
// is queued, the kernels drop them and set kErrRowOutOfRange.
size_t row_bytes(const pskv_shard* s) { return (size_t)s->width * (size_t)s->vb; }

// unit16 of a launch (row_shape): the row size is a multiple of 16 bytes, and
// the arrays the launch touches and every batch's rows are 16-byte aligned.
bool rows_unit16(const pskv_shard* s, std::initializer_list<const void*> arrays, const std::vector<pskv_batch>& v) {
  bool ok = row_bytes(s) % 16 == 0;
  for (const void* p : arrays) ok = ok && aligned16(p);
  for (const auto& b : v) ok = ok && aligned16(b.vals);
  return ok;
}

// A sparse shard's step between a call's front and its row kernels (DESIGN.md
// §8k): the keys of `v` (vals are not looked at) become slot ids, and each
// batch's keys pointer is redirected to them.  writing: the call inserts
// (k_index_insert over every launch group first, then the translate passes: a
// key repeated across groups finds the one slot it got).  in_place: the keys lie
// in the device staging (a host call) and are overwritten; else the ids go to
// the shard's scratch and the caller's keys are only read.  The launches are
// one timed operation (kTimeIndex), elements = the keys.
int sparse_autogrow(pskv_shard* s, uint64_t n);

int sparse_ids(pskv_shard* s, std::vector<pskv_batch>& v, bool writing, bool in_place) {
  std::vector<pskv_batch> io(v.size());  // vals: where the batch's ids go
  uint64_t elems = 0;
  size_t bytes = 0;
  for (const auto& b : v) {
    elems += b.n;
    bytes += round16(b.n * sizeof(uint32_t));
  }
  if (elems == 0) return PSKV_OK;
  // growth first, before any key of the call is inserted (and before sindex()
  // is taken: a growth replaces the arrays it names)
  if (writing && s->sp_max_capacity)
    if (int rc = sparse_autogrow(s, elems)) return rc;
  if (!in_place)
    if (int rc = ensure_scratch(s, &s->sp_ids, &s->sp_ids_bytes, bytes)) return rc;
  size_t at = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    void* ids = in_place ? static_cast<void*>(const_cast<uint32_t*>(v[i].keys)) : static_cast<char*>(s->sp_ids) + at;
    io[i] = pskv_batch{v[i].keys, ids, v[i].n};
    at += round16(v[i].n * sizeof(uint32_t));
  }
  const SparseIndex x = s->sindex();
  const std::vector<Span> spans = split_groups(io);
  LaunchTimer t(s, kTimeIndex, elems);
  if (writing)
    for (const Span& sp : spans) {
      const LaunchGroup g = make_group(io, sp.first, sp.second, kGeneralChunk);
      PSKV_HIP(launch_index_insert(g.ga, g.nwg, x, s->stream));
    }
  for (const Span& sp : spans) {
    const LaunchGroup g = make_group(io, sp.first, sp.second, kGeneralChunk);
    PSKV_HIP(launch_index_translate(writing, g.ga, g.nwg, x, s->stream));
  }
  t.done();
  for (size_t i = 0; i < v.size(); ++i) v[i].keys = static_cast<const uint32_t*>(io[i].vals);
  return PSKV_OK;
}

// The front of every row-shaped call: a row Add or Get, an optimizer step, a
// read or write of optimizer state.
struct RowFront {
  const char* what;      // the call's name in messages
  uint64_t* calls;       // n_add / n_get, or null: counted once the arguments hold
  bool stop_server;      // end a width-1 shard's request server before stream work
  const char* refusal;   // a host call refuses an out-of-range key (null: it does not):
  const char* why;       //   what stands in front of and behind the key
  bool with_values;      // a host call stages its rows behind its keys (an Add's)
};
struct RowCall {
  std::vector<pskv_batch> v;   // the call's pieces, where the caller has them (empty: nothing to do)
  std::vector<pskv_batch> dv;  // a host call's pieces in the device staging
  StageLayout lay;             // and where each lies there (pinned staging: the same offsets)
  bool host = false;
  const std::vector<pskv_batch>& views() const { return host ? dv : v; }  // what the kernels read
};

// What a host call is told about the first key outside the range (both fronts).
int refuse_key(const std::string& who, const char* refusal, uint32_t key, const char* why) {
  return fail(PSKV_EINVAL, who + ": " + refusal + " " + std::to_string(key) + " is outside [key_begin, key_end); " + why +
                               " (nothing was applied)");
}

// The pieces are in c->v (empty: the call holds no key and nothing further was
// done), the call is counted, the device is selected and the server stopped.
// A host call's keys are checked before anything is queued (nothing is
// applied); its pieces are then on their way to the device staging, and
// `hold`, the caller's, is armed.
int rows_front(pskv_shard* s, const std::vector<pskv_batch>& in, int flags, const RowFront& f, HstageHold& hold,
               RowCall* c) {
  for (auto& b : in) {
    if (b.n == 0) continue;
    if (!b.keys || !b.vals) return fail(PSKV_EINVAL, std::string(f.what) + ": null keys/vals with n > 0");
    push_pieces(c->v, b, row_bytes(s));
  }
  if (f.calls) ++*f.calls;
  if (c->v.empty()) return PSKV_OK;
  int rc = use_device(s);
  if (rc) return rc;
  if (f.stop_server && (rc = srv_stop(s))) return rc;
  if (!(flags & PSKV_DEVICE)) {
    if (f.refusal && !s->sparse)  // (a sparse shard owns every key)
      if (const uint32_t* k = first_key_outside(c->v, s->key_begin, s->range))
        return refuse_key(f.what, f.refusal, *k, f.why);
    c->host = true;
    c->lay = stage_layout(c->v, row_bytes(s), StageOrder::kKeysFirst);
    if (int rc = stage_keys_first(s, c->v, c->lay, row_bytes(s), f.with_values, hold, &c->dv)) return rc;
  }
  // a sparse shard: what the kernels read carries slot ids from here on (the
  // calls that bring values are the writing ones, and insert)
  if (s->sparse) return sparse_ids(s, c->host ? c->dv : c->v, /*writing=*/f.with_values, /*in_place=*/c->host);
  return PSKV_OK;
}

// `d`: the array written: the dense array in the shard's mode, or
// (pskv_put_state) one of the optimizer's state arrays, which have the same
// shape, always as an assign.
int rows_add_device(pskv_shard* s, const std::vector<pskv_batch>& v, const DenseView& d, int mode) {
  const bool vec = rows_unit16(s, {d.param}, v);
  for (const Span& sp : split_groups(v)) {
    const LaunchGroup g = make_group(v, sp.first, sp.second, kGeneralChunk);
    if (mode == PSKV_ACCUMULATE) {
      LaunchTimer t(s, PSKV_K_ROW_ACCUMULATE, g.elems);
      PSKV_HIP(launch_row_accumulate(s->dtype, g.ga, g.nwg, d, s->ovf, row_shape(s->width, s->vb, false),
                                     s->stream));
      t.done();
      s->n_general++;
      continue;
    }
    if (int rc = ensure_owner(s)) return rc;
    const uint32_t epoch = next_epoch(s);
    LaunchTimer t(s, PSKV_K_ROW_COMMIT, g.elems);
    PSKV_HIP(launch_general_mark(s->dtype, PSKV_ASSIGN, g.ga, g.nwg, d, s->flag + 1, s->owner, nullptr, epoch,
                                 s->stream));
    PSKV_HIP(launch_row_commit(s->vb, g.ga, g.nwg, d, s->owner, s->ovf, epoch,
                               row_shape(s->width, s->vb, vec), s->stream));
    t.done();
    s->n_general += 2;
  }
  return PSKV_OK;
}

// A row shard has no request server, so neither this nor rows_get_from stops one.
// slot: the array written, -1 the dense array, else the optimizer's state slot
// (looked up behind the front: a sparse shard's front may grow the shard, which
// replaces every array).
int rows_add_to(pskv_shard* s, const std::vector<pskv_batch>& in, int flags, int slot, int mode,
                const RowFront& f) {
  HstageHold hold(s);  // the call returns before its DMA: the hold stays armed
  RowCall c;
  if (int rc = rows_front(s, in, flags, f, hold, &c)) return rc;
  if (c.v.empty()) return PSKV_OK;
  const DenseView d = slot < 0 ? s->dview() : DenseView{s->opt_slot[slot], s->key_begin, s->range, 0};
  return rows_add_device(s, c.views(), d, mode);
}

int rows_add(pskv_shard* s, const std::vector<pskv_batch>& in, int flags) {
  return rows_add_to(s, in, flags, /*slot=*/-1, s->mode,
                     RowFront{"pskv_add", &s->n_add, false, "row shard: key", "a row shard stores no out-of-range keys",
                              /*with_values=*/true});
}

// `d`: the array gathered from: the dense array, or (pskv_get_state) the
// optimizer's accumulator, which has the same shape.
int rows_gather(pskv_shard* s, const std::vector<pskv_batch>& dv, const DenseView& d) {
  const RowShape rs = row_shape(s->width, s->vb, rows_unit16(s, {d.param}, dv));
  for (const Span& sp : split_groups(dv)) {
    const LaunchGroup g = make_group(dv, sp.first, sp.second, kGeneralChunk);
    LaunchTimer t(s, PSKV_K_ROW_GATHER, g.elems);
    PSKV_HIP(launch_row_gather(s->vb, s->tune_nt, g.ga, g.nwg, d, rs, s->stream));
    t.done();
  }
  return PSKV_OK;
}

// The way back of a host call's rows: bytes [at, at + bytes) of the device
// staging go to the same offsets of the pinned staging, the stream is waited
// for (bounded; `waiting` names the wait), the hold is dismissed and the pool
// copies `back` (pinned staging -> the caller's buffers).
int rows_to_host(pskv_shard* s, HstageHold& hold, size_t at, size_t bytes, const char* waiting,
                 std::vector<Piece>& back) {
  PSKV_HIP(hipMemcpyAsync(static_cast<char*>(s->hstage) + at, static_cast<char*>(s->dstage) + at, bytes,
                          hipMemcpyDeviceToHost, s->stream));
  if (int rc = wait_stream(s, s->stream, waiting)) return rc;
  hold.dismiss();
  run_copies(s, back, 0, back.size());
  return PSKV_OK;
}

int rows_get_from(pskv_shard* s, const std::vector<pskv_batch>& in, int flags, const DenseView& src,
                  const char* what, uint64_t* calls) {
  HstageHold hold(s);
  RowCall c;
  int rc = rows_front(s, in, flags, RowFront{what, calls, false, nullptr, nullptr, /*with_values=*/false}, hold, &c);
  if (rc || c.v.empty()) return rc;
  if ((rc = rows_gather(s, c.views(), src)) || !c.host) return rc;
  std::vector<Piece> back;
  for (size_t i = 0; i < c.v.size(); ++i)
    add_pieces(back, static_cast<char*>(s->hstage) + c.lay.at[i].vals, static_cast<char*>(c.v[i].vals),
               c.v[i].n * row_bytes(s), -1);
  return rows_to_host(s, hold, c.lay.key_bytes, c.lay.total - c.lay.key_bytes, "shard stream (row Get to host)", back);
}

int rows_get(pskv_shard* s, const std::vector<pskv_batch>& in, int flags) {
  return rows_get_from(s, in, flags, s->read_view(s->dense), "pskv_get", &s->n_get);
}

// Host pooled batches -> device staging through pinned staging, batch after
// batch (pool_stage_layout): keys, weights where the batch has them and
// offsets -- and, with_rows, the bag rows of a push -- are copied in and
// queued for DMA; a pull's rows get room behind them.  Returns the device-side
// batches in `dv`; the pinned copy of a range lies at the same offset of
// hstage.
int stage_pool_batches(pskv_shard* s, const std::vector<pskv_pool_batch>& v, bool with_rows, HstageHold& hold,
                       std::vector<pskv_pool_batch>* dv) {
  const size_t rb = row_bytes(s);
  const PoolStageLayout lay = pool_stage_layout(v, (size_t)s->vb, rb);
  int rc = ensure_hstage(s, lay.total);
  if (rc || (rc = ensure_dstage(s, lay.total))) return rc;
  char* h = static_cast<char*>(s->hstage);
  char* d = static_cast<char*>(s->dstage);
  std::vector<Piece> pieces;
  dv->resize(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    const pskv_pool_batch& b = v[i];
    const PoolStageSlot& at = lay.at[i];
    add_pieces(pieces, b.keys, h + at.keys, b.n * 4, -1);
    if (b.weights) add_pieces(pieces, b.weights, h + at.weights, b.n * (size_t)s->vb, -1);
    add_pieces(pieces, b.offsets, h + at.offsets, (b.nbags + 1) * sizeof(uint64_t), -1);
    if (with_rows) add_pieces(pieces, b.bag_grads, h + at.rows, b.nbags * rb, -1);
    (*dv)[i] = pskv_pool_batch{reinterpret_cast<const uint32_t*>(d + at.keys), b.weights ? d + at.weights : nullptr,
                               reinterpret_cast<const uint64_t*>(d + at.offsets), d + at.rows, b.n, b.nbags};
  }
  return pipelined_h2d(s, pieces, h, d, hold);
}

// The front of every pooled call (pskv_get_pooled, pskv_apply_pooled,
// pskv_apply_pooled_grouped), beside rows_front.
struct PoolFront {
  const char* what;  // the call's name in messages
  bool writing;      // a push: a sparse shard inserts its keys (growth first); a pull only reads
  bool with_rows;    // a push stages its bag rows; a pull gets room for its result rows
  const char* why;   // a host call's refusal of an out-of-range key: what stands behind the key
};

// `in`: the call's live batches; `index`: each one's number in the caller's
// list (a grouped call's messages name it), or null.  The device is selected
// and the server stopped; a host call's keys are checked before anything is
// queued and its batches then staged under `hold`, the caller's; a sparse
// shard's keys become slot ids (sparse_ids).  `v`: what the kernels read.
int pool_front(pskv_shard* s, const std::vector<pskv_pool_batch>& in, const std::vector<uint64_t>* index, int flags,
               const PoolFront& f, HstageHold& hold, std::vector<pskv_pool_batch>* v) {
  int rc = use_device(s);
  if (rc || (rc = srv_stop(s))) return rc;
  const bool host = !(flags & PSKV_DEVICE);
  for (size_t i = 0; i < in.size() && host && !s->sparse; ++i) {  // (a sparse shard owns every key)
    std::vector<pskv_batch> keys;
    push_pieces(keys, pskv_batch{in[i].keys, nullptr, in[i].n}, 0);
    if (const uint32_t* k = first_key_outside(keys, s->key_begin, s->range))
      return refuse_key(f.what + (index ? ": batch " + std::to_string((*index)[i]) : std::string()), "key", *k, f.why);
  }
  if (!host) *v = in;
  if (host && (rc = stage_pool_batches(s, in, f.with_rows, hold, v))) return rc;
  if (!s->sparse) return PSKV_OK;
  std::vector<pskv_batch> k;
  for (const auto& b : *v) k.push_back(pskv_batch{b.keys, nullptr, b.n});
  if ((rc = sparse_ids(s, k, f.writing, /*in_place=*/host))) return rc;
  for (size_t i = 0; i < k.size(); ++i) (*v)[i].keys = k[i].keys;
  return PSKV_OK;
}

// ------------------------------------------------------------ pooled pulls
// pskv_get_pooled (pskv.h "Pooled pulls"), at any width, 1
// included.  One or two launches, timed as one operation (kTimePooled):
//   k_row_pooled_chunks   only when n > kPoolChunk (else no bag can be long):
//                         the chunks of long bags into their partial rows
//   k_row_pooled          every bag: its sum, or the sum of its partial rows
// The offsets stay where the caller has them, so a device call's launches do
// not depend on them; the kernels clamp every bag (pool_clamp).
// `c`: the call as the kernels read it, bag_grads the room of its result rows.
int pooled_device(pskv_shard* s, const pskv_pool_batch& c) {
  void* out = const_cast<void*>(c.bag_grads);
  PoolArgs a{c.keys, c.weights, c.offsets, c.n, c.nbags, out, nullptr};
  if (c.n > kPoolChunk) {
    if (int rc = ensure_scratch(s, &s->pool_part, &s->pool_part_bytes, pool_slots(c.n) * row_bytes(s))) return rc;
    a.part = s->pool_part;
  }
  const bool unit16 = row_bytes(s) % 16 == 0 && aligned16(s->dense) && aligned16(out) && aligned16(a.part);
  const RowShape rs = row_shape(s->width, s->vb, unit16);
  LaunchTimer t(s, kTimePooled, c.n);
  PSKV_HIP(launch_row_pooled_chunks(s->dtype, a, s->read_view(s->dense), s->ovf, rs, s->stream));
  PSKV_HIP(launch_row_pooled(s->dtype, s->tune_nt, a, s->read_view(s->dense), s->ovf, rs, s->stream));
  t.done();
  return PSKV_OK;
}

// The arguments hold (pskv_get_pooled checked them, a host call's offsets
// included).  A call of bags without a key still writes its rows of zeros.
int pooled_impl(pskv_shard* s, const pskv_pool_batch& call, int flags) {
  ++s->n_get;
  if (call.nbags == 0) return PSKV_OK;
  HstageHold hold(s);
  std::vector<pskv_pool_batch> v;
  int rc = pool_front(s, {call}, nullptr, flags,
                      PoolFront{"pskv_get_pooled", /*writing=*/false, /*with_rows=*/false,
                                "a pooled pull reads the dense array only, not the overflow table; out is untouched"},
                      hold, &v);
  if (rc || (rc = pooled_device(s, v[0])) || (flags & PSKV_DEVICE)) return rc;
  // host buffers: the pooled rows lie behind keys, weights and offsets in the staging
  const size_t at = static_cast<const char*>(v[0].bag_grads) - static_cast<char*>(s->dstage);
  std::vector<Piece> back;
  add_pieces(back, static_cast<char*>(s->hstage) + at, static_cast<char*>(const_cast<void*>(call.bag_grads)),
             call.nbags * row_bytes(s), -1);
  return rows_to_host(s, hold, at, call.nbags * row_bytes(s), "shard stream (pooled pull to host)", back);
}

// -------------------------------------------------------- optimizer steps
// pskv_apply (pskv.h): one call is one step.  Any width, 1
// included: a width-1 shard's step runs on these row kernels, not on the
// scalar paths.  Launches per call of G launch groups (step_device):
//   G x K4a (stamp mode, one epoch per group)   the winner element of each key
//   G x k_row_step_losers                       every other element's row -> gsum
//   G x k_row_step_apply                        each winner steps its key's row
// All marks come first: a key's stamp then belongs to the last group that
// holds it, the key's elements in earlier groups all see a foreign stamp and
// go to gsum, and exactly one element of the call applies the rule.
// Momentum and Adam add a second state array, the step
// counter opt_step (one per call: Adam's bias corrections are computed from it
// here, in double) and pskv_put_state, the row assign Add aimed at a state array.
// (The state slots of a kind: opt_slots, pskv_plan.h; the arrays: pskv_shard::row_array.)
size_t opt_array_bytes(const pskv_shard* s) { return s->rows_held() * row_bytes(s); }

// The hyper-parameters of step `step` as a launch takes them, in double; a
// field the kind does not use is 0.
OptArgs<double> opt_args(const pskv_optimizer_cfg& c, uint64_t step) {
  OptArgs<double> o{};
  o.lr = c.lr;
  o.wd = c.weight_decay;
  o.eps = c.eps;
  if (c.kind == PSKV_OPT_MOMENTUM) {
    o.mu = c.momentum;
    o.nesterov = c.nesterov;
  } else if (c.kind == PSKV_OPT_ADAM) {
    o.beta1 = c.beta1;
    o.beta2 = c.beta2;
    o.omb1 = 1.0 - c.beta1;
    o.omb2 = 1.0 - c.beta2;
    o.a = c.lr / (1.0 - std::pow(c.beta1, (double)step));
    o.b = 1.0 / std::sqrt(1.0 - std::pow(c.beta2, (double)step));
  } else if (c.kind == PSKV_OPT_FTRL) {
    o.l1 = c.l1;
    o.l2 = c.l2;
    o.fbeta = c.ftrl_beta;
    o.inv_lr = 1.0 / c.lr;
  }
  return o;
}

// `start` over rows [first_row, first_row + rows), the last rows of a
// row-shaped array, and zero over the zero row a sparse shard keeps behind
// them (stream-ordered; zeros are one memset, another value is k_fill).
int fill_rows(pskv_shard* s, void* array, uint64_t first_row, uint64_t rows, double start) {
  const size_t rb = row_bytes(s);
  char* at = static_cast<char*>(array) + first_row * rb;
  const uint64_t zero_rows = s->sparse ? 1 : 0;
  if (start == 0.0 && !std::signbit(start)) {
    PSKV_HIP(hipMemsetAsync(at, 0, (rows + zero_rows) * rb, s->stream));
    return PSKV_OK;
  }
  PSKV_HIP(launch_fill(s->dtype, at, rows * (uint64_t)s->width, start, s->stream));
  if (zero_rows) PSKV_HIP(hipMemsetAsync(at + rows * rb, 0, rb, s->stream));
  return PSKV_OK;
}

// The state back to its start values (row_array: Adagrad's h and FTRL's n
// init_accum, every other slot 0), the gradient scratch to zero
// (stream-ordered), the step count to 0.
int opt_reset_state(pskv_shard* s) {
  s->opt_step = 0;
  for (int a : {3, 1, 2})  // the gradient scratch, then the state slots
    if (const auto ra = s->row_array(a); ra.used)
      if (int rc = fill_rows(s, *ra.p, 0, s->range, ra.start)) return rc;
  return PSKV_OK;
}

// ------------------------------------------- sparse shards: growth and erase
// DESIGN.md §8l.  One routine behind pskv_sparse_reserve, automatic growth and
// pskv_sparse_erase: every array of the shard is built again at `new_capacity`
// slots from slot_keys[0 .. count) and swapped in.
struct DevBuf {  // a device allocation that is freed unless it was swapped into the shard
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  bool alloc(size_t bytes) {
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) p = nullptr;
    return p != nullptr;
  }
  // The allocation takes the place of the shard's `field`; what was there goes with this DevBuf.
  template <typename T>
  void swap_with(T*& field) {
    void* old = field;
    field = static_cast<T*>(p);
    p = old;
  }
};

// dead: null (growth: every slot keeps its number and its rows move by plain
// copies), or capacity + 1 flags set in stream order before this call (erase:
// the slots without a flag are compacted, k_index_rebuild).  Waits for the
// stream first and last; every new array is allocated before anything is
// touched, so PSKV_ENOMEM leaves the shard as it was.  The launches are not
// timed operations.
int sparse_rebuild(pskv_shard* s, uint64_t new_capacity, const uint8_t* dead) {
  uint64_t count = 0;
  if (int rc = sparse_count(s, &count)) return rc;
  const size_t rb = row_bytes(s);
  const uint64_t table_slots = sparse_table_slots(new_capacity);
  DevBuf rows[pskv_shard::kRowArrays], owner, slot_keys, table, survivors;
  bool ok = true;
  for (int a = 0; a < pskv_shard::kRowArrays; ++a)
    if (s->row_array(a).used) ok = ok && rows[a].alloc((new_capacity + 1) * rb);
  if (s->owner) ok = ok && owner.alloc(new_capacity * sizeof(unsigned long long));
  ok = ok && slot_keys.alloc(new_capacity * sizeof(uint32_t)) && table.alloc(table_slots * sizeof(unsigned long long));
  if (dead) ok = ok && survivors.alloc((size_t)count * sizeof(uint32_t));
  if (!ok) {
    (void)hipGetLastError();
    return fail(PSKV_ENOMEM, "sparse shard rebuild: allocating the arrays of " + std::to_string(new_capacity) +
                                 " slots failed (the shard is unchanged)");
  }
  // the index
  PSKV_HIP(hipMemsetAsync(table.p, 0, table_slots * sizeof(unsigned long long), s->stream));
  if (dead) PSKV_HIP(hipMemsetAsync(s->ovf.c->stat, 0, sizeof(uint32_t), s->stream));  // the new slot counter
  const SparseIndex nx{static_cast<unsigned long long*>(table.p), static_cast<uint32_t*>(slot_keys.p), s->ovf.c->stat,
                       table_slots - 1, (uint32_t)new_capacity};
  PSKV_HIP(launch_index_rebuild(s->sp_slot_keys, (uint32_t)count, dead, nx, static_cast<uint32_t*>(survivors.p),
                                s->stream));
  uint64_t kept = count;
  if (dead) {  // how many survived: the gather below is sized by it
    if (int rc = sparse_count(s, &kept)) return rc;
    kept = std::min(kept, count);
  }
  // the rows of the survivors (the gradient scratch carries none: it is zero
  // between calls), then each array's start value behind them
  for (int a = 0; a < pskv_shard::kRowArrays; ++a) {
    const pskv_shard::RowArray ra = s->row_array(a);
    if (!ra.used) continue;
    char* fresh = static_cast<char*>(rows[a].p);
    const uint64_t carried = ra.p == &s->opt_gsum ? 0 : kept;
    if (carried && !dead)
      PSKV_HIP(hipMemcpyAsync(fresh, *ra.p, (size_t)carried * rb, hipMemcpyDeviceToDevice, s->stream));
    if (carried && dead) {
      const std::vector<pskv_batch> mv{pskv_batch{static_cast<const uint32_t*>(survivors.p), fresh, carried}};
      const LaunchGroup g = make_group(mv, 0, 1, kGeneralChunk);
      const DenseView from{*ra.p, 0, s->rows_held(), 0};
      const RowShape rs = row_shape(s->width, s->vb, rows_unit16(s, {from.param}, mv));
      PSKV_HIP(launch_row_gather(s->vb, s->tune_nt, g.ga, g.nwg, from, rs, s->stream));
    }
    if (int rc = fill_rows(s, fresh, carried, new_capacity - carried, ra.start)) return rc;
  }
  if (owner.p) PSKV_HIP(hipMemsetAsync(owner.p, 0, new_capacity * sizeof(unsigned long long), s->stream));
  if (int rc = wait_stream(s, s->stream, "shard stream (sparse rebuild)")) return rc;
  // nothing is queued: the new arrays take over and the old ones go with the DevBufs
  for (int a = 0; a < pskv_shard::kRowArrays; ++a)
    if (rows[a].p) rows[a].swap_with(*s->row_array(a).p);
  if (owner.p) owner.swap_with(s->owner);
  slot_keys.swap_with(s->sp_slot_keys);
  table.swap_with(s->sp_table);
  s->sp_table_slots = table_slots;
  s->range = new_capacity;
  s->sp_bound = kept;
  s->ocount_known = kept;
  ++s->sp_rebuilds;
  return PSKV_OK;
}

// The growth rule of a writing call of n key positions (pskv.h "Sparse
// shards"; sparse_grown_capacity, pskv_plan.h).  The count is read -- one
// bounded stream wait -- only when the host-side bound cannot rule the growth
// out (sparse_may_grow): both then make the same decision.
int sparse_autogrow(pskv_shard* s, uint64_t n) {
  if (sparse_may_grow(s->sp_bound, n, s->range, s->sp_max_capacity)) {
    uint64_t count = 0;
    if (int rc = sparse_count(s, &count)) return rc;
    const uint64_t want = sparse_grown_capacity(s->range, count, n, s->sp_max_capacity);
    if (want != s->range)
      if (int rc = sparse_rebuild(s, want, nullptr)) return rc;
  }
  s->sp_bound = std::min(s->sp_bound + n, s->range);  // (count never exceeds the capacity)
  return PSKV_OK;
}

// One step, timed as one operation (kTimeApply).  `marks`: the call's batches
// as the mark takes them (keys and n; vals: where the kernels read the batch's
// rows), `spans` their launch groups; args_of(mark group, span): the argument
// block of a group's loser and apply passes (GroupArgs, PoolPushArgs or
// PoolGroupArgs, pskv_internal.h).
template <typename Args, typename ArgsOf>
int step_device(pskv_shard* s, const std::vector<pskv_batch>& marks, const std::vector<Span>& spans,
                const ArgsOf& args_of) {
  if (int rc = ensure_owner(s)) return rc;
  // 16-byte units for the whole call or for none of it
  const bool vec = rows_unit16(s, {s->dense, s->opt_gsum, s->opt_slot[0], s->opt_slot[1]}, marks);
  struct Group {
    LaunchGroup mark;
    Args a;
    uint32_t epoch;
  };
  std::vector<Group> groups(spans.size());
  uint64_t elems = 0;
  // the call's epochs must not straddle a wrap-around (next_epoch resets the
  // stamps there): take the wrap first.  (One group: nothing to do here,
  // next_epoch takes a wrap-around itself.)
  if (0xFFFFFFFFu - s->epoch < spans.size()) s->epoch = 0xFFFFFFFFu;
  for (size_t i = 0; i < spans.size(); ++i) {
    Group& g = groups[i];
    g.mark = make_group(marks, spans[i].first, spans[i].second, kGeneralChunk);
    g.a = args_of(g.mark, spans[i]);
    g.epoch = next_epoch(s);
    elems += g.mark.elems;
  }
  // one step number for the whole call, whatever its launch groups
  const OptArgs<double> hy = opt_args(s->opt, ++s->opt_step);
  const RowShape rs1 = row_shape(s->width, s->vb, false);
  const RowShape rsv = row_shape(s->width, s->vb, vec);
  LaunchTimer t(s, kTimeApply, elems);
  t.count = groups.size();
  for (const Group& g : groups)
    PSKV_HIP(launch_general_mark(s->dtype, PSKV_ASSIGN, g.mark.ga, g.mark.nwg, s->dview(), s->flag + 1, s->owner,
                                 nullptr, g.epoch, s->stream));
  for (const Group& g : groups)
    PSKV_HIP(launch_row_step_losers(s->dtype, g.a, g.mark.nwg, s->dview(), s->opt_gsum, s->owner, s->ovf, g.epoch, rs1,
                                    s->stream));
  for (const Group& g : groups)
    PSKV_HIP(launch_row_step_apply(s->dtype, s->opt.kind, g.a, g.mark.nwg, s->dview(), s->opt_gsum, s->opt_slot,
                                   s->owner, g.epoch, rsv, hy, s->stream));
  t.done();
  s->n_general += 3 * groups.size();
  return PSKV_OK;
}

int apply_device(pskv_shard* s, const std::vector<pskv_batch>& v) {
  return step_device<GroupArgs>(s, v, split_groups(v), [](const LaunchGroup& mark, const Span&) { return mark.ga; });
}

int apply_impl(pskv_shard* s, const std::vector<pskv_batch>& in, int flags) {
  if (s->opt.kind == PSKV_OPT_NONE)
    return fail(PSKV_EINVAL, "pskv_apply: the shard has no optimizer (pskv_shard_set_optimizer)");
  // a width-1 shard's resident request server runs alone on the shard: as
  // every stream path of add_impl / get_impl, the front ends it first (K8
  // launches are ordinary work of the shard's stream and need nothing)
  HstageHold hold(s);  // the call returns before its DMA: the hold stays armed
  RowCall c;
  if (int rc = rows_front(s, in, flags,
                          RowFront{"pskv_apply", nullptr, /*stop_server=*/true, "key",
                                   "an optimizer step takes no out-of-range keys", /*with_values=*/true},
                          hold, &c))
    return rc;
  return c.v.empty() ? PSKV_OK : apply_device(s, c.views());
}

// ----------------------------------------------------------- pooled pushes
// pskv_apply_pooled (pskv.h "Pooled pushes"): pskv_apply's step
// for one batch whose gradient rows the kernels form themselves,
// weights[i] * bag_grads[bag(i)].  One launch group (n <= kMaxPiece) of
// step_device, its passes over a PoolPushArgs; K4a is unchanged, it reads keys
// only.  pskv_apply_pooled_grouped (pskv.h "Grouped pooled pushes", DESIGN.md
// §8h): the pooled pushes of several workers as ONE step, the live batches cut
// into launch groups (pool_split_groups), the passes over a PoolGroupArgs each.
// The offsets stay where the caller has them: a device call's launches do not
// depend on them, the kernels' bag lookup stays below nbags whatever they hold.
// `v`: live batches where the kernels read them.
int apply_pooled_device(pskv_shard* s, const pskv_pool_batch& c) {
  return step_device<PoolPushArgs>(s, pool_mark_batches({c}), {Span{0, 1}}, [&](const LaunchGroup&, const Span&) {
    return PoolPushArgs{c.keys, c.weights, c.offsets, c.n, c.nbags, c.bag_grads};
  });
}

int apply_pooled_grouped_device(pskv_shard* s, const std::vector<pskv_pool_batch>& v) {
  return step_device<PoolGroupArgs>(s, pool_mark_batches(v), pool_split_groups(v),
                                    [&](const LaunchGroup&, const Span& sp) {
                                      uint32_t nwg = 0;
                                      uint64_t elems = 0;
                                      return make_pool_group(v, sp.first, sp.second, kGeneralChunk, &nwg, &elems);
                                    });
}

// Why the shard takes no pooled step (behind the call's name), or null.
const char* pooled_step_refusal(const pskv_shard* s) {
  if (s->dtype != PSKV_F32 && s->dtype != PSKV_F64)
    return ": float shards only (an int32 shard takes no optimizer step)";
  if (s->opt.kind == PSKV_OPT_NONE) return ": the shard has no optimizer (pskv_shard_set_optimizer)";
  return nullptr;
}

// A pooled push's front: it inserts, and a host call stages its bag rows.
PoolFront pooled_push_front(const char* what) {
  return PoolFront{what, /*writing=*/true, /*with_rows=*/true, "an optimizer step takes no out-of-range keys"};
}

// The arguments hold (pskv_apply_pooled checked them, a host call's offsets included).
int apply_pooled_impl(pskv_shard* s, const pskv_pool_batch& call, int flags) {
  if (const char* why = pooled_step_refusal(s)) return fail(PSKV_EINVAL, std::string("pskv_apply_pooled") + why);
  if (call.n == 0 || call.nbags == 0) return PSKV_OK;  // no key, or no bag to take a row from: no step
  HstageHold hold(s);  // a host call returns before its DMA: the hold stays armed
  std::vector<pskv_pool_batch> v;
  if (int rc = pool_front(s, {call}, nullptr, flags, pooled_push_front("pskv_apply_pooled"), hold, &v)) return rc;
  return apply_pooled_device(s, v[0]);
}

// The arguments hold (pskv_apply_pooled_grouped checked every batch, a host
// call's offsets included).
int apply_pooled_grouped_impl(pskv_shard* s, const pskv_pool_batch* batches, uint64_t nb, int flags) {
  if (const char* why = pooled_step_refusal(s))
    return fail(PSKV_EINVAL, std::string("pskv_apply_pooled_grouped") + why);
  std::vector<uint64_t> index;
  const std::vector<pskv_pool_batch> live = pool_live_batches(batches, nb, &index);
  if (live.empty()) return PSKV_OK;  // no batch with a key and a bag: no step
  HstageHold hold(s);  // a host call returns before its DMA: the hold stays armed
  std::vector<pskv_pool_batch> v;
  if (int rc = pool_front(s, live, &index, flags, pooled_push_front("pskv_apply_pooled_grouped"), hold, &v)) return rc;
  return apply_pooled_grouped_device(s, v);
}

// What is wrong with a configuration, or null (checked before any handle;
// fields a kind does not use are ignored).  legacy: the configuration was
// widened from a pskv_optimizer, which has no size and only the first kinds.
// kOptEx: widened from a pskv_optimizer_ex, which ends before FTRL's fields
// and knows the kinds up to Adam.  c.size is the size of the caller's struct.
enum OptAbi { kOptLegacy, kOptEx, kOptCfg };
static_assert(sizeof(pskv_optimizer_ex) == 72 && offsetof(pskv_optimizer_cfg, beta2) == offsetof(pskv_optimizer_ex, beta2) &&
                  offsetof(pskv_optimizer_cfg, l1) == sizeof(pskv_optimizer_ex) && sizeof(pskv_optimizer_cfg) == 96,
              "pskv_optimizer_cfg begins as pskv_optimizer_ex and adds three doubles");
const char* opt_config_error(const pskv_optimizer_cfg& c, OptAbi abi) {
  if (abi == kOptLegacy) {
    if (c.kind != PSKV_OPT_NONE && c.kind != PSKV_OPT_SGD && c.kind != PSKV_OPT_ADAGRAD)
      return "kind must be PSKV_OPT_NONE, PSKV_OPT_SGD or PSKV_OPT_ADAGRAD";
  } else if (abi == kOptEx) {
    if (c.size != sizeof(pskv_optimizer_ex)) return "size must be sizeof(pskv_optimizer_ex)";
    if (c.kind < PSKV_OPT_NONE || c.kind > PSKV_OPT_ADAM)
      return "kind must be PSKV_OPT_NONE, PSKV_OPT_SGD, PSKV_OPT_ADAGRAD, PSKV_OPT_MOMENTUM or PSKV_OPT_ADAM";
  } else {
    if (c.size != sizeof(pskv_optimizer_cfg)) return "size must be sizeof(pskv_optimizer_cfg)";
    if (c.kind < PSKV_OPT_NONE || c.kind > PSKV_OPT_FTRL)
      return "kind must be PSKV_OPT_NONE, PSKV_OPT_SGD, PSKV_OPT_ADAGRAD, PSKV_OPT_MOMENTUM, PSKV_OPT_ADAM or "
             "PSKV_OPT_FTRL";
  }
  if (c.kind == PSKV_OPT_NONE) return nullptr;
  if (!std::isfinite(c.lr) || !(c.lr > 0)) return "lr must be finite and > 0";
  if (!std::isfinite(c.weight_decay) || !(c.weight_decay >= 0)) return "weight_decay must be finite and >= 0";
  if (c.kind == PSKV_OPT_ADAGRAD || c.kind == PSKV_OPT_ADAM)
    if (!std::isfinite(c.eps) || !(c.eps > 0)) return "eps must be finite and > 0";
  if (c.kind == PSKV_OPT_ADAGRAD || c.kind == PSKV_OPT_FTRL)
    if (!std::isfinite(c.init_accum) || !(c.init_accum >= 0)) return "init_accum must be finite and >= 0";
  if (c.kind == PSKV_OPT_MOMENTUM) {
    if (!std::isfinite(c.momentum) || !(c.momentum >= 0) || !(c.momentum < 1))
      return "momentum must be finite and in [0, 1)";
    if (c.nesterov != 0 && c.nesterov != 1) return "nesterov must be 0 or 1";
  }
  if (c.kind == PSKV_OPT_ADAM) {
    if (!std::isfinite(c.beta1) || !(c.beta1 >= 0) || !(c.beta1 < 1)) return "beta1 must be finite and in [0, 1)";
    if (!std::isfinite(c.beta2) || !(c.beta2 >= 0) || !(c.beta2 < 1)) return "beta2 must be finite and in [0, 1)";
  }
  if (c.kind == PSKV_OPT_FTRL) {
    if (!std::isfinite(c.l1) || !(c.l1 >= 0)) return "l1 must be finite and >= 0";
    if (!std::isfinite(c.l2) || !(c.l2 >= 0)) return "l2 must be finite and >= 0";
    if (!std::isfinite(c.ftrl_beta) || !(c.ftrl_beta >= 0)) return "ftrl_beta must be finite and >= 0";
  }
  return nullptr;
}

int add_impl(pskv_shard* s, const std::vector<pskv_batch>& in, int flags) {
  if (s->width > 1 || s->sparse) return rows_add(s, in, flags);
  std::vector<pskv_batch> v;
  for (auto& b : in) {
    if (b.n == 0) continue;
    if (!b.keys || !b.vals) return fail(PSKV_EINVAL, "pskv_add: null keys/vals with n > 0");
    push_pieces(v, b, (size_t)s->vb);
  }
  s->n_add++;
  if (v.empty()) return PSKV_OK;
  int rc = use_device(s);
  if (rc) return rc;
  const bool device = (flags & PSKV_DEVICE) != 0;
  if (!device && s->tune_inline) {
    uint64_t total = 0;
    for (const auto& b : v) total += b.n;
    if (total <= (uint64_t)kInlineMax * s->tune_inline_add_chunks) return inline_add(s, v);
  }
  rc = srv_stop(s);
  if (rc) return rc;
  bool host_verified = false, host_dense = false;
  std::vector<pskv_batch> framed;  // the host batches, when they are borrowed frames
  // Every exit records the frames' queued uses (pskv_host_free holds a frame
  // until they have run): a failure after some work was queued must not let
  // the frame be reused while that work still reads it.
  auto run = [&]() -> int {
    int rc = PSKV_OK;
    if (!device) {
      // (out-of-range keys need no host step: the single workgroup that
      // inserts them reserves room on the device, ovf_reserve)
      std::vector<pskv_batch> staged, views;
      if ((flags & PSKV_HOST_FRAME) && frame_views(v, (size_t)s->vb, &views)) {
        framed = v;
        rc = frame_batches(s, v, views, &staged, &host_verified, &host_dense);
      } else {
        rc = stage_host_batches(s, v, &staged, &host_verified, &host_dense);
      }
      if (rc) return rc;
      v.swap(staged);
    }
    const bool vec = all_aligned16(v);
    for (auto& g : split_groups(v)) {
      // a replay held by the previous group goes before this group's launches
      if ((rc = flush_replay(s))) return rc;
      const uint32_t epoch = next_epoch(s);
      if (s->mode == PSKV_ACCUMULATE) {
        if (!device && host_dense) {
          // the CPU proved every batch a dense in-range window while staging it
          rc = dense_accumulate(s, v, g.first, g.second, epoch, /*verify=*/false);
        } else if (device && (flags & PSKV_SORTED_HINT)) {
          rc = dense_accumulate(s, v, g.first, g.second, epoch, /*verify=*/true);
        } else {
          // K5 (no global atomics) measured faster than K4a (LDS sums + one
          // atomic add per distinct key per chunk) on cfg 3: 322 vs 380 us per
          // 8M Zipf keys; PSKV_GENERAL=stamps selects K4a
          rc = general_add(s, v, g.first, g.second, epoch);
        }
      } else if (!device && host_verified) {
        // the CPU proved the batches sorted and in range while staging them.
        // Sorted is not dense: a sorted batch that repeats a key and misses
        // another spans exactly n - 1 keys like a window (keys 5, 6, 6, 8), so
        // K2g's dense mode takes it and its per-element check tags it; the
        // replay then applies the group in order.  Only batches the CPU proved
        // strictly contiguous cannot trip that check and skip the replay.
        rc = sorted_add(s, v, g.first, g.second, vec, epoch, /*repair=*/!host_dense, host_dense);
      } else if (device && (flags & PSKV_SORTED_HINT)) {
        rc = sorted_add(s, v, g.first, g.second, vec, epoch, /*repair=*/true, /*maybe_windows=*/true);
      } else {
        rc = general_add(s, v, g.first, g.second, epoch);
      }
      if (rc) return rc;
    }
    return PSKV_OK;
  };
  rc = run();
  if (!framed.empty()) {
    std::string err = rc ? g_last_error : std::string();
    const int rn = note_frame_uses(s, framed);
    if (rc) {
      g_last_error = err;  // report the first failure
      return rc;
    }
    return rn;
  }
  return rc;
}

// K1 over one launch group, batches [b, e) of `v`.  fold_replay: a replay the
// Add of pskv_add_get_grouped held rides on this launch (K1r); it stays held
// (for add_get_impl's trailing K4r) unless the launch is queued.
int gather_group(pskv_shard* s, const std::vector<pskv_batch>& v, size_t b, size_t e, bool vec, bool fold_replay) {
  int gu = 0;
  const LaunchGroup g = make_group_by(v, b, e, [&](uint64_t elems) {
    gu = gather_unroll(s, elems);
    return (uint64_t)stream_chunk(gu);
  });
  LaunchTimer t(s, PSKV_K_GATHER, g.elems);
  if (fold_replay && s->pend_replay && g.nwg > 0) {
    PSKV_HIP(launch_gather_replay(s->vb, vec, gu, s->tune_nt, g.ga, g.nwg, s->dview(), s->ovf, s->pend_rg,
                                  s->flag, s->pend_epoch, s->flag + 16, s->stream));
    s->pend_replay = false;
  } else {
    PSKV_HIP(launch_gather(s->vb, vec, gu, s->tune_nt, g.ga, g.nwg, s->dview(), s->ovf, s->stream));
  }
  t.done();
  return PSKV_OK;
}

// K1 over every launch group of `v`: the K1 loop of every Get path.
int gather_all(pskv_shard* s, const std::vector<pskv_batch>& v, bool vec, bool fold_replay = false) {
  for (const Span& g : split_groups(v))
    if (int rc = gather_group(s, v, g.first, g.second, vec, fold_replay)) return rc;
  return PSKV_OK;
}

// Get in place, page-locked keys and outputs (frames, PSKV_HOST_FRAME, or any
// other pinned memory): K1 reads the keys from and writes the values into the
// caller's buffers, no copy on either side.
int zero_copy_get_views(pskv_shard* s, const std::vector<pskv_batch>& hv) {
  if (int rc = gather_all(s, hv, all_aligned16(hv))) return rc;
  return wait_stream(s, s->stream, "shard stream (Get into page-locked memory)");
}

// Zero-copy host Get of a medium batch: the keys are copied into pinned staging
// by the calling thread, K1 reads them from there and writes the values into
// pinned staging over PCIe (no DMA engine on either side), and the calling
// thread copies the values out.  The staging is default (non-coherent) pinned
// memory: the kernel's writes are visible once the stream is synchronised.
int zero_copy_get(pskv_shard* s, const std::vector<pskv_batch>& v) {
  const StageLayout lay = stage_layout(v, (size_t)s->vb, StageOrder::kKeysFirst);
  if (int rc = ensure_hstage(s, lay.total)) return rc;
  const std::vector<pskv_batch> hv = lay.views(v, static_cast<char*>(s->hstage));
  for (size_t i = 0; i < v.size(); ++i) std::memcpy(const_cast<uint32_t*>(hv[i].keys), v[i].keys, v[i].n * 4);
  HstageHold hold(s);
  hold.arm();  // K1 reads the keys from and writes the values into the staging
  if (int rc = gather_all(s, hv, /*vec=*/true)) return rc;
  if (int rc = wait_stream(s, s->stream, "shard stream (zero-copy Get)")) return rc;
  hold.dismiss();
  for (size_t i = 0; i < v.size(); ++i) std::memcpy(v[i].vals, hv[i].vals, v[i].n * (size_t)s->vb);
  return PSKV_OK;
}

// Get from page-locked caller buffers by DMA: the batches go in windows of
// about kWindowBytes of keys; per window the keys are DMA'd in and K1 runs on
// the shard's stream, and the window's values are DMA'd out on a second
// stream once its K1 is done, so the values of window w travel to the host
// while the keys of window w+1 travel to the device (PCIe is full duplex; the
// two directions use different DMA engines).  The call returns when every
// value has arrived.
int pinned_get(pskv_shard* s, const std::vector<pskv_batch>& v) {
  const StageLayout lay = stage_layout(v, (size_t)s->vb, StageOrder::kInterleaved);
  int rc = ensure_dstage(s, lay.total);
  if (rc) return rc;
  if (!s->out_stream) {
    PSKV_HIP(hipStreamCreateWithFlags(&s->out_stream, hipStreamNonBlocking));
    g_queues.add_stream(s->device, 1);
  }
  const std::vector<pskv_batch> dv = lay.views(v, static_cast<char*>(s->dstage));
  const bool vec = all_aligned16(dv);
  const std::vector<Span> wins = batch_windows(v);  // each one launch group
  while (s->out_events.size() < wins.size()) {
    hipEvent_t e = nullptr;
    PSKV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s->out_events.push_back(e);
  }
  for (size_t w = 0; w < wins.size(); ++w) {
    const size_t b = wins[w].first, e = wins[w].second;
    for (size_t i = b; i < e; ++i)
      PSKV_HIP(hipMemcpyAsync(const_cast<uint32_t*>(dv[i].keys), v[i].keys, v[i].n * 4, hipMemcpyHostToDevice,
                              s->stream));
    if ((rc = gather_group(s, dv, b, e, vec, /*fold_replay=*/false))) return rc;
    PSKV_HIP(hipEventRecord(s->out_events[w], s->stream));
    PSKV_HIP(hipStreamWaitEvent(s->out_stream, s->out_events[w], 0));
    for (size_t i = b; i < e; ++i)
      PSKV_HIP(hipMemcpyAsync(v[i].vals, dv[i].vals, v[i].n * (size_t)s->vb, hipMemcpyDeviceToHost,
                              s->out_stream));
  }
  // the stage is free again once the out stream is done; both streams drained
  if ((rc = wait_stream(s, s->out_stream, "D2H output stream (page-locked Get)"))) return rc;
  return wait_stream(s, s->stream, "shard stream (page-locked Get)");
}

// Pageable host Get through both stagings: keys -> pinned -> device
// (pipelined), K1, then the values D2H into the pinned staging behind the keys
// window by window; the pool copies window w out to the caller while window
// w+1 is still in flight.
int staged_get(pskv_shard* s, const std::vector<pskv_batch>& v) {
  HstageHold hold(s);
  const StageLayout lay = stage_layout(v, (size_t)s->vb, StageOrder::kKeysFirst);
  std::vector<pskv_batch> dv;
  int rc = stage_keys_first(s, v, lay, (size_t)s->vb, /*with_values=*/false, hold, &dv);
  if (!rc) rc = gather_all(s, dv, all_aligned16(dv));
  if (rc) return rc;
  char* h = static_cast<char*>(s->hstage);
  char* d = static_cast<char*>(s->dstage);
  std::vector<Piece> pieces;  // pinned -> caller
  for (size_t i = 0; i < v.size(); ++i)
    add_pieces(pieces, h + lay.at[i].vals, static_cast<char*>(v[i].vals), v[i].n * (size_t)s->vb, -1);
  const std::vector<Span> wins = piece_windows(pieces);
  while (s->win_events.size() < wins.size()) {
    hipEvent_t e = nullptr;
    PSKV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s->win_events.push_back(e);
  }
  for (size_t w = 0; w < wins.size(); ++w) {
    const char* lo = pieces[wins[w].first].src;
    const char* hi = pieces[wins[w].second - 1].src + pieces[wins[w].second - 1].bytes;
    PSKV_HIP(hipMemcpyAsync(const_cast<char*>(lo), d + (lo - h), (size_t)(hi - lo), hipMemcpyDeviceToHost,
                            s->stream));
    PSKV_HIP(hipEventRecord(s->win_events[w], s->stream));
  }
  for (size_t w = 0; w < wins.size(); ++w) {
    if ((rc = wait_event(s, s->win_events[w], "D2H window event (Get to host)", s->win_events[w]))) return rc;
    run_copies(s, pieces, wins[w].first, wins[w].second);
  }
  hold.dismiss();
  return PSKV_OK;
}

// The path choice of a Get.  Host calls, in this order: inline (K8 / K9),
// in-place zero copy, staged zero copy, DMA (page-locked, or pageable and
// large), staged windowed.
int get_impl(pskv_shard* s, const std::vector<pskv_batch>& in, int flags) {
  if (s->width > 1 || s->sparse) return rows_get(s, in, flags);
  std::vector<pskv_batch> v;
  for (auto& b : in) {
    if (b.n == 0) continue;
    if (!b.keys || !b.vals) return fail(PSKV_EINVAL, "pskv_get: null keys/out with n > 0");
    push_pieces(v, b, (size_t)s->vb);
  }
  s->n_get++;
  if (v.empty()) return PSKV_OK;
  int rc = use_device(s);
  if (rc) return rc;
  const bool device = (flags & PSKV_DEVICE) != 0;
  if (!device && s->tune_inline) {
    uint64_t total = 0;
    for (const auto& b : v) total += b.n;
    if (total <= (uint64_t)kInlineGetMax * s->tune_inline_get_chunks) return inline_get(s, v, total);
  }
  rc = srv_stop(s);
  if (rc) return rc;
  if (device) return gather_all(s, v, all_aligned16(v), /*fold_replay=*/true);
  const size_t bytes = staged_bytes(v, (size_t)s->vb);
  std::vector<pskv_batch> views;
  if (bytes <= s->tune_frame_zc_max_bytes &&
      (((flags & PSKV_HOST_FRAME) && frame_views(v, (size_t)s->vb, &views)) ||
       pinned_views(v, (size_t)s->vb, &views)))
    return zero_copy_get_views(s, views);
  bool pinned = true;
  for (const auto& b : v) pinned = pinned && is_pinned(b.keys) && is_pinned(b.vals);
  if (!pinned && s->tune_zc_max_bytes && bytes <= s->tune_zc_max_bytes) return zero_copy_get(s, v);
  // pageable: direct DMA only when large
  if (!pinned && s->tune_pageable_dma) pinned = bytes >= s->tune_dma_min_bytes_get;
  return pinned ? pinned_get(s, v) : staged_get(s, v);
}

// ------------------------------------------------------------ Add then Get
// pskv_add_get_grouped: pskv_add_grouped(adds) followed by
// pskv_get_grouped(gets) in one call -- BSPModel::Clock's flush of the
// deferred Adds followed by the Gets it releases (server/consistency/
// bsp_model.cpp:14-31), or one producer round's push then pull.  Round 4
// built this as ONE fused launch (K10: the Add's and the Get's chunks as work
// units of one co-resident grid, pull keys the same call pushes answered
// from the pushed values) and measured it slower than the two launches at
// every size (headline 5.56 against 6.03 TB/s, the emulated N = 8 ranks
// 44.0-49.5 against 34.7-41.6 us; profiles/r04_probes/fused/): one register
// allocation for both halves costs the Get half of its waves, and a rank's
// fixed cost sits inside each kernel's ramp, not between the launches.  The
// kernel was removed; the call stays, as the two paths.
int add_get_impl(pskv_shard* s, const std::vector<pskv_batch>& adds, const std::vector<pskv_batch>& gets,
                 int flags) {
  if (s->width > 1 || s->sparse) {
    const int rc = rows_add(s, adds, flags);
    return rc ? rc : rows_get(s, gets, flags);
  }
  // Device batches, assign, 4-byte values: the Add's last conditional replay
  // is held and rides on the Get's first K1 launch (K1r) -- one launch fewer
  // per call.  The Get's device path queues nothing before that K1; whatever
  // is still held after it (an empty Get, a failure) is launched as K4r here,
  // with nothing queued in between, so stream order is the sequential one.
  s->defer_replay = s->tune_fold_replay && (flags & PSKV_DEVICE) && s->mode == PSKV_ASSIGN && s->vb == 4;
  int rc = add_impl(s, adds, flags);
  s->defer_replay = false;
  if (!rc) rc = get_impl(s, gets, flags & ~PSKV_SORTED_HINT);
  const int rf = flush_replay(s);
  return rc ? rc : rf;
}

// ------------------------------------------------------------- options
// Every tuning knob and path selector of a shard, by name: pskv_set_option /
// pskv_get_option, and the environment variable PSKV_<NAME> as the creation
// default (the earlier interface; tests and tools now set options per shard).
// Each entry validates its value; DESIGN.md §5 says what each path is for.
struct Option {
  const char* name;
  int64_t lo, hi;  // accepted range
  int64_t (*get)(const pskv_shard*);
  void (*set)(pskv_shard*, int64_t);
};

#define PSKV_OPT(NAME, LO, HI, FIELD, T)                                           \
  Option {                                                                         \
    NAME, LO, HI, [](const pskv_shard* s) -> int64_t { return (int64_t)s->FIELD; }, \
        [](pskv_shard* s, int64_t v) { s->FIELD = (T)v; }                          \
  }

const Option kOptions[] = {
    // general (any order) Add: 0 = K4 stamps, 1 = auto (K5), 2 = K5 always;
    // the environment form also takes "stamps" / "auto" / "radix"
    PSKV_OPT("GENERAL", 0, 2, general_path, int),
    PSKV_OPT("UNROLL", 4, 8, tune_unroll, int),              // 4 or 8 (others: 8)
    PSKV_OPT("GET_UNROLL", 0, 8, tune_get_unroll, int),      // 0 (by size), 4 or 8
    PSKV_OPT("FOLD_REPLAY", 0, 1, tune_fold_replay, int),   // add_get: K4r folded into K1 (K1r)
    // the stamp epoch, a test and diagnosis seam: it only moves forward (every
    // stamp and tag on the device is at most the current epoch, so a later one
    // still beats them all); no environment default
    PSKV_OPT("EPOCH", 0, 0xFFFFFFFFll, epoch, uint32_t),
    PSKV_OPT("NT", 0, 1, tune_nt, bool),
    PSKV_OPT("NTP", 0, 1, tune_ntp, bool),
    PSKV_OPT("RESIDENT_BYTES", -1, INT64_MAX, tune_resident_bytes, int64_t),  // -1 = auto, 0 = off
    PSKV_OPT("EARLY", 0, 2, tune_early, int),
    PSKV_OPT("PAGEABLE_DMA", 0, 1, tune_pageable_dma, bool),
    PSKV_OPT("DMA_MIN_BYTES", 0, INT64_MAX, tune_dma_min_bytes, size_t),
    PSKV_OPT("DMA_MIN_BYTES_GET", 0, INT64_MAX, tune_dma_min_bytes_get, size_t),
    PSKV_OPT("DMA_MIN_BYTES_PINNED", 0, INT64_MAX, tune_dma_min_bytes_pinned, size_t),
    PSKV_OPT("ZC_MAX_BYTES", 0, INT64_MAX, tune_zc_max_bytes, size_t),
    PSKV_OPT("FRAME_ZC_MAX_BYTES", 0, INT64_MAX, tune_frame_zc_max_bytes, size_t),
    PSKV_OPT("INLINE", 0, 1, tune_inline, bool),
    PSKV_OPT("INLINE_ADD_CHUNKS", 1, kInlineMaxChunks, tune_inline_add_chunks, int),
    PSKV_OPT("INLINE_GET_CHUNKS", 1, kInlineMaxChunks, tune_inline_get_chunks, int),
    PSKV_OPT("ISPIN", 0, 1, tune_ispin, bool),
    PSKV_OPT("SERVE", 0, 1, tune_serve, bool),
    PSKV_OPT("SERVE_IDLE_US", 1, 10000000, tune_serve_idle_us, uint32_t),
    PSKV_OPT("TILE_SHIFT", 0, 20, tune_tile_shift, uint32_t),  // 0 = by size, else 10..20
    PSKV_OPT("TILE_GRID", 1, 65536, tune_tile_grid, uint32_t),
    PSKV_OPT("RB_WBITS", 0, 31, tune_rb_wbits, uint32_t),
    PSKV_OPT("RB_NBD", 0, kRbMaxBuckets - 1, tune_rb_nbd, uint32_t),
    PSKV_OPT("RB_TB", 0, 11, tune_rb_tb, uint32_t),
    PSKV_OPT("RB_APPLY_LOG2", 0, 14, tune_rb_apply_log2, int),  // 0 = by size, 13 or 14
    PSKV_OPT("RB_BIN_BLOCK", 512, 1024, tune_rb_bin_block, int),  // 512 or 1024
    PSKV_OPT("SYNC_TIMEOUT_MS", 0, 0x7FFFFFFF, tune_sync_timeout_ms, uint32_t),  // 0 = unbounded waits
};
#undef PSKV_OPT

const Option* find_option(const char* name) {
  for (const auto& o : kOptions)
    if (std::strcmp(o.name, name) == 0) return &o;
  return nullptr;
}

int set_option(pskv_shard* s, const Option& o, int64_t v) {
  if (v < o.lo || v > o.hi) return fail(PSKV_EINVAL, std::string("option ") + o.name + ": value out of range");
  if (std::strcmp(o.name, "UNROLL") == 0 && v != 4 && v != 8) return fail(PSKV_EINVAL, "option UNROLL: 4 or 8");
  if (std::strcmp(o.name, "GET_UNROLL") == 0 && v != 0 && v != 4 && v != 8)
    return fail(PSKV_EINVAL, "option GET_UNROLL: 0, 4 or 8");
  if (std::strcmp(o.name, "TILE_SHIFT") == 0 && v != 0 && v < 10) return fail(PSKV_EINVAL, "option TILE_SHIFT: 0 or 10..20");
  if (std::strcmp(o.name, "RB_APPLY_LOG2") == 0 && v != 0 && v != 13 && v != 14)
    return fail(PSKV_EINVAL, "option RB_APPLY_LOG2: 0, 13 or 14");
  if (std::strcmp(o.name, "RB_BIN_BLOCK") == 0 && v != 512 && v != 1024)
    return fail(PSKV_EINVAL, "option RB_BIN_BLOCK: 512 or 1024");
  if (std::strcmp(o.name, "EPOCH") == 0 && v < (int64_t)s->epoch)
    return fail(PSKV_EINVAL, "option EPOCH: the epoch only moves forward");
  o.set(s, v);
  if (std::strcmp(o.name, "SYNC_TIMEOUT_MS") == 0) refresh_grow_wait(s);
  if (std::strcmp(o.name, "INLINE_ADD_CHUNKS") == 0) s->add_chunks_set = true;
  // a ring slot costs the host ~0.2 us where a K8 launch costs 3-7: with the
  // server, Adds of up to 2 slots (512 keys) take it unless the chunk count
  // was chosen.  Measured (tools/micro/small_latency.cpp, Add then Get): 512
  // keys 17-18 us against 23-27 through the copy; from 1 Ki keys the server's
  // per-slot work (~6 us per 256-key slot) is behind the copy (1 Ki: 31-34
  // against 28)
  if (std::strcmp(o.name, "SERVE") == 0 && !s->add_chunks_set) s->tune_inline_add_chunks = v ? 2 : 1;
  return PSKV_OK;
}

// The environment only sets creation defaults: a value that does not parse or
// that pskv_set_option would reject is reported on stderr (once per variable
// and process) and ignored -- the option keeps its built-in default, and the
// shard is created as without the variable.  pskv_set_option itself stays
// strict (PSKV_EINVAL).
int apply_env_options(pskv_shard* s) {
  static std::mutex warn_mu;
  static std::vector<std::string> warned;
  // options removed after measurement: a script that still sets
  // one would otherwise measure the default path without a word
  static const char* const kRetired[] = {"RB_INSERT", "GET_DEDUP", "GET_NTP", "FUSE"};
  for (const char* name : kRetired) {
    const std::string var = std::string("PSKV_") + name;
    const char* e = std::getenv(var.c_str());
    if (!e || !*e) continue;
    std::lock_guard<std::mutex> g(warn_mu);
    if (std::find(warned.begin(), warned.end(), var) == warned.end()) {
      warned.push_back(var);
      std::fprintf(stderr, "pskv: ignoring environment %s=%s (a retired option: that path was removed)\n",
                   var.c_str(), e);
    }
  }
  for (const auto& o : kOptions) {
    if (std::strcmp(o.name, "EPOCH") == 0) continue;  // (a seam of a live shard, not a creation default)
    const std::string var = std::string("PSKV_") + o.name;
    const char* e = std::getenv(var.c_str());
    if (!e || !*e) continue;
    int64_t v = 0;
    bool ok = true;
    if (std::strcmp(o.name, "GENERAL") == 0 && std::isalpha((unsigned char)e[0]) != 0) {
      if (std::strcmp(e, "stamps") == 0)
        v = 0;
      else if (std::strcmp(e, "auto") == 0)
        v = 1;
      else if (std::strcmp(e, "radix") == 0)
        v = 2;
      else
        ok = false;
    } else {
      char* end = nullptr;
      errno = 0;
      v = std::strtoll(e, &end, 10);
      ok = end != e && *end == '\0' && errno == 0;
    }
    const std::string saved = g_last_error;
    if (ok && set_option(s, o, v) == PSKV_OK) continue;
    const std::string why = ok ? g_last_error : std::string("not a valid value");
    g_last_error = saved;
    std::lock_guard<std::mutex> g(warn_mu);
    if (std::find(warned.begin(), warned.end(), var) == warned.end()) {
      warned.push_back(var);
      std::fprintf(stderr, "pskv: ignoring environment %s=%s (%s); the option keeps its default\n", var.c_str(), e,
                   why.c_str());
    }
  }
  return PSKV_OK;
}

// Every setter ends here, its configuration widened to a pskv_optimizer_cfg
// (abi: which struct it came from; the shard keeps the widened form, size =
// sizeof(pskv_optimizer_cfg)).
int set_optimizer_impl(pskv_shard* s, pskv_optimizer_cfg cfg, OptAbi abi, const std::string& who) {
  // the configuration first: a bad field is reported whatever the handle
  if (const char* what = opt_config_error(cfg, abi)) return fail(PSKV_EINVAL, who + ": " + what);
  cfg.size = sizeof(pskv_optimizer_cfg);
  if (!s) return fail(PSKV_EINVAL, who + ": null shard");
  if (cfg.kind != PSKV_OPT_NONE && s->dtype != PSKV_F32 && s->dtype != PSKV_F64)
    return fail(PSKV_EINVAL, who + ": optimizers need a float shard (PSKV_F32, PSKV_F64)");
  int rc = use_device(s);
  if (rc) return rc;
  if (cfg.kind == s->opt.kind) {  // hyper-parameters only: they travel by value with each later launch
    s->opt = cfg;
    return PSKV_OK;
  }
  // a change of kind: allocate what the new kind needs before anything is
  // given up, so a failure leaves the shard as it was
  const size_t bytes = opt_array_bytes(s);
  const int slots = opt_slots(cfg.kind);
  // (gsum, state: the new arrays until they are swapped in, then the ones that go)
  DevBuf gsum, state[2];
  if (cfg.kind != PSKV_OPT_NONE) {
    if (!s->opt_gsum && !gsum.alloc(bytes)) return fail(PSKV_ENOMEM, who + ": gradient scratch allocation failed");
    for (int i = 0; i < slots; ++i)
      if (!state[i].alloc(bytes)) return fail(PSKV_ENOMEM, who + ": state allocation failed");
    if ((rc = ensure_owner(s))) return rc;
  }
  // queued steps may still use the arrays that go
  if (s->opt_slot[0] || (cfg.kind == PSKV_OPT_NONE && s->opt_gsum))
    if ((rc = srv_stop(s)) || (rc = wait_stream(s, s->stream, "shard stream (optimizer change)"))) return rc;
  if (gsum.p || cfg.kind == PSKV_OPT_NONE) gsum.swap_with(s->opt_gsum);  // (else the scratch it has stays)
  for (int i = 0; i < 2; ++i) state[i].swap_with(s->opt_slot[i]);
  s->opt = cfg;
  return opt_reset_state(s);
}

uint64_t opt_state_bytes(const pskv_shard* s) {
  if (s->opt.kind == PSKV_OPT_NONE) return 0;
  // the row arrays behind the parameters (gradient scratch, state slots) + the stamp array (8 bytes per key)
  uint64_t bytes = s->range * sizeof(unsigned long long);
  for (int a = 1; a < pskv_shard::kRowArrays; ++a)
    if (s->row_array(a).used) bytes += opt_array_bytes(s);
  return bytes;
}

// The state array of `slot`, or null with the error set.
void* opt_slot_array(pskv_shard* s, int slot, const char* who) {
  if (slot < 0 || slot >= opt_slots(s->opt.kind)) {
    (void)fail(PSKV_EINVAL, std::string(who) + ": the shard's optimizer has no state slot " + std::to_string(slot) +
                                " (slots: SGD 0, Adagrad 1, momentum 1, Adam 2, FTRL 2)");
    return nullptr;
  }
  return s->opt_slot[slot];
}

}  // namespace

extern "C" {

int pskv_abi_version(void) { return PSKV_ABI_VERSION; }

const char* pskv_last_error(void) { return g_last_error.c_str(); }

int pskv_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Every constructor ends here.  sparse: a sparse shard of key_end slots
// (pskv_shard_create_sparse validated its arguments; key_begin is 0).
static int create_impl(int device, uint32_t key_begin, uint64_t key_end, int dtype, int mode, uint32_t width,
                       uint64_t overflow_slots, bool sparse, pskv_shard** out) {
  if (!out) return fail(PSKV_EINVAL, "pskv_shard_create: out is null");
  *out = nullptr;
  const int vb = value_bytes(dtype);
  if (!vb) return fail(PSKV_EINVAL, "pskv_shard_create: bad dtype");
  if (mode != PSKV_ASSIGN && mode != PSKV_ACCUMULATE)
    return fail(PSKV_EINVAL, "pskv_shard_create: bad mode");
  if (key_end <= (uint64_t)key_begin || key_end > (1ull << 32))
    return fail(PSKV_EINVAL, "pskv_shard_create: need key_begin < key_end <= 2^32");
  if (width == 0 || width > PSKV_MAX_WIDTH)
    return fail(PSKV_EINVAL, "pskv_shard_create_rows: width must be 1.." + std::to_string(PSKV_MAX_WIDTH));
  if ((key_end - key_begin) * (uint64_t)width * (uint64_t)vb > (1ull << 46))
    return fail(PSKV_EINVAL, "pskv_shard_create_rows: keys * width * value bytes exceeds 2^46 bytes");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(PSKV_EINVAL, "pskv_shard_create: no such HIP device");
  pskv_shard* s = new pskv_shard();
  s->device = device;
  s->dtype = dtype;
  s->mode = mode;
  s->vb = vb;
  s->width = width;
  s->key_begin = key_begin;
  s->range = key_end - key_begin;
  s->sparse = sparse;
  // tuning / path options: creation defaults from the environment (PSKV_<NAME>),
  // changeable later through pskv_set_option (kOptions below)
  if (int rc = apply_env_options(s)) {
    delete s;
    return rc;
  }
  auto bail = [&](int rc) {
    pskv_shard_destroy(s);
    return rc;
  };
  int rc = use_device(s);
  if (rc) return bail(rc);
  // A blocking stream: it orders against the legacy default stream, on which
  // frameworks (torch) stage device inputs and read device outputs.
  if (hipStreamCreateWithFlags(&s->own_stream, hipStreamDefault) != hipSuccess)
    return bail(fail(PSKV_EHIP, "hipStreamCreate failed"));
  s->stream = s->own_stream;
  if (hipEventCreateWithFlags(&s->hstage_free, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->h2d_done, hipEventDisableTiming | hipEventDisableSystemFence) !=
          hipSuccess)
    return bail(fail(PSKV_EHIP, "hipEventCreate failed"));
  if (hipMalloc(&s->dense, s->rows_held() * (size_t)width * (size_t)vb) != hipSuccess)
    return bail(fail(PSKV_ENOMEM, "dense parameter allocation failed"));
  if (fill_rows(s, s->dense, 0, s->range, 0.0) != PSKV_OK) return bail(fail(PSKV_EHIP, "hipMemsetAsync failed"));
  // flag[0]: the sorted path's verification tag
  // the verification tag (16 bytes), then K1r's replay table (add_get's folded replay)
  if (hipMalloc(&s->flag, 64 + kK1rTableWords * sizeof(uint32_t)) != hipSuccess)
    return bail(fail(PSKV_ENOMEM, "flag allocation failed"));
  if (hipMemsetAsync(s->flag, 0, 16, s->stream) != hipSuccess)
    return bail(fail(PSKV_EHIP, "hipMemsetAsync failed"));
  // the overflow table: control block, growth mailbox, first array set
  s->ocap = next_pow2(std::max<uint64_t>(overflow_slots ? overflow_slots : kDefaultOverflowSlots, 64));
  OvfCtl* ctl = nullptr;
  if (hipMalloc(&ctl, sizeof(OvfCtl)) != hipSuccess) return bail(fail(PSKV_ENOMEM, "overflow control block allocation failed"));
  s->ovf.c = ctl;
  {
    void* p = nullptr;
    if (hipHostMalloc(&p, sizeof(OvfMbox), hipHostMallocCoherent) != hipSuccess)
      return bail(fail(PSKV_ENOMEM, "overflow growth mailbox allocation failed"));
    std::memset(p, 0, sizeof(OvfMbox));
    s->mbox = static_cast<OvfMbox*>(p);
  }
  if (hipDeviceGetAttribute(&s->wall_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess) s->wall_khz = 100000;
  refresh_grow_wait(s);
  rc = alloc_tab(s, s->ocap, &s->cur);
  if (rc) return bail(rc);
  OvfCtl init{};
  init.t = s->cur;
  init.mbox = s->mbox;
  if (hipMemcpyAsync(ctl, &init, sizeof(init), hipMemcpyHostToDevice, s->stream) != hipSuccess)
    return bail(fail(PSKV_EHIP, "hipMemcpyAsync failed"));
  if (sparse) {  // the index: an empty table and the key of every slot
    s->sp_table_slots = sparse_table_slots(s->range);
    if (hipMalloc(&s->sp_table, s->sp_table_slots * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&s->sp_slot_keys, s->range * sizeof(uint32_t)) != hipSuccess)
      return bail(fail(PSKV_ENOMEM, "sparse index allocation failed"));
    if (hipMemsetAsync(s->sp_table, 0, s->sp_table_slots * sizeof(unsigned long long), s->stream) != hipSuccess)
      return bail(fail(PSKV_EHIP, "hipMemsetAsync failed"));
  }
  if (int wrc = wait_stream(s, s->stream, "shard stream (creation)")) return bail(wrc);
  s->counted = g_queues.add_shard(device, 1);
  GrowService::get().add(s);
  *out = s;
  return PSKV_OK;
}

int pskv_shard_create_rows(int device, uint32_t key_begin, uint64_t key_end, int dtype, int mode,
                           uint32_t width, uint64_t overflow_slots, pskv_shard** out) {
  return create_impl(device, key_begin, key_end, dtype, mode, width, overflow_slots, /*sparse=*/false, out);
}

int pskv_shard_create_sparse(int device, uint64_t capacity, int dtype, int mode, uint32_t width, pskv_shard** out) {
  if (!out) return fail(PSKV_EINVAL, "pskv_shard_create_sparse: out is null");
  *out = nullptr;
  const int vb = value_bytes(dtype);
  if (!vb) return fail(PSKV_EINVAL, "pskv_shard_create_sparse: bad dtype");
  if (mode != PSKV_ASSIGN && mode != PSKV_ACCUMULATE) return fail(PSKV_EINVAL, "pskv_shard_create_sparse: bad mode");
  if (capacity == 0 || capacity > kSparseMaxCapacity)
    return fail(PSKV_EINVAL, "pskv_shard_create_sparse: capacity must be 1..2^31 - 2");
  if (width == 0 || width > PSKV_MAX_WIDTH)
    return fail(PSKV_EINVAL, "pskv_shard_create_sparse: width must be 1.." + std::to_string(PSKV_MAX_WIDTH));
  if ((capacity + 1) * (uint64_t)width * (uint64_t)vb > (1ull << 46))
    return fail(PSKV_EINVAL, "pskv_shard_create_sparse: (capacity + 1) * width * value bytes exceeds 2^46 bytes");
  // (the overflow table is never used: its smallest size)
  return create_impl(device, 0, capacity, dtype, mode, width, /*overflow_slots=*/64, /*sparse=*/true, out);
}

int pskv_sparse_info_get(pskv_shard* s, pskv_sparse_info* out) {
  if (!out) return fail(PSKV_EINVAL, "pskv_sparse_info_get: null output");
  if (out->size != sizeof(pskv_sparse_info))
    return fail(PSKV_EINVAL, "pskv_sparse_info_get: size must be sizeof(pskv_sparse_info)");
  if (!s) return fail(PSKV_EINVAL, "pskv_sparse_info_get: null shard");
  if (!s->sparse) return fail(PSKV_EINVAL, "pskv_sparse_info_get: not a sparse shard (pskv_shard_create_sparse)");
  int rc = use_device(s);
  if (rc) return rc;
  uint64_t count = 0;
  if ((rc = sparse_count(s, &count))) return rc;
  out->capacity = s->range;
  out->count = count;
  out->table_slots = s->sp_table_slots;
  out->index_bytes = s->sp_table_slots * sizeof(unsigned long long) + s->range * sizeof(uint32_t);
  return PSKV_OK;
}

int pskv_sparse_keys(pskv_shard* s, uint32_t* out, uint64_t cap, uint64_t* n, int flags) {
  if (flags & ~PSKV_DEVICE) return fail(PSKV_EINVAL, "pskv_sparse_keys: unknown flags (PSKV_HOST or PSKV_DEVICE)");
  if (!n) return fail(PSKV_EINVAL, "pskv_sparse_keys: null n");
  if (cap && !out) return fail(PSKV_EINVAL, "pskv_sparse_keys: null out with cap > 0");
  if (!s) return fail(PSKV_EINVAL, "pskv_sparse_keys: null shard");
  if (!s->sparse) return fail(PSKV_EINVAL, "pskv_sparse_keys: not a sparse shard (pskv_shard_create_sparse)");
  int rc = use_device(s);
  if (rc) return rc;
  uint64_t held = 0;
  if ((rc = sparse_count(s, &held))) return rc;  // (waits for the stream)
  *n = held;
  const uint64_t take = std::min(held, cap);
  if (take == 0) return PSKV_OK;
  PSKV_HIP(hipMemcpyAsync(out, s->sp_slot_keys, take * sizeof(uint32_t),
                          (flags & PSKV_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s->stream));
  return wait_stream(s, s->stream, "shard stream (sparse keys)");
}

// What is wrong with `capacity` as a sparse shard's new capacity or growth limit, or null.
static const char* sparse_capacity_refusal(const pskv_shard* s, uint64_t capacity) {
  if (!s->sparse) return "not a sparse shard (pskv_shard_create_sparse)";
  return sparse_capacity_error(s->range, capacity, (uint64_t)s->width * (uint64_t)s->vb);
}

int pskv_sparse_reserve(pskv_shard* s, uint64_t capacity) {
  if (capacity == 0 || capacity > kSparseMaxCapacity)
    return fail(PSKV_EINVAL, "pskv_sparse_reserve: capacity must be 1..2^31 - 2");
  if (!s) return fail(PSKV_EINVAL, "pskv_sparse_reserve: null shard");
  if (const char* why = sparse_capacity_refusal(s, capacity))
    return fail(PSKV_EINVAL, std::string("pskv_sparse_reserve: ") + why);
  if (capacity == s->range) return PSKV_OK;
  int rc = use_device(s);
  if (rc) return rc;
  if ((rc = sparse_rebuild(s, capacity, nullptr))) return rc;
  if (s->sp_max_capacity && s->sp_max_capacity < capacity) s->sp_max_capacity = capacity;  // (never below the capacity)
  return PSKV_OK;
}

int pskv_sparse_set_growth(pskv_shard* s, uint64_t max_capacity) {
  if (max_capacity > kSparseMaxCapacity)
    return fail(PSKV_EINVAL, "pskv_sparse_set_growth: max_capacity must be 0 (fixed) or at most 2^31 - 2");
  if (!s) return fail(PSKV_EINVAL, "pskv_sparse_set_growth: null shard");
  if (const char* why = sparse_capacity_refusal(s, max_capacity ? max_capacity : s->range))
    return fail(PSKV_EINVAL, std::string("pskv_sparse_set_growth: max_capacity: ") + why);
  s->sp_max_capacity = max_capacity;
  s->sp_bound = s->range;  // (no read-back yet: the first call that could grow makes one)
  return PSKV_OK;
}

int pskv_sparse_get_growth(pskv_shard* s, uint64_t* max_capacity, uint64_t* rebuilds) {
  if (!s) return fail(PSKV_EINVAL, "pskv_sparse_get_growth: null shard");
  if (!s->sparse) return fail(PSKV_EINVAL, "pskv_sparse_get_growth: not a sparse shard (pskv_shard_create_sparse)");
  if (max_capacity) *max_capacity = s->sp_max_capacity;
  if (rebuilds) *rebuilds = s->sp_rebuilds;
  return PSKV_OK;
}

int pskv_sparse_erase(pskv_shard* s, const uint32_t* keys, uint64_t n, int flags) {
  if (flags & ~PSKV_DEVICE) return fail(PSKV_EINVAL, "pskv_sparse_erase: unknown flags (PSKV_HOST or PSKV_DEVICE)");
  if (n && !keys) return fail(PSKV_EINVAL, "pskv_sparse_erase: null keys with n > 0");
  if (!s) return fail(PSKV_EINVAL, "pskv_sparse_erase: null shard");
  if (!s->sparse) return fail(PSKV_EINVAL, "pskv_sparse_erase: not a sparse shard (pskv_shard_create_sparse)");
  if (n == 0) return PSKV_OK;
  int rc = use_device(s);
  if (rc) return rc;
  // the list's slot ids (the reading translate: an absent key carries
  // `capacity`), then one flag per id; the rebuild leaves the flagged slots out
  DevBuf ids, dead;
  if (!ids.alloc(n * sizeof(uint32_t)) || !dead.alloc(s->range + 1)) {
    (void)hipGetLastError();
    return fail(PSKV_ENOMEM, "pskv_sparse_erase: scratch allocation failed (the shard is unchanged)");
  }
  uint32_t* idp = static_cast<uint32_t*>(ids.p);
  const uint32_t* from = keys;
  if (!(flags & PSKV_DEVICE)) {  // host keys: into the scratch, translated in place
    PSKV_HIP(hipMemcpyAsync(idp, keys, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    from = idp;
  }
  PSKV_HIP(hipMemsetAsync(dead.p, 0, s->range + 1, s->stream));
  std::vector<pskv_batch> io;
  push_pieces(io, pskv_batch{from, idp, n}, sizeof(uint32_t));
  const SparseIndex x = s->sindex();
  for (const Span& sp : split_groups(io)) {
    const LaunchGroup g = make_group(io, sp.first, sp.second, kGeneralChunk);
    PSKV_HIP(launch_index_translate(/*writing=*/false, g.ga, g.nwg, x, s->stream));
  }
  PSKV_HIP(launch_index_mark_dead(idp, n, (uint32_t)s->range, static_cast<uint8_t*>(dead.p), s->stream));
  return sparse_rebuild(s, s->range, static_cast<const uint8_t*>(dead.p));
}

// The counters of one timed operation (kTimeApply, kTimePooled, kTimeIndex).
static int timed_op_read(pskv_shard* s, const char* who, int slot, uint64_t* launches, double* total_ms,
                         uint64_t* elements) {
  if (!s) return fail(PSKV_EINVAL, std::string(who) + ": null shard");
  int rc = use_device(s);
  if (rc || (rc = drain_timing(s))) return rc;
  if (launches) *launches = s->t_launches[slot];
  if (total_ms) *total_ms = s->t_ms[slot];
  if (elements) *elements = s->t_elems[slot];
  return PSKV_OK;
}

int pskv_index_time(pskv_shard* s, uint64_t* launches, double* total_ms, uint64_t* elements) {
  return timed_op_read(s, "pskv_index_time", kTimeIndex, launches, total_ms, elements);
}

int pskv_shard_create_ex(int device, uint32_t key_begin, uint64_t key_end, int dtype, int mode,
                         uint64_t overflow_slots, pskv_shard** out) {
  return pskv_shard_create_rows(device, key_begin, key_end, dtype, mode, 1, overflow_slots, out);
}

uint32_t pskv_shard_width(pskv_shard* s) { return s ? s->width : 0u; }

int pskv_shard_create(int device, uint32_t key_begin, uint64_t key_end, int dtype, int mode,
                      pskv_shard** out) {
  return pskv_shard_create_ex(device, key_begin, key_end, dtype, mode, 0, out);
}

int pskv_shard_destroy(pskv_shard* s) {
  if (!s) return PSKV_OK;
  (void)hipSetDevice(s->device);
  // (the grow service keeps answering while the streams drain: a growing
  // workgroup may be waiting for it)
  // every wait is bounded (PSKV_SYNC_TIMEOUT_MS): work that never completes
  // keeps its device memory, streams and shard object (leaked, never freed
  // under a running kernel), and the call reports what it waited for
  std::string stuck;
  auto drain = [&](hipStream_t st, const char* what) {
    if (wait_stream(s, st, what) != PSKV_OK) stuck += (stuck.empty() ? "" : "; ") + g_last_error;
  };
  if (s->srv) {
    (void)srv_stop(s);
    if (s->srv_running) {  // srv_stop failed: make the kernel leave anyway
      __atomic_store_n(&s->srv->stop, 1u, __ATOMIC_RELEASE);
      drain(s->srv_stream, "request-server stream (destroy)");
    }
  }
  if (s->out_stream) drain(s->out_stream, "D2H output stream (destroy)");
  if (s->own_stream) drain(s->own_stream, "shard stream (destroy)");
  if (s->stream && s->stream != s->own_stream) drain(s->stream, "caller stream (destroy)");
  if (!stuck.empty()) {
    // the leaked streams keep their hardware queues: they stay counted in
    // g_queues (pskv_queues.h), so later shards on this device do not plan
    // with queues that are still held.  The shard object itself is leaked
    // too: the grow service keeps answering its mailbox (stuck work may be a
    // workgroup waiting for it) and the service holds the pointer.
    std::fprintf(stderr, "pskv: shard destroy: %s; its device memory and streams are not freed\n", stuck.c_str());
    return fail(PSKV_ESTATE, "pskv_shard_destroy: " + stuck);
  }
  GrowService::get().remove(s);
  if (s->counted) g_queues.add_shard(s->device, -1);
  if (s->out_stream) g_queues.add_stream(s->device, -1);
  if (s->srv) (void)hipHostFree(s->srv);
  if (s->srv_stream) (void)hipStreamDestroy(s->srv_stream);
  if (s->srv_dep) (void)hipEventDestroy(s->srv_dep);
  if (s->out_stream) (void)hipStreamDestroy(s->out_stream);
  for (auto e : s->out_events) (void)hipEventDestroy(e);
  for (auto& t : s->pending) {
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  for (auto e : s->event_pool) (void)hipEventDestroy(e);
  if (s->sync_ev) (void)hipEventDestroy(s->sync_ev);
  for (int a = 0; a < pskv_shard::kRowArrays; ++a)
    if (void* p = *s->row_array(a).p) (void)hipFree(p);
  if (s->owner) (void)hipFree(s->owner);
  if (s->flag) (void)hipFree(s->flag);
  for (const auto& t : s->tables) {  // (the service no longer touches the list)
    (void)hipFree(t.keys);
    (void)hipFree(t.vals);
  }
  if (s->ovf.c) (void)hipFree(s->ovf.c);
  if (s->mbox) (void)hipHostFree(s->mbox);
  if (s->dstage) (void)hipFree(s->dstage);
  if (s->rb_loff) (void)hipFree(s->rb_loff);
  if (s->rb_ent) (void)hipFree(s->rb_ent);
  if (s->pool_part) (void)hipFree(s->pool_part);
  if (s->sp_table) (void)hipFree(s->sp_table);
  if (s->sp_slot_keys) (void)hipFree(s->sp_slot_keys);
  if (s->sp_ids) (void)hipFree(s->sp_ids);
  if (s->hstage) (void)hipHostFree(s->hstage);
  if (s->ireply) (void)hipHostFree(s->ireply);
  if (s->stat_host) (void)hipHostFree(s->stat_host);
  if (s->hstage_free) (void)hipEventDestroy(s->hstage_free);
  if (s->h2d_done) (void)hipEventDestroy(s->h2d_done);
  for (auto e : s->win_events) (void)hipEventDestroy(e);
  if (s->own_stream) (void)hipStreamDestroy(s->own_stream);
  delete s;
  return PSKV_OK;
}

// Flag bits a call accepts (pskv.h): a mistyped or foreign flag fails the call
// instead of silently selecting the host path.
static bool bad_flags(int flags) {
  return (flags & ~(PSKV_DEVICE | PSKV_SORTED_HINT | PSKV_HOST_FRAME)) != 0 ||
         ((flags & PSKV_DEVICE) && (flags & PSKV_HOST_FRAME));
}

int pskv_add(pskv_shard* s, const uint32_t* keys, const void* vals, uint64_t n, int flags) {
  if (!s) return fail(PSKV_EINVAL, "pskv_add: null shard");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_add: unknown flags");
  pskv_batch b{keys, const_cast<void*>(vals), n};
  return add_impl(s, std::vector<pskv_batch>{b}, flags);
}

int pskv_get(pskv_shard* s, const uint32_t* keys, uint64_t n, void* out, int flags) {
  if (!s) return fail(PSKV_EINVAL, "pskv_get: null shard");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_get: unknown flags");
  pskv_batch b{keys, out, n};
  return get_impl(s, std::vector<pskv_batch>{b}, flags);
}

int pskv_add_grouped(pskv_shard* s, const pskv_batch* batches, uint64_t nb, int flags) {
  if (!s) return fail(PSKV_EINVAL, "pskv_add_grouped: null shard");
  if (nb && !batches) return fail(PSKV_EINVAL, "pskv_add_grouped: null batches");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_add_grouped: unknown flags");
  return add_impl(s, std::vector<pskv_batch>(batches, batches + nb), flags);
}

int pskv_add_get_grouped(pskv_shard* s, const pskv_batch* adds, uint64_t na, const pskv_batch* gets, uint64_t ng,
                         int flags) {
  if (!s) return fail(PSKV_EINVAL, "pskv_add_get_grouped: null shard");
  if ((na && !adds) || (ng && !gets)) return fail(PSKV_EINVAL, "pskv_add_get_grouped: null batches");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_add_get_grouped: unknown flags");
  return add_get_impl(s, std::vector<pskv_batch>(adds, adds + na), std::vector<pskv_batch>(gets, gets + ng), flags);
}

int pskv_get_grouped(pskv_shard* s, const pskv_batch* batches, uint64_t nb, int flags) {
  if (!s) return fail(PSKV_EINVAL, "pskv_get_grouped: null shard");
  if (nb && !batches) return fail(PSKV_EINVAL, "pskv_get_grouped: null batches");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_get_grouped: unknown flags");
  return get_impl(s, std::vector<pskv_batch>(batches, batches + nb), flags);
}

// Flags, pointers and a host call's offsets are checked before the handle is
// looked at (as pskv_shard_set_optimizer checks its configuration).
int pskv_get_pooled(pskv_shard* s, const uint32_t* keys, uint64_t n, const void* weights, const uint64_t* offsets,
                    uint64_t nbags, void* out, int flags) {
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_get_pooled: unknown flags");
  if (n && !keys) return fail(PSKV_EINVAL, "pskv_get_pooled: null keys with n > 0");
  if (nbags && !offsets) return fail(PSKV_EINVAL, "pskv_get_pooled: null offsets with nbags > 0");
  if (nbags && !out) return fail(PSKV_EINVAL, "pskv_get_pooled: null out with nbags > 0");
  if (!(flags & PSKV_DEVICE)) {
    uint64_t bad = 0;
    if (const char* why = pool_offsets_error(offsets, nbags, n, &bad))
      return fail(PSKV_EINVAL, "pskv_get_pooled: offsets: bag " + std::to_string(bad) + ": " + why + " (n = " +
                                   std::to_string(n) + ", nbags = " + std::to_string(nbags) + ")");
  }
  if (!s) return fail(PSKV_EINVAL, "pskv_get_pooled: null shard");
  return pooled_impl(s, pskv_pool_batch{keys, weights, offsets, out, n, nbags}, flags);
}

int pskv_shard_set_optimizer(pskv_shard* s, const pskv_optimizer* cfg) {
  if (!cfg) return fail(PSKV_EINVAL, "pskv_shard_set_optimizer: null configuration");
  pskv_optimizer_cfg x{};
  x.kind = cfg->kind;
  x.lr = cfg->lr;
  x.weight_decay = cfg->weight_decay;
  x.eps = cfg->eps;
  x.init_accum = cfg->init_accum;
  return set_optimizer_impl(s, x, kOptLegacy, "pskv_shard_set_optimizer");
}

int pskv_shard_set_optimizer_ex(pskv_shard* s, const pskv_optimizer_ex* cfg) {
  if (!cfg) return fail(PSKV_EINVAL, "pskv_shard_set_optimizer_ex: null configuration");
  pskv_optimizer_cfg x{};
  std::memcpy(&x, cfg, sizeof(pskv_optimizer_ex));  // (the common prefix, size included)
  return set_optimizer_impl(s, x, kOptEx, "pskv_shard_set_optimizer_ex");
}

int pskv_shard_set_optimizer_cfg(pskv_shard* s, const pskv_optimizer_cfg* cfg) {
  if (!cfg) return fail(PSKV_EINVAL, "pskv_shard_set_optimizer_cfg: null configuration");
  return set_optimizer_impl(s, *cfg, kOptCfg, "pskv_shard_set_optimizer_cfg");
}

int pskv_shard_get_optimizer(pskv_shard* s, pskv_optimizer* out, uint64_t* state_bytes) {
  if (!s) return fail(PSKV_EINVAL, "pskv_shard_get_optimizer: null shard");
  if (out) {
    out->kind = s->opt.kind;
    out->lr = s->opt.lr;
    out->weight_decay = s->opt.weight_decay;
    out->eps = s->opt.eps;
    out->init_accum = s->opt.init_accum;
  }
  if (state_bytes) *state_bytes = opt_state_bytes(s);
  return PSKV_OK;
}

int pskv_shard_get_optimizer_ex(pskv_shard* s, pskv_optimizer_ex* out, uint64_t* state_bytes) {
  if (!s) return fail(PSKV_EINVAL, "pskv_shard_get_optimizer_ex: null shard");
  if (out) {
    std::memcpy(out, &s->opt, sizeof(pskv_optimizer_ex));  // (the common prefix)
    out->size = sizeof(pskv_optimizer_ex);
  }
  if (state_bytes) *state_bytes = opt_state_bytes(s);
  return PSKV_OK;
}

int pskv_shard_get_optimizer_cfg(pskv_shard* s, pskv_optimizer_cfg* out, uint64_t* state_bytes) {
  if (!s) return fail(PSKV_EINVAL, "pskv_shard_get_optimizer_cfg: null shard");
  if (out) {
    *out = s->opt;
    out->size = sizeof(pskv_optimizer_cfg);
  }
  if (state_bytes) *state_bytes = opt_state_bytes(s);
  return PSKV_OK;
}

int pskv_get_step(pskv_shard* s, uint64_t* t) {
  if (!s) return fail(PSKV_EINVAL, "pskv_get_step: null shard");
  if (!t) return fail(PSKV_EINVAL, "pskv_get_step: null output");
  *t = s->opt_step;
  return PSKV_OK;
}

int pskv_set_step(pskv_shard* s, uint64_t t) {
  if (!s) return fail(PSKV_EINVAL, "pskv_set_step: null shard");
  s->opt_step = t;
  return PSKV_OK;
}

int pskv_apply(pskv_shard* s, const uint32_t* keys, const void* grads, uint64_t n, int flags) {
  if (!s) return fail(PSKV_EINVAL, "pskv_apply: null shard");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_apply: unknown flags");
  pskv_batch b{keys, const_cast<void*>(grads), n};
  return apply_impl(s, std::vector<pskv_batch>{b}, flags);
}

int pskv_apply_grouped(pskv_shard* s, const pskv_batch* batches, uint64_t nb, int flags) {
  if (!s) return fail(PSKV_EINVAL, "pskv_apply_grouped: null shard");
  if (nb && !batches) return fail(PSKV_EINVAL, "pskv_apply_grouped: null batches");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_apply_grouped: unknown flags");
  return apply_impl(s, std::vector<pskv_batch>(batches, batches + nb), flags);
}

// What is wrong with a pooled push's batch, or "": pointers, the size limit
// (`one`: what a batch of at most 2^31 keys is to the call) and a host call's
// offsets, in that order.  who: the call, and in a grouped one the batch.
static std::string pool_batch_error(const std::string& who, const pskv_pool_batch& b, int flags, const char* one) {
  if (b.n && !b.keys) return who + "null keys with n > 0";
  if (b.nbags && !b.offsets) return who + "null offsets with nbags > 0";
  if (b.nbags && !b.bag_grads) return who + "null bag_grads with nbags > 0";
  if (b.n > kMaxPiece) return who + "n = " + std::to_string(b.n) + " exceeds 2^31 keys (" + one + ")";
  if (!(flags & PSKV_DEVICE)) {
    uint64_t bad = 0;
    if (const char* why = pool_offsets_error(b.offsets, b.nbags, b.n, &bad))
      return who + "offsets: bag " + std::to_string(bad) + ": " + why + " (n = " + std::to_string(b.n) +
             ", nbags = " + std::to_string(b.nbags) + ")";
  }
  return "";
}

// Flags and the batch (pool_batch_error) are checked before the handle is
// looked at, as pskv_get_pooled checks its arguments.
int pskv_apply_pooled(pskv_shard* s, const uint32_t* keys, uint64_t n, const void* weights, const uint64_t* offsets,
                      uint64_t nbags, const void* bag_grads, int flags) {
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_apply_pooled: unknown flags");
  const pskv_pool_batch b{keys, weights, offsets, bag_grads, n, nbags};
  const std::string err = pool_batch_error("pskv_apply_pooled: ", b, flags, "a pooled push is one launch group");
  if (!err.empty()) return fail(PSKV_EINVAL, err);
  if (!s) return fail(PSKV_EINVAL, "pskv_apply_pooled: null shard");
  return apply_pooled_impl(s, b, flags);
}

// Every batch gets pskv_apply_pooled's checks, before the handle is looked at;
// a failure names the batch.
int pskv_apply_pooled_grouped(pskv_shard* s, const pskv_pool_batch* batches, uint64_t nb, int flags) {
  if (bad_flags(flags)) return fail(PSKV_EINVAL, "pskv_apply_pooled_grouped: unknown flags");
  if (nb && !batches) return fail(PSKV_EINVAL, "pskv_apply_pooled_grouped: null batches with nb > 0");
  for (uint64_t i = 0; i < nb; ++i) {
    const std::string err = pool_batch_error("pskv_apply_pooled_grouped: batch " + std::to_string(i) + ": ", batches[i],
                                             flags, "a batch lies in one launch group");
    if (!err.empty()) return fail(PSKV_EINVAL, err);
  }
  if (!s) return fail(PSKV_EINVAL, "pskv_apply_pooled_grouped: null shard");
  return apply_pooled_grouped_impl(s, batches, nb, flags);
}

// The three state entry points: a row Get from, or (put) a row assign Add
// to, the array of `slot`.  adagrad_only: pskv_get_state's guard.
static int state_call(pskv_shard* s, const std::string& who, bool adagrad_only, int slot, const uint32_t* keys,
                      void* vals, uint64_t n, int flags, bool put) {
  if (!s) return fail(PSKV_EINVAL, who + ": null shard");
  if (bad_flags(flags)) return fail(PSKV_EINVAL, who + ": unknown flags");
  if (adagrad_only && (s->opt.kind != PSKV_OPT_ADAGRAD || !s->opt_slot[0]))
    return fail(PSKV_EINVAL, who + ": the shard's optimizer is not PSKV_OPT_ADAGRAD (the other kinds' state: "
                                   "pskv_get_state_slot)");
  void* arr = opt_slot_array(s, slot, who.c_str());
  if (!arr) return PSKV_EINVAL;
  int rc = use_device(s);
  if (rc) return rc;
  rc = srv_stop(s);
  if (rc) return rc;
  const std::vector<pskv_batch> in{pskv_batch{keys, vals, n}};
  if (!put) return rows_get_from(s, in, flags, s->read_view(arr), who.c_str(), nullptr);
  return rows_add_to(s, in, flags, slot, PSKV_ASSIGN,
                     RowFront{who.c_str(), nullptr, false, "key",
                              "optimizer state is kept for the shard's own keys only", /*with_values=*/true});
}

int pskv_get_state(pskv_shard* s, const uint32_t* keys, uint64_t n, void* out, int flags) {
  return state_call(s, "pskv_get_state", /*adagrad_only=*/true, 0, keys, out, n, flags, /*put=*/false);
}

int pskv_get_state_slot(pskv_shard* s, int slot, const uint32_t* keys, uint64_t n, void* out, int flags) {
  return state_call(s, "pskv_get_state_slot", false, slot, keys, out, n, flags, /*put=*/false);
}

int pskv_put_state(pskv_shard* s, int slot, const uint32_t* keys, const void* vals, uint64_t n, int flags) {
  return state_call(s, "pskv_put_state", false, slot, keys, const_cast<void*>(vals), n, flags, /*put=*/true);
}

int pskv_apply_time(pskv_shard* s, uint64_t* launches, double* total_ms, uint64_t* elements) {
  return timed_op_read(s, "pskv_apply_time", kTimeApply, launches, total_ms, elements);
}

int pskv_pooled_time(pskv_shard* s, uint64_t* launches, double* total_ms, uint64_t* elements) {
  return timed_op_read(s, "pskv_pooled_time", kTimePooled, launches, total_ms, elements);
}

int pskv_sync(pskv_shard* s) {
  if (!s) return fail(PSKV_EINVAL, "pskv_sync: null shard");
  int rc = use_device(s);
  if (rc) return rc;
  uint32_t cnt = 0, err = 0;
  rc = read_overflow_stat(s, &cnt, &err);
  if (rc) return rc;
  rc = drain_timing(s);
  if (rc) return rc;
  if (s->sparse) {  // (stat[0] is the slot counter; a dropped key is a key that found no slot)
    if (err & (kErrSparseFull | kErrRowOutOfRange))
      return fail(PSKV_ESTATE, "sparse shard full: a writing call met new keys with all " + std::to_string(s->range) +
                                   " slots taken; those keys were dropped whole, the rest of the call was applied "
                                   "(pskv_sparse_reserve, pskv_sparse_erase or pskv_clear resets this)");
    return PSKV_OK;
  }
  if (err & kErrOverflowFull)
    return fail(PSKV_ESTATE,
                "overflow table exhausted: out-of-range keys were dropped (the device-side growth "
                "request was not answered within SYNC_TIMEOUT_MS, or its allocation failed)");
  if (err & kErrRowOutOfRange)
    return fail(PSKV_ESTATE,
                "row shard: a device Add, optimizer step or pooled pull held out-of-range keys; their rows were dropped "
                "(a pooled pull read them as zeros) (a row shard, and an optimizer step or a pooled pull at any "
                "width, holds no key outside [key_begin, key_end); pskv_clear resets this)");
  if (2 * (uint64_t)cnt > s->ocap) return grow_overflow(s, cnt);
  return PSKV_OK;
}

int pskv_clear(pskv_shard* s) {
  if (!s) return fail(PSKV_EINVAL, "pskv_clear: null shard");
  int rc = use_device(s);
  if (rc) return rc;
  uint32_t cnt = 0, err = 0;
  rc = read_overflow_stat(s, &cnt, &err);  // (adopts the current table; stops the server)
  if (rc) return rc;
  if ((rc = fill_rows(s, s->dense, 0, s->range, 0.0))) return rc;
  // a sparse shard: an empty index (the slot counter and the full bit go with stat below)
  if (s->sparse) PSKV_HIP(hipMemsetAsync(s->sp_table, 0, s->sp_table_slots * sizeof(unsigned long long), s->stream));
  PSKV_HIP(hipMemsetAsync(s->cur.keys, 0xFF, s->ocap * sizeof(unsigned long long), s->stream));
  PSKV_HIP(hipMemsetAsync(s->cur.vals, 0, s->ocap * (size_t)s->vb, s->stream));
  PSKV_HIP(hipMemsetAsync(s->ovf.c->stat, 0, 2 * sizeof(uint32_t), s->stream));
  if (int rc2 = opt_reset_state(s)) return rc2;
  s->ocount_known = 0;
  if (int rc2 = wait_stream(s, s->stream, "shard stream (clear)")) return rc2;
  return PSKV_OK;
}

int pskv_set_stream(pskv_shard* s, void* hip_stream) {
  if (!s) return fail(PSKV_EINVAL, "pskv_set_stream: null shard");
  int rc = use_device(s);
  if (rc) return rc;
  rc = srv_stop(s);
  if (rc) return rc;
  // order the switch: everything queued so far completes before the new stream's work
  if (int rc2 = wait_stream(s, s->stream, "shard stream (stream switch)")) return rc2;
  s->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->own_stream;
  return PSKV_OK;
}

void* pskv_get_stream(pskv_shard* s) { return s ? static_cast<void*>(s->stream) : nullptr; }

void* pskv_dense_ptr(pskv_shard* s) { return s ? s->dense : nullptr; }

int pskv_shard_info(pskv_shard* s, pskv_info* info) {
  if (!s || !info) return fail(PSKV_EINVAL, "pskv_shard_info: null argument");
  info->device = s->device;
  info->dtype = s->dtype;
  info->mode = s->mode;
  info->value_bytes = s->vb;
  info->key_begin = s->key_begin;
  info->key_end = s->sparse ? (1ull << 32) : (uint64_t)s->key_begin + s->range;  // (a sparse shard owns every key)
  info->dense_bytes = s->rows_held() * (uint64_t)s->width * (uint64_t)s->vb;
  info->overflow_capacity = s->ocap;
  info->overflow_count = s->sparse ? 0 : s->ocount_known;  // (its stat[0] counts slots, not overflow keys)
  info->n_add_calls = s->n_add;
  info->n_get_calls = s->n_get;
  info->n_sorted_launches = s->n_sorted;
  info->n_general_launches = s->n_general;
  info->resident_bytes = s->resident_bytes();
  return PSKV_OK;
}

int pskv_set_timing(pskv_shard* s, int enable) {
  if (!s) return fail(PSKV_EINVAL, "pskv_set_timing: null shard");
  s->timing_mask = enable ? (1u << kTimeSlots) - 1 : 0u;
  return PSKV_OK;
}

int pskv_set_timing_mask(pskv_shard* s, uint32_t kernel_mask) {
  if (!s) return fail(PSKV_EINVAL, "pskv_set_timing_mask: null shard");
  s->timing_mask = kernel_mask & ((1u << kTimeSlots) - 1);
  return PSKV_OK;
}

int pskv_kernel_time(pskv_shard* s, int kernel, uint64_t* launches, double* total_ms,
                     uint64_t* elements) {
  if (!s || kernel < 0 || kernel >= PSKV_K_COUNT)
    return fail(PSKV_EINVAL, "pskv_kernel_time: bad argument");
  int rc = use_device(s);
  if (rc) return rc;
  rc = drain_timing(s);
  if (rc) return rc;
  if (launches) *launches = s->t_launches[kernel];
  if (total_ms) *total_ms = s->t_ms[kernel];
  if (elements) *elements = s->t_elems[kernel];
  return PSKV_OK;
}

int pskv_reset_timing(pskv_shard* s) {
  if (!s) return fail(PSKV_EINVAL, "pskv_reset_timing: null shard");
  int rc = use_device(s);
  if (rc) return rc;
  rc = drain_timing(s);
  if (rc) return rc;
  for (int k = 0; k < kTimeSlots; ++k) {
    s->t_launches[k] = 0;
    s->t_ms[k] = 0;
    s->t_elems[k] = 0;
  }
  return PSKV_OK;
}

int pskv_set_option(pskv_shard* s, const char* name, int64_t value) {
  if (!s || !name) return fail(PSKV_EINVAL, "pskv_set_option: null argument");
  const Option* o = find_option(name);
  if (!o) return fail(PSKV_EINVAL, std::string("pskv_set_option: unknown option ") + name);
  int rc = use_device(s);
  if (rc) return rc;
  // the request server runs with the options it was launched with: drain and
  // stop it first (it restarts on the next small message if still enabled)
  rc = srv_stop(s);
  if (rc) return rc;
  return set_option(s, *o, value);
}

int pskv_get_option(pskv_shard* s, const char* name, int64_t* value) {
  if (!s || !name || !value) return fail(PSKV_EINVAL, "pskv_get_option: null argument");
  const Option* o = find_option(name);
  if (!o) return fail(PSKV_EINVAL, std::string("pskv_get_option: unknown option ") + name);
  *value = o->get(s);
  return PSKV_OK;
}

int pskv_range_slice(const uint64_t* range_begin, const uint64_t* range_end, int nranges,
                     const uint32_t* keys, uint64_t n, int32_t* slice_range,
                     uint64_t* slice_start, uint64_t* slice_len) {
  // Restates RangePartitionManager::Slice (base/range_partition_manager.hpp:19-46):
  // the range pointer only moves forward; a key stays with the current range if
  // it lies in it or the current range is the last one.
  if (n == 0) return 0;
  if (nranges <= 0 || !range_begin || !range_end || !keys || !slice_range || !slice_start ||
      !slice_len)
    return fail(PSKV_EINVAL, "pskv_range_slice: bad argument");
  int r = 0, cur = -1, ns = 0;
  for (uint64_t i = 0; i < n;) {
    const uint64_t k = keys[i];
    if ((k >= range_begin[r] && k < range_end[r]) || r + 1 >= nranges) {
      if (cur < r) {
        cur = r;
        slice_range[ns] = r;
        slice_start[ns] = i;
        slice_len[ns] = 0;
        ++ns;
      }
      slice_len[ns - 1]++;
      ++i;
    } else {
      ++r;
    }
  }
  return ns;
}

int pskv_jump_hash(const uint32_t* keys, uint64_t n, int32_t nbuckets, int32_t* out_bucket) {
  // Jump consistent hash (Lamping & Veach, "A Fast, Minimal Memory, Consistent
  // Hash Algorithm", 2014), the bucket function of the reference's default
  // partitioner ConsistentHashingPartitionManager::JumpConsistentHash
  // (base/consistent_hashing_partition_manager.hpp:81-89): a 64-bit LCG step
  // per jump, the next candidate bucket (b + 1) * 2^31 / ((state >> 33) + 1)
  // in double precision; the key enters zero-extended to 64 bits.
  if (n == 0) return PSKV_OK;
  if (nbuckets <= 0 || !keys || !out_bucket) return fail(PSKV_EINVAL, "pskv_jump_hash: bad argument");
  auto hash_range = [&](uint64_t b, uint64_t e) {
    for (uint64_t i = b; i < e; ++i) {
      uint64_t key = keys[i];
      int64_t bk = -1, j = 0;
      while (j < nbuckets) {
        bk = j;
        key = key * 2862933555777941757ULL + 1;
        j = (int64_t)((double)(bk + 1) * (double(1LL << 31) / double((key >> 33) + 1)));
      }
      out_bucket[i] = (int32_t)bk;
    }
  };
  constexpr uint64_t kPiece = 1 << 18;
  if (n <= kPiece) {
    hash_range(0, n);
  } else {
    HostPool::get().run((size_t)((n + kPiece - 1) / kPiece), [&](size_t t) {
      hash_range(t * kPiece, std::min<uint64_t>(n, (t + 1) * kPiece));
    });
  }
  return PSKV_OK;
}

int pskv_host_alloc(uint64_t bytes, void** out) {
  std::string err;
  const int rc = frames::alloc((size_t)bytes, out, &err);
  return rc ? fail(rc, err) : PSKV_OK;
}

int pskv_host_free(void* p) {
  std::string err;
  const int rc = frames::release(p, &err);
  return rc ? fail(rc, err) : PSKV_OK;
}

int pskv_host_pool_stats(uint64_t* live_bytes, uint64_t* cached_bytes, uint64_t* held_bytes) {
  frames::stats(live_bytes, cached_bytes, held_bytes);
  return PSKV_OK;
}

int pskv_host_pool_trim(void) {
  std::string err;
  const int rc = frames::trim(&err);
  return rc ? fail(rc, err) : PSKV_OK;
}

}  // extern "C"
