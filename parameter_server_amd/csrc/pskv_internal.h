// pskv_internal.h — device-side data layout and kernel launch wrappers shared by
// pskv_kernels.hip, pskv_rows.hip (device code) and pskv_shard.cpp (the C ABI
// host logic).  The host planner -- pieces, launch groups, staging layout, DMA
// windows, the key check and K5's bucket rule (RbMap), with the limits they
// share with the kernels (kMaxBatches, kRbMaxBuckets) -- is pskv_plan.h,
// included here.
//
// HBM layout of one shard (DESIGN.md "Data layout in HBM"):
//   dense[range]        value array, one slot per owned key, zero-initialised
//   owner[range]        u64 last-writer stamps (epoch<<32 | group index), general path only
//   ctl                 OvfCtl: the overflow table's current arrays, {occupied
//                       slots, sticky error bits}, the growth mailbox
//   keys[cap]           u64 overflow hash keys, EMPTY = ~0
//   vals[cap]           overflow values
//   gsum, state slots   with an optimizer: gradient scratch and up to
//                       two state arrays (Adagrad's h; momentum's v; Adam's m and v),
//                       each shaped as dense
//   A sparse shard: dense, gsum and the state slots hold capacity + 1
//   rows (slots, then the zero row absent keys read), owner[capacity], and the index:
//   table[table_slots] u64 entries and slot_keys[capacity] (SparseIndex below).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pskv_plan.h"

namespace pskv {

constexpr int kBlock = 256;         // threads per workgroup (4 waves)
constexpr int kGatherVec = 4;       // keys per lane per step (16 B loads)
constexpr int kSortedUnroll = 2;
inline int stream_chunk(int unroll) { return kBlock * 4 * unroll; }  // keys per gather / dense chunk
constexpr int kSortedChunk = kBlock * 4 * kSortedUnroll;          // 2048 keys / workgroup
constexpr int kGeneralChunk = 2048;  // keys per workgroup in the dedup path
constexpr int kGeneralSlots = 4096;  // LDS hash slots (load factor <= 1/2)
// K5a workgroup (option RB_BIN_BLOCK): 1024 threads, one per CU.  Two
// 512-thread workgroups per CU on 4 Ki-key super-chunks bin at the same rate
// (K5a 55.0 against 56.0 us per 8 M cfg-3 Zipf keys): K5a is bound by the CU's
// LDS and issue throughput, not by its barrier phases.  With one run per
// resolve thread the 512 form needs two launch pieces per 8 M keys, and the
// whole Add is slower (assign 2 x (32.0 + 58.7) against 56.8 + 86.4 us;
// profiles/r03_probes/ztrace_k5_split_*.txt).
constexpr int kRbBinBlockDefault = 1024;
constexpr uint32_t kRbMaxSc = 1024;  // K5 super-chunks per launch (one run per resolve thread)
constexpr int kInlineMax = 256;      // keys of an inline (kernarg-carried) Add
constexpr int kInlineGetMax = 512;   // keys of an inline Get
constexpr int kInlineMaxChunks = 16;   // inline launches per call at most (reply buffer size)
constexpr unsigned long long kEmpty64 = ~0ull;
constexpr uint32_t kEmpty32 = 0xFFFFFFFFu;

// Error bits in ovf.stat[1].
constexpr uint32_t kErrOverflowFull = 1u;
constexpr uint32_t kErrRowOutOfRange = 2u;  // a row shard's device Add met a key outside its range (dropped)
constexpr uint32_t kErrSparseFull = 4u;     // a sparse shard's writing call met a new key with no slot left (dropped)

struct DevBatch {
  const uint32_t* keys;
  const void* vals;  // input values for Add, output for Get
  uint64_t n;
};

// Passed by value as the kernel argument (fits the 4 KiB kernarg segment).
struct GroupArgs {
  int nb;
  uint32_t wg_prefix[kMaxBatches + 1];  // first workgroup of each batch
  DevBatch b[kMaxBatches];
};
static_assert(sizeof(GroupArgs) <= 1800, "a group plus the other arguments fit the 4 KiB kernarg segment");

// The batches of an Add group whose conditional replay rides on the next Get's
// K1 launch (K1r, pskv_add_get_grouped): a second group in the same kernarg
// segment, without the workgroup prefix the replay does not read.
struct ReplayGroup {
  int nb;
  DevBatch b[kMaxBatches];
};
static_assert(sizeof(GroupArgs) + sizeof(ReplayGroup) <= 3500,
              "K1r's two groups plus its other arguments fit the 4 KiB kernarg segment");

// K8: a whole small message inside the kernel arguments (<= 4 KiB kernarg).
struct InlineAdd {
  uint32_t n;
  uint32_t keys[kInlineMax];
  unsigned long long vals[kInlineMax];  // value bits (4-byte values in the low word)
};
struct InlineGet {
  uint32_t n;
  uint32_t keys[kInlineGetMax];
};
static_assert(sizeof(InlineAdd) + 128 <= 4096 && sizeof(InlineGet) + 128 <= 4096,
              "inline messages must fit the kernarg segment with the other arguments");

// K9: the small-message server (PSKV_SERVE=1): one resident workgroup polls a
// ring of requests in coherent page-locked host memory and applies them in
// ring order, so a small Add or Get costs no kernel launch.
constexpr int kSrvSlots = 64;
constexpr uint32_t kSrvAdd = 1, kSrvGet = 2;
struct SrvSlot {  // the kernel reads {kind, n} and {reply_off, pad} as 8-byte words
  uint32_t kind;       // kSrvAdd / kSrvGet
  uint32_t n;          // keys: <= kInlineMax (Add) / kInlineGetMax (Get)
  uint32_t reply_off;  // Get: first reply element
  uint32_t pad;
  uint32_t keys[kInlineGetMax];
  unsigned long long vals[kInlineMax];  // value bits (4-byte values in the low word)
};
struct SrvRing {  // the kernel polls {req_seq, stop} as one 8-byte word
  uint32_t req_seq;    // host: number of the last request posted
  uint32_t stop;       // host: 1 = leave the loop
  uint32_t pad0[30];
  uint32_t done_seq;   // device: number of the last request applied
  uint32_t alive;      // host sets 1 at launch; device: 0 once the kernel has left its loop
  uint32_t started;    // device: the launch generation now running (stored on entry)
  uint32_t pad1[29];
  SrvSlot slot[kSrvSlots];
};
static_assert(sizeof(SrvSlot) % 8 == 0 && offsetof(SrvRing, slot) % 8 == 0, "8-byte words in the ring");

struct DenseView {
  void* param;
  uint32_t key_begin;
  uint64_t range;  // number of owned keys, <= 2^32
  // The resident window (option RESIDENT_BYTES): offsets [0,
  // resident) of the dense array, in keys from key_begin, are meant to stay in
  // the Infinity Cache.  K2g's dense mode and K1 / K1r reach them with plain
  // stores and loads and every other parameter with non-temporal ones; a cache
  // hint only, every other kernel ignores it.  0: no window.
  uint64_t resident;
};

// The overflow table: open addressing over u64 key slots (EMPTY = ~0) for the
// keys outside the dense range (the last range server's fall-through keys,
// range_partition_manager.hpp:26-27).  Its arrays can be replaced while work
// is queued -- a single-workgroup inserter grows the table on the device
// (ovf_reserve, DESIGN.md §4 "Overflow growth") -- so kernels reach them
// through the shard's control block, whose address is fixed for the shard's
// life, and load them when they meet an out-of-range key.
struct OvfTab {
  unsigned long long* keys;
  void* vals;
  uint64_t mask;  // capacity - 1 (capacity is a power of two)
};
// Growth requests of device-side inserters: one per shard, in coherent
// page-locked host memory; the library's grow service (pskv_shard.cpp) answers
// each with fresh arrays of the asked capacity, the requesting workgroup fills
// and rehashes them itself and switches the control block over.
struct OvfMbox {
  uint32_t req_seq;   // device: number of the last request
  uint32_t pad0;
  uint64_t req_cap;   // device: slots asked for (a power of two)
  uint64_t wait_ticks;  // host: bound of a request's wait (device wall-clock ticks)
  uint64_t pad1[5];
  uint32_t resp_seq;  // host: number of the last request answered
  uint32_t resp_ok;   // host: 1 = resp_tab holds uninitialised arrays of req_cap slots
  OvfTab resp_tab;
  uint64_t pad2[4];
};
static_assert(sizeof(OvfMbox) == 128, "device and host words on separate 64-byte lines");
struct OvfCtl {  // device memory
  OvfTab t;          // the current table
  uint32_t stat[2];  // {occupied slots, sticky error bits}
  OvfMbox* mbox;     // growth requests
};
struct Ovf {  // kernel argument
  OvfCtl* c;
};

// Launch wrappers (pskv_kernels.hip).  vb = value bytes (4 or 8), vec = all
// pointers 16-byte aligned so 16 B vector accesses are legal.
// unroll: 4 or 8 groups of 4 keys per lane (chunk = 256*4*unroll keys);
// nt: non-temporal loads/stores of the streamed push/pull buffers.
hipError_t launch_gather(int vb, bool vec, int unroll, bool nt, const GroupArgs& ga,
                         uint32_t nwg, const DenseView& d, const Ovf& o, hipStream_t st);
hipError_t launch_assign_sorted(int vb, bool vec, const uint32_t* keys, const void* vals,
                                uint64_t n, const DenseView& d, uint32_t* flag, uint32_t epoch,
                                hipStream_t st);
// Grouped sorted Add.  `ga` must be built with stream_chunk(unroll) elements per chunk
// (used by the dense-window mode); the tile mode ignores the chunking.
// ntp: non-temporal parameter stores in the dense-window mode, outside the
// resident window (d.resident; chunks inside it store plainly)
hipError_t launch_assign_group(int vb, bool vec, int unroll, bool nt, bool ntp, bool early,
                               const GroupArgs& ga,
                               const DenseView& d, uint32_t tile_shift, uint64_t ntiles,
                               uint32_t grid, uint32_t* flag, uint32_t epoch, hipStream_t st);
// K4a: in-range keys only; an out-of-range key tags *oor with `epoch` for the
// oor_only replay behind K4.
hipError_t launch_general_mark(int dtype, int mode, const GroupArgs& ga, uint32_t nwg,
                               const DenseView& d, uint32_t* oor, unsigned long long* owner,
                               const uint32_t* cond, uint32_t epoch, hipStream_t st);
hipError_t launch_general_commit(int vb, const GroupArgs& ga, uint32_t nwg, const DenseView& d,
                                 const unsigned long long* owner,
                                 const uint32_t* cond, uint32_t epoch, hipStream_t st);
// Host growth of the table (pskv_sync keeps its load <= 1/2): rehash the
// current table (from_cap slots) into `to` (keys EMPTY, values 0), then
// switch the control block over.
hipError_t launch_ovf_rehash(int vb, const Ovf& o, uint64_t from_cap, const OvfTab& to, hipStream_t st);
// K4r: conditional replay of a group in call order by ONE workgroup (runs only
// when *cond == epoch: a sorted-path hint was broken); assign or accumulate.
// oor_only: only the group's out-of-range keys (behind K4, which leaves them
// to this single workgroup, the only kind of inserter that can grow the table).
hipError_t launch_replay(int dtype, int mode, const GroupArgs& ga, const DenseView& d, const Ovf& o,
                         const uint32_t* cond, uint32_t epoch, hipStream_t st, bool oor_only = false);
// K1r: K1 with an assign group's conditional replay folded in (the launch K4r
// would cost): when *cond == epoch, workgroup 0 replays `rg` and then gathers
// every chunk of `ga` itself while the other workgroups leave; otherwise K1.
// tab: kK1rTableWords words of device scratch (the replay's table, K1r has no LDS).
constexpr uint32_t kK1rTableWords = 4100;
hipError_t launch_gather_replay(int vb, bool vec, int unroll, bool nt, const GroupArgs& ga, uint32_t nwg,
                                const DenseView& d, const Ovf& o, const ReplayGroup& rg,
                                const uint32_t* cond, uint32_t epoch, uint32_t* tab, hipStream_t st);
// K5 radix-bucket general Add (2 launches: K5a bin, K5b resolve).  `ga`
// chunked by rb_superchunk(vb, bin_block) keys (nsc <= kRbMaxSc super-chunks);
// nbd dense buckets (RbMap) plus one out-of-range bucket.  bin_block: K5a's
// workgroup size, 1024 (one per CU) or 512 (two per CU, half the super-chunk).
// Scratch: loff: nsc * (nbd+2) u16 (each super-chunk's bucket starts); tmp:
// nsc * rb_superchunk(vb, bin_block) entries (rb_entry_bytes(vb) each).
// apply_log2: log2 of the resolve workgroup's LDS table slots (13: 64 KiB, two
// workgroups per CU, ~7 Ki entries per bucket in one pass; 14: 128 KiB, ~14 Ki).
hipError_t launch_rb_add(int dtype, int mode, const GroupArgs& ga, uint32_t nsc,
                         const DenseView& d, const Ovf& o, const RbMap& bm,
                         int apply_log2, int bin_block, uint16_t* loff, void* tmp,
                         hipStream_t st);
uint32_t rb_superchunk(int vb, int bin_block);
constexpr size_t kRbTmpPad = 16;  // bytes past the last entry K5b may read (paired loads)
// K8: one small host message carried in the kernarg segment (one workgroup).
// Get writes its n values to `out` (page-locked host memory or device memory);
// with `done` non-null it then stores `seq` there (system-scope release) for a
// host that polls instead of waiting on the stream.
hipError_t launch_inline_add(int dtype, int mode, const InlineAdd& a, const DenseView& d,
                             const Ovf& o, hipStream_t st);
hipError_t launch_inline_get(int vb, const InlineGet& a, const DenseView& d, const Ovf& o,
                             void* out, unsigned int* done, unsigned int seq, hipStream_t st);
// K9: start the request server on `st` (one workgroup; requests start_seq+1..
// are applied as they are posted).  It stores `gen` in ring->started on entry,
// leaves its loop when ring->stop is set or after idle_ticks wall-clock ticks
// without a request, and then clears alive.
hipError_t launch_serve(int dtype, int mode, SrvRing* ring, const DenseView& d, const Ovf& o,
                        void* reply, uint32_t start_seq, unsigned long long idle_ticks,
                        uint32_t gen, hipStream_t st);
size_t rb_entry_bytes(int vb);
// K6: tag `flag` with `epoch` unless every batch is a dense in-range window
// (chunk = kBlock * 4 * 8 keys per workgroup).
hipError_t launch_dense_check(const GroupArgs& ga, uint32_t nchunks, const DenseView& d,
                              uint32_t* flag, uint32_t epoch, hipStream_t st);
// K7: accumulate dense windows (skips when flag == epoch); chunk as K6.
hipError_t launch_acc_dense(int dtype, const GroupArgs& ga, uint32_t grid, const DenseView& d,
                            const uint32_t* flag, uint32_t epoch, hipStream_t st);


// Row-valued shards (pskv_rows.hip): W values per key, row-major.  A row is
// `units` units of `unit_bytes` (16, or the element size); a group of `lanes`
// = min(64, next_pow2(units)) = 1 << lshift lanes owns one row at a time.
struct RowShape {
  uint32_t units;
  uint32_t unit_bytes;
  uint32_t lanes;
  uint32_t lshift;
};
// unit16: the row size is a multiple of 16 bytes and every row pointer of the
// launch is 16-byte aligned (the copy kernels); false: one element per unit.
RowShape row_shape(uint32_t width, int vb, bool unit16);
// `ga` chunked by kGeneralChunk keys; batch pointers step width * vb bytes per key.
// Get: zeros for a key outside the range.
hipError_t launch_row_gather(int vb, bool nt, const GroupArgs& ga, uint32_t nwg, const DenseView& d,
                             const RowShape& rs, hipStream_t st);
// Behind launch_general_mark (stamp mode) over the same `ga` and epoch: the
// element whose tag equals its key's stamp copies its row.  Out-of-range keys
// set kErrRowOutOfRange in o.c->stat[1].
hipError_t launch_row_commit(int vb, const GroupArgs& ga, uint32_t nwg, const DenseView& d,
                             const unsigned long long* owner, const Ovf& o, uint32_t epoch,
                             const RowShape& rs, hipStream_t st);
// One no-return atomic add per element (rs built with unit16 = false).
hipError_t launch_row_accumulate(int dtype, const GroupArgs& ga, uint32_t nwg, const DenseView& d,
                                 const Ovf& o, const RowShape& rs, hipStream_t st);

// Optimizer steps (pskv_apply), float shards of any width
// (1 included).  The hyper-parameters travel by value: OptArgs<double> on the
// host, rounded to the value type once per launch, so a change is ordered by
// the stream.
// Momentum: mu, nesterov.  Adam: beta1, omb1 = 1 - beta1,
// beta2, omb2 = 1 - beta2, and the step's bias corrections a = lr / (1 -
// beta1^t), b = 1 / sqrt(1 - beta2^t), all computed on the host in double.
// FTRL-Proximal: l1, l2, fbeta (the configuration's
// ftrl_beta) and inv_lr = 1 / lr, computed on the host in double.  A launch
// has one kind, and FTRL uses none of momentum's and Adam's fields, so its
// four share their storage: the struct, and with it the kernel arguments and
// the code of every older instantiation, stay as they were.
template <typename T>
struct OptArgs {
  T lr, wd, eps;
  union {
    struct {
      T mu, beta1, omb1, beta2, omb2, a, b;
    };
    struct {
      T l1, l2, fbeta, inv_lr;
    };
  };
  int nesterov;
};
// A step's two launches, behind launch_general_mark (stamp mode) with the same
// epoch, over one of three argument blocks `a` of nwg virtual workgroups of
// kGeneralChunk positions (nwg == 0: nothing is launched):
//   GroupArgs      a launch group with its gradient rows (b[j].vals), as the
//                  mark took it.
//   PoolPushArgs   pooled push (pskv_apply_pooled): one batch of
//                  1 to kMaxPiece keys, the mark over {keys, n}.  The gradient
//                  row of key position i is formed in registers, weights[i] *
//                  bag_grads[bag(i)] (one multiplication rounded to the value
//                  type; weights null: the bag's row itself); nbags >= 1.  The
//                  bag of a position: pskv_plan.h (pool_bag_span,
//                  pool_bags_in); whatever the offsets hold it is below nbags.
//   PoolGroupArgs  grouped pooled push (pskv_apply_pooled_grouped, DESIGN.md
//                  §8h; pskv_plan.h): a launch group of such batches, the mark
//                  over the GroupArgs of the same batches (keys and n).  A
//                  virtual workgroup belongs to one batch; a position's tag
//                  carries the keys of the batches before it.  When some batch
//                  has weights, one without them contributes its bag rows
//                  unmultiplied.
// A pooled block that is not as described is refused (hipErrorInvalidValue).
struct PoolPushArgs {
  const uint32_t* keys;     // n
  const void* weights;      // n values, or null
  const uint64_t* offsets;  // nbags + 1 (the kernels read [0, nbags))
  uint64_t n, nbags;
  const void* bag_grads;    // nbags rows
};
// Every in-range position that is NOT its key's winner adds its gradient row
// into gsum (shaped as the dense array, zero between calls), one no-return
// atomic per element (rs built with unit16 = false).  Out-of-range keys set
// kErrRowOutOfRange.  d.param is not touched.
template <typename Args>
hipError_t launch_row_step_losers(int dtype, const Args& a, uint32_t nwg, const DenseView& d, void* gsum,
                                  const unsigned long long* owner, const Ovf& o, uint32_t epoch, const RowShape& rs,
                                  hipStream_t st);
// Each winner applies the rule (kind: pskv_optimizer_kind, 1 to 5) once to its
// key's row from its own gradient row plus the gsum row, and writes zeros back
// to the gsum units it read non-zero.  state[0]: slot 0 (Adagrad's h,
// momentum's v, Adam's m, FTRL's z); state[1]: slot 1 (Adam's v, FTRL's n).
// unit16 also wants every batch's rows (vals, bag_grads) 16-byte aligned.
template <typename Args>
hipError_t launch_row_step_apply(int dtype, int kind, const Args& a, uint32_t nwg, const DenseView& d, void* gsum,
                                 void* const state[2], const unsigned long long* owner, uint32_t epoch,
                                 const RowShape& rs, const OptArgs<double>& hy, hipStream_t st);
// p[0..n) = v (float or double by dtype): the accumulator's initial value.
hipError_t launch_fill(int dtype, void* p, uint64_t n, double v, hipStream_t st);

// Pooled pull (pskv_get_pooled): out row b = sum over bag b's
// keys of weight * row(key), in the shard's value type; the bags, their clamp,
// the order of the additions and the chunks of long bags: pskv_plan.h.
struct PoolArgs {
  const uint32_t* keys;     // n
  const void* weights;      // n values, or null: every weight is one
  const uint64_t* offsets;  // nbags + 1
  uint64_t n, nbags;
  void* out;   // nbags rows
  void* part;  // pool_slots(n) partial rows of long bags' chunks; null when n <= kPoolChunk
};
// Long bags first (launch_row_pooled_chunks, skipped when no bag can be long:
// n <= kPoolChunk), then every bag (launch_row_pooled).  A key outside the
// range counts as a zero row and sets kErrRowOutOfRange.  rs by row_shape;
// unit16 also wants out, part and the dense array 16-byte aligned.
hipError_t launch_row_pooled_chunks(int dtype, const PoolArgs& a, const DenseView& d, const Ovf& o,
                                    const RowShape& rs, hipStream_t st);
hipError_t launch_row_pooled(int dtype, bool nt, const PoolArgs& a, const DenseView& d, const Ovf& o,
                             const RowShape& rs, hipStream_t st);

// Sparse shards (pskv_index.hip): the hash index that maps a
// uint32 key to a slot of the row arrays.  table: mask + 1 entries (a power of
// two, >= 2 * capacity), linear probing from fmix32(key).  An entry is 0 when
// empty; otherwise key + 1 sits in its low 33 bits and slot + 1 in its high
// 31 bits, 0 there meaning "claimed, no slot yet or none granted".  Entries
// are never emptied while work is queued (pskv_clear zeroes the table).
// slot_keys[slot]: the key of a slot.  stat: the shard's OvfCtl::stat -- a
// sparse shard keeps nothing in its overflow table, so [0] is the number of
// slots handed out and [1] the sticky error word (kErrSparseFull).
constexpr int kIndexKeyBits = 33;
struct SparseIndex {
  unsigned long long* table;
  uint32_t* slot_keys;
  uint32_t* stat;
  uint64_t mask;
  uint32_t capacity;  // slots, <= 2^31 - 2
};
// `ga` chunked by kGeneralChunk keys, nwg virtual workgroups (nwg == 0:
// nothing is launched).  Insert reads b[j].keys only: every key of the group
// that has no entry claims one, and the claimer takes a slot while one is left
// (else the entry stays slotless and kErrSparseFull is set).  No lane waits for
// another, and every probe loop ends after mask + 1 entries.
hipError_t launch_index_insert(const GroupArgs& ga, uint32_t nwg, const SparseIndex& x, hipStream_t st);
// Behind the insert in stream order: b[j].vals (uint32, may be b[j].keys itself)
// receives a slot id per position: the key's slot; for a key without one,
// `capacity` (the zero row) when reading, and when writing 0xFFFFFFFF, which the
// row kernels drop, with kErrSparseFull set.
hipError_t launch_index_translate(bool writing, const GroupArgs& ga, uint32_t nwg, const SparseIndex& x,
                                  hipStream_t st);
// Growth and erase, on a shard with nothing else queued.
// Mark: dead[ids[i]] = 1 for every id <= capacity (`dead`: capacity + 1 zeroed
// flags; ids from a reading translate).  Rebuild: the index of `x` -- its table
// zeroed by the caller -- from old_keys[0 .. count), the keys of the old slots.
// dead == nullptr: every slot keeps its number and x.stat[0] is left alone.
// Else the slots without a flag are compacted in unspecified order: new numbers
// are drawn from x.stat[0], which the caller zeroed and which ends at the
// number of survivors, and survivors[new slot] = old slot.  Either way
// x.slot_keys is written and the full bits of x.stat[1] are cleared.
hipError_t launch_index_mark_dead(const uint32_t* ids, uint64_t n, uint32_t capacity, uint8_t* dead, hipStream_t st);
hipError_t launch_index_rebuild(const uint32_t* old_keys, uint32_t count, const uint8_t* dead, const SparseIndex& x,
                                uint32_t* survivors, hipStream_t st);

}  // namespace pskv
