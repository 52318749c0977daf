// ps/hip_storage.hpp — HipStorage<Val>: the HBM-backed drop-in for the
// reference's MapStorage<Val> (server/map_storage.hpp) and VectorStorage<Val>
// (server/vector_storage.hpp), implemented over the pskv C ABI (pskv.h).
//
// Inside the reference tree define PSKV_IN_REFERENCE_TREE before including
// this header so it derives from the reference's own server/abstract_storage.hpp
// (after adding the virtual destructor); standalone it
// uses the restated boundary in include/ps/.
//
// Contract kept from the reference:
//   * SubAdd: CHECK_EQ(keys, vals) then last-write-wins assign (map_storage.hpp:19-24)
//   * SubGet: a new owning SArray<char> of keys.size() values, 0 for missing keys
//     (map_storage.hpp:29-45); the reply keys alias the request (abstract_storage.hpp:27)
//   * errors abort, as glog CHECK does (abstract_storage.hpp:15,20)
//   * called from one server thread; the device is selected inside every call
//     because Engine::CreateTable constructs storages on another thread
//     (driver/engine.hpp:100-109)
// Page-locked frames (ps/host_frames.hpp): every call passes
// PSKV_HOST_FRAME, so request payloads the mailbox received into frames are
// read in place (an Add returns once queued; the frames stay alive through
// the message's SArrays and the pool holds them until the work has run), and
// Get replies are frames the kernel writes directly.  Payloads outside frames
// take the ordinary host paths.
// Row-valued storage (width > 1, pskv_shard_create_rows): every key holds
// `width` values; SubAdd takes keys.size() * width values (row-major), SubGet
// replies with as many.  Such a storage holds only the keys of its range
// (pskv.h), so construct it with the range the server owns.
// Optimizer (last constructor argument, pskv_shard_set_optimizer; a
// pskv_optimizer_ex there, pskv_shard_set_optimizer_ex, also gives momentum
// and Adam; a pskv_optimizer_cfg, pskv_shard_set_optimizer_cfg, also
// FTRL-Proximal): the storage applies optimizer steps.  SubAdd then carries GRADIENTS and is one step
// (pskv_apply); AddGrouped, the BSP model's flush, is ONE step over the summed
// gradients of all its messages (pskv_apply_grouped).  Float Val only; keys
// outside the range abort the call (pskv.h "Optimizer steps").
// Pooled pulls (SubGetPooled, pskv_get_pooled): one reply row per bag of keys,
// the weighted sum of the bag's rows computed in the shard -- the margin
// sum_i w[key_i] * x_i of the reference's logistic-regression worker as one
// pull of one value per sample.  Keys outside the range abort.
// Pooled pushes (SubApplyPooled, pskv_apply_pooled): one gradient row per bag,
// expanded in the shard inside one optimizer step; SubApplyPooledGrouped
// (pskv_apply_pooled_grouped) makes ONE step of several workers' pooled pushes,
// the BSP flush, as AddGrouped does of their plain pushes.
// Sparse storage (HipStorage<Val>::Sparse, pskv_shard_create_sparse): the
// storage owns EVERY key and holds at most `capacity` distinct ones, `width`
// values each, in memory that follows capacity -- the storage of a server under
// consistent hashing, or of a table of hashed feature ids (pskv.h "Sparse
// shards").  Every method above works unchanged on it; a key
// that finds no room is dropped and FinishIter aborts ("sparse shard full").
// Reserve grows it, SetGrowth lets the pushes grow it themselves up to a limit
// (as the reference's std::map takes whatever keys arrive) and Erase forgets
// keys, as std::map::erase does.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "pskv.h"
#include "ps/host_frames.hpp"

#ifdef PSKV_IN_REFERENCE_TREE
#include "server/abstract_storage.hpp"
#else
#include "ps/abstract_storage.hpp"
#endif

namespace csci5570 {

template <typename Val>
struct PskvDtype;
template <>
struct PskvDtype<int> {
  static constexpr int value = PSKV_I32;
};
template <>
struct PskvDtype<float> {
  static constexpr int value = PSKV_F32;
};
template <>
struct PskvDtype<double> {
  static constexpr int value = PSKV_F64;
};

inline void pskv_check(int rc, const char* what) {
  if (rc != PSKV_OK) {
    std::fprintf(stderr, "Check failed: %s returned %d: %s\n", what, rc, pskv_last_error());
    std::abort();
  }
}

template <typename Val>
class HipStorage : public AbstractStorage {
 public:
  // No arguments = the reference's construction: whole key space, assign.
  explicit HipStorage(int device = 0, uint32_t key_begin = 0, uint64_t key_end = 1ull << 32,
                      int mode = PSKV_ASSIGN, uint64_t overflow_slots = 0, uint32_t width = 1,
                      const pskv_optimizer* optimizer = nullptr)
      : width_(width), stepping_(optimizer != nullptr && optimizer->kind != PSKV_OPT_NONE) {
    Create(device, key_begin, key_end, mode, overflow_slots);
    if (optimizer) pskv_check(pskv_shard_set_optimizer(shard_, optimizer), "pskv_shard_set_optimizer");
  }
  // The same with the extended configuration (momentum, Adam; every argument given).
  HipStorage(int device, uint32_t key_begin, uint64_t key_end, int mode, uint64_t overflow_slots, uint32_t width,
             const pskv_optimizer_ex* optimizer)
      : width_(width), stepping_(optimizer != nullptr && optimizer->kind != PSKV_OPT_NONE) {
    Create(device, key_begin, key_end, mode, overflow_slots);
    if (optimizer) pskv_check(pskv_shard_set_optimizer_ex(shard_, optimizer), "pskv_shard_set_optimizer_ex");
  }
  // The same with the configuration that also holds FTRL-Proximal (l1, l2, ftrl_beta).
  HipStorage(int device, uint32_t key_begin, uint64_t key_end, int mode, uint64_t overflow_slots, uint32_t width,
             const pskv_optimizer_cfg* optimizer)
      : width_(width), stepping_(optimizer != nullptr && optimizer->kind != PSKV_OPT_NONE) {
    Create(device, key_begin, key_end, mode, overflow_slots);
    if (optimizer) pskv_check(pskv_shard_set_optimizer_cfg(shard_, optimizer), "pskv_shard_set_optimizer_cfg");
  }
  // A sparse storage of at most `capacity` distinct keys; optimizer: null, or
  // any of the three configuration structs, as the constructors take them.
  static std::unique_ptr<HipStorage> Sparse(int device, uint64_t capacity, int mode = PSKV_ASSIGN, uint32_t width = 1) {
    return std::unique_ptr<HipStorage>(new HipStorage(SparseTag(), device, capacity, mode, width));
  }
  static std::unique_ptr<HipStorage> Sparse(int device, uint64_t capacity, int mode, uint32_t width,
                                            const pskv_optimizer* optimizer) {
    auto st = Sparse(device, capacity, mode, width);
    if (optimizer) pskv_check(pskv_shard_set_optimizer(st->shard_, optimizer), "pskv_shard_set_optimizer");
    st->stepping_ = optimizer != nullptr && optimizer->kind != PSKV_OPT_NONE;
    return st;
  }
  static std::unique_ptr<HipStorage> Sparse(int device, uint64_t capacity, int mode, uint32_t width,
                                            const pskv_optimizer_ex* optimizer) {
    auto st = Sparse(device, capacity, mode, width);
    if (optimizer) pskv_check(pskv_shard_set_optimizer_ex(st->shard_, optimizer), "pskv_shard_set_optimizer_ex");
    st->stepping_ = optimizer != nullptr && optimizer->kind != PSKV_OPT_NONE;
    return st;
  }
  static std::unique_ptr<HipStorage> Sparse(int device, uint64_t capacity, int mode, uint32_t width,
                                            const pskv_optimizer_cfg* optimizer) {
    auto st = Sparse(device, capacity, mode, width);
    if (optimizer) pskv_check(pskv_shard_set_optimizer_cfg(st->shard_, optimizer), "pskv_shard_set_optimizer_cfg");
    st->stepping_ = optimizer != nullptr && optimizer->kind != PSKV_OPT_NONE;
    return st;
  }
  ~HipStorage() override { pskv_shard_destroy(shard_); }
  HipStorage(const HipStorage&) = delete;
  HipStorage& operator=(const HipStorage&) = delete;

  void SubAdd(const third_party::SArray<Key>& typed_keys,
              const third_party::SArray<char>& vals) override {
    auto typed_vals = third_party::SArray<Val>(vals);
    if (typed_keys.size() * width_ != typed_vals.size()) {
      std::fprintf(stderr, "Check failed: typed_keys.size() * width == typed_vals.size() (%zu * %u vs %zu)\n",
                   (size_t)typed_keys.size(), (unsigned)width_, (size_t)typed_vals.size());
      std::abort();
    }
    if (stepping_) {
      pskv_check(pskv_apply(shard_, typed_keys.data(), typed_vals.data(), typed_keys.size(),
                            PSKV_HOST | PSKV_HOST_FRAME),
                 "pskv_apply");
      return;
    }
    pskv_check(pskv_add(shard_, typed_keys.data(), typed_vals.data(), typed_keys.size(),
                        PSKV_HOST | PSKV_HOST_FRAME),
               "pskv_add");
  }

#ifndef PSKV_IN_REFERENCE_TREE
  // One staged copy and one grouped launch for a run of Add messages (BSP flush).
  void AddGrouped(std::vector<Message>& msgs) override {
    std::vector<pskv_batch> batches;
    std::vector<third_party::SArray<Key>> keep_k;
    std::vector<third_party::SArray<Val>> keep_v;
    batches.reserve(msgs.size());
    for (auto& m : msgs) {
      if (m.data.size() != 2) {
        std::fprintf(stderr, "Check failed: msg.data.size() == 2\n");
        std::abort();
      }
      keep_k.emplace_back(m.data[0]);
      keep_v.emplace_back(m.data[1]);
      if (keep_k.back().size() * width_ != keep_v.back().size()) {
        std::fprintf(stderr, "Check failed: typed_keys.size() * width == typed_vals.size()\n");
        std::abort();
      }
      batches.push_back(pskv_batch{keep_k.back().data(), keep_v.back().data(), keep_k.back().size()});
    }
    if (stepping_) {
      pskv_check(pskv_apply_grouped(shard_, batches.data(), batches.size(), PSKV_HOST | PSKV_HOST_FRAME),
                 "pskv_apply_grouped");
      return;
    }
    pskv_check(pskv_add_grouped(shard_, batches.data(), batches.size(), PSKV_HOST | PSKV_HOST_FRAME),
               "pskv_add_grouped");
  }
#endif

  third_party::SArray<char> SubGet(const third_party::SArray<Key>& typed_keys) override {
    // the reply is a page-locked frame: written in place by the kernel when the
    // request keys are a frame too, and sent zero-copy by the Sender
    auto reply_vals = FrameArray<Val>(typed_keys.size() * width_);
    pskv_check(pskv_get(shard_, typed_keys.data(), typed_keys.size(), reply_vals.data(),
                        PSKV_HOST | PSKV_HOST_FRAME),
               "pskv_get");
    return third_party::SArray<char>(reply_vals);
  }

  // One pooled row per bag (pskv_get_pooled): bag b is typed_keys[offsets[b],
  // offsets[b+1]); weights null: every weight one.  The reply is a frame of
  // (offsets.size() - 1) * width values.  Not part of AbstractStorage.
  third_party::SArray<char> SubGetPooled(const third_party::SArray<Key>& typed_keys,
                                         const third_party::SArray<Val>* weights,
                                         const third_party::SArray<uint64_t>& offsets) {
    if (offsets.size() == 0 || (weights && weights->size() != typed_keys.size())) {
      std::fprintf(stderr, "Check failed: offsets.size() >= 1 and weights.size() == typed_keys.size()\n");
      std::abort();
    }
    const uint64_t nbags = offsets.size() - 1;
    auto reply_vals = FrameArray<Val>(nbags * width_);
    pskv_check(pskv_get_pooled(shard_, typed_keys.data(), typed_keys.size(), weights ? weights->data() : nullptr,
                               offsets.data(), nbags, reply_vals.data(), PSKV_HOST | PSKV_HOST_FRAME),
               "pskv_get_pooled");
    return third_party::SArray<char>(reply_vals);
  }

  // One optimizer step from one gradient row per bag (pskv_apply_pooled), the
  // bags as SubGetPooled's: the gradient row of typed_keys[i] is weights[i] *
  // bag_grads[b], b the bag that holds position i; bag_grads holds
  // (offsets.size() - 1) * width values.  Not part of AbstractStorage.
  void SubApplyPooled(const third_party::SArray<Key>& typed_keys, const third_party::SArray<Val>* weights,
                      const third_party::SArray<uint64_t>& offsets, const third_party::SArray<Val>& bag_grads) {
    if (offsets.size() == 0 || (weights && weights->size() != typed_keys.size()) ||
        bag_grads.size() != (offsets.size() - 1) * width_) {
      std::fprintf(stderr, "Check failed: offsets.size() >= 1, weights.size() == typed_keys.size() and "
                           "bag_grads.size() == (offsets.size() - 1) * width\n");
      std::abort();
    }
    pskv_check(pskv_apply_pooled(shard_, typed_keys.data(), typed_keys.size(), weights ? weights->data() : nullptr,
                                 offsets.data(), offsets.size() - 1, bag_grads.data(), PSKV_HOST | PSKV_HOST_FRAME),
               "pskv_apply_pooled");
  }

  // The four arrays of one SubApplyPooled call, each a counted reference, so a
  // deferred push keeps its data alive until the flush (weighted false: every
  // weight is one and `weights` is not read).
  struct PooledPush {
    third_party::SArray<Key> keys;
    third_party::SArray<Val> weights;
    bool weighted;
    third_party::SArray<uint64_t> offsets;
    third_party::SArray<Val> bag_grads;
  };

  // ONE optimizer step from the pooled pushes of several workers
  // (pskv_apply_pooled_grouped): the BSP flush of an iteration's deferred
  // SubApplyPooled calls, as AddGrouped is to SubAdd.  Not part of AbstractStorage.
  void SubApplyPooledGrouped(const std::vector<PooledPush>& pushes) {
    std::vector<pskv_pool_batch> batches;
    batches.reserve(pushes.size());
    for (const PooledPush& p : pushes) {
      if (p.offsets.size() == 0 || (p.weighted && p.weights.size() != p.keys.size()) ||
          p.bag_grads.size() != (p.offsets.size() - 1) * width_) {
        std::fprintf(stderr, "Check failed: batch %zu: offsets.size() >= 1, weights.size() == keys.size() and "
                             "bag_grads.size() == (offsets.size() - 1) * width\n", batches.size());
        std::abort();
      }
      batches.push_back(pskv_pool_batch{p.keys.data(), p.weighted ? p.weights.data() : nullptr, p.offsets.data(),
                                        p.bag_grads.data(), p.keys.size(), p.offsets.size() - 1});
    }
    pskv_check(pskv_apply_pooled_grouped(shard_, batches.data(), batches.size(), PSKV_HOST | PSKV_HOST_FRAME),
               "pskv_apply_pooled_grouped");
  }

  // A sparse storage only (pskv.h "Sparse shards"; not part of AbstractStorage).
  // Reserve: room for `capacity` distinct keys, every stored row kept.
  // SetGrowth: pushes grow the storage themselves, up to max_capacity keys (0:
  // fixed).  Erase: the keys are forgotten (absent keys are legal); a
  // maintenance call whose cost follows the keys stored.
  void Reserve(uint64_t capacity) { pskv_check(pskv_sparse_reserve(shard_, capacity), "pskv_sparse_reserve"); }
  void SetGrowth(uint64_t max_capacity) {
    pskv_check(pskv_sparse_set_growth(shard_, max_capacity), "pskv_sparse_set_growth");
  }
  void Erase(const third_party::SArray<Key>& typed_keys) {
    pskv_check(pskv_sparse_erase(shard_, typed_keys.data(), typed_keys.size(), PSKV_HOST), "pskv_sparse_erase");
  }

  // The reference's FinishIter is a no-op (map_storage.hpp:47); here it is the
  // point where deferred device errors surface and the overflow table, which
  // grows on the device as keys arrive, is trimmed and its old arrays freed.
  void FinishIter() override { pskv_check(pskv_sync(shard_), "pskv_sync"); }

  pskv_shard* shard() const { return shard_; }
  uint32_t width() const { return width_; }

 private:
  struct SparseTag {};
  HipStorage(SparseTag, int device, uint64_t capacity, int mode, uint32_t width) : width_(width) {
    pskv_check(pskv_shard_create_sparse(device, capacity, PskvDtype<Val>::value, mode, width_, &shard_),
               "pskv_shard_create_sparse");
  }
  // Both constructors' shard.
  void Create(int device, uint32_t key_begin, uint64_t key_end, int mode, uint64_t overflow_slots) {
    pskv_check(pskv_shard_create_rows(device, key_begin, key_end, PskvDtype<Val>::value, mode, width_,
                                      overflow_slots, &shard_),
               "pskv_shard_create");
  }

  pskv_shard* shard_ = nullptr;
  uint32_t width_ = 1;
  bool stepping_ = false;  // an optimizer is set: Adds are optimizer steps
};

}  // namespace csci5570
