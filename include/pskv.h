/*
 * pskv.h — C ABI of the MI355X-native parameter-shard store (Add/Get hot path).
 *
 * This is the drop-in boundary that replaces the arithmetic of the reference's
 * storage plugins:
 *
 *   reference interface                                   replaced by
 *   ---------------------------------------------------  -----------------------------
 *   AbstractStorage::SubAdd  server/abstract_storage.hpp:35-36   pskv_add / pskv_add_grouped
 *   AbstractStorage::SubGet  server/abstract_storage.hpp:39      pskv_get / pskv_get_grouped
 *   AbstractStorage::FinishIter server/abstract_storage.hpp:41   pskv_sync (the reference's is a no-op)
 *   MapStorage<Val>()        server/map_storage.hpp:15           pskv_shard_create(..., PSKV_ASSIGN)
 *   VectorStorage<Val>()     server/vector_storage.hpp:14        pskv_shard_create(..., PSKV_ASSIGN)
 *   ~AbstractStorage (missing in the reference) pskv_shard_destroy
 *   RangePartitionManager::Slice base/range_partition_manager.hpp:19-46,48-77  pskv_range_slice
 *   ConsistentHashingPartitionManager::JumpConsistentHash
 *                     base/consistent_hashing_partition_manager.hpp:81-89       pskv_jump_hash
 *   zmq receive buffer of a data frame, Mailbox::Recv comm/mailbox.cpp:246-257,
 *   and SubGet's reply allocation server/map_storage.hpp:30     pskv_host_alloc / pskv_host_free
 *
 * Semantics (PSKV_ASSIGN, the reference semantics; map_storage.hpp:22-23,
 * vector_storage.hpp:21-43): a shard is a last-write-wins key/value store with
 * uint32 keys (base/magic.hpp:7).  Within one call the LAST occurrence of a key
 * wins (index order), across calls the later call wins (call order on the
 * shard's stream).  A key that was never written reads as 0
 * (map_storage.hpp:33-37; zero-filled SArray in vector_storage.hpp:33).  Values
 * are copied bit-for-bit, so parity is bit-exact for every value type.
 *
 * PSKV_ACCUMULATE is the north-star gradient-reduction mode (param[k] += v for
 * every occurrence).  It has no reference counterpart; float sums follow the
 * tolerance stated in DESIGN.md (recursive-summation bound), int32 is exact.
 *
 * Keys outside [key_begin, key_end) are legal (the reference's last range
 * server receives every out-of-range key, range_partition_manager.hpp:26-27):
 * they live in a device-side overflow hash table with the same semantics, and
 * there is no limit on how many (as the reference's std::map has none).  Every
 * out-of-range insert, from host or device inputs, is made by ONE workgroup
 * that first reserves room: when the table would pass 3/4 load it asks the
 * library's grow service (a host thread) for larger arrays and rehashes into
 * them on the device, in stream order, so device callers need no host step
 * and no sizing (round 6; DESIGN.md §4 "Overflow growth").  pskv_sync trims
 * the load back to <= 1/2.  Keys are dropped -- and the next pskv_sync returns
 * PSKV_ESTATE -- only if a growth request is not answered within
 * SYNC_TIMEOUT_MS or its allocation fails (device memory exhausted).
 *
 * Row-valued shards (pskv_shard_create_rows, width W > 1): every key holds a
 * row of W values -- an embedding vector, a latent factor of the reference's
 * matrix-factorisation app (app/mf.cpp:392-397 flattens such a row into W
 * scalar keys for want of a row type).  Every call keeps its signature; n and
 * pskv_batch.n count KEYS; vals and out hold n * W values, row i at element
 * i * W (row-major), and so does the dense array.  PSKV_ASSIGN: the last
 * occurrence of a key wins and the WHOLE row comes from it (a stored row is
 * never a mix of two pushes); PSKV_ACCUMULATE: element-wise sums.  Column j of
 * a row shard behaves exactly like a scalar shard fed (keys, vals[:, j]).
 * PSKV_SORTED_HINT and the tuning options are accepted and change nothing;
 * PSKV_HOST_FRAME buffers are treated as plain host memory.
 * ONE LIMIT: a row shard stores no key outside [key_begin, key_end) (the
 * overflow table holds one value per slot; a sparse shard, below, takes every
 * key).  It refuses such keys loudly: a
 * host Add that contains one returns PSKV_EINVAL naming the first and applies
 * nothing; a device Add applies its in-range rows, drops the others, and the
 * next pskv_sync returns PSKV_ESTATE ("row shard ... out-of-range"; pskv_clear
 * resets it); a Get of such a key returns a row of zeros.
 *
 * Optimizer steps (pskv_shard_set_optimizer, pskv_apply): a
 * shard may carry an optimizer, and workers then push GRADIENTS.  pskv_apply
 * and pskv_apply_grouped take (key, gradient-row) batches shaped exactly like
 * an Add's, and ONE CALL IS ONE OPTIMIZER STEP:
 *   1. for every distinct in-range key k of the call (over all batches of a
 *      grouped call) g[k] is the element-wise sum of the gradient rows of all
 *      its occurrences, in unspecified order (as in accumulate);
 *   2. the rule is applied exactly once to that key's row, in the shard's
 *      value type T, with the hyper-parameters rounded to T once:
 *          d = g + weight_decay * p
 *          SGD:      p <- p - lr * d
 *          Adagrad:  h <- h + d*d ;  p <- p - lr * d / (sqrt(h) + eps)
 *      h is one accumulator per value (the shape of the dense array),
 *      starting at init_accum;
 *   3. keys not in the call keep p and h bit for bit.  Non-finite gradients
 *      propagate by IEEE rules; nothing checks for them.
 * A BSP flush of several workers' deferred pushes is one grouped call, hence
 * one step over the summed minibatch gradient.  Scope and limits:
 *   - float shards only (PSKV_F32, PSKV_F64); PSKV_I32 gives PSKV_EINVAL;
 *   - any width, 1 included (a width-1 step runs on the row kernels);
 *   - either creation mode; pskv_add and pskv_get keep their meaning on such
 *     a shard (an assign Add initialises the parameters);
 *   - keys outside [key_begin, key_end) are refused as a row shard's Add
 *     refuses them, also at width 1: a host call returns PSKV_EINVAL naming
 *     the first and applies nothing; a device call applies the in-range keys,
 *     drops the others, and the next pskv_sync returns PSKV_ESTATE
 *     (pskv_clear resets it).  The overflow table is not involved;
 *   - pskv_apply without an optimizer gives PSKV_EINVAL;
 *   - pskv_clear zeroes the parameters, resets h to init_accum and leaves the
 *     gradient scratch zero;
 *   - PSKV_SORTED_HINT is accepted and changes nothing; PSKV_HOST_FRAME
 *     buffers are treated as plain host memory;
 *   - with the resident request server (SERVE = 1) a step first ends the
 *     server, as every stream path of pskv_add / pskv_get does;
 *   - not provided: optimizer state for overflow keys.
 *
 * Momentum and Adam (pskv_shard_set_optimizer_ex).  Steps 1 and
 * 3 above are unchanged; d = g + weight_decay * p in T, every hyper-parameter
 * rounded to T once per launch:
 *   MOMENTUM  slot 0 is v, starting at 0:
 *               v <- momentum * v + d
 *               p <- p - lr * v        or, with nesterov,
 *               p <- p - lr * (d + momentum * v)   (the new v)
 *   ADAM      slot 0 is m, slot 1 is v, both starting at 0; t is this call's
 *             step number (1 for the first step after creation, pskv_clear or
 *             a kind change):
 *               m <- beta1 * m + (1 - beta1) * d
 *               v <- beta2 * v + (1 - beta2) * d * d
 *               p <- p - a * m / (sqrt(v) * b + eps)
 *             with a = lr / (1 - beta1^t) and b = 1 / sqrt(1 - beta2^t); a, b,
 *             1 - beta1 and 1 - beta2 are computed on the host in double and
 *             rounded to T once.  This is LAZY Adam: a key not in the call
 *             keeps p, m and v bit for bit, and the bias correction follows
 *             the shard's step count, not the key's.
 * Step counter: one uint64 per shard on the host, kept for every kind.  Every
 * pskv_apply / pskv_apply_grouped call that queues work advances it by one,
 * however many launch groups the call has (all use the same t); a call with no
 * keys or a refused call (host call with an out-of-range key, no optimizer, bad
 * argument) does not; a device call that drops out-of-range keys does.  The
 * same kind again keeps t and the state, another kind resets both; pskv_clear
 * resets t to 0 and the state to its start values.  pskv_set_step lets a
 * restored shard continue where the saved one stopped.
 * State slots (pskv_get_state_slot, pskv_put_state): SGD has none, Adagrad one
 * (h), momentum one (v), Adam two (m, v), FTRL two (z, n).  Saving p and
 * every slot of the whole range with the step count, and putting them back
 * with pskv_add, pskv_put_state and pskv_set_step, restores a shard bit for bit.
 * Not provided: decoupled weight decay (AdamW), amsgrad, per-key step counts.
 *
 * FTRL-Proximal (pskv_shard_set_optimizer_cfg, PSKV_OPT_FTRL):
 * the per-coordinate rule of McMahan et al., "Ad Click Prediction: a View
 * from the Trenches" (2013), whose L1 threshold leaves most weights of a
 * sparse model EXACTLY zero.  Steps 1 and 3 of "Optimizer steps" are
 * unchanged.  Slot 0 is z, starting at 0; slot 1 is n, starting at
 * init_accum.  Everything is computed in T, every hyper-parameter rounded to
 * T once per launch; inv_lr = 1 / lr is computed on the host in double:
 *     d  = g + weight_decay * p
 *     n' = n + d * d
 *     r  = sqrt(n')                        (computed once, used twice)
 *     s  = (r - sqrt(n)) * inv_lr
 *     z' = (z + d) - s * p
 *     p' = +0                                                 if |z'| <= l1
 *          (copysign(l1, z') - z') / ((ftrl_beta + r) * inv_lr + l2)   otherwise
 *   - the zero is +0 (bit pattern 0), never -0;
 *   - FTRL OWNS p: a step overwrites p with the closed form of z' and n'.  A
 *     p written by pskv_add enters the step only through s * p and the
 *     weight-decay term and is then replaced; to start from given weights,
 *     put the matching z with pskv_put_state;
 *   - non-finite inputs, and a negative n written by pskv_put_state, propagate
 *     by IEEE rules (sqrt of a negative n is a NaN); nothing checks for them
 *     ("Non-finite, subnormal and overflowing values" below);
 *   - the step counter, pskv_clear (z to 0, n to init_accum, t to 0) and a kind
 *     change follow the rules above; lazy as Adam: a key not in the call keeps
 *     p, z and n bit for bit;
 *   - not provided: lr_power other than -1/2, L2 shrinkage, per-key step
 *     counts.
 *
 * Non-finite, subnormal and overflowing values.  No call
 * checks for them and none treats them specially; one contract holds for every
 * step kind (SGD, Adagrad, momentum, Nesterov, Adam, FTRL) through pskv_apply,
 * pskv_apply_grouped, pskv_apply_pooled and pskv_apply_pooled_grouped, for
 * accumulate Adds on every path and for pooled pulls:
 *   - values propagate by IEEE 754 rules in T, element by element.  A NaN
 *     among a key's addends, or both infinities, gives NaN; one infinity gives
 *     itself; a sum or product that overflows T gives the infinity T
 *     arithmetic gives (max + max, Adagrad's h + d*d, Adam's v, FTRL's n, a
 *     weight times a bag row); 0 * inf of a weighted pooled call is NaN.  The
 *     rule then runs on that value as written above;
 *   - a non-finite value reaches only its own element of its own key: the other
 *     columns of the row, every other key and every later call on other keys
 *     are what they would be without it.  In particular the gradient scratch
 *     of the step kernels is all-zero bits again after every call, whatever
 *     the losers' sum was (NaN, an infinity, a subnormal, -0);
 *   - subnormal addends, sums and products are kept, not flushed to zero, in
 *     float and double, by the float atomics as by the plain arithmetic; -0.0
 *     added onto +0 is +0;
 *   - assign Adds and every Get move bits: NaN payloads, -0.0
 *     and subnormals come back unchanged.
 *
 * Pooled pulls (pskv_get_pooled): one row per BAG of keys, a bag
 * being one sample's contiguous run of the call's keys (bag b = keys
 * [offsets[b], offsets[b+1])):
 *     out[b*W + j] = sum over i in the bag of weights[i] * row(keys[i])[j]
 * -- the margin sum_i w[key_i] * x_i of the reference's logistic-regression
 * and SVM workers (app/logistic_regression.cpp:441-446), an embedding bag --
 * computed in the shard, so the reply holds nbags * W values, not n * W.
 *   - any dtype, any width (1 included), either creation mode; the dense
 *     parameter array is the only source (no optimizer state, no overflow
 *     table); the call counts in n_get_calls;
 *   - everything is computed in the shard's value type T.  weights == NULL:
 *     every weight is one and nothing is multiplied.  The sum of an empty bag
 *     is +0; the sum of one term is that term (a bag of one key with NULL
 *     weights equals pskv_get of the key bit for bit); a longer bag's
 *     additions run in an order that is a function of the bag's LENGTH alone
 *     (key order; a bag of more than 256 keys in chunks of 256 whose partial
 *     sums are added in chunk order), never of the launch, the alignment, an
 *     option or timing, and there are no atomics: the same call on the same
 *     contents returns the same bits.  Each multiply-add is one fused
 *     operation.  PSKV_I32: int32 weights, two's complement with wrap;
 *   - keys outside [key_begin, key_end) follow pskv_apply's rule at every
 *     width: a host call returns PSKV_EINVAL naming the first and writes
 *     nothing; a device call counts such a key as a row of zeros and the next
 *     pskv_sync returns PSKV_ESTATE (pskv_clear resets it).  This holds at
 *     width 1 too, where pskv_get would have served the key from the overflow
 *     table;
 *   - flags, null pointers with a non-zero count and a host call's offsets
 *     (offsets[0] == 0, non-decreasing, offsets[nbags] == n) are checked
 *     before the handle is looked at: PSKV_EINVAL naming the first bad bag,
 *     also for a null shard.  nbags == 0 is a successful call that does
 *     nothing more; n == 0 with nbags > 0 writes zeros;
 *   - device offsets cannot be read by the library: the kernels clamp bag b
 *     to [min(o_b, n), min(max(o_b+1, o_b), n)), so malformed device offsets
 *     give unspecified values and never an access outside keys, weights, out;
 *   - PSKV_HOST_FRAME buffers are treated as plain host memory; a host call is
 *     synchronous, a device call stream-ordered, as pskv_get; with the
 *     resident request server (SERVE = 1) the call first ends the server;
 *   - not provided: a grouped form, mean or max pooling (weights give the
 *     mean), overflow keys.  The backward pass is the pooled push below.
 *
 * Pooled pushes (pskv_apply_pooled): the backward half of a
 * pooled pull.  The caller sends one gradient row per BAG (the reference's
 * err_s, app/logistic_regression.cpp:451-456; an embedding bag's output
 * gradient) and the per-key weights of the pull; the shard forms each key
 * position's gradient row itself,
 *     rows[i] = weights[i] * bag_grads[bag(i)],   offsets[bag(i)] <= i < offsets[bag(i)+1]
 * in registers inside the optimizer step, so the push holds nbags * W values,
 * not n * W.
 *   - one call is one step, the step pskv_apply(keys, rows, n) would make
 *     ("Optimizer steps", "Momentum and Adam"): the rows of all occurrences of
 *     a key are summed in unspecified order, the shard's rule is applied once
 *     per distinct key, every other key keeps p and state bit for bit.  A key
 *     whose weight or whose bag's row is zero is still a key of the call and
 *     takes a step with that zero contribution (weight decay, momentum and
 *     Adam decay act on it), as a zero gradient row does in pskv_apply;
 *   - arithmetic in the shard's type T: each product is ONE multiplication
 *     rounded to T (never contracted with the addition behind it);
 *     weights == NULL: the term is the bag's row itself, bit for bit; the rest
 *     is pskv_apply's expression.  When every key of the call is distinct the
 *     result (p, every state slot) equals pskv_apply of the rows
 *     fl_T(weights[i] * bag_grads[...]) bit for bit; with duplicated keys the
 *     sums differ from it by their order only;
 *   - float shards only (PSKV_I32: PSKV_EINVAL), any width (1 included),
 *     either creation mode; a shard without an optimizer: PSKV_EINVAL;
 *   - the step counter follows pskv_apply's rules: a call that queues work
 *     advances it by one; n == 0 (whatever nbags) or nbags == 0 does nothing,
 *     returns PSKV_OK and does not advance it; a refused call does not; a
 *     device call that drops out-of-range keys does;
 *   - flags, null keys / offsets / bag_grads with a non-zero count, n > 2^31
 *     (a pooled push is one launch group: PSKV_EINVAL) and a host call's
 *     offsets (as a pooled pull's) are checked before the handle is looked
 *     at: PSKV_EINVAL naming the first bad bag, also for a null shard;
 *   - keys outside [key_begin, key_end) follow pskv_apply's rule at every
 *     width: a host call returns PSKV_EINVAL naming the first and applies
 *     nothing; a device call applies the in-range keys, drops the others and
 *     the next pskv_sync returns PSKV_ESTATE (pskv_clear resets it);
 *   - device offsets cannot be read by the library: the kernels take for
 *     position i a bag index that is always below nbags, so malformed device
 *     offsets give unspecified values to the keys of the call, never an access
 *     outside keys, weights, offsets[0..nbags], bag_grads[0 .. nbags*W), and
 *     never a change to a key that is not in `keys`;
 *   - PSKV_HOST_FRAME buffers are treated as plain host memory; a host call
 *     returns as a host pskv_apply does (once its copies are queued), a device
 *     call is stream-ordered; with the resident request server (SERVE = 1)
 *     the call first ends the server;
 *   - timing: one operation of pskv_apply_time's slot (PSKV_TIME_APPLY), with
 *     elements = n;
 *   - not provided: an accumulate-mode pskv_add counterpart,
 *     int32, slicing inside KVClientTable (a worker of a range-partitioned
 *     table sends each server its part of every bag with the bag's full
 *     gradient row).
 *
 * Grouped pooled pushes (pskv_apply_pooled_grouped): the pooled
 * pushes of several workers as one step, as pskv_apply_grouped is to
 * pskv_apply (a BSP flush is one step over the summed minibatch gradient).
 *   - the call is the ONE step pskv_apply_pooled would make of the
 *     concatenation of the batches: keys, weights and bag rows back to back,
 *     each batch's offsets shifted by the keys before it.  Occurrences of a
 *     key in any batch are summed in unspecified order, the rule is applied
 *     once per distinct key, every other key keeps p and its state bit for bit;
 *   - the step counter advances by one per call that queues work, however
 *     many batches or launch groups (32 batches, fewer than 2^32 keys each)
 *     the call has; every launch group uses the same t;
 *   - each product is one multiplication rounded to T, as in
 *     pskv_apply_pooled; a batch with weights == NULL beside weighted batches
 *     contributes its bag rows bit for bit.  When every key of the whole call
 *     is distinct, p and every state slot equal, bit for bit,
 *     pskv_apply_pooled of the concatenation and pskv_apply_grouped of the
 *     host-expanded rows fl_T(w_i * bg);
 *   - a batch with n == 0 or nbags == 0 contributes nothing; a call of such
 *     batches only, or nb == 0, returns PSKV_OK, queues nothing and leaves
 *     the step counter alone;
 *   - checked before the handle is looked at: flags as for
 *     pskv_apply_pooled; null batches with nb > 0; per batch the null
 *     pointers, n > 2^31 and a host call's offsets as pskv_apply_pooled
 *     checks them: PSKV_EINVAL naming the BATCH and the first bad bag;
 *   - with the handle: float shards with an optimizer only; a host call that
 *     holds a key outside [key_begin, key_end) returns PSKV_EINVAL naming the
 *     batch and the key and applies nothing; a device call drops such keys and
 *     the next pskv_sync returns PSKV_ESTATE; SERVE = 1 is ended first;
 *   - malformed device offsets in any batch give unspecified values to the
 *     keys of the call, never an access outside that batch's arrays and never
 *     a change to a key that is not in the call;
 *   - a host call returns as a host pskv_apply does; timing: PSKV_TIME_APPLY's
 *     slot, one operation per launch group, elements = the sum of n;
 *   - not provided: a grouped pooled PULL (it would save launches only).
 *
 * Sparse shards (pskv_shard_create_sparse): a shard whose memory
 * follows the number of keys it holds, not the span of the key space -- the
 * storage of a server under consistent hashing (a scattered 1/N of the keys),
 * of a table of hashed feature ids or embedding ids.  It owns EVERY uint32 key,
 * 0 and 0xFFFFFFFF included, and holds at most `capacity` distinct keys, W
 * values each, any W (1 included; width 1 runs on the row kernels).  In HBM:
 * the row array, one array of the same shape per optimizer state slot and the
 * stamp array, over capacity slots as a row shard has them over its range, and
 * a hash index from keys to slots (pskv_sparse_info.index_bytes).
 *   - unchanged meaning, stated by relabelling: take any call sequence and any
 *     injective map `rank` from its keys to [0, capacity).  The sparse shard fed
 *     keys K returns what a row shard [0, capacity) of the same dtype, mode,
 *     width and optimizer returns when fed rank(K) -- every call of this
 *     header, and the step counter.  Where the row shard's result is specified
 *     bit for bit (assign; optimizer steps and pooled pushes with distinct keys;
 *     pooled pulls; state round trips) so is the sparse shard's; where a
 *     summation order is left open the same bound holds.  One difference, for a
 *     key that was never written: see "reading calls" below;
 *   - writing calls insert: pskv_add, pskv_add_grouped, the Add half of
 *     pskv_add_get_grouped, pskv_apply, pskv_apply_grouped, pskv_apply_pooled,
 *     pskv_apply_pooled_grouped and pskv_put_state give a key that has no slot
 *     one.  A new key starts with a row of zeros and the optimizer's start state
 *     (init_accum for Adagrad's h and FTRL's n, else 0);
 *   - reading calls never insert: pskv_get, pskv_get_grouped, pskv_get_pooled,
 *     pskv_get_state, pskv_get_state_slot.  A key that is not stored reads as a
 *     row of zeros (the reference's map semantics) from the parameters AND from
 *     every state array (where a row shard's untouched key shows init_accum);
 *     in a pooled pull, from device buffers too, it is legal and sets no error;
 *   - no key is refused: the host-side refusal of out-of-range keys does not
 *     apply.  int32, float and double for Add and Get; optimizer steps keep
 *     their float-only rule.  PSKV_SORTED_HINT and PSKV_HOST_FRAME are accepted
 *     and change nothing; the tuning options are accepted and echoed,
 *     pskv_info.resident_bytes is 0;
 *   - a full shard: when a writing call meets a new key and capacity keys are
 *     stored, that key is dropped whole -- every occurrence in the call, every
 *     element of its row -- and the rest of the call is applied; the next
 *     pskv_sync returns PSKV_ESTATE ("sparse shard full"; pskv_clear resets
 *     it), host and device calls alike.  Keys already stored are always served
 *     and count never exceeds capacity; when a call holds more new keys than
 *     there is room for, which of them are dropped is unspecified; the step
 *     counter advances as for a device call that drops keys.  A key dropped
 *     once stays dropped until pskv_clear, pskv_sparse_reserve, a growth or
 *     pskv_sparse_erase (below);
 *   - pskv_info keeps its layout: key_begin 0, key_end 2^32, dense_bytes the
 *     row array (capacity + 1 rows: the last one is the zero row absent keys
 *     read), an empty overflow table.  pskv_dense_ptr returns the row array,
 *     whose row order is unspecified (pskv_sparse_keys lists the keys, pskv_get
 *     reads them);
 *   - pskv_clear empties the index (count 0), zeroes the rows and resets the
 *     state and the step counter; setting or changing an optimizer keeps the
 *     index and follows the rules above for the state;
 *   - timing: the index launches of a call (insert, translate) are one
 *     operation of pskv_index_time's slot (PSKV_TIME_INDEX), elements = keys;
 *   - growth: pskv_sparse_reserve(capacity) makes room for
 *     `capacity` distinct keys.  Checked before the handle: capacity 0 or above
 *     2^31 - 2 is PSKV_EINVAL naming "capacity".  Then: a shard that is not
 *     sparse, a capacity below the current one (no shrinking) or row arrays of
 *     more than 2^46 bytes are PSKV_EINVAL; the current capacity is PSKV_OK and
 *     does nothing.  Otherwise the call runs in stream order behind everything
 *     queued and returns when it is done, as pskv_clear does.  Every stored key
 *     keeps its row and every state slot bit for bit; count, the step counter,
 *     the optimizer configuration and the options are unchanged; capacity is
 *     the new value and table_slots = max(16, next_pow2(2 * capacity)).  Every
 *     new array is allocated before anything is given up: PSKV_ENOMEM leaves the
 *     shard exactly as it was.  A successful growing call clears the "sparse
 *     shard full" condition: keys dropped earlier are forgotten and a later
 *     writing call may insert them (the data they were pushed with is lost).
 *     pskv_dense_ptr and pskv_shard_info.dense_bytes CHANGE with every growth
 *     and every erase: a pointer taken before is dangling afterwards;
 *   - automatic growth: pskv_sparse_set_growth(max_capacity) lets the writing
 *     calls listed above grow the shard themselves.  max_capacity is 0 (fixed,
 *     the default) or lies in [current capacity, 2^31 - 2] with row arrays of at
 *     most 2^46 bytes at that size; anything else is PSKV_EINVAL, the range
 *     check coming before the handle.  With a limit, a writing call first
 *     looks at count, the keys stored after everything queued, and at n, its
 *     key positions (all batches of a grouped call), and grows iff
 *     count + n > capacity, to min(max_capacity, max(2 * capacity, count + n)),
 *     before its first key is inserted.  The capacities a shard goes through so
 *     depend on the call sequence alone, never on timing, and a key is dropped
 *     only when the distinct stored keys would exceed max_capacity, exactly as
 *     at a fixed shard of that capacity.  The library keeps a host-side upper
 *     bound of count (the count at its last read-back plus the key positions of
 *     every writing call since) and reads the true count, one bounded stream
 *     wait, only when bound + n > capacity; a call that does not grow so queues
 *     its work as before.  A call that GROWS waits for the shard's stream, a
 *     device call too, and therefore cannot be captured into a graph: reserve
 *     beforehand where calls are captured.  pskv_sparse_reserve beyond the limit
 *     raises the limit to the new capacity.  pskv_sparse_get_growth returns the
 *     limit and the number of rebuilds done so far (reserve, automatic growth
 *     and erase each count one);
 *   - erase: pskv_sparse_erase(keys, n, flags) forgets keys: their slots are
 *     freed, their rows and optimizer state are gone.  Checked before the
 *     handle: flags other than PSKV_HOST / PSKV_DEVICE, null keys with n > 0.
 *     n == 0 is PSKV_OK and does nothing at all.  Keys that are not stored and
 *     keys listed twice are legal and set no error; the call never inserts.  It
 *     runs in stream order and returns when done.  Afterwards an erased key is
 *     not stored: it reads a zero row from the parameters and from every state
 *     array, is absent from pskv_sparse_keys, and count has dropped by the
 *     number of distinct stored keys erased.  Every other stored key keeps its
 *     row and every state slot bit for bit.  A later writing call that names an
 *     erased key inserts it as a new key (a zero row, the optimizer's start
 *     state), and freed slots are usable again: at a full shard, erasing k
 *     stored keys makes room for exactly k new ones.  Capacity, the step
 *     counter and the configuration are unchanged; the full condition is
 *     cleared and dropped keys are forgotten, as for reserve.  By relabelling:
 *     on the row-shard twin an erase is an assign Add of zero rows plus
 *     pskv_put_state of the start values at rank(K), after which rank may be
 *     re-drawn for those keys.  This is a MAINTENANCE call: it rebuilds the
 *     index and moves every surviving row, so its cost follows the keys stored,
 *     not n, and it holds a second set of row arrays while it runs
 *     (PSKV_ENOMEM leaves the shard as it was);
 *   - the launches of a growth or an erase are counted in no pskv_*_time slot;
 *   - not provided: shrinking; growth requested from the device without a host
 *     step; eviction policies such as LRU or "erase zero rows" (a caller builds
 *     them from pskv_sparse_keys, pskv_get and pskv_sparse_erase); an erase
 *     whose cost follows n (tombstones and a free list); 64-bit keys; a sparse
 *     scalar fast path (the resident request server and inline messages serve
 *     scalar range shards only).
 *
 * Threading: one shard handle is used by one host thread at a time (the
 * reference calls a storage only from its ServerThread, server_thread.cpp:20-50);
 * distinct handles may be used concurrently.  Every call selects the shard's
 * device itself, so construction and use may happen on different threads
 * (Engine::CreateTable constructs storages on the engine thread,
 * driver/engine.hpp:100-109).
 *
 * Errors: every function returns 0 on success and a negative PSKV_E* code on
 * failure; pskv_last_error() returns this thread's message for the last
 * failure.  The C++ HipStorage adaptor (include/ps/hip_storage.hpp) turns a
 * non-zero status into an abort, keeping the reference's glog CHECK convention
 * (abstract_storage.hpp:15,20; map_storage.hpp:20).
 */
#ifndef PSKV_H_
#define PSKV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSKV_ABI_VERSION 1

/* status codes */
#define PSKV_OK 0
#define PSKV_EINVAL (-1)   /* bad argument (null pointer, bad dtype, n mismatch ...) */
#define PSKV_EHIP (-2)     /* a HIP runtime call failed */
#define PSKV_ENOMEM (-3)   /* device or pinned allocation failed */
#define PSKV_ESTATE (-4)   /* sticky device-side error (overflow table exhausted) */

/* value types used by the reference (driver/engine.cpp:254,261; apps use double) */
enum pskv_dtype { PSKV_I32 = 0, PSKV_F32 = 1, PSKV_F64 = 2 };

/* update semantics */
enum pskv_mode {
  PSKV_ASSIGN = 0,     /* reference: last write wins (drop-in default) */
  PSKV_ACCUMULATE = 1  /* north star: scatter-accumulate (gradient reduction) */
};

/* call flags */
#define PSKV_HOST 0x0        /* keys/vals/out are host memory (the zmq buffers of comm/mailbox.cpp) */
#define PSKV_DEVICE 0x1      /* keys/vals/out are device memory on the shard's device */
#define PSKV_SORTED_HINT 0x2 /* caller believes keys are non-decreasing: take the sorted path.
                                The kernel verifies the claim and repairs the result on the
                                device if it was wrong, so a wrong hint costs time, never
                                correctness.  What it costs: the group is replayed in call
                                order by ONE workgroup (K4r), ~1 GB/s of keys and values --
                                64 M 4-byte keys take ~0.3 s -- on top of the sorted pass. */
#define PSKV_HOST_FRAME 0x4  /* host keys/vals/out that lie in pskv_host_alloc frames are
                                BORROWED until pskv_host_free: the call reads and writes them
                                in place (no staging copy) and an Add returns once its work
                                is queued, without waiting for it.  The caller must not
                                modify such a frame before freeing it; pskv_host_free holds
                                it back from reuse until every queued call that reads it has
                                run.  Host pointers outside frames ignore the flag. */
/* Any other flag bit, or PSKV_HOST_FRAME together with PSKV_DEVICE, is
 * rejected with PSKV_EINVAL (the call does nothing). */

typedef struct pskv_shard pskv_shard;

/* One push or pull batch of a grouped call.  For an Add `vals` is read
 * (n values), for a Get `vals` is the output (n values). */
typedef struct pskv_batch {
  const uint32_t* keys;
  void* vals;
  uint64_t n;
} pskv_batch;

typedef struct pskv_info {
  int device;
  int dtype;
  int mode;
  int value_bytes;
  uint32_t key_begin;
  uint64_t key_end;          /* exclusive, may be 2^32 */
  uint64_t dense_bytes;      /* HBM held by the dense parameter array (keys * width * value_bytes) */
  uint64_t overflow_capacity;/* slots of the overflow hash table */
  uint64_t overflow_count;   /* keys stored in the overflow table (as of the last sync) */
  uint64_t n_add_calls;
  uint64_t n_get_calls;
  uint64_t n_sorted_launches;   /* sorted-path kernel launches */
  uint64_t n_general_launches;  /* general (dedup) path launches, repairs included */
  uint64_t resident_bytes;      /* the effective resident window (option RESIDENT_BYTES), 0 = none */
} pskv_info;

/* Kernel ids for pskv_kernel_time. */
enum pskv_kernel {
  PSKV_K_GATHER = 0,        /* K1: gather (Get) */
  PSKV_K_ASSIGN_SORTED = 1, /* K2: sorted last-wins scatter (single batch) */
  PSKV_K_ASSIGN_TILES = 2,  /* K2g: grouped sorted scatter, key-tile owner */
  PSKV_K_GENERAL_MARK = 3,  /* K4a: chunk dedup + stamps / accumulate */
  PSKV_K_GENERAL_COMMIT = 4,/* K4b: winner write */
  PSKV_K_RADIX = 5,         /* K5a-d: radix-bucket general Add (timed as one operation) */
  PSKV_K_DENSE_CHECK = 6,   /* K6: accumulate, prove the batches dense windows */
  PSKV_K_ACC_DENSE = 7,     /* K7: accumulate dense windows, one RMW per key */
  PSKV_K_INLINE_ADD = 8,    /* K8: small host Add carried in the kernel arguments */
  PSKV_K_INLINE_GET = 9,    /* K8: small host Get, reply written to page-locked memory */
  PSKV_K_REPLAY = 10,       /* K4r: conditional replay behind a verifying sorted-path group */
  PSKV_K_ROW_GATHER = 11,   /* row shard Get */
  PSKV_K_ROW_COMMIT = 12,   /* row shard assign Add: K4a stamps on the keys + whole-row winner copy */
  PSKV_K_ROW_ACCUMULATE = 13, /* row shard accumulate Add: one atomic add per element */
  PSKV_K_COUNT = 14
};

/* Create a shard owning keys [key_begin, key_end) on `device`.  The dense
 * array ((key_end-key_begin) values) is allocated in HBM and zero-filled.
 * key_end may be 2^32 (the whole key space: 17.2 GB for float). */
int pskv_shard_create(int device, uint32_t key_begin, uint64_t key_end, int dtype, int mode,
                      pskv_shard** out);
/* As pskv_shard_create, with an explicit overflow-table capacity (slots, rounded
 * up to a power of two; 0 = default). */
int pskv_shard_create_ex(int device, uint32_t key_begin, uint64_t key_end, int dtype, int mode,
                         uint64_t overflow_slots, pskv_shard** out);
#define PSKV_MAX_WIDTH 4096
/* As pskv_shard_create_ex, with `width` values per key (a row).  width == 1 is
 * exactly pskv_shard_create_ex.  width 0, width > PSKV_MAX_WIDTH or a dense
 * array of more than 2^46 bytes is PSKV_EINVAL. */
int pskv_shard_create_rows(int device, uint32_t key_begin, uint64_t key_end, int dtype, int mode,
                           uint32_t width, uint64_t overflow_slots, pskv_shard** out);
/* Values per key of this shard (1 for every shard made by the older
 * constructors); 0 for a null shard. */
uint32_t pskv_shard_width(pskv_shard* s);
/* A sparse shard (semantics: the header comment, "Sparse shards"): it owns
 * every uint32 key and holds at most `capacity` distinct keys, `width` values
 * each; its memory follows capacity, not the key space.  Validated before the
 * device is looked at, PSKV_EINVAL naming the field: capacity 0 or above
 * 2^31 - 2, width 0 or above PSKV_MAX_WIDTH, a bad dtype or mode, row arrays
 * of more than 2^46 bytes. */
int pskv_shard_create_sparse(int device, uint64_t capacity, int dtype, int mode, uint32_t width,
                             pskv_shard** out);
typedef struct pskv_sparse_info {
  uint32_t size;          /* sizeof(pskv_sparse_info); any other value is PSKV_EINVAL naming "size" */
  uint64_t capacity;      /* distinct keys the shard can hold */
  uint64_t count;         /* distinct keys held, after everything queued so far */
  uint64_t table_slots;   /* entries of the hash index (a power of two, >= 2 * capacity) */
  uint64_t index_bytes;   /* HBM held by the index beyond the row arrays */
} pskv_sparse_info;
/* Waits for the shard's stream.  PSKV_EINVAL for a shard that is not sparse. */
int pskv_sparse_info_get(pskv_shard* s, pskv_sparse_info* out);
/* The stored keys, in unspecified order: at most cap of them into out (host
 * memory, or device memory with PSKV_DEVICE), *n = the number stored (it may
 * exceed cap: nothing past cap is written).  Waits for the shard's stream. */
int pskv_sparse_keys(pskv_shard* s, uint32_t* out, uint64_t cap, uint64_t* n, int flags);
/* Growth and erase of a sparse shard (semantics: the header comment, "Sparse
 * shards").  Grow to hold `capacity` distinct keys; returns when done. */
int pskv_sparse_reserve(pskv_shard* s, uint64_t capacity);
/* Let writing calls grow the shard themselves, up to max_capacity (0 = fixed,
 * the default).  A call that grows waits for the shard's stream. */
int pskv_sparse_set_growth(pskv_shard* s, uint64_t max_capacity);
/* The limit and the rebuilds done so far; either output may be null. */
int pskv_sparse_get_growth(pskv_shard* s, uint64_t* max_capacity, uint64_t* rebuilds);
/* Forget keys (host memory, or device memory with PSKV_DEVICE): their slots
 * are freed, their rows and optimizer state are gone.  A maintenance call whose
 * cost follows the keys stored; returns when done. */
int pskv_sparse_erase(pskv_shard* s, const uint32_t* keys, uint64_t n, int flags);
int pskv_shard_destroy(pskv_shard* s);

/* Push: apply n (key, value) pairs.  Asynchronous on the shard's stream for
 * PSKV_DEVICE inputs (the caller keeps them alive until the stream passes the
 * call); host inputs are staged before return and may be reused immediately.
 * A host Add of at most 256 keys in all (grouped: summed over its batches)
 * travels inside the kernel arguments and returns once the launch is
 * enqueued; a host Get of at most 1024 keys likewise, 512 keys per launch,
 * its reply written by the kernels into page-locked memory (PSKV_INLINE=0
 * disables; PSKV_SERVE=1 sends them to a resident request-server kernel
 * instead).  Larger pageable host Adds below 32 MiB are copied
 * into pinned staging and return once the copy is queued for DMA. */
int pskv_add(pskv_shard* s, const uint32_t* keys, const void* vals, uint64_t n, int flags);
/* Pull: out[i] = value of keys[i] (0 if never written).  Synchronous for host
 * `out` (PSKV_HOST), stream-ordered for device `out` (PSKV_DEVICE). */
int pskv_get(pskv_shard* s, const uint32_t* keys, uint64_t n, void* out, int flags);

/* Pooled pull (semantics: the header comment, "Pooled pulls"):
 * out[b*W + j] = sum over i in [offsets[b], offsets[b+1]) of weights[i] * row(keys[i])[j].
 * keys: n keys, bag after bag; weights: n values of the shard's type, or NULL
 * (every weight one); offsets: nbags + 1 values; out: nbags * W values.
 * Synchronous for host buffers, stream-ordered for PSKV_DEVICE ones. */
int pskv_get_pooled(pskv_shard* s, const uint32_t* keys, uint64_t n, const void* weights,
                    const uint64_t* offsets, uint64_t nbags, void* out, int flags);

/* Pooled push: one optimizer step (semantics: "Optimizer steps", "Momentum and Adam",
 * "Pooled pushes") whose gradient row for key position i is
 * weights[i] * bag_grads[bag(i)], bag(i) the bag b with
 * offsets[b] <= i < offsets[b+1].  keys: n keys, bag after bag; weights: n values of the shard's
 * type or NULL (every weight one, nothing is multiplied); offsets: nbags + 1 values;
 * bag_grads: nbags * W values, row b at element b * W. */
int pskv_apply_pooled(pskv_shard* s, const uint32_t* keys, uint64_t n, const void* weights,
                      const uint64_t* offsets, uint64_t nbags, const void* bag_grads, int flags);

/* Grouped pooled push (semantics: "Grouped pooled pushes"): ONE optimizer step
 * from the pooled pushes of nb workers, the step pskv_apply_pooled would make
 * of their concatenation.  Each batch holds the arguments of one
 * pskv_apply_pooled call. */
typedef struct pskv_pool_batch {
  const uint32_t* keys;      /* n keys, bag after bag */
  const void* weights;       /* n values of the shard's type, or NULL (every weight one) */
  const uint64_t* offsets;   /* nbags + 1 */
  const void* bag_grads;     /* nbags * W values */
  uint64_t n, nbags;
} pskv_pool_batch;
int pskv_apply_pooled_grouped(pskv_shard* s, const pskv_pool_batch* batches, uint64_t nb, int flags);

/* Grouped forms: nb batches in one call, semantically identical to nb
 * consecutive pskv_add / pskv_get calls in array order, executed in a small,
 * fixed number of kernel launches. */
int pskv_add_grouped(pskv_shard* s, const pskv_batch* batches, uint64_t nb, int flags);
int pskv_get_grouped(pskv_shard* s, const pskv_batch* batches, uint64_t nb, int flags);
/* pskv_add_grouped(adds) then pskv_get_grouped(gets) in one call (flags as
 * for both; PSKV_SORTED_HINT applies to the Adds): the BSP model's flush of
 * its deferred Adds followed by the Gets that flush releases
 * (server/consistency/bsp_model.cpp:14-31), or one worker round's push then
 * pull.  Identical results to the two calls.  Device batches, assign mode,
 * 4-byte values: the Add's conditional replay (K4r) rides on the Get's first
 * K1 launch (K1r), one launch fewer than the two calls (option FOLD_REPLAY).
 * (A single fused launch for the pair was built and measured slower than the
 * two launches) */
int pskv_add_get_grouped(pskv_shard* s, const pskv_batch* adds, uint64_t na, const pskv_batch* gets,
                         uint64_t ng, int flags);

/* Optimizers (semantics: the header comment, "Optimizer steps"). */
enum pskv_optimizer_kind {
  PSKV_OPT_NONE = 0,
  PSKV_OPT_SGD = 1,
  PSKV_OPT_ADAGRAD = 2,
  PSKV_OPT_MOMENTUM = 3, /* only through pskv_shard_set_optimizer_ex */
  PSKV_OPT_ADAM = 4,     /* only through pskv_shard_set_optimizer_ex */
  PSKV_OPT_FTRL = 5      /* only through pskv_shard_set_optimizer_cfg */
};
typedef struct pskv_optimizer {
  int kind;
  double lr;            /* finite, > 0 */
  double weight_decay;  /* finite, >= 0 */
  double eps;           /* Adagrad: finite, > 0; ignored by SGD */
  double init_accum;    /* Adagrad: finite, >= 0 */
} pskv_optimizer;
/* Give the shard an optimizer, change its hyper-parameters, or (kind
 * PSKV_OPT_NONE) take it away.  The configuration is validated before the
 * handle is looked at: a bad field returns PSKV_EINVAL naming the field, also
 * for a null shard.  The same kind again only changes the hyper-parameters of
 * later calls (they travel by value with each launch, so the change is ordered
 * by the stream; h keeps its contents and a new init_accum only takes effect
 * at the next pskv_clear).  Another kind reallocates the state and resets it
 * to init_accum, in stream order.  The gradient scratch, the accumulator and
 * the stamp array are allocated here, never in pskv_apply; PSKV_ENOMEM leaves
 * the shard as it was. */
int pskv_shard_set_optimizer(pskv_shard* s, const pskv_optimizer* cfg);
/* The current configuration and what the optimizer holds in HBM beyond the
 * dense array: gradient scratch (dense_bytes) + h (dense_bytes, Adagrad only)
 * + the stamp array (8 bytes per key); 0 without an optimizer.  Either output
 * may be null. */
int pskv_shard_get_optimizer(pskv_shard* s, pskv_optimizer* out, uint64_t* state_bytes);
/* One optimizer step from n (key, gradient-row) pairs / from nb batches.
 * Asynchronous for PSKV_DEVICE inputs; host inputs are staged before return. */
int pskv_apply(pskv_shard* s, const uint32_t* keys, const void* grads, uint64_t n, int flags);
int pskv_apply_grouped(pskv_shard* s, const pskv_batch* batches, uint64_t nb, int flags);
/* A Get on Adagrad's accumulator h (flags and paths as pskv_get; a key outside
 * the range reads as zeros): for checkpoints and tests.  PSKV_EINVAL unless
 * the optimizer is PSKV_OPT_ADAGRAD. */
int pskv_get_state(pskv_shard* s, const uint32_t* keys, uint64_t n, void* out, int flags);

/* The extended configuration: every kind, PSKV_OPT_MOMENTUM and PSKV_OPT_ADAM
 * included (rules: the header comment, "Momentum and Adam").  Fields a kind
 * does not use are ignored. */
typedef struct pskv_optimizer_ex {
  uint32_t size;        /* sizeof(pskv_optimizer_ex); any other value is PSKV_EINVAL naming "size" */
  int kind;             /* NONE, SGD, ADAGRAD, MOMENTUM, ADAM */
  double lr;            /* as pskv_optimizer */
  double weight_decay;  /* as pskv_optimizer */
  double eps;           /* ADAGRAD and ADAM: finite, > 0 */
  double init_accum;    /* ADAGRAD: finite, >= 0 */
  double momentum;      /* MOMENTUM: finite, in [0, 1) */
  int nesterov;         /* MOMENTUM: 0 or 1 */
  double beta1, beta2;  /* ADAM: finite, in [0, 1) */
} pskv_optimizer_ex;
/* As pskv_shard_set_optimizer (validated before the handle; the same kind
 * again keeps the state and the step count, another kind resets both; every
 * array is allocated here, PSKV_ENOMEM leaves the shard as it was).  With kind
 * NONE, SGD or ADAGRAD exactly pskv_shard_set_optimizer. */
int pskv_shard_set_optimizer_ex(pskv_shard* s, const pskv_optimizer_ex* cfg);
/* state_bytes: gradient scratch + one dense-sized array per state slot + the
 * stamp array (8 bytes per key).  (pskv_shard_get_optimizer on a shard with a
 * new kind fills the fields it has and reports the new kind number.) */
int pskv_shard_get_optimizer_ex(pskv_shard* s, pskv_optimizer_ex* out, uint64_t* state_bytes);
/* pskv_get_state with a slot number (slots per kind: SGD 0, Adagrad 1,
 * momentum 1, Adam 2, FTRL 2); a slot the kind lacks is PSKV_EINVAL. */
int pskv_get_state_slot(pskv_shard* s, int slot, const uint32_t* keys, uint64_t n, void* out, int flags);
/* Write state rows: a row shard's assign Add aimed at a state array (the last
 * occurrence of a key wins with its whole row; host and device paths as
 * pskv_add on a row shard, at any width, 1 included).  Keys outside the range
 * are refused as pskv_apply refuses them.  For restoring a checkpoint. */
int pskv_put_state(pskv_shard* s, int slot, const uint32_t* keys, const void* vals, uint64_t n, int flags);
/* The configuration that can grow: every kind, PSKV_OPT_FTRL included (rule:
 * the header comment, "FTRL-Proximal").  The first 72 bytes are laid out
 * exactly as pskv_optimizer_ex; fields a kind does not use are ignored. */
typedef struct pskv_optimizer_cfg {
  uint32_t size;        /* sizeof(pskv_optimizer_cfg); any other value is PSKV_EINVAL naming "size" */
  int kind;             /* NONE, SGD, ADAGRAD, MOMENTUM, ADAM, FTRL */
  double lr;            /* as pskv_optimizer */
  double weight_decay;  /* as pskv_optimizer */
  double eps;           /* ADAGRAD and ADAM: finite, > 0 */
  double init_accum;    /* ADAGRAD and FTRL: finite, >= 0 */
  double momentum;      /* MOMENTUM: finite, in [0, 1) */
  int nesterov;         /* MOMENTUM: 0 or 1 */
  double beta1, beta2;  /* ADAM: finite, in [0, 1) */
  double l1, l2;        /* FTRL: finite, >= 0 */
  double ftrl_beta;     /* FTRL: finite, >= 0 (the paper's beta; 1 is its usual value) */
} pskv_optimizer_cfg;
/* As pskv_shard_set_optimizer_ex (validated before the handle, a bad field
 * named also for a null shard; the same kind again keeps the state and the step
 * count, another kind resets both).  With kinds NONE to ADAM exactly
 * pskv_shard_set_optimizer_ex.  The two older setters refuse PSKV_OPT_FTRL. */
int pskv_shard_set_optimizer_cfg(pskv_shard* s, const pskv_optimizer_cfg* cfg);
/* The older getters on an FTRL shard fill the fields they have and report kind 5. */
int pskv_shard_get_optimizer_cfg(pskv_shard* s, pskv_optimizer_cfg* out, uint64_t* state_bytes);
/* The step counter: the number of steps since creation, pskv_clear or a kind
 * change (the next step is t + 1). */
int pskv_get_step(pskv_shard* s, uint64_t* t);
int pskv_set_step(pskv_shard* s, uint64_t t);

/* Wait for the shard's stream, adopt the overflow table as the kernels left
 * it (freeing arrays a device-side growth replaced; trimming its load to
 * <= 1/2), report sticky device errors.  Every host wait of the library (this one, a host
 * Get's, the staging and scratch waits, destroy's) is bounded by the option
 * SYNC_TIMEOUT_MS (default 120000; 0 = unbounded): work that does not complete
 * in time fails the call with PSKV_ESTATE, and pskv_last_error() names the
 * stream or event waited for, the device and the last kernel the shard
 * queued.  Nothing is cancelled or restarted: after a call fails with
 * PSKV_ESTATE its queued work may still read the call's host inputs (a direct
 * DMA from the caller's buffers) or write its host outputs (a Get's values
 * into page-locked memory), so the caller keeps those buffers alive and
 * unmodified until a later pskv_sync succeeds.  (The library's own staging is
 * held back the same way: the next call waits for it, bounded.) */
int pskv_sync(pskv_shard* s);
/* Zero every value (dense array and overflow table); with an optimizer, also
 * reset h to init_accum, the other kinds' state slots to 0 and the step
 * counter to 0. */
int pskv_clear(pskv_shard* s);

/* Run the shard's work on an external hipStream_t (NULL = the shard's own
 * stream, a blocking stream that orders against the legacy default stream). */
int pskv_set_stream(pskv_shard* s, void* hip_stream);
void* pskv_get_stream(pskv_shard* s);
/* Device pointer of the dense array (for zero-copy inspection by tests/benches). */
void* pskv_dense_ptr(pskv_shard* s);
int pskv_shard_info(pskv_shard* s, pskv_info* info);

/* Tuning and path options of one shard, by name (DESIGN.md §5 lists them and
 * what each selects): GENERAL (0 = K4 stamps, 1 = auto, 2 = K5 always),
 * UNROLL, GET_UNROLL (K1's keys per lane: 0 = by launch size, 4, 8), NT, NTP,
 * RESIDENT_BYTES (the resident window, DESIGN.md §7: this many bytes of the
 * dense array from its start are kept in the 256 MiB Infinity Cache -- the
 * dense-window Add (K2g) stores there plainly and the Get (K1 / K1r) loads
 * there plainly, and both reach every other parameter non-temporally, so that
 * nothing displaces the window; -1 = auto, the default: no window for an array
 * of at most 224 MiB, else 224 MiB; 0 = off; a larger value is clamped to the
 * array; pskv_info.resident_bytes reports the effective value.  The budget is
 * one shard's: shards busy on one device at the same time share the cache, and
 * should have the option set explicitly so that their windows together fit
 * it.  Scalar-valued shards only; a workload whose hot keys all lie outside
 * the window is better off with 0),
 * EARLY (K2g early loads: 0 never, 1 always, 2 auto),
 * PAGEABLE_DMA, DMA_MIN_BYTES, DMA_MIN_BYTES_GET,
 * DMA_MIN_BYTES_PINNED, ZC_MAX_BYTES, FRAME_ZC_MAX_BYTES, INLINE,
 * INLINE_ADD_CHUNKS, INLINE_GET_CHUNKS, ISPIN, SERVE, SERVE_IDLE_US,
 * TILE_SHIFT, TILE_GRID, RB_WBITS, RB_NBD, RB_TB, RB_APPLY_LOG2, RB_BIN_BLOCK,
 * SYNC_TIMEOUT_MS (the bound of every host wait, pskv_sync), FOLD_REPLAY
 * (pskv_add_get_grouped: the Add's conditional replay rides on the Get's
 * first K1 launch, K1r, instead of a K4r launch of its own; 1 = on),
 * EPOCH (a test and diagnosis seam: the shard's 32-bit stamp epoch, which
 * advances once per launch group and wraps after 0xFFFFFFFF.  Get returns the
 * current value; set accepts current <= value <= 0xFFFFFFFF, so that the
 * wrap-around can be reached without 2^32 calls -- every stamp and tag on the
 * device is at most the current epoch, so forward is always safe; anything
 * else is PSKV_EINVAL.  It has no environment default).
 * Every option changes speed only, never results.  Some apply only together
 * with others (a value is accepted and echoed either way):
 *   EARLY = 1     K2g with UNROLL 8 and NT 1 (otherwise the default loads)
 *   SERVE = 1     only while the device's hardware queues hold the server
 *                 (DESIGN.md §8); INLINE_*_CHUNKS and ISPIN only on the K8 path
 *   RB_* options  only on the K5 path (unhinted Adds)
 * pskv_set_option returns PSKV_EINVAL for an unknown name or a value out of
 * range (the shard is unchanged).  The environment variable PSKV_<NAME> sets a
 * creation default; an invalid value there is reported on stderr and ignored
 * (the built-in default stays; creation does not fail); so is a retired
 * option's variable (RB_INSERT, GET_DEDUP, GET_NTP, FUSE). */
int pskv_set_option(pskv_shard* s, const char* name, int64_t value);
int pskv_get_option(pskv_shard* s, const char* name, int64_t* value);

/* Per-kernel timing with HIP events on the launch stream (off by default).
 * pskv_set_timing brackets every kernel; pskv_set_timing_mask only the kernels
 * whose bit (1 << pskv_kernel) is set. */
int pskv_set_timing(pskv_shard* s, int enable);
int pskv_set_timing_mask(pskv_shard* s, uint32_t kernel_mask);
int pskv_kernel_time(pskv_shard* s, int kernel, uint64_t* launches, double* total_ms,
                     uint64_t* elements);
int pskv_reset_timing(pskv_shard* s);
/* An optimizer step's launches are timed as ONE operation in a slot of its
 * own, outside enum pskv_kernel: enabled by pskv_set_timing(s, 1) or by this
 * bit of pskv_set_timing_mask, cleared by pskv_reset_timing.  launches counts
 * one operation per launch group (a call of at most 64 batches is one). */
#define PSKV_TIME_APPLY (1u << 14)
int pskv_apply_time(pskv_shard* s, uint64_t* launches, double* total_ms, uint64_t* elements);
/* A pooled pull's launches likewise: one operation per call in a slot of its
 * own; elements counts keys. */
#define PSKV_TIME_POOLED (1u << 15)
int pskv_pooled_time(pskv_shard* s, uint64_t* launches, double* total_ms, uint64_t* elements);
/* A sparse shard's index launches of one call (insert and translate) likewise:
 * one operation per call; elements counts keys. */
#define PSKV_TIME_INDEX (1u << 16)
int pskv_index_time(pskv_shard* s, uint64_t* launches, double* total_ms, uint64_t* elements);

/* Mirror of RangePartitionManager::Slice (base/range_partition_manager.hpp:19-46):
 * walk `keys` once; a key goes to the current range if it lies in it or the
 * current range is the last one, otherwise the range pointer advances.  Emits
 * contiguous slices (range index, first key index, length) in order; at most
 * nranges slices.  Returns the number of slices, or a negative error. */
int pskv_range_slice(const uint64_t* range_begin, const uint64_t* range_end, int nranges,
                     const uint32_t* keys, uint64_t n, int32_t* slice_range,
                     uint64_t* slice_start, uint64_t* slice_len);

/* Bucket of every key under jump consistent hashing over `nbuckets` servers:
 * the bucket function of ConsistentHashingPartitionManager::Slice, the
 * reference Engine's default partitioner
 * (base/consistent_hashing_partition_manager.hpp:18-42,81-89;
 * driver/engine.hpp:143-150).  out_bucket[i] in [0, nbuckets); the slice of key
 * i goes to server_thread_ids[out_bucket[i]].  Host memory, any n. */
int pskv_jump_hash(const uint32_t* keys, uint64_t n, int32_t nbuckets, int32_t* out_bucket);

/* Page-locked host frames for message payloads (the mailbox
 * receives data frames, comm/mailbox.cpp:211-261, into memory the GPU reads
 * directly).  Pooled by power-of-two size class, so steady traffic allocates
 * nothing; thread-safe; usable by every device.  *out is 4 KiB-aligned.  A
 * freed frame whose queued reads (PSKV_HOST_FRAME Adds) have not run yet is
 * held back until they have.  Free frames beyond PSKV_FRAME_CACHE_BYTES
 * (default 1 GiB) are returned to the system. */
int pskv_host_alloc(uint64_t bytes, void** out);
int pskv_host_free(void* p);
/* Bytes held by live frames, by cached free frames, and by freed frames still
 * awaiting their queued reads. */
int pskv_host_pool_stats(uint64_t* live_bytes, uint64_t* cached_bytes, uint64_t* held_bytes);
/* Return every cached free frame to the system (waits for held ones first). */
int pskv_host_pool_trim(void);

const char* pskv_last_error(void);
int pskv_abi_version(void);
/* Number of HIP devices visible (0 when there is no GPU). */
int pskv_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* PSKV_H_ */
