"""Growth and erase of sparse shards (include/pskv.h "Sparse shards", DESIGN.md
§8l): what the tests of pskv_sparse_reserve, pskv_sparse_set_growth and
pskv_sparse_erase share.

  grown_capacity   the growth rule as a pure function: a writing call of n key
                   positions at a shard of `capacity` slots holding `count` keys
                   grows iff count + n > capacity, to min(max, max(2 * capacity,
                   count + n)); max 0 = growth off
  CapacityModel    the rule applied along a call sequence: capacity, the stored
                   key set and the rebuilds a shard must show after each call
  Pair             sparse_util.Twin between a sparse shard that grows by itself
                   and a FIXED sparse shard of ample capacity fed the same keys
                   (work the fixed shard could do before growth existed)
  draw_scenario    the fuzz scenarios of tests/test_sparse_grow_fuzz.py as pure
                   data (no GPU): every call with its keys, the capacity and the
                   count the shard must show behind it, and `order_dependent`
                   for the calls whose result the model cannot fix bit for bit
                   -- duplicated keys in an accumulate Add or in a step.  Those
                   calls, and no others, are left out of the bit-for-bit
                   comparison; comparable_share() is the share that is compared.
"""
import numpy as np

import pooled_push_util as ppu
import sparse_util as su

KEY_LIMIT = 2**31 - 2


def table_slots(capacity):
    return max(16, 1 << (2 * int(capacity) - 1).bit_length())


def grown_capacity(capacity, count, n, max_capacity):
    """The capacity behind a writing call of n key positions (pskv.h)."""
    if not max_capacity or capacity >= max_capacity or count + n <= capacity:
        return capacity
    return min(max_capacity, max(2 * capacity, count + n))


class CapacityModel:
    """Capacity, stored keys and rebuilds along a call sequence.  The scenarios
    that use it never overfill: write() asserts that every new key finds room."""

    def __init__(self, capacity, max_capacity=0):
        self.capacity, self.max, self.stored, self.rebuilds = int(capacity), int(max_capacity), set(), 0

    @property
    def count(self):
        return len(self.stored)

    def room(self):
        """New distinct keys a writing call can still bring."""
        return max(self.capacity, self.max) - self.count

    def write(self, keys):
        keys = [int(k) for k in np.asarray(keys).ravel()]
        if not keys:
            return
        new = grown_capacity(self.capacity, self.count, len(keys), self.max)
        if new != self.capacity:
            self.capacity, self.rebuilds = new, self.rebuilds + 1
        self.stored.update(keys)
        assert self.count <= self.capacity, "the scenario overfills the shard"

    def reserve(self, capacity):
        assert capacity >= self.capacity
        if capacity > self.capacity:
            self.capacity, self.rebuilds = int(capacity), self.rebuilds + 1
            if self.max:
                self.max = max(self.max, self.capacity)

    def set_growth(self, max_capacity):
        assert max_capacity == 0 or max_capacity >= self.capacity
        self.max = int(max_capacity)

    def erase(self, keys):
        keys = [int(k) for k in np.asarray(keys).ravel()]
        if keys:
            self.stored.difference_update(keys)
            self.rebuilds += 1


class Pair(su.Twin):
    """`sp`: a sparse shard of `capacity` slots that may grow to max_capacity;
    `dn`: a fixed sparse shard of fixed_capacity slots.  Both take the raw keys."""

    def __init__(self, ps, capacity, max_capacity, fixed_capacity, dtype, mode, width, rl, cuda):
        self.rl, self.w, self.dt, self.cuda = rl, int(width), np.dtype(dtype), cuda
        self.sp = ps.Shard.sparse(capacity, dtype, mode, width=width, max_capacity=max_capacity)
        self.dn = ps.Shard.sparse(fixed_capacity, dtype, mode, width=width)
        raw = lambda k: np.asarray(k, dtype=np.uint32)  # noqa: E731
        self.shards = ((self.sp, raw), (self.dn, raw))

    def add_get(self, adds, gets, dev=False, what="add_get_grouped"):
        """add_get_grouped of [(keys, vals), ...] and [keys, ...]: the replies, checked equal."""
        def one(sh, f):
            outs = [su_empty(len(q), self.w, self.dt, self.cuda if dev else None) for q in gets]
            sh.add_get_grouped([(self._k(f, k, dev), self._v(v, dev)) for k, v in adds],
                               [(self._k(f, q, dev), o) for q, o in zip(gets, outs)])
            return [su._host(o).reshape(len(q), self.w) for q, o in zip(gets, outs)]
        a, b = self.each(one)
        for x, y in zip(a, b):
            su.same_bits(x, y, what)
        return a


def su_empty(n, w, dt, cuda=None):
    shape = (n, w) if w > 1 else (n,)
    if cuda is None:
        return np.empty(shape, dtype=dt)
    import torch

    from parameter_server_amd.shard import _torch_dtype

    return torch.empty(shape, dtype=_torch_dtype(dt), device=cuda)


# ------------------------------------------------------------------ fuzz scenarios
FUZZ_CAPACITIES = [8, 9, 16, 31, 100, 256]
FUZZ_WIDTHS = [1, 3, 4, 16, 33]
FUZZ_MAX_KEYS = 600  # key positions per call at most
FUZZ_KINDS = ["sgd", "adagrad", "momentum", "nesterov", "adam", "ftrl"]
DUP_SHARE = 0.06  # of the accumulate Adds and the steps: duplicated keys (order-dependent)


def draw_scenario(seed):
    """One scenario as data.  Even seeds: a storage scenario (a mode, any dtype,
    no optimizer); odd seeds: an optimizer scenario (assign, a float dtype, one of
    the six kinds).  calls: dicts with `op`, the keys (as positions of `pool`;
    erase and read calls also name absent keys through `gone`), `dev`, and behind
    every call the `capacity` and `count` the shard must report."""
    rng = np.random.default_rng([seed, 0x5EED])
    storage = seed % 2 == 0
    cap = int(rng.choice(FUZZ_CAPACITIES))
    m = int(rng.integers(cap + 1, 601))  # more keys than the first capacity: the shard has to grow
    sc = {"seed": seed, "kind": "storage" if storage else "optimizer", "capacity": cap, "w": int(rng.choice(FUZZ_WIDTHS)),
          "pool": su.key_pool(rng, m), "calls": []}
    sc["gone"] = su.absent_keys(rng, sc["pool"], 40)
    if storage:
        sc["dtype"] = ["int32", "float32", "float64"][int(rng.integers(0, 3))]
        sc["mode"] = ("assign", "accumulate")[int(rng.integers(0, 2))]
    else:
        sc["dtype"] = ["float32", "float64"][int(rng.integers(0, 2))]
        sc["mode"] = "assign"
        sc["opt"] = FUZZ_KINDS[int(rng.integers(0, len(FUZZ_KINDS)))]
        sc["wd"] = float(rng.choice([0.0, 0.01]))
    slots = 0 if storage else {"sgd": 0, "adagrad": 1, "momentum": 1, "nesterov": 1, "adam": 2, "ftrl": 2}[sc["opt"]]
    cm = CapacityModel(cap, 0)
    # growth comes on early: with it off a scenario can only hold `cap` keys
    script = ["set_growth"] + [None] * int(rng.integers(8, 17))

    def write_positions(dups):
        """Positions of a writing call that fits: stored keys and at most room() new ones."""
        stored = np.flatnonzero(np.isin(sc["pool"], np.array(sorted(cm.stored), dtype=np.uint32)))
        fresh = np.setdiff1d(np.arange(m), stored)
        n_new = int(min(fresh.size, cm.room(), rng.integers(0, FUZZ_MAX_KEYS // 2)))
        n_old = int(min(stored.size, rng.integers(0, FUZZ_MAX_KEYS // 2)))
        pos = np.concatenate([rng.permutation(fresh)[:n_new], rng.permutation(stored)[:n_old]])
        if pos.size == 0:  # never an empty call: a stored key, or the first key of all
            pos = stored[:1] if stored.size else fresh[:1]
        if dups and pos.size:
            pos = np.concatenate([pos, pos[rng.integers(0, pos.size, size=min(pos.size, FUZZ_MAX_KEYS - pos.size))]])
        return rng.permutation(pos)[:FUZZ_MAX_KEYS]

    def cuts(n):
        """2 to 4 batches of a grouped call, an empty one among them."""
        c = np.sort(rng.integers(0, n + 1, size=int(rng.integers(1, 4))))
        return [0] + [int(x) for x in c] + [n]

    def read_keys():
        n = int(rng.integers(1, FUZZ_MAX_KEYS))
        k = sc["pool"][rng.integers(0, m, size=n)]
        hole = rng.random(n) < 0.15
        k[hole] = sc["gone"][rng.integers(0, sc["gone"].size, size=int(hole.sum()))]
        return k

    for forced in script:
        writes = ["add", "add_grouped", "add_get_grouped"] if storage else \
            ["apply", "apply_grouped", "apply_pooled", "apply_pooled_grouped", "put_state", "add"]
        reads = ["get", "get_grouped", "get_pooled"] if storage else ["get", "get_state"]
        op = forced or str(rng.choice(writes * 3 + reads + ["reserve", "set_growth", "erase", "erase", "sync"]))
        if op == "put_state" and not slots:
            op = "apply"
        if op == "get_state" and not slots:
            op = "get"
        call = {"op": op, "dev": bool(rng.integers(0, 2)), "order_dependent": False}
        if op in writes:
            summing = (storage and sc["mode"] == "accumulate") or op.startswith("apply")
            dups = bool(rng.random() < (DUP_SHARE if summing else 0.5)) and op != "put_state"
            pos = write_positions(dups)
            call["keys"] = sc["pool"][pos]
            call["order_dependent"] = bool(summing and np.unique(pos).size != pos.size)
            if "grouped" in op:
                call["cuts"] = cuts(pos.size)
            if "pooled" in op:
                call["bags"] = str(rng.choice(["ones", "eights", "mixed", "one_bag"]))
                call["weighted"] = bool(rng.integers(0, 2))
            if op == "add_get_grouped":
                call["reads"] = [read_keys() for _ in range(int(rng.integers(1, 3)))]
            if op == "put_state":
                call["slot"] = int(rng.integers(0, slots))
            cm.write(call["keys"])
        elif op in reads:
            call["keys"] = read_keys()
            if op == "get_grouped":
                call["cuts"] = cuts(call["keys"].size)
            if op == "get_pooled":
                call["bags"] = str(rng.choice(["ones", "eights", "mixed", "one_bag"]))
                call["weighted"] = bool(rng.integers(0, 2))
            if op == "get_state":
                call["slot"] = int(rng.integers(0, slots))
        elif op == "reserve":
            call["to"] = int(cm.capacity + rng.integers(0, 2 * cm.capacity))
            cm.reserve(call["to"])
        elif op == "set_growth":
            # a limit that leaves room to grow; off only while the shard still has free slots
            call["to"] = 0 if (forced is None and cm.count < cm.capacity and rng.random() < 0.2) \
                else int(max(cm.capacity, m) + rng.integers(0, 64))
            cm.set_growth(call["to"])
        elif op == "erase":
            stored = np.array(sorted(cm.stored), dtype=np.uint32)
            form = int(rng.integers(0, 5))
            take = {0: 1, 1: stored.size // 3, 2: stored.size, 3: stored.size // 2, 4: 0}[form]
            k = rng.permutation(stored)[:take]
            if form == 3 and k.size:  # absent keys and repeats in the list
                k = np.concatenate([k, sc["gone"][:9], k[: k.size // 2 + 1]])
                k = rng.permutation(k)[:FUZZ_MAX_KEYS]
            call["keys"] = k.astype(np.uint32)
            cm.erase(call["keys"])
        call["capacity"], call["count"], call["rebuilds"] = cm.capacity, cm.count, cm.rebuilds
        sc["calls"].append(call)
    return sc


def comparable_share(scenarios):
    """The share of calls that the fuzz compares bit for bit: all but the
    order-dependent ones."""
    calls = [c for sc in scenarios for c in sc["calls"]]
    return sum(not c["order_dependent"] for c in calls) / max(len(calls), 1)


def bag_offsets(call):
    """The bag offsets of a pooled call of the scenario."""
    import pooled_util as pu

    return pu.offsets_of(ppu.bag_lens(call["bags"], len(call["keys"])))
