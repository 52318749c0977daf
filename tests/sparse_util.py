"""Relabelling: how the sparse-shard tests reuse the dense oracles.

A sparse shard (pskv_shard_create_sparse) fed keys K returns what a dense row
shard [0, capacity) of the same dtype, mode, width and optimizer returns when
fed rank(K), for ANY injective map `rank` from the scenario's keys to
[0, capacity) (include/pskv.h, "Sparse shards").  `Relabel` is one such map --
np.unique's order -- so a scenario's keys become row numbers for RowOracle's
accumulate sums, opt_util / ftrl_util's one-step checks and pooled_util's
reference, and for a dense twin shard that runs the same calls.

`key_pool` draws the keys themselves: m distinct uint32 keys from the whole key
space that always hold 0, 2^31 and 0xFFFFFFFF, placed where rows_util's
`range_ends` pattern (first, middle, last element = the range's ends) and
pooled_util.draw_keys (both ends) are sure to use them; `pool_patterns` maps
rows_util.key_patterns over a pool, so every duplicate pattern of the row tests
runs on scattered keys.
"""
import numpy as np

from rows_util import key_patterns

SPECIAL = (0, 2**31, 0xFFFFFFFF)


class Relabel:
    """rank: the scenario's distinct keys -> 0 .. m - 1 (their sorted order)."""

    def __init__(self, *key_arrays):
        allk = np.concatenate([np.asarray(k, dtype=np.uint32).ravel() for k in key_arrays]) if key_arrays \
            else np.empty(0, dtype=np.uint32)
        self.uniq, inv = np.unique(allk, return_inverse=True)
        self.m = int(self.uniq.size)
        self._first = inv  # the ranks of the concatenated inputs (the self-test reads them)

    def rank(self, keys):
        """uint32 ranks of `keys`; every key must be one of the scenario's."""
        keys = np.asarray(keys, dtype=np.uint32)
        r = np.searchsorted(self.uniq, keys)
        ok = (r < self.m) & (self.uniq[np.minimum(r, max(self.m - 1, 0))] == keys) if self.m else np.zeros(keys.shape, bool)
        assert ok.all(), f"{int((~ok).sum())} keys are not part of the scenario"
        return r.astype(np.uint32)

    def holds(self, keys):
        keys = np.asarray(keys, dtype=np.uint32)
        r = np.minimum(np.searchsorted(self.uniq, keys), max(self.m - 1, 0))
        return (self.uniq[r] == keys) if self.m else np.zeros(keys.shape, bool)


def key_pool(rng, m):
    """m distinct uint32 keys: pool[0] = 0, pool[-1] = 0xFFFFFFFF and, from m = 3,
    pool[m // 2] = 2^31; the rest uniform over the key space, unsorted."""
    assert m >= 1
    rest = set()
    while len(rest) < m:
        for k in rng.integers(0, 1 << 32, size=m + 8, dtype=np.uint64):
            if int(k) not in SPECIAL and len(rest) < m:
                rest.add(int(k))
    pool = np.array(sorted(rest), dtype=np.uint64)
    rng.shuffle(pool)
    pool[0] = 0
    if m >= 2:
        pool[-1] = 0xFFFFFFFF
    if m >= 3:
        pool[m // 2] = 2**31
    assert np.unique(pool).size == m
    return pool.astype(np.uint32)


def pool_patterns(rng, n, pool):
    """rows_util.key_patterns over positions of `pool`: name -> n keys."""
    return {name: pool[pos] for name, pos in key_patterns(rng, n, 0, pool.size).items()}


def absent_keys(rng, pool, n):
    """n keys that are not in `pool` (neighbours of its keys among them: a probe
    for key + 1 starts elsewhere, but a wrong match on a truncated key would show)."""
    have = set(int(k) for k in pool)
    out = []
    for k in pool[: n // 2]:
        c = (int(k) + 1) & 0xFFFFFFFF
        if c not in have:
            out.append(c)
            have.add(c)
    while len(out) < n:
        c = int(rng.integers(0, 1 << 32, dtype=np.uint64))
        if c not in have:
            out.append(c)
            have.add(c)
    return np.array(out[:n], dtype=np.uint32)


def self_test():
    rng = np.random.default_rng(5)
    for m in (1, 2, 3, 8, 100, 4100):
        pool = key_pool(rng, m)
        assert pool.dtype == np.uint32 and np.unique(pool).size == m and pool[0] == 0
        if m >= 3:
            assert set(SPECIAL) <= set(int(k) for k in pool)
        a, b = pool[rng.integers(0, m, size=50)], pool[rng.integers(0, m, size=7)]
        rl = Relabel(a, b)
        # injective, onto 0 .. m' - 1, and the same key always gets the same rank
        ra, rb = rl.rank(a), rl.rank(b)
        assert ra.dtype == np.uint32 and rl.m == np.unique(np.concatenate([a, b])).size
        assert np.array_equal(rl.uniq[ra], a) and np.array_equal(rl.uniq[rb], b)
        assert np.array_equal(np.concatenate([ra, rb]), rl._first.astype(np.uint32))
        assert rl.holds(a).all()
        gone = absent_keys(rng, pool, 9)
        assert not np.isin(gone, pool).any() and np.unique(gone).size == 9
        if rl.m:
            assert not rl.holds(gone[~np.isin(gone, rl.uniq)]).any()
        try:
            rl.rank(gone)
        except AssertionError:
            pass
        else:
            raise AssertionError("rank accepted a key outside the scenario")
        for n in (1, 5, 2049):
            for name, keys in pool_patterns(rng, n, pool).items():
                assert keys.size == n and np.isin(keys, pool).all(), name
                if name == "range_ends" and m >= 2 and n > 1:
                    assert keys[0] == 0 and keys[-1] == 0xFFFFFFFF
                if name == "distinct":
                    assert np.unique(keys).size == n
    assert Relabel().m == 0
    return True


# ------------------------------------------------------------------ twin shards
def _dev(x, cuda):
    from test_gpu_parity import tdev

    return tdev(np.ascontiguousarray(x), cuda)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.size == b.size, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    bad = np.flatnonzero(a.reshape(-1).view(u) != b.reshape(-1).view(u))
    assert bad.size == 0, (f"{what}: {bad.size} of {a.size} values differ between the sparse shard and its dense twin, "
                           f"first at {bad[:3].tolist()}: {a.reshape(-1)[bad[0]]!r} vs {b.reshape(-1)[bad[0]]!r}")


class Twin:
    """A sparse shard fed keys and the dense row shard [0, rl.m) fed their ranks:
    every call goes to both, every reply must be the same bits.  (GPU tests;
    keys must be the scenario's, `rl` = Relabel of them.)  dev: through device
    tensors on `cuda`, else host arrays."""

    def __init__(self, ps, capacity, dtype, mode, width, rl, cuda):
        self.rl, self.w, self.dt, self.cuda = rl, int(width), np.dtype(dtype), cuda
        self.sp = ps.Shard.sparse(capacity, dtype, mode, width=width)
        self.dn = ps.Shard(0, max(rl.m, 1), dtype, mode, width=width)
        self.shards = ((self.sp, lambda k: np.asarray(k, dtype=np.uint32)), (self.dn, rl.rank))

    def close(self):
        self.sp.close()
        self.dn.close()

    def _k(self, f, keys, dev):
        k = np.ascontiguousarray(f(keys), dtype=np.uint32)
        return _dev(k, self.cuda) if dev else k

    def _v(self, vals, dev):
        v = np.ascontiguousarray(vals, dtype=self.dt)
        return _dev(v, self.cuda) if dev else v

    def each(self, fn):
        """fn(shard, keymap) on both; returns the two results."""
        return [fn(sh, f) for sh, f in self.shards]

    def write(self, method, keys, vals, dev=False, **kw):
        """add / apply / put_state."""
        self.each(lambda sh, f: getattr(sh, method)(self._k(f, keys, dev), self._v(vals, dev), **kw))

    def write_grouped(self, method, batches, dev=False):
        """add_grouped / apply_grouped of [(keys, vals), ...]."""
        self.each(lambda sh, f: getattr(sh, method)([(self._k(f, k, dev), self._v(v, dev)) for k, v in batches]))

    def read(self, method, keys, dev=False, what="", **kw):
        """get / get_state: the rows, checked equal."""
        a, b = self.each(lambda sh, f: _host(getattr(sh, method)(self._k(f, keys, dev), **kw)).reshape(len(keys), self.w))
        same_bits(a, b, what or method)
        return a

    def _off(self, offsets, dev):
        import torch

        o = np.asarray(offsets)
        return torch.from_numpy(o.astype(np.int64)).to(self.cuda) if dev else o.astype(np.uint64)

    def get_pooled(self, keys, offsets, weights, dev=False, what="get_pooled"):
        w = None if weights is None else self._v(weights, dev)
        a, b = self.each(lambda sh, f: _host(sh.get_pooled(self._k(f, keys, dev), self._off(offsets, dev), w)))
        same_bits(a, b, what)
        return a.reshape(len(offsets) - 1, self.w)

    def _pool_batch(self, f, batch, dev):
        keys, offsets, bag_grads = batch[:3]
        weights = batch[3] if len(batch) == 4 else None
        out = (self._k(f, keys, dev), self._off(offsets, dev), self._v(np.asarray(bag_grads).reshape(-1), dev))
        return out + ((self._v(weights, dev),) if weights is not None else ())

    def apply_pooled(self, keys, offsets, bag_grads, weights=None, dev=False):
        def one(sh, f):
            b = self._pool_batch(f, (keys, offsets, bag_grads) + ((weights,) if weights is not None else ()), dev)
            sh.apply_pooled(b[0], b[1], b[2], b[3] if len(b) == 4 else None)
        self.each(one)

    def apply_pooled_grouped(self, batches, dev=False):
        self.each(lambda sh, f: sh.apply_pooled_grouped([self._pool_batch(f, b, dev) for b in batches]))

    def check_all(self, slots, what="final"):
        """p, every state slot and the step counter of every key of the scenario."""
        self.read("get", self.rl.uniq, what=what + " p")
        for i in range(slots):
            self.read("get_state", self.rl.uniq, what=f"{what} slot {i}", slot=i)
        assert self.sp.step == self.dn.step, (what, self.sp.step, self.dn.step)
        self.sp.sync()
        self.dn.sync()


if __name__ == "__main__":
    self_test()
    print("sparse_util self-test OK")
