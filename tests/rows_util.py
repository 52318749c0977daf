"""The per-column oracle of row-valued shards, shared by the row tests.

Column j of a width-W shard behaves exactly like the reference storage fed
(keys, vals[:, j]):
  assign      one MapStorageRef (server/map_storage.hpp:17-45 restated) per
              column, bit-exact
  accumulate  oracle.accumulate_ref per column: float64 sums and |v| sums, plus
              the push count m per key, for the bound of tests/test_gpu_parity.py:
                  |gpu - ref64| <= 1.01 (m + 1) u (|p0| + sum|v_i|)
              (p0 = 0: a shard starts, and is cleared to, zeros); int32 exact
              with two's-complement wrap.
"""
import numpy as np

WIDTHS = [1, 2, 3, 4, 5, 16, 33, 64, 100]
LAYOUTS = [(0, 5000), (2**31 - 700, 2**31 + 700)]
U_ROUND = {np.dtype(np.float32): 2.0**-24, np.dtype(np.float64): 2.0**-53}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


class RowOracle:
    def __init__(self, oracle_mod, dtype, mode, width, key_begin, key_end):
        self.o, self.dt, self.mode, self.w = oracle_mod, np.dtype(dtype), mode, int(width)
        self.kb, self.ke = int(key_begin), int(key_end)
        self.clear()

    def clear(self):
        n = self.ke - self.kb
        if self.mode == "assign":
            self.cols = [self.o.MapStorageRef(self.dt) for _ in range(self.w)]
        else:
            self.sum = np.zeros((n, self.w), dtype=np.float64)
            self.abs = np.zeros((n, self.w), dtype=np.float64)
            self.cnt = np.zeros(n, dtype=np.int64)

    def add(self, keys, vals):
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        vals = np.asarray(vals, dtype=self.dt).reshape(keys.size, self.w)
        if keys.size == 0:
            return
        if self.mode == "assign":
            for j, c in enumerate(self.cols):
                c.add(keys, np.ascontiguousarray(vals[:, j]))
            return
        for j in range(self.w):
            self.o.accumulate_ref(self.sum[:, j], self.abs[:, j], self.kb, keys, vals[:, j])
        np.add.at(self.cnt, keys.astype(np.int64) - self.kb, 1)

    def expect(self, keys):
        """Assign / int32: the exact (n, W) rows.  Float accumulate: (ref64, bound)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        if self.mode == "assign":
            out = np.empty((keys.size, self.w), dtype=self.dt)
            for j, c in enumerate(self.cols):
                out[:, j] = c.get(keys)
            return out
        idx = keys.astype(np.int64) - self.kb
        inside = (idx >= 0) & (idx < self.ke - self.kb)
        idx = np.where(inside, idx, 0)
        ref = np.where(inside[:, None], self.sum[idx], 0.0)
        if self.dt == np.int32:
            return (ref.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        bound = 1.01 * (self.cnt[idx][:, None] + 1) * U_ROUND[self.dt] * self.abs[idx]
        return ref, np.where(inside[:, None], bound, 0.0)

    def check(self, keys, got, msg=""):
        got = np.asarray(got).reshape(len(keys), self.w)
        assert got.dtype == self.dt, (got.dtype, self.dt)
        want = self.expect(keys)
        if isinstance(want, tuple):
            ref, bound = want
            err = np.abs(got.astype(np.float64) - ref)
            bad = np.argwhere(~(err <= bound))  # (a NaN fails)
            assert bad.size == 0, (f"{msg}: {len(bad)} elements beyond the bound, first (row, col) {bad[:3].tolist()}: "
                                   f"err {err[tuple(bad[0])]:.3e} bound {bound[tuple(bad[0])]:.3e}")
            return
        g, w = bits(got), bits(want)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{msg}: {len(bad)} elements differ, first (row, col) {bad[:3].tolist()}: "
                                 f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")

    def all_keys(self):
        return np.arange(self.kb, self.ke, dtype=np.int64).astype(np.uint32)


class ValueSource:
    """Values unique per (occurrence, column), so a mixed row or a wrong winner
    cannot compare equal: a running counter, exactly representable in every
    dtype (below 2^24).  Accumulate mode draws random values instead: any
    int32 (the sums wrap), normal floats."""

    def __init__(self, dtype, mode, rng):
        self.dt, self.mode, self.rng, self.next = np.dtype(dtype), mode, rng, 1

    def rows(self, n, w):
        if self.mode == "accumulate":
            if self.dt == np.int32:
                return self.rng.integers(-2**31, 2**31, size=(n, w)).astype(np.int32)
            return (self.rng.standard_normal((n, w)) * 3).astype(self.dt)
        v = (self.next + np.arange(n * w, dtype=np.int64)) % (2**24 - 1) + 1
        self.next += n * w
        return v.reshape(n, w).astype(self.dt)


def key_patterns(rng, n, kb, ke):
    """name -> n keys of [kb, ke).  `distinct` only when the range has n keys."""
    span = ke - kb
    out = {}
    if n <= span:
        out["distinct"] = kb + rng.permutation(span)[:n]
    out["all_equal"] = np.full(n, kb + int(rng.integers(0, span)))
    # duplicates inside one 2048-key chunk: few keys, repeated at once
    out["dups_in_chunk"] = kb + rng.integers(0, min(span, max(1, n // 8 + 1)), size=n)
    # duplicates across chunks: element i repeats element i - per, which lies in
    # another 2048-key chunk once n passes 2048 (per = 1025 at n = 2049, 2051 at 4100)
    per = max(1, min(span, n // 2 + 1))
    out["dups_across_chunks"] = kb + (np.arange(n) % per)
    ends = kb + rng.integers(0, span, size=n)
    ends[0] = kb
    ends[-1] = ke - 1
    if n > 2:
        ends[n // 2] = ke - 1
    out["range_ends"] = ends
    return {k: np.asarray(v, dtype=np.int64).astype(np.uint32) for k, v in out.items()}
