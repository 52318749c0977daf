"""The resident window (option RESIDENT_BYTES) selects cache hints
only: K2g's dense mode stores plainly inside the window and non-temporally
outside, K1 / K1r load plainly inside and non-temporally outside.  Whatever the
option is, every result is the oracle's bit for bit.

A 40,000-key shard at key_begin 1000, f32 and f64, with the window's edge at 0
(off), 6 keys (inside the first lane group, not on a 16-byte slot), 8,192 keys
(a K2g chunk edge), 8,192 + 4,098 keys, the whole array, and past the array.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KB, SIZE = 1000, 40_000
RES_KEYS = [0, 6, 8192, 8192 + 4098, SIZE, SIZE + 10_000]
# one group of three dense windows (offset from key_begin, keys): phases 0, 1
# and 3 of a 16-byte slot of f32; the second overlaps the first and the third
# overlaps it too (the later window wins); between them they straddle every
# edge of RES_KEYS inside the array
WINDOWS = [(4_000, 20_000), (20_001, 9_000), (3, 8_192)]
# pulls: both sides of every edge and across it, at phases 0-3; 4 Ki- and 8 Ki-key chunks
PULLS = ([(ph, 8_192) for ph in range(4)] + [(8_192 + ph, 8_192) for ph in range(4)] +
         [(24_000 + ph, 4_096) for ph in range(4)] + [(0, SIZE)])


def tdev(a, cuda):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(cuda)


def bits(x):
    x = np.asarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def assert_bits_equal(got, want, msg):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        raise AssertionError(f"{msg}: {bad.size} mismatches, first at {bad[:5]}")


def window_keys(off, n):
    return np.arange(KB + off, KB + off + n, dtype=np.uint32)


def scattered_keys():
    """An unsorted pull: repeats, keys on both sides of every edge, keys below
    and above the shard's range and keys no push wrote."""
    rng = np.random.default_rng(5)
    q = rng.integers(KB - 50, KB + SIZE + 50, size=6_000).astype(np.uint32)
    q[100:200] = q[0:100]           # repeats
    q[0] = KB + 1                   # never written by WINDOWS
    q[1] = KB + SIZE - 1
    return q


@functools.lru_cache(maxsize=None)
def reference(dtype_name):
    """The pushes and the oracle's answer to every pull, computed once per dtype
    and shared (read only)."""
    import oracle

    dt = np.dtype(dtype_name)
    rng = np.random.default_rng(21)
    batches = [(window_keys(off, n), rng.standard_normal(n).astype(dt)) for off, n in WINDOWS]
    ref = oracle.MapStorageRef(dt)
    for k, v in batches:
        ref.add(k, v)
    pulls = [window_keys(off, n) for off, n in PULLS] + [scattered_keys()]
    want = [ref.get(k) for k in pulls]
    ref.close()
    return batches, pulls, want


@pytest.mark.parametrize("path", ["add_grouped", "add_get_grouped"])
@pytest.mark.parametrize("early", [0, 1])
@pytest.mark.parametrize("res_keys", RES_KEYS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_resident_window_is_bit_exact(cuda, oracle_mod, dtype, res_keys, early, path):
    import torch

    import parameter_server_amd as ps

    dt = np.dtype(dtype)
    batches, pulls, want = reference(dt.name)
    res_bytes = res_keys * dt.itemsize
    with ps.Shard(KB, KB + SIZE, dt, options={"RESIDENT_BYTES": res_bytes, "EARLY": early}) as sh:
        assert sh.get_option("RESIDENT_BYTES") == res_bytes
        assert sh.info()["resident_bytes"] == min(res_bytes, SIZE * dt.itemsize)
        adds = [(tdev(k, cuda), tdev(v, cuda)) for k, v in batches]
        dk = [tdev(k, cuda) for k in pulls]
        tdt = {4: torch.float32, 8: torch.float64}[dt.itemsize]
        for unroll in (4, 8):
            sh.set_option("GET_UNROLL", unroll)
            outs = [torch.empty(k.numel(), dtype=tdt, device=cuda) for k in dk]
            if path == "add_grouped":
                sh.add_grouped(adds, sorted_hint=True)
                sh.get_grouped(list(zip(dk, outs)))
            else:
                sh.add_get_grouped(adds, list(zip(dk, outs)), sorted_hint=True)
            sh.sync()
            for i, (o, w) in enumerate(zip(outs, want)):
                assert_bits_equal(o.cpu().numpy(), w, f"pull {i}, window {res_keys} keys, GET_UNROLL {unroll}")


@pytest.mark.parametrize("path", ["add_grouped", "add_get_grouped"])
@pytest.mark.parametrize("res_keys", [6, 8192 + 4098])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_resident_window_lookalike_is_repaired(cuda, oracle_mod, dtype, res_keys, path):
    """Prior values in the shard and a batch whose endpoints say 'dense window'
    while its keys repeat one key and miss another (5, 6, 6, 8): the sorted pass
    must not write the missing key and the replay repairs the rest, on both
    sides of the window's edge."""
    import torch

    import parameter_server_amd as ps

    dt = np.dtype(dtype)
    rng = np.random.default_rng(31)
    prior = rng.standard_normal(SIZE).astype(dt)
    dense = prior.copy()
    batches = []
    for (off, n), dups in zip(WINDOWS, ([5, 8_190, 8_300, 19_998], [], [6, 4_000])):
        k = window_keys(off, n)
        for i in dups:  # k[i] repeats k[i + 1]: key off + i is missing, the endpoints stay
            k[i] = k[i + 1]
        v = rng.standard_normal(n).astype(dt)
        batches.append((k, v))
        oracle_mod.dense_last_wins(dense, KB, k, v)
    every = window_keys(0, SIZE)
    with ps.Shard(KB, KB + SIZE, dt, options={"RESIDENT_BYTES": res_keys * dt.itemsize}) as sh:
        sh.add(every, prior)
        adds = [(tdev(k, cuda), tdev(v, cuda)) for k, v in batches]
        if path == "add_grouped":
            sh.add_grouped(adds, sorted_hint=True)
            got = sh.get(every)
        else:
            out = torch.empty(SIZE, dtype={4: torch.float32, 8: torch.float64}[dt.itemsize], device=cuda)
            sh.add_get_grouped(adds, [(tdev(every, cuda), out)], sorted_hint=True)
            sh.sync()
            got = out.cpu().numpy()
    assert_bits_equal(got, dense, f"look-alike, window {res_keys} keys")


def test_resident_option_changes_between_calls(cuda, oracle_mod):
    """The option changed between two calls on one shard leaves the results
    unchanged; info() reports the effective value; values out of range raise."""
    import parameter_server_amd as ps
    from parameter_server_amd import PskvError, _lib

    batches, pulls, want = reference("float32")
    dense_bytes = SIZE * 4
    with ps.Shard(KB, KB + SIZE, np.float32) as sh:
        assert sh.info()["resident_bytes"] == 0  # whatever the default: this array is below any budget
        adds = [(tdev(k, cuda), tdev(v, cuda)) for k, v in batches]
        for put, pull in ((0, 4 * 8192), (24, 0), (dense_bytes + 1, 24), (4 * (8192 + 4098), dense_bytes), (-1, -1)):
            sh.set_option("RESIDENT_BYTES", put)
            assert sh.info()["resident_bytes"] == (0 if put < 0 else min(put, dense_bytes))
            sh.add_grouped(adds, sorted_hint=True)
            sh.set_option("RESIDENT_BYTES", pull)
            assert sh.get_option("RESIDENT_BYTES") == pull
            for i, (k, w) in enumerate(zip(pulls, want)):
                assert_bits_equal(sh.get(tdev(k, cuda)).cpu().numpy(), w, f"pull {i}, window {put} then {pull} bytes")
        for bad in (-2, -(1 << 40)):
            with pytest.raises(PskvError) as ei:
                sh.set_option("RESIDENT_BYTES", bad)
            assert ei.value.code == _lib.PSKV_EINVAL
            assert sh.get_option("RESIDENT_BYTES") == -1
    with ps.Shard(0, 1000, np.float32, width=8, options={"RESIDENT_BYTES": 4096}) as sh:
        assert sh.info()["resident_bytes"] == 0  # a row shard has no window (the row kernels ignore it)


def test_resident_auto_rule(cuda):
    """Auto (-1): no window for a dense array of at most the budget (the cache
    holds it anyway), the budget for a larger one."""
    import parameter_server_amd as ps

    budget = 224 << 20
    with ps.Shard(0, budget // 4, np.float32, options={"RESIDENT_BYTES": -1}) as sh:
        assert sh.info()["resident_bytes"] == 0
    with ps.Shard(0, budget // 4 + 4, np.float32, options={"RESIDENT_BYTES": -1}) as sh:
        assert sh.info()["resident_bytes"] == budget
        assert sh.get_option("RESIDENT_BYTES") == -1
        sh.set_option("RESIDENT_BYTES", 0)
        assert sh.info()["resident_bytes"] == 0
