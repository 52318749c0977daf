"""GPU tests of pooled pulls (pskv_get_pooled, Shard.get_pooled): one row per
bag of keys, summed in the shard.  Reference and bound: tests/pooled_util.py
(float64 sums; floats within 1.01 (m + 1) u sum|w_i||p_i|, derived; int32
exact with wrap).  Every case is compared, empty bags included."""
import os
import subprocess

import numpy as np
import pytest

import pooled_util as pu
from rows_util import LAYOUTS, WIDTHS, bits
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.int32, np.float32, np.float64]


def make(kb, ke, dt, w, **kw):
    from parameter_server_amd import Shard

    return Shard(kb, ke, dtype=dt, mode="assign", width=w, **kw)


def weights_for(rng, n, dt, weighted):
    return pu.draw_values(rng, n, dt) if weighted else None


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["low", "straddle"])
def test_pooled_matches_the_reference(cuda, layout, w, dt):
    """Every bag-length pattern, weighted and not, host and device path."""
    kb, ke = layout
    rng = np.random.default_rng(1000 * w + 10 * kb % 97 + np.dtype(dt).itemsize)
    with make(kb, ke, dt, w) as sh:
        p = pu.fill(sh, rng)
        for name, lens in pu.bag_patterns().items():
            off = pu.offsets_of(lens)
            keys = pu.draw_keys(rng, lens, kb, ke)
            for weighted in (False, True):
                wts = weights_for(rng, keys.size, dt, weighted)
                want = pu.reference(p, kb, keys, off, wts)
                for dev in (None, cuda):
                    got = pu.pooled(sh, keys, off, wts, dev)
                    pu.check(got, want, f"{name} weighted={weighted} device={dev is not None}")
        sh.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_pooled_at_max_width(cuda, dt):
    from parameter_server_amd import _lib

    w = _lib.PSKV_MAX_WIDTH
    rng = np.random.default_rng(3)
    with make(10, 40, dt, w) as sh:
        p = pu.fill(sh, rng)
        lens = [5, 0, 9]
        off, keys = pu.offsets_of(lens), pu.draw_keys(rng, lens, 10, 40)
        for weighted in (False, True):
            wts = weights_for(rng, keys.size, dt, weighted)
            want = pu.reference(p, 10, keys, off, wts)
            for dev in (None, cuda):
                pu.check(pu.pooled(sh, keys, off, wts, dev), want, f"max width weighted={weighted}")


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("w", [1, 4, 5])
def test_bag_of_one_key_equals_get_bit_for_bit(cuda, w, dt):
    dt = np.dtype(dt)
    fi = np.finfo(dt)
    special = np.array([-0.0, 0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, fi.max, -fi.max,
                        fi.tiny, 1.0, -3.5], dtype=dt)
    kb, ke = 100, 100 + 4 * special.size
    rng = np.random.default_rng(4)
    with make(kb, ke, dt, w) as sh:
        keys = np.arange(kb, ke, dtype=np.uint32)
        p = rng.permutation(np.resize(special, keys.size * w)).reshape(keys.size, w).astype(dt)
        sh.add(keys, p)
        q = rng.permutation(keys)
        off = pu.offsets_of([1] * q.size)
        want = np.asarray(sh.get(q)).reshape(q.size, w)
        assert np.array_equal(bits(want), bits(pu.rows_of(p, kb, q)))
        for dev in (None, cuda):
            got = pu.pooled(sh, q, off, None, dev)
            assert np.array_equal(bits(got), bits(want)), f"device={dev is not None}"
        dgot = sh.get(tdev(q, cuda)).cpu().numpy().reshape(q.size, w)
        assert np.array_equal(bits(pu.pooled(sh, q, off, None, cuda)), bits(dgot))


def _mixed_call(rng, kb, ke):
    c = pu.CHUNK
    lens = [0, 1, 5, c + 1, 0, 3 * c + 2, 17, c, 2]
    return pu.offsets_of(lens), pu.draw_keys(rng, lens, kb, ke)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_same_call_same_bits(cuda, dt):
    """Twice in a row, and again after unrelated calls; NT 0 and 1; an aligned
    `out` (unit-16 path) and one offset by an element (element path)."""
    kb, ke, w = 0, 3000, 4
    rng = np.random.default_rng(5)
    with make(kb, ke, dt, w) as sh:
        p = pu.fill(sh, rng)
        off, keys = _mixed_call(rng, kb, ke)
        for weighted in (False, True):
            wts = weights_for(rng, keys.size, dt, weighted)
            want = pu.reference(p, kb, keys, off, wts)
            first = pu.pooled(sh, keys, off, wts, cuda)
            pu.check(first, want, "first")
            assert np.array_equal(bits(pu.pooled(sh, keys, off, wts, cuda)), bits(first)), "second call"
            # unrelated calls in between: a Get, another pooled pull, a host pooled pull
            sh.get(tdev(keys[:100], cuda))
            off2, keys2 = _mixed_call(rng, kb, ke)
            pu.pooled(sh, keys2, off2, None, cuda)
            assert np.array_equal(bits(pu.pooled(sh, keys, off, wts, None)), bits(first)), "host path"
            assert np.array_equal(bits(pu.pooled(sh, keys, off, wts, cuda)), bits(first)), "after unrelated calls"
            assert np.array_equal(bits(pu.pooled(sh, keys, off, wts, cuda, out_offset=1)), bits(first)), "element path"
            sh.set_option("NT", 0)
            assert np.array_equal(bits(pu.pooled(sh, keys, off, wts, cuda)), bits(first)), "NT = 0"
            assert np.array_equal(bits(pu.pooled(sh, keys, off, wts, cuda, out_offset=1)), bits(first)), "NT = 0, element"
            sh.set_option("NT", 1)


def test_host_call_refuses_an_out_of_range_key(cuda):
    from parameter_server_amd import PskvError, _lib

    kb, ke = 1000, 2000
    rng = np.random.default_rng(6)
    for w in (1, 3):
        with make(kb, ke, np.float32, w) as sh:
            pu.fill(sh, rng)
            keys = np.array([1000, 1500, 2000, 999, 1999], dtype=np.uint32)
            off = pu.offsets_of([2, 3])
            out = np.full((2, w) if w > 1 else 2, 7.5, dtype=np.float32)
            with pytest.raises(PskvError) as e:
                sh.get_pooled(keys, off, out=out)
            assert e.value.code == _lib.PSKV_EINVAL and "key 2000 " in str(e.value), str(e.value)
            assert (out == 7.5).all()
            sh.sync()  # nothing sticky


@pytest.mark.parametrize("w", [1, 4])
def test_device_call_counts_an_out_of_range_key_as_zeros(cuda, w):
    from parameter_server_amd import PskvError, _lib

    kb, ke = 1000, 2000
    rng = np.random.default_rng(7)
    c = pu.CHUNK
    with make(kb, ke, np.float64, w) as sh:
        p = pu.fill(sh, rng)
        lens = [3, c + 5, 1]
        off, keys = pu.offsets_of(lens), pu.draw_keys(rng, lens, kb, ke)
        keys[1], keys[3 + c + 2], keys[-1] = 2000, 999, 2**32 - 1  # a short bag, a long bag's second chunk, a bag of one
        for weighted in (False, True):
            wts = weights_for(rng, keys.size, np.float64, weighted)
            want = pu.reference(p, kb, keys, off, wts)  # (rows_of: zeros for such keys)
            got = pu.pooled(sh, keys, off, wts, cuda)
            pu.check(got, want, "device call with out-of-range keys")
            assert not got[2].any()
            with pytest.raises(PskvError) as e:
                sh.sync()
            assert e.value.code == _lib.PSKV_ESTATE and "out-of-range" in str(e.value)
            sh.clear()
            sh.sync()
            sh.add(np.arange(kb, ke, dtype=np.uint32), p)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_two_shards_splitting_a_range_add_up(cuda, dt):
    """A range-partitioned table: each shard gets its part of every bag, the
    partial pooled rows add up (the sum is linear)."""
    kb, mid, ke, w = 0, 1300, 3000, 5
    rng = np.random.default_rng(8)
    with make(kb, ke, dt, w) as whole, make(kb, mid, dt, w) as lo, make(mid, ke, dt, w) as hi:
        p = pu.fill(whole, rng)
        allk = np.arange(kb, ke, dtype=np.uint32)
        lo.add(allk[:mid], p[:mid])
        hi.add(allk[mid:], p[mid:])
        off, keys = _mixed_call(rng, kb, ke)
        wts = weights_for(rng, keys.size, dt, True)
        lens = np.diff(off.astype(np.int64))
        bag = np.repeat(np.arange(lens.size), lens)
        want = pu.reference(p, kb, keys, off, wts)
        pu.check(pu.pooled(whole, keys, off, wts, cuda), want, "one shard")
        parts, bounds = [], []
        for sh, sel, base, pp in ((lo, keys < mid, kb, p[:mid]), (hi, keys >= mid, mid, p[mid:])):
            soff = pu.offsets_of(np.bincount(bag[sel], minlength=lens.size))
            got = pu.pooled(sh, keys[sel], soff, wts[sel], cuda)
            part_want = pu.reference(pp, base, keys[sel], soff, wts[sel])
            pu.check(got, part_want, "part")
            parts.append(got)
            bounds.append(part_want[1] if isinstance(part_want, tuple) else None)
            sh.sync()
        if np.dtype(dt) == np.int32:
            total = (parts[0].view(np.uint32) + parts[1].view(np.uint32)).view(np.int32)
            pu.check(total, want, "sum of the parts")
        else:
            total = parts[0].astype(np.float64) + parts[1].astype(np.float64)
            assert (np.abs(total - want[0]) <= bounds[0] + bounds[1]).all()


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_pooled_pull_sees_the_optimizer_steps(cuda, kind):
    kb, ke, w = 0, 600, 4
    rng = np.random.default_rng(9)
    with make(kb, ke, np.float32, w) as sh:
        pu.fill(sh, rng)
        sh.set_optimizer(kind, lr=0.1)
        for _ in range(3):
            k = rng.integers(kb, ke, size=300).astype(np.uint32)
            sh.apply(tdev(k, cuda), tdev(pu.draw_values(rng, (k.size, w), np.float32), cuda))
        allk = np.arange(kb, ke, dtype=np.uint32)
        p = np.asarray(sh.get(allk)).reshape(ke - kb, w)
        off, keys = _mixed_call(rng, kb, ke)
        wts = weights_for(rng, keys.size, np.float32, True)
        want = pu.reference(p, kb, keys, off, wts)
        for dev in (None, cuda):
            pu.check(pu.pooled(sh, keys, off, wts, dev), want, f"after {kind} steps")
        sh.sync()


def test_width_one_with_the_request_server(cuda):
    kb, ke = 0, 4000
    rng = np.random.default_rng(10)
    with make(kb, ke, np.float32, 1, options={"SERVE": 1}) as sh:
        p = pu.fill(sh, rng)
        small = rng.integers(kb, ke, size=20).astype(np.uint32)
        assert np.array_equal(sh.get(small), p[small, 0])  # (a small host Get: the server's)
        off, keys = _mixed_call(rng, kb, ke)
        want = pu.reference(p, kb, keys, off, None)
        for dev in (cuda, None):
            got = pu.pooled(sh, keys, off, None, dev)
            pu.check(got, want, "SERVE = 1")
            assert np.array_equal(sh.get(small), p[small, 0])
        sh.sync()


def test_pooled_time_and_counters(cuda):
    from parameter_server_amd import _lib

    kb, ke, w = 0, 3000, 4
    rng = np.random.default_rng(11)
    with make(kb, ke, np.float32, w) as sh:
        pu.fill(sh, rng)
        sh.sync()
        sh.set_timing(True)
        sh.reset_timing()
        before = {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)}
        gets = sh.info()["n_get_calls"]
        off, keys = _mixed_call(rng, kb, ke)  # long bags: two launches, one operation
        pu.pooled(sh, keys, off, None, cuda)
        pu.pooled(sh, keys[:5], pu.offsets_of([2, 3]), None, cuda)
        sh.get_pooled(np.zeros(0, np.uint32), np.zeros(1, np.uint64))  # no bag: counted, nothing launched
        sh.sync()
        t = sh.pooled_time()
        assert t["launches"] == 2 and t["elements"] == keys.size + 5 and t["total_ms"] > 0, t
        assert sh.info()["n_get_calls"] == gets + 3
        assert {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)} == before
        assert sh.apply_time()["launches"] == 0
        sh.reset_timing()
        assert sh.pooled_time() == {"launches": 0, "total_ms": 0.0, "elements": 0}
        sh.set_timing(True, kernels=[15])  # PSKV_TIME_POOLED's bit alone
        pu.pooled(sh, keys[:5], pu.offsets_of([2, 3]), None, cuda)
        sh.get(tdev(keys[:5], cuda))
        assert sh.pooled_time()["launches"] == 1 and sh.kernel_time(_lib.PSKV_K_ROW_GATHER)["launches"] == 0


def test_no_key_but_bags_writes_zeros(cuda):
    import torch

    with make(0, 100, np.float32, 3) as sh:
        off = pu.offsets_of([0, 0, 0, 0])
        out = np.full((4, 3), 5.0, dtype=np.float32)
        sh.get_pooled(np.zeros(0, np.uint32), off, out=out)
        assert not bits(out).any()
        dout = torch.full((4, 3), 5.0, dtype=torch.float32, device=cuda)
        sh.get_pooled(torch.zeros(0, dtype=torch.int32, device=cuda), torch.from_numpy(off.astype(np.int64)).to(cuda),
                      out=dout)
        assert not bits(dout.cpu().numpy()).any()


def test_cpp_pooled_program(cuda):
    """tests/cpp/hip_storage_pooled_test.cpp: HipStorage::SubGetPooled against
    SubGet plus a host sum, for float, double and int."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_pooled_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
