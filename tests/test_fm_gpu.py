"""GPU tests of the factorization-machine pooled calls (Shard.get_pooled_fm,
Shard.apply_pooled_fm), host and device path, float32 and float64, against the
references and tolerances of tests/fm_util.py."""
import os
import subprocess

import numpy as np
import pytest

import fm_util as fu
import opt_util as ou
from rows_util import bits
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
KB = 7  # the first key of the row shards


def make(rows, dt, w, kind=None):
    import parameter_server_amd as ps

    sh = ps.Shard(KB, KB + rows, dt, width=w)
    if kind:
        fu.set_optimizer(sh, kind)
    return sh


def all_keys(rows):
    return np.arange(KB, KB + rows, dtype=np.uint32)


def dev(a, cuda):
    if cuda is None or a is None:
        return a
    return tdev(a.astype(np.int64) if a.dtype == np.uint64 else a, cuda)


def host(x):
    return None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())


def pull(sh, keys, off, wts, cuda, want_sum=True):
    s, pair = sh.get_pooled_fm(dev(keys, cuda), dev(off, cuda), dev(wts, cuda), want_sum=want_sum)
    return host(s), host(pair)


def push(sh, keys, off, c, wts, bg, cuda):
    sh.apply_pooled_fm(dev(keys, cuda), dev(off, cuda), dev(c, cuda), dev(wts, cuda), dev(bg, cuda))


def same_bits(a, b, msg):
    assert np.array_equal(bits(a), bits(b)), f"{msg}: {int((bits(a) != bits(b)).sum())} elements differ"


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w", [1, 3, 4, 16, 33, 100, 1024])
def test_pull_meets_the_float64_reference(cuda, w, device, dt):
    dt = np.dtype(dt)
    rows = 300
    lens = np.array([0, 1, 2, 3, 5, 256, 257, 600])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rng = np.random.default_rng(ou.case_seed("fm-pull", w, device, dt.name))
    p = rng.standard_normal((rows, w)).astype(dt)
    idx = rng.integers(0, rows, int(lens.sum()))
    keys = (idx + KB).astype(np.uint32)
    path = cuda if device else None
    with make(rows, dt, w) as sh:
        sh.add(all_keys(rows), p)
        for wts in (None, rng.standard_normal(idx.size).astype(dt)):
            _, want, tol = fu.pull_ref(p, idx, off, wts, dt)
            s, pair = pull(sh, keys, off, wts, path)
            err = np.abs(pair.astype(np.float64) - want)
            print(f"w={w} weighted={wts is not None}: err/tol per bag {np.round(err[1:] / tol[1:], 4).tolist()}")
            assert (err <= tol).all(), (err, tol)
            same_bits(s.reshape(-1), host(sh.get_pooled(dev(keys, path), dev(off, path), dev(wts, path))).reshape(-1),
                      "out_sum against get_pooled")
            assert (bits(pair[lens <= 1]) == 0).all(), "a bag of 0 or 1 key: pair is +0"
            s2, pair2 = pull(sh, keys, off, wts, path)
            same_bits(pair, pair2, "the same call twice")
            same_bits(s, s2, "the same call twice, the sums")
            none, pair3 = pull(sh, keys, off, wts, path, want_sum=False)
            assert none is None
            same_bits(pair, pair3, "out_sum = NULL")
        # nbags == 0: a successful call that does nothing; n == 0: zeros to both outputs
        s, pair = pull(sh, keys[:0], off[:1], None, path)
        assert s.size == 0 and pair.size == 0
        s, pair = pull(sh, keys[:0], np.zeros(4, dtype=np.uint64), None, path)
        assert (bits(s) == 0).all() and (bits(pair) == 0).all() and pair.size == 3
        sh.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w", [1, 5, 16, 100])
@pytest.mark.parametrize("kind", ["sgd", "adagrad", "momentum", "adam", "ftrl"])
def test_push_of_distinct_keys_equals_apply_bit_for_bit(cuda, kind, w, device, dt):
    """Four steps on a twin pair; 2100 keys: two virtual workgroups, every row of a bag rewritten by its reader."""
    dt = np.dtype(dt)
    rows, lens = 2200, [2, 3, 9] * 150
    rng = np.random.default_rng(ou.case_seed("fm-twin", kind, w, device, dt.name))
    p0 = rng.standard_normal((rows, w)).astype(dt)
    path = cuda if device else None
    with make(rows, dt, w, kind) as a, make(rows, dt, w, kind) as b:
        for sh in (a, b):
            sh.add(all_keys(rows), p0)
        for t, (weighted, with_grads) in enumerate([(False, False), (True, True), (True, False), (False, True)], 1):
            idx, off, c, wts, bg = fu.draw_push(rng, rows, lens, w, dt, weighted, with_grads, distinct=True)
            keys = (idx + KB).astype(np.uint32)
            S = np.asarray(a.get_pooled(keys, off, wts)).reshape(len(lens), w)
            prow = np.asarray(a.get(keys)).reshape(idx.size, w)
            grads = fu.push_rows(prow, S, np.repeat(np.arange(len(lens)), lens), c, wts, bg)
            assert grads.dtype == dt
            push(a, keys, off, c, wts, bg, path)
            b.apply(dev(keys, path), dev(grads, path))
            assert a.step == b.step == t
            for x, y, name in zip(fu.state(a, all_keys(rows)), fu.state(b, all_keys(rows)), ["p", "slot 0", "slot 1"]):
                same_bits(x, y, f"{name}, step {t} weighted={weighted} bag_grads={with_grads}")
        # no key, or no bag: PSKV_OK, no step
        push(a, keys[:0], np.zeros(4, dtype=np.uint64), c[:3], None, None, path)
        push(a, keys[:0], off[:1], c[:0], None, None, path)
        assert a.step == 4
        a.sync()
        b.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["adagrad", "adam"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_push_of_repeated_keys_reads_every_row_before_the_step(cuda, weighted, kind, device, dt):
    """A key twice inside a bag and in several bags, 2280 positions over 300 rows: fm_util's one-step check."""
    dt = np.dtype(dt)
    rows, w, lens = 300, 5, [3, 2, 9, 1, 0, 4] * 120
    rng = np.random.default_rng(ou.case_seed("fm-dups", weighted, kind, device, dt.name))
    hp = ou.hyper(kind, wd=0.01)
    ks = all_keys(rows)
    with make(rows, dt, w, kind) as sh:
        sh.add(ks, rng.standard_normal((rows, w)).astype(dt))
        for t in range(1, 4):
            idx, off, c, wts, bg = fu.draw_push(rng, rows, lens, w, dt, weighted, t != 2, distinct=False)
            before = fu.state(sh, ks)
            push(sh, (idx + KB).astype(np.uint32), off, c, wts, bg, cuda if device else None)
            after = fu.state(sh, ks)
            pre = fu.push_prepare(before[0], before[1:], idx, off, c, wts, bg, dt, hp, t)
            problems = ou.step_errors(before[0], before[1:], idx, None, after[0], after[1:], dt, hp, t, pre=pre)
            assert not problems, f"step {t}: {problems}"
        sh.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_sparse_shard_equals_the_row_shard_of_its_keys_ranks(cuda, dt):
    import parameter_server_amd as ps

    dt = np.dtype(dt)
    w, held, fresh, lens = 8, 40, 10, [2, 3, 9, 0, 5]
    rng = np.random.default_rng(ou.case_seed("fm-sparse", dt.name))
    K = np.unique(rng.integers(0, 2**32, 3 * (held + fresh), dtype=np.uint64))[: held + fresh].astype(np.uint32)
    K = K[rng.permutation(K.size)]
    rank = np.argsort(np.argsort(K)).astype(np.uint32) + KB  # the key of K[i] in the twin
    p0 = rng.standard_normal((held, w)).astype(dt)
    with ps.Shard.sparse(held + fresh, dt, width=w) as a, make(held + fresh, dt, w, "adagrad") as b:
        fu.set_optimizer(a, "adagrad")
        a.add(K[:held], p0)
        b.add(rank[:held], p0)
        # the pull: stored keys and absent ones (zero rows in both, no insertion, no error)
        pos = rng.permutation(held + fresh)[: sum(lens)]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        wts = rng.standard_normal(pos.size).astype(dt)
        for x, y in zip(pull(a, K[pos], off, wts, cuda), pull(b, rank[pos], off, wts, cuda)):
            same_bits(x, y, "pull")
        a.sync()
        assert a.sparse_info()["count"] == held
        # the push inserts the new keys before anything is read: they count as zero rows in S
        c = rng.standard_normal(len(lens)).astype(dt)
        push(a, K[pos], off, c, wts, None, cuda)
        push(b, rank[pos], off, c, wts, None, cuda)
        a.sync()
        assert a.sparse_info()["count"] == np.unique(np.concatenate([np.arange(held), pos])).size
        every = np.unique(np.concatenate([np.arange(held), pos]))  # the keys the sparse shard holds
        for x, y, name in zip(fu.state(a, K[every]), fu.state(b, rank[every]), ["p", "h"]):
            same_bits(x, y, f"push, {name}")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_an_infinity_reaches_only_the_bags_and_keys_that_hold_it(cuda, dt):
    dt = np.dtype(dt)
    rows, w, lens, bad, col = 40, 5, [3, 2, 4, 1, 6], 11, 2
    rng = np.random.default_rng(ou.case_seed("fm-inf", dt.name))
    p0 = rng.standard_normal((rows, w)).astype(dt)
    idx = rng.permutation(rows)[: sum(lens)]
    idx[0:2], idx[6] = bad, bad  # twice in bag 0 (its sum of gradient rows runs through gsum), once in bag 2
    idx[3:5] = [5, 5]  # a clean duplicate in bag 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    keys = (idx + KB).astype(np.uint32)
    bag = np.repeat(np.arange(len(lens)), lens)
    hit_bags = np.unique(bag[idx == bad])
    with make(rows, dt, w, "sgd") as a, make(rows, dt, w, "sgd") as b:
        a.add(all_keys(rows), p0)
        a.add(np.array([KB + bad], dtype=np.uint32), np.where(np.arange(w) == col, np.inf, p0[bad])[None].astype(dt))
        _, pair = pull(a, keys, off, None, cuda)
        assert np.isnan(pair[hit_bags]).all() and np.isfinite(np.delete(pair, hit_bags)).all(), pair
        push(a, keys, off, rng.standard_normal(len(lens)).astype(dt), None, None, cuda)
        p = fu.state(a, all_keys(rows))[0]
        touched = np.zeros((rows, w), dtype=bool)
        touched[np.unique(idx[np.isin(bag, hit_bags)]), col] = True
        assert not np.isfinite(p[touched]).any() and np.isfinite(p[~touched]).all()
        # the gradient scratch is zero again: refilled, a step of distinct keys equals the twin's
        g = rng.standard_normal((rows, w)).astype(dt)
        for sh in (a, b):
            sh.add(all_keys(rows), p0)
            sh.apply(all_keys(rows), g)
        same_bits(fu.state(a, all_keys(rows))[0], fu.state(b, all_keys(rows))[0], "the step after the push")
        a.sync()


def test_mf_step_through_hip_storage(cuda):
    """tests/cpp/hip_storage_fm_test.cpp: a matrix-factorisation step through HipStorage."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_fm_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
