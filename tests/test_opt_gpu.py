"""GPU tests of optimizer steps (pskv_apply): one call is one step, applied
exactly once per distinct key of the call to the SUM of the key's gradient rows.

Two bars (tests/opt_util.py):
  * dyadic SGD inputs, whose every sum, product and difference is exact in
    float32 (tests/test_opt_cpu.py proves it): compared bit for bit, which
    catches a step per occurrence, a dropped loser, a gradient scratch left
    dirty, a wrong winner row and a mixed row with zero tolerance;
  * random inputs, Adagrad and SGD with weight decay: the one-step check
    against a float64 step from the shard's own state, with the tolerances
    derived in DESIGN.md §8c, on p and on h, every element of the range.
"""
import os
import subprocess

import numpy as np
import pytest

import opt_util as ou
from rows_util import LAYOUTS, bits
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 3, 4, 16, 33, 64]
COUNTS = [1, 2049, 4100]
PATTERNS = ["distinct", "all_equal", "dups_in_chunk", "dups_across_chunks", "range_ends"]
PATHS = ["device", "host", "device_grouped", "host_grouped", "device_unaligned"]


def all_keys(kb, ke):
    return np.arange(kb, ke, dtype=np.int64).astype(np.uint32)


def rows_of(sh, a):
    return np.asarray(a).reshape(-1, sh.width)


def read_p(sh):
    return rows_of(sh, sh.get(all_keys(sh.key_begin, sh.key_end)))


def read_h(sh):
    return rows_of(sh, sh.get_state(all_keys(sh.key_begin, sh.key_end)))


def split3(keys, grads):
    """Three batches: a third, an empty one, the rest."""
    a = keys.size // 3
    return [(keys[:a], grads[:a]), (keys[:0], grads[:0]), (keys[a:], grads[a:])]


def do_apply(sh, keys, grads, path, cuda):
    w = sh.width
    if path == "host":
        sh.apply(keys, grads if keys.size % 2 else grads.reshape(-1))
    elif path == "device":
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
    elif path == "device_unaligned":  # one element off 16 bytes: the element unit
        dv = tdev(grads.reshape(-1), cuda, 1)
        sh.apply(tdev(keys, cuda, 1), dv.view(keys.size, w) if w > 1 else dv)
    elif path == "host_grouped":
        sh.apply_grouped(split3(keys, grads))
    elif path == "device_grouped":
        sh.apply_grouped([(tdev(k, cuda), tdev(g, cuda)) for k, g in split3(keys, grads)])
    else:
        raise ValueError(path)


def assert_bits(got, want, msg):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{msg}: {len(bad)} elements differ, first (row, col) {bad[:3].tolist()}: "
                             f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


# ------------------------------------------------------- SGD, bit-exact
def _dyadic_combos():
    out = []
    for li, (kb, ke) in enumerate(LAYOUTS):
        for n in COUNTS:
            for pat in PATTERNS:
                if pat == "distinct" and n > ke - kb:
                    continue
                c = len(out)
                out.append((li, n, pat, WIDTHS[(c + c // 6) % 6]))
    return out


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("li,n,pat,w", _dyadic_combos())
def test_sgd_dyadic_is_bit_exact(cuda, dt, li, n, pat, w):
    """3 steps with overlapping key sets on every path; the bits after each."""
    import parameter_server_amd as ps

    dt = np.dtype(dt)
    kb, ke = LAYOUTS[li]
    p0, calls = ou.dyadic_steps(ou.case_seed(n, w, pat, li), kb, ke, n, w, pat, dt)
    keys_all = all_keys(kb, ke)
    with ps.Shard(kb, ke, dt, width=w, mode="accumulate" if n == 2049 else "assign") as sh:
        sh.set_optimizer("sgd", lr=ou.DYADIC_LR)
        for path in PATHS:
            sh.clear()
            sh.add(keys_all, p0)  # an Add initialises the parameters
            p = p0.astype(np.float64)
            for step, (keys, grads) in enumerate(calls):
                do_apply(sh, keys, grads, path, cuda)
                p = ou.step64(p, None, keys.astype(np.int64) - kb, grads, "sgd", ou.DYADIC_LR)["p"]
                assert_bits(read_p(sh), p.astype(dt), f"{path} step {step}")
        sh.sync()


# ------------------------------------- Adagrad, SGD with weight decay: bounds
def _bound_params():
    out = []
    for i, case in enumerate(ou.bound_cases()):
        for dt in (np.float32, np.float64):
            out.append(pytest.param(case, dt, PATHS[i % len(PATHS)],
                                    id=f"{'-'.join(map(str, case))}-{np.dtype(dt).name}-{PATHS[i % len(PATHS)]}"))
    return out


@pytest.mark.parametrize("case,dt,path", _bound_params())
def test_steps_meet_the_one_step_bound(cuda, case, dt, path):
    import parameter_server_amd as ps

    li, n, w, pat, kind, wd = case
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[li]
    p0, calls = ou.bound_steps(ou.case_seed(case, dt.name), kb, ke, n, w, pat, dt)
    lr, eps = ou.BOUND_LR, ou.BOUND_EPS
    with ps.Shard(kb, ke, dt, width=w) as sh:
        sh.set_optimizer(kind, lr=lr, weight_decay=wd, eps=eps, init_accum=ou.BOUND_INIT_ACCUM)
        sh.add(all_keys(kb, ke), p0)
        if kind == "adagrad":
            assert_bits(read_h(sh), np.full(p0.shape, ou.BOUND_INIT_ACCUM, dtype=dt), "initial accumulator")
        for step, (keys, grads) in enumerate(calls):
            p = read_p(sh)
            h = read_h(sh) if kind == "adagrad" else None
            do_apply(sh, keys, grads, path, cuda)
            ou.check_step64(p, h, keys.astype(np.int64) - kb, grads, read_p(sh),
                          read_h(sh) if kind == "adagrad" else None, dt, kind, lr, wd, eps,
                          msg=f"{path} step {step}")
        sh.sync()


# ------------------------------------------- more than 64 batches in a call
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w", [1, 4])
@pytest.mark.parametrize("nb", [65, 130])
def test_more_than_64_batches_are_still_one_step(cuda, nb, w, device):
    """Tiny batches that share keys across the 64-batch boundary of the launch
    groups: bit-exact, and equal to the same batches concatenated into one."""
    import parameter_server_amd as ps

    kb, ke = 100, 140
    rng = np.random.default_rng(nb * 10 + w)
    p0 = ou.dyadic_params(rng, ke - kb, w, np.float32)
    # Adagrad-free but not linear in the call count: weight decay 2^-2 (exact
    # on these inputs) makes two steps differ from one step on the sum
    lr, wd = 2.0**-3, 2.0**-2
    batches = [((kb + rng.integers(0, 12, size=3)).astype(np.uint32), ou.dyadic_grads(rng, 3, w, np.float32))
               for _ in range(nb)]
    batches[64] = (batches[0][0].copy(), batches[64][1])  # the same keys on both sides of the boundary
    cat_k = np.concatenate([k for k, _ in batches])
    cat_g = np.concatenate([g for _, g in batches])
    want = ou.step64(p0, None, cat_k.astype(np.int64) - kb, cat_g, "sgd", lr, wd)["p"]
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)  # exact in float32
    got = []
    for grouped in (True, False):
        with ps.Shard(kb, ke, np.float32, width=w) as sh:
            sh.set_optimizer("sgd", lr=lr, weight_decay=wd)
            sh.add(all_keys(kb, ke), p0)
            if grouped:
                sh.apply_grouped([(tdev(k, cuda), tdev(g, cuda)) for k, g in batches] if device else batches)
            elif device:
                sh.apply(tdev(cat_k, cuda), tdev(cat_g, cuda))
            else:
                sh.apply(cat_k, cat_g)
            got.append(read_p(sh))
            # the gradient scratch is clean again: a second step sees only its own gradients
            sh.apply(cat_k[:1], np.zeros((1, w), dtype=np.float32))
            again = ou.step64(want, None, cat_k[:1].astype(np.int64) - kb, np.zeros((1, w)), "sgd", lr, wd)["p"]
            assert_bits(read_p(sh), again.astype(np.float32), "the step after")
            sh.sync()
    assert_bits(got[0], want.astype(np.float32), f"{nb} batches")
    assert_bits(got[1], got[0], "concatenated")


# ------------------------------------------------ interleaving with Add / Get
@pytest.mark.parametrize("w,options", [(1, {"GENERAL": 0}), (1, None), (16, None), (3, None)])
def test_apply_interleaves_with_add_and_get(cuda, w, options):
    """assign Add (whose stamps share the stamp array and the epochs), apply,
    Add to some keys, apply, Get: p follows the oracle, h ignores Adds; clear
    resets p to 0 and h to init_accum."""
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[0]
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(40 + w)
    lr, wd, eps, init = 0.05, 0.01, 1e-8, 0.1
    keys_all = all_keys(kb, ke)

    def step(sh, n):
        keys = (kb + rng.integers(0, 600, size=n)).astype(np.uint32)
        grads = (rng.standard_normal((n, w)) * 3).astype(dt)
        p, h = read_p(sh), read_h(sh)
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        ou.check_step64(p, h, keys.astype(np.int64) - kb, grads, read_p(sh), read_h(sh), dt, "adagrad", lr, wd, eps)

    with ps.Shard(kb, ke, dt, width=w, options=options) as sh:
        sh.set_optimizer("adagrad", lr=lr, weight_decay=wd, eps=eps, init_accum=init)
        p0 = rng.standard_normal((ke - kb, w)).astype(dt)
        sh.add(tdev(keys_all, cuda), tdev(p0, cuda))  # device assign Add: the stamp path
        assert_bits(read_p(sh), p0, "initial Add")
        step(sh, 2049)
        h = read_h(sh)
        p = read_p(sh)
        some = (kb + rng.integers(0, 600, size=300)).astype(np.uint32)  # with duplicates: last wins
        vals = rng.standard_normal((300, w)).astype(dt)
        sh.add(tdev(some, cuda), tdev(vals, cuda))
        for i, k in enumerate(some):
            p[int(k) - kb] = vals[i]
        assert_bits(read_p(sh), p, "Add between steps")
        assert_bits(read_h(sh), h, "an Add must not touch h")
        step(sh, 4100)
        sh.clear()
        assert not read_p(sh).any()
        assert_bits(read_h(sh), np.full((ke - kb, w), init, dtype=dt), "h after clear")
        step(sh, 2049)  # behaves like a first step
        sh.sync()


@pytest.mark.parametrize("options", [{"SERVE": 1}, {"INLINE": 1}, {"INLINE": 0}], ids=["serve", "inline", "staged"])
def test_apply_orders_against_small_host_adds_and_gets(cuda, options):
    """A width-1 shard's small host Adds and Gets go to the resident request
    server (SERVE = 1) or travel in kernel arguments (K8): steps between them
    see what they wrote, and they see the steps."""
    import parameter_server_amd as ps

    kb, ke = 0, 5000
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(55)
    keys = np.arange(100, 300, dtype=np.uint32)  # 200 keys: inline / request-server size
    p = np.zeros((ke - kb, 1))
    with ps.Shard(kb, ke, dt, options=options) as sh:
        sh.set_optimizer("sgd", lr=ou.DYADIC_LR)
        for step in range(3):
            vals = ou.dyadic_params(rng, keys.size, 1, dt)
            sh.add(keys, vals.reshape(-1))
            p[keys.astype(np.int64) - kb] = vals
            k = (kb + rng.integers(50, 350, size=400)).astype(np.uint32)
            g = ou.dyadic_grads(rng, 400, 1, dt)
            if step % 2:
                sh.apply(k, g)
            else:
                sh.apply(tdev(k, cuda), tdev(g, cuda))
            p = ou.step64(p, None, k.astype(np.int64) - kb, g, "sgd", ou.DYADIC_LR)["p"]
            q = np.arange(0, 400, dtype=np.uint32)
            assert_bits(sh.get(q).reshape(-1, 1), p[:400].astype(dt), f"step {step}")
        sh.sync()


# ------------------------------------------------------- out-of-range keys
@pytest.mark.parametrize("w", [1, 16])
def test_out_of_range_keys_are_refused(cuda, w):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke = 1000, 3000
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(60 + w)
    p0 = ou.dyadic_params(rng, ke - kb, w, dt)
    keys = (kb + rng.integers(0, ke - kb, size=500)).astype(np.uint32)
    keys[77], keys[300] = 3007, 12  # outside on both sides
    grads = ou.dyadic_grads(rng, 500, w, dt)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        sh.set_optimizer("adagrad", lr=2.0**-3, init_accum=0.5)
        sh.add(all_keys(kb, ke), p0)
        h0 = read_h(sh)
        with pytest.raises(_lib.PskvError) as e:
            sh.apply(keys, grads)
        assert e.value.code == _lib.PSKV_EINVAL and "3007" in str(e.value)
        assert_bits(read_p(sh), p0, "a refused host apply changed p")
        assert_bits(read_h(sh), h0, "a refused host apply changed h")
        sh.sync()
        # device: the in-range keys are applied, the others dropped and reported
        sh.set_optimizer("sgd", lr=2.0**-3)
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        inside = (keys >= kb) & (keys < ke)
        want = ou.step64(p0, None, keys[inside].astype(np.int64) - kb, grads[inside], "sgd", 2.0**-3)["p"]
        assert_bits(read_p(sh), want.astype(dt), "device apply with out-of-range keys")
        with pytest.raises(_lib.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE and "out-of-range" in str(e.value)
        sh.clear()
        sh.sync()


# ------------------------------------------------------------ set_optimizer
def test_set_optimizer_semantics(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, w = 0, 3000, 4
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(70)
    p0 = ou.dyadic_params(rng, ke - kb, w, dt)
    keys = rng.integers(kb, ke, size=2049).astype(np.uint32)
    grads = ou.dyadic_grads(rng, 2049, w, dt)
    idx = keys.astype(np.int64) - kb
    with ps.Shard(kb, ke, dt, width=w) as sh:
        assert sh.optimizer()["kind"] is None and sh.optimizer()["state_bytes"] == 0
        with pytest.raises(_lib.PskvError) as e:
            sh.apply(keys, grads)
        assert e.value.code == _lib.PSKV_EINVAL and "optimizer" in str(e.value)
        with pytest.raises(_lib.PskvError) as e:
            sh.get_state(keys)
        assert e.value.code == _lib.PSKV_EINVAL
        # a hyper-parameter change takes effect from the next call
        sh.set_optimizer("sgd", lr=2.0**-3)
        sh.add(all_keys(kb, ke), p0)
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        sh.set_optimizer("sgd", lr=2.0**-5)
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        p1 = ou.step64(p0, None, idx, grads, "sgd", 2.0**-3)["p"]
        p2 = ou.step64(p1, None, idx, grads, "sgd", 2.0**-5)["p"]
        assert_bits(read_p(sh), p2.astype(dt), "two learning rates")
        o = sh.optimizer()
        assert (o["kind"], o["lr"], o["weight_decay"]) == ("sgd", 2.0**-5, 0.0)
        dense = (ke - kb) * w * 4
        assert o["state_bytes"] == dense + 8 * (ke - kb)  # gradient scratch + stamps
        # a kind change resets h
        sh.set_optimizer("adagrad", lr=0.05, weight_decay=0.01, eps=1e-8, init_accum=0.25)
        o = sh.optimizer()
        assert o == {"kind": "adagrad", "lr": 0.05, "weight_decay": 0.01, "eps": 1e-8, "init_accum": 0.25,
                     "state_bytes": 2 * dense + 8 * (ke - kb)}
        assert_bits(read_h(sh), np.full((ke - kb, w), 0.25, dtype=dt), "h after set_optimizer")
        sh.apply(keys, grads)
        assert (read_h(sh)[np.unique(idx)] > 0.25).any()
        sh.set_optimizer("sgd", lr=0.05)
        sh.set_optimizer("adagrad", lr=0.05, init_accum=0.5)
        assert_bits(read_h(sh), np.full((ke - kb, w), 0.5, dtype=dt), "h after a kind change")
        sh.set_optimizer(None)
        assert sh.optimizer()["state_bytes"] == 0
        sh.sync()
    with ps.Shard(kb, ke, np.int32) as si:
        with pytest.raises(_lib.PskvError) as e:
            si.set_optimizer("sgd", lr=0.1)
        assert e.value.code == _lib.PSKV_EINVAL and "float" in str(e.value)
        with pytest.raises(_lib.PskvError) as e:
            si.apply(keys, np.ones(keys.size, dtype=np.int32))
        assert e.value.code == _lib.PSKV_EINVAL


# ------------------------------------------------------------------- timing
def test_apply_time_counts_one_operation_per_launch_group(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, w = 0, 3000, 4
    rng = np.random.default_rng(80)
    keys = rng.integers(kb, ke, size=2049).astype(np.uint32)
    grads = rng.standard_normal((2049, w)).astype(np.float32)
    tiny = [(keys[i:i + 2], grads[i:i + 2]) for i in range(65)]
    with ps.Shard(kb, ke, np.float32, width=w) as sh:
        sh.set_optimizer("adagrad", lr=0.05)
        sh.apply(keys, grads)  # timing off
        assert sh.apply_time() == {"launches": 0, "total_ms": 0.0, "elements": 0}
        sh.set_timing(True)
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        t = sh.apply_time()
        assert t["launches"] == 1 and t["elements"] == 2049 and t["total_ms"] > 0
        sh.apply_grouped(tiny)  # 65 batches: two launch groups
        t = sh.apply_time()
        assert t["launches"] == 3 and t["elements"] == 2049 + 130
        for k in range(_lib.PSKV_K_COUNT):
            assert sh.kernel_time(k)["launches"] == 0, _lib.KERNEL_NAMES[k]
        sh.get_state(keys)
        assert sh.kernel_time(_lib.PSKV_K_ROW_GATHER)["launches"] == 1
        sh.reset_timing()
        assert sh.apply_time()["launches"] == 0
        # the slot's own mask bit
        sh.set_timing(False)
        _lib.check(_lib.lib.pskv_set_timing_mask(sh.handle, _lib.PSKV_TIME_APPLY))
        sh.apply(keys, grads)
        sh.get_state(keys)
        assert sh.apply_time()["launches"] == 1
        assert sh.kernel_time(_lib.PSKV_K_ROW_GATHER)["launches"] == 0
        sh.sync()


# -------------------------------------------------------------- HipStorage
def test_hip_storage_with_an_optimizer(cuda):
    """Through Message / Add / Get: two Add messages on one key are two steps,
    AddGrouped of the same two is ONE step on the sum (weight decay 2^-2,
    exact on these inputs, tells them apart)."""
    from parameter_server_amd.storage import Flag, HipStorage, Message, typed

    lr, wd, w = 2.0**-3, 2.0**-2, 4
    opt = {"kind": "sgd", "lr": lr, "weight_decay": wd}
    keys = np.array([5, 9, 5], dtype=np.uint32)
    g1 = np.arange(12, dtype=np.float32).reshape(3, w) / 4
    g2 = g1[::-1].copy() + 1

    def msg(k, v=None, flag=Flag.kAdd):
        m = Message()
        m.meta.flag = flag
        m.AddData(k)
        if v is not None:
            m.AddData(v)
        return m

    def pull(st):
        rep = st.Get(msg(np.array([5, 9, 7], dtype=np.uint32), flag=Flag.kGet))
        return typed(rep.data[1], np.float32).reshape(3, w).astype(np.float64)

    idx = np.array([0, 1, 0])  # rows of keys 5, 9 (7 is row 2)
    zero = np.zeros((3, w))
    two = ou.step64(ou.step64(zero, None, idx, g1, "sgd", lr, wd)["p"], None, idx, g2, "sgd", lr, wd)["p"]
    one = ou.step64(zero, None, np.concatenate([idx, idx]), np.concatenate([g1, g2]), "sgd", lr, wd)["p"]
    assert not np.array_equal(one, two)
    st = HipStorage(np.float32, 0, 100, width=w, optimizer=opt)
    try:
        st.Add(msg(keys, g1))
        st.Add(msg(keys, g2))
        assert np.array_equal(pull(st), two)
        st.FinishIter()
    finally:
        st.close()
    st = HipStorage(np.float32, 0, 100, width=w, optimizer=opt)
    try:
        st.AddGrouped([msg(keys, g1), msg(keys, g2)])
        assert np.array_equal(pull(st), one)
        st.FinishIter()
    finally:
        st.close()


def test_cpp_opt_program(cuda):
    """tests/cpp/hip_storage_opt_test.cpp: HipStorage<float> with an SGD
    optimizer behind std::unique_ptr<AbstractStorage>: SubAdd is a step,
    AddGrouped of two messages on overlapping keys is one step."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_opt_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
