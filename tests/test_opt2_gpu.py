"""GPU tests of momentum and Adam steps (pskv_shard_set_optimizer_ex), of the
step counter, of state slot access (pskv_get_state_slot, pskv_put_state) and of
checkpoints (Shard.state_dict / load_state_dict).

Two bars (tests/opt_util.py), as tests/test_opt_gpu.py:
  * dyadic momentum inputs, whose every intermediate is exact in float32
    (tests/test_opt2_cpu.py proves it): p and v compared bit for bit;
  * random inputs, momentum (Nesterov on and off) and Adam, weight decay 0 and
    0.01: the one-step check against an extended-precision step from the
    shard's own p and slots, with the tolerances derived in DESIGN.md §8d, on p
    and on every slot, every element of the range.
"""
import os
import subprocess

import numpy as np
import pytest

import opt_util as ou
from rows_util import LAYOUTS, bits
from test_gpu_parity import tdev
from test_opt_gpu import PATHS, all_keys, assert_bits, do_apply, read_p, rows_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 3, 4, 16, 33, 64]
COUNTS = [1, 2, 2049, 4100]
PATTERNS = ["distinct", "all_equal", "dups_in_chunk", "dups_across_chunks", "range_ends"]


def read_slots(sh, kind):
    keys = all_keys(sh.key_begin, sh.key_end)
    return [rows_of(sh, sh.get_state(keys, slot=i)) for i in range(ou.SLOTS[kind])]


# ------------------------------------------------ dyadic momentum, bit-exact
def _dyadic_combos():
    out = []
    for li, (kb, ke) in enumerate(LAYOUTS):
        for n in COUNTS:
            for pat in PATTERNS:
                if pat == "distinct" and n > ke - kb:
                    continue
                c = len(out)
                out.append((li, n, pat, WIDTHS[(c + c // 6) % 6], bool(c % 2)))
    return out


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("li,n,pat,w,nesterov", _dyadic_combos())
def test_momentum_dyadic_is_bit_exact(cuda, dt, li, n, pat, w, nesterov):
    """3 steps with overlapping key sets on every path; the bits of p and v after each."""
    import parameter_server_amd as ps

    dt = np.dtype(dt)
    kb, ke = LAYOUTS[li]
    p0, calls = ou.dyadic_steps2(n, w, pat, li, dt)
    hp = ou.dyadic_hyper(nesterov)
    keys_all = all_keys(kb, ke)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        sh.set_optimizer("momentum", **ou.set_optimizer_kwargs(hp))
        for path in PATHS:
            sh.clear()
            sh.add(keys_all, p0)
            p, v = p0, np.zeros(p0.shape, dtype=dt)
            for step, (keys, grads) in enumerate(calls):
                do_apply(sh, keys, grads, path, cuda)
                ref = ou.step_ref(p, [v], keys.astype(np.int64) - kb, grads, hp)
                p, v = ref["p"].astype(dt), ref["slots"][0].astype(dt)
                assert_bits(read_p(sh), p, f"p {path} step {step}")
                assert_bits(read_slots(sh, "momentum")[0], v, f"v {path} step {step}")
            assert sh.step == len(calls)
        sh.sync()


# ------------------------------------------------ momentum and Adam: bounds
def _bound_params():
    out = []
    for i, case in enumerate(ou.bound_cases2()):
        for dt in (np.float32, np.float64):
            path = PATHS[i % len(PATHS)]
            out.append(pytest.param(case, dt, path, id=f"{'-'.join(map(str, case))}-{np.dtype(dt).name}-{path}"))
    return out


@pytest.mark.parametrize("case,dt,path", _bound_params())
def test_steps_meet_the_one_step_bound(cuda, case, dt, path):
    import parameter_server_amd as ps

    li, n, w, pat, kind, _, _ = case
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[li]
    hp = ou.case_hyper(case)
    p0, calls = ou.bound_steps2(case, dt)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        sh.set_optimizer(kind, **ou.set_optimizer_kwargs(hp))
        sh.add(all_keys(kb, ke), p0)
        for s in read_slots(sh, kind):
            assert not s.any(), "initial state"
        for t, (keys, grads) in enumerate(calls, 1):
            p, slots = read_p(sh), read_slots(sh, kind)
            do_apply(sh, keys, grads, path, cuda)
            assert sh.step == t
            ou.check_step(p, slots, keys.astype(np.int64) - kb, grads, read_p(sh), read_slots(sh, kind), dt, hp, t,
                          msg=f"{path} step {t}")
        sh.sync()


# ------------------------------------------- more than 64 batches in a call
def _tiny_batches(rng, kb, w, nb=65):
    batches = [((kb + rng.integers(0, 12, size=3)).astype(np.uint32), ou.dyadic_grads(rng, 3, w, np.float32))
               for _ in range(nb)]
    batches[64] = (batches[0][0].copy(), batches[64][1])  # the same keys on both sides of the group boundary
    return batches, np.concatenate([k for k, _ in batches]), np.concatenate([g for _, g in batches])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w", [1, 4])
def test_65_batches_are_one_momentum_step(cuda, w, device):
    """Two launch groups sharing keys: one step (v = the sum, not 0.5 v + ...),
    bit-exact in the dyadic form and equal to the concatenated call."""
    import parameter_server_amd as ps

    kb, ke = 100, 140
    rng = np.random.default_rng(650 + w)
    p0 = ou.dyadic_params(rng, ke - kb, w, np.float32)
    hp = ou.dyadic_hyper(True)
    batches, cat_k, cat_g = _tiny_batches(rng, kb, w)
    ref = ou.step_ref(p0, [np.zeros_like(p0)], cat_k.astype(np.int64) - kb, cat_g, hp)
    got = []
    for grouped in (True, False):
        with ps.Shard(kb, ke, np.float32, width=w) as sh:
            sh.set_optimizer("momentum", **ou.set_optimizer_kwargs(hp))
            sh.add(all_keys(kb, ke), p0)
            if grouped:
                sh.apply_grouped([(tdev(k, cuda), tdev(g, cuda)) for k, g in batches] if device else batches)
            elif device:
                sh.apply(tdev(cat_k, cuda), tdev(cat_g, cuda))
            else:
                sh.apply(cat_k, cat_g)
            assert sh.step == 1
            got.append((read_p(sh), read_slots(sh, "momentum")[0]))
            sh.sync()
    assert_bits(got[0][0], ref["p"].astype(np.float32), "p, 65 batches")
    assert_bits(got[0][1], ref["slots"][0].astype(np.float32), "v, 65 batches")
    assert_bits(got[1][0], got[0][0], "p, concatenated")
    assert_bits(got[1][1], got[0][1], "v, concatenated")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_65_batches_are_one_adam_step(cuda, device):
    """Both launch groups use t = 1; the step counter reads 1 afterwards; the
    result meets the one-step bound, as the concatenated call's does."""
    import parameter_server_amd as ps

    kb, ke, w = 100, 140, 4
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(651)
    p0 = rng.standard_normal((ke - kb, w)).astype(dt)
    hp = ou.hyper("adam", wd=0.01)
    batches, cat_k, cat_g = _tiny_batches(rng, kb, w)
    for grouped in (True, False):
        with ps.Shard(kb, ke, dt, width=w) as sh:
            sh.set_optimizer("adam", **ou.set_optimizer_kwargs(hp))
            sh.add(all_keys(kb, ke), p0)
            if grouped:
                sh.apply_grouped([(tdev(k, cuda), tdev(g, cuda)) for k, g in batches] if device else batches)
            else:
                sh.apply(tdev(cat_k, cuda), tdev(cat_g, cuda)) if device else sh.apply(cat_k, cat_g)
            assert sh.step == 1
            ou.check_step(p0, ou.zero_slots("adam", p0.shape, dt), cat_k.astype(np.int64) - kb, cat_g, read_p(sh),
                          read_slots(sh, "adam"), dt, hp, 1, msg=f"grouped {grouped}")
            sh.sync()


# ------------------------------------------------------------ step counter
def test_step_counter(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, w = 1000, 3000, 4
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(90)
    p0 = rng.standard_normal((ke - kb, w)).astype(dt)
    keys = (kb + rng.integers(0, ke - kb, size=500)).astype(np.uint32)
    grads = (rng.standard_normal((500, w)) * 3).astype(dt)
    bad = keys.copy()
    bad[77], bad[300] = 3007, 12  # outside on both sides
    inside = (bad >= kb) & (bad < ke)
    hp = ou.hyper("adam")
    with ps.Shard(kb, ke, dt, width=w) as sh:
        assert sh.step == 0
        sh.set_optimizer("adam", **ou.set_optimizer_kwargs(hp))
        sh.add(all_keys(kb, ke), p0)
        assert sh.step == 0  # an Add is no step
        sh.apply(keys, grads)
        assert sh.step == 1
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        assert sh.step == 2
        sh.apply(keys[:0], grads[:0])  # no keys: no step
        sh.apply_grouped([(keys[:0], grads[:0]), (keys[:0], grads[:0])])
        assert sh.step == 2
        # a refused host call: nothing applied, no step
        p, slots = read_p(sh), read_slots(sh, "adam")
        with pytest.raises(_lib.PskvError) as e:
            sh.apply(bad, grads)
        assert e.value.code == _lib.PSKV_EINVAL and "3007" in str(e.value)
        assert sh.step == 2
        assert_bits(read_p(sh), p, "a refused host apply changed p")
        for a, b, nm in zip(read_slots(sh, "adam"), slots, "mv"):
            assert_bits(a, b, f"a refused host apply changed {nm}")
        # a device call with out-of-range keys: the in-range keys step (t = 3), the next sync reports
        sh.apply(tdev(bad, cuda), tdev(grads, cuda))
        assert sh.step == 3
        ou.check_step(p, slots, bad[inside].astype(np.int64) - kb, grads[inside], read_p(sh), read_slots(sh, "adam"),
                      dt, hp, 3, msg="device apply with out-of-range keys")
        with pytest.raises(_lib.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE and "out-of-range" in str(e.value)
        # the same kind with a new lr keeps t and the state
        slots = read_slots(sh, "adam")
        sh.set_optimizer("adam", **dict(ou.set_optimizer_kwargs(hp), lr=0.01))
        assert sh.step == 3 and sh.optimizer()["lr"] == 0.01
        for a, b, nm in zip(read_slots(sh, "adam"), slots, "mv"):
            assert_bits(a, b, f"a new lr changed {nm}")
        # clear: t = 0, p, m and v zero; the next step is a first step
        sh.clear()
        sh.sync()
        assert sh.step == 0 and not read_p(sh).any()
        for s in read_slots(sh, "adam"):
            assert not s.any()
        hp2 = ou.hyper("adam", lr=0.01)
        sh.apply(keys, grads)
        assert sh.step == 1
        ou.check_step(np.zeros_like(p0), ou.zero_slots("adam", p0.shape, dt), keys.astype(np.int64) - kb, grads,
                      read_p(sh), read_slots(sh, "adam"), dt, hp2, 1, msg="the step after clear")
        # a kind change resets t and the state
        sh.set_optimizer("momentum", lr=0.05, momentum=0.9)
        assert sh.step == 0
        assert not read_slots(sh, "momentum")[0].any()
        sh.apply(keys, grads)
        assert sh.step == 1
        sh.step = 41  # kept for every kind
        sh.apply(keys, grads)
        assert sh.step == 42
        sh.set_optimizer("sgd", lr=0.05)
        assert sh.step == 0
        sh.apply(keys, grads)
        assert sh.step == 1
        sh.sync()


# -------------------------------------------------------------- slot access
@pytest.mark.parametrize("kind,w", [("adam", 1), ("adam", 4), ("momentum", 33), ("adagrad", 16), ("adagrad", 1)])
def test_put_state_round_trip(cuda, kind, w):
    """put_state then get_state on every slot, host and device, with duplicated
    keys (the last row wins whole); a slot written does not touch p or the other slot."""
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[1]
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(100 + w)
    nslots = {"adam": 2, "momentum": 1, "adagrad": 1}[kind]
    keys_all = all_keys(kb, ke)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        sh.set_optimizer(kind, lr=0.05, eps=1e-8, init_accum=0.5)
        p0 = rng.standard_normal((ke - kb, w)).astype(dt)
        sh.add(keys_all, p0)
        want = [rows_of(sh, sh.get_state(keys_all, slot=i)).copy() for i in range(nslots)]
        for rnd, device in enumerate((False, True, False, True)):
            for slot in range(nslots):
                n = 2049
                keys = (kb + rng.integers(0, 300, size=n)).astype(np.uint32)  # many duplicates
                vals = (np.arange(n * w, dtype=np.float32).reshape(n, w) + 1 + 100000 * (2 * rnd + slot))
                if device:
                    sh.put_state(tdev(keys, cuda), tdev(vals, cuda), slot=slot)
                else:
                    sh.put_state(keys, vals if w > 1 else vals.reshape(-1), slot=slot)
                for i, k in enumerate(keys):
                    want[slot][int(k) - kb] = vals[i]
                for s in range(nslots):
                    got = sh.get_state(tdev(keys_all, cuda), slot=s).cpu().numpy() if device else \
                        sh.get_state(keys_all, slot=s)
                    assert_bits(rows_of(sh, got), want[s], f"slot {s} after put to slot {slot}, round {rnd}")
        assert_bits(read_p(sh), p0, "put_state touched p")
        if kind == "adagrad":  # h written by put_state reads back through the old entry point
            from parameter_server_amd import _lib

            out = np.empty((ke - kb, w), dtype=dt)
            _lib.check(_lib.lib.pskv_get_state(sh.handle, keys_all.ctypes.data, keys_all.size, out.ctypes.data,
                                               _lib.PSKV_HOST))
            assert_bits(out, want[0], "pskv_get_state after put_state")
        assert sh.step == 0
        sh.sync()


def test_slot_errors(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, w = 1000, 3000, 4
    keys = np.array([1000, 2999, 1500], dtype=np.uint32)
    vals = np.ones((3, w), dtype=np.float32)
    with ps.Shard(kb, ke, np.float32, width=w) as sh:
        for kind, nslots in ((None, 0), ("sgd", 0), ("adagrad", 1), ("momentum", 1), ("adam", 2)):
            sh.set_optimizer(kind, lr=0.05)
            for slot in (-1, 0, 1, 2):
                if 0 <= slot < nslots:
                    sh.put_state(keys, vals, slot=slot)
                    assert np.array_equal(sh.get_state(keys, slot=slot), vals)
                    continue
                for call in (lambda: sh.get_state(keys, slot=slot), lambda: sh.put_state(keys, vals, slot=slot)):
                    with pytest.raises(_lib.PskvError) as e:
                        call()
                    assert e.value.code == _lib.PSKV_EINVAL and "slot" in str(e.value), (kind, slot)
        # out-of-range keys: a host put is refused and writes nothing; a device put drops them and sync reports
        bad = np.array([1000, 3007, 1500], dtype=np.uint32)
        before = sh.get_state(keys, slot=1)
        with pytest.raises(_lib.PskvError) as e:
            sh.put_state(bad, vals * 7, slot=1)
        assert e.value.code == _lib.PSKV_EINVAL and "3007" in str(e.value)
        assert np.array_equal(sh.get_state(keys, slot=1), before)
        assert not sh.get_state(bad, slot=1)[1].any()  # a Get of such a key reads zeros
        sh.sync()
        sh.put_state(tdev(bad, cuda), tdev(vals * 7, cuda), slot=1)
        got = sh.get_state(keys, slot=1)
        assert np.array_equal(got[0], vals[0] * 7) and np.array_equal(got[2], vals[2] * 7)
        with pytest.raises(_lib.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE and "out-of-range" in str(e.value)
        sh.clear()
        sh.sync()


# -------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("kind", ["adam", "adagrad", "momentum"])
def test_checkpoint_restores_bit_for_bit(cuda, kind):
    """Two steps on A, state_dict, load_state_dict into a fresh B, a third step
    on both: p, every slot and the step count agree bit for bit.  Restored
    without the step count, Adam's p differs: the counter matters."""
    import parameter_server_amd as ps

    kb, ke, w = 500, 3500, 4
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(110)
    nslots = {"adam": 2, "momentum": 1, "adagrad": 1}[kind]
    kw = dict(lr=0.05, weight_decay=0.01, eps=1e-8, init_accum=0.1, momentum=0.9)
    keys_all = all_keys(kb, ke)
    calls = [((kb + rng.integers(0, ke - kb, size=2049)).astype(np.uint32),
              (rng.standard_normal((2049, w)) * 3).astype(dt)) for _ in range(2)]
    third = ((kb + rng.permutation(ke - kb)[:2049]).astype(np.uint32), (rng.standard_normal((2049, w)) * 3).astype(dt))

    def state(sh):
        return [read_p(sh)] + [rows_of(sh, sh.get_state(keys_all, slot=i)) for i in range(nslots)]

    with ps.Shard(kb, ke, dt, width=w) as a, ps.Shard(kb, ke, dt, width=w) as b, \
            ps.Shard(kb, ke, dt, width=w) as c:
        a.set_optimizer(kind, **kw)
        a.add(keys_all, rng.standard_normal((ke - kb, w)).astype(dt))
        for k, g in calls:
            a.apply(tdev(k, cuda), tdev(g, cuda))
        d = a.state_dict()
        assert d["t"] == 2 and len(d["slots"]) == nslots and d["optimizer"]["kind"] == kind
        b.set_optimizer(kind, **kw)
        b.load_state_dict(d)
        assert b.step == 2
        for x, y in zip(state(a), state(b)):
            assert_bits(y, x, "restored")
        c.set_optimizer(kind, **kw)
        c.load_state_dict(dict(d, t=0))  # everything but the step count
        for sh in (a, b, c):
            sh.apply(third[0], third[1])
        assert a.step == b.step == 3 and c.step == 1
        sa, sb, sc = state(a), state(b), state(c)
        for x, y, nm in zip(sa, sb, ["p", "slot 0", "slot 1"]):
            assert_bits(y, x, f"{nm} after the third step")
        for x, y in zip(sa[1:], sc[1:]):  # the slots do not depend on t
            assert_bits(y, x, "slots without the step count")
        assert (bits(sa[0]) != bits(sc[0])).any() == (kind == "adam")
        for sh in (a, b, c):
            sh.sync()


# ------------------------------------------------- configuration and memory
def test_optimizer_dict_and_state_bytes(cuda):
    import parameter_server_amd as ps

    kb, ke, w = 0, 3000, 4
    dense, stamps = (ke - kb) * w * 4, 8 * (ke - kb)
    with ps.Shard(kb, ke, np.float32, width=w) as sh:
        assert sh.optimizer() == {"kind": None, "lr": 0.0, "weight_decay": 0.0, "eps": 0.0, "init_accum": 0.0,
                                  "state_bytes": 0}
        sh.set_optimizer("sgd", lr=0.05)
        assert sh.optimizer()["state_bytes"] == dense + stamps
        assert set(sh.optimizer()) == {"kind", "lr", "weight_decay", "eps", "init_accum", "state_bytes"}
        sh.set_optimizer("adagrad", lr=0.05, init_accum=0.25)
        assert sh.optimizer()["state_bytes"] == 2 * dense + stamps
        sh.set_optimizer("momentum", lr=0.05, weight_decay=0.01, momentum=0.75, nesterov=True)
        o = sh.optimizer()
        assert o["state_bytes"] == 2 * dense + stamps
        assert (o["kind"], o["lr"], o["weight_decay"], o["momentum"], o["nesterov"]) == ("momentum", 0.05, 0.01, 0.75,
                                                                                         True)
        assert set(o) == {"kind", "lr", "weight_decay", "eps", "init_accum", "state_bytes", "momentum", "nesterov"}
        sh.set_optimizer("adam", lr=0.001)
        o = sh.optimizer()
        assert o["state_bytes"] == 3 * dense + stamps
        assert (o["kind"], o["lr"], o["eps"], o["beta1"], o["beta2"]) == ("adam", 0.001, 1e-10, 0.9, 0.999)
        assert set(o) == {"kind", "lr", "weight_decay", "eps", "init_accum", "state_bytes", "beta1", "beta2"}
        # the old getter on a new kind: the fields it has, the new kind number
        import ctypes

        from parameter_server_amd import _lib

        cfg, nb = _lib.PskvOptimizer(), ctypes.c_uint64()
        _lib.check(_lib.lib.pskv_shard_get_optimizer(sh.handle, ctypes.byref(cfg), ctypes.byref(nb)))
        assert (cfg.kind, cfg.lr, nb.value) == (_lib.PSKV_OPT_ADAM, 0.001, 3 * dense + stamps)
        # the _ex setter with an old kind is the old setter
        x = _lib.PskvOptimizerEx(ctypes.sizeof(_lib.PskvOptimizerEx), _lib.PSKV_OPT_ADAGRAD, 0.05, 0.0, 1e-8, 0.5, 0.0,
                                 0, 0.0, 0.0)
        _lib.check(_lib.lib.pskv_shard_set_optimizer_ex(sh.handle, ctypes.byref(x)))
        assert sh.optimizer() == {"kind": "adagrad", "lr": 0.05, "weight_decay": 0.0, "eps": 1e-8, "init_accum": 0.5,
                                  "state_bytes": 2 * dense + stamps}
        h = sh.get_state(all_keys(kb, ke))
        assert_bits(h, np.full(h.shape, 0.5, dtype=np.float32), "h after the _ex setter")
        sh.set_optimizer(None)
        assert sh.optimizer()["state_bytes"] == 0
        sh.sync()
    with ps.Shard(kb, ke, np.int32) as si:
        with pytest.raises(_lib.PskvError) as e:
            si.set_optimizer("adam", lr=0.1)
        assert e.value.code == _lib.PSKV_EINVAL and "float" in str(e.value)


# ------------------------------------------------------------------- timing
@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_apply_time_counts_the_new_kinds_as_before(cuda, kind):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, w = 0, 3000, 4
    rng = np.random.default_rng(120)
    keys = rng.integers(kb, ke, size=2049).astype(np.uint32)
    grads = rng.standard_normal((2049, w)).astype(np.float32)
    tiny = [(keys[i:i + 2], grads[i:i + 2]) for i in range(65)]
    with ps.Shard(kb, ke, np.float32, width=w) as sh:
        sh.set_optimizer(kind, lr=0.05, momentum=0.9)
        sh.set_timing(True)
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        t = sh.apply_time()
        assert t["launches"] == 1 and t["elements"] == 2049 and t["total_ms"] > 0
        sh.apply_grouped(tiny)  # 65 batches: two launch groups
        t = sh.apply_time()
        assert t["launches"] == 3 and t["elements"] == 2049 + 130
        for k in range(_lib.PSKV_K_COUNT):
            assert sh.kernel_time(k)["launches"] == 0, _lib.KERNEL_NAMES[k]
        sh.get_state(keys, slot=0)
        assert sh.kernel_time(_lib.PSKV_K_ROW_GATHER)["launches"] == 1
        sh.put_state(keys, grads, slot=0)
        assert sh.kernel_time(_lib.PSKV_K_ROW_COMMIT)["launches"] == 1
        assert sh.apply_time()["launches"] == 3
        sh.sync()


# -------------------------------------------------------------- HipStorage
def test_hip_storage_with_a_momentum_optimizer(cuda):
    """Two Add messages on one key are two steps, AddGrouped of the same two is
    ONE step on the sum (dyadic inputs, exact)."""
    from parameter_server_amd.storage import Flag, HipStorage, Message, typed

    w = 4
    hp = ou.dyadic_hyper(False)
    opt = dict(kind="momentum", **ou.set_optimizer_kwargs(hp))
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
        return typed(rep.data[1], np.float32).reshape(3, w)

    idx = np.array([0, 1, 0])  # rows of keys 5, 9 (7 is row 2)
    zero = np.zeros((3, w))
    r1 = ou.step_ref(zero, [zero], idx, g1, hp)
    two = ou.step_ref(r1["p"], r1["slots"], idx, g2, hp)["p"]
    one = ou.step_ref(zero, [zero], np.concatenate([idx, idx]), np.concatenate([g1, g2]), hp)["p"]
    assert not np.array_equal(one, two)
    st = HipStorage(np.float32, 0, 100, width=w, optimizer=opt)
    try:
        st.Add(msg(keys, g1))
        st.Add(msg(keys, g2))
        assert_bits(pull(st), two.astype(np.float32), "two Adds")
        assert st.shard.step == 2
        st.FinishIter()
    finally:
        st.close()
    st = HipStorage(np.float32, 0, 100, width=w, optimizer=opt)
    try:
        st.AddGrouped([msg(keys, g1), msg(keys, g2)])
        assert_bits(pull(st), one.astype(np.float32), "AddGrouped")
        assert st.shard.step == 1
        st.FinishIter()
    finally:
        st.close()


def test_cpp_opt2_program(cuda):
    """tests/cpp/hip_storage_opt2_test.cpp: HipStorage<float> with a momentum
    optimizer through the pskv_optimizer_ex constructor."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_opt2_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
