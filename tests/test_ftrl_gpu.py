"""GPU tests of FTRL-Proximal steps (pskv_shard_set_optimizer_cfg, PSKV_OPT_FTRL)
through every push form the library has.

Two bars (tests/ftrl_util.py):
  * random inputs (gradients of order 1, l1 = 0.5): the one-step check against
    an extended-precision step from the shard's own p, z and n, with the
    tolerances and the threshold band derived in DESIGN.md §8i, every element
    of the range, untouched rows bit-identical;
  * distinct keys: the push forms agree with each other bit for bit.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ftrl_util as fu
import opt_util as ou
import pooled_push_group_util as gu
import pooled_push_util as ppu
import pooled_util as pu
from rows_util import bits
from test_gpu_parity import tdev
from test_opt_gpu import all_keys, assert_bits, do_apply, read_p, rows_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = fu.F
DTYPES = [np.float32, np.float64]
# host and device apply, the device call with misaligned pointers (the element
# path), apply_grouped with 65 batches (two launch groups), apply_pooled
# weighted and with null weights, apply_pooled_grouped with 33 batches (two
# launch groups)
PATHS = ["host", "device", "device_unaligned", "host_grouped65", "device_grouped65", "pooled_host_weighted",
         "pooled_device_weighted", "pooled_host_null", "pooled_device_null", "pooled_device_unaligned",
         "pooled_grouped33_host", "pooled_grouped33_device"]
BAGPATS = ["eights", "mixed", "ones", "boundary", "one_bag"]


def make(rows, kb, dt, w, hp):
    import parameter_server_amd as ps

    sh = ps.Shard(kb, kb + rows, dt, width=w)
    fu.set_optimizer(sh, hp)
    return sh


def read_slots(sh):
    keys = all_keys(sh.key_begin, sh.key_end)
    return [rows_of(sh, sh.get_state(keys, slot=i)) for i in range(2)]


def state(sh):
    return [read_p(sh)] + read_slots(sh)


def assert_same_state(a, b, msg):
    for x, y, nm in zip(state(a), state(b), ["p", "z", "n"]):
        assert_bits(x, y, f"{msg}: {nm}")


def pooled_call(rng, keys, w, dt, weighted, bagpat):
    """(keys, offsets, bag_grads, weights) over the given keys: bag rows of order 1."""
    off = pu.offsets_of(ppu.bag_lens(bagpat, keys.size))
    bg = rng.standard_normal((off.size - 1, w)).astype(dt)
    wts = rng.standard_normal(keys.size).astype(dt) if weighted else None
    return keys, off, bg, wts


def pooled_batches(rng, keys, w, dt, nb):
    """The keys dealt over nb batches, weighted or not and the bag patterns rotating."""
    out = []
    for j, part in enumerate(np.array_split(keys, nb)):
        out.append(pooled_call(rng, part.copy(), w, dt, bool(j % 3), BAGPATS[j % 3]))
    return out


def push(sh, path, keys, grads, cuda, rng):
    """One step of `path` from the call (keys, grads); the pooled paths draw bag
    rows and weights of their own over the same keys.  Returns what the
    reference needs: (idx-ready keys, reference rows in longdouble, (R,) bool
    of the keys that carry the weight's extra rounding, or None)."""
    kb, rows, w, dt = sh.key_begin, sh.key_end - sh.key_begin, sh.width, sh.dtype
    if path in ("host", "device", "device_unaligned"):
        do_apply(sh, keys, grads, path, cuda)
        return keys, grads, None
    if path.endswith("grouped65"):
        batches = list(zip(np.array_split(keys, 65), np.array_split(grads, 65)))
        assert len(batches) == 65
        if path.startswith("device"):
            batches = [(tdev(k, cuda), tdev(g, cuda)) for k, g in batches]
        sh.apply_grouped(batches)
        return keys, grads, None
    if path.startswith("pooled_grouped33"):
        batches = pooled_batches(rng, keys, w, dt, 33)
        gu.apply_grouped(sh, batches, cuda if path.endswith("device") else None)
        return keys, gu.ref_rows(batches, w), gu.weighted_keys(batches, kb, rows)
    weighted = "weighted" in path or "unaligned" in path
    k, off, bg, wts = pooled_call(rng, keys, w, dt, weighted, BAGPATS[int(rng.integers(0, len(BAGPATS)))])
    ppu.apply_pooled(sh, k, off, bg, wts, None if "host" in path else cuda, bg_offset=1 if "unaligned" in path else 0)
    extra = np.zeros(rows, dtype=bool)
    if weighted:
        extra[k.astype(np.int64) - kb] = True
    return keys, ppu.ref_grads(wts, bg, ppu.bag_index(off)), extra


# ------------------------------------------------------------------ bounds
def _bound_params():
    out = []
    for ci in range(len(fu.BOUND_CASES)):
        for path in PATHS:
            for dt in DTYPES:  # (a case takes a tenth of a second)
                out.append(pytest.param(ci, dt, path,
                                        id=f"case{ci}-w{fu.BOUND_CASES[ci][3]}-{np.dtype(dt).name}-{path}"))
    return out


@pytest.mark.parametrize("ci,dt,path", _bound_params())
def test_steps_meet_the_one_step_bound(cuda, ci, dt, path):
    rows, kb, n, w, pat = fu.BOUND_CASES[ci]
    dt = np.dtype(dt)
    hp = fu.case_hyper(ci)
    p0, calls = fu.bound_steps(ci, dt)
    rng = np.random.default_rng(ou.case_seed("ftrl-gpu", ci, path))
    with make(rows, kb, dt, w, hp) as sh:
        sh.add(all_keys(kb, kb + rows), p0)
        z, nacc = read_slots(sh)
        assert not z.any(), "z starts at 0"
        assert_bits(nacc, np.full(p0.shape, hp["init_accum"], dtype=dt), "n starts at init_accum")
        for t, (keys, grads) in enumerate(calls, 1):
            p, slots = read_p(sh), read_slots(sh)
            k, ref_rows, extra = push(sh, path, keys, grads, cuda, rng)
            assert sh.step == t
            pre = fu.prepare(p, slots, k.astype(np.int64) - kb, ref_rows, dt, hp, m_extra=extra)
            got_p, got_s = read_p(sh), read_slots(sh)
            problems, band, checked = fu.step_report(p, slots, got_p, got_s, dt, hp, pre)
            print(f"{path} step {t}: checked {checked} band {band} zeros {int((bits(got_p) == 0).sum())}")
            fu.check_step(p, slots, None, None, got_p, got_s, dt, hp, pre=pre, msg=f"{path} step {t}")
        sh.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_thousands_of_occurrences_of_one_key(cuda, dt, device):
    """Dyadic gradients: the sum is exact in any order, so the m = 1 bounds hold
    (tests/test_ftrl_cpu.py shows that they notice one dropped gradient)."""
    dt = np.dtype(dt)
    hp = fu.hyper()
    p0, keys, grads, _ = fu.dyadic_many(dt)
    kb, rows, w = 5, p0.shape[0], p0.shape[1]
    with make(rows, kb, dt, w, hp) as sh:
        sh.add(all_keys(kb, kb + rows), p0)
        p, slots = read_p(sh), read_slots(sh)
        do_apply(sh, keys, grads, "device" if device else "host", cuda)
        fu.check_step(p, slots, keys.astype(np.int64) - kb, grads, read_p(sh), read_slots(sh), dt, hp, exact_sum=True,
                      msg="dyadic, m = 1 bounds")
        sh.sync()


# ------------------------------------------------------------ bit for bit
def _distinct_batches(rng, rows, kb, w, dt, sizes):
    return gu.draw_distinct_group(rng, sizes, w, kb, kb + rows, dt, c=1)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("w", [1, 3, 4, 16, 20])
def test_distinct_keys_the_push_forms_agree_bit_for_bit(cuda, w, dt):
    """apply_pooled equals apply of the host-expanded rows; apply_pooled_grouped
    equals apply_pooled of the concatenation; the same call on the same state
    twice gives the same bits.  Two steps each, host and device."""
    dt = np.dtype(dt)
    rows, kb = 4096, 2**31 - 2000
    hp = fu.hyper(wd=0.01)
    rng = np.random.default_rng(ou.case_seed("ftrl-bits", w, dt.name))
    p0 = rng.standard_normal((rows, w)).astype(dt)
    steps = [_distinct_batches(rng, rows, kb, w, dt, [2049, 7, 1500]) for _ in range(2)]
    for device in (False, True):
        dev = cuda if device else None
        with make(rows, kb, dt, w, hp) as a, make(rows, kb, dt, w, hp) as b, make(rows, kb, dt, w, hp) as c, \
                make(rows, kb, dt, w, hp) as d:
            for sh in (a, b, c, d):
                sh.add(all_keys(kb, kb + rows), p0)
            for t, batches in enumerate(steps, 1):
                keys, off, bg, wts = gu.concatenated(batches, dt)
                expanded = ppu.expand(wts, bg, ppu.bag_index(off), dt)
                gu.apply_grouped(a, batches, dev)
                ppu.apply_pooled(b, keys, off, bg, wts, dev)
                do_apply(c, keys, expanded, "device" if device else "host", cuda)
                ppu.apply_pooled(d, keys, off, bg, wts, dev)
                assert_same_state(a, b, f"grouped pooled against pooled, step {t}")
                assert_same_state(b, c, f"pooled against apply of the expanded rows, step {t}")
                assert_same_state(b, d, f"the same call twice, step {t}")
            touched = np.unique(np.concatenate([gu.indices(bt, kb) for bt in steps]))
            assert (bits(read_p(a))[touched] == 0).any() and (bits(read_p(a))[touched] != 0).any()
            for sh in (a, b, c, d):
                sh.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("w", [1, 4, 20])
def test_a_large_l1_makes_every_touched_element_plus_zero(cuda, w, dt):
    dt = np.dtype(dt)
    rows, kb, n = 1000, 100, 5000
    hp = fu.hyper(l1=1e6)
    rng = np.random.default_rng(ou.case_seed("ftrl-l1", w))
    p0 = rng.standard_normal((rows, w)).astype(dt)
    keys = (kb + rng.integers(0, rows // 2, size=n)).astype(np.uint32)  # the upper half stays untouched
    with make(rows, kb, dt, w, hp) as sh:
        sh.add(all_keys(kb, kb + rows), p0)
        for t in range(2):
            grads = (rng.standard_normal((n, w)) * np.where(rng.random((n, 1)) < 0.5, -1, 1)).astype(dt)
            do_apply(sh, keys, grads, ("device", "host")[t], cuda)
            got = read_p(sh)
            touched = np.unique(keys.astype(np.int64) - kb)
            assert not bits(got[touched]).any(), "a touched element is not the bit pattern +0 (a -0 counts)"
            assert_bits(got[rows // 2:], p0[rows // 2:], "untouched p")
        z, nacc = read_slots(sh)
        assert z[touched].any() and (nacc[touched] > hp["init_accum"]).all()  # the state goes on
        sh.sync()


def test_checkpoint_continues_bit_for_bit(cuda):
    dt = np.dtype(np.float32)
    rows, kb, w, n = 3000, 500, 4, 4100
    hp = fu.hyper(wd=0.01)
    rng = np.random.default_rng(113)
    calls = [((kb + rng.integers(0, rows, size=n)).astype(np.uint32), rng.standard_normal((n, w)).astype(dt))
             for _ in range(2)]
    third = ((kb + rng.permutation(rows)[:2049]).astype(np.uint32), rng.standard_normal((2049, w)).astype(dt))
    with make(rows, kb, dt, w, hp) as a, make(rows, kb, dt, w, hp) as b:
        a.add(all_keys(kb, kb + rows), rng.standard_normal((rows, w)).astype(dt))
        for k, g in calls:
            a.apply(tdev(k, cuda), tdev(g, cuda))
        d = a.state_dict()
        assert d["t"] == 2 and len(d["slots"]) == 2 and d["optimizer"]["kind"] == "ftrl"
        b.load_state_dict(d)
        assert b.step == 2
        assert_same_state(a, b, "restored")
        for sh in (a, b):
            sh.apply(third[0], third[1])
        assert a.step == b.step == 3
        assert_same_state(a, b, "after the third step")
        for sh in (a, b):
            sh.sync()


# --------------------------------------------------------- other behaviour
def test_clear_kind_change_and_the_same_kind_again(cuda):
    dt = np.dtype(np.float32)
    rows, kb, w = 2000, 1000, 4
    hp = fu.hyper()
    rng = np.random.default_rng(114)
    keys = (kb + rng.integers(0, rows, size=500)).astype(np.uint32)
    grads = rng.standard_normal((500, w)).astype(dt)
    full = lambda v: np.full((rows, w), v, dtype=dt)  # noqa: E731
    with make(rows, kb, dt, w, hp) as sh:
        assert sh.step == 0
        sh.apply(keys, grads)
        sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        assert sh.step == 2
        before = state(sh)
        assert before[1].any() and (before[2] > np.float32(hp["init_accum"])).any()
        # the same kind with new hyper-parameters keeps z, n and t
        sh.set_optimizer("ftrl", lr=0.1, l1=0.25, l2=0.0, ftrl_beta=2.0, init_accum=0.7)
        assert sh.step == 2
        o = sh.optimizer()
        assert (o["kind"], o["lr"], o["l1"], o["l2"], o["ftrl_beta"], o["init_accum"]) == ("ftrl", 0.1, 0.25, 0.0, 2.0,
                                                                                          0.7)
        for x, y, nm in zip(state(sh), before, "pzn"):
            assert_bits(x, y, f"the same kind again changed {nm}")
        # clear: z to 0, n to the new init_accum, t to 0; the next step is a first step
        sh.clear()
        sh.sync()
        assert sh.step == 0
        p, z, nacc = state(sh)
        assert not bits(p).any() and not bits(z).any()
        assert_bits(nacc, full(0.7), "n after clear")
        hp2 = fu.hyper(lr=0.1, l1=0.25, l2=0.0, beta=2.0, init_accum=0.7)
        sh.apply(keys, grads)
        assert sh.step == 1
        fu.check_step(p, [z, nacc], keys.astype(np.int64) - kb, grads, read_p(sh), read_slots(sh), dt, hp2,
                      msg="the step after clear")
        # another kind resets the state and t, and back again
        sh.set_optimizer("adam", lr=0.001)
        assert sh.step == 0
        assert not sh.get_state(all_keys(kb, kb + rows), slot=1).any()
        sh.apply(keys, grads)
        assert sh.step == 1
        fu.set_optimizer(sh, hp)
        assert sh.step == 0
        z, nacc = read_slots(sh)
        assert not bits(z).any()
        assert_bits(nacc, full(hp["init_accum"]), "n after a kind change")
        sh.sync()


def test_out_of_range_keys(cuda):
    from parameter_server_amd import _lib

    dt = np.dtype(np.float32)
    rows, kb, w = 2000, 1000, 4
    hp = fu.hyper()
    rng = np.random.default_rng(115)
    keys = (kb + rng.integers(0, rows, size=500)).astype(np.uint32)
    grads = rng.standard_normal((500, w)).astype(dt)
    bad = keys.copy()
    bad[77], bad[300] = 3007, 12  # outside on both sides
    inside = (bad >= kb) & (bad < kb + rows)
    with make(rows, kb, dt, w, hp) as sh:
        sh.add(all_keys(kb, kb + rows), rng.standard_normal((rows, w)).astype(dt))
        sh.apply(keys, grads)
        before = state(sh)
        with pytest.raises(_lib.PskvError) as e:
            sh.apply(bad, grads)
        assert e.value.code == _lib.PSKV_EINVAL and "3007" in str(e.value)
        assert sh.step == 1
        for x, y, nm in zip(state(sh), before, "pzn"):
            assert_bits(x, y, f"a refused host apply changed {nm}")
        sh.apply(tdev(bad, cuda), tdev(grads, cuda))
        assert sh.step == 2
        fu.check_step(before[0], before[1:], bad[inside].astype(np.int64) - kb, grads[inside], read_p(sh),
                      read_slots(sh), dt, hp, msg="device apply with out-of-range keys")
        with pytest.raises(_lib.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE and "out-of-range" in str(e.value)
        sh.clear()
        sh.sync()


def test_getters_and_state_bytes(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    rows, kb, w = 3000, 0, 4
    dense, stamps = rows * w * 4, 8 * rows
    with ps.Shard(kb, kb + rows, np.float32, width=w) as sh:
        sh.set_optimizer("ftrl", lr=0.05, l1=0.5)
        o = sh.optimizer()
        assert o == {"kind": "ftrl", "lr": 0.05, "weight_decay": 0.0, "eps": 1e-10, "init_accum": 0.1, "l1": 0.5,
                     "l2": 0.0, "ftrl_beta": 1.0, "state_bytes": 3 * dense + stamps}
        old, nb = _lib.PskvOptimizer(), ctypes.c_uint64()
        _lib.check(_lib.lib.pskv_shard_get_optimizer(sh.handle, ctypes.byref(old), ctypes.byref(nb)))
        assert (old.kind, old.lr, old.init_accum, nb.value) == (_lib.PSKV_OPT_FTRL, 0.05, 0.1, 3 * dense + stamps)
        ex = _lib.PskvOptimizerEx()
        _lib.check(_lib.lib.pskv_shard_get_optimizer_ex(sh.handle, ctypes.byref(ex), ctypes.byref(nb)))
        assert (ex.size, ex.kind, ex.lr, ex.init_accum, nb.value) == (72, 5, 0.05, 0.1, 3 * dense + stamps)
        cfg = _lib.PskvOptimizerCfg()
        _lib.check(_lib.lib.pskv_shard_get_optimizer_cfg(sh.handle, ctypes.byref(cfg), None))
        assert (cfg.size, cfg.kind, cfg.l1, cfg.l2, cfg.ftrl_beta) == (96, 5, 0.5, 0.0, 1.0)
        # slots 0 and 1, no slot 2; pskv_get_state keeps its Adagrad-only meaning
        keys = np.array([0, 2999, 1500], dtype=np.uint32)
        vals = np.arange(12, dtype=np.float32).reshape(3, w)
        for slot in (0, 1):
            sh.put_state(keys, vals + slot, slot=slot)
            assert np.array_equal(sh.get_state(keys, slot=slot), vals + slot)
        for call in (lambda: sh.get_state(keys, slot=2), lambda: sh.put_state(keys, vals, slot=2)):
            with pytest.raises(_lib.PskvError) as e:
                call()
            assert e.value.code == _lib.PSKV_EINVAL and "slot" in str(e.value)
        out = np.empty((3, w), dtype=np.float32)
        assert _lib.lib.pskv_get_state(sh.handle, keys.ctypes.data, 3, out.ctypes.data, 0) == _lib.PSKV_EINVAL
        # the older kinds through the new setter are the older setters
        x = _lib.PskvOptimizerCfg(96, _lib.PSKV_OPT_ADAGRAD, 0.05, 0.0, 1e-8, 0.5, 0.0, 0, 0.0, 0.0, -1.0, -1.0, -1.0)
        _lib.check(_lib.lib.pskv_shard_set_optimizer_cfg(sh.handle, ctypes.byref(x)))
        assert sh.optimizer() == {"kind": "adagrad", "lr": 0.05, "weight_decay": 0.0, "eps": 1e-8, "init_accum": 0.5,
                                  "state_bytes": 2 * dense + stamps}
        sh.sync()
    with ps.Shard(kb, kb + rows, np.int32) as si:
        with pytest.raises(_lib.PskvError) as e:
            si.set_optimizer("ftrl", lr=0.1)
        assert e.value.code == _lib.PSKV_EINVAL and "float" in str(e.value)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_zero_gradient_key_still_takes_a_step(cuda, device):
    """FTRL owns p: a key of the call whose gradient is zero gets the closed form
    of its (unchanged) z, here +0 in the place of the p an Add wrote; z and n
    keep their bits, and a key not in the call keeps everything."""
    dt = np.dtype(np.float32)
    rows, kb, w = 64, 10, 3
    hp = fu.hyper()
    p0 = np.arange(1, rows * w + 1, dtype=dt).reshape(rows, w)
    keys = np.array([kb + 3, kb + 40], dtype=np.uint32)
    grads = np.zeros((2, w), dtype=dt)
    with make(rows, kb, dt, w, hp) as sh:
        sh.add(all_keys(kb, kb + rows), p0)
        before = state(sh)
        if device:
            sh.apply(tdev(keys, cuda), tdev(grads, cuda))
        else:
            sh.apply(keys, grads)
        assert sh.step == 1
        p, z, nacc = state(sh)
        fu.check_step(before[0], before[1:], keys.astype(np.int64) - kb, grads, p, [z, nacc], dt, hp, msg="zero rows")
        assert not bits(p[[3, 40]]).any()
        assert_bits(z, before[1], "z")
        assert_bits(nacc, before[2], "n")
        sh.sync()


def test_hip_storage_with_an_ftrl_optimizer(cuda):
    """parameter_server_amd.storage.HipStorage hands its optimizer dict to
    Shard.set_optimizer: two Adds are two steps, AddGrouped of the two is one."""
    from parameter_server_amd.storage import Flag, HipStorage, Message, typed

    w = 4
    opt = dict(kind="ftrl", lr=1.0, l1=0.0, l2=0.0, ftrl_beta=0.0, init_accum=0.0)
    keys = np.array([5, 9], dtype=np.uint32)
    g1 = np.array([[3.0] * w, [6.0] * w], dtype=np.float32)
    g2 = np.array([[4.0] * w, [8.0] * w], dtype=np.float32)

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

    st = HipStorage(np.float32, 0, 100, width=w, optimizer=opt)
    try:
        st.Add(msg(keys, g1))
        st.Add(msg(keys, g2))
        got = pull(st)
        assert np.allclose(got[:2], -1.8, rtol=3e-7, atol=0) and not got[2].any()
        assert st.shard.step == 2
        st.FinishIter()
    finally:
        st.close()
    st = HipStorage(np.float32, 0, 100, width=w, optimizer=opt)
    try:
        st.AddGrouped([msg(keys, g1), msg(keys, g2)])
        got = pull(st)
        assert np.array_equal(got[:2], np.full((2, w), -1.0, dtype=np.float32)) and not got[2].any()
        assert st.shard.step == 1
        st.FinishIter()
    finally:
        st.close()


def test_cpp_ftrl_program(cuda):
    """tests/cpp/hip_storage_ftrl_test.cpp: HipStorage<float> with an FTRL
    optimizer through the pskv_optimizer_cfg constructor."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_ftrl_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
