"""GPU tests of pooled pushes (pskv_apply_pooled, Shard.apply_pooled): one
gradient row per bag, expanded in the shard inside the optimizer step.

Three bars (tests/pooled_push_util.py):
  * random inputs, every optimizer kind: the one-step check against a
    longdouble step from the shard's own state, opt_util's tolerances with
    m + 1 for m when the call is weighted (derived; tests/test_pooled_push_cpu.py
    proves the checker's teeth on these inputs);
  * distinct keys: a twin shard that takes pskv_apply of the host-expanded
    rows must hold the same bits, p, every slot and the step;
  * dyadic inputs (exact in float32, proven on the CPU): bit-equal to the twin
    and to the reference with duplicated keys too.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
from rows_util import LAYOUTS, bits, key_patterns
from test_gpu_parity import tdev
from test_opt_gpu import all_keys, assert_bits, read_p
from test_opt2_gpu import read_slots

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 3), (2049, 1), (2049, 3), (2049, 4), (4100, 16), (4100, 33), (2049, 64), (4100, 100)]
PATTERNS = ["distinct", "dups_in_chunk", "dups_across_chunks", "range_ends"]
# every (key pattern, bag pattern, weighted, device) combination, in a fixed shuffled order
COMBOS = list(itertools.product(PATTERNS, ppu.BAG_PATTERNS, (False, True), (False, True)))
np.random.default_rng(2024).shuffle(COMBOS)
DTYPES = [np.float32, np.float64]


def make(kb, ke, dt, w, hp=None, **kw):
    import parameter_server_amd as ps

    sh = ps.Shard(kb, ke, dt, width=w, **kw)
    if hp is not None:
        ppu.set_optimizer(sh, hp)
    return sh


def slots_of(sh, hp):
    return read_slots(sh, hp["kind"])


def assert_same_state(a, b, hp, msg):
    assert_bits(read_p(a), read_p(b), f"p {msg}")
    for i, (x, y) in enumerate(zip(slots_of(a, hp), slots_of(b, hp))):
        assert_bits(x, y, f"slot {i} {msg}")
    assert a.step == b.step, msg


# ------------------------------------------------------ against the reference
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"{n}x{w}" for n, w in SHAPES])
@pytest.mark.parametrize("li", range(len(LAYOUTS)), ids=["low", "straddle"])
def test_steps_meet_the_one_step_bound(cuda, li, si, dt):
    """Every kind, three consecutive steps each; the key pattern, the bag
    pattern, weighted or not, host or device path and the weight decay rotate
    through every combination over the cases."""
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[li]
    n, w = SHAPES[si]
    rng = np.random.default_rng(ou.case_seed("push-gpu", li, si, dt.name))
    c = (li * len(SHAPES) + si) * 2 + (dt.itemsize == 8)
    for ki, (kind, nesterov) in enumerate(ppu.KINDS):
        hp = ppu.hyper(kind, nesterov, wd=(0.0, 0.01)[(c + ki) % 2])
        with make(kb, ke, dt, w, hp) as sh:
            sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
            for t in range(1, 4):
                pat, bagpat, weighted, device = COMBOS[(c * 15 + ki * 3 + t) % len(COMBOS)]
                if pat == "distinct" and n > ke - kb:
                    pat = "range_ends"
                keys, off, bg, wts = ppu.draw_call(rng, n, w, pat, bagpat, kb, ke, dt, weighted)
                p, slots = read_p(sh), slots_of(sh, hp)
                ppu.apply_pooled(sh, keys, off, bg, wts, cuda if device else None)
                assert sh.step == t
                ppu.check_step(p, slots, keys.astype(np.int64) - kb, wts, bg, ppu.bag_index(off), read_p(sh),
                               slots_of(sh, hp), dt, hp, t,
                               msg=f"{kind} nesterov={nesterov} wd={hp['wd']} {pat} {bagpat} weighted={weighted} "
                                   f"device={device} step {t}")
            sh.sync()


# ------------------------------------- distinct keys: pskv_apply's bits
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("w", [1, 4, 5])
@pytest.mark.parametrize("kind,nesterov", ppu.KINDS)
def test_distinct_keys_equal_apply_bit_for_bit(cuda, kind, nesterov, w, dt):
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[0]
    hp = ppu.hyper(kind, nesterov, wd=0.01)
    rng = np.random.default_rng(ou.case_seed("push-twin", kind, nesterov, w, dt.name))
    p0 = rng.standard_normal((ke - kb, w)).astype(dt)
    for weighted in (False, True):
        with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b:
            for sh in (a, b):
                sh.add(all_keys(kb, ke), p0)
            for t in range(1, 4):
                bagpat = ppu.BAG_PATTERNS[(t + w) % len(ppu.BAG_PATTERNS)]
                keys, off, bg, wts = ppu.draw_call(rng, 4100, w, "distinct", bagpat, kb, ke, dt, weighted)
                rows = ppu.expand(wts, bg, ppu.bag_index(off), dt)
                device = bool(t % 2)
                ppu.apply_pooled(a, keys, off, bg, wts, cuda if device else None)
                if device:
                    b.apply(tdev(keys, cuda), tdev(rows, cuda))
                else:
                    b.apply(keys, rows)
                assert_same_state(a, b, hp, f"weighted={weighted} step {t} {bagpat} device={device}")
            a.sync()
            b.sync()


# ---------------------------------------------- dyadic, duplicated keys
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,w,pat,bagpat", [(4100, 1, "all_equal", "one_bag"), (4100, 4, "all_equal", "eights"),
                                            (4100, 3, "dups_in_chunk", "mixed"),
                                            (2049, 4, "dups_across_chunks", "boundary"), (2049, 5, "distinct", "ones")])
@pytest.mark.parametrize("kind,nesterov", [("sgd", False), ("momentum", False), ("momentum", True)])
def test_dyadic_duplicates_are_bit_exact(cuda, kind, nesterov, n, w, pat, bagpat, dt):
    """(the inputs of test_pooled_push_cpu.py's exactness proof)"""
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[0]
    hp = ou.hyper("sgd", lr=ou.DYADIC_LR) if kind == "sgd" else ou.dyadic_hyper(nesterov)
    rng = np.random.default_rng(ou.case_seed("push-dyadic", n, w, pat, bagpat, kind, nesterov))
    p = ou.dyadic_params(rng, ke - kb, w, dt)
    slots = ou.zero_slots(kind, p.shape, dt)
    with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b:
        for sh in (a, b):
            sh.add(all_keys(kb, ke), p)
        for t in range(1, 4):
            keys, off, bg, wts = ppu.draw_call(rng, n, w, pat, bagpat, kb, ke, dt, True, dyadic=True)
            bag = ppu.bag_index(off)
            device = bool(t % 2)
            ppu.apply_pooled(a, keys, off, bg, wts, cuda if device else None)
            b.apply(tdev(keys, cuda), tdev(ppu.expand(wts, bg, bag, dt), cuda))
            ref = ou.step_ref(p, slots, keys.astype(np.int64) - kb, ppu.ref_grads(wts, bg, bag), hp, t)
            p, slots = ref["p"].astype(dt), [s.astype(dt) for s in ref["slots"]]
            assert_bits(read_p(a), p, f"p against the reference, step {t}")
            for i, s in enumerate(slots):
                assert_bits(slots_of(a, hp)[i], s, f"slot {i} against the reference, step {t}")
            assert_same_state(a, b, hp, f"against the twin, step {t}")
        a.sync()
        b.sync()


# ------------------------------------------------------------- unit paths
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["sgd", "momentum"])
def test_unit_16_and_element_path_give_the_same_bits(cuda, kind, dt):
    """W = 4: 16-byte-aligned bag rows take the 16-byte units, bag rows one
    element off take the element path; dyadic inputs make both exact."""
    dt = np.dtype(dt)
    kb, ke, w = 0, 5000, 4
    hp = ou.hyper("sgd", lr=ou.DYADIC_LR) if kind == "sgd" else ou.dyadic_hyper(False)
    rng = np.random.default_rng(31)
    p0 = ou.dyadic_params(rng, ke - kb, w, dt)
    keys, off, bg, wts = ppu.draw_call(rng, 4100, w, "dups_in_chunk", "mixed", kb, ke, dt, True, dyadic=True)
    with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b:
        for sh, shift in ((a, 0), (b, 1)):
            sh.add(all_keys(kb, ke), p0)
            ppu.apply_pooled(sh, keys, off, bg, wts, cuda, bg_offset=shift)
        assert_same_state(a, b, hp, "aligned against one element off")
        ref = ou.step_ref(p0, ou.zero_slots(kind, p0.shape, dt), keys.astype(np.int64) - kb,
                          ppu.ref_grads(wts, bg, ppu.bag_index(off)), hp)
        assert_bits(read_p(a), ref["p"].astype(dt), "against the reference")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_max_width(cuda, dt):
    from parameter_server_amd import _lib

    dt = np.dtype(dt)
    w, kb, ke = _lib.PSKV_MAX_WIDTH, 10, 40
    hp = ppu.hyper("adam", wd=0.01)
    rng = np.random.default_rng(3)
    lens = [5, 0, 9]
    off, keys = pu.offsets_of(lens), pu.draw_keys(rng, lens, kb, ke)
    with make(kb, ke, dt, w, hp) as sh:
        sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        for t, (weighted, device) in enumerate([(False, True), (True, False), (True, True)], 1):
            bg = (rng.standard_normal((3, w)) * 3).astype(dt)
            wts = rng.standard_normal(keys.size).astype(dt) if weighted else None
            p, slots = read_p(sh), slots_of(sh, hp)
            ppu.apply_pooled(sh, keys, off, bg, wts, cuda if device else None)
            ppu.check_step(p, slots, keys.astype(np.int64) - kb, wts, bg, ppu.bag_index(off), read_p(sh),
                           slots_of(sh, hp), dt, hp, t, msg=f"max width step {t}")
        sh.sync()


def test_gsum_is_zero_again_after_a_pooled_push(cuda):
    """After a pooled push with duplicates an ordinary apply on the same shard
    meets the reference: the gradient scratch is back to zero."""
    dt = np.dtype(np.float32)
    kb, ke, w = 0, 5000, 16
    hp = ppu.hyper("adagrad", wd=0.01)
    rng = np.random.default_rng(41)
    with make(kb, ke, dt, w, hp) as sh:
        sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        keys, off, bg, wts = ppu.draw_call(rng, 4100, w, "dups_in_chunk", "eights", kb, ke, dt, True)
        ppu.apply_pooled(sh, keys, off, bg, wts, cuda)
        k2 = key_patterns(rng, 4100, kb, ke)["dups_across_chunks"]
        g2 = (rng.standard_normal((4100, w)) * 3).astype(dt)
        p, slots = read_p(sh), slots_of(sh, hp)
        sh.apply(tdev(k2, cuda), tdev(g2, cuda))
        ou.check_step(p, slots, k2.astype(np.int64) - kb, g2, read_p(sh), slots_of(sh, hp), dt, hp, 2, msg="apply")
        sh.sync()


# ------------------------------------------------------- out-of-range keys
@pytest.mark.parametrize("w", [1, 16])
def test_out_of_range_keys(cuda, w):
    from parameter_server_amd import _lib

    kb, ke = 1000, 3000
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(60 + w)
    p0 = ou.dyadic_params(rng, ke - kb, w, dt)
    keys, off, bg, wts = ppu.draw_call(rng, 500, w, "dups_in_chunk", "eights", kb, ke, dt, True, dyadic=True)
    keys[77], keys[300] = 3007, 12  # outside on both sides
    hp = ou.hyper("adagrad", lr=2.0**-3, eps=1e-10)
    with make(kb, ke, dt, w) as sh:
        sh.set_optimizer("adagrad", lr=2.0**-3, init_accum=0.5)
        sh.add(all_keys(kb, ke), p0)
        h0 = slots_of(sh, hp)[0]
        with pytest.raises(_lib.PskvError) as e:
            sh.apply_pooled(keys, off, bg, wts)
        assert e.value.code == _lib.PSKV_EINVAL and "3007" in str(e.value)
        assert_bits(read_p(sh), p0, "a refused host pooled push changed p")
        assert_bits(slots_of(sh, hp)[0], h0, "a refused host pooled push changed h")
        assert sh.step == 0
        sh.sync()
        # device: the in-range keys are applied, the others dropped and reported
        sh.set_optimizer("sgd", lr=2.0**-3)
        ppu.apply_pooled(sh, keys, off, bg, wts, cuda)
        inside = (keys >= kb) & (keys < ke)
        rows = ppu.ref_grads(wts, bg, ppu.bag_index(off))
        want = ou.step_ref(p0, [], keys[inside].astype(np.int64) - kb, rows[inside], ou.hyper("sgd", lr=2.0**-3))["p"]
        assert_bits(read_p(sh), want.astype(dt), "device pooled push with out-of-range keys")
        assert sh.step == 1
        with pytest.raises(_lib.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE and "out-of-range" in str(e.value)
        sh.clear()
        sh.sync()


def test_refusals_leave_the_step(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    keys = np.arange(7, dtype=np.uint32)
    off = pu.offsets_of([3, 0, 4])
    with ps.Shard(0, 100, np.float32, width=2) as sh:  # no optimizer
        with pytest.raises(_lib.PskvError) as e:
            sh.apply_pooled(keys, off, np.ones((3, 2), np.float32))
        assert e.value.code == _lib.PSKV_EINVAL and "no optimizer" in str(e.value)
        assert sh.step == 0
        sh.set_optimizer("sgd", lr=0.5)
        rc = _lib.lib.pskv_apply_pooled(sh._h, keys.ctypes.data, 7, None, off.ctypes.data, 3, None, _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL and "null bag_grads" in _lib.lib.pskv_last_error().decode()
        assert sh.step == 0 and not read_p(sh).any()
    with ps.Shard(0, 100, np.int32, width=2) as sh:
        bg = np.ones((3, 2), np.int32)
        rc = _lib.lib.pskv_apply_pooled(sh._h, keys.ctypes.data, 7, None, off.ctypes.data, 3, bg.ctypes.data,
                                        _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL and "float shards only" in _lib.lib.pskv_last_error().decode()
        assert sh.step == 0
        sh.sync()


# ------------------------------------------------ step counter and restore
def test_empty_calls_do_not_advance_the_step(cuda):
    import torch

    with make(0, 100, np.float32, 3, ppu.hyper("adam")) as sh:
        p0 = read_p(sh)
        none_k, none_g = np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)
        sh.apply_pooled(none_k, pu.offsets_of([]), none_g)                               # n == 0, nbags == 0
        sh.apply_pooled(none_k, pu.offsets_of([0, 0]), np.ones((2, 3), np.float32))      # n == 0, two empty bags
        sh.apply_pooled(torch.zeros(0, dtype=torch.int32, device=cuda),
                        torch.zeros(3, dtype=torch.int64, device=cuda), torch.ones((2, 3), device=cuda))
        sh.apply_pooled(tdev(np.arange(4, dtype=np.uint32), cuda), torch.zeros(1, dtype=torch.int64, device=cuda),
                        torch.zeros((0, 3), device=cuda))                                # nbags == 0 with keys
        assert sh.step == 0
        assert_bits(read_p(sh), p0, "empty calls")
        sh.sync()


def test_checkpoint_restores_bit_for_bit(cuda):
    dt = np.dtype(np.float32)
    kb, ke, w = 0, 3000, 4
    hp = ppu.hyper("adam", wd=0.01)
    rng = np.random.default_rng(71)
    calls = [ppu.draw_call(rng, 2049, w, "dups_in_chunk", bp, kb, ke, dt, True) for bp in ("mixed", "eights", "boundary")]
    with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b:
        a.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        for keys, off, bg, wts in calls[:2]:
            ppu.apply_pooled(a, keys, off, bg, wts, cuda)
        b.load_state_dict(a.state_dict())
        assert b.step == 2
        keys, off, bg, wts = calls[2]
        # (duplicated keys: the sums' order is unspecified, so the third push runs on distinct keys)
        keys = key_patterns(rng, 2049, kb, ke)["distinct"]
        for sh in (a, b):
            ppu.apply_pooled(sh, keys, off, bg, wts, cuda)
        assert_same_state(a, b, hp, "after the restore")


# ------------------------------------------------------- width 1, ordering
def test_pooled_push_orders_against_small_host_adds_and_gets(cuda):
    """A width-1 shard at default options: small host Adds and Gets travel in
    kernel arguments (K8); pooled pushes between them see what they wrote, and
    they see the pushes."""
    kb, ke = 0, 5000
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(55)
    keys = np.arange(100, 300, dtype=np.uint32)
    p = np.zeros((ke - kb, 1))
    hp = ou.hyper("sgd", lr=ou.DYADIC_LR)
    with make(kb, ke, dt, 1, hp) as sh:
        for step in range(3):
            vals = ou.dyadic_params(rng, keys.size, 1, dt)
            sh.add(keys, vals.reshape(-1))
            p[keys.astype(np.int64) - kb] = vals
            k = (kb + rng.integers(50, 350, size=400)).astype(np.uint32)
            off = pu.offsets_of(ppu.bag_lens("eights", 400))
            bg = (rng.integers(-64, 65, size=(50, 1)) / 16.0).astype(dt)
            wts = rng.integers(-2, 3, size=400).astype(dt)
            ppu.apply_pooled(sh, k, off, bg, wts, cuda if step % 2 == 0 else None)
            p = ou.step_ref(p, [], k.astype(np.int64) - kb, ppu.ref_grads(wts, bg, ppu.bag_index(off)), hp)["p"]
            q = np.arange(0, 400, dtype=np.uint32)
            assert_bits(sh.get(q).reshape(-1, 1), p[:400].astype(dt), f"step {step}")
        sh.sync()


def test_timing_slot(cuda):
    from parameter_server_amd import _lib

    kb, ke, w = 0, 3000, 4
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(81)
    with make(kb, ke, dt, w, ppu.hyper("adagrad")) as sh:
        sh.sync()
        sh.set_timing(True)
        sh.reset_timing()
        before = {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)}
        total = 0
        for n, device in ((2049, True), (4100, True), (300, False)):
            keys, off, bg, wts = ppu.draw_call(rng, n, w, "dups_in_chunk", "mixed", kb, ke, dt, True)
            ppu.apply_pooled(sh, keys, off, bg, wts, cuda if device else None)
            total += n
        sh.sync()
        t = sh.apply_time()
        assert t["launches"] == 3 and t["elements"] == total and t["total_ms"] > 0, t
        assert {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)} == before
        assert sh.pooled_time()["launches"] == 0


# ------------------------------------------------ malformed device offsets
@pytest.mark.parametrize("w", [1, 4, 33])
def test_malformed_device_offsets_touch_only_the_calls_keys(cuda, w):
    """The call returns, sync succeeds and every key not in `keys` keeps its
    bits; what the call's keys hold is unspecified and not compared."""
    import torch

    dt = np.dtype(np.float32)
    kb, ke, n = 0, 5000, 4100
    rng = np.random.default_rng(91 + w)
    with make(kb, ke, dt, w, ppu.hyper("adam", wd=0.01)) as sh:
        sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        keys = (kb + rng.integers(0, 2000, size=n)).astype(np.uint32)  # keys 2000.. are not in the call
        nbags = 300
        bad = [np.arange(nbags + 1)[::-1] * 13,                        # decreasing
               np.arange(nbags + 1) * 1000 + n,                        # beyond n
               np.concatenate([[5], np.sort(rng.integers(5, n, size=nbags - 1)), [n]]),  # offsets[0] != 0
               rng.integers(0, 2**62, size=nbags + 1)]                 # anything
        for off in bad:
            p, slots = read_p(sh), slots_of(sh, {"kind": "adam"})
            bg = (rng.standard_normal((nbags, w)) * 3).astype(dt)
            wts = rng.standard_normal(n).astype(dt)
            sh.apply_pooled(tdev(keys, cuda), torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(cuda),
                            tdev(bg, cuda), tdev(wts, cuda))
            sh.sync()
            untouched = np.ones(ke - kb, dtype=bool)
            untouched[keys.astype(np.int64) - kb] = False
            assert np.array_equal(bits(read_p(sh)[untouched]), bits(p[untouched]))
            for a, b in zip(slots_of(sh, {"kind": "adam"}), slots):
                assert np.array_equal(bits(a[untouched]), bits(b[untouched]))


def test_width_one_with_the_request_server(cuda):
    """SERVE = 1: the pooled push first ends the server; small host Gets see it."""
    kb, ke = 0, 4000
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(10)
    hp = ou.hyper("sgd", lr=ou.DYADIC_LR)
    with make(kb, ke, dt, 1, hp, options={"SERVE": 1}) as sh:
        p = ou.dyadic_params(rng, ke - kb, 1, dt)
        sh.add(all_keys(kb, ke), p.reshape(-1))
        small = rng.integers(kb, ke, size=20).astype(np.uint32)
        assert np.array_equal(sh.get(small), p[small, 0])  # (a small host Get: the server's)
        for device in (True, False):
            keys, off, bg, wts = ppu.draw_call(rng, 2049, 1, "dups_in_chunk", "mixed", kb, ke, dt, True, dyadic=True)
            ppu.apply_pooled(sh, keys, off, bg, wts, cuda if device else None)
            p = ou.step_ref(p, [], keys.astype(np.int64) - kb, ppu.ref_grads(wts, bg, ppu.bag_index(off)),
                            hp)["p"].astype(dt)
            assert np.array_equal(bits(sh.get(small)), bits(p[small, 0]))
        sh.sync()


def test_cpp_pooled_push_program(cuda):
    """tests/cpp/hip_storage_pooled_push_test.cpp: SubGetPooled, SubApplyPooled,
    SubGet through HipStorage<float> and <double> with Adagrad."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_pooled_push_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
