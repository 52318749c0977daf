"""CPU tests of the factorization-machine pooled calls: the symbols, the
refusals that come before the handle, and the teeth of the push's tolerance
(tests/fm_util.py).  No kernel is launched."""
import os
import re
import subprocess

import numpy as np
import pytest

import fm_util as fu
import opt_util as ou
import pooled_push_util as ppu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_are_exported_and_declared():
    from parameter_server_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "parameter_server_amd", "libpskv.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pskv_\w+)", out))
    with open(os.path.join(ROOT, "include", "pskv.h")) as f:
        txt = f.read()
    for sym in ("pskv_get_pooled_fm", "pskv_apply_pooled_fm"):
        assert sym in exported and sym in _lib.EXPORTED and callable(getattr(_lib.lib, sym))
        assert re.search(rf"^int {sym}\(pskv_shard\* s, const uint32_t\* keys, uint64_t n,", txt, re.M)
    assert "Factorization-machine pooled calls" in txt
    assert _lib.lib.pskv_abi_version() == 1


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _pull(keys, n, offsets, nbags, out_sum, out_pair, flags):
    from parameter_server_amd import _lib

    rc = _lib.lib.pskv_get_pooled_fm(None, _ptr(keys), n, None, _ptr(offsets), nbags, _ptr(out_sum), _ptr(out_pair),
                                     flags)
    return rc, _lib.lib.pskv_last_error().decode()


def _push(keys, n, offsets, nbags, scale, grads, flags):
    from parameter_server_amd import _lib

    rc = _lib.lib.pskv_apply_pooled_fm(None, _ptr(keys), n, None, _ptr(offsets), nbags, _ptr(scale), _ptr(grads), flags)
    return rc, _lib.lib.pskv_last_error().decode()


@pytest.mark.parametrize("push", [False, True], ids=["pull", "push"])
def test_arguments_are_checked_before_the_handle(push):
    from parameter_server_amd import _lib

    keys = np.arange(7, dtype=np.uint32)
    rows = np.full(3 * 4, 9.0, dtype=np.float32)
    per_bag = np.full(3, 9.0, dtype=np.float32)
    good = np.array([0, 3, 3, 7], dtype=np.uint64)

    def call(k, n, off, nbags, last, flags):  # last: out_pair / bag_scale, the array that must not be null
        return _push(k, n, off, nbags, last, None, flags) if push else _pull(k, n, off, nbags, None, last, flags)

    # every argument holds, the optional array absent or present: only the null shard is left
    for rc, msg in (call(keys, 7, good, 3, per_bag, _lib.PSKV_HOST),
                    _push(keys, 7, good, 3, per_bag, rows, 0) if push else _pull(keys, 7, good, 3, rows, per_bag, 0)):
        assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for off, bag, word in [(np.array([1, 3, 3, 7], dtype=np.uint64), 0, "offsets[0]"),
                           (np.array([0, 5, 4, 7], dtype=np.uint64), 1, "decrease"),
                           (np.array([0, 3, 3, 6], dtype=np.uint64), 2, "offsets[nbags]"),
                           (np.array([0, 3, 8, 8], dtype=np.uint64), 1, "past")]:
        rc, msg = call(keys, 7, off, 3, per_bag, _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL and "offsets" in msg and f"bag {bag}:" in msg and word in msg, msg
        assert "null shard" not in msg, msg
    # device offsets cannot be read: the same bad array gets as far as the handle
    rc, msg = call(keys, 7, np.array([1, 3, 3, 7], dtype=np.uint64), 3, per_bag, _lib.PSKV_DEVICE)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for flags in (0x8, 0x100, _lib.PSKV_DEVICE | _lib.PSKV_HOST_FRAME):
        rc, msg = call(keys, 7, good, 3, per_bag, flags)
        assert rc == _lib.PSKV_EINVAL and "flags" in msg, msg
    for args, word in [((None, 7, good, 3, per_bag), "null keys"), ((keys, 7, None, 3, per_bag), "null offsets"),
                       ((keys, 7, good, 3, None), "null bag_scale" if push else "null out_pair")]:
        rc, msg = call(*args, _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL and word in msg and "null shard" not in msg, msg
    if push:  # more than 2^31 keys: refused on the count alone, as pskv_apply_pooled
        rc, msg = call(keys, 2**31 + 1, good, 3, per_bag, _lib.PSKV_DEVICE)
        assert rc == _lib.PSKV_EINVAL and "2^31" in msg and "null shard" not in msg, msg
    # nbags == 0 (and n == 0): null pointers pass every check; with a shard the
    # call is PSKV_OK (tests/test_fm_gpu.py), here the null shard is named
    rc, msg = call(None, 0, None, 0, None, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    assert (rows == 9.0).all() and (per_bag == 9.0).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["adagrad", "adam"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_the_push_tolerance_holds_the_emulation_and_rejects_a_late_read_of_s(weighted, kind, dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(ou.case_seed("fm-teeth", weighted, kind, dt.name))
    hp = ou.hyper(kind, wd=0.01)
    rows, w, lens = 12, 5, [3, 2, 9, 1, 0, 4]
    p = rng.standard_normal((rows, w)).astype(dt)
    slots = ppu.initial_slots(kind, p.shape, dt)
    idx, off, c, wts, bg = fu.draw_push(rng, rows, lens, w, dt, weighted, True, distinct=False)
    bag = ppu.bag_index(off)
    pre = fu.push_prepare(p, slots, idx, off, c, wts, bg, dt, hp)
    grads = fu.push_rows(p[idx], fu.sums_in(dt, p, idx, off, wts), bag, c, wts, bg)
    assert grads.dtype == dt
    for trial in range(4):  # the kernels' order, the losers in a random order
        p1, s1 = ou.emulate(p, slots, idx, grads, dt, hp, rng=rng)
        assert ou.step_errors(p, slots, idx, None, p1, s1, dt, hp, pre=pre) == [], trial
    # the rows of half the keys already stepped when S is read
    late = p.copy()
    late[: rows // 2] = p1[: rows // 2]
    wrong = fu.push_rows(p[idx], fu.sums_in(dt, late, idx, off, wts), bag, c, wts, bg)
    p2, s2 = ou.emulate(p, slots, idx, wrong, dt, hp)
    assert ou.step_errors(p, slots, idx, None, p2, s2, dt, hp, pre=pre) != []
