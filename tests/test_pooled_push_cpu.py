"""CPU tests of pooled pushes (pskv_apply_pooled): the symbol, the argument
checks made before the handle is looked at, the bag lookup of the kernels
replayed on the host (tests/cpp/pooled_push_plan_test.cpp, built with g++ and
also run under the host sanitizers as a stand-alone program), the teeth of the
checker of tests/pooled_push_util.py on the GPU tests' own inputs, and the proof
that the dyadic inputs are exact in float32.  No kernel is launched."""
import os
import re
import subprocess

import numpy as np
import pytest

import opt_util as ou
import pooled_push_util as ppu
from rows_util import LAYOUTS, bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build_and_run(tmp_path, name, extra):
    src = os.path.join(ROOT, "tests", "cpp", "pooled_push_plan_test.cpp")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra,
                        "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "parameter_server_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


def test_pooled_push_plan(tmp_path):
    _build_and_run(tmp_path, "pooled_push_plan_test", [])


def test_pooled_push_plan_under_host_sanitizers(tmp_path):
    """The same host-only program with AddressSanitizer and UBSan: a stand-alone
    executable, nothing loaded into Python."""
    _build_and_run(tmp_path, "pooled_push_plan_test_san",
                   ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_the_symbol_is_exported_and_declared():
    from parameter_server_amd import _lib

    assert "pskv_apply_pooled" in _lib.EXPORTED
    assert callable(_lib.lib.pskv_apply_pooled)
    with open(os.path.join(ROOT, "include", "pskv.h")) as f:
        txt = f.read()
    assert re.search(r"^int pskv_apply_pooled\(pskv_shard\* s, const uint32_t\* keys, uint64_t n,", txt, re.M)
    assert "Pooled pushes" in txt
    assert _lib.PSKV_K_COUNT == 14 and _lib.PSKV_TIME_APPLY == 1 << 14  # no new kernel id, no new slot


def _call(keys, n, weights, offsets, nbags, bag_grads, flags):
    from parameter_server_amd import _lib

    def ptr(a):
        return a.ctypes.data if a is not None else None

    rc = _lib.lib.pskv_apply_pooled(None, ptr(keys), n, ptr(weights), ptr(offsets), nbags, ptr(bag_grads), flags)
    return rc, _lib.lib.pskv_last_error().decode()


def test_apply_pooled_checks_its_arguments_before_the_handle():
    from parameter_server_amd import _lib

    keys = np.arange(7, dtype=np.uint32)
    bg = np.full(3 * 4, 9.0, dtype=np.float32)
    good = np.array([0, 3, 3, 7], dtype=np.uint64)
    # every argument holds: only the null shard is left to object to
    rc, msg = _call(keys, 7, None, good, 3, bg, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for off, bag, word in [(np.array([1, 3, 3, 7], dtype=np.uint64), 0, "offsets[0]"),
                           (np.array([0, 5, 4, 7], dtype=np.uint64), 1, "decrease"),
                           (np.array([0, 3, 3, 6], dtype=np.uint64), 2, "offsets[nbags]"),
                           (np.array([0, 3, 8, 8], dtype=np.uint64), 1, "past")]:
        rc, msg = _call(keys, 7, None, off, 3, bg, _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL, (off, rc, msg)
        assert "offsets" in msg and f"bag {bag}:" in msg and word in msg and "null shard" not in msg, msg
    # device offsets cannot be read: the same bad array gets as far as the handle
    rc, msg = _call(keys, 7, None, np.array([1, 3, 3, 7], dtype=np.uint64), 3, bg, _lib.PSKV_DEVICE)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for flags in (0x8, 0x100, _lib.PSKV_DEVICE | _lib.PSKV_HOST_FRAME):
        rc, msg = _call(keys, 7, None, good, 3, bg, flags)
        assert rc == _lib.PSKV_EINVAL and "flags" in msg, msg
    rc, msg = _call(None, 7, None, good, 3, bg, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null keys" in msg, msg
    rc, msg = _call(keys, 7, None, None, 3, bg, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null offsets" in msg, msg
    rc, msg = _call(keys, 7, None, good, 3, None, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null bag_grads" in msg, msg
    # more than 2^31 keys: refused on the count alone (device flags: no offset is read)
    rc, msg = _call(keys, 2**31 + 1, None, good, 3, bg, _lib.PSKV_DEVICE)
    assert rc == _lib.PSKV_EINVAL and "2^31" in msg and "null shard" not in msg, msg
    rc, msg = _call(keys, 2**31, None, good, 3, bg, _lib.PSKV_DEVICE)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    # no key, no bag: the null pointers are fine, the null shard is named
    rc, msg = _call(None, 0, None, None, 0, None, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    assert (bg == 9.0).all()


# ------------------------------------------------------- the checker's teeth
# the shapes of the derivation check (the issue's), each with both bag patterns
TEETH_SHAPES = [(2049, 3, "dups_in_chunk"), (4100, 16, "dups_across_chunks"), (2049, 4, "distinct"),
                (4100, 4, "dups_in_chunk")]


def _wrong_results(p, slots, idx, wts, bg, bag, dt, hp, rng):
    """Three wrong semantics, each as (name, p, slots) in dt: one element takes
    the next bag's row; the weights are ignored; one loser's term is dropped
    (a winner's where every key is distinct)."""
    out = []
    w = p.shape[1]
    rows = ppu.expand(wts, bg, bag, dt)
    # one element of one position takes the next (or previous) bag's row
    wrong_bag = rows.copy()
    i = int(rng.integers(0, idx.size))
    other = bag[i] + 1 if bag[i] + 1 < bg.shape[0] else bag[i] - 1
    col = int(rng.integers(0, w))
    wrong_bag[i, col] = (1.0 if wts is None else wts[i]) * bg[other, col]
    out.append(("next bag's row", wrong_bag, idx))
    out.append(("weights ignored", ppu.expand(None, bg, bag, dt), idx))
    m = np.bincount(idx, minlength=p.shape[0])
    dup = np.flatnonzero(m > 1)
    k = int(dup[0]) if dup.size else int(idx[0])
    first = int(np.flatnonzero(idx == k)[0])
    keep = np.ones(idx.size, dtype=bool)
    keep[first] = False
    dropped = rows.copy()
    dropped[first] = 0  # the key stays a key of the call: its term is lost, not its step
    out.append(("dropped term", dropped, idx))
    res = []
    for name, g, ix in out:
        pn, sn = ppu.emulate_any(p, slots, ix, g, dt, hp, 1, rng)
        res.append((name, pn, sn))
    return res


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,nesterov", ppu.KINDS)
def test_the_checker_accepts_the_kernel_order_and_rejects_wrong_semantics(kind, nesterov, dt):
    """On the GPU tests' inputs: an emulation of the kernels' order on the
    once-rounded products, in a random order, lies inside the tolerances;
    each of three wrong semantics lies outside."""
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[0]
    for wd in (0.0, 0.01):
        hp = ppu.hyper(kind, nesterov, wd)
        for n, w, pat in TEETH_SHAPES:
            for bagpat in ("eights", "mixed"):
                rng = np.random.default_rng(ou.case_seed("push", n, w, pat, bagpat, kind, nesterov, wd, dt.name))
                p = rng.standard_normal((ke - kb, w)).astype(dt)
                slots = ppu.initial_slots(kind, p.shape, dt)
                keys, off, bg, wts = ppu.draw_call(rng, n, w, pat, bagpat, kb, ke, dt, True)
                idx, bag = keys.astype(np.int64) - kb, ppu.bag_index(off)
                pre = ppu.prepare(p, slots, idx, wts, bg, bag, dt, hp)
                pn, sn = ppu.emulate_any(p, slots, idx, ppu.expand(wts, bg, bag, dt), dt, hp, 1, rng)
                tag = f"{kind} nesterov={nesterov} wd={wd} {(n, w, pat)} {bagpat}"
                assert not ppu.step_errors(p, slots, idx, wts, bg, bag, pn, sn, dt, hp, pre=pre), tag
                for name, wp, ws in _wrong_results(p, slots, idx, wts, bg, bag, dt, hp, rng):
                    assert ppu.step_errors(p, slots, idx, wts, bg, bag, wp, ws, dt, hp, pre=pre), f"{name} accepted: {tag}"


def test_unweighted_calls_keep_opt_utils_tolerances():
    """weights None: the tolerances are opt_util's own, m as it is."""
    dt = np.dtype(np.float32)
    kb, ke = LAYOUTS[0]
    rng = np.random.default_rng(5)
    hp = ppu.hyper("adagrad", wd=0.01)
    p = rng.standard_normal((ke - kb, 3)).astype(dt)
    slots = ppu.initial_slots("adagrad", p.shape, dt)
    keys, off, bg, _ = ppu.draw_call(rng, 2049, 3, "dups_in_chunk", "eights", kb, ke, dt, False)
    idx, bag = keys.astype(np.int64) - kb, ppu.bag_index(off)
    ref, tol_p, tol_s = ppu.prepare(p, slots, idx, None, bg, bag, dt, hp)
    ref0, tol_p0, tol_s0 = ou.prepare(p, slots, idx, bg[bag], dt, hp)
    assert np.array_equal(ref["m"], ref0["m"]) and np.array_equal(tol_p, tol_p0) and np.array_equal(tol_s[0], tol_s0[0])
    wts = np.ones(2049, dtype=dt)
    _, tol_pw, _ = ppu.prepare(p, slots, idx, wts, bg, bag, dt, hp)
    hit = ref["m"] > 0
    assert (tol_pw[hit] > tol_p[hit]).all()


# ------------------------------------------------------------------ dyadic
def test_dyadic_cases_are_exact_in_float32():
    """The dyadic inputs of tests/test_pooled_push_gpu.py: weights in {-2..2},
    bag rows multiples of 2^-4 in [-4, 4], so every product is a multiple of
    2^-4 in [-8, 8] (opt_util.dyadic_grads' values) and every partial sum of up
    to 4100 of them stays below 2^24 * 2^-4.  The longdouble reference of three
    steps is then representable in float32 (p and momentum's v), and a float32
    emulation in a random order returns the reference's bits."""
    dt = np.dtype(np.float32)
    kb, ke = LAYOUTS[0]
    for kind, nesterov, hp in [("sgd", False, ou.hyper("sgd", lr=ou.DYADIC_LR)), ("momentum", False, ou.dyadic_hyper(False)),
                               ("momentum", True, ou.dyadic_hyper(True))]:
        for n, w, pat, bagpat in [(4100, 1, "all_equal", "one_bag"), (4100, 4, "all_equal", "eights"),
                                  (4100, 3, "dups_in_chunk", "mixed"), (2049, 4, "dups_across_chunks", "boundary"),
                                  (2049, 5, "distinct", "ones")]:
            rng = np.random.default_rng(ou.case_seed("push-dyadic", n, w, pat, bagpat, kind, nesterov))
            p = ou.dyadic_params(rng, ke - kb, w, dt)
            slots = ou.zero_slots(kind, p.shape, dt)
            for t in range(1, 4):
                keys, off, bg, wts = ppu.draw_call(rng, n, w, pat, bagpat, kb, ke, dt, True, dyadic=True)
                idx, bag = keys.astype(np.int64) - kb, ppu.bag_index(off)
                rows = ppu.expand(wts, bg, bag, dt)
                exact = ppu.ref_grads(wts, bg, bag)
                assert np.array_equal(rows.astype(ou.F), exact)
                assert np.array_equal(exact * 16, np.round(exact * 16)) and np.abs(exact).max() <= 8
                ref = ou.step_ref(p, slots, idx, exact, hp, t)
                assert ref["G"].max() * 16 < 2**24
                for want in [ref["p"]] + ref["slots"]:
                    assert np.array_equal(want.astype(dt).astype(ou.F), want), (kind, n, w, pat, t)
                pn, sn = ppu.emulate_any(p, slots, idx, rows, dt, hp, t, rng)
                assert np.array_equal(bits(pn), bits(ref["p"].astype(dt)))
                for got, want in zip(sn, ref["slots"]):
                    assert np.array_equal(bits(got), bits(want.astype(dt)))
                p, slots = pn, sn
