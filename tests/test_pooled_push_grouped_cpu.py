"""CPU tests of grouped pooled pushes (pskv_apply_pooled_grouped): the symbol,
the argument checks made before the handle is looked at (every message names
the batch), the planner and the kernels' per-batch lookup replayed on the host
(tests/cpp/pooled_push_group_plan_test.cpp, built with g++ and also run under
the host sanitizers as a stand-alone program), and the teeth of the checker of
tests/pooled_push_group_util.py for the two hazards a grouped call adds.  No
kernel is launched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import opt_util as ou
import pooled_push_group_util as gu
import pooled_push_util as ppu
from rows_util import LAYOUTS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build_and_run(tmp_path, name, extra):
    src = os.path.join(ROOT, "tests", "cpp", "pooled_push_group_plan_test.cpp")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra,
                        "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "parameter_server_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


def test_pooled_push_group_plan(tmp_path):
    _build_and_run(tmp_path, "pooled_push_group_plan_test", [])


def test_pooled_push_group_plan_under_host_sanitizers(tmp_path):
    """The same host-only program with AddressSanitizer and UBSan: a stand-alone
    executable, nothing loaded into Python."""
    _build_and_run(tmp_path, "pooled_push_group_plan_test_san",
                   ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_the_symbol_is_exported_and_declared():
    from parameter_server_amd import _lib

    assert "pskv_apply_pooled_grouped" in _lib.EXPORTED
    assert callable(_lib.lib.pskv_apply_pooled_grouped)
    with open(os.path.join(ROOT, "include", "pskv.h")) as f:
        txt = f.read()
    assert re.search(r"^int pskv_apply_pooled_grouped\(pskv_shard\* s, const pskv_pool_batch\* batches, uint64_t nb, "
                     r"int flags\);", txt, re.M)
    assert "Grouped pooled pushes" in txt and "typedef struct pskv_pool_batch" in txt
    assert ctypes.sizeof(_lib.PskvPoolBatch) == 48
    assert _lib.PSKV_K_COUNT == 14 and _lib.PSKV_TIME_APPLY == 1 << 14  # no new kernel id, no new slot
    assert gu.MAX_POOL_BATCHES == 32


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _call(batches, flags, nb=None, null_array=False):
    """batches: list of (keys, n, weights, offsets, nbags, bag_grads) with n and nbags as given."""
    from parameter_server_amd import _lib

    arr = (_lib.PskvPoolBatch * max(len(batches), 1))()
    for i, (keys, n, wts, off, nbags, bg) in enumerate(batches):
        arr[i] = _lib.PskvPoolBatch(_ptr(keys), _ptr(wts), _ptr(off), _ptr(bg), n, nbags)
    rc = _lib.lib.pskv_apply_pooled_grouped(None, None if null_array else arr, len(batches) if nb is None else nb, flags)
    return rc, _lib.lib.pskv_last_error().decode()


def test_apply_pooled_grouped_checks_its_arguments_before_the_handle():
    from parameter_server_amd import _lib

    keys = np.arange(7, dtype=np.uint32)
    bg = np.full(3 * 4, 9.0, dtype=np.float32)
    good = np.array([0, 3, 3, 7], dtype=np.uint64)
    ok = (keys, 7, None, good, 3, bg)
    H, D = _lib.PSKV_HOST, _lib.PSKV_DEVICE
    # every argument holds: only the null shard is left to object to
    for batches in ([ok], [ok, ok, ok], []):
        rc, msg = _call(batches, H)
        assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    rc, msg = _call([ok], H, nb=0, null_array=True)  # nb == 0: a null array is fine
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    rc, msg = _call([ok], H, nb=2, null_array=True)
    assert rc == _lib.PSKV_EINVAL and "null batches" in msg and "null shard" not in msg, msg
    # a host call's offsets, in the third of four batches: the batch and the first bad bag are named
    for off, bag, word in [(np.array([1, 3, 3, 7], dtype=np.uint64), 0, "offsets[0]"),
                           (np.array([0, 5, 4, 7], dtype=np.uint64), 1, "decrease"),
                           (np.array([0, 3, 3, 6], dtype=np.uint64), 2, "offsets[nbags]"),
                           (np.array([0, 3, 8, 8], dtype=np.uint64), 1, "past")]:
        rc, msg = _call([ok, ok, (keys, 7, None, off, 3, bg), ok], H)
        assert rc == _lib.PSKV_EINVAL, (off, rc, msg)
        assert "batch 2:" in msg and "offsets" in msg and f"bag {bag}:" in msg and word in msg, msg
        assert "null shard" not in msg, msg
    # device offsets cannot be read: the same bad array gets as far as the handle
    rc, msg = _call([ok, (keys, 7, None, np.array([1, 3, 3, 7], dtype=np.uint64), 3, bg)], D)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for flags in (0x8, 0x100, D | _lib.PSKV_HOST_FRAME):
        rc, msg = _call([ok], flags)
        assert rc == _lib.PSKV_EINVAL and "flags" in msg, msg
    for bad, word in [((None, 7, None, good, 3, bg), "null keys"), ((keys, 7, None, None, 3, bg), "null offsets"),
                      ((keys, 7, None, good, 3, None), "null bag_grads")]:
        for place in (0, 1):
            batches = [ok, ok]
            batches[place] = bad
            rc, msg = _call(batches, H)
            assert rc == _lib.PSKV_EINVAL and word in msg and f"batch {place}:" in msg, msg
    # more than 2^31 keys in one batch: refused on the count alone (device flags: no offset is read)
    rc, msg = _call([ok, (keys, 2**31 + 1, None, good, 3, bg)], D)
    assert rc == _lib.PSKV_EINVAL and "2^31" in msg and "batch 1:" in msg and "null shard" not in msg, msg
    rc, msg = _call([ok, (keys, 2**31, None, good, 3, bg)], D)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    # a batch without a key or a bag: its null pointers are fine, the null shard is named
    rc, msg = _call([(None, 0, None, None, 0, None), ok], H)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    assert (bg == 9.0).all()


# ------------------------------------------------------- the checker's teeth
SIZES = (2049, 1, 4100)           # the issue's: 3 batches, two and three virtual workgroups, and one key
WIDTHS = (3, 16)
BAGS = ("eights", "ones", "mixed")  # consecutive batches have different bags


def _teeth_call(rng, w, kb, ke, dt):
    """Three batches with duplicates inside and across them: the middle one is
    weighted, the first is not (a mixed call)."""
    batches = []
    for j, n in enumerate(SIZES):
        keys, off, bg, wts = ppu.draw_call(rng, n, w, "dups_in_chunk", BAGS[j], kb, ke, dt, j != 0)
        batches.append((keys, off, bg, wts))
    sets = [set(b[0].tolist()) for b in batches]
    assert sets[0] & sets[2] and sets[1] & sets[2], "the call must repeat keys across batches"
    return batches


def _emulate(p, slots, kb, batches, dt, hp, t, rng):
    """The kernels' order on the concatenation: the once-rounded products, the
    losers summed in a random order, the winner the key's last position."""
    rows = np.vstack(gu.expanded_rows(batches, dt))
    return ppu.emulate_any(p, slots, gu.indices(batches, kb), rows, dt, hp, t, rng)


def _one_step_per_batch(p, slots, kb, batches, dt, hp, rng):
    """Wrong: every batch its own step (what nb pskv_apply_pooled calls make)."""
    for t, b in enumerate(batches, 1):
        p, slots = _emulate(p, slots, kb, [b], dt, hp, t, rng)
    return p, slots


def _previous_batchs_offsets(p, slots, kb, batches, dt, hp, rng):
    """Wrong: the positions of batch j looked up in batch j - 1's offsets (the
    bag index the kernels' bounded search would return there: below nbags)."""
    rows = []
    for j, (keys, off, bg, wts) in enumerate(batches):
        look = np.asarray(batches[j - 1][1] if j else off).astype(np.int64)
        bag = np.searchsorted(look[:-1], np.arange(keys.size), side="right") - 1
        bag = np.clip(bag, 0, bg.shape[0] - 1)
        rows.append(ppu.expand(wts, bg, bag, dt))
    return ppu.emulate_any(p, slots, gu.indices(batches, kb), np.vstack(rows), dt, hp, 1, rng)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,nesterov", ppu.KINDS)
def test_the_checker_accepts_the_kernel_order_and_rejects_the_grouped_hazards(kind, nesterov, dt):
    """An emulation of the kernels' order on the concatenated call lies inside
    the tolerances; one step per batch and a batch looked up in the previous
    batch's offsets lie outside.  (SGD without weight decay is linear in the
    gradient: one step per batch IS the one step there, p - lr (g1 + g2), so
    that hazard cannot show and is asserted at wd = 0.01 only.)"""
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[0]
    for wd in (0.0, 0.01):
        hp = ppu.hyper(kind, nesterov, wd)
        for w in WIDTHS:
            rng = np.random.default_rng(ou.case_seed("push-group", w, kind, nesterov, wd, dt.name))
            p = rng.standard_normal((ke - kb, w)).astype(dt)
            slots = ppu.initial_slots(kind, p.shape, dt)
            batches = _teeth_call(rng, w, kb, ke, dt)
            pre = gu.prepare(p, slots, kb, batches, dt, hp)
            tag = f"{kind} nesterov={nesterov} wd={wd} w={w}"
            pn, sn = _emulate(p, slots, kb, batches, dt, hp, 1, rng)
            assert not gu.step_errors(p, slots, kb, batches, pn, sn, dt, hp, pre=pre), tag
            wp, ws = _previous_batchs_offsets(p, slots, kb, batches, dt, hp, rng)
            assert gu.step_errors(p, slots, kb, batches, wp, ws, dt, hp, pre=pre), f"previous offsets accepted: {tag}"
            if kind == "sgd" and wd == 0.0:
                continue
            wp, ws = _one_step_per_batch(p, slots, kb, batches, dt, hp, rng)
            assert gu.step_errors(p, slots, kb, batches, wp, ws, dt, hp, pre=pre), f"a step per batch accepted: {tag}"


def test_the_tolerances_count_m_over_the_whole_call():
    """A key of an unweighted batch that also occurs in a weighted batch gets
    m + 1; a key of unweighted batches only keeps m; m spans the batches."""
    dt = np.dtype(np.float32)
    kb, ke, w = 0, 100, 2
    bg = np.ones((1, w), dtype=dt)
    off = lambda n: np.array([0, n], dtype=np.uint64)  # noqa: E731
    batches = [(np.array([5, 6, 6], np.uint32), off(3), bg, None),
               (np.array([6, 7], np.uint32), off(2), bg, np.ones(2, dtype=dt)),
               gu.empty_batch(w, dt, nbags=2), gu.empty_batch(w, dt, keys=3)]
    p = np.zeros((ke - kb, w), dtype=dt)
    ref, _, _ = gu.prepare(p, [], kb, batches, dt, ppu.hyper("sgd"))
    assert ref["m"][5] == 1 and ref["m"][6] == 3 + 1 and ref["m"][7] == 1 + 1 and ref["m"][8] == 0
    keys, coff, cbg, cw = gu.concatenated(batches, dt)
    assert keys.tolist() == [5, 6, 6, 6, 7] and coff.tolist() == [0, 3, 5] and cbg.shape == (2, w)
    assert cw.tolist() == [1, 1, 1, 1, 1]
