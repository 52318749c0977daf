"""GPU tests of grouped pooled pushes (pskv_apply_pooled_grouped,
Shard.apply_pooled_grouped): the pooled pushes of several workers as ONE
optimizer step.

Three bars (tests/pooled_push_group_util.py):
  * random inputs, every optimizer kind: the one-step check against a
    longdouble step of the concatenated call from the shard's own state,
    opt_util's tolerances with m over the whole call and m + 1 for a key with a
    weighted occurrence (derived; tests/test_pooled_push_grouped_cpu.py proves
    the checker's teeth for the hazards a grouped call adds);
  * distinct keys over the whole call: a twin that takes pskv_apply_pooled of
    the concatenation and a third shard that takes pskv_apply_grouped of the
    host-expanded rows must hold the same bits, p, every slot and the step;
  * dyadic inputs (exact in float32, tests/test_pooled_push_cpu.py): bit-equal
    to the reference and to both twins with duplicated keys too, inside and
    across batches and launch groups.
"""
import os
import subprocess

import numpy as np
import pytest

import opt_util as ou
import pooled_push_group_util as gu
import pooled_push_util as ppu
from rows_util import LAYOUTS, bits
from test_gpu_parity import tdev
from test_opt_gpu import all_keys, assert_bits, read_p
from test_pooled_push_gpu import assert_same_state, make, slots_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 3, 4, 16, 33, 64]
# groups of 1, 3 and 5 batches of n in {1, 7, 2049, 4100} (2049 and 4100 cross one and two
# virtual-workgroup boundaries of 2048); the single batch's size rotates with the case
GROUPS = {1: None, 3: [2049, 1, 4100], 5: [7, 4100, 1, 2049, 7]}
SINGLES = [1, 7, 2049, 4100]
DTYPES = [np.float32, np.float64]
L = gu.MAX_POOL_BATCHES


def dyadic_hp(kind, nesterov):
    return ou.hyper("sgd", lr=ou.DYADIC_LR) if kind == "sgd" else ou.dyadic_hyper(nesterov)


def exact_ref(p, slots, kb, batches, w, hp, t, dt):
    """The reference step of a dyadic call, with the proof that the call is
    exact in dt: every partial sum of a key's terms (multiples of 2^-4) stays
    below 2^24 * 2^-4, and the new p and slots are representable."""
    ref = ou.step_ref(p, slots, gu.indices(batches, kb), gu.ref_rows(batches, w), hp, t)
    assert ref["G"].max() * 16 < 2**24
    for want in [ref["p"]] + ref["slots"]:
        assert np.array_equal(want.astype(dt).astype(ou.F), want), "the dyadic inputs are not exact at this shape"
    return ref


def apply_twins(batches, pooled, grouped, dt, cuda, device):
    """pskv_apply_pooled of the concatenation on `pooled`, pskv_apply_grouped of
    the host-expanded rows on `grouped`."""
    keys, off, bg, wts = gu.concatenated(batches, dt)
    ppu.apply_pooled(pooled, keys, off, bg, wts, cuda if device else None)
    rows = gu.expanded_rows(batches, dt)
    ks = [b[0] for b in gu.live(batches)]
    if device:
        grouped.apply_grouped([(tdev(k, cuda), tdev(r, cuda)) for k, r in zip(ks, rows)])
    else:
        grouped.apply_grouped(list(zip(ks, rows)))


# ------------------------------------------------------ against the reference
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("nb", sorted(GROUPS))
@pytest.mark.parametrize("li", range(len(LAYOUTS)), ids=["low", "straddle"])
def test_grouped_steps_meet_the_one_step_bound(cuda, li, nb, w, dt):
    """Every kind, three consecutive grouped steps each; the key pattern and the
    bag pattern of every batch, weighted and unweighted batches mixed in one
    call, the host and device paths and the weight decay rotate over the
    cases.  Every call of more than one batch has a key in two batches."""
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[li]
    c = ((li * 3 + sorted(GROUPS).index(nb)) * len(WIDTHS) + WIDTHS.index(w)) * 2 + (dt.itemsize == 8)
    rng = np.random.default_rng(ou.case_seed("push-group-gpu", li, nb, w, dt.name))
    for ki, (kind, nesterov) in enumerate(ppu.KINDS):
        hp = ppu.hyper(kind, nesterov, wd=(0.0, 0.01)[(c + ki) % 2])
        with make(kb, ke, dt, w, hp) as sh:
            sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
            for t in range(1, 4):
                r = c * 15 + ki * 3 + t
                sizes = GROUPS[nb] or [SINGLES[r % len(SINGLES)]]
                batches = gu.draw_group(rng, sizes, w, kb, ke, dt, c=r)
                device = bool((r // 2) % 2)
                if nb > 1:
                    assert set(batches[0][0].tolist()) & set(batches[1][0].tolist())
                p, slots = read_p(sh), slots_of(sh, hp)
                gu.apply_grouped(sh, batches, cuda if device else None)
                assert sh.step == t
                gu.check_step(p, slots, kb, batches, read_p(sh), slots_of(sh, hp), dt, hp, t,
                              msg=f"{kind} nesterov={nesterov} wd={hp['wd']} sizes={sizes} rotation={r} "
                                  f"weighted={[b[3] is not None for b in batches]} device={device} step {t}")
            sh.sync()


# --------------------- distinct keys over the whole call: both twins' bits
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("w", [1, 4, 5])
@pytest.mark.parametrize("kind,nesterov", ppu.KINDS)
def test_distinct_keys_equal_both_twins_bit_for_bit(cuda, kind, nesterov, w, dt):
    dt = np.dtype(dt)
    kb, ke = 0, 8000
    hp = ppu.hyper(kind, nesterov, wd=0.01)
    rng = np.random.default_rng(ou.case_seed("push-group-twin", kind, nesterov, w, dt.name))
    p0 = rng.standard_normal((ke - kb, w)).astype(dt)
    with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b, make(kb, ke, dt, w, hp) as g:
        for sh in (a, b, g):
            sh.add(all_keys(kb, ke), p0)
        for t in range(1, 4):
            batches = gu.draw_distinct_group(rng, [2049, 1, 4100, 7], w, kb, ke, dt, c=t + w)
            assert any(x[3] is None for x in batches) and any(x[3] is not None for x in batches)
            device = bool(t % 2)
            gu.apply_grouped(a, batches, cuda if device else None)
            apply_twins(batches, b, g, dt, cuda, device)
            assert_same_state(a, b, hp, f"against pskv_apply_pooled of the concatenation, step {t} device={device}")
            assert_same_state(a, g, hp, f"against pskv_apply_grouped of the expanded rows, step {t} device={device}")
        for sh in (a, b, g):
            sh.sync()


# ---------------------------------------------- dyadic, duplicated keys
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("w", [1, 4, 5])
@pytest.mark.parametrize("kind,nesterov", [("sgd", False), ("momentum", False), ("momentum", True)])
def test_dyadic_duplicates_are_bit_exact(cuda, kind, nesterov, w, dt):
    """Duplicates inside and across batches; exact sums, so the reference's
    bits and both twins' (test_pooled_push_cpu.py proves the inputs exact: every
    product a multiple of 2^-4 in [-8, 8], here up to 6157 of them per key)."""
    dt = np.dtype(dt)
    kb, ke = LAYOUTS[0]
    hp = dyadic_hp(kind, nesterov)
    rng = np.random.default_rng(ou.case_seed("push-group-dyadic", kind, nesterov, w))
    p = ou.dyadic_params(rng, ke - kb, w, dt)
    slots = ou.zero_slots(kind, p.shape, dt)
    with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b, make(kb, ke, dt, w, hp) as g:
        for sh in (a, b, g):
            sh.add(all_keys(kb, ke), p)
        for t in range(1, 4):
            batches = gu.draw_group(rng, [2049, 1, 4100, 7], w, kb, ke, dt, c=t, dyadic=True)
            if t == 2:  # one key in every position of two batches
                batches[0] = (np.full_like(batches[0][0], kb + 17),) + batches[0][1:]
                batches[2] = (np.full_like(batches[2][0], kb + 17),) + batches[2][1:]
            device = bool(t % 2)
            gu.apply_grouped(a, batches, cuda if device else None)
            apply_twins(batches, b, g, dt, cuda, device)
            ref = exact_ref(p, slots, kb, batches, w, hp, t, dt)
            p, slots = ref["p"].astype(dt), [s.astype(dt) for s in ref["slots"]]
            assert_bits(read_p(a), p, f"p against the reference, step {t}")
            for i, s in enumerate(slots):
                assert_bits(slots_of(a, hp)[i], s, f"slot {i} against the reference, step {t}")
            assert_same_state(a, b, hp, f"against the pooled twin, step {t}")
            assert_same_state(a, g, hp, f"against the grouped twin, step {t}")
        for sh in (a, b, g):
            sh.sync()


# ------------------------------------- more batches than one launch group
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("nb", [L + 1, 2 * L + 3], ids=["limit+1", "2limit+3"])
@pytest.mark.parametrize("kind,nesterov", [("sgd", False), ("momentum", True)])
def test_more_batches_than_one_launch_group(cuda, kind, nesterov, nb, dt):
    """Batches of 1 to 40 keys over a small range, so keys repeat on both sides
    of every launch-group boundary; dyadic, bit-exact; ONE step; one timed
    operation per launch group."""
    dt = np.dtype(dt)
    kb, ke, w = 0, 600, 4
    hp = dyadic_hp(kind, nesterov)
    rng = np.random.default_rng(ou.case_seed("push-group-many", kind, nesterov, nb))
    p = ou.dyadic_params(rng, ke - kb, w, dt)
    slots = ou.zero_slots(kind, p.shape, dt)
    groups = -(-nb // L)
    with make(kb, ke, dt, w, hp) as sh:
        sh.add(all_keys(kb, ke), p)
        sh.sync()
        sh.set_timing(True)
        for t, device in ((1, True), (2, False)):
            sizes = [int(n) for n in rng.integers(1, 41, size=nb)]
            batches = gu.draw_group(rng, sizes, w, kb, ke, dt, c=t, dyadic=True)
            for edge in range(L, nb, L):  # the batches on both sides of a boundary share keys
                assert set(batches[edge - 1][0].tolist()) & set(batches[edge][0].tolist())
            sh.reset_timing()
            gu.apply_grouped(sh, batches, cuda if device else None)
            assert sh.step == t
            sh.sync()
            tm = sh.apply_time()
            assert tm["launches"] == groups and tm["elements"] == sum(sizes), (tm, groups, sum(sizes))
            ref = exact_ref(p, slots, kb, batches, w, hp, t, dt)
            p, slots = ref["p"].astype(dt), [s.astype(dt) for s in ref["slots"]]
            assert_bits(read_p(sh), p, f"p against the reference, step {t}")
            for i, s in enumerate(slots):
                assert_bits(slots_of(sh, hp)[i], s, f"slot {i} against the reference, step {t}")


# ------------------------------------------------------------- unit paths
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["sgd", "momentum"])
def test_one_unaligned_batch_gives_the_same_bits(cuda, kind, dt):
    """W = 4: one batch's bag rows one element off 16-byte alignment send the
    WHOLE call down the element path; dyadic inputs make both paths exact."""
    dt = np.dtype(dt)
    kb, ke, w = 0, 5000, 4
    hp = dyadic_hp(kind, False)
    rng = np.random.default_rng(33)
    p0 = ou.dyadic_params(rng, ke - kb, w, dt)
    batches = gu.draw_group(rng, [2049, 4100, 7], w, kb, ke, dt, c=1, dyadic=True)
    with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b:
        for sh, shifts in ((a, [0, 0, 0]), (b, [0, 1, 0])):
            sh.add(all_keys(kb, ke), p0)
            gu.apply_grouped(sh, batches, cuda, bg_offsets=shifts)
        assert_same_state(a, b, hp, "all aligned against one batch one element off")
        ref = ou.step_ref(p0, ou.zero_slots(kind, p0.shape, dt), gu.indices(batches, kb), gu.ref_rows(batches, w), hp)
        assert_bits(read_p(a), ref["p"].astype(dt), "against the reference")


# ----------------------------------------------------------- empty batches
def test_empty_batches_between_live_ones(cuda):
    dt = np.dtype(np.float32)
    kb, ke, w = 0, 5000, 3
    hp = ppu.hyper("adam", wd=0.01)
    rng = np.random.default_rng(44)
    with make(kb, ke, dt, w, hp) as sh:
        sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        for t, device in ((1, True), (2, False)):
            x, y = gu.draw_group(rng, [2049, 7], w, kb, ke, dt, c=t)
            batches = [gu.empty_batch(w, dt), x, gu.empty_batch(w, dt, nbags=2), gu.empty_batch(w, dt, keys=3), y,
                       gu.empty_batch(w, dt)]
            p, slots = read_p(sh), slots_of(sh, hp)
            gu.apply_grouped(sh, batches, cuda if device else None)
            assert sh.step == t
            gu.check_step(p, slots, kb, batches, read_p(sh), slots_of(sh, hp), dt, hp, t, msg=f"step {t}")
        sh.sync()


def test_calls_of_empty_batches_only_do_not_step(cuda):
    dt = np.dtype(np.float32)
    w = 3
    with make(0, 100, dt, w, ppu.hyper("adam")) as sh:
        p0 = read_p(sh)
        sh.sync()
        sh.set_timing(True)
        sh.reset_timing()
        empties = [gu.empty_batch(w, dt), gu.empty_batch(w, dt, nbags=2), gu.empty_batch(w, dt, keys=4)]
        sh.apply_pooled_grouped([])
        sh.apply_pooled_grouped(empties)
        gu.apply_grouped(sh, empties, cuda)
        assert sh.step == 0
        assert_bits(read_p(sh), p0, "empty calls")
        sh.sync()
        assert sh.apply_time()["launches"] == 0  # (timing is on: nothing was queued)


# ------------------------------------------------------- out-of-range keys
@pytest.mark.parametrize("w", [1, 16])
def test_out_of_range_keys(cuda, w):
    from parameter_server_amd import _lib

    kb, ke = 1000, 3000
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(62 + w)
    p0 = ou.dyadic_params(rng, ke - kb, w, dt)
    batches = gu.draw_group(rng, [300, 500, 40], w, kb, ke, dt, c=1, dyadic=True)
    batches[1][0][77], batches[1][0][300] = 3007, 12  # batch 1 of 0..2: outside on both sides
    hp = ou.hyper("adagrad", lr=2.0**-3, eps=1e-10)
    with make(kb, ke, dt, w) as sh:
        sh.set_optimizer("adagrad", lr=2.0**-3, init_accum=0.5)
        sh.add(all_keys(kb, ke), p0)
        h0 = slots_of(sh, hp)[0]
        with pytest.raises(_lib.PskvError) as e:
            sh.apply_pooled_grouped(batches)
        assert e.value.code == _lib.PSKV_EINVAL and "batch 1:" in str(e.value) and "3007" in str(e.value)
        assert_bits(read_p(sh), p0, "a refused host call changed p")
        assert_bits(slots_of(sh, hp)[0], h0, "a refused host call changed h")
        assert sh.step == 0
        sh.sync()
        # device: the in-range keys are applied, the others dropped and reported
        sh.set_optimizer("sgd", lr=2.0**-3)
        gu.apply_grouped(sh, batches, cuda)
        idx, rows = gu.indices(batches, kb), gu.ref_rows(batches, w)
        inside = (idx >= 0) & (idx < ke - kb)
        want = ou.step_ref(p0, [], idx[inside], rows[inside], ou.hyper("sgd", lr=2.0**-3))["p"]
        assert_bits(read_p(sh), want.astype(dt), "device call with out-of-range keys")
        assert sh.step == 1
        with pytest.raises(_lib.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE and "out-of-range" in str(e.value)
        sh.clear()
        sh.sync()


# ------------------------------------------------ malformed device offsets
@pytest.mark.parametrize("w", [1, 4, 33])
def test_malformed_device_offsets_touch_only_the_calls_keys(cuda, w):
    """The middle batch of three has malformed device offsets (the four shapes
    of the single-batch test): the call returns, sync succeeds and every key
    not in the call keeps its bits; what the call's keys hold is unspecified."""
    import torch

    dt = np.dtype(np.float32)
    kb, ke, n, nbags = 0, 5000, 4100, 300
    rng = np.random.default_rng(93 + w)
    with make(kb, ke, dt, w, ppu.hyper("adam", wd=0.01)) as sh:
        sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        bad = [np.arange(nbags + 1)[::-1] * 13,                        # decreasing
               np.arange(nbags + 1) * 1000 + n,                        # beyond n
               np.concatenate([[5], np.sort(rng.integers(5, n, size=nbags - 1)), [n]]),  # offsets[0] != 0
               rng.integers(0, 2**62, size=nbags + 1)]                 # anything
        for off in bad:
            x, y = gu.draw_group(rng, [2049, 7], w, kb, 2000, dt, c=2)  # keys 2000.. are not in the call
            keys = (kb + rng.integers(0, 2000, size=n)).astype(np.uint32)
            bg = (rng.standard_normal((nbags, w)) * 3).astype(dt)
            wts = rng.standard_normal(n).astype(dt)
            p, slots = read_p(sh), slots_of(sh, {"kind": "adam"})
            dev = [gu.device_batch(sh, x, cuda),
                   (tdev(keys, cuda), torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(cuda),
                    tdev(bg.reshape(-1), cuda), tdev(wts, cuda)),
                   gu.device_batch(sh, y, cuda)]
            sh.apply_pooled_grouped(dev)
            sh.sync()
            untouched = np.ones(ke - kb, dtype=bool)
            untouched[:2000] = False
            assert np.array_equal(bits(read_p(sh)[untouched]), bits(p[untouched]))
            for a, b in zip(slots_of(sh, {"kind": "adam"}), slots):
                assert np.array_equal(bits(a[untouched]), bits(b[untouched]))


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_step(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    keys = np.arange(7, dtype=np.uint32)
    off = ppu.pu.offsets_of([3, 0, 4])
    H = _lib.PSKV_HOST

    def raw(sh, n, bag_grads, flags=H):
        arr = (_lib.PskvPoolBatch * 2)()
        good = np.ones((3, 2), np.float32)
        arr[0] = _lib.PskvPoolBatch(keys.ctypes.data, None, off.ctypes.data, good.ctypes.data, 7, 3)
        arr[1] = _lib.PskvPoolBatch(keys.ctypes.data, None, off.ctypes.data,
                                    bag_grads.ctypes.data if bag_grads is not None else None, n, 3)
        return _lib.lib.pskv_apply_pooled_grouped(sh._h, arr, 2, flags), _lib.lib.pskv_last_error().decode()

    with ps.Shard(0, 100, np.float32, width=2) as sh:  # no optimizer
        with pytest.raises(_lib.PskvError) as e:
            sh.apply_pooled_grouped([(keys, off, np.ones((3, 2), np.float32))])
        assert e.value.code == _lib.PSKV_EINVAL and "no optimizer" in str(e.value)
        assert sh.step == 0
        sh.set_optimizer("sgd", lr=0.5)
        rc, msg = raw(sh, 7, None)
        assert rc == _lib.PSKV_EINVAL and "null bag_grads" in msg and "batch 1:" in msg
        # n > 2^31: refused on the count (device flags: no buffer is touched)
        rc, msg = raw(sh, 2**31 + 1, np.ones((3, 2), np.float32), _lib.PSKV_DEVICE)
        assert rc == _lib.PSKV_EINVAL and "2^31" in msg and "batch 1:" in msg
        with pytest.raises(ValueError):
            sh.apply_pooled_grouped([(keys, off, np.ones((3, 2), np.float32)),
                                     (tdev(keys, cuda), off, np.ones((3, 2), np.float32))])
        with pytest.raises(ValueError):
            sh.apply_pooled_grouped([(keys, off, np.ones((2, 2), np.float32))])
        assert sh.step == 0 and not read_p(sh).any()
    with ps.Shard(0, 100, np.int32, width=2) as sh:
        rc, msg = raw(sh, 7, np.ones((3, 2), np.int32))
        assert rc == _lib.PSKV_EINVAL and "float shards only" in msg
        assert sh.step == 0
        sh.sync()


# ------------------------------------------------------------- other paths
def test_gsum_is_zero_again_after_a_grouped_push(cuda):
    """After a grouped pooled push with duplicates inside and across batches an
    ordinary apply on the same shard meets its bound: the gradient scratch is
    back to zero."""
    from rows_util import key_patterns

    dt = np.dtype(np.float32)
    kb, ke, w = 0, 5000, 16
    hp = ppu.hyper("adagrad", wd=0.01)
    rng = np.random.default_rng(43)
    with make(kb, ke, dt, w, hp) as sh:
        sh.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        gu.apply_grouped(sh, gu.draw_group(rng, [4100, 2049, 7], w, kb, ke, dt, c=1), cuda)
        k2 = key_patterns(rng, 4100, kb, ke)["dups_across_chunks"]
        g2 = (rng.standard_normal((4100, w)) * 3).astype(dt)
        p, slots = read_p(sh), slots_of(sh, hp)
        sh.apply(tdev(k2, cuda), tdev(g2, cuda))
        ou.check_step(p, slots, k2.astype(np.int64) - kb, g2, read_p(sh), slots_of(sh, hp), dt, hp, 2, msg="apply")
        sh.sync()


def test_checkpoint_restores_bit_for_bit(cuda):
    dt = np.dtype(np.float32)
    kb, ke, w = 0, 8000, 4
    hp = ppu.hyper("adam", wd=0.01)
    rng = np.random.default_rng(73)
    with make(kb, ke, dt, w, hp) as a, make(kb, ke, dt, w, hp) as b:
        a.add(all_keys(kb, ke), rng.standard_normal((ke - kb, w)).astype(dt))
        for c in (1, 2):
            gu.apply_grouped(a, gu.draw_group(rng, [2049, 7, 300], w, kb, ke, dt, c=c), cuda)
        b.load_state_dict(a.state_dict())
        assert b.step == 2
        # (duplicated keys: the sums' order is unspecified, so the third call runs on distinct keys)
        batches = gu.draw_distinct_group(rng, [2049, 7, 300], w, kb, ke, dt, c=3)
        for sh in (a, b):
            gu.apply_grouped(sh, batches, cuda)
        assert_same_state(a, b, hp, "after the restore")


def test_width_one_with_the_request_server(cuda):
    """SERVE = 1: the grouped pooled push first ends the server; small host Gets see it."""
    kb, ke = 0, 4000
    dt = np.dtype(np.float32)
    rng = np.random.default_rng(12)
    hp = ou.hyper("sgd", lr=ou.DYADIC_LR)
    with make(kb, ke, dt, 1, hp, options={"SERVE": 1}) as sh:
        p = ou.dyadic_params(rng, ke - kb, 1, dt)
        sh.add(all_keys(kb, ke), p.reshape(-1))
        small = rng.integers(kb, ke, size=20).astype(np.uint32)
        assert np.array_equal(sh.get(small), p[small, 0])  # (a small host Get: the server's)
        for device in (True, False):
            batches = gu.draw_group(rng, [2049, 7, 1], 1, kb, ke, dt, c=1, dyadic=True)
            gu.apply_grouped(sh, batches, cuda if device else None)
            p = ou.step_ref(p, [], gu.indices(batches, kb), gu.ref_rows(batches, 1), hp)["p"].astype(dt)
            assert np.array_equal(bits(sh.get(small)), bits(p[small, 0]))
        sh.sync()


def test_cpp_pooled_push_group_program(cuda):
    """tests/cpp/hip_storage_pooled_push_group_test.cpp: SubApplyPooledGrouped
    through HipStorage<float> and <double> against an expanded AddGrouped."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_pooled_push_group_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
