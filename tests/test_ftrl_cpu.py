"""CPU tests of FTRL-Proximal steps: the new exports and the configuration
struct, the argument checks that need no device, the np.longdouble oracle of
tests/ftrl_util.py pinned by a known answer and by opt_util's Adagrad
reference, and the conditions that bind the tolerances on the GPU bound tests'
own inputs.  No kernel is launched here."""
import ctypes
import math
import os

import numpy as np
import pytest

import ftrl_util as fu
import opt_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pskv_shard_set_optimizer_cfg", "pskv_shard_get_optimizer_cfg"]
F = fu.F


def _last_error():
    from parameter_server_amd import _lib

    return _lib.lib.pskv_last_error().decode()


def _cfg(**kw):
    from parameter_server_amd import _lib

    c = dict(size=ctypes.sizeof(_lib.PskvOptimizerCfg), kind=5, lr=0.05, weight_decay=0.01, eps=1e-8, init_accum=0.1,
             momentum=0.9, nesterov=0, beta1=0.9, beta2=0.999, l1=0.5, l2=0.01, ftrl_beta=1.0)
    c.update(kw)
    return _lib.PskvOptimizerCfg(c["size"], c["kind"], c["lr"], c["weight_decay"], c["eps"], c["init_accum"],
                                 c["momentum"], c["nesterov"], c["beta1"], c["beta2"], c["l1"], c["l2"],
                                 c["ftrl_beta"])


# ------------------------------------------------------- exports, constants
def test_new_symbols_are_exported_and_declared():
    from parameter_server_amd import _lib

    assert set(NEW) <= set(_lib.EXPORTED)
    header = open(os.path.join(ROOT, "include", "pskv.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(_lib.lib, name)
    assert _lib.PSKV_OPT_FTRL == 5 and "PSKV_OPT_FTRL = 5" in header
    assert "} pskv_optimizer_cfg;" in header and "FTRL-Proximal" in header
    for word in ("lr_power", "L2 shrinkage", "per-key step", "FTRL OWNS p"):  # what is not provided is said
        assert word in header, word
    assert _lib.PSKV_K_COUNT == 14 and _lib.lib.pskv_abi_version() == 1


def test_the_struct_begins_as_pskv_optimizer_ex():
    from parameter_server_amd import _lib

    ex, cfg = _lib.PskvOptimizerEx, _lib.PskvOptimizerCfg
    assert ctypes.sizeof(ex) == 72 and ctypes.sizeof(cfg) == 96
    for name, _ in ex._fields_:
        assert getattr(cfg, name).offset == getattr(ex, name).offset, name
    assert (cfg.l1.offset, cfg.l2.offset, cfg.ftrl_beta.offset) == (72, 80, 88)


def test_null_shard_and_null_configuration():
    from parameter_server_amd import _lib

    L = _lib.lib
    cfg, out, nb = _cfg(), _lib.PskvOptimizerCfg(), ctypes.c_uint64()
    assert L.pskv_shard_set_optimizer_cfg(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
    assert _last_error().startswith("pskv_shard_set_optimizer_cfg:") and "null shard" in _last_error()
    assert L.pskv_shard_get_optimizer_cfg(None, ctypes.byref(out), ctypes.byref(nb)) == _lib.PSKV_EINVAL
    assert _last_error().startswith("pskv_shard_get_optimizer_cfg:") and "null shard" in _last_error()
    assert L.pskv_shard_set_optimizer_cfg(None, None) == _lib.PSKV_EINVAL
    assert "null configuration" in _last_error()


@pytest.mark.parametrize("field,value,kind", [
    ("size", 0, 5), ("size", 72, 5), ("size", 72, 4), ("size", 104, 0),
    ("kind", 6, None), ("kind", -1, None),
    ("lr", 0.0, 5), ("lr", math.nan, 5), ("lr", math.inf, 5), ("lr", -1.0, 5),
    ("weight_decay", -1.0, 5), ("weight_decay", math.inf, 5),
    ("init_accum", -1.0, 5), ("init_accum", math.nan, 5), ("init_accum", math.inf, 5),
    ("l1", -0.5, 5), ("l1", math.nan, 5), ("l1", math.inf, 5),
    ("l2", -0.5, 5), ("l2", math.nan, 5), ("l2", math.inf, 5),
    ("ftrl_beta", -1.0, 5), ("ftrl_beta", math.nan, 5), ("ftrl_beta", math.inf, 5),
    # the older kinds' fields through the new setter, as through _ex
    ("eps", 0.0, 4), ("eps", -1.0, 2), ("init_accum", -1.0, 2), ("momentum", 1.0, 3), ("nesterov", 2, 3),
    ("beta1", 1.0, 4), ("beta2", math.nan, 4),
])
def test_set_optimizer_cfg_reports_the_bad_field_without_a_shard(field, value, kind):
    from parameter_server_amd import _lib

    kw = {field: value}
    if kind is not None:
        kw["kind"] = kind
    cfg = _cfg(**kw)
    assert _lib.lib.pskv_shard_set_optimizer_cfg(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
    msg = _last_error()
    assert field in msg and "null shard" not in msg, msg


def test_fields_ftrl_does_not_use_are_ignored_and_every_kind_reaches_the_handle():
    from parameter_server_amd import _lib

    for kw in (dict(kind=5, eps=0.0, momentum=7.0, nesterov=9, beta1=2.0, beta2=math.nan),
               dict(kind=5, l1=0.0, l2=0.0, ftrl_beta=0.0, init_accum=0.0, weight_decay=0.0),
               dict(kind=4, l1=-1.0, l2=math.nan, ftrl_beta=-1.0, init_accum=-1.0),  # Adam: no FTRL fields
               dict(kind=3, l1=math.inf, eps=0.0), dict(kind=2, l2=-1.0), dict(kind=1, ftrl_beta=math.nan, eps=0.0),
               dict(kind=0, lr=0.0, l1=-1.0)):
        cfg = _cfg(**kw)
        assert _lib.lib.pskv_shard_set_optimizer_cfg(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
        msg = _last_error()
        assert "null shard" in msg and " must" not in msg, msg


def test_the_older_setters_still_refuse_ftrl():
    from parameter_server_amd import _lib

    x = _lib.PskvOptimizerEx(ctypes.sizeof(_lib.PskvOptimizerEx), 5, 0.05, 0.0, 1e-8, 0.1, 0.0, 0, 0.9, 0.999)
    assert _lib.lib.pskv_shard_set_optimizer_ex(None, ctypes.byref(x)) == _lib.PSKV_EINVAL
    msg = _last_error()
    assert msg.startswith("pskv_shard_set_optimizer_ex:") and "kind" in msg and "null shard" not in msg, msg
    x.size, x.kind = 96, 4  # a pskv_optimizer_cfg's size is not an _ex's
    assert _lib.lib.pskv_shard_set_optimizer_ex(None, ctypes.byref(x)) == _lib.PSKV_EINVAL
    assert "size" in _last_error()
    old = _lib.PskvOptimizer(5, 0.05, 0.0, 1e-8, 0.1)
    assert _lib.lib.pskv_shard_set_optimizer(None, ctypes.byref(old)) == _lib.PSKV_EINVAL
    msg = _last_error()
    assert "kind" in msg and "null shard" not in msg, msg


def test_shard_class_knows_ftrl():
    import inspect

    import parameter_server_amd as ps

    assert ps.Shard._OPT_SLOTS["ftrl"] == 2 and ps.Shard._OPT_KIND["ftrl"] == 5 and ps.Shard._OPT_NAME[5] == "ftrl"
    sig = inspect.signature(ps.Shard.set_optimizer).parameters
    assert (sig["l1"].default, sig["l2"].default, sig["ftrl_beta"].default) == (0.0, 0.0, 1.0)


# ------------------------------------------------------------------ oracle
def test_known_answer():
    """lr 1, beta = l1 = l2 = 0, n from 0, gradients 3, 4, 12 on one key from p = 0."""
    hp = fu.hyper(lr=1.0, l1=0.0, l2=0.0, beta=0.0, init_accum=0.0)
    p, z, n = np.zeros((2, 1)), np.zeros((2, 1)), np.zeros((2, 1))
    want = [(9, 3, -1), (25, 9, -1.8), (169, 35.4, -35.4 / 13)]
    for g, (wn, wz, wp) in zip((3.0, 4.0, 12.0), want):
        ref = fu.step_ref(p, [z, n], [0], [[g]], hp)
        p, (z, n) = ref["p"], ref["slots"]
        assert math.isclose(n[0, 0], wn, rel_tol=1e-15) and math.isclose(z[0, 0], wz, rel_tol=1e-15)
        assert math.isclose(p[0, 0], wp, rel_tol=1e-15)
        assert p[1, 0] == 0 and z[1, 0] == 0 and n[1, 0] == 0
    # the emulation of the kernel's order gives the same in both types
    for dt in (np.float32, np.float64):
        p, s = np.zeros((2, 1), dtype=dt), [np.zeros((2, 1), dtype=dt), np.zeros((2, 1), dtype=dt)]
        for g, (wn, wz, wp) in zip((3.0, 4.0, 12.0), want):
            p, s = fu.emulate(p, s, [0], np.array([[g]], dtype=dt), dt, hp)
            assert s[1][0, 0] == wn
            assert math.isclose(s[0][0, 0], wz, rel_tol=4e-7) and math.isclose(p[0, 0], wp, rel_tol=4e-7)


def test_the_threshold_gives_plus_zero_and_shrinks_towards_it():
    hp = fu.hyper(lr=0.5, l1=1.0, l2=0.25, beta=1.0, init_accum=0.0)
    p, z, n = np.zeros((3, 1)), np.zeros((3, 1)), np.zeros((3, 1))
    ref = fu.step_ref(p, [z, n], [0, 1, 2], [[1.0], [-1.0], [-3.0]], hp)
    assert ref["p"][0, 0] == 0 and not np.signbit(ref["p"][0, 0])  # |z'| = l1: zero
    assert ref["p"][1, 0] == 0 and not np.signbit(ref["p"][1, 0])
    # z' = -3, r = 3: p' = (-1 + 3) / ((1 + 3) * 2 + 0.25)
    assert math.isclose(ref["p"][2, 0], 2 / 8.25, rel_tol=1e-15)
    for dt in (np.float32, np.float64):
        pe, _ = fu.emulate(p.astype(dt), [z.astype(dt), n.astype(dt)], [0, 1, 2],
                           np.array([[1.0], [-1.0], [-3.0]], dtype=dt), dt, hp)
        assert fu.bits(pe)[0, 0] == 0 and fu.bits(pe)[1, 0] == 0


def test_ftrl_without_regularisation_is_adagrad():
    """l1 = l2 = beta = 0 from a zero start: p' = p - lr d / sqrt(n'), Adagrad
    with h = n and a negligible eps; several steps with duplicated keys, each
    reference carrying its own state."""
    rng = np.random.default_rng(31)
    rows, w = 24, 3
    hp = fu.hyper(lr=0.05, l1=0.0, l2=0.0, beta=0.0, init_accum=0.0)
    ha = ou.hyper("adagrad", lr=0.05, eps=1e-300)
    pf, sf = np.zeros((rows, w), dtype=F), [np.zeros((rows, w), dtype=F), np.zeros((rows, w), dtype=F)]
    pa, ha_slots = np.zeros((rows, w), dtype=F), [np.zeros((rows, w), dtype=F)]
    for _ in range(6):
        idx = rng.integers(0, rows - 3, size=40)
        assert np.unique(idx).size < idx.size
        grads = rng.standard_normal((40, w))
        rf = fu.step_ref(pf, sf, idx, grads, hp)
        ra = ou.step_ref(pa, ha_slots, idx, grads, ha)
        pf, sf, pa, ha_slots = rf["p"], rf["slots"], ra["p"], ra["slots"]
        assert np.allclose(np.asarray(pf, dtype=np.float64), np.asarray(pa, dtype=np.float64), rtol=1e-12, atol=1e-14)
        assert np.allclose(np.asarray(sf[1], dtype=np.float64), np.asarray(ha_slots[0], dtype=np.float64), rtol=1e-14,
                           atol=0)
        assert not pf[rows - 3:].any() and not sf[0][rows - 3:].any()


# -------------------------------------------------------------- tolerances
def _walk(ci, dt):
    """The bound case's three steps along the oracle: (p, slots, idx, grads, pre, hp) per step."""
    rows, kb, n, w, pat = fu.BOUND_CASES[ci]
    hp = fu.case_hyper(ci)
    p0, calls = fu.bound_steps(ci, dt)
    p, slots = p0.copy(), fu.initial_slots(p0.shape, dt, hp)
    for keys, grads in calls:
        idx = keys.astype(np.int64) - kb
        assert idx.min() >= 0 and idx.max() < rows
        pre = fu.prepare(p, slots, idx, grads, dt, hp)
        yield p, slots, idx, grads, pre, hp
        p, slots = pre[0]["p"].astype(dt), [s.astype(dt) for s in pre[0]["slots"]]


def test_the_bound_cases_are_the_issues_shapes():
    assert {c[3] for c in fu.BOUND_CASES} == {1, 3, 4, 16, 20}
    # (the one distinct case fills its range: exactly two 2048-key chunks)
    assert all(64 <= c[0] <= 4096 and (c[2] > 2 * 2048 or c[4] == "distinct") for c in fu.BOUND_CASES)
    assert min(c[0] for c in fu.BOUND_CASES) == 64 and max(c[0] for c in fu.BOUND_CASES) == 4096


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_an_emulation_of_the_kernel_order_passes_the_checker(dt):
    """Condition (a): on every bound case and step, the kernel's operation order
    in float32 / float64 numpy arithmetic -- the losers' rows added one by one
    in call order and in a random order, then the own row, then the rule -- is
    inside the tolerances, and so is the oracle's own result rounded to the
    type; the band stays far inside its limit (both kinds of zero occur)."""
    dt = np.dtype(dt)
    zeros = nonzeros = 0
    for ci in range(len(fu.BOUND_CASES)):
        rng = np.random.default_rng(ou.case_seed("ftrl-perm", ci))
        for t, (p, slots, idx, grads, pre, hp) in enumerate(_walk(ci, dt), 1):
            ref = pre[0]
            fu.check_step(p, slots, idx, grads, ref["p"].astype(dt), [s.astype(dt) for s in ref["slots"]], dt, hp,
                          pre=pre, msg=f"oracle, case {ci} step {t}")
            for order in (None, rng):
                got_p, got_s = fu.emulate(p, slots, idx, grads, dt, hp, order)
                fu.check_step(p, slots, idx, grads, got_p, got_s, dt, hp, pre=pre, msg=f"case {ci} step {t}")
                _, band, checked = fu.step_report(p, slots, got_p, got_s, dt, hp, pre)
                assert band <= 0.001 * checked, (ci, t, band, checked)  # a tenth of the limit
            hit = ref["m"] > 0
            zeros += int((ref["p"][hit] == 0).sum())
            nonzeros += int((ref["p"][hit] != 0).sum())
    assert zeros > 1000 and nonzeros > 1000


def _sequential(ref, p, slots, idx, grads, rows, hp, dt):
    """The WRONG semantics at the keys `rows`: one step per occurrence, in call order."""
    pn, sn = ref["p"].copy(), [s.copy() for s in ref["slots"]]
    for k in rows:
        pk, sk = p[k:k + 1].astype(F), [s[k:k + 1].astype(F) for s in slots]
        for i in np.flatnonzero(idx == k):
            r = fu.step_ref(pk, sk, [0], grads[i:i + 1], hp, dt)
            pk, sk = r["p"], r["slots"]
        pn[k] = pk[0]
        for s, x in zip(sn, sk):
            s[k] = x[0]
    return pn, sn


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_checker_rejects_wrong_semantics_on_the_gpu_tests_inputs(dt):
    """Condition (b): on every bound case and step with a duplicated key, a
    result of m sequential steps and a result with one loser's gradient dropped
    both fall outside the tolerance in at least one of p, z, n."""
    dt = np.dtype(dt)
    seen = 0
    carried_by = set()
    for ci in range(len(fu.BOUND_CASES)):
        for t, (p, slots, idx, grads, pre, hp) in enumerate(_walk(ci, dt), 1):
            ref = pre[0]
            dup = np.flatnonzero(ref["m"] > 1)
            if not dup.size:
                continue
            seen += 1
            sp, ss = _sequential(ref, p, slots, idx, grads, dup[:4], hp, dt)
            bad = fu.step_errors(p, slots, idx, grads, sp.astype(dt), [s.astype(dt) for s in ss], dt, hp, pre=pre)
            assert bad, f"sequential steps accepted: case {ci} step {t}"
            carried_by |= {name for name, _ in bad}
            first = int(np.flatnonzero(idx == dup[0])[0])  # a loser: not the key's last occurrence
            keep = np.ones(idx.size, dtype=bool)
            keep[first] = False
            dr = fu.step_ref(p, slots, idx[keep], grads[keep], hp, dt)
            bad = fu.step_errors(p, slots, idx, grads, dr["p"].astype(dt), [s.astype(dt) for s in dr["slots"]], dt,
                                 hp, pre=pre)
            assert bad, f"a dropped loser accepted: case {ci} step {t}"
            carried_by |= {name for name, _ in bad}
    assert seen >= 3 * (len(fu.BOUND_CASES) - 1)
    assert {"z", "n"} <= carried_by


def test_the_checker_objects_to_a_moved_untouched_key_and_to_minus_zero():
    dt = np.dtype(np.float32)
    p, slots, idx, grads, pre, hp = next(_walk(0, dt))
    ref = pre[0]
    good = [ref["p"].astype(dt)] + [s.astype(dt) for s in ref["slots"]]
    untouched = int(np.flatnonzero(ref["m"] == 0)[0]) if (ref["m"] == 0).any() else None
    assert not fu.step_errors(p, slots, idx, grads, good[0], good[1:], dt, hp, pre=pre)
    if untouched is not None:
        for which in range(3):
            moved = [a.copy() for a in good]
            moved[which][untouched, 0] += 1
            assert fu.step_errors(p, slots, idx, grads, moved[0], moved[1:], dt, hp, pre=pre)
    hit = np.flatnonzero(ref["m"] > 0)
    zero_at = [(k, j) for k in hit for j in range(p.shape[1]) if fu.bits(good[0])[k, j] == 0]
    assert zero_at
    wrong = good[0].copy()
    wrong[zero_at[0]] = dt.type(-0.0)
    bad = fu.step_errors(p, slots, idx, grads, wrong, good[1:], dt, hp, pre=pre)
    assert bad and "not +0" in bad[0][1]
    # a zero where the closed form is far from the threshold is refused too
    nz = [(k, j) for k in hit for j in range(p.shape[1]) if abs(float(good[0][k, j])) > 1e-3]
    wrong = good[0].copy()
    wrong[nz[0]] = 0
    assert fu.step_errors(p, slots, idx, grads, wrong, good[1:], dt, hp, pre=pre)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_thousands_of_occurrences_of_one_key_with_dyadic_gradients(dt):
    """The gradient sum is exact in any order, so the step is checked with the
    m = 1 bounds; with those a dropped gradient is rejected, which the bounds
    of m = 4000 would let pass in float32."""
    dt = np.dtype(dt)
    hp = fu.hyper()
    p0, keys, grads, hot = fu.dyadic_many(dt)
    kb = 5
    idx = keys.astype(np.int64) - kb
    slots = fu.initial_slots(p0.shape, dt, hp)
    assert (idx == hot).sum() > 4000
    g = np.asarray(grads, dtype=F)
    assert np.array_equal(g * 16, np.round(g * 16)) and np.abs(g).sum(axis=0).max() * 16 < 2**24
    pre = fu.prepare(p0, slots, idx, grads, dt, hp, exact_sum=True)
    rng = np.random.default_rng(5)
    for order in (None, rng):
        got_p, got_s = fu.emulate(p0, slots, idx, grads, dt, hp, order)
        fu.check_step(p0, slots, idx, grads, got_p, got_s, dt, hp, pre=pre, msg="dyadic, m = 1 bounds")
    drop = int(np.flatnonzero((idx == hot) & (np.abs(grads).min(axis=1) > 0))[0])
    keep = np.ones(idx.size, dtype=bool)
    keep[drop] = False
    dr = fu.step_ref(p0, slots, idx[keep], grads[keep], hp, dt)
    got = dr["p"].astype(dt), [s.astype(dt) for s in dr["slots"]]
    bad = fu.step_errors(p0, slots, idx, grads, got[0], got[1], dt, hp, pre=pre)
    assert {name for name, _ in bad} >= {"z", "n"}
