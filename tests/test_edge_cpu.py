"""The special-value checkers have teeth (no GPU): on the very inputs of
tests/test_edge_gpu.py the dt emulation passes every checker of
tests/edge_util.py, and each wrong result named below is rejected.  The
condition on the step inputs (no tainted element depends on the summation
order) is checked here too.
"""
import numpy as np
import pytest

import edge_util as eu
import ftrl_util as fu
import opt_util as ou
import pooled_push_util as ppu
from rows_util import RowOracle, bits

DTYPES = [np.float32, np.float64]
ids = lambda d: np.dtype(d).name  # noqa: E731


# ------------------------------------------------------------- RowOracle
def test_row_oracle_rejects_a_nan_and_one_ulp_outside_the_bound(oracle_mod):
    orc = RowOracle(oracle_mod, np.float32, "accumulate", 1, 0, 8)
    keys = np.array([3, 3, 3], dtype=np.uint32)
    orc.add(keys, np.array([1.0, 2.0, 0.5], dtype=np.float32))
    q = np.array([3], dtype=np.uint32)
    ref, bound = orc.expect(q)
    assert ref[0, 0] == 3.5 and bound[0, 0] > 0
    inside = np.float32(3.5)
    while abs(np.float64(np.nextafter(inside, np.float32(9))) - 3.5) <= bound[0, 0]:
        inside = np.nextafter(inside, np.float32(9))
    orc.check(q, np.array([inside], dtype=np.float32))  # the last value inside the bound
    with pytest.raises(AssertionError):
        orc.check(q, np.array([np.nextafter(inside, np.float32(9))], dtype=np.float32))
    with pytest.raises(AssertionError):
        orc.check(q, np.array([np.nan], dtype=np.float32))


# --------------------------------------------------------------- lattice
def _sequential(idx, vals, slots, order=None):
    out = np.zeros((slots, vals.shape[1]), dtype=vals.dtype)
    order = np.arange(idx.size) if order is None else order
    with np.errstate(all="ignore"):
        np.add.at(out, idx[order], vals[order])  # one addition after the other, in dt
    return out


@pytest.mark.parametrize("scale", eu.SCALES)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
def test_lattice_checker_has_teeth(dt, scale):
    rng = np.random.default_rng(ou.case_seed("lattice-cpu", np.dtype(dt).name, scale))
    rows, n, w = 3000, 45_000, 3
    lat = eu.Lattice(dt, scale, rows + 2, w)
    idx, vals = eu.general_call(rng, lat, n, rows, extra=2)
    want = lat.want()
    assert (idx == eu.HOT).sum() > 10_000
    for order in (None, rng.permutation(n), np.argsort(idx, kind="stable")):
        assert eu.lattice_problems(_sequential(idx, vals, rows + 2, order), want) is None
    if np.dtype(dt) == np.float32 and scale == "sub":  # the hot key's sum left the subnormal range
        assert (np.abs(want[eu.HOT]) >= np.finfo(dt).tiny).all()
    hot = np.flatnonzero((idx == eu.HOT) & (vals[:, 1] != 0) & (np.abs(lat.values(np.array(3))) >= np.abs(vals[:, 1])))
    # one addend of the key with more than 10 000 occurrences dropped, one flushed to zero
    keep = np.ones(n, dtype=bool)
    keep[hot[0]] = False
    assert eu.lattice_problems(_sequential(idx[keep], vals[keep], rows + 2), want) is not None
    flushed = vals.copy()
    flushed[hot[1], 1] = 0
    assert eu.lattice_problems(_sequential(idx, flushed, rows + 2), want) is not None
    good = _sequential(idx, vals, rows + 2)
    r, c = np.argwhere(np.isnan(want))[0]
    for mutate in ("finite", "next column", "next row"):
        got = good.copy()
        if mutate == "finite":
            got[r, c] = 1
        elif mutate == "next column":
            assert not np.isnan(want[r, (c + 1) % w])
            got[r, (c + 1) % w] = np.nan
        else:
            assert not np.isnan(want[r + 1, c])
            got[r + 1, c] = np.nan
        assert eu.lattice_problems(got, want) is not None, mutate
    r, c = np.argwhere(np.isposinf(want))[0]
    got = good.copy()
    got[r, c] = -np.inf
    assert eu.lattice_problems(got, want) is not None
    got = good.copy()
    got[eu.ONCE_NEG0] = -0.0  # -0.0 stored instead of added
    assert eu.lattice_problems(got, want) is not None


@pytest.mark.parametrize("aligned", [True, False])
def test_window_calls_are_dense_windows_with_every_class(aligned):
    rng = np.random.default_rng(ou.case_seed("windows-cpu", aligned))
    lat = eu.Lattice(np.float32, "sub", 40_000, 1)
    got = np.zeros((40_000, 1), dtype=np.float32)
    for k, v in eu.window_calls(rng, lat, 40_000, aligned):
        assert np.array_equal(k, np.arange(k[0], k[0] + k.size)) and (not aligned or k[0] % 4 == 0 or k.size == 1)
        with np.errstate(all="ignore"):
            np.add.at(got, k, v)
    want = lat.want()
    assert eu.lattice_problems(got, want) is None
    assert np.isnan(want).sum() >= 2 and np.isposinf(want).sum() >= 2 and np.isneginf(want).any()


# ----------------------------------------------------------------- steps
def _initial_slots(hp, shape, dt):
    if hp["kind"] == "ftrl":
        return fu.initial_slots(shape, dt, hp)
    return ppu.initial_slots(hp["kind"], shape, dt)


def _mutations(arrays, w):
    """(what, arrays with one element changed)."""
    out = []

    def changed(a, at, v):
        new = [x.copy() for x in arrays]
        new[a][at] = v
        return new

    for a, x in enumerate(arrays):
        nan = np.argwhere(np.isnan(x))
        if len(nan):
            r, c = nan[0]
            out.append((f"array {a}: a NaN made finite", changed(a, (r, c), 0.25)))
            if w > 1:
                free = [(r, c) for r, c in nan if not np.isnan(x[r, (c + 1) % w])]
                r, c = free[0]
                out.append((f"array {a}: a NaN copied into the next column", changed(a, (r, (c + 1) % w), np.nan)))
            free = [(r, c) for r, c in nan if r + 1 < x.shape[0] and not np.isnan(x[r + 1, c])]
            r, c = free[0]
            out.append((f"array {a}: a NaN copied into the next row", changed(a, (r + 1, c), np.nan)))
        inf = np.argwhere(np.isinf(x))
        if len(inf):
            r, c = inf[0]
            out.append((f"array {a}: an infinity of the other sign", changed(a, (r, c), -x[r, c])))
    return out


@pytest.mark.parametrize("w", [1, 3, 4, 33])  # every width of the GPU cases: the seed holds it
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", eu.KINDS)
def test_step_checker_has_teeth_and_inputs_are_order_free(kind, dt, w):
    kb, ke, n = 0, 5000, 2049
    hp = eu.kind_hyper(kind)
    p0, calls, taints = eu.edge_steps(ou.case_seed("edge", kind, np.dtype(dt).name, n, w), kb, ke, n, w, dt)
    assert {(name, where) for _, _, name, where in taints[0]} >= {("nan", "winner"), ("+inf", "loser"),
                                                                 ("sub", "once"), ("-0", "winner"), ("both", "pair")}
    p, slots = p0, _initial_slots(hp, p0.shape, dt)
    seen = set()
    for step, (keys, grads) in enumerate(calls):
        idx = keys.astype(np.int64) - kb
        t = step + 1
        assert eu.order_problems(p, slots, idx, grads, dt, hp, idx, t) == []
        pn, sn = eu.emulate_step(p, slots, idx, grads, dt, hp, t)
        assert eu.edge_step_errors(p, slots, idx, grads, pn, sn, dt, hp, t) == []
        for what, (pm, *sm) in _mutations([pn] + sn, w):
            assert eu.edge_step_errors(p, slots, idx, grads, pm, sm, dt, hp, t), f"{what} was accepted"
            seen.add(what.split(": ")[1])
        # an untouched key changed, and an ordinary element off by more than its tolerance
        untouched = np.setdiff1d(np.arange(ke - kb), idx)[0]
        pm = pn.copy()
        pm[untouched, 0] = np.nextafter(pm[untouched, 0], np.inf)
        assert eu.edge_step_errors(p, slots, idx, grads, pm, sn, dt, hp, t)
        p, slots = pn, sn
    assert seen == {"a NaN made finite", "a NaN copied into the next row", "an infinity of the other sign"} | (
        {"a NaN copied into the next column"} if w > 1 else set())


@pytest.mark.parametrize("w", [1, 3, 4, 33])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", ["sgd", "adam", "ftrl"])
def test_pooled_step_checker_has_teeth_and_inputs_are_order_free(kind, dt, weighted, w):
    kb, ke, n = 0, 5000, 2049
    hp = eu.kind_hyper(kind)
    rng = np.random.default_rng(5)
    p = rng.standard_normal((ke - kb, w)).astype(dt)
    slots = _initial_slots(hp, p.shape, dt)
    keys, off, bg, wts = eu.pooled_edge_call(ou.case_seed("edge-pooled", kind, np.dtype(dt).name, weighted), kb, ke, n,
                                             w, dt, weighted)
    idx = keys.astype(np.int64) - kb
    pooled = (wts, bg, ppu.bag_index(off))
    assert eu.order_problems(p, slots, idx, None, dt, hp, idx, 1, pooled) == []
    pn, sn = eu.emulate_step(p, slots, idx, None, dt, hp, 1, pooled)
    assert eu.edge_step_errors(p, slots, idx, None, pn, sn, dt, hp, 1, pooled) == []
    assert np.isnan(pn).any()
    once = np.flatnonzero(np.bincount(idx, minlength=ke - kb) == 1)
    assert once.size and not np.isfinite(pn[once]).all(), "the key present once is not tainted"
    if weighted:  # the NaN weight taints its key's whole row, 0 * inf and inf * 0 one element each
        assert np.isnan(pn).all(axis=1).any()
    muts = _mutations([pn] + sn, w)
    assert len(muts) >= 3
    for what, (pm, *sm) in muts:
        assert eu.edge_step_errors(p, slots, idx, None, pm, sm, dt, hp, 1, pooled), f"{what} was accepted"


# --------------------------------------------------------------- residue
@pytest.mark.parametrize("residue", eu.RESIDUES)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", ["adagrad", "ftrl", "adam"])
def test_a_stale_gradient_scratch_changes_the_follow_up_steps(kind, dt, residue):
    case = eu.residue_case(kind, dt, 3, residue)
    clean = eu.residue_follow(case, dt)
    stale = eu.residue_follow(case, dt, stale=case["stale"])
    same = all(np.array_equal(bits(a), bits(b)) for (cp, cs), (sp, ss) in zip(clean, stale)
               for a, b in zip([cp] + cs, [sp] + ss))
    if residue == "zero":  # the losers cancel: +0 is what the scratch must hold anyway
        assert not case["stale"].any() and not np.signbit(case["stale"]).any() and same
    else:
        assert not same, "the twin comparison would not see this residue"
    idx = case["first"][0]
    assert (np.bincount(idx)[:eu.PROBES] == 3).all()
    for fi, _ in case["follow"]:
        assert np.unique(fi).size == fi.size and np.isin(np.arange(eu.PROBES), fi).all()


# ------------------------------------------------ subnormal-scale dyadic
DYADIC = [(2049, "distinct"), (2049, "all_equal"), (2049, "dups_in_chunk"), (2049, "dups_across_chunks"),
          (2049, "range_ends"), (4100, "all_equal"), (4100, "dups_across_chunks")]


@pytest.mark.parametrize("n,pat", DYADIC)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov"])
def test_scaled_dyadic_cases_are_exact_and_see_a_flushed_gradient(kind, dt, n, pat):
    dt = np.dtype(dt)
    w, kb = 3, 0
    hp, p0, calls, expect = eu.dyadic_case(kind, n, w, pat, dt)
    fi = np.finfo(dt)
    unit = -(eu.SUB_EXP[dt] + 2)  # 1 / (4 * smallest_subnormal)
    p, slots = p0, ou.zero_slots(hp["kind"], p0.shape, dt)
    for step, (keys, grads) in enumerate(calls):
        assert (np.abs(grads[grads != 0]) < fi.tiny).all()  # every gradient is a subnormal
        p, slots = eu.emulate_step(p, slots, keys.astype(np.int64) - kb, grads, dt, hp, step + 1)
        for got, want in zip([p] + slots, [expect[step][0]] + expect[step][1]):
            assert np.array_equal(bits(got), bits(want)), step
            m = np.ldexp(want.astype(eu.F), unit)
            assert np.array_equal(m, np.rint(m))  # a multiple of the granule
    m = np.ldexp(expect[-1][0].astype(eu.F), unit)
    if pat != "all_equal":  # (one stepped row need not land on an odd multiple)
        assert (np.fmod(m, 2) != 0).any(), "the granule 4 * smallest_subnormal is not reached"
    # one subnormal gradient flushed to zero in the first step
    keys, grads = calls[0]
    flushed = grads.copy()
    i = tuple(np.argwhere(grads != 0)[0])
    flushed[i] = 0
    pm, sm = eu.emulate_step(p0, ou.zero_slots(hp["kind"], p0.shape, dt), keys.astype(np.int64) - kb, flushed, dt, hp, 1)
    assert not np.array_equal(bits(pm), bits(expect[0][0]))
