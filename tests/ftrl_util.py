"""The oracle, the checker and a kernel-order emulation of FTRL-Proximal steps
(PSKV_OPT_FTRL), shared by tests/test_ftrl_{cpu,gpu,fuzz}.py.

One call is one step (include/pskv.h "Optimizer steps", "FTRL-Proximal"):
  1. g[k] = sum of the gradient rows of all occurrences of key k in the call
  2. d  = g + wd * p
     n' = n + d d;  r = sqrt(n');  s = (r - sqrt(n)) / lr
     z' = (z + d) - s p
     p' = +0 if |z'| <= l1, else (copysign(l1, z') - z') / ((beta + r) / lr + l2)
  3. keys not in the call keep p, z and n bit for bit
Slot 0 is z, slot 1 is n.

`step_ref` restates that in np.longdouble from a given (p, z, n); the threshold
compares with l1 ROUNDED TO THE SHARD'S TYPE (every hyper-parameter is rounded
to T once per launch: that is the rule, not an error of it).  `step_errors`
makes the ONE-STEP check of tests/opt_util.py on p, z and n.  The tolerances
count the roundings of the order the kernel is built in, to first order in u,
times 1.01, with one rounding of slack per count (DESIGN.md §8i has the
derivation).  u = 2^-24 / 2^-53, m the occurrences of the key, G = sum |g_i|,
D = G + wd |p|, q = sqrt(n), il = 1 / lr, x' the reference's value, c = 1.01:
  dd     = c (m + 3) u D                               the bound on d's error (§8c)
  tol_n  = 2 |d| dd + dd^2 + c u (2 d^2 + 2 |n'|)
  er     = min(tol_n / r, sqrt(tol_n)) + 3 c u r       the error of r (sqrt: up to 1 ulp + slack)
  eq     = 3 c u q                                     the error of sqrt(n), n read exactly
  tol_s  = il (er + eq) + 4 c u |s|                    ABSOLUTE: s is a difference of roots
  tol_z  = dd + |p| tol_s + c u (2 |z + d| + 2 |s p| + 2 |z'|)
  num    = copysign(l1, z') - z';  den = (beta + r) il + l2
  enum   = tol_z + c u (2 l1 + 2 |num|)
  eden   = il er + c u (5 il (beta + r) + 2 l2 + 2 den);  den_lo = den - eden
  tol_p  = enum / den_lo + |num| (1 / den_lo - 1 / den) + 6 c u |num / den|
           (division: up to 2.5 ulp + slack, so the bound does not ask for a
           correctly rounded one)
The threshold, with zr the reference's z' and l1 as the shard holds it:
  |zr| + tol_z <= l1   p must be the bit pattern +0
  |zr| - tol_z >  l1   p must lie within tol_p of the closed form
  otherwise            the element is in the BAND: either outcome is accepted
and band elements may be at most BAND_LIMIT of the checked elements.
"""
import numpy as np

import opt_util as ou
from rows_util import LAYOUTS, U_ROUND, bits, key_patterns

F = ou.F
SLOT_NAMES = ["z", "n"]
BAND_LIMIT = 0.01
# the bound tests' hyper-parameters: gradients of order 1, l1 around 0.5
BOUND_LR, BOUND_L1, BOUND_L2, BOUND_BETA, BOUND_INIT_ACCUM = 0.05, 0.5, 0.01, 1.0, 0.1


def hyper(lr=BOUND_LR, l1=BOUND_L1, l2=BOUND_L2, beta=BOUND_BETA, wd=0.0, init_accum=BOUND_INIT_ACCUM):
    return {"kind": "ftrl", "lr": lr, "l1": l1, "l2": l2, "beta": beta, "wd": wd, "init_accum": init_accum}


def set_optimizer(sh, hp):
    sh.set_optimizer("ftrl", lr=hp["lr"], l1=hp["l1"], l2=hp["l2"], ftrl_beta=hp["beta"], weight_decay=hp["wd"],
                     init_accum=hp["init_accum"])


def initial_slots(shape, dt, hp):
    return [np.zeros(shape, dtype=dt), np.full(shape, hp["init_accum"], dtype=dt)]


def l1_held(hp, dt):
    """l1 as a shard of type dt holds it."""
    return F(np.dtype(dt).type(hp["l1"]))


def step_ref(p, slots, idx, grads, hp, dt=None):
    """One step in the reference's precision.  p: (R, W); slots: [z, n]; idx:
    row of every occurrence; grads: (n, W).  dt: the shard's type, whose
    rounding of l1 the threshold uses (None: l1 itself).  Returns p, slots
    (new arrays), m (R,), G, d (R, W), and the closed form `cf` of every
    element whatever the threshold says."""
    p = np.asarray(p, dtype=F)
    w = p.shape[1]
    idx = np.asarray(idx, dtype=np.int64)
    gl = np.asarray(grads, dtype=F).reshape(idx.size, w)
    g, G = np.zeros_like(p), np.zeros_like(p)
    m = np.zeros(p.shape[0], dtype=np.int64)
    np.add.at(g, idx, gl)
    np.add.at(G, idx, np.abs(gl))
    np.add.at(m, idx, 1)
    hit = m > 0
    il, wd, l2, beta = F(1) / F(hp["lr"]), F(hp["wd"]), F(hp["l2"]), F(hp["beta"])
    l1 = F(hp["l1"]) if dt is None else l1_held(hp, dt)
    z, n = (np.asarray(s, dtype=F) for s in slots)
    d = np.where(hit[:, None], g + wd * p, F(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = n + d * d
        r = np.sqrt(nn)
        s = (r - np.sqrt(n)) * il
        zn = (z + d) - s * p
        cf = (np.copysign(l1, zn) - zn) / ((beta + r) * il + l2)
    pn = np.where(np.abs(zn) <= l1, F(0), cf)
    h = hit[:, None]
    return {"p": np.where(h, pn, p), "slots": [np.where(h, zn, z), np.where(h, nn, n)], "m": m, "G": G, "d": d,
            "cf": cf, "s": s, "r": r}


def tolerances(ref, p, slots, dt, hp, exact_sum=False):
    """(tol_p, [tol_z, tol_n]) per element for `ref` = step_ref(p, slots, ...).
    exact_sum: the call's gradient sums are exact in any order (dyadic
    inputs), so d has the roundings of m = 1."""
    u, c = F(U_ROUND[np.dtype(dt)]), F(1.01)
    p = np.abs(np.asarray(p, dtype=F))
    z, n = (np.asarray(s, dtype=F) for s in slots)
    m = np.minimum(ref["m"], 1)[:, None].astype(F) if exact_sum else ref["m"][:, None].astype(F)
    il, l2, beta, l1 = F(1) / F(hp["lr"]), F(hp["l2"]), F(hp["beta"]), l1_held(hp, dt)
    d, r, s = np.abs(ref["d"]), ref["r"], np.abs(ref["s"])
    zn, nn = ref["slots"]
    D = ref["G"] + F(hp["wd"]) * p
    dd = c * (m + 3) * u * D
    with np.errstate(invalid="ignore", divide="ignore"):
        tol_n = 2 * d * dd + dd * dd + c * u * (2 * d * d + 2 * np.abs(nn))
        er = np.where(r > 0, np.minimum(tol_n / np.where(r > 0, r, F(1)), np.sqrt(tol_n)), np.sqrt(tol_n)) + 3 * c * u * r
        eq = 3 * c * u * np.sqrt(n)
        tol_s = il * (er + eq) + 4 * c * u * s
        tol_z = dd + p * tol_s + c * u * (2 * np.abs(z + ref["d"]) + 2 * s * p + 2 * np.abs(zn))
        num = np.abs(np.copysign(l1, zn) - zn)
        den = (beta + r) * il + l2
        enum = tol_z + c * u * (2 * l1 + 2 * num)
        eden = il * er + c * u * (5 * il * (beta + r) + 2 * l2 + 2 * den)
        den_lo = den - eden
        tol_p = enum / den_lo + num * (1 / den_lo - 1 / den) + 6 * c * u * (num / den)
        tol_p = np.where(den_lo > 0, tol_p, F(np.inf))
    return tol_p, [tol_z, tol_n]


def prepare(p, slots, idx, grads, dt, hp, exact_sum=False, m_extra=None):
    """The reference step and its tolerances.  m_extra: (R,) added to m for the
    tolerances (a pooled push's weighted keys carry one more rounding)."""
    ref = step_ref(p, slots, idx, grads, hp, dt)
    if m_extra is not None:
        ref = dict(ref, m=ref["m"] + ((ref["m"] > 0) & np.asarray(m_extra, dtype=bool)))
    return (ref,) + tolerances(ref, p, slots, dt, hp, exact_sum)


def step_report(p, slots, p_got, slots_got, dt, hp, pre):
    """The one-step check as data: (problems, band, checked).  problems: a list
    of (array name, message); band: elements of p in the threshold's band;
    checked: elements of touched keys."""
    dt = np.dtype(dt)
    ref, tol_p, tol_s = pre
    hit = ref["m"] > 0
    out = []
    # z and n: opt_util's comparison
    pairs = [(nm, np.asarray(slots[i]), np.asarray(slots_got[i]), ref["slots"][i], tol_s[i])
             for i, nm in enumerate(SLOT_NAMES)]
    pairs.insert(0, ("p", np.asarray(p), np.asarray(p_got), None, None))
    for name, before, got, want, tol in pairs:
        assert got.dtype == dt and before.dtype == dt, (name, got.dtype, before.dtype, dt)
        same = bits(before[~hit]) == bits(got[~hit])
        if not same.all():
            out.append((name, f"{name}: {int((~same).sum())} elements of untouched keys changed"))
        if want is None:
            continue
        err = np.abs(got[hit].astype(F) - want[hit])
        bad = ~(err <= tol[hit])  # (a NaN fails)
        if bad.any():
            rows = np.flatnonzero(hit)[np.argwhere(bad)[:, 0]]
            i = tuple(np.argwhere(bad)[0])
            out.append((name, f"{name}: {int(bad.sum())} elements beyond the tolerance, rows {rows[:3].tolist()}: "
                              f"err {float(err[i]):.3e} tol {float(tol[hit][i]):.3e} m {int(ref['m'][rows[0]])}"))
    # p: the threshold
    l1 = l1_held(hp, dt)
    got = np.asarray(p_got)[hit]
    zr, tz = np.abs(ref["slots"][0][hit]), tol_s[0][hit]
    must_zero = zr + tz <= l1
    must_form = zr - tz > l1
    band = ~(must_zero | must_form)
    is_zero = bits(got) == 0
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(F) - ref["cf"][hit])
        close = err <= tol_p[hit]
    bad = (must_zero & ~is_zero) | (must_form & ~close) | (band & ~(is_zero | close))
    if bad.any():
        rows = np.flatnonzero(hit)[np.argwhere(bad)[:, 0]]
        i = tuple(np.argwhere(bad)[0])
        what = "not +0" if must_zero[i] else "beyond the tolerance"
        out.append(("p", f"p: {int(bad.sum())} elements wrong, rows {rows[:3].tolist()}: {what}, got {got[i]!r} "
                         f"err {float(err[i]):.3e} tol {float(tol_p[hit][i]):.3e} |z'| {float(zr[i]):.6g} "
                         f"m {int(ref['m'][rows[0]])}"))
    return out, int(band.sum()), int(got.size)


def step_errors(p, slots, idx, grads, p_got, slots_got, dt, hp, pre=None, exact_sum=False):
    pre = pre or prepare(p, slots, idx, grads, dt, hp, exact_sum)
    return step_report(p, slots, p_got, slots_got, dt, hp, pre)[0]


def check_step(p, slots, idx, grads, p_got, slots_got, dt, hp, pre=None, exact_sum=False, msg=""):
    """The bound tests' assertion: no problem, and the band holds at most
    BAND_LIMIT of the checked elements."""
    pre = pre or prepare(p, slots, idx, grads, dt, hp, exact_sum)
    problems, band, checked = step_report(p, slots, p_got, slots_got, dt, hp, pre)
    assert not problems, f"{msg}: " + "; ".join(text for _, text in problems)
    assert band <= BAND_LIMIT * checked, f"{msg}: {band} of {checked} elements in the threshold's band"


# --------------------------------------------------------------- emulation
def emulate(p, slots, idx, grads, dt, hp, rng=None):
    """The kernel's operation order in numpy arithmetic of type dt (no FMA):
    gsum = the losers' gradient rows added one by one into zero (in call order,
    or in a random order with `rng`), the winner = the key's LAST occurrence,
    d = (g_own + gsum) + wd * p, then the rule with every hyper-parameter
    rounded to dt once and 1 / lr computed in float64 first."""
    dt = np.dtype(dt).type
    pn = np.asarray(p, dtype=dt).copy()
    zn, nn = (np.asarray(s, dtype=dt).copy() for s in slots)
    g = np.asarray(grads, dtype=dt).reshape(len(idx), pn.shape[1])
    idx = np.asarray(idx, dtype=np.int64)
    wd, l1, l2, beta = dt(hp["wd"]), dt(hp["l1"]), dt(hp["l2"]), dt(hp["beta"])
    il = dt(1.0 / np.float64(hp["lr"]))
    order = np.argsort(idx, kind="stable")
    starts = np.flatnonzero(np.r_[True, idx[order][1:] != idx[order][:-1]])
    for a, b in zip(starts, np.r_[starts[1:], idx.size]):
        occ = order[a:b]
        k = idx[occ[0]]
        losers = occ[:-1] if rng is None else rng.permutation(occ[:-1])
        gsum = np.zeros(pn.shape[1], dtype=dt)
        for i in losers:
            gsum = gsum + g[i]
        pk = pn[k]
        d = (g[occ[-1]] + gsum) + wd * pk
        n1 = nn[k] + d * d
        r = np.sqrt(n1)
        s = (r - np.sqrt(nn[k])) * il
        z1 = (zn[k] + d) - s * pk
        nn[k], zn[k] = n1, z1
        pn[k] = np.where(np.abs(z1) <= l1, dt(0), (np.copysign(l1, z1) - z1) / ((beta + r) * il + l2))
    assert pn.dtype == dt and zn.dtype == dt and nn.dtype == dt
    return pn, [zn, nn]


# ------------------------------------------------------------------ inputs
# The bound tests' cases: (rows of the shard, key_begin, n keys of a call,
# width, key pattern).  Shards of 64 to 4096 rows; widths 1, 3, 4, 16, 20 (the
# 16-byte-unit and element paths, more than one unit strip, width 1); batches
# of about 5000 keys, more than two 2048-key chunks, with duplicates.
BOUND_CASES = [(64, 0, 5000, 1, "dups_in_chunk"), (257, 2**31 - 100, 4100, 3, "dups_across_chunks"),
               (4096, 1000, 4097, 4, "dups_across_chunks"), (4096, 0, 5000, 16, "range_ends"),
               (1000, 2**32 - 1000, 5000, 20, "dups_in_chunk"), (4096, 7, 4096, 4, "distinct")]
WDS = [0.0, 0.01]


def case_hyper(ci):
    return hyper(wd=WDS[ci % 2])


def bound_steps(ci, dt, steps=3):
    """(p0, calls) of BOUND_CASES[ci]: normal initial parameters, normal
    gradients (order 1), fresh keys per step over the same range."""
    rows, kb, n, w, pat = BOUND_CASES[ci]
    rng = np.random.default_rng(ou.case_seed("ftrl", ci, np.dtype(dt).name))
    p0 = rng.standard_normal((rows, w)).astype(dt)
    calls = []
    for _ in range(steps):
        calls.append((key_patterns(rng, n, kb, kb + rows)[pat], rng.standard_normal((n, w)).astype(dt)))
    return p0, calls


def dyadic_many(dt, n=4100, w=3, rows=64, kb=5):
    """Thousands of occurrences of ONE key with dyadic gradients (multiples of
    2^-4 in [-8, 8]: every partial sum is exact in any order), beside a few
    other keys: (p0, keys, grads, the hot row)."""
    rng = np.random.default_rng(ou.case_seed("ftrl-many", np.dtype(dt).name))
    p0 = rng.standard_normal((rows, w)).astype(dt)
    keys = np.full(n, kb + 17, dtype=np.uint32)
    keys[::500] = kb + np.arange(len(keys[::500]))
    return p0, keys, ou.dyadic_grads(rng, n, w, dt), 17
