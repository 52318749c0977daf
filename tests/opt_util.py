"""The oracle, the checker and a kernel-order emulation of optimizer steps
(pskv_apply), shared by tests/test_opt_{cpu,gpu}.py (SGD, Adagrad) and
tests/test_opt2_{cpu,gpu}.py (momentum, Adam).

One call is one step (include/pskv.h "Optimizer steps", "Momentum and Adam"):
  1. g[k] = sum of the gradient rows of all occurrences of key k in the call
  2. d = g + wd * p, then the kind's rule on its state slots:
       sgd       p <- p - lr d
       adagrad   h <- h + d d;  p <- p - lr d / (sqrt(h) + eps)
       momentum  v <- mu v + d;  p <- p - lr v   (nesterov: p <- p - lr (d + mu v), the new v)
       adam      m <- b1 m + (1 - b1) d;  v <- b2 v + (1 - b2) d d;
                 p <- p - a m / (sqrt(v) b + eps),  a = lr / (1 - b1^t),  b = 1 / sqrt(1 - b2^t)
  3. keys not in the call keep p and every slot bit for bit

`step_ref` restates that from a given (p, slots) and step number t, in numpy's
extended precision (np.longdouble, u = 2^-64 where the platform has it): a
float64 reference would carry roundings of its own as large as a float64
shard's, and the tolerances below leave no room for a second set.
`check_step` makes the ONE-STEP check: the test reads the shard's own p and
slots of the whole range before a step, runs one reference step from those, and
compares every element afterwards.  The tolerances count the roundings of the
order the kernel is built in; u = 2^-24 / 2^-53, m the
occurrences of the key, G = sum |g_i| per element, D = G + wd |p|,
dd = 1.01 (m + 3) u D (the bound on d's error), x' the reference's new value:
  sgd p       1.01 u (|p'| + (m + 5) lr D)
  adagrad h   1.01 u (h' + (2m + 8) D D)
  adagrad p   1.01 u |p'| + lr (dd / (sqrt(h + max(|d| - dd, 0)^2) + eps) + 8 * 1.01 u |r|),
              r = d / (sqrt(h') + eps)
  momentum v  dd + 1.01 u (3 mu |v| + |v'|)
  momentum p  1.01 u |p'| + lr (tol_v + 3 * 1.01 u |v'|)
  nesterov p  s = d + mu v':  1.01 u |p'| + lr (dd + mu tol_v + 1.01 u (3 mu |v'| + 4 |s|))
  adam m      (1 - b1) dd + 1.01 u (3 b1 |m| + 3 (1 - b1) |d| + |m'|)
  adam v      (1 - b2) (2 |d| dd + dd^2) + 1.01 u (3 b2 v + 4 (1 - b2) d^2 + v')
  adam p      the denominator den = sqrt(v') b + eps lies in
                [sqrt(max(v' - tol_v, 0)) b (1 - e) + eps,  sqrt(v' + tol_v) b (1 + e) + eps],
              e = 1.01 (4 u + eb);  with r = m' / den:
              1.01 u |p'| + a (tol_m / den_lo + |m'| max(1 / den_lo - 1 / den, 1 / den - 1 / den_hi)
                               + 1.01 (5 u + ea) |r|)
              ea, eb: what the host's double arithmetic can put on a and b
              (pow within one ulp, amplified by b^t / (1 - b^t); only a float64 shard sees it)
  untouched   bit-identical p and slots
"""
import zlib

import numpy as np

from rows_util import LAYOUTS, U_ROUND, bits, key_patterns

F = np.longdouble  # the reference's arithmetic
U64 = 2.0**-53
SLOT_NAMES = {"sgd": [], "adagrad": ["h"], "momentum": ["v"], "adam": ["m", "v"]}
SLOTS = {kind: len(names) for kind, names in SLOT_NAMES.items()}

# the bound tests' hyper-parameters (the GPU tests; the CPU tests prove the
# checker rejects wrong semantics on exactly these inputs)
BOUND_LR, BOUND_EPS, BOUND_INIT_ACCUM = 0.05, 1e-8, 0.1
BOUND_MU, BOUND_BETA1, BOUND_BETA2 = 0.9, 0.9, 0.999
# the dyadic cases (SGD, momentum): every sum, product and difference exact in float32
DYADIC_LR, DYADIC_MU = 2.0**-3, 0.5


def hyper(kind, lr=BOUND_LR, wd=0.0, eps=BOUND_EPS, mu=BOUND_MU, nesterov=False, beta1=BOUND_BETA1,
          beta2=BOUND_BETA2):
    return {"kind": kind, "lr": lr, "wd": wd, "eps": eps, "mu": mu, "nesterov": bool(nesterov), "beta1": beta1,
            "beta2": beta2}


def set_optimizer_kwargs(hp):
    """The keyword arguments of Shard.set_optimizer for `hp` (momentum, Adam)."""
    kw = {"lr": hp["lr"], "weight_decay": hp["wd"]}
    if hp["kind"] == "momentum":
        kw.update(momentum=hp["mu"], nesterov=hp["nesterov"])
    else:
        kw.update(eps=hp["eps"], beta1=hp["beta1"], beta2=hp["beta2"])
    return kw


def bias_corrections(hp, t, f=F):
    """(a, b) of step t in the arithmetic f (np.longdouble: the reference; np.float64: the host's)."""
    b1, b2, lr = f(hp["beta1"]), f(hp["beta2"]), f(hp["lr"])
    return lr / (f(1) - b1**f(t)), f(1) / np.sqrt(f(1) - b2**f(t))


def step_ref(p, slots, idx, grads, hp, t=1):
    """One step in the reference's precision.  p: (R, W); slots: list of (R, W)
    arrays (sgd [], adagrad [h], momentum [v], adam [m, v]); idx: row of every
    occurrence; grads: (n, W); t: the step number.  Returns p, slots (new
    arrays), m (R,) occurrences, G (R, W) sum |g_i|, d (R, W)."""
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
    kind, lr, wd, eps = hp["kind"], F(hp["lr"]), F(hp["wd"]), F(hp["eps"])
    d = np.where(hit[:, None], g + wd * p, F(0))
    pn = p.copy()
    sn = [np.asarray(s, dtype=F).copy() for s in slots]
    assert len(sn) == SLOTS[kind]
    if kind == "sgd":
        pn[hit] = p[hit] - lr * d[hit]
    elif kind == "adagrad":
        sn[0][hit] = sn[0][hit] + d[hit] * d[hit]
        pn[hit] = p[hit] - lr * d[hit] / (np.sqrt(sn[0][hit]) + eps)
    elif kind == "momentum":
        mu = F(hp["mu"])
        sn[0][hit] = mu * sn[0][hit] + d[hit]
        pn[hit] = p[hit] - lr * ((d[hit] + mu * sn[0][hit]) if hp["nesterov"] else sn[0][hit])
    else:
        b1, b2 = F(hp["beta1"]), F(hp["beta2"])
        a, b = bias_corrections(hp, t)
        sn[0][hit] = b1 * sn[0][hit] + (F(1) - b1) * d[hit]
        sn[1][hit] = b2 * sn[1][hit] + (F(1) - b2) * d[hit] * d[hit]
        pn[hit] = p[hit] - a * sn[0][hit] / (np.sqrt(sn[1][hit]) * b + eps)
    return {"p": pn, "slots": sn, "m": m, "G": G, "d": d}


def tolerances(ref, p, slots, dt, hp, t=1):
    """(tol_p, [tol per slot]) per element for `ref` = step_ref(p, slots, ...)."""
    kind = hp["kind"]
    p = np.asarray(p, dtype=F)
    m = ref["m"][:, None].astype(F)
    if kind in ("sgd", "adagrad"):
        u, lr, wd, eps = U_ROUND[np.dtype(dt)], hp["lr"], hp["wd"], hp["eps"]
        D = ref["G"] + wd * np.abs(p)
        if kind == "sgd":
            return 1.01 * u * (np.abs(ref["p"]) + (m + 5) * lr * D), []
        h, hn = np.asarray(slots[0], dtype=F), ref["slots"][0]
        dd = 1.01 * (m + 3) * u * D
        tol_h = 1.01 * u * (hn + (2 * m + 8) * D * D)
        r = ref["d"] / (np.sqrt(hn) + eps)
        lo = np.maximum(np.abs(ref["d"]) - dd, F(0))
        tol_p = 1.01 * u * np.abs(ref["p"]) + lr * (dd / (np.sqrt(h + lo * lo) + eps) + 8 * 1.01 * u * np.abs(r))
        return tol_p, [tol_h]
    u = F(U_ROUND[np.dtype(dt)])
    c = F(1.01)
    s0 = [np.asarray(s, dtype=F) for s in slots]
    lr = F(hp["lr"])
    D = ref["G"] + F(hp["wd"]) * np.abs(p)
    dd = c * (m + 3) * u * D
    d, pn, sn = np.abs(ref["d"]), np.abs(ref["p"]), ref["slots"]
    if kind == "momentum":
        mu = F(hp["mu"])
        tol_v = dd + c * u * (3 * mu * np.abs(s0[0]) + np.abs(sn[0]))
        if hp["nesterov"]:
            s = np.abs(ref["d"] + mu * sn[0])
            tol_p = c * u * pn + lr * (dd + mu * tol_v + c * u * (3 * mu * np.abs(sn[0]) + 4 * s))
        else:
            tol_p = c * u * pn + lr * (tol_v + 3 * c * u * np.abs(sn[0]))
        return tol_p, [tol_v]
    b1, b2, eps = F(hp["beta1"]), F(hp["beta2"]), F(hp["eps"])
    a, b = bias_corrections(hp, t)
    k1, k2 = b1**F(t) / (1 - b1**F(t)), b2**F(t) / (1 - b2**F(t))
    ea, eb = (2 * k1 + 3) * F(U64), (k2 + 3) * F(U64)
    tol_m = (1 - b1) * dd + c * u * (3 * b1 * np.abs(s0[0]) + 3 * (1 - b1) * d + np.abs(sn[0]))
    tol_v = (1 - b2) * (2 * d * dd + dd * dd) + c * u * (3 * b2 * s0[1] + 4 * (1 - b2) * d * d + sn[1])
    e = c * (4 * u + eb)
    den = np.sqrt(sn[1]) * b + eps
    den_lo = np.sqrt(np.maximum(sn[1] - tol_v, F(0))) * b * (1 - e) + eps
    den_hi = np.sqrt(sn[1] + tol_v) * b * (1 + e) + eps
    r = np.abs(sn[0]) / den
    tol_p = c * u * pn + a * (tol_m / den_lo + np.abs(sn[0]) * np.maximum(1 / den_lo - 1 / den, 1 / den - 1 / den_hi)
                              + c * (5 * u + ea) * r)
    return tol_p, [tol_m, tol_v]


def prepare(p, slots, idx, grads, dt, hp, t=1):
    """The reference step and its tolerances, for several step_errors calls on one step."""
    ref = step_ref(p, slots, idx, grads, hp, t)
    return (ref,) + tolerances(ref, p, slots, dt, hp, t)


def step_errors(p, slots, idx, grads, p_got, slots_got, dt, hp, t=1, pre=None):
    """The one-step check as data: a list of (array name, message) problems
    (empty = the step is right).  p, slots: the shard's rows before the step;
    p_got, slots_got: after; pre: prepare() of the same step, if at hand."""
    dt = np.dtype(dt)
    ref, tol_p, tol_s = pre or prepare(p, slots, idx, grads, dt, hp, t)
    hit = ref["m"] > 0
    out = []
    pairs = [("p", np.asarray(p), np.asarray(p_got), ref["p"], tol_p)]
    for i, nm in enumerate(SLOT_NAMES[hp["kind"]]):
        pairs.append((nm, np.asarray(slots[i]), np.asarray(slots_got[i]), ref["slots"][i], tol_s[i]))
    for name, before, got, want, tol in pairs:
        assert got.dtype == dt and before.dtype == dt, (name, got.dtype, before.dtype, dt)
        same = bits(before[~hit]) == bits(got[~hit])
        if not same.all():
            out.append((name, f"{name}: {int((~same).sum())} elements of untouched keys changed"))
        err = np.abs(got[hit].astype(F) - want[hit])
        bad = ~(err <= tol[hit])  # (a NaN fails)
        if bad.any():
            rows = np.flatnonzero(hit)[np.argwhere(bad)[:, 0]]
            i = tuple(np.argwhere(bad)[0])
            out.append((name, f"{name}: {int(bad.sum())} elements beyond the tolerance, rows {rows[:3].tolist()}: "
                              f"err {float(err[i]):.3e} tol {float(tol[hit][i]):.3e} m {int(ref['m'][rows[0]])}"))
    return out


def check_step(*a, msg="", **kw):
    problems = step_errors(*a, **kw)
    assert not problems, f"{msg}: " + "; ".join(text for _, text in problems)


# SGD and Adagrad as test_opt_* write them: one accumulator h (ignored, and
# None allowed, for "sgd") and the hyper-parameters one by one.
def _h_slots(kind, h):
    return [] if kind == "sgd" else [h]


def step64(p, h, idx, grads, kind, lr, wd=0.0, eps=0.0):
    """step_ref with the new accumulator under "h"."""
    ref = step_ref(p, _h_slots(kind, h), idx, grads, hyper(kind, lr=lr, wd=wd, eps=eps))
    ref["h"] = ref["slots"][0] if ref["slots"] else None if h is None else np.asarray(h, dtype=F).copy()
    return ref


def step_errors64(p, h, idx, grads, p_got, h_got, dt, kind, lr, wd=0.0, eps=0.0):
    return step_errors(p, _h_slots(kind, h), idx, grads, p_got, _h_slots(kind, h_got), dt,
                       hyper(kind, lr=lr, wd=wd, eps=eps))


def check_step64(p, h, idx, grads, p_got, h_got, dt, kind, lr, wd=0.0, eps=0.0, msg=""):
    check_step(p, _h_slots(kind, h), idx, grads, p_got, _h_slots(kind, h_got), dt,
               hyper(kind, lr=lr, wd=wd, eps=eps), msg=msg)


# --------------------------------------------------------------- emulation
def emulate(p, slots, idx, grads, dt, hp, t=1, rng=None):
    """The kernel's operation order (opt_step_unit) in numpy arithmetic of type
    dt (no FMA), every kind of SLOT_NAMES:
    gsum = the losers' gradient rows added one by one into zero (in call order,
    or in a random order with `rng`), the winner = the key's LAST occurrence,
    d = (g_own + gsum) + wd * p, then the rule with every hyper-parameter
    rounded to dt once and a, b, 1 - beta computed in float64 first."""
    dt = np.dtype(dt).type
    p = np.asarray(p, dtype=dt)
    idx = np.asarray(idx, dtype=np.int64)
    g = np.asarray(grads, dtype=dt).reshape(idx.size, p.shape[1])
    order = np.arange(idx.size) if rng is None else rng.permutation(idx.size)
    last = np.full(p.shape[0], -1, dtype=np.int64)
    np.maximum.at(last, idx, np.arange(idx.size))
    losers = order[last[idx[order]] != order]
    gsum = np.zeros_like(p)
    # sequential adds per key: the j-th loser of every key in one vector operation
    rank = np.zeros(losers.size, dtype=np.int64)
    seen = {}
    for i, e in enumerate(losers):
        k = int(idx[e])
        rank[i] = seen.get(k, 0)
        seen[k] = rank[i] + 1
    for j in range(int(rank.max()) + 1 if losers.size else 0):
        sel = losers[rank == j]
        gsum[idx[sel]] = gsum[idx[sel]] + g[sel]
    rows = np.flatnonzero(last >= 0)
    own = g[last[rows]]
    lr, wd = dt(hp["lr"]), dt(hp["wd"])
    pr = p[rows]
    d = (own + gsum[rows]) + wd * pr
    pn = p.copy()
    sn = [np.asarray(s, dtype=dt).copy() for s in slots]
    if hp["kind"] == "sgd":
        pn[rows] = pr - lr * d
    elif hp["kind"] == "adagrad":
        h = sn[0][rows] + d * d
        sn[0][rows] = h
        pn[rows] = pr - lr * (d / (np.sqrt(h) + dt(hp["eps"])))
    elif hp["kind"] == "momentum":
        mu = dt(hp["mu"])
        v = mu * sn[0][rows] + d
        sn[0][rows] = v
        pn[rows] = pr - lr * ((d + mu * v) if hp["nesterov"] else v)
    else:
        a64, b64 = bias_corrections(hp, t, np.float64)
        a, b, eps = dt(a64), dt(b64), dt(hp["eps"])
        b1, b2 = dt(hp["beta1"]), dt(hp["beta2"])
        o1, o2 = dt(1.0 - np.float64(hp["beta1"])), dt(1.0 - np.float64(hp["beta2"]))
        mm = b1 * sn[0][rows] + o1 * d
        vv = b2 * sn[1][rows] + o2 * (d * d)
        sn[0][rows], sn[1][rows] = mm, vv
        pn[rows] = pr - a * (mm / (np.sqrt(vv) * b + eps))
    assert pn.dtype == dt and all(s.dtype == dt for s in sn)
    return pn, sn


# ------------------------------------------------------------------ inputs
def zero_slots(kind, shape, dt):
    return [np.zeros(shape, dtype=dt) for _ in range(SLOTS[kind])]


def dyadic_params(rng, rows, w, dt):
    """Multiples of 2^-4 in [-64, 64]."""
    return (rng.integers(-1024, 1025, size=(rows, w)) / 16.0).astype(dt)


def dyadic_grads(rng, n, w, dt):
    """Multiples of 2^-4 in [-8, 8]."""
    return (rng.integers(-128, 129, size=(n, w)) / 16.0).astype(dt)


def _steps(seed, kb, ke, n, w, pattern, steps, params, grads):
    """Initial parameters of the whole range and `steps` (keys, grads) calls of
    one key pattern, drawn afresh per step over the same range (overlapping key
    sets).  None if the pattern does not exist at this n."""
    rng = np.random.default_rng(seed)
    p0 = params(rng)
    calls = []
    for _ in range(steps):
        pats = key_patterns(rng, n, kb, ke)
        if pattern not in pats:
            return None
        calls.append((pats[pattern], grads(rng)))
    return p0, calls


def dyadic_steps(seed, kb, ke, n, w, pattern, dt, steps=3):
    """The dyadic cases: dyadic_params, dyadic_grads."""
    return _steps(seed, kb, ke, n, w, pattern, steps, lambda rng: dyadic_params(rng, ke - kb, w, dt),
                  lambda rng: dyadic_grads(rng, n, w, dt))


def bound_steps(seed, kb, ke, n, w, pattern, dt, steps=3):
    """The bound tests' case: normal initial parameters, normal * 3 gradients."""
    return _steps(seed, kb, ke, n, w, pattern, steps, lambda rng: rng.standard_normal((ke - kb, w)).astype(dt),
                  lambda rng: (rng.standard_normal((n, w)) * 3).astype(dt))


def case_seed(*parts):
    """A stable seed from a case's parameters (the CPU and GPU tests draw the same inputs)."""
    return zlib.crc32(repr(parts).encode())


# The bound tests' shapes (n, width, pattern) per layout.  all_equal stands
# only at n = 2: with thousands of occurrences of ONE key the rounding
# allowance (it grows with m * sum|g|) exceeds one dropped gradient, so that
# shape is left to the bit-exact dyadic tests (the CPU tests prove the
# checker's teeth on every case listed here).
BOUND_SHAPES = [(1, 1, "range_ends"), (2, 3, "all_equal"), (2049, 1, "dups_across_chunks"), (2049, 3, "dups_in_chunk"),
                (2049, 4, "distinct"), (4100, 16, "dups_across_chunks"), (4100, 33, "range_ends"),
                (2049, 64, "dups_in_chunk"), (4100, 4, "dups_in_chunk")]


def _bound_shapes():
    for li, (kb, ke) in enumerate(LAYOUTS):
        for si, (n, w, pat) in enumerate(BOUND_SHAPES):
            if pat == "distinct" and n > ke - kb:
                continue
            yield li, si, n, w, pat


def bound_cases():
    """test_opt_*: (layout index, n, width, pattern, kind, wd)."""
    return [(li, n, w, pat, kind, wd) for li, _, n, w, pat in _bound_shapes()
            for kind, wd in (("adagrad", 0.0), ("adagrad", 0.01), ("sgd", 0.01))]


def bound_cases2():
    """test_opt2_*: (layout index, n, width, pattern, kind, nesterov, wd).  Adam
    runs with both weight decays on every shape; momentum with two of its four
    (nesterov, wd) combinations per shape, alternating."""
    cases = []
    for li, si, n, w, pat in _bound_shapes():
        flip = (si + li) % 2
        for kind, nest, wd in (("momentum", False, (0.0, 0.01)[flip]), ("momentum", True, (0.01, 0.0)[flip]),
                               ("adam", False, 0.0), ("adam", False, 0.01)):
            cases.append((li, n, w, pat, kind, nest, wd))
    return cases


def case_hyper(case):
    _, _, _, _, kind, nest, wd = case
    return hyper(kind, wd=wd, nesterov=nest)


def bound_steps2(case, dt):
    """(p0, calls) of a bound_cases2 case."""
    li, n, w, pat = case[:4]
    kb, ke = LAYOUTS[li]
    return bound_steps(case_seed("opt2", case, np.dtype(dt).name), kb, ke, n, w, pat, np.dtype(dt))


def dyadic_hyper(nesterov):
    return hyper("momentum", lr=DYADIC_LR, mu=DYADIC_MU, nesterov=nesterov)


def dyadic_steps2(n, w, pat, li, dt):
    """test_opt2_*'s dyadic case (three steps)."""
    kb, ke = LAYOUTS[li]
    return dyadic_steps(case_seed("opt2", n, w, pat, li), kb, ke, n, w, pat, np.dtype(dt))
