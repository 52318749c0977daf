"""The oracle and the checker of optimizer steps (pskv_apply), shared by
tests/test_opt_cpu.py and tests/test_opt_gpu.py.

One call is one step (include/pskv.h "Optimizer steps"):
  1. g[k] = sum of the gradient rows of all occurrences of key k in the call
  2. d = g + wd * p;  SGD: p <- p - lr * d
                      Adagrad: h <- h + d*d;  p <- p - lr * d / (sqrt(h) + eps)
  3. keys not in the call keep p and h bit for bit

`step64` restates that from a given (p, h), in numpy's extended precision
(np.longdouble, u = 2^-64 where the platform has it): a float64 reference
would carry roundings of its own as large as a float64 shard's, and the
tolerances below leave no room for a second set.  `check_step` makes the
ONE-STEP check: the test reads the shard's own p (and h) of the whole range
before a step, runs one float64 step from those, and compares every element
afterwards.  With u = 2^-24 / 2^-53, m the occurrences of the key, G = sum|g_i|
per element, D = G + wd |p| and dd = 1.01 (m + 3) u D (DESIGN.md §8c derives
them by counting roundings):
  SGD         |p^' - p'| <= 1.01 u (|p'| + (m + 5) lr D)
  Adagrad h   |h^' - h'| <= 1.01 u (h' + (2m + 8) D D)
  Adagrad p   |p^' - p'| <= 1.01 u |p'|
                            + lr (dd / (sqrt(h + max(|d| - dd, 0)^2) + eps) + 8 * 1.01 u |r|),
              r = d / (sqrt(h') + eps)
  untouched   bit-identical p and h
"""
import numpy as np

from rows_util import U_ROUND, bits, key_patterns

# the bound tests' hyper-parameters (tests/test_opt_gpu.py; test_opt_cpu.py
# proves the checker rejects wrong semantics on exactly these inputs)
BOUND_LR, BOUND_EPS, BOUND_INIT_ACCUM = 0.05, 1e-8, 0.1
# the dyadic SGD cases: every sum, product and difference exact in float32
DYADIC_LR = 2.0**-3
F = np.longdouble  # the reference's arithmetic


def step64(p, h, idx, grads, kind, lr, wd=0.0, eps=0.0):
    """One step in the reference's precision.  p, h: (R, W) arrays (h ignored for "sgd"); idx: row
    index of every occurrence; grads: (n, W).  Returns a dict: p, h (new arrays),
    m (R,) occurrences, G (R, W) sum|g_i|, d (R, W)."""
    p = np.asarray(p, dtype=F)
    w = p.shape[1]
    idx = np.asarray(idx, dtype=np.int64)
    lr, wd, eps = F(lr), F(wd), F(eps)
    g64 = np.asarray(grads, dtype=F).reshape(idx.size, w)
    g = np.zeros_like(p)
    G = np.zeros_like(p)
    m = np.zeros(p.shape[0], dtype=np.int64)
    np.add.at(g, idx, g64)
    np.add.at(G, idx, np.abs(g64))
    np.add.at(m, idx, 1)
    hit = m > 0
    d = np.where(hit[:, None], g + wd * p, F(0))
    pn = p.copy()
    hn = None if h is None else np.asarray(h, dtype=F).copy()
    if kind == "sgd":
        pn[hit] = p[hit] - lr * d[hit]
    elif kind == "adagrad":
        hn[hit] = hn[hit] + d[hit] * d[hit]
        pn[hit] = p[hit] - lr * d[hit] / (np.sqrt(hn[hit]) + eps)
    else:
        raise ValueError(kind)
    return {"p": pn, "h": hn, "m": m, "G": G, "d": d}


def tolerances(ref, p, h, dt, kind, lr, wd, eps):
    """(tol_p, tol_h) per element for a step `ref` = step64(p, h, ...) (tol_h None for sgd)."""
    u = U_ROUND[np.dtype(dt)]
    p = np.asarray(p, dtype=F)
    m = ref["m"][:, None].astype(F)
    D = ref["G"] + wd * np.abs(p)
    if kind == "sgd":
        return 1.01 * u * (np.abs(ref["p"]) + (m + 5) * lr * D), None
    h = np.asarray(h, dtype=F)
    dd = 1.01 * (m + 3) * u * D
    tol_h = 1.01 * u * (ref["h"] + (2 * m + 8) * D * D)
    r = ref["d"] / (np.sqrt(ref["h"]) + eps)
    lo = np.maximum(np.abs(ref["d"]) - dd, F(0))
    tol_p = 1.01 * u * np.abs(ref["p"]) + lr * (dd / (np.sqrt(h + lo * lo) + eps) + 8 * 1.01 * u * np.abs(r))
    return tol_p, tol_h


def step_errors(p, h, idx, grads, p_got, h_got, dt, kind, lr, wd=0.0, eps=0.0):
    """The one-step check as data: a list of problems (empty = the step is right).
    p, h: the shard's rows before the step; p_got, h_got: after."""
    dt = np.dtype(dt)
    ref = step64(p, h, idx, grads, kind, lr, wd, eps)
    tol_p, tol_h = tolerances(ref, p, h, dt, kind, lr, wd, eps)
    hit = ref["m"] > 0
    out = []
    pairs = [("p", np.asarray(p), np.asarray(p_got), ref["p"], tol_p)]
    if kind == "adagrad":
        pairs.append(("h", np.asarray(h), np.asarray(h_got), ref["h"], tol_h))
    for name, before, got, want, tol in pairs:
        assert got.dtype == dt and before.dtype == dt, (name, got.dtype, before.dtype, dt)
        same = bits(before[~hit]) == bits(got[~hit])
        if not same.all():
            out.append(f"{name}: {int((~same).sum())} elements of untouched keys changed")
        err = np.abs(got[hit].astype(F) - want[hit])
        bad = ~(err <= tol[hit])  # (a NaN fails)
        if bad.any():
            rows = np.flatnonzero(hit)[np.argwhere(bad)[:, 0]]
            i = tuple(np.argwhere(bad)[0])
            out.append(f"{name}: {int(bad.sum())} elements beyond the tolerance, rows {rows[:3].tolist()}: "
                       f"err {err[i]:.3e} tol {tol[hit][i]:.3e} m {int(ref['m'][rows[0]])}")
    return out


def check_step(*a, msg="", **kw):
    problems = step_errors(*a, **kw)
    assert not problems, f"{msg}: " + "; ".join(problems)


# ------------------------------------------------------------------ inputs
def dyadic_params(rng, rows, w, dt):
    """Multiples of 2^-4 in [-64, 64]."""
    return (rng.integers(-1024, 1025, size=(rows, w)) / 16.0).astype(dt)


def dyadic_grads(rng, n, w, dt):
    """Multiples of 2^-4 in [-8, 8]."""
    return (rng.integers(-128, 129, size=(n, w)) / 16.0).astype(dt)


def dyadic_steps(seed, kb, ke, n, w, pattern, dt, steps=3):
    """The dyadic SGD case: initial parameters of the whole range and `steps`
    (keys, grads) calls of one key pattern, drawn afresh per step over the same
    range (overlapping key sets).  None if the pattern does not exist at this n."""
    rng = np.random.default_rng(seed)
    p0 = dyadic_params(rng, ke - kb, w, dt)
    calls = []
    for _ in range(steps):
        pats = key_patterns(rng, n, kb, ke)
        if pattern not in pats:
            return None
        calls.append((pats[pattern], dyadic_grads(rng, n, w, dt)))
    return p0, calls


def bound_steps(seed, kb, ke, n, w, pattern, dt, steps=3):
    """The bound tests' case: normal initial parameters, normal * 3 gradients."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal((ke - kb, w)).astype(dt)
    calls = []
    for _ in range(steps):
        pats = key_patterns(rng, n, kb, ke)
        if pattern not in pats:
            return None
        calls.append((pats[pattern], (rng.standard_normal((n, w)) * 3).astype(dt)))
    return p0, calls


# The bound tests' parametrisation: (layout index, n, width, pattern, kind, wd).
# all_equal stands only at n = 2: with thousands of occurrences of ONE key the
# rounding allowance (it grows with m * sum|g|) exceeds one dropped gradient,
# so that shape is left to the bit-exact dyadic tests (test_opt_cpu.py proves
# the checker's teeth on every case listed here).
def bound_cases():
    from rows_util import LAYOUTS

    cases = []
    shapes = [(1, 1, "range_ends"), (2, 3, "all_equal"), (2049, 1, "dups_across_chunks"), (2049, 3, "dups_in_chunk"),
              (2049, 4, "distinct"), (4100, 16, "dups_across_chunks"), (4100, 33, "range_ends"),
              (2049, 64, "dups_in_chunk"), (4100, 4, "dups_in_chunk")]
    for li, (kb, ke) in enumerate(LAYOUTS):
        for n, w, pat in shapes:
            if pat == "distinct" and n > ke - kb:
                continue
            for kind, wd in (("adagrad", 0.0), ("adagrad", 0.01), ("sgd", 0.01)):
                cases.append((li, n, w, pat, kind, wd))
    return cases


def case_seed(*parts):
    """A stable seed from a case's parameters (the CPU and GPU tests draw the same inputs)."""
    import zlib

    return zlib.crc32(repr(parts).encode())
