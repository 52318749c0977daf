"""References of the factorization-machine pooled calls (include/pskv.h), plain
numpy from the stated formulas; the bounds are derived in DESIGN.md §8p.
The pull in float64; its bound per bag of m keys, u the unit roundoff:
    0.5 * 1.01 (2 m + W + 4) u sum_j [(sum_i |x_ij|)^2 + sum_i x_ij^2]
The push: `push_rows` in whatever type its inputs have -- the shard's type
restates the kernel's roundings one by one (numpy fuses nothing), longdouble is
the reference.  Its tolerance is opt_util's with, per occurrence of a key,
    magnitude  A_i = |w_i| (|c_b| sum_i' |x_i'| + |bag_grads[b]|) + |e_i p_i|
    roundings  m grows by the longest bag + 4 (S_b; c S, + bag_grads, w t, the difference)."""
import numpy as np

import opt_util as ou
from rows_util import U_ROUND

F = ou.F
KINDS = {"sgd": 0, "adagrad": 1, "momentum": 1, "adam": 2, "ftrl": 2}  # kind -> state slots


def set_optimizer(sh, kind, wd=0.01):
    kw = {"l1": 0.05, "l2": 0.01} if kind == "ftrl" else {"eps": ou.BOUND_EPS, "momentum": ou.BOUND_MU}
    sh.set_optimizer(kind, lr=ou.BOUND_LR, weight_decay=wd, init_accum=ou.BOUND_INIT_ACCUM, **kw)


def state(sh, keys):
    """[p, slot 0, ...] of `keys`, (len(keys), W) each."""
    n = KINDS[sh.optimizer()["kind"]]
    return [np.asarray(a).reshape(len(keys), sh.width)
            for a in [sh.get(keys)] + [sh.get_state(keys, slot=i) for i in range(n)]]


def terms(p, idx, weights, f):
    x = np.asarray(p, dtype=f)[idx]
    return x if weights is None else np.asarray(weights, dtype=f)[:, None] * x


def pull_ref(p, idx, off, weights, dt):
    """(S (nbags, W), pair (nbags,), tolerance of pair (nbags,)) in float64; idx: the row of every key position."""
    x = terms(p, idx, weights, np.float64)
    nb, w = len(off) - 1, x.shape[1]
    S, pair, tol = np.zeros((nb, w)), np.zeros(nb), np.zeros(nb)
    for b in range(nb):
        xb = x[int(off[b]):int(off[b + 1])]
        S[b], Q = xb.sum(0), (xb * xb).sum(0)
        pair[b] = 0.5 * (S[b] * S[b] - Q).sum()
        tol[b] = 0.5 * 1.01 * (2 * len(xb) + w + 4) * U_ROUND[np.dtype(dt)] * (np.abs(xb).sum(0) ** 2 + Q).sum()
    return S, pair, tol


def push_rows(prow, S, bag, c, weights, bag_grads):
    """rows (n, W) by the header's expression, in the type of prow (the pre-step row of every position)."""
    f = prow.dtype.type
    t = np.asarray(c, dtype=f)[:, None] * np.asarray(S, dtype=f)
    if bag_grads is not None:
        t = t + np.asarray(bag_grads, dtype=f).reshape(t.shape)
    cb = np.asarray(c, dtype=f)[bag]
    if weights is None:
        return t[bag] - cb[:, None] * prow
    w = np.asarray(weights, dtype=f)
    return w[:, None] * t[bag] - (cb * (w * w))[:, None] * prow


def push_prepare(p, slots, idx, off, c, weights, bag_grads, dt, hp, t=1):
    """opt_util.prepare of an FM push from the pre-step (p, slots): the
    reference step in longdouble and the tolerances above."""
    bag = np.repeat(np.arange(len(off) - 1), np.diff(np.asarray(off).astype(np.int64)))
    x = terms(p, idx, weights, F)
    S = np.zeros((len(off) - 1, x.shape[1]), dtype=F)
    A = np.zeros_like(S)
    np.add.at(S, bag, x)
    np.add.at(A, bag, np.abs(x))
    prow = np.asarray(p, dtype=F)[idx]
    rows = push_rows(prow, S, bag, c, weights, bag_grads)
    w = np.ones(len(idx), dtype=F) if weights is None else np.abs(np.asarray(weights, dtype=F))
    cb = np.abs(np.asarray(c, dtype=F))[bag]
    mag = np.abs(np.asarray(c, dtype=F))[:, None] * A
    if bag_grads is not None:
        mag = mag + np.abs(np.asarray(bag_grads, dtype=F).reshape(mag.shape))
    mag = w[:, None] * mag[bag] + (cb * w * w)[:, None] * np.abs(prow)
    ref = ou.step_ref(p, slots, idx, rows, hp, t)
    G = np.zeros_like(ref["G"])
    np.add.at(G, idx, mag)
    extra = int(np.diff(np.asarray(off).astype(np.int64)).max()) + 4
    ref = dict(ref, G=G, m=ref["m"] + extra * (ref["m"] > 0))
    return (ref,) + ou.tolerances(ref, p, slots, dt, hp, t)


def draw_push(rng, rows, lens, w, dt, weighted, with_grads, distinct):
    """A push over `rows` stored rows: (idx, offsets, c, weights, bag_grads).
    distinct: every row at most once; else rows repeat inside a bag (the first
    two positions hold the same row) and across bags."""
    n = int(sum(lens))
    idx = rng.permutation(rows)[:n] if distinct else rng.integers(0, rows, n)
    if not distinct:
        idx[1] = idx[0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    c = rng.standard_normal(len(lens)).astype(dt)
    wts = rng.standard_normal(n).astype(dt) if weighted else None
    bg = rng.standard_normal((len(lens), w)).astype(dt) if with_grads else None
    return idx.astype(np.int64), off, c, wts, bg


def sums_in(dt, p, idx, off, weights):
    """S of every bag in the type dt, term after term in key order."""
    x = terms(p, idx, weights, dt)
    S = np.zeros((len(off) - 1, x.shape[1]), dtype=dt)
    for b in range(len(off) - 1):
        for i in range(int(off[b]), int(off[b + 1])):
            S[b] = S[b] + x[i]
    return S
