"""The reference and the checker of pooled pushes (pskv_apply_pooled), built on
tests/opt_util.py and tests/pooled_util.py.

One call is pskv_apply's step with the gradient row of key position i formed in
the shard: rows[i] = weights[i] * bag_grads[bag(i)] (include/pskv.h "Pooled
pushes").  The reference forms those rows in np.longdouble and feeds them to
opt_util.step_ref; the check is opt_util's one-step check.

Tolerances: opt_util.tolerances with m + 1 in the place of m for the keys of a
WEIGHTED call, m as it is when weights is None (the term is then the bag's row
itself).  Derived, not measured: every term w_i * bg carries one more relative
rounding u than a pushed gradient row, so |d^ - d| grows by at most u * G and
dd = 1.01 (m + 3) u D becomes 1.01 (m + 4) u D; every tolerance is a function
of m through dd and the (m + c) factors alone, and all of them grow with m.
tests/test_pooled_push_cpu.py checks the derivation against an emulation of
the kernels' order and proves the checker rejects three wrong semantics.
"""
import numpy as np

import opt_util as ou
import pooled_util as pu
from rows_util import key_patterns

F = ou.F
GENERAL_CHUNK = pu._constant("kGeneralChunk", "pskv_internal.h")  # positions per virtual workgroup
KINDS = [("sgd", False), ("adagrad", False), ("momentum", False), ("momentum", True), ("adam", False)]
BAG_PATTERNS = ["ones", "eights", "mixed", "one_bag", "boundary"]


def hyper(kind, nesterov=False, wd=0.0):
    """The bound tests' hyper-parameters (opt_util's)."""
    return ou.hyper(kind, wd=wd, nesterov=nesterov)


def set_optimizer(sh, hp):
    """Shard.set_optimizer for any kind (Adagrad starts from opt_util.BOUND_INIT_ACCUM)."""
    sh.set_optimizer(hp["kind"], lr=hp["lr"], weight_decay=hp["wd"], eps=hp["eps"], init_accum=ou.BOUND_INIT_ACCUM,
                     momentum=hp["mu"], nesterov=hp["nesterov"], beta1=hp["beta1"], beta2=hp["beta2"])


def initial_slots(kind, shape, dt):
    if kind == "adagrad":
        return [np.full(shape, ou.BOUND_INIT_ACCUM, dtype=dt)]
    return ou.zero_slots(kind, shape, dt)


def bag_lens(name, n):
    """Bag lengths that sum to n.  mixed: pooled pulls' list around the pull's
    chunk, an empty first and an empty last bag; boundary: a bag ends exactly at
    the workgroup boundary (position kGeneralChunk, or n // 2 for a shorter
    call) with two empty bags there; one_bag: one bag covers every workgroup."""
    c = pu.CHUNK
    if name == "ones":
        return [1] * n
    if name == "eights":
        return [8] * (n // 8) + ([n % 8] if n % 8 else [])
    if name == "one_bag":
        return [n]
    if name == "mixed":
        menu = [1, 5, c + 1, 0, 3 * c + 2, 17, c, 2]
        lens, left, i = [0], n, 0
        while left:
            m = min(menu[i % len(menu)], left)
            lens.append(m)
            left -= m
            i += 1
        return lens + [0]
    if name == "boundary":
        cut = GENERAL_CHUNK if n > GENERAL_CHUNK else n // 2
        head = [3] * (cut // 3) + ([cut % 3] if cut % 3 else [])
        rest = n - cut
        tail = [rest // 2, rest - rest // 2] if rest > 1 else ([rest] if rest else [])
        return head + [0, 0] + tail
    raise ValueError(name)


def bag_index(offsets):
    lens = np.diff(np.asarray(offsets).astype(np.int64))
    return np.repeat(np.arange(lens.size), lens)


def expand(weights, bag_grads, bag, dt):
    """The host-expanded rows of pskv_apply's twin: each fl_T(w_i * bg), one rounding."""
    bg = np.asarray(bag_grads, dtype=dt).reshape(-1, np.asarray(bag_grads).shape[-1] if np.ndim(bag_grads) > 1 else 1)
    rows = bg[bag]
    if weights is None:
        return rows.copy()
    out = np.asarray(weights, dtype=dt)[:, None] * rows
    assert out.dtype == np.dtype(dt)
    return out


def ref_grads(weights, bag_grads, bag):
    """The reference's rows, in np.longdouble."""
    rows = np.asarray(bag_grads, dtype=F)[bag]
    return rows if weights is None else np.asarray(weights, dtype=F)[:, None] * rows


def prepare(p, slots, idx, weights, bag_grads, bag, dt, hp, t=1):
    """opt_util.prepare of the step, with the pooled push's tolerances."""
    ref = ou.step_ref(p, slots, idx, ref_grads(weights, bag_grads, bag), hp, t)
    if weights is not None:
        ref = dict(ref, m=ref["m"] + (ref["m"] > 0))
    return (ref,) + ou.tolerances(ref, p, slots, dt, hp, t)


def step_errors(p, slots, idx, weights, bag_grads, bag, p_got, slots_got, dt, hp, t=1, pre=None):
    pre = pre or prepare(p, slots, idx, weights, bag_grads, bag, dt, hp, t)
    return ou.step_errors(p, slots, idx, None, p_got, slots_got, dt, hp, t, pre=pre)


def check_step(*a, msg="", **kw):
    problems = step_errors(*a, **kw)
    assert not problems, f"{msg}: " + "; ".join(text for _, text in problems)


def draw_call(rng, n, w, pattern, bagpat, kb, ke, dt, weighted, dyadic=False):
    """(keys, offsets, bag_grads (nbags, w), weights or None).  dyadic: bag rows
    multiples of 2^-4 in [-4, 4] and weights in {-2, -1, 0, 1, 2}, so every
    product is one of opt_util.dyadic_grads' values."""
    keys = key_patterns(rng, n, kb, ke)[pattern]
    off = pu.offsets_of(bag_lens(bagpat, n))
    nbags = off.size - 1
    if dyadic:
        bg = (rng.integers(-64, 65, size=(nbags, w)) / 16.0).astype(dt)
        wts = rng.integers(-2, 3, size=n).astype(dt) if weighted else None
    else:
        bg = (rng.standard_normal((nbags, w)) * 3).astype(dt)
        wts = rng.standard_normal(n).astype(dt) if weighted else None
    return keys, off, bg, wts


def emulate_any(p, slots, idx, grads, dt, hp, t=1, rng=None):
    """The kernels' order in numpy arithmetic of type dt for every kind:
    opt_util.emulate for momentum and Adam; SGD and Adagrad as a loop per key
    (the losers' rows added one by one into zero, the winner = the key's last
    occurrence, d = (g_own + gsum) + wd * p)."""
    if hp["kind"] in ("momentum", "adam"):
        return ou.emulate(p, slots, idx, grads, dt, hp, t, rng)
    dt = np.dtype(dt).type
    pn = np.asarray(p, dtype=dt).copy()
    sn = [np.asarray(s, dtype=dt).copy() for s in slots]
    g = np.asarray(grads, dtype=dt)
    idx = np.asarray(idx, dtype=np.int64)
    lr, wd, eps = dt(hp["lr"]), dt(hp["wd"]), dt(hp["eps"])
    for k in np.unique(idx):
        occ = np.flatnonzero(idx == k)
        losers = occ[:-1] if rng is None else rng.permutation(occ[:-1])
        gsum = np.zeros(pn.shape[1], dtype=dt)
        for i in losers:
            gsum = gsum + g[i]
        d = (g[occ[-1]] + gsum) + wd * pn[k]
        if hp["kind"] == "adagrad":
            sn[0][k] = sn[0][k] + d * d
            pn[k] = pn[k] - lr * (d / (np.sqrt(sn[0][k]) + eps))
        else:
            pn[k] = pn[k] - lr * d
    assert pn.dtype == dt
    return pn, sn


def apply_pooled(sh, keys, offsets, bag_grads, weights, cuda=None, bg_offset=0):
    """One pooled push through the host path (cuda None) or the device path;
    bg_offset > 0: the device bag rows start that many elements into a larger
    buffer (the element path)."""
    if cuda is None:
        sh.apply_pooled(keys, offsets, bag_grads, weights)
        return
    import torch

    from test_gpu_parity import tdev

    dk = tdev(np.asarray(keys, dtype=np.uint32), cuda)
    do = torch.from_numpy(np.asarray(offsets).astype(np.int64)).to(cuda)
    dw = None if weights is None else tdev(np.asarray(weights, dtype=sh.dtype), cuda)
    dg = tdev(np.ascontiguousarray(bag_grads, dtype=sh.dtype).reshape(-1), cuda, bg_offset)
    sh.apply_pooled(dk, do, dg, dw)
