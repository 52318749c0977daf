"""Inputs and checkers of the special-value tests (tests/test_edge_cpu.py,
tests/test_edge_gpu.py): non-finite, subnormal and overflowing values on every
path that writes floats.

Lattice accumulate.  A pushed value is scale * integer: ordinary integers in
[-3, 3], a few per call up to +-2^22, and per key sum |integer| < 2^24 (the
generator asserts it).  Every partial sum of a key, in every order, is then an
integer below 2^24 times the scale: exact in float32 and float64, at scale 1
and at scale = finfo.smallest_subnormal.  The expectation is the int64 sum
times the scale (a zero sum is +0) and the comparison is bits(): no tolerance.
In float32 the subnormal range ends at 2^23 lattice units, so the clean hot
key, which takes three +-2^22 addends of one sign, crosses into the normal
range (float64's boundary, 2^52 units, is out of the lattice's reach).
Special occurrences are planted on reserved keys, one column each, and fix the
element's class whatever the order: a NaN or both infinities give NaN, one
infinity gives itself, max + max gives +inf, -0.0 onto +0 gives +0.

Steps with special values.  `edge_steps` draws opt_util.bound_steps' case on the
dups_across_chunks pattern (every key twice: position i the loser, whose row
travels through gsum, position i + per the winner) and plants NaN, +-inf,
finfo.max, a subnormal and -0.0 on a winner, on a loser and on a key present
once, and both infinities on one key.  A key has at most two occurrences, so a
tainted element is one commutative addition: its class, and its bits where
finite, do not depend on the order (`order_problems` checks it, cap zero).
`edge_step_errors` accepts an element iff the dt emulation is NaN and so is the
shard, or it is an infinity and the shard holds the same one, or their bits
are equal, or the shard lies within the (finite) tolerance of the
extended-precision reference.

Residue.  `residue_case`: a first step whose losers leave a NaN, an infinity,
both infinities, a subnormal sum or an exact zero in gsum; then new parameters
and state, zeros and ones on the probe keys so that a stale subnormal shows
(Adagrad: p = -lr * stale; Adam: m = (1 - beta1) * stale; FTRL: z = stale);
then two steps on distinct keys, the first with zero gradients on the probes.

Subnormal-scale dyadic steps.  The dyadic cases are multiples of 2^-4; with
lr = 2^-3 an SGD step reaches multiples of 2^-7 and stays there (wd = 0).
Momentum with mu = 1/2: v_1 is a multiple of 2^-4, v_2 of 2^-5, v_3 of 2^-6,
so p_3 = p_2 - lr v_3 reaches 2^-9; Nesterov's d + mu v_3 reaches 2^-7 and
its p_3 2^-10.  Every input is multiplied by 2^e with 2^e * granule =
4 * smallest_subnormal (`dyadic_exp`); the rules are homogeneous of degree one,
so the expectations are the unscaled ones times 2^e, exactly.  With that
granule the drawn values do NOT straddle the normal range: a gradient is at
most 2^15 units of smallest_subnormal and the normal range starts at 2^23
units in float32 (2^52 in float64); only a sum of thousands of equal-signed
gradients on one key could get there.  These cases are subnormal arithmetic;
the subnormal/normal boundary is crossed by the lattice's hot key alone.
"""
import numpy as np

import ftrl_util as fu
import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
from rows_util import bits, key_patterns

F = ou.F
HAVE_EXTENDED = bool(np.finfo(np.longdouble).max > np.finfo(np.float64).max)
SUB_EXP = {np.dtype(np.float32): -149, np.dtype(np.float64): -1074}
SCALES = ["one", "sub"]
BIG = 2**22
LIMIT = 2**24


def scale_exp(dt, scale):
    dt = np.dtype(dt)
    assert np.ldexp(dt.type(1), SUB_EXP[dt]) == np.finfo(dt).smallest_subnormal
    return {"one": 0, "sub": SUB_EXP[dt]}[scale]


def special_value(name, dt):
    fi = np.finfo(dt)
    return np.dtype(dt).type({"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "max": fi.max,
                              "sub": 5 * fi.smallest_subnormal, "-0": -0.0}[name])


# ---------------------------------------------------------------- lattice
class Lattice:
    """The exact expectation of an accumulate shard of `slots` rows of width w
    (a dense shard's out-of-range keys are slots after its range)."""

    def __init__(self, dt, scale, slots, w):
        self.dt, self.e, self.w = np.dtype(dt), scale_exp(dt, scale), int(w)
        self.sum = np.zeros((slots, w), dtype=np.int64)
        self.abs = np.zeros((slots, w), dtype=np.int64)
        self.nan, self.pinf, self.ninf = (np.zeros((slots, w), dtype=bool) for _ in range(3))
        self.nmax = np.zeros((slots, w), dtype=np.int64)

    def values(self, ints):
        return np.ldexp(np.asarray(ints).astype(self.dt), self.e)

    def add(self, idx, ints, special=()):
        """One call: occurrence i adds ints[i] to slot idx[i]; special: (position,
        column, name) replaces that element.  Returns the (n, w) values to push."""
        idx = np.asarray(idx, dtype=np.int64)
        ints = np.array(ints, dtype=np.int64).reshape(idx.size, self.w)
        for pos, col, _ in special:
            ints[pos, col] = 0
        vals = self.values(ints)
        for pos, col, name in special:
            vals[pos, col] = special_value(name, self.dt)
            at = (idx[pos], col)
            if name == "nan":
                self.nan[at] = True
            elif name == "+inf":
                self.pinf[at] = True
            elif name == "-inf":
                self.ninf[at] = True
            elif name == "max":
                self.nmax[at] += 1
            else:
                assert name == "-0", name
        np.add.at(self.sum, idx, ints)
        np.add.at(self.abs, idx, np.abs(ints))
        assert self.abs.max() < LIMIT, "a key's sum |integer| reaches 2^24: its partial sums may round"
        return vals

    def tainted(self):
        return self.nan | self.pinf | self.ninf | (self.nmax > 0)

    def want(self):
        """The (slots, w) expectation: NaN where the class is NaN, else the bits."""
        assert not (self.nmax == 1).any(), "one finfo.max alone: plant two"
        assert not ((self.nmax > 0) & (self.nan | self.pinf | self.ninf)).any()
        out = self.values(self.sum)
        assert not np.signbit(out[self.sum == 0]).any()
        nan = self.nan | (self.pinf & self.ninf)
        out[(self.pinf | (self.nmax >= 2)) & ~nan] = np.inf
        out[self.ninf & ~nan] = -np.inf
        out[nan] = np.nan
        return out


def lattice_problems(got, want, msg=""):
    """None, or what differs: a NaN expectation wants a NaN, anything else its bits."""
    want = np.asarray(want)
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    nan = np.isnan(want)
    ok = np.where(nan, np.isnan(got), bits(got) == bits(want))
    if ok.all():
        return None
    bad = np.argwhere(~ok)
    i = tuple(bad[0])
    return (f"{msg}: {len(bad)} elements differ, first (slot, col) {bad[:3].tolist()}: got {got[i]!r} "
            f"(bits {int(bits(got)[i]):#x}) want {want[i]!r} (bits {int(bits(want)[i]):#x})")


# reserved slots of a general call (the ordinary occurrences start at ORDINARY)
FIRST, HOT, TAINTED_HOT, ONCE_PINF, MAXMAX, ONCE_NEG0, ONCE_CLEAN, ORDINARY = 0, 5, 7, 9, 11, 13, 15, 16


def general_call(rng, lat, n, rows, extra=0, bigs=True):
    """One call of n occurrences in any order over slots [0, rows) and `extra`
    (0 or 2) slots behind them.  A clean hot key takes n // 4 of them and a
    NaN-tainted one n // 2; -inf sits on the first key at call position 2047,
    +inf and -inf on the last key (+inf at position 2048), +inf alone and -0.0
    alone on keys with one occurrence, max twice on one key; with `extra`, +inf
    on the first extra slot and plain lattice values on the second.  bigs: the
    +-2^22 addends (once per shard: three of them fill the clean hot key's
    allowance).  Returns (idx (n,), vals (n, w))."""
    w = lat.w
    assert n >= 128 and rows >= 64
    last = rows - 1
    pa, pb = (2047, 2048) if n > 2048 else (n // 2 - 1, n // 2)
    span = max(8, min(rows - ORDINARY - 1, n // 8 + 1))
    idx = ORDINARY + rng.integers(0, span, size=n)
    free = rng.permutation(np.setdiff1d(np.arange(n), [pa, pb]))
    at = [0]

    def take(m):
        out = free[at[0]:at[0] + m]
        at[0] += m
        assert out.size == m
        return out

    thot, hot = take(n // 2), take(n // 4)
    firsts, lasts, once_pinf, maxes, neg0, clean = take(2), take(3), take(1), take(4), take(1), take(1)
    idx[thot], idx[hot], idx[firsts], idx[lasts] = TAINTED_HOT, HOT, FIRST, last
    idx[once_pinf], idx[maxes], idx[neg0], idx[clean] = ONCE_PINF, MAXMAX, ONCE_NEG0, ONCE_CLEAN
    idx[pa], idx[pb] = FIRST, last
    col = [0]

    def nextcol():
        col[0] += 1
        return (col[0] - 1) % w

    c = nextcol()
    special = [(int(thot[thot.size // 2]), c, "nan")]
    special.append((int(once_pinf[0]), nextcol(), "+inf"))
    special.append((pa, nextcol(), "-inf"))
    c = nextcol()
    special += [(pb, c, "+inf"), (int(lasts[0]), c, "-inf")]
    c = nextcol()
    special += [(int(maxes[0]), c, "max"), (int(maxes[1]), c, "max")]
    special.append((int(neg0[0]), nextcol(), "-0"))
    if extra:
        assert extra == 2
        ex = take(5)
        idx[ex[:3]], idx[ex[3:]] = rows, rows + 1
        special.append((int(ex[0]), nextcol(), "+inf"))
    ints = rng.integers(-3, 4, size=(n, w))
    if bigs:
        sign = rng.choice([-1, 1], size=w)
        ints[hot[:3]] = BIG * sign  # one sign per column: the sum passes 2^23 units
        ints[thot[0]] = rng.integers(BIG // 4, BIG + 1, size=w) * rng.choice([-1, 1], size=w)
        ordinary = free[at[0]:]
        for p in ordinary[:2]:
            ints[p] = rng.integers(BIG // 4, BIG + 1, size=w) * rng.choice([-1, 1], size=w)
    return idx, lat.add(idx, ints, special)


def window_calls(rng, lat, rows, aligned, lookalike=False, lengths=(1, 3, 1000, 8191, 8192, 20_001)):
    """Dense windows (one batch each, a key once per window) over slots
    [0, rows - 1): the last two overlap, and carry +inf / -inf on one key and
    max twice on the next; NaN, +inf and -inf sit alone in the others; one more
    window of one key, the last slot, holds -0.0.  aligned: every window starts
    at a multiple of 4 (the 16-byte RMW).  lookalike: the first window of 1000
    keys or more swaps two keys and repeats one, still sorted at its ends.
    Returns [(idx, vals), ...]."""
    w = lat.w
    wins = []
    for i, n in enumerate(lengths):
        first = int(rng.integers(0, rows - 1 - n + 1))
        if i == len(lengths) - 1:  # overlaps the one before it
            pf, pn = int(wins[-1][0]), wins[-1].size
            first = min(pf + pn // 2, rows - 1 - n)
        first -= first % 4 if aligned else 0
        if not aligned and first % 4 == 0 and first + n < rows - 1:
            first += 1
        wins.append(np.arange(first, first + n, dtype=np.int64))
    a, b = wins[-2], wins[-1]
    both = np.intersect1d(a, b)
    assert both.size >= 2
    planted = {len(wins) - 2: [(int(both[0] - a[0]), "+inf"), (int(both[1] - a[0]), "max")],
               len(wins) - 1: [(int(both[0] - b[0]), "-inf"), (int(both[1] - b[0]), "max")],
               2: [(wins[2].size // 2, "nan")], 1: [(0, "+inf")], 3: [(wins[3].size - 1, "-inf")]}
    # the singles must not fall on a key that another special taints otherwise
    out = []
    big_left = 3
    for i, k in enumerate(wins):
        k = k.copy()
        if lookalike and k.size >= 1000:
            k[10], k[11] = k[11], k[10]
            k[500] = k[499]
            lookalike = False
        ints = rng.integers(-3, 4, size=(k.size, w))
        if k.size >= 1000 and big_left:
            ints[k.size // 3] = rng.integers(BIG // 4, BIG + 1, size=w) * rng.choice([-1, 1], size=w)
            big_left -= 1
        special = [(pos, (i + j) % w, name) for j, (pos, name) in enumerate(planted.get(i, []))]
        if i in (len(wins) - 2, len(wins) - 1):  # the pair shares its columns
            special = [(pos, j % w, name) for j, (pos, name) in enumerate(planted[i])]
        out.append((k, lat.add(k, ints, special)))
    k = np.array([rows - 1], dtype=np.int64)
    out.append((k, lat.add(k, np.zeros((1, w), dtype=np.int64), [(0, 0, "-0")])))
    return out


def small_messages(rng, lat, rows, count, max_n, extra=2):
    """Host messages of 128..max_n keys for the inline and request-server paths:
    general_call's layout per message (the +-2^22 addends in the first only)."""
    out = []
    for i in range(count):
        n = max_n if i % 3 == 0 else int(rng.integers(128, max_n + 1))
        out.append(general_call(rng, lat, n, rows, extra=extra, bigs=i == 0))
    return out


# ------------------------------------------------------------------ steps
STEP_SPECIALS = ["nan", "+inf", "-inf", "max", "sub", "-0"]
KINDS = ["sgd", "adagrad", "momentum", "nesterov", "adam", "ftrl"]


def kind_hyper(kind, wd=0.01):
    """The bound tests' hyper-parameters of a kind of KINDS."""
    if kind == "ftrl":
        return fu.hyper(wd=wd)
    return ou.hyper("momentum" if kind == "nesterov" else kind, wd=wd, nesterov=kind == "nesterov")


def set_optimizer(sh, hp):
    if hp["kind"] == "ftrl":
        fu.set_optimizer(sh, hp)
    else:
        ppu.set_optimizer(sh, hp)


def slot_count(hp):
    return 2 if hp["kind"] == "ftrl" else ou.SLOTS[hp["kind"]]


def plantable(name, dt):
    """float64's overflow cases need a reference type wider than float64."""
    return name != "max" or np.dtype(dt) == np.float32 or HAVE_EXTENDED


def edge_steps(seed, kb, ke, n, w, dt, steps=2):
    """(p0, calls, taints): bound_steps' dups_across_chunks case with the special
    gradients planted; taints[s] lists (row, column, name, where) of step s."""
    dt = np.dtype(dt)
    p0, calls = ou.bound_steps(seed, kb, ke, n, w, "dups_across_chunks", dt, steps)
    per = max(1, min(ke - kb, n // 2 + 1))
    nt = 3 * len(STEP_SPECIALS) + 1
    assert n - per >= 10 + 37 * nt + steps and n <= 2 * per, "every planted key has a loser and a winner"
    assert per + 100 + nt < ke - kb, "no room for the keys present once"
    out, taints = [], []
    for s, (keys, grads) in enumerate(calls):
        keys, grads = keys.copy(), grads.copy()
        tl = []
        for t in range(nt):
            i = 10 + 37 * t + s
            col = (t + s) % w
            if t == nt - 1:
                grads[i, col], grads[i + per, col] = np.inf, -np.inf
                tl.append((int(keys[i]) - kb, col, "both", "pair"))
                continue
            name = STEP_SPECIALS[t % len(STEP_SPECIALS)]
            where = ("winner", "loser", "once")[t // len(STEP_SPECIALS)]
            if where == "once":
                keys[i] = kb + per + 100 + t
            if not plantable(name, dt):
                continue
            pos = i + per if where == "winner" else i
            grads[pos, col] = special_value(name, dt)
            tl.append((int(keys[pos]) - kb, col, name, where))
        out.append((keys, grads))
        taints.append(tl)
    return p0, out, taints


def pooled_edge_call(seed, kb, ke, n, w, dt, weighted):
    """One pooled push on the dups_across_chunks keys, bags of eight: special bag
    gradients (each reaches eight keys, in the first half losers, in the
    second winners; one more bag holds the key present once) and, weighted, special weights: NaN, 0 against an inf bag
    gradient, inf against a 0 one.  Returns (keys, offsets, bag_grads, weights)."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    keys = key_patterns(rng, n, kb, ke)["dups_across_chunks"]
    off = pu.offsets_of(ppu.bag_lens("eights", n))
    nbags = off.size - 1
    bg = (rng.standard_normal((nbags, w)) * 3).astype(dt)
    wts = rng.standard_normal(n).astype(dt) if weighted else None
    names = [x for x in STEP_SPECIALS if plantable(x, dt)]
    for half, b0 in enumerate((3, nbags // 2 + 10)):
        for j, name in enumerate(names):
            bg[b0 + 5 * j, (j + half) % w] = special_value(name, dt)
    # the keys present once (positions n - per .. per - 1): a winner that reads a clean gsum
    per = max(1, min(ke - kb, n // 2 + 1))
    once = (n - per) // 8
    assert off[once] <= n - per < off[once + 1] and n - per < per and once not in range(3, 3 + 5 * len(names) + 1)
    bg[once, 0], bg[once, w - 1] = np.nan, np.inf
    if weighted:
        b = 60
        wts[8 * b + 1] = np.nan                      # a whole row of NaN
        bg[b + 2, 0] = np.inf
        wts[8 * (b + 2) + 3] = 0.0                    # 0 * inf
        bg[b + 4, w - 1] = 0.0
        wts[8 * (b + 4) + 5] = np.inf                 # inf * 0, and infinities beside it
    return keys, off, bg, wts


def split_pooled(keys, off, bg, wts, cuts=(40, 41)):
    """The call as pooled batches cut at bags `cuts` (one batch of a single bag)."""
    off = np.asarray(off).astype(np.int64)
    edges = [0] + list(cuts) + [off.size - 1]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        ka, kb_ = int(off[a]), int(off[b])
        batch = (keys[ka:kb_], (off[a:b + 1] - off[a]).astype(np.uint64), bg[a:b])
        out.append(batch + ((wts[ka:kb_],) if wts is not None else ()))
    return out


def _ld_and_emu(p, slots, idx, grads, dt, hp, t, pooled, rng=None):
    with np.errstate(all="ignore"):
        weighted = False
        if pooled is not None:
            weights, bag_grads, bag = pooled
            weighted = weights is not None
            rows_dt = ppu.expand(weights, bag_grads, bag, dt)
            rows_ld = ppu.ref_grads(weights, bag_grads, bag)
        else:
            rows_dt = np.asarray(grads, dtype=dt).reshape(len(idx), -1)
            rows_ld = rows_dt
        if hp["kind"] == "ftrl":
            extra = np.ones(np.asarray(p).shape[0], dtype=bool) if weighted else None
            pre = fu.prepare(p, slots, idx, rows_ld, dt, hp, m_extra=extra)
            emu = fu.emulate(p, slots, idx, rows_dt, dt, hp, rng=rng)
        else:
            ref = ou.step_ref(p, slots, idx, rows_ld, hp, t)
            if weighted:
                ref = dict(ref, m=ref["m"] + (ref["m"] > 0))
            pre = (ref,) + ou.tolerances(ref, p, slots, dt, hp, t)
            emu = ou.emulate(p, slots, idx, rows_dt, dt, hp, t, rng=rng)
    return pre, emu


def edge_step_errors(p, slots, idx, grads, p_got, slots_got, dt, hp, t=1, pooled=None):
    """The one-step check with special values as data: a list of (array name,
    message) problems.  p, slots: the shard's rows before the step; pooled:
    (weights or None, bag_grads, bag of every position) in the place of grads."""
    dt = np.dtype(dt)
    pre, (emu_p, emu_s) = _ld_and_emu(p, slots, idx, grads, dt, hp, t, pooled)
    ref, tol_p, tol_s = pre
    hit = ref["m"] > 0
    names = fu.SLOT_NAMES if hp["kind"] == "ftrl" else ou.SLOT_NAMES[hp["kind"]]
    out = []
    pairs = [("p", p, p_got, emu_p, ref["p"], tol_p)]
    for i, nm in enumerate(names):
        pairs.append((nm, slots[i], slots_got[i], emu_s[i], ref["slots"][i], tol_s[i]))
    with np.errstate(all="ignore"):
        for name, before, got, emu, want, tol in pairs:
            before, got = np.asarray(before), np.asarray(got)
            assert got.dtype == dt and before.dtype == dt and emu.dtype == dt, (name, got.dtype, before.dtype, emu.dtype)
            same = bits(before[~hit]) == bits(got[~hit])
            if not same.all():
                out.append((name, f"{name}: {int((~same).sum())} elements of untouched keys changed"))
            g, e = got[hit], emu[hit]
            err = np.abs(g.astype(F) - want[hit])
            near = np.isfinite(tol[hit]) & (err <= tol[hit])
            if name == "p" and hp["kind"] == "ftrl":
                # the threshold of ftrl_util.step_report, per element
                l1 = fu.l1_held(hp, dt)
                zr, tz = np.abs(ref["slots"][0][hit]), tol_s[0][hit]
                must_zero, must_form = zr + tz <= l1, zr - tz > l1
                band = ~(must_zero | must_form) & np.isfinite(zr) & np.isfinite(tz)
                is_zero = bits(g) == 0
                cerr = np.abs(g.astype(F) - ref["cf"][hit])
                close = np.isfinite(tol_p[hit]) & (cerr <= tol_p[hit])
                near = (must_zero & is_zero) | (must_form & close) | (band & (is_zero | close))
                err = cerr
                if band.sum() > fu.BAND_LIMIT * band.size:
                    out.append(("p", f"p: {int(band.sum())} of {band.size} elements in the threshold's band"))
            ok = (np.isnan(e) & np.isnan(g)) | (np.isinf(e) & (g == e)) | (bits(g) == bits(e)) | near
            if not ok.all():
                bad = np.argwhere(~ok)
                rows = np.flatnonzero(hit)[bad[:, 0]]
                i = tuple(bad[0])
                out.append((name, f"{name}: {len(bad)} elements wrong, (row, col) "
                                  f"{[(int(r), int(c)) for r, c in zip(rows[:3], bad[:3, 1])]}: got {g[i]!r} emulation "
                                  f"{e[i]!r} reference {float(want[hit][i])!r} err {float(err[i]):.3e} "
                                  f"tol {float(tol[hit][i]):.3e}"))
    return out


def emulate_step(p, slots, idx, grads, dt, hp, t=1, pooled=None, rng=None):
    """The dt emulation alone: (p, slots)."""
    return _ld_and_emu(p, slots, idx, grads, dt, hp, t, pooled, rng)[1]


def _class(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    return np.where(np.isnan(x), 1, np.where(np.isposinf(x), 2, np.where(np.isneginf(x), 3, 0)))


def order_problems(p, slots, idx, grads, dt, hp, tainted_rows, t=1, pooled=None, orders=3, seed=0):
    """The condition on the inputs: on the tainted rows the emulation under the
    call order and under `orders` random orders gives the same classes, and the
    same bits where finite.  Returns a list of messages (empty: the cap, zero
    order-dependent elements, is met)."""
    rows = np.asarray(sorted(set(tainted_rows)), dtype=np.int64)
    base = emulate_step(p, slots, idx, grads, dt, hp, t, pooled)
    out = []
    for o in range(orders):
        other = emulate_step(p, slots, idx, grads, dt, hp, t, pooled, rng=np.random.default_rng(seed + o))
        for name, a, b in [("p", base[0], other[0])] + [(f"slot {i}", x, y) for i, (x, y) in
                                                       enumerate(zip(base[1], other[1]))]:
            a, b = a[rows], b[rows]
            bad = (_class(a) != _class(b)) | ((_class(a) == 0) & (bits(a) != bits(b)))
            if bad.any():
                out.append(f"order {o} {name}: {int(bad.sum())} tainted elements depend on the order")
    return out


# ---------------------------------------------------------------- residue
RESIDUES = ["nan", "+inf", "both", "sub", "zero"]
PROBES = 64


def residue_case(kind, dt, w, residue, rows=5000, n=2049):
    """The no-residue scenario (module docstring) in row numbers: hp; `first` =
    (idx, grads), three occurrences of every probe row, whose two losers leave
    `residue` in gsum; `p1`, `slots1`, the refill; `follow`, two (idx, grads)
    on distinct rows; `stale`, the (PROBES, w) loser sums in dt."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(ou.case_seed("residue", kind, dt.name, w, residue))
    hp = kind_hyper(kind)
    per = n // 2 + 1
    idx = np.concatenate([np.arange(n) % per, np.arange(PROBES)])  # losers i, i + per; the winner behind them
    grads = (rng.standard_normal((idx.size, w)) * 3).astype(dt)
    a, b = np.arange(PROBES), np.arange(PROBES) + per
    sub = np.ldexp(dt.type(1), SUB_EXP[dt] + 10)
    if residue == "nan":
        grads[a] = np.nan
    elif residue == "+inf":
        grads[a] = np.inf
    elif residue == "both":
        grads[a], grads[b] = np.inf, -np.inf
    elif residue == "sub":
        grads[a], grads[b] = sub, sub
    else:
        grads[b] = -grads[a]
    with np.errstate(all="ignore"):
        stale = grads[a] + grads[b]
    shape = (rows, w)
    p1 = rng.standard_normal(shape).astype(dt)
    pos = lambda: (np.abs(rng.standard_normal(shape)) + 0.1).astype(dt)  # noqa: E731
    if kind == "adagrad":
        slots1, probe = [pos()], [1.0]
    elif kind == "ftrl":
        slots1, probe = [rng.standard_normal(shape).astype(dt), pos()], [0.0, 1.0]
    elif kind == "adam":
        slots1, probe = [(rng.standard_normal(shape) * 0.1).astype(dt), pos()], [0.0, 1.0]
    else:
        raise ValueError(kind)
    p1[:PROBES] = 0
    for s, v in zip(slots1, probe):
        s[:PROBES] = v
    follow = []
    for step in range(2):
        fi = rng.permutation(rows)[:n]
        fi[:PROBES] = rng.permutation(PROBES)  # the probes are part of both steps
        fi[PROBES:] = PROBES + rng.permutation(rows - PROBES)[:n - PROBES]
        fg = (rng.standard_normal((n, w)) * 3).astype(dt)
        if step == 0:
            fg[:PROBES] = 0
        order = rng.permutation(n)
        follow.append((fi[order], fg[order]))
    return {"hp": hp, "first": (idx, grads), "p1": p1, "slots1": slots1, "follow": follow, "stale": stale}


def residue_follow(case, dt, stale=None, t0=1):
    """The follow-up steps in the dt emulation from the refill: [(p, slots)
    after each step] (an ordinary second step rounds a stale subnormal away, so
    the twins are compared after every step).  stale: added to the probe rows' gradients of the first follow-up step (what
    a gsum that was not put back to zero does)."""
    p, slots = case["p1"], case["slots1"]
    out = []
    for step, (idx, grads) in enumerate(case["follow"]):
        if stale is not None and step == 0:
            grads = grads.copy()
            with np.errstate(all="ignore"):
                for r in range(PROBES):
                    at = np.flatnonzero(idx == r)
                    grads[at] = grads[at] + stale[r]
        p, slots = emulate_step(p, slots, idx, grads, dt, case["hp"], t=t0 + 1 + step)
        out.append((p, slots))
    return out


# ------------------------------------------------- subnormal-scale dyadic
DYADIC_GRANULE = {"sgd": -7, "momentum": -9, "nesterov": -10}


def dyadic_exp(dt, kind):
    """e with 2^e * (the smallest granule of three steps) = 4 * smallest_subnormal."""
    return SUB_EXP[np.dtype(dt)] + 2 - DYADIC_GRANULE[kind]


def scaled(x, e, dt):
    """x * 2^e in dt, which must hold it exactly."""
    dt = np.dtype(dt)
    want = np.ldexp(np.asarray(x, dtype=F), e)
    out = want.astype(dt)
    assert np.array_equal(out.astype(F), want), "a scaled value is not representable"
    return out


def dyadic_case(kind, n, w, pat, dt, li=0):
    """(hp, p0, calls, expect): the existing dyadic case of `kind` (sgd:
    test_sgd_dyadic_is_bit_exact's; momentum, nesterov: dyadic_steps2) times
    2^dyadic_exp; expect[s] = (p, slots) after step s, the unscaled reference's
    values times the same power.  None where the pattern has no such n."""
    from rows_util import LAYOUTS

    dt = np.dtype(dt)
    kb, ke = LAYOUTS[li]
    if kind == "sgd":
        hp = ou.hyper("sgd", lr=ou.DYADIC_LR)
        drawn = ou.dyadic_steps(ou.case_seed(n, w, pat, li), kb, ke, n, w, pat, dt)
    else:
        hp = ou.dyadic_hyper(kind == "nesterov")
        drawn = ou.dyadic_steps2(n, w, pat, li, dt)
    if drawn is None:
        return None
    p0, calls = drawn
    e = dyadic_exp(dt, kind)
    p, slots = p0.astype(F), [np.zeros(p0.shape, dtype=F) for _ in range(ou.SLOTS[hp["kind"]])]
    expect = []
    for keys, grads in calls:
        ref = ou.step_ref(p, slots, keys.astype(np.int64) - kb, grads, hp)
        p, slots = ref["p"], ref["slots"]
        assert np.array_equal(p.astype(dt).astype(F), p)  # the unscaled case is exact in dt
        expect.append((scaled(p, e, dt), [scaled(s, e, dt) for s in slots]))
    return hp, scaled(p0, e, dt), [(k, scaled(g, e, dt)) for k, g in calls], expect
