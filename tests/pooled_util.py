"""Helpers of the pooled-pull tests (pskv_get_pooled).

The shard is filled by an assign Add of known values, which reads back
bit-exact, so the host holds the exact parameters P.  Reference per output
element, in float64:
    ref = sum_i w_i p_i        A = sum_i |w_i| |p_i|
Floats must satisfy |got - ref| <= 1.01 (m + 1) u A, m the bag's length, u the
unit roundoff (tests/rows_util.py's accumulate bound).  It is derived, not
measured: one rounding per product plus at most m - 1 per sum gives gamma_m
for any order of the additions, contracted or not, and 1.01 (m + 1) u covers
gamma_m while m u < 0.0099 -- bags stay below 100 000 keys.  int32 is exact
with two's-complement wrap.
"""
import os
import re

import numpy as np

from rows_util import U_ROUND, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name, path):
    with open(os.path.join(ROOT, "parameter_server_amd", "csrc", path)) as f:
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)", f.read())
    return int(m.group(1))


CHUNK = _constant("kPoolChunk", "pskv_plan.h")            # keys per chunk of a long bag
BAGS_PER_WG = _constant("kPoolBagsPerWg", "pskv_plan.h")  # bags per virtual workgroup
ROWS_IN_FLIGHT = _constant("kRowsInFlight", "pskv_rows.hip")
MAX_BAG = 100_000


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint64)


def bag_patterns():
    """name -> bag lengths: the smallest shapes at which the kernel takes another path."""
    c, b = CHUNK, BAGS_PER_WG
    return {
        "all_empty": [0] * 5,
        "empties": [0, 3, 0, 0, 5, 1, 0],                 # empty first, last, consecutive
        "around_in_flight": [1, ROWS_IN_FLIGHT - 1, ROWS_IN_FLIGHT, ROWS_IN_FLIGHT + 1, 2 * ROWS_IN_FLIGHT + 1],
        "around_chunk": [c - 1, c, c + 1, 2 * c + 1],
        "one_bag": [3 * c + 7],                            # one bag holds all n keys
        "bags_below_wg": [(i % 4) for i in range(b - 1)],
        "bags_at_wg": [(i % 3) + 1 for i in range(b)],
        "bags_above_wg": [(i % 5) for i in range(b + 1)],
    }


def draw_keys(rng, lens, kb, ke):
    """Keys for these bags: random in [kb, ke), some from a few keys only, each
    bag of two or more repeats a key inside the bag, and both range ends occur."""
    n = int(np.sum(lens))
    span = ke - kb
    keys = kb + rng.integers(0, span, size=n)
    few = rng.random(n) < 0.4
    keys[few] = kb + rng.integers(0, min(span, 7), size=int(few.sum()))
    at = 0
    for i, m in enumerate(lens):
        if m >= 1:
            keys[at] = kb if i % 2 == 0 else ke - 1
        if m >= 3:
            keys[at + 1] = ke - 1 if i % 2 == 0 else kb
        if m >= 2:
            keys[at + m - 1] = keys[at + (m - 1) // 2]
        at += m
    return np.asarray(keys, dtype=np.int64).astype(np.uint32)


def draw_values(rng, shape, dt):
    dt = np.dtype(dt)
    if dt == np.int32:
        return rng.integers(-2**31, 2**31, size=shape).astype(np.int32)
    return (rng.standard_normal(shape) * 3).astype(dt)


def fill(sh, rng):
    """Assign-Add known values to every key of the shard; returns P (range, W)."""
    keys = np.arange(sh.key_begin, sh.key_end, dtype=np.int64).astype(np.uint32)
    p = draw_values(rng, (keys.size, sh.width), sh.dtype)
    sh.add(keys, p)
    got = np.asarray(sh.get(keys)).reshape(keys.size, sh.width)
    assert np.array_equal(bits(got), bits(p)), "the assign Add did not read back bit-exact"
    return p


def rows_of(p, kb, keys):
    """The rows of `keys` in P, zeros for a key outside the range."""
    idx = keys.astype(np.int64) - kb
    inside = (idx >= 0) & (idx < p.shape[0])
    rows = p[np.where(inside, idx, 0)]
    rows[~inside] = 0
    return rows


def reference(p, kb, keys, offsets, weights):
    """int32: the exact (nbags, W) result.  Floats: (ref64, bound)."""
    dt = p.dtype
    off = np.asarray(offsets).astype(np.int64)
    lens = np.diff(off)
    nbags, w = lens.size, p.shape[1]
    assert lens.max(initial=0) < MAX_BAG
    bag = np.repeat(np.arange(nbags), lens)
    rows = rows_of(p, kb, np.asarray(keys, dtype=np.uint32))
    if dt == np.int32:
        r = rows.astype(np.int64).astype(np.uint64)
        if weights is not None:
            r = r * np.asarray(weights, dtype=np.int32).astype(np.int64).astype(np.uint64)[:, None]
        acc = np.zeros((nbags, w), dtype=np.uint64)
        np.add.at(acc, bag, r)
        return (acc & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    r = rows.astype(np.float64)
    if weights is not None:
        r = r * np.asarray(weights, dtype=dt).astype(np.float64)[:, None]
    ref = np.zeros((nbags, w))
    mag = np.zeros((nbags, w))
    np.add.at(ref, bag, r)
    np.add.at(mag, bag, np.abs(r))
    return ref, 1.01 * (lens[:, None] + 1) * U_ROUND[np.dtype(dt)] * mag


def check(got, want, msg=""):
    """No element is left out: every one is compared, empty bags (bound 0) included."""
    if isinstance(want, tuple):
        ref, bound = want
        got = np.asarray(got).reshape(ref.shape)
        err = np.abs(got.astype(np.float64) - ref)
        bad = np.argwhere(~(err <= bound))
        assert bad.size == 0, (f"{msg}: {len(bad)} elements beyond the bound, first (bag, col) {bad[:3].tolist()}: "
                               f"got {got[tuple(bad[0])]!r} ref {ref[tuple(bad[0])]!r} err {err[tuple(bad[0])]:.3e} "
                               f"bound {bound[tuple(bad[0])]:.3e}")
        return
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{msg}: {len(bad)} elements differ, first (bag, col) {bad[:3].tolist()}: "
                             f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def pooled(sh, keys, offsets, weights, cuda=None, out_offset=0):
    """One pooled pull through the host path (cuda None) or the device path;
    out_offset > 0: the device output starts that many elements into a larger
    buffer (the element path).  Returns numpy (nbags, W)."""
    nbags = len(offsets) - 1
    if cuda is None:
        return np.asarray(sh.get_pooled(keys, offsets, weights)).reshape(nbags, sh.width)
    import torch

    from parameter_server_amd.shard import _torch_dtype
    from test_gpu_parity import tdev

    dk = tdev(np.asarray(keys, dtype=np.uint32), cuda)
    do = torch.from_numpy(np.asarray(offsets).astype(np.int64)).to(cuda)
    dw = None if weights is None else tdev(np.asarray(weights, dtype=sh.dtype), cuda)
    out = None
    if out_offset:
        buf = torch.empty(nbags * sh.width + out_offset, dtype=_torch_dtype(sh.dtype), device=cuda)
        out = buf[out_offset:]
    got = sh.get_pooled(dk, do, dw, out=out)
    return got.cpu().numpy().reshape(nbags, sh.width)
