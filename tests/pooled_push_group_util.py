"""The reference and the checker of grouped pooled pushes
(pskv_apply_pooled_grouped, Shard.apply_pooled_grouped), built on
tests/pooled_push_util.py and tests/opt_util.py.

One call is the ONE step pskv_apply_pooled would make of the concatenation of
its batches (include/pskv.h "Grouped pooled pushes").  A batch here is
pooled_push_util.draw_call's tuple (keys, offsets, bag_grads (nbags, w),
weights or None), which is also the order Shard.apply_pooled_grouped takes.
The reference is opt_util.step_ref on the concatenated call: the rows
pooled_push_util.ref_grads forms per batch, stacked in batch order.

Tolerances: opt_util.tolerances with m counted over the WHOLE call, and m + 1
in the place of m for a key that has any weighted occurrence (DESIGN.md §8g's
derived bound: a weighted term carries one more rounding; the tolerances grow
with m, so m + 1 for the whole key covers a key whose occurrences are partly
weighted).  tests/test_pooled_push_grouped_cpu.py checks this against an
emulation of the kernels' order and proves the checker rejects the two wrong
semantics a grouped call can newly have.
"""
import numpy as np

import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu

F = ou.F
MAX_POOL_BATCHES = pu._constant("kMaxPoolBatches", "pskv_plan.h")  # batches per launch group
KEY_PATTERNS = ["distinct", "dups_in_chunk", "dups_across_chunks", "range_ends"]


def live(batches):
    """The batches that contribute: at least one key and one bag."""
    return [b for b in batches if np.asarray(b[0]).size and np.asarray(b[1]).size > 1]


def indices(batches, kb):
    """Row of every key position of the call, in batch order."""
    parts = [np.asarray(b[0]).astype(np.int64) - kb for b in live(batches)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def ref_rows(batches, w):
    """The reference's rows of the concatenated call, in np.longdouble."""
    parts = [ppu.ref_grads(b[3], b[2], ppu.bag_index(b[1])) for b in live(batches)]
    return np.vstack(parts) if parts else np.zeros((0, w), dtype=F)


def expanded_rows(batches, dt):
    """Per live batch the host-expanded rows fl_T(w_i * bg) (pskv_apply_grouped's twin)."""
    return [ppu.expand(b[3], b[2], ppu.bag_index(b[1]), dt) for b in live(batches)]


def concatenated(batches, dt):
    """(keys, offsets, bag_grads, weights) of the one pskv_apply_pooled call the
    grouped call stands for: offsets shifted by the keys before the batch; a
    batch without weights beside weighted ones gets weights of one (exact)."""
    bs = live(batches)
    keys = np.concatenate([np.asarray(b[0], dtype=np.uint32) for b in bs])
    off, at = [np.zeros(1, dtype=np.uint64)], 0
    for b in bs:
        off.append(np.asarray(b[1], dtype=np.uint64)[1:] + np.uint64(at))
        at += np.asarray(b[0]).size
    bg = np.vstack([np.asarray(b[2], dtype=dt) for b in bs])
    wts = None
    if any(b[3] is not None for b in bs):
        wts = np.concatenate([np.ones(np.asarray(b[0]).size, dtype=dt) if b[3] is None else np.asarray(b[3], dtype=dt)
                              for b in bs])
    return keys, np.concatenate(off), bg, wts


def weighted_keys(batches, kb, rows):
    """(rows,) bool: the key has a weighted occurrence somewhere in the call."""
    out = np.zeros(rows, dtype=bool)
    for b in live(batches):
        if b[3] is not None:
            out[np.asarray(b[0]).astype(np.int64) - kb] = True
    return out


def prepare(p, slots, kb, batches, dt, hp, t=1):
    """opt_util.prepare of the concatenated step, with the tolerances above."""
    ref = ou.step_ref(p, slots, indices(batches, kb), ref_rows(batches, p.shape[1]), hp, t)
    ref = dict(ref, m=ref["m"] + ((ref["m"] > 0) & weighted_keys(batches, kb, p.shape[0])))
    return (ref,) + ou.tolerances(ref, p, slots, dt, hp, t)


def step_errors(p, slots, kb, batches, p_got, slots_got, dt, hp, t=1, pre=None):
    pre = pre or prepare(p, slots, kb, batches, dt, hp, t)
    return ou.step_errors(p, slots, None, None, p_got, slots_got, dt, hp, t, pre=pre)


def check_step(*a, msg="", **kw):
    problems = step_errors(*a, **kw)
    assert not problems, f"{msg}: " + "; ".join(text for _, text in problems)


def draw_group(rng, sizes, w, kb, ke, dt, c=0, dyadic=False, weighted=None):
    """One call of len(sizes) batches.  The key pattern, the bag pattern and
    weighted-or-not rotate with c + the batch's place (weighted: a list forces
    it), so a call of several batches mixes them; every batch after the first
    repeats a key of the batch before it, so the call has the same key in two
    batches."""
    batches = []
    for j, n in enumerate(sizes):
        pat = KEY_PATTERNS[(c + j) % len(KEY_PATTERNS)]
        if pat == "distinct" and n > ke - kb:
            pat = "range_ends"
        bagpat = ppu.BAG_PATTERNS[(c + 2 * j) % len(ppu.BAG_PATTERNS)]
        wtd = bool((c + j) % 3) if weighted is None else weighted[j]
        keys, off, bg, wts = ppu.draw_call(rng, n, w, pat, bagpat, kb, ke, dt, wtd, dyadic=dyadic)
        if batches:
            keys[0] = batches[-1][0][-1]
        batches.append((keys, off, bg, wts))
    return batches


def draw_distinct_group(rng, sizes, w, kb, ke, dt, c=0, weighted=None, dyadic=False):
    """As draw_group, with every key of the whole call distinct: a permutation
    of the range dealt out over the batches."""
    assert sum(sizes) <= ke - kb
    deck = (kb + rng.permutation(ke - kb)).astype(np.int64).astype(np.uint32)
    batches, at = [], 0
    for j, n in enumerate(sizes):
        bagpat = ppu.BAG_PATTERNS[(c + 2 * j) % len(ppu.BAG_PATTERNS)]
        wtd = bool((c + j) % 3) if weighted is None else weighted[j]
        _, off, bg, wts = ppu.draw_call(rng, n, w, "dups_in_chunk", bagpat, kb, ke, dt, wtd, dyadic=dyadic)
        batches.append((deck[at:at + n].copy(), off, bg, wts))
        at += n
    return batches


def empty_batch(w, dt, nbags=0, keys=0):
    """A batch that contributes nothing: no key (with nbags empty bags), or
    `keys` keys and no bag."""
    off = np.zeros(nbags + 1, dtype=np.uint64)
    wts = np.ones(keys, dtype=dt) if keys else None
    return np.arange(keys, dtype=np.uint32), off, np.ones((nbags, w), dtype=dt), wts


def device_batch(sh, b, cuda, bg_offset=0):
    """The batch as torch tensors on `cuda`; bg_offset > 0: the bag rows start
    that many elements into a larger buffer (off 16-byte alignment)."""
    import torch

    from test_gpu_parity import tdev

    keys, off, bg, wts = b
    dk = tdev(np.asarray(keys, dtype=np.uint32), cuda)
    do = torch.from_numpy(np.asarray(off).astype(np.int64)).to(cuda)
    dg = tdev(np.ascontiguousarray(bg, dtype=sh.dtype).reshape(-1), cuda, bg_offset)
    dw = None if wts is None else tdev(np.asarray(wts, dtype=sh.dtype), cuda)
    return dk, do, dg, dw


def apply_grouped(sh, batches, cuda=None, bg_offsets=None):
    """One grouped pooled push through the host path (cuda None) or the device path."""
    if cuda is None:
        sh.apply_pooled_grouped(batches)
        return
    offs = bg_offsets or [0] * len(batches)
    dev = [device_batch(sh, b, cuda, o) for b, o in zip(batches, offs)]
    sh.apply_pooled_grouped(dev)
