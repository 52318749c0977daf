"""Seeded scenarios of FTRL-Proximal shards: the five push forms (apply,
apply_grouped, apply_pooled, apply_pooled_grouped, host and device), put_state,
clear and checkpoint / restore in random order, every step checked against the
extended-precision reference from the shard's own state before it
(tests/ftrl_util.py), everything else bit for bit."""
import numpy as np
import pytest

import ftrl_util as fu
import pooled_push_group_util as gu
import pooled_push_util as ppu
from test_ftrl_gpu import assert_same_state, make, pooled_batches, pooled_call, read_slots, state
from test_gpu_parity import tdev
from test_opt_gpu import all_keys, assert_bits, read_p

pytestmark = pytest.mark.gpu

OPS = ["apply", "apply_grouped", "apply_pooled", "apply_pooled_grouped", "put_state", "clear", "checkpoint"]


def _keys(rng, kb, rows, n):
    """n keys with duplicates: half of them from a small hot set."""
    hot = kb + rng.integers(0, max(1, rows // 16), size=n)
    cold = kb + rng.integers(0, rows, size=n)
    return np.where(rng.random(n) < 0.5, hot, cold).astype(np.int64).astype(np.uint32)


@pytest.mark.parametrize("seed", range(20))
def test_scenario(cuda, seed):
    rng = np.random.default_rng(7000 + seed)
    dt = np.dtype([np.float32, np.float64][seed % 2])
    w = [1, 3, 4, 16, 20][seed % 5]
    rows = int(rng.choice([64, 257, 1000, 4096]))
    kb = int(rng.choice([0, 1000, 2**31 - 30, 2**32 - 4096]))
    # l1 a dyadic value, so that the shard's float32 holds the l1 the user gave
    hp = fu.hyper(lr=float(rng.choice([0.02, 0.05, 0.5])), l1=float(rng.choice([0.25, 0.5, 0.75])),
                  l2=float(rng.choice([0.0, 0.01])), beta=float(rng.choice([0.0, 1.0])),
                  wd=float(rng.choice([0.0, 0.01])), init_accum=float(rng.choice([0.1, 1.0])))
    keys_all = all_keys(kb, kb + rows)
    sh = make(rows, kb, dt, w, hp)
    try:
        sh.add(keys_all, rng.standard_normal((rows, w)).astype(dt))
        t = 0
        ops = ["apply"] + [OPS[int(rng.integers(0, len(OPS)))] for _ in range(6)]
        for op in ops:
            device = bool(rng.integers(0, 2))
            dev = cuda if device else None
            n = int(rng.choice([1, 40, 2049, 5000]))
            p, slots = read_p(sh), read_slots(sh)
            if op in ("apply", "apply_grouped", "apply_pooled", "apply_pooled_grouped"):
                keys = _keys(rng, kb, rows, n)
                extra = None
                if op == "apply":
                    grads = rng.standard_normal((n, w)).astype(dt)
                    sh.apply(tdev(keys, cuda), tdev(grads, cuda)) if device else sh.apply(keys, grads)
                    ref_rows = grads
                elif op == "apply_grouped":
                    grads = rng.standard_normal((n, w)).astype(dt)
                    parts = list(zip(np.array_split(keys, 3), np.array_split(grads, 3)))
                    sh.apply_grouped([(tdev(k, cuda), tdev(g, cuda)) for k, g in parts] if device else parts)
                    ref_rows = grads
                elif op == "apply_pooled":
                    weighted = bool(rng.integers(0, 2))
                    k, off, bg, wts = pooled_call(rng, keys, w, dt, weighted, ["eights", "mixed", "ones"][seed % 3])
                    ppu.apply_pooled(sh, k, off, bg, wts, dev)
                    ref_rows = ppu.ref_grads(wts, bg, ppu.bag_index(off))
                    extra = np.zeros(rows, dtype=bool)
                    extra[keys.astype(np.int64) - kb] = weighted
                else:
                    batches = pooled_batches(rng, keys, w, dt, min(n, 4))
                    gu.apply_grouped(sh, batches, dev)
                    ref_rows = gu.ref_rows(batches, w)
                    extra = gu.weighted_keys(batches, kb, rows)
                t += 1
                assert sh.step == t
                pre = fu.prepare(p, slots, keys.astype(np.int64) - kb, ref_rows, dt, hp, m_extra=extra)
                fu.check_step(p, slots, None, None, read_p(sh), read_slots(sh), dt, hp, pre=pre,
                              msg=f"seed {seed} {op} device {device}")
            elif op == "put_state":
                slot = int(rng.integers(0, 2))
                keys = _keys(rng, kb, rows, 40)
                vals = rng.standard_normal((40, w)).astype(dt)
                if slot == 1:
                    vals = np.abs(vals)  # n is a sum of squares
                sh.put_state(tdev(keys, cuda), tdev(vals, cuda), slot=slot) if device else \
                    sh.put_state(keys, vals if w > 1 else vals.reshape(-1), slot=slot)
                want = slots[slot].copy()
                for i, k in enumerate(keys):
                    want[int(k) - kb] = vals[i]
                got = read_slots(sh)
                assert_bits(got[slot], want, f"seed {seed} put_state slot {slot}")
                assert_bits(got[1 - slot], slots[1 - slot], "the other slot")
                assert_bits(read_p(sh), p, "p after put_state")
            elif op == "clear":
                sh.clear()
                sh.sync()
                t = 0
                got = state(sh)
                assert sh.step == 0 and not got[0].any() and not got[1].any()
                assert_bits(got[2], np.full((rows, w), hp["init_accum"], dtype=dt), "n after clear")
            else:
                d = sh.state_dict()
                assert d["t"] == t
                fresh = make(rows, kb, dt, w, hp)
                fresh.load_state_dict(d)
                assert_same_state(fresh, sh, f"seed {seed} restored")
                assert fresh.step == t
                sh.sync()
                sh.close()
                sh = fresh
        sh.sync()
    finally:
        sh.close()
