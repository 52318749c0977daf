"""Differential fuzzing of grouped pooled pushes (pskv_apply_pooled_grouped)
against the reference of tests/pooled_push_group_util.py.  Each seeded scenario
draws a float dtype, a width, a key range of at most 3,000 keys and an
optimizer kind, then mixes assign Adds, Gets, plain optimizer steps, pooled
pushes and grouped pooled pushes of 1 to 6 batches -- host and device path,
aligned bag rows and one batch one element off, weighted and unweighted and
empty batches in one call, over random bag patterns -- and checks every step
at once: a step of any of the three kinds by the one-step check from the
shard's own state read just before it, a Get against that state.

Seeded: a failure prints its seed and step, and reruns identically
(FUZZ_SEED0, FUZZ_SCENARIOS).
"""
import os

import numpy as np
import pytest

import opt_util as ou
import pooled_push_group_util as gu
import pooled_push_util as ppu
import pooled_util as pu
from rows_util import WIDTHS, bits
from test_gpu_parity import tdev
from test_opt_gpu import read_p
from test_opt2_gpu import read_slots
from test_pooled_push_fuzz import draw_lens

pytestmark = pytest.mark.gpu

N_SCENARIOS = int(os.environ.get("FUZZ_SCENARIOS", "30"))
SEED0 = int(os.environ.get("FUZZ_SEED0", "0"))
GROUP = 10  # scenarios per test case


def draw_batch(rng, kb, span, w, dt):
    """One worker's push, or (one time in six) a batch that contributes nothing."""
    form = int(rng.integers(0, 6))
    if form == 0:
        return gu.empty_batch(w, dt, nbags=int(rng.integers(0, 3)), keys=0)
    n = int(rng.choice([1, 7, 300, 2049, 4100]))
    k = np.asarray(kb + rng.integers(0, span, size=n), dtype=np.int64).astype(np.uint32)
    off = pu.offsets_of(draw_lens(rng, n))
    bg = pu.draw_values(rng, (off.size - 1, w), dt)
    wts = pu.draw_values(rng, n, dt) if rng.integers(0, 2) else None
    return k, off, bg, wts


def scenario(seed, cuda):
    import parameter_server_amd as ps

    rng = np.random.default_rng(1_000_000 + seed)
    dt = np.dtype([np.float32, np.float64][int(rng.integers(0, 2))])
    w = int(rng.choice(WIDTHS))
    span = int(rng.integers(1, 3001))
    kb = int(rng.choice([0, 12345, 2**31 - span // 2, 2**32 - span]))
    ke = kb + span
    kind, nesterov = ppu.KINDS[int(rng.integers(0, len(ppu.KINDS)))]
    hp = ppu.hyper(kind, nesterov, wd=float(rng.choice([0.0, 0.01])))
    tag = f"seed {seed} {dt.name} W={w} [{kb}, {ke}) {kind} nesterov={nesterov} wd={hp['wd']}"
    allk = np.arange(kb, ke, dtype=np.int64).astype(np.uint32)
    with ps.Shard(kb, ke, dt, mode="assign", width=w) as sh:
        ppu.set_optimizer(sh, hp)
        sh.add(allk, pu.draw_values(rng, (span, w), dt))
        t = 0
        for step in range(int(rng.integers(5, 11))):
            op = int(rng.integers(0, 8))
            device = bool(rng.integers(0, 2))
            where = f"{tag} step {step} op {op} device={device}"
            n = int(rng.choice([1, 5, 300, 2049, 4100]))
            k = np.asarray(kb + rng.integers(0, span, size=n), dtype=np.int64).astype(np.uint32)
            if op == 0:  # assign Add
                v = pu.draw_values(rng, (n, w), dt)
                if device:
                    sh.add(tdev(k, cuda), tdev(v, cuda))
                else:
                    sh.add(k, v)
            elif op == 1:  # Get
                p = read_p(sh)
                got = np.asarray(sh.get(k)).reshape(n, w)
                assert np.array_equal(bits(got), bits(p[k.astype(np.int64) - kb])), where
            elif op == 2:  # plain optimizer step
                g = pu.draw_values(rng, (n, w), dt)
                p, slots = read_p(sh), read_slots(sh, kind)
                if device:
                    sh.apply(tdev(k, cuda), tdev(g, cuda))
                else:
                    sh.apply(k, g)
                t += 1
                ou.check_step(p, slots, k.astype(np.int64) - kb, g, read_p(sh), read_slots(sh, kind), dt, hp, t,
                              msg=where)
            elif op == 3:  # pooled push
                off = pu.offsets_of(draw_lens(rng, n))
                bg = pu.draw_values(rng, (off.size - 1, w), dt)
                wts = pu.draw_values(rng, n, dt) if rng.integers(0, 2) else None
                p, slots = read_p(sh), read_slots(sh, kind)
                ppu.apply_pooled(sh, k, off, bg, wts, cuda if device else None)
                t += 1
                ppu.check_step(p, slots, k.astype(np.int64) - kb, wts, bg, ppu.bag_index(off), read_p(sh),
                               read_slots(sh, kind), dt, hp, t, msg=where)
            else:  # grouped pooled push
                batches = [draw_batch(rng, kb, span, w, dt) for _ in range(int(rng.integers(1, 7)))]
                shifts = [0] * len(batches)
                if device and rng.integers(0, 2):
                    shifts[int(rng.integers(0, len(batches)))] = 1
                p, slots = read_p(sh), read_slots(sh, kind)
                gu.apply_grouped(sh, batches, cuda if device else None, bg_offsets=shifts)
                where += f" sizes={[b[0].size for b in batches]} weighted={[b[3] is not None for b in batches]}"
                if not gu.live(batches):  # empty batches only: no step, no change
                    for got, was in zip([read_p(sh)] + read_slots(sh, kind), [p] + slots):
                        assert np.array_equal(bits(got), bits(was)), where
                else:
                    t += 1
                    gu.check_step(p, slots, kb, batches, read_p(sh), read_slots(sh, kind), dt, hp, t, msg=where)
            assert sh.step == t, where
        sh.sync()


@pytest.mark.parametrize("first", range(SEED0, SEED0 + N_SCENARIOS, GROUP))
def test_pooled_push_grouped_fuzz(cuda, first):
    for seed in range(first, min(first + GROUP, SEED0 + N_SCENARIOS)):
        try:
            scenario(seed, cuda)
        except BaseException:
            print(f"grouped pooled push fuzz: failing seed {seed} (rerun with FUZZ_SEED0={seed} FUZZ_SCENARIOS=1)")
            raise
