"""Differential fuzzing of pooled pushes (pskv_apply_pooled) against the
reference of tests/pooled_push_util.py.  Each seeded scenario draws a float
dtype, a width, a key range of at most 3,000 keys and an optimizer kind, then
mixes assign Adds, plain optimizer steps, pooled pulls and pooled pushes --
host and device path, aligned bag rows and one element off, weighted and not,
over random bag patterns with empty, single, short and long bags -- and checks
every step at once: a push or an apply by the one-step check from the shard's
own state read just before it, a pull against pooled_util's reference.

Seeded: a failure prints its seed and step, and reruns identically
(FUZZ_SEED0, FUZZ_SCENARIOS).
"""
import os

import numpy as np
import pytest

import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
from rows_util import WIDTHS
from test_gpu_parity import tdev
from test_opt_gpu import read_p
from test_opt2_gpu import read_slots

pytestmark = pytest.mark.gpu

N_SCENARIOS = int(os.environ.get("FUZZ_SCENARIOS", "40"))
SEED0 = int(os.environ.get("FUZZ_SEED0", "0"))
GROUP = 10  # scenarios per test case


def draw_lens(rng, n):
    """Bag lengths that sum to n."""
    form = int(rng.integers(0, 5))
    if form < len(ppu.BAG_PATTERNS) - 1:
        return ppu.bag_lens(ppu.BAG_PATTERNS[form], n)
    lens, left = [], n
    menu = [0, 0, 1, 1, 2, 3, 9, 40, pu.CHUNK, pu.CHUNK + 1, 700]
    while left:
        m = min(int(rng.choice(menu)), left)
        lens.append(m)
        left -= m
    return lens + [0] * int(rng.integers(0, 3))


def scenario(seed, cuda):
    import parameter_server_amd as ps

    rng = np.random.default_rng(seed)
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
        for step in range(int(rng.integers(5, 13))):
            op = int(rng.integers(0, 6))
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
            elif op == 1:  # plain optimizer step
                g = pu.draw_values(rng, (n, w), dt)
                p, slots = read_p(sh), read_slots(sh, kind)
                if device:
                    sh.apply(tdev(k, cuda), tdev(g, cuda))
                else:
                    sh.apply(k, g)
                t += 1
                ou.check_step(p, slots, k.astype(np.int64) - kb, g, read_p(sh), read_slots(sh, kind), dt, hp, t,
                              msg=where)
            elif op == 2:  # pooled pull
                off = pu.offsets_of(draw_lens(rng, n))
                wts = pu.draw_values(rng, n, dt) if rng.integers(0, 2) else None
                want = pu.reference(read_p(sh), kb, k, off, wts)
                pu.check(pu.pooled(sh, k, off, wts, cuda if device else None), want, where)
            else:  # pooled push
                off = pu.offsets_of(draw_lens(rng, n))
                bg = pu.draw_values(rng, (off.size - 1, w), dt)
                wts = pu.draw_values(rng, n, dt) if rng.integers(0, 2) else None
                p, slots = read_p(sh), read_slots(sh, kind)
                ppu.apply_pooled(sh, k, off, bg, wts, cuda if device else None,
                                 bg_offset=int(rng.integers(0, 2)) if device else 0)
                t += 1
                ppu.check_step(p, slots, k.astype(np.int64) - kb, wts, bg, ppu.bag_index(off), read_p(sh),
                               read_slots(sh, kind), dt, hp, t, msg=where)
            assert sh.step == t, where
        sh.sync()


@pytest.mark.parametrize("first", range(SEED0, SEED0 + N_SCENARIOS, GROUP))
def test_pooled_push_fuzz(cuda, first):
    for seed in range(first, min(first + GROUP, SEED0 + N_SCENARIOS)):
        try:
            scenario(seed, cuda)
        except BaseException:
            print(f"pooled push fuzz: failing seed {seed} (rerun with FUZZ_SEED0={seed} FUZZ_SCENARIOS=1)")
            raise
