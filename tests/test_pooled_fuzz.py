"""Differential fuzzing of pooled pulls (pskv_get_pooled) against the reference
of tests/pooled_util.py.  Each seeded scenario draws a dtype, a width and a key
range of at most 3,000 keys, then mixes assign Adds, optimizer steps (float
shards) and pooled pulls -- host and device path, aligned output and one
element off, weighted and not, over random bag patterns with empty, single,
short and longer-than-a-chunk bags -- and checks every pull at once.  After an
Add the host mirrors the parameters itself (last occurrence wins); after an
optimizer step it reads them back with a Get of the whole range.

Seeded: a failure prints its seed and step, and reruns identically
(FUZZ_SEED0, FUZZ_SCENARIOS).
"""
import os

import numpy as np
import pytest

import pooled_util as pu
from rows_util import WIDTHS
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

N_SCENARIOS = int(os.environ.get("FUZZ_SCENARIOS", "40"))
SEED0 = int(os.environ.get("FUZZ_SEED0", "0"))
GROUP = 10  # scenarios per test case
DTYPES = [np.int32, np.float32, np.float64]


def draw_lens(rng):
    c = pu.CHUNK
    menu = [0, 0, 1, 1, 2, pu.ROWS_IN_FLIGHT - 1, pu.ROWS_IN_FLIGHT, pu.ROWS_IN_FLIGHT + 1, 9, 40, c - 1, c, c + 1,
            2 * c + 1, 3 * c - 5]
    form = int(rng.integers(0, 4))
    if form == 0:  # many short bags, around the bags-per-workgroup constant
        nb = int(rng.choice([pu.BAGS_PER_WG - 1, pu.BAGS_PER_WG, pu.BAGS_PER_WG + 1, 3 * pu.BAGS_PER_WG + 2]))
        return [int(x) for x in rng.integers(0, 7, size=nb)]
    if form == 1:  # one bag
        return [int(rng.choice(menu))]
    return [int(x) for x in rng.choice(menu, size=int(rng.integers(1, 12)))]


def scenario(seed, cuda):
    import parameter_server_amd as ps

    rng = np.random.default_rng(seed)
    dt = np.dtype(DTYPES[int(rng.integers(0, 3))])
    w = int(rng.choice(WIDTHS))
    span = int(rng.integers(1, 3001))
    kb = int(rng.choice([0, 12345, 2**31 - span // 2, 2**32 - span]))
    ke = kb + span
    stepping = dt != np.int32 and bool(rng.integers(0, 2))
    tag = f"seed {seed} {dt.name} W={w} [{kb}, {ke}) optimizer={stepping}"
    allk = np.arange(kb, ke, dtype=np.int64).astype(np.uint32)
    with ps.Shard(kb, ke, dt, mode="assign", width=w) as sh:
        p = pu.fill(sh, rng)
        if stepping:
            sh.set_optimizer(str(rng.choice(["sgd", "adagrad", "momentum", "adam"])), lr=0.05, momentum=0.5)
        for step in range(int(rng.integers(5, 13))):
            op = int(rng.integers(0, 6))
            device = bool(rng.integers(0, 2))
            where = f"{tag} step {step} op {op} device={device}"
            if op == 0:  # assign Add: the last occurrence of a key wins
                k = kb + rng.integers(0, span, size=int(rng.choice([1, 5, 300, 2049])))
                k = np.asarray(k, dtype=np.int64).astype(np.uint32)
                v = pu.draw_values(rng, (k.size, w), dt)
                if device:
                    sh.add(tdev(k, cuda), tdev(v, cuda))
                else:
                    sh.add(k, v)
                last = k.size - 1 - np.unique(k[::-1], return_index=True)[1]
                p[k[last].astype(np.int64) - kb] = v[last]
            elif op == 1 and stepping:  # optimizer step: read the parameters back
                k = kb + rng.integers(0, span, size=int(rng.choice([1, 64, 700])))
                k = np.asarray(k, dtype=np.int64).astype(np.uint32)
                g = pu.draw_values(rng, (k.size, w), dt)
                if device:
                    sh.apply(tdev(k, cuda), tdev(g, cuda))
                else:
                    sh.apply(k, g)
                p = np.asarray(sh.get(allk)).reshape(span, w).copy()
            else:  # pooled pull
                lens = draw_lens(rng)
                off, keys = pu.offsets_of(lens), pu.draw_keys(rng, lens, kb, ke)
                wts = pu.draw_values(rng, keys.size, dt) if rng.integers(0, 2) else None
                want = pu.reference(p, kb, keys, off, wts)
                got = pu.pooled(sh, keys, off, wts, cuda if device else None,
                                out_offset=int(rng.integers(0, 2)) if device else 0)
                pu.check(got, want, where)
        sh.sync()


@pytest.mark.parametrize("first", range(SEED0, SEED0 + N_SCENARIOS, GROUP))
def test_pooled_fuzz(cuda, first):
    for seed in range(first, min(first + GROUP, SEED0 + N_SCENARIOS)):
        try:
            scenario(seed, cuda)
        except BaseException:
            print(f"pooled fuzz: failing seed {seed} (rerun with FUZZ_SEED0={seed} FUZZ_SCENARIOS=1)")
            raise
