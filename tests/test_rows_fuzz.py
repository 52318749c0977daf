"""Differential fuzzing of row-valued shards against the per-column oracle
(tests/rows_util.py).  Each seeded scenario draws a dtype, a mode, a width and a
key range of at most 3,000 keys, then runs a random sequence of 5-15 calls over
every entry point, host and device (aligned and one element off), with heavy
key duplication; every Get is checked at once and the whole range at the end.
Out-of-range keys are left out (tests/test_rows_gpu.py covers them).

Seeded: a failure names its scenario and step, and reruns identically.
"""
import os

import numpy as np
import pytest

from rows_util import WIDTHS, RowOracle, ValueSource
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

N_SCENARIOS = int(os.environ.get("FUZZ_SCENARIOS", "40"))
SEED0 = int(os.environ.get("FUZZ_SEED0", "0"))
GROUP = 10  # scenarios per test case
SIZES = [0, 1, 5, 63, 64, 65, 300, 2047, 2048, 2049, 3000]
DTYPES = [np.int32, np.float32, np.float64]


def draw_keys(rng, kb, ke):
    n = int(rng.choice(SIZES))
    span = ke - kb
    form = int(rng.integers(0, 4))
    if form == 0:  # uniform
        k = rng.integers(kb, ke, size=n)
    elif form == 1:  # a handful of hot keys
        k = kb + rng.integers(0, min(span, 7), size=n)
    elif form == 2:  # Zipf-like
        k = kb + np.minimum(rng.zipf(1.3, size=n) - 1, span - 1)
    else:  # sorted with repeats
        k = np.sort(rng.integers(kb, kb + max(1, span // 4), size=n))
    return np.asarray(k, dtype=np.int64).astype(np.uint32)


def empty_out(n, w, dt, cuda=None, offset=0):
    shape = (n, w) if w > 1 else (n,)
    if cuda is None:
        return np.empty(shape, dtype=dt)
    import torch

    from parameter_server_amd.shard import _torch_dtype

    buf = torch.empty(n * w + offset, dtype=_torch_dtype(dt), device=cuda)
    return buf[offset:].view(*shape)


def scenario(seed, cuda, oracle_mod):
    import parameter_server_amd as ps

    rng = np.random.default_rng(seed)
    dt = DTYPES[int(rng.integers(0, 3))]
    mode = ("assign", "accumulate")[int(rng.integers(0, 2))]
    w = int(rng.choice(WIDTHS))
    span = int(rng.integers(1, 3001))
    kb = int(rng.choice([0, 12345, 2**31 - span // 2, 2**32 - span]))
    ke = kb + span
    orc = RowOracle(oracle_mod, dt, mode, w, kb, ke)
    src = ValueSource(dt, mode, rng)
    tag = f"seed {seed} {np.dtype(dt).name} {mode} W={w} [{kb}, {ke})"

    def dev(k, v=None, off=0):
        dk = tdev(k, cuda, off)
        if v is None:
            return dk
        dv = tdev(v.reshape(-1), cuda, off)
        return dk, (dv.view(k.size, w) if w > 1 else dv)

    with ps.Shard(kb, ke, dt, mode=mode, width=w) as sh:
        for step in range(int(rng.integers(5, 16))):
            op = int(rng.integers(0, 9))
            where = f"{tag} step {step} op {op}"
            device = bool(rng.integers(0, 2))
            off = int(rng.integers(0, 2)) if device else 0
            if op in (0, 1):  # add
                k = draw_keys(rng, kb, ke)
                v = src.rows(k.size, w)
                if device:
                    sh.add(*dev(k, v, off), sorted_hint=bool(rng.integers(0, 2)))
                else:
                    sh.add(k, v if rng.random() < 0.5 else v.reshape(-1))
                orc.add(k, v)
            elif op in (2, 3):  # get
                k = draw_keys(rng, kb, ke)
                if device:
                    got = sh.get(dev(k, None, off), out=empty_out(k.size, w, dt, cuda, off)).cpu().numpy()
                else:
                    got = sh.get(k)
                orc.check(k, got, where)
            elif op in (4, 5):  # grouped add
                ks = [draw_keys(rng, kb, ke) for _ in range(int(rng.integers(1, 6)))]
                vs = [src.rows(k.size, w) for k in ks]
                sh.add_grouped([dev(k, v, off) for k, v in zip(ks, vs)] if device else list(zip(ks, vs)))
                for k, v in zip(ks, vs):
                    orc.add(k, v)
            elif op == 6:  # grouped get
                ks = [draw_keys(rng, kb, ke) for _ in range(int(rng.integers(1, 6)))]
                outs = [empty_out(k.size, w, dt, cuda if device else None, off) for k in ks]
                sh.get_grouped([(dev(k, None, off) if device else k, o) for k, o in zip(ks, outs)])
                for k, o in zip(ks, outs):
                    orc.check(k, o.cpu().numpy() if device else o, where)
            elif op == 7:  # add then get in one call
                ks = [draw_keys(rng, kb, ke) for _ in range(int(rng.integers(1, 4)))]
                vs = [src.rows(k.size, w) for k in ks]
                qs = [draw_keys(rng, kb, ke) for _ in range(int(rng.integers(1, 4)))]
                outs = [empty_out(k.size, w, dt, cuda if device else None, off) for k in qs]
                sh.add_get_grouped([dev(k, v, off) for k, v in zip(ks, vs)] if device else list(zip(ks, vs)),
                                   [(dev(k, None, off) if device else k, o) for k, o in zip(qs, outs)])
                for k, v in zip(ks, vs):
                    orc.add(k, v)
                for k, o in zip(qs, outs):
                    orc.check(k, o.cpu().numpy() if device else o, where)
            elif rng.random() < 0.3:  # clear
                sh.clear()
                orc.clear()
            else:
                sh.sync()
        q = orc.all_keys()
        orc.check(q, sh.get(q), f"{tag} final host get")
        orc.check(q, sh.dense_view().cpu().numpy(), f"{tag} final dense view")
        sh.sync()


@pytest.mark.parametrize("first", range(SEED0, SEED0 + N_SCENARIOS, GROUP))
def test_row_fuzz(cuda, oracle_mod, first):
    for seed in range(first, min(first + GROUP, SEED0 + N_SCENARIOS)):
        scenario(seed, cuda, oracle_mod)
