"""Differential fuzzing of sparse shards against the relabelled oracles
(tests/sparse_util.py).  Each seeded scenario draws a capacity of 8 to 4096, a
pool of distinct uint32 keys that fits it (0, 2^31 and 0xFFFFFFFF among them),
a dtype and a width, and runs a random sequence of calls, host and device, with
heavy key duplication.  Two kinds of scenario:

  storage    a mode and no optimizer: add, get, the grouped forms, add then get,
             pooled pulls, clear -- every reply checked at once against
             RowOracle (assign: the raw keys, bit-exact; accumulate: the ranks,
             within its bound; int32 exact), absent keys reading zeros, and the
             stored key set against the keys written;
  optimizer  one of the six kinds: apply, apply_grouped, apply_pooled,
             apply_pooled_grouped, each step checked by the one-step check of
             opt_util / ftrl_util / pooled_push_util from the shard's own state
             before it (a key the shard does not hold yet standing at zeros and
             the start state); put_state / get_state round trips, bit-exact.

Seeded: a failure names its scenario and step, and reruns identically.  No
scenario is skipped: one that cannot be built fails.
"""
import os

import numpy as np
import pytest

import ftrl_util as fu
import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
import sparse_util as su
from rows_util import RowOracle, ValueSource, bits
from test_gpu_parity import tdev
from test_sparse_gpu import KINDS, hyper_of, n_slots, rows, set_opt, start_slots

pytestmark = pytest.mark.gpu

N_SCENARIOS = int(os.environ.get("FUZZ_SCENARIOS", "40"))
SEED0 = int(os.environ.get("FUZZ_SEED0", "0"))
GROUP = 10  # scenarios per test case
SIZES = [0, 1, 5, 63, 255, 300, 2047, 2048, 2049, 3000]
WIDTHS = [1, 3, 4, 16, 33]
CAPACITIES = [8, 9, 16, 100, 1000, 2048, 4096]


def draw_positions(rng, m, n=None):
    """n positions of a pool of m keys: uniform, a handful of hot keys, Zipf-like, or sorted with repeats."""
    n = int(rng.choice(SIZES)) if n is None else n
    form = int(rng.integers(0, 4))
    if form == 0:
        k = rng.integers(0, m, size=n)
    elif form == 1:
        k = rng.integers(0, min(m, 7), size=n)
    elif form == 2:
        k = np.minimum(rng.zipf(1.3, size=n) - 1, m - 1)
    else:
        k = np.sort(rng.integers(0, max(1, m // 4), size=n))
    return np.asarray(k, dtype=np.int64)


def draw_pool(rng):
    cap = int(rng.choice(CAPACITIES))
    m = int(rng.integers(1, min(cap, 3000) + 1))
    return cap, su.key_pool(rng, m)


def empty_out(n, w, dt, cuda=None):
    shape = (n, w) if w > 1 else (n,)
    if cuda is None:
        return np.empty(shape, dtype=dt)
    import torch

    from parameter_server_amd.shard import _torch_dtype

    return torch.empty(shape, dtype=_torch_dtype(dt), device=cuda)


def storage_scenario(seed, cuda, oracle_mod):
    import parameter_server_amd as ps

    rng = np.random.default_rng(seed)
    dt = [np.int32, np.float32, np.float64][int(rng.integers(0, 3))]
    mode = ("assign", "accumulate")[int(rng.integers(0, 2))]
    w = int(rng.choice(WIDTHS))
    cap, pool = draw_pool(rng)
    m = pool.size
    rl = su.Relabel(pool)
    gone = su.absent_keys(rng, pool, 64)
    # assign: the raw keys (MapStorageRef takes any key); accumulate: the ranks
    orc = RowOracle(oracle_mod, dt, mode, w, 0, (1 << 32) if mode == "assign" else m)
    src = ValueSource(dt, mode, rng)
    tag = f"storage seed {seed} {np.dtype(dt).name} {mode} W={w} capacity {cap} keys {m}"
    stored = set()

    def wkeys():
        return pool[draw_positions(rng, m)]

    def rkeys():  # stored, never written and absent keys mixed
        k = pool[draw_positions(rng, m)]
        hole = rng.random(k.size) < 0.2
        k[hole] = gone[rng.integers(0, gone.size, size=int(hole.sum()))]
        return k

    def note(k, v):
        orc.add(k if mode == "assign" else rl.rank(k), v)
        stored.update(int(x) for x in k)

    def check(k, got, where):
        got = np.asarray(got).reshape(k.size, w)
        inside = rl.holds(k)
        assert not got[~inside].any(), f"{where}: an absent key reads non-zero"
        orc.check(k[inside] if mode == "assign" else rl.rank(k[inside]), got[inside], where)

    def dev(k, v=None):
        return tdev(k, cuda) if v is None else (tdev(k, cuda), tdev(v, cuda))

    with ps.Shard.sparse(cap, dt, mode, width=w) as sh:
        for step in range(int(rng.integers(5, 16))):
            op = int(rng.integers(0, 10))
            where = f"{tag} step {step} op {op}"
            device = bool(rng.integers(0, 2))
            if op in (0, 1):
                k = wkeys()
                v = src.rows(k.size, w)
                if device:
                    sh.add(*dev(k, v), sorted_hint=bool(rng.integers(0, 2)))
                else:
                    sh.add(k, v)
                note(k, v)
            elif op in (2, 3):
                k = rkeys()
                check(k, sh.get(dev(k)).cpu().numpy() if device else sh.get(k), where)
            elif op in (4, 5):
                ks = [wkeys() for _ in range(int(rng.integers(1, 6)))]
                vs = [src.rows(k.size, w) for k in ks]
                sh.add_grouped([dev(k, v) for k, v in zip(ks, vs)] if device else list(zip(ks, vs)))
                for k, v in zip(ks, vs):
                    note(k, v)
            elif op == 6:
                ks = [rkeys() for _ in range(int(rng.integers(1, 6)))]
                outs = [empty_out(k.size, w, dt, cuda if device else None) for k in ks]
                sh.get_grouped([(dev(k) if device else k, o) for k, o in zip(ks, outs)])
                for k, o in zip(ks, outs):
                    check(k, o.cpu().numpy() if device else o, where)
            elif op == 7:
                ks = [wkeys() for _ in range(int(rng.integers(1, 4)))]
                vs = [src.rows(k.size, w) for k in ks]
                qs = [rkeys() for _ in range(int(rng.integers(1, 4)))]
                outs = [empty_out(k.size, w, dt, cuda if device else None) for k in qs]
                sh.add_get_grouped([dev(k, v) for k, v in zip(ks, vs)] if device else list(zip(ks, vs)),
                                   [(dev(k) if device else k, o) for k, o in zip(qs, outs)])
                for k, v in zip(ks, vs):
                    note(k, v)
                for k, o in zip(qs, outs):
                    check(k, o.cpu().numpy() if device else o, where)
            elif op == 8:  # a pooled pull, from the rows a Get returns (Gets are checked above)
                lens = [int(x) for x in rng.choice([0, 1, 2, 5, 40, 300], size=int(rng.integers(1, 8)))]
                k = rkeys()[: sum(lens)]
                k = np.concatenate([k, pool[draw_positions(rng, m, sum(lens) - k.size)]])
                wts = pu.draw_values(rng, k.size, dt) if rng.random() < 0.5 else None
                p = rows(sh, rl.uniq)
                idx = np.where(rl.holds(k), np.searchsorted(rl.uniq, k), m).astype(np.uint32)  # absent: past p, zeros
                pu.check(pu.pooled(sh, k, pu.offsets_of(lens), wts, cuda if device else None),
                         pu.reference(p, 0, idx, pu.offsets_of(lens), wts), where)
            elif rng.random() < 0.3:
                sh.clear()
                orc.clear()
                stored.clear()
            else:
                sh.sync()
            if step % 4 == 3:
                assert sh.sparse_info()["count"] == len(stored), where
        check(pool, sh.get(pool), f"{tag} final get")
        assert sorted(int(k) for k in sh.keys()) == sorted(stored), f"{tag} final keys"
        sh.sync()  # never full: the scenario's keys fit the capacity


def ftrl_check(before, idx, grads, p_got, s_got, dt, hp, where):
    """ftrl_util's one-step check without its limit on the share of elements in
    the threshold's band: a scenario may hold a single element."""
    problems = fu.step_errors(before[0], before[1], idx, grads, p_got, s_got, dt, hp)
    assert not problems, f"{where}: " + "; ".join(text for _, text in problems)


def optimizer_scenario(seed, cuda):
    import parameter_server_amd as ps

    rng = np.random.default_rng(seed)
    dt = [np.float32, np.float64][int(rng.integers(0, 2))]
    kind, nesterov = KINDS[int(rng.integers(0, len(KINDS)))]
    w = int(rng.choice(WIDTHS))
    cap, pool = draw_pool(rng)
    m = pool.size
    rl = su.Relabel(pool)
    hp = hyper_of(kind, nesterov, wd=float(rng.choice([0.0, 0.01])))
    ns = n_slots(hp)
    tag = f"optimizer seed {seed} {np.dtype(dt).name} {kind} nesterov={nesterov} W={w} capacity {cap} keys {m}"

    def grads(n):
        return (rng.standard_normal((n, w)) * 3).astype(dt)

    def keys_of(n=None):
        pos = draw_positions(rng, m, n)
        if pos.size > 4 and np.unique(pos).size == 1:
            pos = pos[:2]  # (thousands of one key leave the bound no teeth: opt_util.BOUND_SHAPES)
        return pool[pos]

    def state_of(sh):
        """(p, slots) of rl.uniq as the oracles see them: a key the shard does not
        hold stands at zeros and the start state, and reads zeros from every array."""
        have = np.isin(rl.uniq, sh.keys())
        p = rows(sh, rl.uniq)
        slots = [rows(sh, rl.uniq, slot=i) for i in range(ns)]
        assert not p[~have].any() and not any(s[~have].any() for s in slots), f"{tag}: an absent key reads non-zero"
        for s, s0 in zip(slots, start_slots(hp, p.shape, dt)):
            s[~have] = s0[~have]
        return p, slots

    with ps.Shard.sparse(cap, dt, "assign", width=w) as sh:
        set_opt(sh, hp)
        first = pool[rng.permutation(m)[: int(rng.integers(0, m + 1))]]
        sh.add(first, rng.standard_normal((first.size, w)).astype(dt))
        steps = 0
        for step in range(int(rng.integers(4, 10))):
            op = int(rng.integers(0, 7))
            where = f"{tag} step {step} op {op}"
            device = bool(rng.integers(0, 2))
            c = cuda if device else None
            before = state_of(sh)
            if op in (0, 1):  # apply, apply_grouped
                ks = [keys_of() for _ in range(1 if op == 0 else int(rng.integers(2, 5)))]
                gs = [grads(k.size) for k in ks]
                if op == 0:
                    sh.apply(*((tdev(ks[0], cuda), tdev(gs[0], cuda)) if device else (ks[0], gs[0])))
                else:
                    sh.apply_grouped([(tdev(k, cuda), tdev(g, cuda)) if device else (k, g) for k, g in zip(ks, gs)])
                k, g = np.concatenate(ks), np.vstack(gs)
                if k.size == 0:
                    assert sh.step == steps, where  # no key: no step
                    continue
                steps += 1
                p_got, s_got = state_of(sh)
                idx = rl.rank(k).astype(np.int64)
                if kind == "ftrl":
                    ftrl_check(before, idx, g, p_got, s_got, dt, hp, where)
                else:
                    ou.check_step(before[0], before[1], idx, g, p_got, s_got, dt, hp, t=steps, msg=where)
            elif op in (2, 3):  # apply_pooled, apply_pooled_grouped
                weighted = kind != "ftrl" and bool(rng.integers(0, 2))  # (FTRL: the bag's row itself, bit for bit)
                batches = []
                for _ in range(1 if op == 2 else int(rng.integers(2, 4))):
                    k = keys_of(int(rng.choice([1, 5, 255, 2049])))
                    off = pu.offsets_of(ppu.bag_lens(str(rng.choice(["ones", "eights", "mixed", "one_bag"])), k.size))
                    bg = (rng.standard_normal((off.size - 1, w)) * 3).astype(dt)
                    batches.append((k, off, bg) + ((rng.standard_normal(k.size).astype(dt),) if weighted else ()))
                if op == 2:
                    b = batches[0]
                    ppu.apply_pooled(sh, b[0], b[1], b[2], b[3] if weighted else None, c)
                elif device:
                    import torch

                    sh.apply_pooled_grouped([(tdev(b[0], cuda), torch.from_numpy(b[1].astype(np.int64)).to(cuda),
                                              tdev(b[2].reshape(-1), cuda)) + ((tdev(b[3], cuda),) if weighted else ())
                                             for b in batches])
                else:
                    sh.apply_pooled_grouped(batches)
                steps += 1
                p_got, s_got = state_of(sh)
                # the one step of the concatenation: keys, bag rows and bag numbers back to back
                k = np.concatenate([b[0] for b in batches])
                bg = np.vstack([b[2] for b in batches])
                first_bag = np.cumsum([0] + [b[2].shape[0] for b in batches[:-1]])
                bag = np.concatenate([ppu.bag_index(b[1]) + f0 for b, f0 in zip(batches, first_bag)])
                wts = np.concatenate([b[3] for b in batches]) if weighted else None
                idx = rl.rank(k).astype(np.int64)
                if kind == "ftrl":
                    ftrl_check(before, idx, bg[bag], p_got, s_got, dt, hp, where)
                else:
                    ppu.check_step(before[0], before[1], idx, wts, bg, bag, p_got, s_got, dt, hp, t=steps, msg=where)
            elif op == 4 and ns:  # put_state then get_state: the rows come back bit for bit
                slot = int(rng.integers(0, ns))
                k = pool[rng.permutation(m)[: int(rng.integers(1, m + 1))]]
                v = np.abs(grads(k.size)) + dt(0.5)
                sh.put_state(*((tdev(k, cuda), tdev(v, cuda)) if device else (k, v)), slot=slot)
                assert np.array_equal(bits(rows(sh, k, None if device else cuda, slot=slot)), bits(v)), where
                assert np.isin(k, sh.keys()).all(), where  # a writing call: its keys are stored now
            elif op == 5:  # an assign Add between steps (it initialises parameters), host or device
                k = pool[rng.permutation(m)[: int(rng.integers(1, m + 1))]]
                v = rng.standard_normal((k.size, w)).astype(dt)
                sh.add(*((tdev(k, cuda), tdev(v, cuda)) if device else (k, v)))
                assert np.array_equal(bits(rows(sh, k, c)), bits(v)), where
            else:
                sh.sync()
            assert sh.step == steps, where
        assert sh.sparse_info()["count"] <= m
        sh.sync()


@pytest.mark.parametrize("first", range(SEED0, SEED0 + N_SCENARIOS, GROUP))
def test_sparse_fuzz(cuda, oracle_mod, first):
    for seed in range(first, min(first + GROUP, SEED0 + N_SCENARIOS)):
        if seed % 2 == 0:
            storage_scenario(seed, cuda, oracle_mod)
        else:
            optimizer_scenario(seed, cuda)
