"""Differential fuzzing of sparse shards that grow and forget (pskv_sparse_reserve,
pskv_sparse_set_growth, pskv_sparse_erase) against a model.  The 40 seeded
scenarios are drawn on the CPU by sparse_grow_util.draw_scenario (capacities 8
to 256, at most 600 key positions per call, more keys than the first capacity)
and mix reserve, set_growth and erase with every read and write call, host and
device.

  storage    (even seeds) a mode, any dtype, no optimizer.  The model is a
             Python dict, key -> row: an assign Add stores the last row of a key
             (RowOracle's map semantics), an accumulate Add of distinct keys adds
             once in the shard's own dtype (one rounding, as the kernel's), an
             erase deletes the entry, an absent key reads zeros.
  optimizer  (odd seeds) one of the six kinds.  The model is the row-shard twin
             of the relabelling statement (include/pskv.h): the dense row shard
             [0, m) fed rank(K), where an erase is an assign Add of zero rows
             plus put_state of the start values; a key the model does not hold
             must read zeros from the sparse shard.

Every call is compared bit for bit -- after it, the whole pool's rows (and
state) against the model, the capacity and the count against the growth rule
-- except the calls the model marks order_dependent (duplicated keys in an
accumulate Add or a step): those are applied, and the model takes the shard's
rows of their keys.  tests/test_sparse_grow_cpu.py checks on the model alone
that at least 90 % of the calls are compared.

Seeded: a failure names its scenario and call, and reruns identically.
"""
import os

import numpy as np
import pytest

import pooled_push_util as ppu
import pooled_util as pu
import sparse_grow_util as gu
import sparse_util as su
from rows_util import bits
from test_gpu_parity import tdev
from test_sparse_gpu import KIND_IDS, KINDS, hyper_of, n_slots, rows, set_opt, start_slots

pytestmark = pytest.mark.gpu

N_SCENARIOS = int(os.environ.get("FUZZ_SCENARIOS", "40"))
SEED0 = int(os.environ.get("FUZZ_SEED0", "0"))
GROUP = 10  # scenarios per test case


def batches_of(call, vals):
    c = call["cuts"]
    return [(call["keys"][a:b], vals[a:b]) for a, b in zip(c[:-1], c[1:])]


def maintenance(sh, call, cuda):
    """reserve / set_growth / erase / sync on the sparse shard; True when the call was one."""
    op = call["op"]
    if op == "reserve":
        sh.reserve(call["to"])
    elif op == "set_growth":
        sh.set_growth(call["to"])
    elif op == "erase":
        sh.erase(tdev(call["keys"], cuda) if call["dev"] and call["keys"].size else call["keys"])
    elif op == "sync":
        sh.sync()
    else:
        return False
    return True


def check_shape(sh, call, where):
    i = sh.sparse_info()
    assert (i["capacity"], i["count"], i["table_slots"]) == (call["capacity"], call["count"],
                                                            gu.table_slots(call["capacity"])), where
    assert sh.growth()["rebuilds"] == call["rebuilds"], where


def storage_scenario(sc, cuda):
    import parameter_server_amd as ps

    rng = np.random.default_rng([sc["seed"], 1])
    dt, w, mode, pool = np.dtype(sc["dtype"]), sc["w"], sc["mode"], sc["pool"]
    model = {}  # key -> row
    zero = np.zeros(w, dtype=dt)
    everything = np.concatenate([pool, sc["gone"]])
    counter = [1]

    def values(n):
        if mode == "accumulate":
            if dt == np.int32:
                return rng.integers(-2**31, 2**31, size=(n, w)).astype(np.int32)
            return (rng.standard_normal((n, w)) * 3).astype(dt)
        v = (counter[0] + np.arange(n * w, dtype=np.int64)) % (2**24 - 1) + 1  # unique per occurrence and column
        counter[0] += n * w
        return v.reshape(n, w).astype(dt)

    def note(keys, vals):
        for k, v in zip(keys.tolist(), vals):
            model[k] = v.copy() if mode == "assign" else model.get(k, zero) + v  # (int32 wraps, floats round once)

    def expect(keys):
        return np.array([model.get(k, zero) for k in keys.tolist()], dtype=dt).reshape(len(keys), w)

    def compare(keys, got, where):
        got = np.asarray(got).reshape(len(keys), w)
        assert got.dtype == dt and np.array_equal(bits(got), bits(expect(keys))), where

    def dev(x, on):
        return tdev(np.ascontiguousarray(x), cuda) if on else x

    with ps.Shard.sparse(sc["capacity"], dt, mode, width=w) as sh:
        for ci, call in enumerate(sc["calls"]):
            op, d = call["op"], call["dev"]
            where = f"storage seed {sc['seed']} {dt.name} {mode} W={w} call {ci} {op} dev={d}"
            if maintenance(sh, call, cuda):
                if op == "erase":
                    for k in call["keys"].tolist():
                        model.pop(k, None)
            elif op in ("add", "add_grouped", "add_get_grouped"):
                keys, vals = call["keys"], values(call["keys"].size)
                if op == "add":
                    sh.add(dev(keys, d), dev(vals, d))
                elif op == "add_grouped":
                    sh.add_grouped([(dev(k, d), dev(v, d)) for k, v in batches_of(call, vals)])
                else:
                    outs = [gu.su_empty(q.size, w, dt, cuda if d else None) for q in call["reads"]]
                    sh.add_get_grouped([(dev(k, d), dev(v, d)) for k, v in batches_of(call, vals)],
                                       [(dev(q, d), o) for q, o in zip(call["reads"], outs)])
                if call["order_dependent"]:  # left out: the model takes the shard's rows of these keys
                    uniq = np.unique(keys)
                    for k, r in zip(uniq.tolist(), rows(sh, uniq)):
                        model[k] = r.copy()
                else:
                    note(keys, vals)
                    if op == "add_get_grouped":  # the Get half sees the Add half
                        for q, o in zip(call["reads"], outs):
                            compare(q, su._host(o), where + " (the Get half)")
            elif op == "get":
                compare(call["keys"], su._host(sh.get(dev(call["keys"], d))), where)
            elif op == "get_grouped":
                parts = batches_of(call, call["keys"])
                outs = [gu.su_empty(k.size, w, dt, cuda if d else None) for k, _ in parts]
                sh.get_grouped([(dev(k, d), o) for (k, _), o in zip(parts, outs)])
                for (k, _), o in zip(parts, outs):
                    compare(k, su._host(o), where)
            elif op == "get_pooled":  # from the model's rows: absent keys index the zero row behind them
                keys, off = call["keys"], gu.bag_offsets(call)
                wts = pu.draw_values(rng, keys.size, dt) if call["weighted"] else None
                uniq = np.unique(keys)
                p = np.vstack([expect(uniq), zero[None, :]])
                idx = np.searchsorted(uniq, keys).astype(np.uint32)
                pu.check(pu.pooled(sh, keys, off, wts, cuda if d else None), pu.reference(p, 0, idx, off, wts), where)
            else:
                raise ValueError(op)
            if not call["order_dependent"]:
                compare(everything, rows(sh, everything, cuda if ci % 2 else None), where + ": the whole pool afterwards")
            check_shape(sh, call, where)
            assert sorted(sh.keys().tolist()) == sorted(model), where
        sh.sync()  # never full: the scenarios do not overfill


def optimizer_scenario(sc, cuda):
    import parameter_server_amd as ps

    rng = np.random.default_rng([sc["seed"], 2])
    dt, w, pool = np.dtype(sc["dtype"]), sc["w"], sc["pool"]
    kind, nesterov = KINDS[KIND_IDS.index(sc["opt"])]
    hp = hyper_of(kind, nesterov, wd=sc["wd"])
    ns = n_slots(hp)
    rl = su.Relabel(pool)
    start = start_slots(hp, (1, w), dt)
    stored = set()
    tw = su.Twin(ps, sc["capacity"], dt, "assign", w, rl, cuda)

    def g(n):
        return (rng.standard_normal((n, w)) * 3).astype(dt)

    def compare(where, c):
        """Stored keys: the twin's bits; every other key of the pool, and absent keys: zeros."""
        have = np.isin(rl.uniq, np.array(sorted(stored), dtype=np.uint32))
        for slot in [None] + list(range(ns)):
            a = rows(tw.sp, rl.uniq, c, slot=slot)
            b = rows(tw.dn, rl.rank(rl.uniq), c, slot=slot)
            assert np.array_equal(bits(a[have]), bits(b[have])), f"{where}: stored keys differ from the twin, slot {slot}"
            assert not a[~have].any() and not rows(tw.sp, sc["gone"], c, slot=slot).any(), \
                f"{where}: a key that is not stored reads non-zero, slot {slot}"
        assert tw.sp.step == tw.dn.step, where

    def resync(keys):
        """An order-dependent step: the twin takes the sparse shard's rows of its keys."""
        uniq = np.unique(keys)
        tw.dn.add(rl.rank(uniq), rows(tw.sp, uniq))
        for slot in range(ns):
            tw.dn.put_state(rl.rank(uniq), rows(tw.sp, uniq, slot=slot), slot=slot)

    try:
        tw.each(lambda sh, f: set_opt(sh, hp))
        for ci, call in enumerate(sc["calls"]):
            op, d = call["op"], call["dev"]
            where = f"optimizer seed {sc['seed']} {dt.name} {sc['opt']} W={w} call {ci} {op} dev={d}"
            if maintenance(tw.sp, call, cuda):
                if op == "erase":  # on the twin: zero rows and the start state at rank(K)
                    k = np.array(sorted(stored & set(call["keys"].tolist())), dtype=np.uint32)
                    if k.size:
                        tw.dn.add(rl.rank(k), np.zeros((k.size, w), dtype=dt))
                        for slot in range(ns):
                            tw.dn.put_state(rl.rank(k), np.repeat(start[slot], k.size, axis=0), slot=slot)
                    stored.difference_update(call["keys"].tolist())
            elif op in ("apply", "add"):
                tw.write(op, call["keys"], g(call["keys"].size), dev=d)
            elif op == "apply_grouped":
                tw.write_grouped(op, batches_of(call, g(call["keys"].size)), dev=d)
            elif op == "put_state":
                tw.write(op, call["keys"], np.abs(g(call["keys"].size)) + dt.type(0.5), dev=d, slot=call["slot"])
            elif op == "apply_pooled":
                off = gu.bag_offsets(call)
                wts = rng.standard_normal(call["keys"].size).astype(dt) if call["weighted"] else None
                tw.apply_pooled(call["keys"], off, g(off.size - 1), wts, dev=d)
            elif op == "apply_pooled_grouped":
                batches = []
                for a, b in zip(call["cuts"][:-1], call["cuts"][1:]):
                    if a == b:
                        continue  # (a pooled batch holds a key)
                    off = pu.offsets_of(ppu.bag_lens(call["bags"], b - a))
                    batches.append((call["keys"][a:b], off, g(off.size - 1)) +
                                   ((rng.standard_normal(b - a).astype(dt),) if call["weighted"] else ()))
                tw.apply_pooled_grouped(batches, dev=d)
            elif op in ("get", "get_state"):
                kw = {"slot": call["slot"]} if op == "get_state" else {}
                inside = rl.holds(call["keys"]) & np.isin(call["keys"], np.array(sorted(stored), dtype=np.uint32))
                got = su._host(getattr(tw.sp, op)(tdev(call["keys"], cuda) if d else call["keys"], **kw))
                got = got.reshape(call["keys"].size, w)
                want = rows(tw.dn, rl.rank(call["keys"][inside]), slot=kw.get("slot"))
                assert np.array_equal(bits(got[inside]), bits(want)) and not got[~inside].any(), where
            else:
                raise ValueError(op)
            if "keys" in call and op not in ("erase", "get", "get_state"):
                stored.update(call["keys"].tolist())
            if call["order_dependent"]:
                resync(call["keys"])
            else:
                compare(where, cuda if ci % 2 else None)
            check_shape(tw.sp, call, where)
            assert sorted(tw.sp.keys().tolist()) == sorted(stored), where
        tw.sp.sync()
        tw.dn.sync()
    finally:
        tw.close()


@pytest.mark.parametrize("first", range(SEED0, SEED0 + N_SCENARIOS, GROUP))
def test_sparse_grow_fuzz(cuda, first):
    for seed in range(first, min(first + GROUP, SEED0 + N_SCENARIOS)):
        sc = gu.draw_scenario(seed)
        if sc["kind"] == "storage":
            storage_scenario(sc, cuda)
        else:
            optimizer_scenario(sc, cuda)
