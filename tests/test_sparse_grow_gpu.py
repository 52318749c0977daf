"""GPU tests of growth and erase of sparse shards (pskv_sparse_reserve,
pskv_sparse_set_growth, pskv_sparse_erase; include/pskv.h "Sparse shards",
DESIGN.md §8l).

The bars:
  * reserve and erase keep every surviving key's row and every state slot bit
    for bit (the shard's own replies before and after);
  * a shard that grows by itself returns, with distinct keys per call, the very
    bits a FIXED sparse shard of ample capacity returns for the same calls
    (sparse_grow_util.Pair) -- work the fixed shard could always do -- and
    assign Adds are bit-exact against RowOracle on the raw keys;
  * the capacities a growing shard goes through are those of the growth rule
    (sparse_grow_util.grown_capacity), whatever the timing;
  * an erased key reads zeros everywhere, is gone from keys(), and comes back as
    a new key; at a full shard erasing k keys makes room for exactly k.
Keys come from the whole uint32 space with 0, 2^31 and 0xFFFFFFFF among them
(sparse_util.key_pool); capacity 8 starts from a 16-entry index.
"""
import os
import subprocess

import numpy as np
import pytest

import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
import sparse_grow_util as gu
import sparse_util as su
from rows_util import RowOracle, ValueSource, bits
from test_gpu_parity import tdev
from test_sparse_gpu import (KIND_IDS, KINDS, PATHS, hyper_of, n_slots, one_step_check_stored, ps_mod, push, rows, set_opt,
                             start_slots)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSKV_EINVAL, PSKV_ESTATE = -1, -4
WIDTHS = [1, 3, 4, 16, 33]


def snapshot(sh, keys, ns, cuda=None):
    """[p, slot 0, ...] of `keys` as bit patterns."""
    return [bits(rows(sh, keys, cuda))] + [bits(rows(sh, keys, cuda, slot=i)) for i in range(ns)]


def same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{what}: array {i} (0 = p, then the state slots) changed"


def full_error(ps, sh):
    with pytest.raises(ps.PskvError) as e:
        sh.sync()
    assert e.value.code == PSKV_ESTATE and "sparse shard full" in str(e.value)


def conf_of(sh):
    """The optimizer configuration (state_bytes follows the capacity)."""
    return {k: v for k, v in sh.optimizer().items() if k != "state_bytes"}


def info(sh):
    i = sh.sparse_info()
    return i["capacity"], i["count"], i["table_slots"]


# ---------------------------------------------------------------------- reserve
@pytest.mark.parametrize("kind,nesterov", KINDS, ids=KIND_IDS)
def test_reserve_keeps_rows_state_step_and_configuration(cuda, kind, nesterov):
    """Capacity 8 (a 16-entry table) filled exactly, reserve(20) (64 entries)."""
    ps = ps_mod()
    ki = KIND_IDS.index("nesterov" if nesterov else kind)
    w, dtype = [1, 3, 4, 16, 33, 3][ki], [np.float32, np.float64][ki % 2]
    rng = np.random.default_rng(ou.case_seed("grow-reserve", kind, nesterov))
    pool = su.key_pool(rng, 21)
    hp = hyper_of(kind, nesterov)
    ns = n_slots(hp)
    g = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
    with ps.Shard.sparse(8, dtype, "assign", width=w) as sh:
        set_opt(sh, hp)
        sh.add(pool[:8], g(8))
        sh.apply(tdev(pool[:8], cuda), tdev(g(8), cuda))
        sh.apply(pool[2:7], g(5))
        assert info(sh) == (8, 8, 16)
        sh.set_option("NT", 0)
        before, conf = snapshot(sh, pool, ns), conf_of(sh)
        sh.reserve(20)
        assert info(sh) == (20, 8, 64) and sh.sparse_info()["index_bytes"] == 64 * 8 + 20 * 4
        assert sh.info()["dense_bytes"] == 21 * w * np.dtype(dtype).itemsize
        same(before, snapshot(sh, pool, ns), "reserve(20), host reads")
        same(before, snapshot(sh, pool, ns, cuda), "reserve(20), device reads")
        assert sh.step == 2 and conf_of(sh) == conf and sh.get_option("NT") == 0
        assert sorted(sh.keys().tolist()) == sorted(pool[:8].tolist())
        assert sh.growth() == {"max_capacity": 0, "rebuilds": 1}
        # twelve more keys fit; the first step of a new key starts from the start state
        sh.apply(tdev(pool[8:20], cuda), tdev(g(12), cuda))
        sh.sync()
        assert info(sh) == (20, 20, 64) and sh.step == 3
        same([b[:8] for b in before], [a[:8] for a in snapshot(sh, pool, ns)], "the old keys after the new keys' step")
        sh.apply(pool[19:21], g(2))  # the 21st key is dropped
        full_error(ps, sh)
        assert info(sh)[1] == 20 and not rows(sh, pool[20:]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32], ids=["f32", "f64", "i32"])
@pytest.mark.parametrize("cap,to,w", [(8, 20, 1), (8, 20, 33), (100, 101, 3), (100, 2049, 4), (100, 300, 16)])
def test_reserve_on_a_shard_filled_exactly_against_the_map_oracle(oracle_mod, cuda, cap, to, w, dtype):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-reserve-map", cap, to, w, np.dtype(dtype).name))
    pool = su.key_pool(rng, to + 1)
    orc = RowOracle(oracle_mod, dtype, "assign", w, 0, 1 << 32)
    src = ValueSource(dtype, "assign", rng)
    with ps.Shard.sparse(cap, dtype, "assign", width=w) as sh:
        for a in (0, 1):  # twice: the second Add meets stored keys only
            keys = pool[:cap][rng.permutation(cap)]
            vals = src.rows(cap, w)
            push(sh, PATHS[2 * a + (w % 2)], keys, vals, cuda)
            orc.add(keys, vals)
        sh.sync()
        assert info(sh)[:2] == (cap, cap)
        sh.reserve(to)
        assert info(sh) == (to, cap, gu.table_slots(to))
        orc.check(pool, rows(sh, pool, cuda), "after reserve")
        keys, vals = pool[:to][rng.permutation(to)], src.rows(to, w)
        push(sh, PATHS[w % 4], keys, vals, cuda)
        orc.add(keys, vals)
        sh.sync()  # clean: every key found room
        assert info(sh)[:2] == (to, to)
        orc.check(pool, rows(sh, pool), "filled exactly after reserve")
        sh.add(pool[to:], src.rows(1, w))
        full_error(ps, sh)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_reserve_recovers_a_full_shard(cuda, dev):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-recover", dev))
    w, dtype = 3, np.float32
    pool = su.key_pool(rng, 12)
    vals = ou.dyadic_grads(rng, 12, w, dtype) + dtype(50)
    with ps.Shard.sparse(8, dtype, "assign", width=w) as sh:
        push(sh, "device" if dev else "host", pool, vals, cuda)
        full_error(ps, sh)
        full_error(ps, sh)  # sticky
        held = sh.keys()
        dropped = pool[~np.isin(pool, held)]
        assert held.size == 8 and dropped.size == 4
        sh.reserve(12)
        sh.sync()  # the condition is cleared
        assert info(sh) == (12, 8, 32) and not rows(sh, dropped).any()
        push(sh, "device" if dev else "host", dropped, vals[:4], cuda)  # dropped keys are forgotten: they insert now
        sh.sync()
        assert info(sh)[1] == 12
        assert np.array_equal(bits(rows(sh, dropped, cuda if dev else None)), bits(vals[:4]))
        at = {int(k): i for i, k in enumerate(pool)}
        assert np.array_equal(bits(rows(sh, held)), bits(vals[[at[int(k)] for k in held]]))


def test_reserve_equal_smaller_and_calls_on_a_dense_shard(cuda):
    ps = ps_mod()
    from parameter_server_amd import _lib

    lib = _lib.lib
    err = lambda: lib.pskv_last_error().decode()  # noqa: E731
    keys = np.array([5, 0xFFFFFFFF, 9], dtype=np.uint32)
    vals = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    with ps.Shard.sparse(8, np.float32, "assign", width=4) as sh:
        sh.add(keys, vals)
        ptr = sh.info()["dense_bytes"]
        assert lib.pskv_sparse_reserve(sh.handle, 8) == 0  # equal: nothing happens
        assert lib.pskv_sparse_reserve(sh.handle, 7) == PSKV_EINVAL and "capacity" in err()
        assert lib.pskv_sparse_reserve(sh.handle, 1) == PSKV_EINVAL
        assert lib.pskv_sparse_set_growth(sh.handle, 7) == PSKV_EINVAL and "max_capacity" in err()
        assert info(sh) == (8, 3, 16) and sh.growth() == {"max_capacity": 0, "rebuilds": 0}
        assert sh.info()["dense_bytes"] == ptr and np.array_equal(rows(sh, keys), vals)
        sh.set_growth(8)  # the current capacity is a legal limit
        sh.set_growth(0)
        sh.erase(np.empty(0, dtype=np.uint32))  # n == 0: nothing at all
        assert sh.growth()["rebuilds"] == 0
        sh.sync()
    with ps.Shard(0, 64, np.float32, "assign", width=4) as dn:
        dn.add(np.array([3], dtype=np.uint32), vals[:1])
        assert lib.pskv_sparse_reserve(dn.handle, 100) == PSKV_EINVAL and "not a sparse shard" in err()
        assert lib.pskv_sparse_set_growth(dn.handle, 100) == PSKV_EINVAL and "not a sparse shard" in err()
        assert lib.pskv_sparse_set_growth(dn.handle, 0) == PSKV_EINVAL
        assert lib.pskv_sparse_get_growth(dn.handle, None, None) == PSKV_EINVAL and "not a sparse shard" in err()
        assert lib.pskv_sparse_erase(dn.handle, keys.ctypes.data, 3, 0) == PSKV_EINVAL and "not a sparse shard" in err()
        assert np.array_equal(rows(dn, np.array([3], dtype=np.uint32)), vals[:1])
        dn.sync()


# ------------------------------------------------------------------ auto-growth
@pytest.mark.parametrize("dtype,w", [(np.float32, 1), (np.float64, 3), (np.int32, 4), (np.float32, 16), (np.int32, 33)],
                         ids=["f32-1", "f64-3", "i32-4", "f32-16", "i32-33"])
@pytest.mark.parametrize("per_call", [4100, 37])
def test_autogrowth_assign_from_capacity_8_to_the_limit(oracle_mod, cuda, per_call, dtype, w):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-assign", per_call, np.dtype(dtype).name, w))
    pool = su.key_pool(rng, 4101)
    orc = RowOracle(oracle_mod, dtype, "assign", w, 0, 1 << 32)
    src = ValueSource(dtype, "assign", rng)
    cm = gu.CapacityModel(8, 4100)
    with ps.Shard.sparse(8, dtype, "assign", width=w, max_capacity=4100) as sh:
        assert sh.growth() == {"max_capacity": 4100, "rebuilds": 0}
        for i, a in enumerate(range(0, 4100, per_call)):
            keys = pool[a:min(a + per_call, 4100)]
            vals = src.rows(keys.size, w)
            push(sh, PATHS[i % 4], keys, vals, cuda)
            orc.add(keys, vals)
            cm.write(keys)
            if per_call == 4100 or i % 7 == 0 or cm.capacity == 4100:
                assert info(sh) == (cm.capacity, cm.count, gu.table_slots(cm.capacity)), f"call {i}"
        sh.sync()  # no key was dropped on the way
        assert info(sh)[:2] == (4100, 4100) and sh.growth()["rebuilds"] == cm.rebuilds
        assert cm.rebuilds == (1 if per_call == 4100 else 8)
        orc.check(pool, rows(sh, pool, cuda), "after growth, device read")
        orc.check(pool, rows(sh, pool), "after growth, host read")
        assert sorted(sh.keys().tolist()) == sorted(pool[:4100].tolist())
        sh.add(pool[4090:], src.rows(11, w))  # key 4101: past the limit
        full_error(ps, sh)
        assert info(sh)[:2] == (4100, 4100) and not rows(sh, pool[4100:]).any()


def _entry_call(tw, entry, keys, dtype, w, rng, dev):
    """One writing call of `keys` through `entry` on both shards of the pair."""
    g = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
    n = keys.size
    cut = [0, 1, n // 3, n // 3, n]
    if entry == "add":
        tw.write("add", keys, g(n), dev=dev)
    elif entry == "add_grouped":
        tw.write_grouped("add_grouped", [(keys[a:b], g(b - a)) for a, b in zip(cut[:-1], cut[1:])], dev=dev)
    elif entry == "add_get_grouped":
        tw.add_get([(keys[a:b], g(b - a)) for a, b in zip(cut[:-1], cut[1:])], [keys[::-1], keys[:5]], dev=dev)
    elif entry == "apply":
        tw.write("apply", keys, g(n), dev=dev)
    elif entry == "apply_grouped":
        tw.write_grouped("apply_grouped", [(keys[a:b], g(b - a)) for a, b in zip(cut[:-1], cut[1:])], dev=dev)
    elif entry == "apply_pooled":
        off = pu.offsets_of(ppu.bag_lens("mixed", n))
        tw.apply_pooled(keys, off, g(off.size - 1), rng.standard_normal(n).astype(dtype), dev=dev)
    elif entry == "apply_pooled_grouped":
        batches = []
        for a, b in zip(cut[:-1], cut[1:]):
            if b > a:
                off = pu.offsets_of(ppu.bag_lens("eights", b - a))
                batches.append((keys[a:b], off, g(off.size - 1), rng.standard_normal(b - a).astype(dtype)))
        tw.apply_pooled_grouped(batches, dev=dev)
    elif entry == "put_state":
        tw.write("put_state", keys, np.abs(g(n)) + dtype(0.5), dev=dev, slot=0)
    else:
        raise ValueError(entry)


ENTRIES = ["add", "add_grouped", "add_get_grouped", "apply", "apply_grouped", "apply_pooled", "apply_pooled_grouped",
           "put_state"]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_writing_entry_point_grows_the_shard_itself(cuda, entry, dev):
    """From capacity 8; with distinct keys the grown shard holds the bits of a
    fixed shard of capacity 8192 fed the same calls."""
    ps = ps_mod()
    ei = ENTRIES.index(entry)
    w, dtype = WIDTHS[ei % 5], [np.float32, np.float64][(ei + dev) % 2]
    rng = np.random.default_rng(ou.case_seed("grow-entry", entry, dev))
    pool = su.key_pool(rng, 2600)
    hp = hyper_of("adagrad" if ei % 2 else "adam", False)
    tw = gu.Pair(ps, 8, 8192, 8192, dtype, "assign", w, su.Relabel(pool), cuda)
    cm = gu.CapacityModel(8, 8192)
    try:
        tw.each(lambda sh, f: set_opt(sh, hp))
        for n in (5, 2049, 300):  # fits; grows past a chunk; old and new keys side by side
            keys = pool[rng.permutation(pool.size)[:n]]
            _entry_call(tw, entry, keys, dtype, w, rng, dev)
            cm.write(keys)
            assert info(tw.sp) == (cm.capacity, cm.count, gu.table_slots(cm.capacity)), (entry, n)
        assert cm.rebuilds >= 1 and tw.sp.growth()["rebuilds"] == cm.rebuilds and tw.dn.growth()["rebuilds"] == 0
        tw.check_all(n_slots(hp), what=f"{entry} dev={dev}")
        assert sorted(tw.sp.keys().tolist()) == sorted(tw.dn.keys().tolist())
    finally:
        tw.close()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_a_grouped_call_grows_before_its_first_insert_not_between_launch_groups(cuda, dev):
    """70 batches are two launch groups (64 batches each at most): the rule sees
    the key positions of all of them, and the shard grows once, in front."""
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-groups", dev))
    w, dtype = 3, np.float32
    pool = su.key_pool(rng, 210)
    tw = gu.Pair(ps, 8, 8192, 8192, dtype, "assign", w, su.Relabel(pool), cuda)
    try:
        tw.each(lambda sh, f: sh.set_optimizer("sgd", lr=0.125))
        g = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
        tw.write_grouped("add_grouped", [(pool[3 * i:3 * i + 3], g(3)) for i in range(70)], dev=dev)
        assert info(tw.sp) == (210, 210, 512) and tw.sp.growth()["rebuilds"] == 1
        keys = pool[rng.permutation(210)]
        tw.write_grouped("apply_grouped", [(keys[3 * i:3 * i + 3], g(3)) for i in range(70)], dev=dev)
        assert info(tw.sp) == (420, 210, 1024) and tw.sp.growth()["rebuilds"] == 2  # 210 + 210 positions > 210
        tw.check_all(0, what="70 batches")
    finally:
        tw.close()


@pytest.mark.parametrize("grow", [False, True], ids=["fixed", "grows"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype,w", [(np.float32, 3), (np.float32, 4), (np.float64, 3), (np.float64, 4)],
                         ids=["f32-w3", "f32-w4", "f64-w3", "f64-w4"])
def test_tiny_pooled_calls_at_capacity_8_against_the_reference_models(cuda, dtype, w, dev, grow):
    """The three pooled calls through their one front, each against its Python
    model on ranks: a grouped push whose caller batch 0 is empty, a single
    push and a pull, 2-3 bags over 5-11 keys with a key in two bags, the pull
    with an absent key.  grows: each push has more key positions than the shard
    has free slots, so growth (limit 64) fires inside the call."""
    import pooled_push_group_util as ggu

    ps, hp, dt = ps_mod(), ppu.hyper("sgd"), np.dtype(dtype)
    rng = np.random.default_rng(ou.case_seed("tiny-pooled", dt.name, w, dev, grow))
    pool = su.key_pool(rng, 16)
    rl = su.Relabel(pool)
    c = cuda if dev else None
    bag_rows = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
    cm = gu.CapacityModel(8, 64 if grow else 0)
    with ps.Shard.sparse(8, dtype, "assign", width=w, max_capacity=64 if grow else None) as sh:
        ppu.set_optimizer(sh, hp)
        p = np.zeros((rl.m, w), dtype=dtype)
        # grouped push: the live batch is the caller's batch 1; its first key is also its last
        k = np.append(pool[:10 if grow else 5], pool[0])
        live = (k, pu.offsets_of([3, 0, k.size - 3]), bag_rows(3), rng.standard_normal(k.size).astype(dtype))
        ggu.apply_grouped(sh, [ggu.empty_batch(w, dtype, nbags=1), live], c)
        cm.write(k)
        assert info(sh) == (cm.capacity, cm.count, gu.table_slots(cm.capacity)) and sh.growth()["rebuilds"] == cm.rebuilds
        got = rows(sh, rl.uniq)
        ggu.check_step(p, [], 0, [(rl.rank(k),) + live[1:]], got, [], dt, hp, t=1, msg="grouped push")
        p = got
        # single push: stored and new keys, unweighted
        k = np.concatenate([pool[3:5], pool[10:14] if grow else pool[5:7], pool[3:4]])
        off, bg = pu.offsets_of([2, k.size - 2]), bag_rows(2)
        ppu.apply_pooled(sh, k, off, bg, None, c)
        cm.write(k)
        assert info(sh) == (cm.capacity, cm.count, gu.table_slots(cm.capacity)) and sh.growth()["rebuilds"] == cm.rebuilds
        got = rows(sh, rl.uniq)
        ppu.check_step(p, [], rl.rank(k).astype(np.int64), None, bg, ppu.bag_index(off), got, [], dt, hp, t=2,
                       msg="single push")
        p = got
        # pull: pool[0] in two bags, pool[15] absent (it reads zeros and is not inserted)
        k = pool[[0, 1, 15, 0, 2, 3, 4]]
        off, wts = pu.offsets_of([3, 0, 4]), rng.standard_normal(7).astype(dtype)
        assert not p[rl.rank(pool[15:16])].any()
        pu.check(pu.pooled(sh, k, off, wts, c), pu.reference(p, 0, rl.rank(k), off, wts), "pull")
        assert info(sh)[:2] == (cm.capacity, cm.count) and sh.step == 2
        assert cm.rebuilds == (2 if grow else 0) and cm.capacity == (32 if grow else 8)
        sh.sync()


@pytest.mark.parametrize("kind", ["adagrad", "adam", "ftrl"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_a_growing_step_with_duplicated_keys_passes_the_one_step_check(cuda, kind, dev):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-dups", kind, dev))
    w, dtype = [3, 4, 16][["adagrad", "adam", "ftrl"].index(kind)], np.float32
    pool = su.key_pool(rng, 600)
    rl = su.Relabel(pool)
    hp = hyper_of(kind, False, wd=0.0)
    with ps.Shard.sparse(8, dtype, "assign", width=w, max_capacity=1024) as sh:
        set_opt(sh, hp)
        state = (np.zeros((rl.m, w), dtype=dtype), start_slots(hp, (rl.m, w), dtype))
        for step, (name, keys) in enumerate(su.pool_patterns(rng, 2049, pool).items()):
            if name == "all_equal":
                keys = keys[:2]  # (opt_util.BOUND_SHAPES: thousands of one key leave the bound no teeth)
            grads = (rng.standard_normal((keys.size, w)) * 3).astype(dtype)
            push(sh, ("device" if dev else "host") + ("_grouped" if step % 2 else ""), keys, grads, cuda, method="apply")
            have = np.isin(rl.uniq, sh.keys())
            state = one_step_check_stored(sh, rl, hp, state, keys, grads, have, f"{name} step {step}")
        sh.sync()
        assert sh.growth()["rebuilds"] >= 1 and info(sh)[0] > 8


@pytest.mark.parametrize("kind,nesterov", KINDS, ids=KIND_IDS)
def test_growth_in_mid_training_equals_the_fixed_shard(cuda, kind, nesterov):
    """12 steps over a widening key set, distinct keys per call."""
    ps = ps_mod()
    ki = KIND_IDS.index("nesterov" if nesterov else kind)
    w, dtype = WIDTHS[ki % 5], [np.float32, np.float64][ki % 2]
    rng = np.random.default_rng(ou.case_seed("grow-train", kind, nesterov))
    pool = su.key_pool(rng, 3000)
    hp = hyper_of(kind, nesterov)
    tw = gu.Pair(ps, 8, 4096, 4096, dtype, "assign", w, su.Relabel(pool), cuda)
    cm = gu.CapacityModel(8, 4096)
    try:
        tw.each(lambda sh, f: set_opt(sh, hp))
        g = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
        for step in range(12):
            wide = min(pool.size, 6 * 2**step)  # 6, 12, ... keys in play: rebuilds fall between steps
            keys = pool[:wide][rng.permutation(wide)[: max(3, (2 * wide) // 3)]]
            dev = bool(step % 2)
            if step % 3 == 2:
                cut = keys.size // 2
                tw.write_grouped("apply_grouped", [(keys[:cut], g(cut)), (keys[cut:], g(keys.size - cut))], dev=dev)
            else:
                tw.write("apply", keys, g(keys.size), dev=dev)
            cm.write(keys)
            if step % 4 == 3:
                tw.check_all(n_slots(hp), what=f"step {step}")
                assert info(tw.sp)[:2] == (cm.capacity, cm.count)
        tw.check_all(n_slots(hp))
        assert tw.sp.step == tw.dn.step == 12
        assert tw.sp.growth()["rebuilds"] == cm.rebuilds and cm.rebuilds >= 4
        assert info(tw.sp) == (cm.capacity, cm.count, gu.table_slots(cm.capacity))
    finally:
        tw.close()


# ------------------------------------------------------------------------ erase
def _erase_list(form, rng, stored, gone):
    if form == "one":
        return stored[5:6]
    if form == "subset":
        return stored[rng.permutation(stored.size)[:700]]
    if form == "all":
        return stored[rng.permutation(stored.size)]
    if form == "4100_of_8192":
        return stored[rng.permutation(stored.size)[:4100]]
    if form == "absent_and_repeats":
        k = stored[rng.permutation(stored.size)[:300]]
        return rng.permutation(np.concatenate([k, gone, k[:150], gone[:7]]))
    if form == "only_absent":
        return gone
    assert form == "empty"
    return stored[:0]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("form", ["one", "subset", "all", "4100_of_8192", "absent_and_repeats", "only_absent", "empty"])
def test_erase_forgets_the_listed_keys_and_keeps_the_rest(cuda, form, dev):
    ps = ps_mod()
    fi = ["one", "subset", "all", "4100_of_8192", "absent_and_repeats", "only_absent", "empty"].index(form)
    kind, nesterov = KINDS[fi % 6]
    w, dtype = WIDTHS[fi % 5], [np.float32, np.float64][fi % 2]
    rng = np.random.default_rng(ou.case_seed("grow-erase", form, dev))
    m = 8192 if form == "4100_of_8192" else 2100
    pool = su.key_pool(rng, m)
    gone = su.absent_keys(rng, pool, 40)
    hp = hyper_of(kind, nesterov)
    ns = n_slots(hp)
    with ps.Shard.sparse(m, dtype, "assign", width=w) as sh:
        set_opt(sh, hp)
        sh.add(pool, rng.standard_normal((m, w)).astype(dtype))
        sh.apply(tdev(pool, cuda), tdev((rng.standard_normal((m, w)) * 3).astype(dtype), cuda))
        sh.sync()
        conf = conf_of(sh)
        k = _erase_list(form, rng, pool, gone)
        out = np.isin(pool, k)
        before = snapshot(sh, pool, ns)
        sh.erase(tdev(k, cuda) if dev else k)
        assert info(sh) == (m, m - int(out.sum()), gu.table_slots(m))
        assert sh.growth()["rebuilds"] == (0 if form == "empty" else 1)
        for c in (None, cuda):
            after = snapshot(sh, np.concatenate([pool, gone]), ns, c)
            same([b[~out] for b in before], [a[:m][~out] for a in after], f"{form}: survivors")
            assert not any(a[:m][out].any() or a[m:].any() for a in after), f"{form}: an erased or absent key reads non-zero"
        assert sorted(sh.keys().tolist()) == sorted(pool[~out].tolist())
        assert sh.step == 1 and conf_of(sh) == conf
        sh.sync()


@pytest.mark.parametrize("kind", ["adagrad", "ftrl"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_an_erased_key_comes_back_as_a_new_key(cuda, kind, dev):
    """One step with the same gradient row for an erased key and for a key never
    seen: the same p and the same state, bit for bit; survivors step on."""
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-reinsert", kind, dev))
    w, dtype = 4, np.float32
    pool = su.key_pool(rng, 300)
    old, fresh = pool[:200], pool[200:]
    hp = hyper_of(kind, False, wd=0.01)
    ns = n_slots(hp)
    g = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
    with ps.Shard.sparse(512, dtype, "assign", width=w) as sh, ps.Shard.sparse(512, dtype, "assign", width=w) as ref:
        for s in (sh, ref):
            set_opt(s, hp)
        v, g1, g2 = g(200), g(200), g(200)
        for s in (sh, ref):
            s.add(old, v)
            s.apply(old, g1)
        sh.erase(tdev(old[:100], cuda) if dev else old[:100])
        assert info(sh)[1] == 100
        # erased keys [0, 100) and never-seen keys get the same rows; survivors [100, 200) their own
        keys = np.concatenate([old[:100], fresh, old[100:]])
        grads = np.concatenate([g2[:100], g2[:100], g2[100:]])
        push(sh, "device" if dev else "host", keys, grads, cuda, method="apply")
        same(snapshot(sh, old[:100], ns), snapshot(sh, fresh, ns), "an erased key against a never-seen key")
        # the survivors equal a shard that never erased: the same second step from the same state
        ref.apply(old, g2)
        same(snapshot(ref, old[100:], ns), snapshot(sh, old[100:], ns), "survivors against a shard without the erase")
        assert not np.array_equal(snapshot(ref, old[:100], ns)[0], snapshot(sh, old[:100], ns)[0])  # (it did start over)
        assert sh.step == 2 and info(sh)[1] == 300
        sh.sync()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_at_a_full_shard_erasing_seven_keys_makes_room_for_exactly_seven(cuda, dev):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-room", dev))
    w, dtype = 3, np.float32
    pool = su.key_pool(rng, 109)
    vals = ou.dyadic_grads(rng, 109, w, dtype) + dtype(50)
    with ps.Shard.sparse(100, dtype, "assign", width=w) as sh:
        sh.add(pool[:100], vals[:100])
        sh.add(pool[100:101], vals[100:101])  # full: dropped
        full_error(ps, sh)
        gone = pool[10:17]
        sh.erase(tdev(gone, cuda) if dev else gone)
        sh.sync()  # erase clears the full condition
        assert info(sh) == (100, 93, 256)
        push(sh, "device" if dev else "host", pool[101:109], vals[101:109], cuda)  # eight new keys, room for seven
        full_error(ps, sh)
        held = sh.keys()
        assert info(sh)[1] == 100 and np.isin(pool[101:109], held).sum() == 7 and not np.isin(gone, held).any()
        keep = np.isin(pool, held)
        assert np.array_equal(bits(rows(sh, pool[keep])), bits(vals[keep])) and not rows(sh, pool[~keep]).any()


# ------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("kind", ["adam", "ftrl"])
def test_state_dict_round_trip_after_growth_and_erase(cuda, kind):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("grow-ckpt", kind))
    w, dtype = 5, np.float32
    pool = su.key_pool(rng, 700)
    hp = hyper_of(kind, False)
    ns = n_slots(hp)
    g = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
    with ps.Shard.sparse(8, dtype, "assign", width=w, max_capacity=1000) as a, \
            ps.Shard.sparse(8, dtype, "assign", width=w, max_capacity=1000) as b, \
            ps.Shard.sparse(8, dtype, "assign", width=w) as fixed:
        for s in (a, b, fixed):
            set_opt(s, hp)
        a.apply(pool[:600], g(600))
        a.apply(tdev(pool[100:], cuda), tdev(g(600), cuda))
        a.erase(pool[50:250])
        d = a.state_dict()
        assert sorted(d["keys"].tolist()) == sorted(np.concatenate([pool[:50], pool[250:]]).tolist()) and d["t"] == 2
        b.load_state_dict(d)
        # one reserve sized by the checkpoint, then its writing calls under the rule:
        # the Add fits, each put_state brings 500 positions to 500 stored keys
        cm = gu.CapacityModel(8, 1000)
        cm.reserve(500)
        for _ in range(1 + ns):
            cm.write(d["keys"])
        assert info(b)[:2] == (cm.capacity, 500) and b.growth()["rebuilds"] == cm.rebuilds == 2 and b.step == 2
        same(snapshot(a, pool, ns), snapshot(b, pool, ns), "restored")
        k = pool[rng.permutation(700)[:650]]
        gr = g(650)
        a.apply(k, gr)
        b.apply(tdev(k, cuda), tdev(gr, cuda))
        same(snapshot(a, pool, ns), snapshot(b, pool, ns), "the next step, on stored, erased and new keys")
        fixed.load_state_dict(d)  # growth off and too small: the keys that find no room are dropped, as before
        full_error(ps, fixed)
        assert info(fixed)[:2] == (8, 8)
        a.sync()
        b.sync()


def test_cpp_sparse_grow_program(cuda):
    """tests/cpp/hip_storage_sparse_grow_test.cpp: CreateTable's sparse_max_capacity,
    HipStorage::Reserve / SetGrowth / Erase against a std::map."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_sparse_grow_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
