"""GPU tests of sparse shards (pskv_shard_create_sparse; include/pskv.h "Sparse
shards").

The bar is the relabelling statement: a sparse shard fed keys K returns what a
dense row shard [0, capacity) returns when fed rank(K).  So
  * assign Adds are bit-exact against RowOracle on the raw keys (its
    MapStorageRef takes any key), accumulate Adds within RowOracle's bound on
    ranks (int32 exact);
  * a sparse shard and a dense twin that get the same calls with distinct keys
    per call agree bit for bit in every reply, in p, in every state slot and in
    the step counter (sparse_util.Twin), for every optimizer kind;
  * with duplicated keys every step of either shard passes the one-step check
    of opt_util / ftrl_util from the shard's own state before the step;
  * an absent key reads zeros and is never inserted by a reading call; a key
    that finds no slot is dropped whole and pskv_sync says so.
Keys come from the whole uint32 space and always hold 0, 2^31 and 0xFFFFFFFF
(sparse_util.key_pool); capacity 8 gives a 16-entry index, where collisions,
long probes and wrap-around are certain.
"""
import os
import subprocess

import numpy as np
import pytest

import ftrl_util as fu
import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
import sparse_util as su
from rows_util import RowOracle, ValueSource, bits
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSKV_ESTATE = -4
KINDS = [("sgd", False), ("adagrad", False), ("momentum", False), ("momentum", True), ("adam", False), ("ftrl", False)]
KIND_IDS = ["sgd", "adagrad", "momentum", "nesterov", "adam", "ftrl"]


def ps_mod():
    """(imported inside the tests: torch's HIP runtime loads first, through the `cuda` fixture)"""
    import parameter_server_amd as ps

    return ps


def hyper_of(kind, nesterov, wd=0.01):
    return fu.hyper(wd=wd) if kind == "ftrl" else ppu.hyper(kind, nesterov, wd)


def set_opt(sh, hp):
    if hp["kind"] == "ftrl":
        fu.set_optimizer(sh, hp)
    else:
        ppu.set_optimizer(sh, hp)


def n_slots(hp):
    return 2 if hp["kind"] == "ftrl" else ou.SLOTS[hp["kind"]]


def start_slots(hp, shape, dt):
    return fu.initial_slots(shape, dt, hp) if hp["kind"] == "ftrl" else ppu.initial_slots(hp["kind"], shape, dt)


def rows(sh, keys, cuda=None, slot=None):
    """The rows of `keys` (p, or state slot `slot`), host or device path, as (n, W)."""
    keys = np.asarray(keys, dtype=np.uint32)
    k = tdev(keys, cuda) if cuda is not None else keys
    got = sh.get(k) if slot is None else sh.get_state(k, slot=slot)
    got = got.cpu().numpy() if cuda is not None else np.asarray(got)
    return got.reshape(keys.size, sh.width)


def split(keys, vals, parts):
    """(keys, vals) cut into `parts` batches with an empty one in front."""
    cuts = np.linspace(0, keys.size, parts + 1).astype(int)
    out = [(keys[:0], vals[:0])]
    return out + [(keys[a:b], vals[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def push(sh, path, keys, vals, cuda, method="add"):
    """One writing call through one of the entry points."""
    grouped = {"add": "add_grouped", "apply": "apply_grouped"}[method]
    if path == "host":
        getattr(sh, method)(keys, vals)
    elif path == "device":
        getattr(sh, method)(tdev(keys, cuda), tdev(vals, cuda))
    elif path == "host_grouped":
        getattr(sh, grouped)(split(keys, vals, 3))
    elif path == "device_grouped":
        getattr(sh, grouped)([(tdev(k, cuda), tdev(v, cuda)) for k, v in split(keys, vals, 2)])
    else:
        raise ValueError(path)


PATHS = ["host", "device", "host_grouped", "device_grouped"]
# (n, width, capacity, distinct keys in play): the 2048-key chunk boundary, more
# than one virtual workgroup, every width class (1, odd, 16-byte rows, > 64-lane
# rows), a full 16-entry index and a shard filled exactly to its capacity
SHAPES = [(1, 1, 8, 1), (255, 3, 8, 8), (2047, 4, 100, 100), (2049, 16, 8192, 2049), (4100, 33, 8192, 4100),
          (2049, 1, 8192, 700), (4100, 4, 8192, 3000)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32], ids=["f32", "f64", "i32"])
@pytest.mark.parametrize("n,w,cap,m", SHAPES)
def test_assign_every_path_against_the_map_oracle(oracle_mod, cuda, n, w, cap, m, dtype):
    import torch

    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("sparse-assign", n, w, cap, np.dtype(dtype).name))
    pool = su.key_pool(rng, m)
    gone = su.absent_keys(rng, pool, 40)
    orc = RowOracle(oracle_mod, dtype, "assign", w, 0, 1 << 32)
    src = ValueSource(dtype, "assign", rng)
    stored = set()
    with ps.Shard.sparse(cap, dtype, "assign", width=w) as sh:
        assert sh.sparse_info() == {"capacity": cap, "count": 0, "table_slots": max(16, 1 << (2 * cap - 1).bit_length()),
                                    "index_bytes": max(16, 1 << (2 * cap - 1).bit_length()) * 8 + cap * 4}
        for i, (name, keys) in enumerate(su.pool_patterns(rng, n, pool).items()):
            vals = src.rows(n, w)
            push(sh, PATHS[i % 4], keys, vals, cuda)
            orc.add(keys, vals)
            stored |= set(int(k) for k in keys)
            q = np.concatenate([pool, gone, keys[: 50]])
            rng.shuffle(q)
            orc.check(q, rows(sh, q, cuda if i % 2 else None), f"{name} via {PATHS[i % 4]}")
            assert sh.sparse_info()["count"] == len(stored), name  # the Get of absent keys inserted none
        # add_get_grouped, host and device: the Get half sees the Add half and inserts nothing
        for dev in (False, True):
            keys = pool[rng.integers(0, m, size=min(n, 300))]
            vals = src.rows(keys.size, w)
            q = np.concatenate([gone[:7], keys[::-1]])
            if dev:
                out = torch.empty((q.size, w) if w > 1 else q.size, dtype=tdev(vals, cuda).dtype, device=cuda)
                sh.add_get_grouped([(tdev(keys, cuda), tdev(vals, cuda))], [(tdev(q, cuda), out)])
                got = out.cpu().numpy()
            else:
                got = np.empty((q.size, w) if w > 1 else q.size, dtype=dtype)
                sh.add_get_grouped([(keys, vals)], [(q, got)])
            orc.add(keys, vals)
            stored |= set(int(k) for k in keys)
            orc.check(q, got, f"add_get_grouped device={dev}")
        # pooled pulls of stored and absent keys: zeros for the absent, no error, no insert
        off = pu.offsets_of([3, 0, gone.size, 2])
        pk = np.concatenate([pool[[0, -1, m // 2]], gone, pool[[0, 0]]])
        p_rows = orc.expect(pk)
        want = pu.reference(p_rows, 0, np.arange(pk.size, dtype=np.uint32), off, None)
        for c in (None, cuda):
            pu.check(pu.pooled(sh, pk, off, None, c), want, f"pooled pull device={c is not None}")
        sh.sync()  # no sticky error: absent keys are legal in every reading call
        assert sh.sparse_info()["count"] == len(stored)
        assert sorted(int(k) for k in sh.keys()) == sorted(stored)
        info = sh.info()
        assert (info["key_begin"], info["key_end"], info["overflow_count"], info["resident_bytes"]) == (0, 1 << 32, 0, 0)
        assert info["dense_bytes"] == (cap + 1) * w * np.dtype(dtype).itemsize and info["width"] == w
        # clear: an empty index, zero rows
        sh.clear()
        assert sh.sparse_info()["count"] == 0 and sh.keys().size == 0
        assert not rows(sh, pool).any()
        sh.sync()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32], ids=["f32", "f64", "i32"])
@pytest.mark.parametrize("n,w,cap,m", SHAPES)
def test_accumulate_within_the_row_oracle_bound(oracle_mod, cuda, n, w, cap, m, dtype):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("sparse-acc", n, w, cap, np.dtype(dtype).name))
    pool = su.key_pool(rng, m)
    rl = su.Relabel(pool)
    gone = su.absent_keys(rng, pool, 10)
    orc = RowOracle(oracle_mod, dtype, "accumulate", w, 0, m)
    src = ValueSource(dtype, "accumulate", rng)
    with ps.Shard.sparse(cap, dtype, "accumulate", width=w) as sh:
        for i, (name, keys) in enumerate(su.pool_patterns(rng, n, pool).items()):
            vals = src.rows(n, w)
            push(sh, PATHS[(i + 1) % 4], keys, vals, cuda)
            orc.add(rl.rank(keys), vals)
            orc.check(rl.rank(pool), rows(sh, pool, cuda if i % 2 == 0 else None), f"{name} via {PATHS[(i + 1) % 4]}")
            assert not rows(sh, gone).any(), name
        sh.sync()


def test_one_new_key_in_two_chunks_and_in_two_batches_gets_one_slot(cuda):
    ps = ps_mod()
    rng = np.random.default_rng(3)
    pool = su.key_pool(rng, 4100)
    w = 4
    for dev in (False, True):
        with ps.Shard.sparse(8192, np.float32, "assign", width=w) as sh:
            # position 5 and position 2048 + 5 of one call: two virtual workgroups race for the key
            keys = pool[:4100].copy()
            keys[2053] = keys[5]
            keys[4099] = keys[5]
            vals = ValueSource(np.float32, "assign", rng).rows(keys.size, w)
            push(sh, "device" if dev else "host", keys, vals, cuda)
            assert sh.sparse_info()["count"] == np.unique(keys).size
            assert sorted(sh.keys().tolist()) == sorted(np.unique(keys).tolist())
            assert np.array_equal(bits(rows(sh, keys[[5]])), bits(vals[[4099]]))  # the last occurrence won, whole
        with ps.Shard.sparse(100, np.float32, "assign", width=w) as sh:
            # the same new key in two batches of a grouped call (and twice in one of them)
            a, b = pool[:30].copy(), pool[20:60].copy()
            b[7] = a[3]
            b[39] = a[3]
            va, vb = (ValueSource(np.float32, "assign", rng).rows(x.size, w) for x in (a, b))
            if dev:
                sh.add_grouped([(tdev(a, cuda), tdev(va, cuda)), (tdev(b, cuda), tdev(vb, cuda))])
            else:
                sh.add_grouped([(a, va), (b, vb)])
            distinct = np.unique(np.concatenate([a, b]))
            assert sh.sparse_info()["count"] == distinct.size
            assert sorted(sh.keys().tolist()) == sorted(distinct.tolist())
            sh.sync()


def _distinct(rng, pool, n):
    return pool[rng.permutation(pool.size)[:n]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,nesterov", KINDS, ids=KIND_IDS)
def test_twin_shards_agree_bit_for_bit_with_distinct_keys(cuda, kind, nesterov, dtype):
    """Add / apply / apply_grouped / apply_pooled / apply_pooled_grouped /
    get_pooled / put_state / get_state, host and device, distinct keys per
    call: every reply and the final p and state are identical."""
    ps = ps_mod()
    ki = KIND_IDS.index("nesterov" if nesterov else kind)
    w = [1, 3, 4, 16, 33, 4][ki]
    rng = np.random.default_rng(ou.case_seed("sparse-twin", kind, nesterov, np.dtype(dtype).name))
    pool = su.key_pool(rng, 3000)
    rl = su.Relabel(pool)
    hp = hyper_of(kind, nesterov)
    tw = su.Twin(ps, 4096 if ki % 2 else 3000, dtype, "assign", w, rl, cuda)
    try:
        tw.each(lambda sh, f: set_opt(sh, hp))
        g = lambda n: (rng.standard_normal((n, w)) * 3).astype(dtype)  # noqa: E731
        # the first 2049 keys by an Add, the other 951 by their first optimizer
        # step: from there on every key of the scenario is stored (a key that is
        # not reads zeros from a state array, where the dense twin's untouched
        # row holds the start value)
        tw.write("add", pool[:2049], g(2049), dev=False)
        tw.read("get", pool[:2049:4], dev=True, what="get after add")
        tw.write("apply", pool[951:], g(2049), dev=True)
        k = _distinct(rng, pool, 255)
        tw.write("apply", k, g(k.size), dev=False)
        k = _distinct(rng, pool, 2500)
        tw.write_grouped("apply_grouped", [(k[:1], g(1)), (k[1:2100], g(2099)), (k[2100:], g(400))], dev=True)
        tw.write_grouped("apply_grouped", [(k[:300], g(300)), (k[300:301], g(1))], dev=False)
        tw.read("get", pool, dev=False, what="get after steps")
        for dev, weighted, bagpat, n in ((False, True, "mixed", 2049), (True, False, "boundary", 2500),
                                         (True, True, "eights", 255), (False, False, "one_bag", 1)):
            k = _distinct(rng, pool, n)
            off = pu.offsets_of(ppu.bag_lens(bagpat, n))
            bg = (rng.standard_normal((off.size - 1, w)) * 3).astype(dtype)
            tw.apply_pooled(k, off, bg, rng.standard_normal(n).astype(dtype) if weighted else None, dev=dev)
        for dev in (True, False):
            k = _distinct(rng, pool, 2600)
            batches = []
            for a, b, weighted in ((0, 2100, True), (2100, 2101, False), (2101, 2600, dev)):
                off = pu.offsets_of(ppu.bag_lens("eights", b - a))
                bg = (rng.standard_normal((off.size - 1, w)) * 3).astype(dtype)
                batches.append((k[a:b], off, bg) + ((rng.standard_normal(b - a).astype(dtype),) if weighted else ()))
            tw.apply_pooled_grouped(batches, dev=dev)
        # pooled pulls may repeat keys: a bag's additions run in an order fixed by its length
        for dev in (False, True):
            lens = [1, 0, 5, 300, 17, 2]
            pk = pool[rng.integers(0, pool.size, size=sum(lens))]
            tw.get_pooled(pk, pu.offsets_of(lens), rng.standard_normal(pk.size).astype(dtype) if dev else None, dev=dev)
        for slot in range(n_slots(hp)):
            k = _distinct(rng, pool, 700)
            tw.write("put_state", k, np.abs(g(k.size)), dev=bool(slot), slot=slot)
            tw.read("get_state", pool[:900], dev=not slot, what=f"get_state {slot}", slot=slot)
        k = _distinct(rng, pool, 2049)
        tw.write("apply", k, g(k.size), dev=True)
        tw.check_all(n_slots(hp))
        assert tw.sp.step == 11
        assert tw.sp.sparse_info()["count"] <= pool.size
    finally:
        tw.close()


def one_step_check(sh, rl, hp, before, call, msg):
    """The one-step check of opt_util / ftrl_util from the shard's own state:
    `before` = (p, slots) of rl.uniq read before the step, call = ("rows", keys,
    grads) or ("pooled", keys, offsets, bag_grads, weights)."""
    keymap = (lambda k: k) if sh.is_sparse else rl.rank
    p, slots = before
    p_got = rows(sh, keymap(rl.uniq))
    s_got = [rows(sh, keymap(rl.uniq), slot=i) for i in range(len(slots))]
    idx = rl.rank(call[1]).astype(np.int64)
    if hp["kind"] == "ftrl":
        assert call[0] == "rows"
        fu.check_step(p, slots, idx, call[2], p_got, s_got, sh.dtype, hp, msg=msg)
    elif call[0] == "rows":
        ou.check_step(p, slots, idx, call[2], p_got, s_got, sh.dtype, hp, t=sh.step, msg=msg)
    else:
        _, _, off, bg, wts = call
        ppu.check_step(p, slots, idx, wts, bg, ppu.bag_index(off), p_got, s_got, sh.dtype, hp, t=sh.step, msg=msg)
    return p_got, s_got


@pytest.mark.parametrize("kind,nesterov", KINDS, ids=KIND_IDS)
def test_duplicated_keys_pass_the_one_step_check_on_both_twins(cuda, kind, nesterov):
    """Steps whose keys repeat leave the summation order open: the sparse shard
    and the dense twin each meet opt_util's / ftrl_util's tolerances from their
    own state, as tests/test_opt_gpu.py checks a dense shard."""
    ps = ps_mod()
    ki = KIND_IDS.index("nesterov" if nesterov else kind)
    w, dtype = [4, 1, 3, 16, 33, 4][ki], [np.float32, np.float64][ki % 2]
    rng = np.random.default_rng(ou.case_seed("sparse-dups", kind, nesterov))
    pool = su.key_pool(rng, 600)
    rl = su.Relabel(pool)
    hp = hyper_of(kind, nesterov, wd=0.0 if ki % 2 else 0.01)
    tw = su.Twin(ps, 1024, dtype, "assign", w, rl, cuda)
    try:
        tw.each(lambda sh, f: set_opt(sh, hp))
        tw.write("add", pool, rng.standard_normal((pool.size, w)).astype(dtype))
        for sh, f in tw.shards:
            state = (rows(sh, f(rl.uniq)), [rows(sh, f(rl.uniq), slot=i) for i in range(n_slots(hp))])
            for i, (name, keys) in enumerate(su.pool_patterns(rng, 2049, pool).items()):
                if name == "all_equal":
                    keys = keys[:2]  # (opt_util.BOUND_SHAPES: thousands of one key leave the bound no teeth)
                grads = (rng.standard_normal((keys.size, w)) * 3).astype(dtype)
                push(sh, PATHS[i % 4], f(keys), grads, cuda, method="apply")
                state = one_step_check(sh, rl, hp, state, ("rows", keys, grads), f"{name} sparse={sh.is_sparse}")
            if kind != "ftrl":
                for dev in (False, True):
                    keys, off, bg, wts = ppu.draw_call(rng, 2049, w, "dups_across_chunks", "mixed", 0, pool.size, dtype,
                                                       weighted=dev)
                    keys = pool[keys]
                    ppu.apply_pooled(sh, f(keys), off, bg, wts, cuda if dev else None)
                    state = one_step_check(sh, rl, hp, state, ("pooled", keys, off, bg, wts),
                                           f"pooled push device={dev} sparse={sh.is_sparse}")
            sh.sync()
        assert tw.sp.step == tw.dn.step
    finally:
        tw.close()


@pytest.mark.parametrize("kind", ["adagrad", "ftrl"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_a_new_keys_first_step_starts_from_zeros_and_the_start_state(cuda, kind, dev):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("sparse-first", kind, dev))
    w, dtype = 3, np.float32
    pool = su.key_pool(rng, 300)
    rl = su.Relabel(pool)
    hp = hyper_of(kind, False, wd=0.0)
    assert (hp["init_accum"] if kind == "ftrl" else ou.BOUND_INIT_ACCUM) > 0
    with ps.Shard.sparse(512, dtype, "assign", width=w) as sh:
        set_opt(sh, hp)
        # nothing stored: the state every key will start from, as the oracles hold it
        state = (np.zeros((rl.m, w), dtype=dtype), start_slots(hp, (rl.m, w), dtype))
        for step in range(2):  # the second step meets old and new keys side by side
            keys = _distinct(rng, pool, 150)
            grads = (rng.standard_normal((150, w)) * 3).astype(dtype)
            push(sh, "device" if dev else "host", keys, grads, cuda, method="apply")
            # keys not stored yet read zeros from every array; the oracle holds
            # their start state instead, so compare what is stored
            have = np.isin(rl.uniq, sh.keys())
            got = one_step_check_stored(sh, rl, hp, state, keys, grads, have, f"step {step}")
            state = got
        sh.sync()


def one_step_check_stored(sh, rl, hp, before, keys, grads, have, msg):
    """one_step_check where keys not stored so far still hold the start state in
    the oracle's view: what the shard returns for them (zeros) is replaced by it."""
    p, slots = before
    start = start_slots(hp, p.shape, sh.dtype)
    p_got = rows(sh, rl.uniq)
    s_got = [rows(sh, rl.uniq, slot=i) for i in range(len(slots))]
    assert not p_got[~have].any() and not any(s[~have].any() for s in s_got), f"{msg}: an absent key reads non-zero"
    for s, s0 in zip(s_got, start):
        s[~have] = s0[~have]
    idx = rl.rank(keys).astype(np.int64)
    if hp["kind"] == "ftrl":
        fu.check_step(p, slots, idx, grads, p_got, s_got, sh.dtype, hp, msg=msg)
    else:
        ou.check_step(p, slots, idx, grads, p_got, s_got, sh.dtype, hp, t=sh.step, msg=msg)
    return p_got, s_got


@pytest.mark.parametrize("path", ["device_add", "host_add", "device_apply", "host_apply", "device_pooled"])
def test_full_shard_drops_new_keys_whole_and_says_so(cuda, path):
    """Capacity 100 holding 60 keys; one call of those 60 plus 150 new distinct keys."""
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("sparse-full", path))
    w, dtype, lr = 4, np.float32, 2.0**-3
    pool = su.key_pool(rng, 210)
    old, new = pool[:60], pool[60:]
    with ps.Shard.sparse(100, dtype, "assign", width=w) as sh:
        if "add" not in path:
            sh.set_optimizer("sgd", lr=lr)
        p_old = ou.dyadic_params(rng, 60, w, dtype)
        sh.add(old, p_old)
        sh.sync()
        keys = pool[rng.permutation(210)]
        vals = ou.dyadic_grads(rng, 210, w, dtype) + dtype(100)  # never a zero row
        kd, vd = tdev(keys, cuda), tdev(vals, cuda)
        if path == "device_add":
            sh.add(kd, vd)
        elif path == "host_add":
            sh.add(keys, vals)
        elif path == "device_apply":
            sh.apply(kd, vd)
        elif path == "host_apply":
            sh.apply(keys, vals)
        else:
            sh.apply_pooled(kd, tdev(np.arange(211, dtype=np.int64), cuda), vd)  # one key per bag
        with pytest.raises(ps.PskvError) as e:
            sh.sync()
        assert e.value.code == PSKV_ESTATE and "sparse shard full" in str(e.value)
        assert sh.sparse_info()["count"] == 100
        if "add" not in path:
            assert sh.step == 1  # the step counter advances as for a device call that drops keys
        held = sh.keys()
        assert held.size == 100 and np.isin(old, held).all()  # keys already stored are always served
        # what the oracle expects of a key that got in: the row pushed (assign), or one exact SGD step
        at = {int(k): i for i, k in enumerate(keys)}
        start = np.zeros((210, w), dtype=dtype)
        start[[at[int(k)] for k in old]] = p_old
        want = vals if "add" in path else start - dtype(lr) * vals
        got = rows(sh, keys, cuda)
        inside = np.isin(keys, held)
        assert inside.sum() == 100
        assert np.array_equal(bits(got[inside]), bits(want[inside])), "a stored key holds another row than the oracle's"
        assert not got[~inside].any(), "a dropped key reads a partial or non-zero row"
        # the error is sticky until clear, which empties the shard
        with pytest.raises(ps.PskvError):
            sh.sync()
        sh.clear()
        sh.sync()
        assert sh.sparse_info()["count"] == 0 and sh.step == 0
        sh.add(new[:100], vals[:100])  # and all 100 slots are free again
        sh.sync()
        assert sh.sparse_info()["count"] == 100


@pytest.mark.parametrize("kind", ["adam", "ftrl"])
def test_state_dict_restores_a_sparse_shard_bit_for_bit(cuda, kind):
    ps = ps_mod()
    rng = np.random.default_rng(ou.case_seed("sparse-ckpt", kind))
    w, dtype = 5, np.float32
    pool = su.key_pool(rng, 700)
    hp = hyper_of(kind, False)
    with ps.Shard.sparse(1024, dtype, "assign", width=w) as a, ps.Shard.sparse(1024, dtype, "assign", width=w) as b:
        set_opt(a, hp)
        set_opt(b, hp)
        a.add(pool[:300], rng.standard_normal((300, w)).astype(dtype))
        for _ in range(3):
            k = pool[rng.integers(0, 500, size=400)]
            a.apply(tdev(k, cuda), tdev((rng.standard_normal((400, w)) * 3).astype(dtype), cuda))
        d = a.state_dict()
        assert sorted(d["keys"].tolist()) == sorted(a.keys().tolist()) and d["t"] == 3
        assert d["p"].shape == (d["keys"].size, w) and len(d["slots"]) == 2
        b.load_state_dict(d)
        assert b.step == 3 and sorted(b.keys().tolist()) == sorted(a.keys().tolist())
        # the next step, on stored and on new keys (distinct: the result is specified bit for bit)
        k = _distinct(rng, pool, 600)
        g = (rng.standard_normal((600, w)) * 3).astype(dtype)
        a.apply(k, g)
        b.apply(tdev(k, cuda), tdev(g, cuda))
        assert np.array_equal(bits(rows(a, pool)), bits(rows(b, pool)))
        for slot in range(2):
            assert np.array_equal(bits(rows(a, pool, slot=slot)), bits(rows(b, pool, slot=slot)))
        assert a.step == b.step == 4
        with pytest.raises(ValueError):
            b.load_state_dict({k2: v for k2, v in d.items() if k2 != "keys"})
        a.sync()
        b.sync()


def test_index_time_counts_one_operation_per_call_and_its_keys(cuda):
    ps = ps_mod()
    rng = np.random.default_rng(9)
    pool = su.key_pool(rng, 5000)
    w = 4
    with ps.Shard.sparse(8192, np.float32, "assign", width=w) as sh:
        sh.set_optimizer("sgd", lr=0.1)
        sh.set_timing(True)
        v = lambda n: rng.standard_normal((n, w)).astype(np.float32)  # noqa: E731
        assert sh.index_time() == {"launches": 0, "total_ms": 0.0, "elements": 0}
        sh.add(tdev(pool[:3000], cuda), tdev(v(3000), cuda))
        t = sh.index_time()
        assert (t["launches"], t["elements"]) == (1, 3000) and t["total_ms"] > 0
        sh.get(pool[:700])
        sh.add_grouped([(pool[:10], v(10)), (pool[4000:4100], v(100))])
        sh.apply(tdev(pool[:2500], cuda), tdev(v(2500), cuda))
        pu.pooled(sh, pool[:40], pu.offsets_of([40]), None, cuda)
        sh.get(pool[:0])  # no key: no operation
        t = sh.index_time()
        assert (t["launches"], t["elements"]) == (5, 3000 + 700 + 110 + 2500 + 40)
        assert sh.apply_time()["launches"] == 1  # the step's own slot is untouched by the index
        sh.reset_timing()
        assert sh.index_time()["launches"] == 0
        sh.set_timing(False)
        sh.get(pool[:5])
        assert sh.index_time()["launches"] == 0
        sh.sync()


def test_flags_options_and_views(cuda):
    ps = ps_mod()
    rng = np.random.default_rng(2)
    pool = su.key_pool(rng, 50)
    with ps.Shard.sparse(64, np.float64, "assign", width=2, options={"RESIDENT_BYTES": 1 << 20, "NT": 0}) as sh:
        assert sh.get_option("RESIDENT_BYTES") == 1 << 20 and sh.get_option("NT") == 0  # accepted and echoed
        assert sh.info()["resident_bytes"] == 0
        v = rng.standard_normal((50, 2))
        order = np.argsort(pool)
        sh.add(tdev(pool[order], cuda), tdev(v[order], cuda), sorted_hint=True)  # accepted, changes nothing
        assert np.array_equal(rows(sh, pool), v)
        frame = ps.HostFrame(50 * 4 + 64)
        try:
            fk = frame.array(np.uint32, 50)
            fk[:] = pool
            assert np.array_equal(np.asarray(sh.get(fk, frame=True)).reshape(50, 2), v)  # plain host memory to the shard
        finally:
            frame.free()
        assert sh.dense_ptr() != 0
        with pytest.raises(ValueError):
            sh.dense_view()
        sh.sync()
    with ps.Shard(capacity=16, dtype=np.int32) as sh:  # the constructor form; width 1 runs on the row kernels
        assert sh.is_sparse and sh.width == 1
        sh.add(np.array([7, 0xFFFFFFFF, 7], dtype=np.uint32), np.array([1, 2, 3], dtype=np.int32))
        assert sh.get(np.array([0xFFFFFFFF, 7, 8], dtype=np.uint32)).tolist() == [2, 3, 0]
        assert sh.sparse_info()["count"] == 2
    with ps.Shard(0, 100, np.float32) as dense:
        with pytest.raises(ps.PskvError):
            dense.sparse_info()
    st = ps.HipStorage(np.float32, capacity=32, width=2)  # the Python storage, as a consistency model holds it
    try:
        st.SubAdd(np.array([5, 4000000000], dtype=np.uint32), np.array([1, 2, 3, 4], dtype=np.float32))
        got = ps.typed(st.SubGet(np.array([4000000000, 6, 5], dtype=np.uint32)), np.float32)
        assert got.tolist() == [3, 4, 0, 0, 1, 2] and st.shard.sparse_info()["count"] == 2
        st.FinishIter()
    finally:
        st.shard.close()


@pytest.mark.parametrize("dtype,w", [(np.float32, 3), (np.float64, 4)], ids=["f32-w3", "f64-w4"])
def test_a_dense_row_shards_host_grouped_pooled_push_names_the_callers_batch(cuda, dtype, w):
    """The dense side of the pooled front that sparse shards share: caller batch
    0 is empty, so the refused key lies in live batch 0 and the message must
    still say batch 1; nothing is applied and the step is not counted.  A sparse
    shard takes the same call (it owns every key)."""
    import pooled_push_group_util as ggu

    ps, hp = ps_mod(), ppu.hyper("sgd")
    rng = np.random.default_rng(ou.case_seed("front-refusal", np.dtype(dtype).name, w))
    keys = np.array([1001, 1005, 3007, 1002, 1001], dtype=np.uint32)  # 3007 is outside; 1001 lies in both bags
    batches = [ggu.empty_batch(w, dtype, nbags=1),
               (keys, pu.offsets_of([2, 3]), (rng.standard_normal((2, w)) * 3).astype(dtype), None)]
    with ps.Shard(1000, 1040, dtype, width=w) as sh:
        ppu.set_optimizer(sh, hp)
        with pytest.raises(ps.PskvError) as e:
            sh.apply_pooled_grouped(batches)
        assert str(e.value) == ("pskv error -1: pskv_apply_pooled_grouped: batch 1: key 3007 is outside [key_begin, "
                                "key_end); an optimizer step takes no out-of-range keys (nothing was applied)")
        assert sh.step == 0 and not rows(sh, np.arange(1000, 1040)).any()
        sh.sync()
    with ps.Shard.sparse(8, dtype, "assign", width=w) as sh:
        ppu.set_optimizer(sh, hp)
        sh.apply_pooled_grouped(batches)
        assert sh.step == 1 and sorted(sh.keys().tolist()) == [1001, 1002, 1005, 3007]
        ggu.check_step(np.zeros((4, w), dtype=dtype), [], 0, [(su.Relabel(keys).rank(keys),) + batches[1][1:]],
                       rows(sh, np.unique(keys)), [], np.dtype(dtype), hp, t=1, msg="sparse grouped push")
        sh.sync()


def test_cpp_sparse_program(cuda):
    """tests/cpp/hip_storage_sparse_test.cpp: HipStorage::Sparse and CreateTable's
    sparse_capacity, two servers under jump hashing."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_sparse_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
