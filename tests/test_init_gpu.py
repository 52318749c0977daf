"""GPU tests of row initializers (Shard.set_initializer, Shard.init_rows; the
kernels of pskv_init.hip) against the numpy restatement of tests/init_util.py:
evaluation, insertion into sparse shards by every writing call, lifecycle."""
import numpy as np
import pytest

import init_util as iu
from rows_util import U_ROUND, bits
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

EDGE_KEYS = [0, 1, 7, 2**31, 0xFFFFFFFF]
UNI = dict(kind="uniform", a=-0.5, b=0.25, seed=0x1234567_89ABCDEF)  # bit-exact: the twins' rule
CAP = 4096


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def dev(x, cuda):
    if cuda is None or x is None:
        return x
    return tdev(x.astype(np.int64) if x.dtype == np.uint64 else x, cuda)


def same_bits(a, b, msg):
    a, b = bits(host(a)).reshape(-1), bits(host(b)).reshape(-1)
    assert np.array_equal(a, b), f"{msg}: {int((a != b).sum())} of {a.size} elements differ"


def ref_rows(keys, w, dt):
    return iu.init_ref(keys, w, dt, UNI["kind"], UNI["a"], UNI["b"], UNI["seed"])[0]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dt,w", [(np.float32, w) for w in (1, 3, 4, 5, 16, 33, 1024)] +
                         [(np.float64, w) for w in (1, 3, 4, 5, 16, 33, 260, 1024)])
def test_init_rows_equal_the_reference(cuda, dt, w, device):
    import parameter_server_amd as ps

    dt = np.dtype(dt)
    rng = np.random.default_rng(w)
    keys = np.concatenate([EDGE_KEYS, rng.integers(0, 1 << 32, 40)]).astype(np.uint32)
    with ps.Shard.sparse(64, dt, width=w) as sh:
        assert (bits(sh.init_rows(keys)) == 0).all() and sh.initializer()["kind"] == "zero"
        for kind, a, b, seed in [("constant", 0.01, 0.0, 0), ("uniform", -0.5, 0.25, 7), ("uniform", 3.0, 3.0, 7),
                                 ("normal", 0.25, 2.0, (1 << 63) + 5), ("normal", -1.0, 0.0, 1)]:
            sh.set_initializer(kind, a, b, seed)
            assert sh.initializer() == {"kind": kind, "a": a, "b": b, "seed": seed}
            got = host(sh.init_rows(dev(keys, cuda if device else None))).reshape(keys.size, w)
            want, rad = iu.init_ref(keys, w, dt, kind, a, b, seed)
            if kind != "normal":
                same_bits(got, want, f"{kind} w={w}")
                continue
            tol = iu.C_NORMAL[dt] * U_ROUND[dt] * (abs(a) + abs(b) * rad)
            err = np.abs(got.astype(np.float64) - want)
            unit = U_ROUND[dt] * (abs(a) + abs(b) * rad)
            print(f"normal {dt.name} w={w} b={b}: largest err / (u_T (|a| + |b| rad)) = {(err / unit).max():.3f}")
            assert (err <= tol).all(), (err / unit).max()
        assert sh.init_rows(keys[:0]).size == 0 and sh.sparse_info()["count"] == 0


def draw_call(rng, how, keys, w, dt):
    """One writing call's data, drawn once and replayed on the shard and its twin."""
    n = keys.size
    if how in ("pooled", "fm"):
        off = np.unique(np.concatenate([[0, n], rng.integers(0, n, n // 4)])).astype(np.uint64)
        nb = off.size - 1
        return dict(off=off, wts=rng.standard_normal(n).astype(dt), bg=rng.standard_normal((nb, w)).astype(dt),
                    c=rng.standard_normal(nb).astype(dt))
    vals = rng.standard_normal((n, w)).astype(dt)
    first = {}
    for i, k in enumerate(keys.tolist()):  # a repeated key carries one row: any order of the adds gives the same bits
        vals[i] = vals[first.setdefault(k, i)]
    return dict(vals=vals)


def write(sh, how, keys, d, cuda):
    k = dev(keys, cuda)
    if how in ("assign", "accumulate"):
        sh.add(k, dev(d["vals"], cuda))
    elif how == "apply":
        sh.apply(k, dev(d["vals"], cuda))
    elif how == "put_state":
        sh.put_state(k, dev(d["vals"], cuda))
    elif how == "pooled":
        sh.apply_pooled(k, dev(d["off"], cuda), dev(d["bg"], cuda), dev(d["wts"], cuda))
    else:
        sh.apply_pooled_fm(k, dev(d["off"], cuda), dev(d["c"], cuda), dev(d["wts"], cuda))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w", [1, 5, 16])
@pytest.mark.parametrize("how", ["assign", "accumulate", "apply", "pooled", "fm", "put_state"])
def test_inserted_keys_start_as_init_like_the_row_shard_twin(cuda, how, w, device):
    """SGD (put_state needs a state array: Adagrad).  Call 1 inserts 257 keys,
    call 2 mixes them with 3000 new ones and a repeated key; the twin is a row
    shard over the keys' ranks whose rows were assigned the reference init."""
    import parameter_server_amd as ps

    dt = np.dtype(np.float32)
    rng = np.random.default_rng([w, int(device), sum(map(ord, how))])
    pool = np.unique(np.concatenate([EDGE_KEYS, rng.integers(0, 1 << 32, 3300)]).astype(np.uint32))[:3257]
    pool = rng.permutation(pool)
    rank = {int(k): i for i, k in enumerate(pool)}
    k1 = pool[:257]
    k2 = rng.permutation(np.concatenate([pool[100:], pool[300:301]]))
    # (a pooled push gives the repeated key's two positions different gradient rows: its row is left out)
    cmp = np.arange(pool.size) != 300 if how in ("pooled", "fm") else np.ones(pool.size, bool)
    mode = "accumulate" if how == "accumulate" else "assign"
    opt = "adagrad" if how == "put_state" else "sgd"
    path = cuda if device else None
    with ps.Shard.sparse(CAP, dt, mode, width=w, init=UNI) as sh, ps.Shard(0, pool.size, dt, mode, width=w) as twin:
        ranks = np.arange(pool.size, dtype=np.uint32)
        twin.add(ranks, ref_rows(pool, w, dt))
        for s in (sh, twin):
            s.set_optimizer(opt, lr=0.05)
        for keys in (k1, k2):
            d = draw_call(rng, how, keys, w, dt)
            write(sh, how, keys, d, path)
            write(twin, how, np.array([rank[int(k)] for k in keys], dtype=np.uint32), d, path)
        same_bits(sh.get(pool).reshape(-1, w)[cmp], twin.get(ranks).reshape(-1, w)[cmp], f"{how}: against the twin")
        if how == "put_state":
            same_bits(sh.get_state(pool), twin.get_state(ranks), "state against the twin")
            same_bits(sh.get(pool), ref_rows(pool, w, dt), "put_state leaves init in the parameters")
        else:  # call 1's keys that call 2 left alone keep their stepped rows
            moved = bits(sh.get(pool[:100])) != bits(ref_rows(pool[:100], w, dt))
            assert moved.any(axis=None), "the first call's rows are back at init"
        assert sh.sparse_info()["count"] == pool.size
        sh.sync()


@pytest.mark.parametrize("w", [1, 5, 16])
def test_fm_rows_leave_zero_only_with_an_initializer(cuda, w):
    import parameter_server_amd as ps

    dt = np.dtype(np.float32)
    keys = np.arange(1000, 1064, dtype=np.uint32)
    off = np.arange(0, 65, 4, dtype=np.uint64)
    c = np.ones(16, dtype=dt)
    for init, leaves in [(None, False), (UNI, True)]:
        with ps.Shard.sparse(CAP, dt, width=w, init=init) as sh:
            sh.set_optimizer("sgd", lr=0.05)
            sh.apply_pooled_fm(keys, off, c)
            got = sh.get(keys).reshape(64, w)
            start = ref_rows(keys, w, dt) if leaves else np.zeros((64, w), dt)
            assert (bits(got) != bits(start)).any() == leaves and ((got != 0).any() == leaves)


@pytest.mark.parametrize("w", [1, 5, 16])
def test_lifecycle_erase_reserve_full_and_zero(cuda, w):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    dt = np.dtype(np.float32)
    rng = np.random.default_rng(w)
    keys = rng.permutation(np.unique(rng.integers(0, 1 << 32, 400).astype(np.uint32)))[:300]
    zeros = np.zeros((300, w), dt)
    vals = rng.standard_normal((300, w)).astype(dt)
    with ps.Shard.sparse(256, dt, "accumulate", width=w, init=UNI) as sh:
        first = ref_rows(keys, w, dt)
        sh.add(keys[:100], zeros[:100])  # init + 0
        same_bits(sh.get(keys[:100]), first[:100], "first bits")
        sh.add(keys[:100], vals[:100])
        # an erased key comes back with its first bits
        sh.erase(keys[:40])
        assert (bits(sh.get(keys[:40])) == 0).all(), "an erased key reads zeros"
        sh.add(keys[20:40], zeros[20:40])
        same_bits(sh.get(keys[20:40]), first[20:40], "erased and inserted again")
        same_bits(sh.get(keys[40:100]), first[40:100] + vals[40:100], "the survivors of the erase")
        # reserve between two inserting calls keeps the old rows, only new keys are initialised
        sh.add(keys[100:150], vals[100:150])
        sh.reserve(512)
        sh.add(keys[140:300], vals[140:300])
        same_bits(sh.get(keys[40:140]), first[40:140] + vals[40:140], "rows from before the reserve")
        same_bits(sh.get(keys[140:150]), (first[140:150] + vals[140:150]) + vals[140:150], "written on both sides")
        same_bits(sh.get(keys[150:300]), first[150:300] + vals[150:300], "new keys behind the reserve")
        sh.sync()
    # a full shard drops the extra keys and keeps what it stores
    with ps.Shard.sparse(64, dt, "accumulate", width=w, init=UNI) as sh:
        sh.add(keys[:64], vals[:64])
        sh.add(keys[32:96], vals[32:96])
        with pytest.raises(_lib.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE
        same_bits(sh.get(keys[:32]), first[:32] + vals[:32], "stored rows the overfull call did not name")
        same_bits(sh.get(keys[32:64]), (first[32:64] + vals[32:64]) + vals[32:64], "stored rows it named")
        assert (bits(sh.get(keys[64:96])) == 0).all() and sh.sparse_info()["count"] == 64
        sh.clear()
    # clear on a dense row shard: init(key), key_begin counts
    kd = np.arange(7, 7 + 300, dtype=np.uint32)
    with ps.Shard(7, 307, dt, width=w, init=UNI) as sh:
        same_bits(sh.get(kd), ref_rows(kd, w, dt), "a fresh row shard")
        sh.add(kd, vals)
        sh.clear()
        same_bits(sh.get(kd), ref_rows(kd, w, dt), "after clear")
    # kind ZERO set explicitly is the shard that never had an initializer
    with ps.Shard.sparse(512, dt, width=w) as a, ps.Shard.sparse(512, dt, width=w, init=("normal", 0.0, 1.0, 3)) as b:
        b.set_initializer("zero")
        for sh in (a, b):
            sh.set_optimizer("adagrad", lr=0.05)
            sh.apply(keys, vals)
        same_bits(a.get(keys), b.get(keys), "ZERO against never set")
        assert (bits(b.init_rows(keys)) == 0).all()
