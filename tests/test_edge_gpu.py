"""GPU tests of non-finite, subnormal and overflowing values on every path that
writes floats (tests/edge_util.py has the inputs, the checkers and their
derivations; tests/test_edge_cpu.py proves the checkers' teeth on these very
inputs).  Every expectation is the exact lattice sum, the extended-precision
reference, the dt emulation, or a twin shard that never saw the special values.
"""
import numpy as np
import pytest

import edge_util as eu
import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
import sparse_util as su
from rows_util import LAYOUTS, bits
from test_gpu_parity import tdev
from test_opt_gpu import PATHS, all_keys, assert_bits, do_apply, split3

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ids = lambda d: np.dtype(d).name  # noqa: E731


def rows_of(a, w):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.reshape(-1, w)


def read_all(sh, keys, slots):
    """p and every state slot of `keys`."""
    return rows_of(sh.get(keys), sh.width), [rows_of(sh.get_state(keys, slot=i), sh.width) for i in range(slots)]


# =================================================== 1. lattice accumulate
def push(sh, keys, vals, entry, cuda):
    if entry == "host":
        sh.add(keys, vals)
    elif entry == "device":
        sh.add(tdev(keys, cuda), tdev(vals, cuda))
    elif entry == "host_grouped":
        sh.add_grouped(split3(keys, vals))
    elif entry == "device_grouped":
        sh.add_grouped([(tdev(k, cuda), tdev(v, cuda)) for k, v in split3(keys, vals)])
    else:
        raise ValueError(entry)


ENTRIES = ["host", "device", "host_grouped", "device_grouped"]


@pytest.mark.parametrize("w", [1, 3, 4, 33])
@pytest.mark.parametrize("scale", eu.SCALES)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
def test_lattice_accumulate_row_shards(cuda, dt, scale, w):
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[0]
    rows = ke - kb
    rng = np.random.default_rng(ou.case_seed("lattice-rows", np.dtype(dt).name, scale, w))
    keys_all = all_keys(kb, ke)
    with ps.Shard(kb, ke, dt, mode="accumulate", width=w) as sh:
        for n in (2049, 4100):
            for entry in ENTRIES:
                sh.clear()
                lat = eu.Lattice(dt, scale, rows, w)
                idx, vals = eu.general_call(rng, lat, n, rows)
                push(sh, (kb + idx).astype(np.uint32), vals, entry, cuda)
                bad = eu.lattice_problems(rows_of(sh.get(keys_all), w), lat.want(), f"n {n} {entry}")
                assert bad is None, bad
        sh.sync()


@pytest.mark.parametrize("scale", eu.SCALES)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
def test_lattice_accumulate_sparse_shard(cuda, dt, scale):
    import parameter_server_amd as ps

    rows, w = 5000, 4
    rng = np.random.default_rng(ou.case_seed("lattice-sparse", np.dtype(dt).name, scale))
    pool = su.key_pool(rng, rows)
    with ps.Shard.sparse(8192, dt, "accumulate", width=w) as sh:
        lat = eu.Lattice(dt, scale, rows, w)
        for i, entry in enumerate(ENTRIES):
            idx, vals = eu.general_call(rng, lat, 4100 if i % 2 else 2049, rows, bigs=i == 0)
            push(sh, pool[idx], vals, entry, cuda)
        bad = eu.lattice_problems(rows_of(sh.get(pool), w), lat.want(), "sparse")
        assert bad is None, bad
        sh.sync()


DENSE_PATHS = ["k5", "k4a_stamps", "k7_aligned", "k7_unaligned", "k7_host", "lookalike", "inline", "serve"]


@pytest.mark.parametrize("path", DENSE_PATHS)
@pytest.mark.parametrize("scale", eu.SCALES)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
def test_lattice_accumulate_dense_shard(cuda, dt, scale, path):
    """A width-less shard's accumulate paths, by the selectors of
    tests/test_gpu_parity.py and tests/test_serve.py; k5 hits one key more than
    20 000 times in its call.  Out-of-range keys go to the overflow table."""
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    rng = np.random.default_rng(ou.case_seed("lattice-dense", np.dtype(dt).name, scale, path))
    kb = 1000
    rows = {"k5": 4096, "k4a_stamps": 4096, "inline": 2048, "serve": 2048}.get(path, 40_000)
    ke = kb + rows
    extra = np.array([ke + 7, 0xFFFFFFF0], dtype=np.uint32)
    options = {"k4a_stamps": {"GENERAL": "stamps"}, "inline": {"INLINE_ADD_CHUNKS": 8}, "serve": {"SERVE": 1}}.get(path)
    windows = path.startswith("k7") or path == "lookalike"
    lat = eu.Lattice(dt, scale, rows + 2, 1)

    def keys_of(idx):
        return np.where(idx < rows, kb + idx, extra[np.maximum(idx - rows, 0)]).astype(np.uint32)

    with ps.Shard(kb, ke, dt, mode="accumulate", overflow_slots=64, options=options) as sh:
        sh.set_timing(True)
        if windows:
            batches = [(keys_of(k), v.reshape(-1)) for k, v in
                       eu.window_calls(rng, lat, rows, aligned=path != "k7_unaligned", lookalike=path == "lookalike")]
            if path == "k7_host":
                sh.add_grouped(batches)
            else:
                off = 1 if path == "k7_unaligned" else 0
                sh.add_grouped([(tdev(k, cuda), tdev(v, cuda, off)) for k, v in batches], sorted_hint=True)
        elif path in ("inline", "serve"):
            inline_launches = 0
            for idx, vals in eu.small_messages(rng, lat, rows, 12, 2048 if path == "inline" else 256):
                sh.add(keys_of(idx), vals.reshape(-1))
                inline_launches += -(-idx.size // 256)  # kernel-argument messages of 256 keys
        else:
            n = 90_000 if path == "k5" else 45_000
            idx, vals = eu.general_call(rng, lat, n, rows, extra=2)
            assert path != "k5" or (idx == eu.HOT).sum() >= 20_000
            sh.add(tdev(keys_of(idx), cuda), tdev(vals.reshape(-1), cuda))
        q = np.concatenate([all_keys(kb, ke), extra])
        got = rows_of(sh.get(q), 1)
        launches = {k: sh.kernel_time(k)["launches"] for k in range(_lib.PSKV_K_COUNT)}
        sh.sync()
    ran = {_lib.KERNEL_NAMES[k] for k, c in launches.items() if c and k not in (_lib.PSKV_K_GATHER,
                                                                               _lib.PSKV_K_INLINE_GET)}
    names = lambda *ks: {_lib.KERNEL_NAMES[k] for k in ks}  # noqa: E731
    if path == "k7_host":  # the CPU proved the windows dense: K7 alone
        assert ran == names(_lib.PSKV_K_ACC_DENSE), ran
    elif windows:
        # K6, then K7, then the replay, which takes the group where K6 refused it:
        # all three are launched either way (K7 and the replay decide on the
        # device, by K6's flag), so the launches cannot tell a fallback; no other
        # Add kernel may run
        assert ran == names(_lib.PSKV_K_DENSE_CHECK, _lib.PSKV_K_ACC_DENSE, _lib.PSKV_K_REPLAY), ran
    elif path == "k5":
        assert ran == names(_lib.PSKV_K_RADIX), ran
    elif path == "k4a_stamps":
        assert ran <= names(_lib.PSKV_K_GENERAL_MARK, _lib.PSKV_K_REPLAY) and launches[_lib.PSKV_K_GENERAL_MARK] > 0, ran
    elif path == "inline":  # every message went in kernel arguments
        assert ran == names(_lib.PSKV_K_INLINE_ADD) and launches[_lib.PSKV_K_INLINE_ADD] == inline_launches, launches
    else:  # the request server takes ring slots, not launches: a fallback to K8 or to the staged path would show
        assert not ran, ran
    bad = eu.lattice_problems(got, lat.want(), path)
    assert bad is None, bad


# ================================================ 2. steps, special values
def _third_width(kind):
    return 33 if eu.KINDS.index(kind) % 2 else 3


def _step_params():
    out = []
    for kind in eu.KINDS:
        for w, path in ((1, "device"), (4, "host"), (_third_width(kind), "device_grouped"), (4, "host_grouped"),
                        (1, "device_unaligned")):
            out.append(pytest.param(kind, w, path, id=f"{kind}-{w}-{path}"))
    return out


def check_edge_step(sh, keys_all, idx, grads, hp, do, msg, pooled=None):
    """One step through `do`, checked from the shard's own state before it."""
    ns = eu.slot_count(hp)
    p, slots = read_all(sh, keys_all, ns)
    t = sh.step + 1
    do()
    pn, sn = read_all(sh, keys_all, ns)
    problems = eu.edge_step_errors(p, slots, idx, grads, pn, sn, sh.dtype, hp, t, pooled)
    assert not problems, f"{msg}: " + "; ".join(text for _, text in problems)


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind,w,path", _step_params())
def test_steps_with_special_values(cuda, kind, w, path, dt):
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[0]
    n = 2049
    hp = eu.kind_hyper(kind)
    p0, calls, _ = eu.edge_steps(ou.case_seed("edge", kind, np.dtype(dt).name, n, w), kb, ke, n, w, dt)
    keys_all = all_keys(kb, ke)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        eu.set_optimizer(sh, hp)
        sh.add(keys_all, p0)
        for step, (keys, grads) in enumerate(calls):
            check_edge_step(sh, keys_all, keys.astype(np.int64) - kb, grads, hp,
                            lambda: do_apply(sh, keys, grads, path, cuda), f"{path} step {step}")
        sh.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", eu.KINDS)
def test_steps_with_special_values_sparse_shard(cuda, kind, dt):
    import parameter_server_amd as ps

    rows, n, w = 5000, 2049, 4
    hp = eu.kind_hyper(kind)
    seed = ou.case_seed("edge-sparse", kind, np.dtype(dt).name)
    pool = su.key_pool(np.random.default_rng(seed), rows)
    p0, calls, _ = eu.edge_steps(seed, 0, rows, n, w, dt)
    with ps.Shard.sparse(8192, dt, "assign", width=w) as sh:
        eu.set_optimizer(sh, hp)
        sh.add(pool, p0)  # every key of the scenario is stored from here on
        for step, (keys, grads) in enumerate(calls):
            path = ("device", "host_grouped")[step % 2]
            check_edge_step(sh, pool, keys.astype(np.int64), grads, hp,
                            lambda: do_apply(sh, pool[keys], grads, path, cuda), f"{path} step {step}")
        sh.sync()


def _pooled_params():
    out = []
    for kind in ("sgd", "adam", "ftrl"):
        for w, path, weighted in ((1, "host", True), (4, "device", False), (4, "device_grouped", True),
                                  (_third_width(kind), "host_grouped", False), (4, "device", True)):
            out.append(pytest.param(kind, w, path, weighted, id=f"{kind}-{w}-{path}-{'w' if weighted else 'u'}"))
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind,w,path,weighted", _pooled_params())
def test_pooled_pushes_with_special_values(cuda, kind, w, path, weighted, dt):
    import torch

    import parameter_server_amd as ps

    kb, ke = LAYOUTS[0]
    n = 2049
    hp = eu.kind_hyper(kind)
    seed = ou.case_seed("edge-pooled", kind, np.dtype(dt).name, weighted)
    keys, off, bg, wts = eu.pooled_edge_call(seed, kb, ke, n, w, dt, weighted)
    p0 = np.random.default_rng(seed + 1).standard_normal((ke - kb, w)).astype(dt)
    keys_all = all_keys(kb, ke)

    def dev(batch):
        k, o, g = batch[:3]
        out = (tdev(k, cuda), torch.from_numpy(np.asarray(o).astype(np.int64)).to(cuda), tdev(g.reshape(-1), cuda))
        return out + ((tdev(batch[3], cuda),) if len(batch) == 4 else ())

    def do():
        if path == "host":
            ppu.apply_pooled(sh, keys, off, bg, wts)
        elif path == "device":
            ppu.apply_pooled(sh, keys, off, bg, wts, cuda)
        else:
            batches = eu.split_pooled(keys, off, bg, wts)
            sh.apply_pooled_grouped([dev(b) for b in batches] if path == "device_grouped" else batches)

    with ps.Shard(kb, ke, dt, width=w) as sh:
        eu.set_optimizer(sh, hp)
        sh.add(keys_all, p0)
        for step in range(2):  # the second step starts from a state that holds NaNs and infinities
            check_edge_step(sh, keys_all, keys.astype(np.int64) - kb, None, hp, do, f"{path} step {step}",
                            pooled=(wts, bg, ppu.bag_index(off)))
        sh.sync()


# ======================================== 3. no residue in the gradient scratch
@pytest.mark.parametrize("residue", eu.RESIDUES)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", ["adagrad", "ftrl", "adam"])
def test_no_residue_in_the_gradient_scratch(cuda, kind, dt, residue):
    """Twin shards: A's first step leaves `residue` as its losers' sum, B never
    sees it.  After the same refill the same steps on distinct keys (bit for
    bit specified) must leave the same bits, after each step."""
    import parameter_server_amd as ps

    sparse = kind == "adam"
    w, rows = (4, 5000) if sparse else (3, 5000)
    case = eu.residue_case(kind, dt, w, residue, rows)
    hp = case["hp"]
    rng = np.random.default_rng(ou.case_seed("residue-keys", kind))
    keymap = su.key_pool(rng, rows) if sparse else all_keys(0, rows)
    make = (lambda: ps.Shard.sparse(8192, dt, "assign", width=w)) if sparse else (lambda: ps.Shard(0, rows, dt, width=w))
    ns = eu.slot_count(hp)
    with make() as a, make() as b:
        for sh in (a, b):
            eu.set_optimizer(sh, hp)
            sh.add(keymap, np.zeros((rows, w), dtype=dt))
        idx, grads = case["first"]
        a.apply(tdev(keymap[idx], cuda), tdev(grads, cuda))
        b.step = a.step
        for sh in (a, b):
            sh.add(keymap, case["p1"])
            for i, s in enumerate(case["slots1"]):
                sh.put_state(keymap, s, slot=i)
        for step, (fi, fg) in enumerate(case["follow"]):
            for sh in (a, b):
                if step:
                    sh.apply(keymap[fi], fg)
                else:
                    sh.apply(tdev(keymap[fi], cuda), tdev(fg, cuda))
            (pa, sa), (pb, sb) = read_all(a, keymap, ns), read_all(b, keymap, ns)
            assert_bits(pa, pb, f"p after follow-up step {step}")
            for i in range(ns):
                assert_bits(sa[i], sb[i], f"slot {i} after follow-up step {step}")
        a.sync()
        b.sync()


# ========================================== 4. subnormal-scale dyadic steps
def _dyadic_params():
    out = []
    widths = [1, 3, 4, 16, 33, 64]
    for n in (2049, 4100):
        for pat in ("distinct", "all_equal", "dups_in_chunk", "dups_across_chunks", "range_ends"):
            c = len(out)
            out.append((n, pat, widths[(c + c // 6) % 6]))
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("n,pat,w", _dyadic_params())
@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov"])
def test_subnormal_scale_dyadic_steps_are_bit_exact(cuda, kind, n, pat, w, dt):
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[0]
    hp, p0, calls, expect = eu.dyadic_case(kind, n, w, pat, dt)
    keys_all = all_keys(kb, ke)
    ns = eu.slot_count(hp)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        eu.set_optimizer(sh, hp)
        for path in PATHS:
            sh.clear()
            sh.add(keys_all, p0)
            for step, (keys, grads) in enumerate(calls):
                do_apply(sh, keys, grads, path, cuda)
                p, slots = read_all(sh, keys_all, ns)
                assert_bits(p, expect[step][0], f"p {path} step {step}")
                for i in range(ns):
                    assert_bits(slots[i], expect[step][1][i], f"slot {i} {path} step {step}")
        sh.sync()


# ============================================================ 5. pooled pulls
R_PINF, R_NINF, R_INF2, R_MAX, R_NAN, R_LAT = 10, 11, 12, 13, 14, 20


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("w", [1, 4, 5])
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
def test_pooled_pulls_with_special_rows(cuda, dt, w, weighted):
    """Shard A holds the special rows, its twin B ordinary values in their
    place.  B meets the pooled bound; A differs from B only in the tainted
    bags' tainted column, whose class is fixed; the subnormal lattice bag is
    exact in both."""
    import parameter_server_amd as ps

    dt = np.dtype(dt)
    kb, ke = 0, 3000
    rng = np.random.default_rng(ou.case_seed("edge-pull", dt.name, w, weighted))
    c = 1 if w > 1 else 0
    pb = pu.draw_values(rng, (ke - kb, w), dt)
    lat_ints = rng.integers(-3, 4, size=(8, w))
    lat_ints[3] = eu.BIG
    pb[R_LAT:R_LAT + 8] = np.ldexp(lat_ints.astype(dt), eu.SUB_EXP[dt])
    pa = pb.copy()
    pa[R_PINF, c], pa[R_NINF, c], pa[R_INF2, c], pa[R_NAN, c] = np.inf, -np.inf, np.inf, np.nan
    pa[R_MAX, c] = np.finfo(dt).max
    lens = [6, 5, 4, 12, pu.CHUNK + 50, 7, 0, 3]
    off = pu.offsets_of(lens).astype(np.int64)
    keys = (kb + rng.integers(40, ke - kb, size=int(off[-1]))).astype(np.uint32)
    wts = pu.draw_values(rng, keys.size, dt) if weighted else None
    plant = {int(off[0]) + 1: (R_PINF, 1.5), int(off[0]) + 4: (R_NINF, 2.0), int(off[1]) + 2: (R_INF2, 0.0),
             int(off[2]): (R_MAX, 1.0), int(off[2]) + 3: (R_MAX, 1.0), int(off[4]) + pu.CHUNK + 10: (R_NAN, 1.0)}
    lat_w = rng.choice([-2, -1, 1, 2], size=12)
    lat_rows = rng.integers(0, 8, size=12)
    lat_rows[lat_rows == 3] = 4
    lat_rows[5] = 3  # the +-2^22 row is part of the bag, once
    lat_mul = lat_w[:, None] if weighted else np.ones((12, 1), dtype=np.int64)
    assert (np.abs(lat_ints[lat_rows] * lat_mul).sum(axis=0) < eu.LIMIT).all(), "the lattice condition"
    for j in range(12):
        plant[int(off[3]) + j] = (R_LAT + int(lat_rows[j]), float(lat_w[j]))
    for pos, (row, wt) in plant.items():
        keys[pos] = kb + row
        if weighted:
            wts[pos] = wt
    want_c = {0: np.nan, 1: np.nan if weighted else np.inf, 2: np.inf, 4: np.nan}
    exact = np.ldexp((lat_ints[lat_rows] * lat_mul).sum(axis=0).astype(dt), eu.SUB_EXP[dt])
    keys_all = all_keys(kb, ke)
    with ps.Shard(kb, ke, dt, width=w) as a, ps.Shard(kb, ke, dt, width=w) as b:
        a.add(keys_all, pa)
        b.add(keys_all, pb)
        ref = pu.reference(pb, kb, keys, off.astype(np.uint64), wts)
        for dev in (None, cuda):
            ga = pu.pooled(a, keys, off.astype(np.uint64), wts, dev)
            gb = pu.pooled(b, keys, off.astype(np.uint64), wts, dev)
            msg = f"device={dev is not None}"
            pu.check(gb, ref, msg)
            same = bits(ga) == bits(gb)
            for bag, v in want_c.items():
                same[bag, c] = np.isnan(ga[bag, c]) if np.isnan(v) else ga[bag, c] == v
            assert same.all(), f"{msg}: (bag, col) {np.argwhere(~same)[:4].tolist()} got {ga[~same][:4]}"
            assert_bits(ga[3:4], exact[None, :], f"{msg}: the subnormal lattice bag")
            assert_bits(gb[3:4], exact[None, :], f"{msg}: the subnormal lattice bag of the twin")
        a.sync()
        b.sync()


# ============================================= 6. assign Adds and Gets keep bits
SPECIAL_BITS = {
    np.dtype(np.float32): [0x7FC00001, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x80000000, 0x00000001, 0x80000001,
                           0x007FFFFF, 0x00400000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x3F800000],
    np.dtype(np.float64): [0x7FF8000000000001, 0x7FF0000000000001, 0xFFF8000012345678, 0x7FFFFFFFFFFFFFFF,
                           0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF,
                           0x0008000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000,
                           0xFFF0000000000000, 0x3FF0000000000000],
}


def special_rows(rng, n, w, dt):
    u = {4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]
    return rng.choice(np.array(SPECIAL_BITS[np.dtype(dt)], dtype=u), size=(n, w)).view(dt)


class LastWins:
    """key -> the bits of its last pushed row."""

    def __init__(self, w, dt):
        self.w, self.dt, self.rows = w, np.dtype(dt), {}

    def add(self, keys, vals):
        vals = np.asarray(vals).reshape(len(keys), self.w)
        for k, v in zip(np.asarray(keys).tolist(), vals):
            self.rows[k] = v

    def get(self, keys):
        zero = np.zeros(self.w, dtype=self.dt)
        return np.array([self.rows.get(k, zero) for k in np.asarray(keys).tolist()], dtype=self.dt).reshape(-1, self.w)


def _assign_knobs():
    """tests/test_fuzz.py's option sets, each once."""
    from test_fuzz import KNOBS

    out = []
    for k in KNOBS:
        if k not in out:
            out.append(k)
    return out


def _knob_id(k):
    return "-".join(f"{a}-{b}" for a, b in k.items()) or "default"


@pytest.mark.parametrize("knobs", _assign_knobs(), ids=_knob_id)
@pytest.mark.parametrize("dt", DTYPES, ids=ids)
def test_assign_keeps_bits_dense_shard(cuda, dt, knobs):
    """Every option set of tests/test_fuzz.py, and its calls: host and device
    Adds, single and grouped, small and large, unsorted, sorted and dense
    windows (the host-verified sorted path; the device ones with and without
    the hint, aligned and not), add_get_grouped with and without the hint,
    out-of-range keys through the overflow table; host, device and grouped
    Gets.  A Get returns the last occurrence's bits, NaN payloads included."""
    import torch

    import parameter_server_amd as ps

    dt = np.dtype(dt)
    kb, ke = 1000, 1000 + 65_536
    rng = np.random.default_rng(ou.case_seed("edge-assign", dt.name, repr(knobs)))
    ref = LastWins(1, dt)
    tdt = torch.float32 if dt == np.float32 else torch.float64

    def draw(n, kind="uniform"):
        if kind == "dense":
            first = int(rng.integers(kb, ke - n + 1))
            return np.arange(first, first + n, dtype=np.uint32)
        k = rng.integers(kb - 30, ke + 30, size=n)
        k[::17] = k[0]
        return (np.sort(k) if kind == "sorted" else k).astype(np.uint32)

    def vals(k):
        return special_rows(rng, k.size, 1, dt).reshape(-1)

    def add(k, dev=False, off=0, hint=False):
        v = vals(k)
        if dev:
            sh.add(tdev(k, cuda, off), tdev(v, cuda, off), sorted_hint=hint)
        else:
            sh.add(k, v)
        ref.add(k, v)

    def add_grouped(ks, dev=False, hint=False):
        batches = [(k, vals(k)) for k in ks]
        if dev:
            sh.add_grouped([(tdev(k, cuda), tdev(v, cuda)) for k, v in batches], sorted_hint=hint)
        else:
            sh.add_grouped(batches)
        for k, v in batches:
            ref.add(k, v)

    with ps.Shard(kb, ke, dt, overflow_slots=64, options=knobs) as sh:
        for kind in ("uniform", "sorted", "dense"):  # host: inline / request server / staged, then the large paths
            for n in (200, 5000, 40_000):
                add(draw(n, kind))
            add_grouped([draw(2100, kind), draw(33, kind), draw(20_001, kind)])
        for off, hint in ((0, False), (1, False), (0, True), (3, True)):
            add(draw(5000, "sorted" if hint else "uniform"), dev=True, off=off, hint=hint)
        add(draw(40_000), dev=True)
        add(draw(40_000, "dense"), dev=True, hint=True)
        add(draw(5000), dev=True, hint=True)  # a wrong hint: repaired
        wins = [np.arange(f, f + m, dtype=np.uint32) for f, m in ((kb + 8, 30_000), (kb + 15_000, 20_001), (kb + 9, 1))]
        add_grouped(wins, dev=True, hint=True)
        add_grouped([draw(2100), draw(33), draw(20_001, "sorted")], dev=True)
        for hint in (False, True):
            kind = "dense" if hint else "uniform"
            adds = [(k, vals(k)) for k in (draw(8192, kind), draw(1, kind), draw(3000, "sorted" if hint else "uniform"))]
            qs = [adds[0][0][100:4100].copy(), draw(700), draw(300, "sorted")]
            outs = [torch.empty(q.size, dtype=tdt, device=cuda) for q in qs]
            sh.add_get_grouped([(tdev(k, cuda), tdev(v, cuda)) for k, v in adds],
                               [(tdev(q, cuda), o) for q, o in zip(qs, outs)], sorted_hint=hint)
            for k, v in adds:
                ref.add(k, v)
            for q, o in zip(qs, outs):
                assert_bits(rows_of(o, 1), ref.get(q), f"add_get_grouped hint={hint}")
        q = np.arange(kb - 40, ke + 40, dtype=np.uint32)
        assert_bits(rows_of(sh.get(q), 1), ref.get(q), "host get")
        assert_bits(rows_of(sh.get(q[:300]), 1), ref.get(q[:300]), "small host get")
        assert_bits(rows_of(sh.get(tdev(q, cuda)), 1), ref.get(q), "device get")
        assert_bits(rows_of(sh.get(tdev(q, cuda, 1)), 1), ref.get(q), "unaligned device get")
        qs = [draw(300), draw(5000, "dense"), draw(1), draw(5000, "sorted")]
        outs = [np.empty(k.size, dtype=dt) for k in qs]
        sh.get_grouped(list(zip(qs, outs)))
        for k, o in zip(qs, outs):
            assert_bits(rows_of(o, 1), ref.get(k), "host get_grouped")
        outs = [torch.empty(k.size, dtype=tdt, device=cuda) for k in qs]
        sh.get_grouped([(tdev(k, cuda), o) for k, o in zip(qs, outs)])
        for k, o in zip(qs, outs):
            assert_bits(rows_of(o, 1), ref.get(k), "device get_grouped")
        sh.sync()


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
def test_assign_keeps_bits_row_shard(cuda, dt):
    import parameter_server_amd as ps

    dt = np.dtype(dt)
    kb, ke, w = LAYOUTS[0][0], LAYOUTS[0][1], 3
    rng = np.random.default_rng(ou.case_seed("edge-assign-rows", dt.name))
    ref = LastWins(w, dt)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        for entry in ENTRIES:
            for n in (200, 2049):
                k = (kb + rng.integers(0, 600, size=n)).astype(np.uint32)
                v = special_rows(rng, n, w, dt)
                push(sh, k, v, entry, cuda)
                ref.add(k, v)
        q = all_keys(kb, ke)
        assert_bits(rows_of(sh.get(q), w), ref.get(q), "host get")
        assert_bits(rows_of(sh.get(tdev(q, cuda)), w), ref.get(q), "device get")
        sh.sync()
