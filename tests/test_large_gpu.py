"""GPU tests at array offsets past 2^32: row arrays that cross
byte offset 2^32 and element index 2^31, a sparse shard of that size, a scalar
shard of 2^31 + 8192 keys with its 17 GB of stamps, and scalar shards of the
whole key space.

Every call touches a few hundred to a few thousand keys: at the bottom of the
range, within 2048 keys of every boundary the array crosses, and at its top,
with duplicates across those bands.  (A row of width 4096 is 16 KiB, so the row
cases draw about a thousand distinct keys, not several thousand.)  The
references are the suite's, fed compact row numbers (the rank of a key among
the keys the case may touch or probe), so that no host array follows the
shard's size: last-write-wins by numpy assignment per row (one MapStorageRef
per column is out of reach at width 4096) or the oracle's MapStorageRef
(scalar shards), edge_util.Lattice and test_fuzz.AccRef for sums,
pooled_util.reference, opt_util.step_ref on dyadic values (exact).  After each
case the probe keys on both sides of every boundary that no call touched must
read zero, and every touched key its reference's bits: a write that wrapped
lands on neither.

A case skips only where the device has less free memory than it needs plus
8 GiB; none holds more than 40 GiB.
"""
import numpy as np
import pytest

import edge_util as eu
import opt_util as ou
import pooled_push_util as ppu
import pooled_util as pu
import test_fuzz as tf
from rows_util import bits
from test_gpu_parity import assert_bits_equal, tdev
from test_opt_gpu import assert_bits

pytestmark = pytest.mark.gpu

GIB = 1 << 30
BAND = 2048
PEAK = {"bytes": 0}


def need(cuda, gib):
    """Skip unless `gib` GiB and 8 more are free; returns the bytes in use before the case."""
    import torch

    free, total = torch.cuda.mem_get_info(cuda)
    if free < (gib + 8) * GIB:
        pytest.skip(f"{free / GIB:.0f} GiB of HBM free, the case needs {gib} + 8")
    return total - free


def held(cuda, before, limit_gib=40):
    """The HBM the case holds now (beyond what was in use before it)."""
    import torch

    free, total = torch.cuda.mem_get_info(cuda)
    now = total - free - before
    PEAK["bytes"] = max(PEAK["bytes"], now)
    print(f"HBM held by this case: {now / GIB:.1f} GiB (peak of the module so far {PEAK['bytes'] / GIB:.1f} GiB)")
    assert now <= limit_gib * GIB, f"the case holds {now / GIB:.1f} GiB"
    return now


class Keys:
    """The keys a case may touch (`t`) and the probes it never touches (`u`),
    offsets into a range of `span` keys from kb: the bottom band, +-BAND around
    every boundary, the top band.  b - 1, b, 0 and span - 1 are always touched,
    b - 2 and b + 1 never."""

    def __init__(self, rng, kb, span, boundaries, per, probes):
        bands = [(0, BAND)] + [(b - BAND, b + BAND) for b in boundaries] + [(span - BAND, span)]
        t, u = [0, span - 1], []
        for b in boundaries:
            t += [b - 1, b]
            u += [b - 2, b + 1]
        for lo, hi in bands:
            assert 0 <= lo < hi <= span
            pick = lo + rng.permutation(hi - lo)[:per + probes]
            t += pick[:per].tolist()
            u += pick[per:].tolist()
        self.u = np.setdiff1d(np.unique(u), [0, span - 1] + [x for b in boundaries for x in (b - 1, b)])
        self.t = np.setdiff1d(np.unique(t), self.u)
        self.offs = np.union1d(self.t, self.u)  # sorted: a key's row number is its rank here
        self.kb, self.span, self.boundaries, self.rng = kb, span, list(boundaries), rng
        self.all = self.key(self.offs)
        self.touched = np.isin(self.offs, self.t)
        for b in boundaries:  # keys on both sides of every boundary, touched and not
            assert ((self.t < b).any() and (self.t >= b).any() and (self.u < b).any() and (self.u >= b).any())

    def key(self, offs):
        return (np.asarray(offs, dtype=np.int64) + self.kb).astype(np.uint32)

    def rank(self, keys):
        offs = (np.asarray(keys).astype(np.int64) - self.kb) % (1 << 32)
        r = np.searchsorted(self.offs, offs)
        assert np.array_equal(self.offs[r], offs)
        return r

    def draw(self, n, distinct=False, sort=False):
        """n touched keys; repeated ones lie anywhere in the call, so a key's
        occurrences straddle the bands of the keys between them."""
        if distinct:
            offs = self.rng.permutation(self.t)[:n]
        else:
            offs = self.t[self.rng.integers(0, self.t.size, size=n)]
            offs[-1] = offs[0]  # one key first and last
            offs[n // 2] = self.span - 1
            offs[n // 2 + 1] = 0
        if sort:
            offs = np.sort(offs)
        return self.key(offs)

    def untouched_zero(self, got, what):
        got = np.asarray(got).reshape(self.offs.size, -1)
        bad = np.flatnonzero(bits(got[~self.touched]).any(axis=1))
        assert bad.size == 0, f"{what}: {bad.size} untouched keys are not zero, first offsets {self.offs[~self.touched][bad[:3]]}"


def unique_rows(c, n, w, dt):
    """Values that name their occurrence and column (exact in every dtype)."""
    v = (c * 7919 + np.arange(n, dtype=np.int64)[:, None] * 131 + np.arange(w, dtype=np.int64)[None, :]) % (2**24 - 1) + 1
    return v.astype(dt)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ================================================================= row shards
# float32 rows; (width, keys, boundaries in keys): byte offset 2^32 and element index 2^31
W4096 = (4096, 2**19 + 4096, [2**18, 2**19])
W1000 = (1000, 2147484 + 4096, [-(-2**32 // 4000), -(-2**31 // 1000)])
ROW_BASES = ["low", "high"]


def row_case(shape, base, seed, per=160, probes=48):
    w, span, boundaries = shape
    assert span * w * 4 > 2**33 and boundaries[0] * w * 4 >= 2**32 > (boundaries[0] - 1) * w * 4
    assert boundaries[1] * w >= 2**31 > (boundaries[1] - 1) * w
    kb = 0 if base == "low" else 2**32 - span
    rng = np.random.default_rng(ou.case_seed("large-rows", w, base, seed))
    return w, kb, kb + span, Keys(rng, kb, span, boundaries, per, probes), rng


def check_rows(sh, ks, want, what, cuda=None, state=None):
    q = ks.all if cuda is None else tdev(ks.all, cuda)
    got = host(sh.get(q) if state is None else sh.get_state(q, slot=state)).reshape(want.shape)
    assert_bits(got, want, what)
    ks.untouched_zero(got, what)


@pytest.mark.parametrize("base", ROW_BASES)
@pytest.mark.parametrize("shape", [W4096, W1000], ids=["w4096", "w1000"])
def test_row_assign_and_get(cuda, shape, base):
    import parameter_server_amd as ps

    w, kb, ke, ks, rng = row_case(shape, base, "assign")
    before = need(cuda, 9)
    want = np.zeros((ks.offs.size, w), dtype=np.float32)
    with ps.Shard(kb, ke, np.float32, width=w) as sh:
        for c, entry in enumerate(["device", "host", "device_grouped"]):
            k = ks.draw(1500)
            v = unique_rows(c, k.size, w, np.float32)
            if entry == "device":
                sh.add(tdev(k, cuda), tdev(v, cuda))
            elif entry == "host":
                sh.add(k, v)
            else:
                sh.add_grouped([(tdev(k[:700], cuda), tdev(v[:700], cuda)), (tdev(k[700:], cuda), tdev(v[700:], cuda))])
            want[ks.rank(k)] = v  # (a repeated row number: the last assignment stays)
            check_rows(sh, ks, want, f"{entry} add, host get")
        check_rows(sh, ks, want, "device get", cuda)
        held(cuda, before)
        sh.sync()


@pytest.mark.parametrize("base", ROW_BASES)
def test_row_accumulate(cuda, base):
    import parameter_server_amd as ps

    w, kb, ke, ks, rng = row_case(W4096, base, "accumulate", per=96, probes=32)
    before = need(cuda, 9)
    lat = eu.Lattice(np.float32, "one", ks.offs.size, w)
    with ps.Shard(kb, ke, np.float32, mode="accumulate", width=w) as sh:
        for entry in ("device", "host"):
            k = ks.draw(1200)
            vals = lat.add(ks.rank(k), rng.integers(-3, 4, size=(k.size, w)))
            if entry == "device":
                sh.add(tdev(k, cuda), tdev(vals, cuda))
            else:
                sh.add(k, vals)
            got = np.asarray(sh.get(ks.all)).reshape(-1, w)
            bad = eu.lattice_problems(got, lat.want(), f"{entry} accumulate")
            assert bad is None, bad
            ks.untouched_zero(got, entry)
        held(cuda, before)
        sh.sync()


@pytest.mark.parametrize("base", ROW_BASES)
def test_row_pooled_pull(cuda, base):
    import parameter_server_amd as ps

    w, kb, ke, ks, rng = row_case(W4096, base, "pooled", per=96, probes=32)
    before = need(cuda, 9)
    p = np.zeros((ks.offs.size, w), dtype=np.float32)
    with ps.Shard(kb, ke, np.float32, width=w) as sh:
        k = ks.draw(ks.t.size, distinct=True)
        p[ks.rank(k)] = pu.draw_values(rng, (k.size, w), np.float32)
        sh.add(tdev(k, cuda), tdev(p[ks.rank(k)], cuda))
        for lens, weighted, device in (([1, 2, 8, 0, 3, 5] * 20, False, True), ([300, 1, 260, 7], True, True),
                                       ([4, 300, 2], True, False)):
            n = int(np.sum(lens))
            q = ks.key(ks.offs[rng.integers(0, ks.offs.size, size=n)])  # touched and untouched rows
            off = pu.offsets_of(lens)
            wts = pu.draw_values(rng, n, np.float32) if weighted else None
            got = pu.pooled(sh, q, off, wts, cuda if device else None)
            pu.check(got, pu.reference(p, 0, ks.rank(q).astype(np.uint32), off, wts), f"bags {lens[:4]} device {device}")
        held(cuda, before)
        sh.sync()


def dyadic_step(p, slots, idx, rows, hp, t, dt):
    """opt_util.step_ref on dyadic values: exact, so the expectation is its bits."""
    ref = ou.step_ref(p, slots, idx, rows, hp, t)
    out = [ref["p"]] + list(ref["slots"])
    for a in out:
        assert np.array_equal(a.astype(dt).astype(ou.F), a), "the dyadic step is not exact in the shard's type"
    return out[0].astype(dt), [s.astype(dt) for s in out[1:]]


STEP_CASES = [("sgd", W4096, "low"), ("sgd", W4096, "high"), ("momentum", W4096, "low"), ("momentum", W4096, "high"),
              ("sgd", W1000, "high")]


@pytest.mark.parametrize("kind,shape,base", STEP_CASES, ids=[f"{k}-w{s[0]}-{b}" for k, s, b in STEP_CASES])
def test_row_steps_and_state(cuda, kind, shape, base):
    """pskv_put_state / pskv_get_state_slot (momentum), then a step through
    pskv_apply and one through pskv_apply_pooled, on dyadic values."""
    import parameter_server_amd as ps

    w, kb, ke, ks, rng = row_case(shape, base, kind, per=96, probes=32)
    dt = np.dtype(np.float32)
    hp = ou.hyper("sgd", lr=ou.DYADIC_LR) if kind == "sgd" else ou.dyadic_hyper(False)
    ns = ou.SLOTS[kind]
    before = need(cuda, 9 * (2 + ns) + 5)  # p, the gradient scratch, the state, the stamps
    rows = ks.offs.size
    p = np.zeros((rows, w), dtype=dt)
    slots = [np.zeros((rows, w), dtype=dt) for _ in range(ns)]
    with ps.Shard(kb, ke, dt, width=w) as sh:
        ppu.set_optimizer(sh, hp)
        k = ks.draw(ks.t.size, distinct=True)
        p[ks.rank(k)] = ou.dyadic_params(rng, k.size, w, dt)
        sh.add(tdev(k, cuda), tdev(p[ks.rank(k)], cuda))
        if ns:
            k = ks.draw(900)
            v = (rng.integers(-64, 65, size=(k.size, w)) / 16.0).astype(dt)
            sh.put_state(tdev(k, cuda), tdev(v, cuda), slot=0)
            slots[0][ks.rank(k)] = v
            check_rows(sh, ks, slots[0], "put_state", cuda, state=0)
        k = ks.draw(1200)
        g = ou.dyadic_grads(rng, k.size, w, dt)
        sh.apply(tdev(k, cuda), tdev(g, cuda))
        p, slots = dyadic_step(p, slots, ks.rank(k), g, hp, 1, dt)
        check_rows(sh, ks, p, "p after pskv_apply")
        for i in range(ns):
            check_rows(sh, ks, slots[i], f"slot {i} after pskv_apply", state=i)
        k, off, bg, wts = ppu.draw_call(rng, 1200, w, "dups_in_chunk", "mixed", 0, 8, dt, True, dyadic=True)
        k = ks.draw(1200)
        ppu.apply_pooled(sh, k, off, bg, wts, cuda)
        p, slots = dyadic_step(p, slots, ks.rank(k), ppu.ref_grads(wts, bg, ppu.bag_index(off)), hp, 2, dt)
        check_rows(sh, ks, p, "p after pskv_apply_pooled", cuda)
        for i in range(ns):
            check_rows(sh, ks, slots[i], f"slot {i} after pskv_apply_pooled", cuda, state=i)
        assert sh.step == 2
        held(cuda, before)
        sh.sync()


# =============================================================== sparse shard
def test_sparse_shard_slots_past_the_boundaries(cuda):
    """Capacity 2^19 + 4096 rows of width 4096; one device Add stores 2^19 + 3072
    scattered keys (0 and 0xFFFFFFFF among them), so slots on both sides of byte
    offset 2^32 and element index 2^31 are in use whatever the index does.
    Lattice values made on the device; the reference is their formula."""
    import torch

    import parameter_server_amd as ps

    w, cap = 4096, 2**19 + 4096
    n = 2**19 + 3072
    before = need(cuda, 26)
    rng = np.random.default_rng(ou.case_seed("large-sparse"))
    keys = (np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % (1 << 32)  # an odd multiplier: distinct
    keys[1], keys[-2] = 0, 0xFFFFFFFF
    keys = keys.astype(np.uint32)
    assert np.unique(keys).size == n

    def first_rows(i):  # the row of insertion number i: small integers
        i = np.asarray(i, dtype=np.int64)
        return ((i[:, None] % 7 - 3) + (np.arange(w, dtype=np.int64)[None, :] % 5)).astype(np.float32)

    # probes: the first and last insertions and a spread; absent keys read zero
    probe = np.unique(np.concatenate([np.arange(3000), np.arange(n - 3000, n), rng.integers(0, n, size=500),
                                      np.arange(2**18 - 300, 2**18 + 300), np.arange(2**19 - 300, 2**19 + 300)]))
    absent = np.setdiff1d(rng.integers(0, 1 << 32, size=200).astype(np.uint32), keys)
    with ps.Shard.sparse(cap, np.float32, "assign", width=w) as sh:
        i = torch.arange(n, device=cuda, dtype=torch.int64)
        vals = (i % 7 - 3).to(torch.float32)[:, None] + (torch.arange(w, device=cuda) % 5).to(torch.float32)[None, :]
        sh.add(tdev(keys, cuda), vals)
        sh.sync()
        del vals, i
        torch.cuda.empty_cache()
        info = sh.sparse_info()
        assert info["count"] == n > 2**19 + 2048 and info["capacity"] == cap
        want = first_rows(probe)
        assert_bits(host(sh.get(tdev(keys[probe], cuda))).reshape(want.shape), want, "after the first Add, device get")
        assert not np.asarray(sh.get(absent)).any(), "an absent key reads non-zero"
        # a second Add on the probes, with repeats across them: the last occurrence's row stays
        r = rng.integers(0, probe.size, size=1500)
        r[-1] = r[0]
        v = unique_rows(1, r.size, w, np.float32) % 4093  # (small: the step below stays exact in float32)
        sh.add(tdev(keys[probe[r]], cuda), tdev(v, cuda))
        want[r] = v
        got = np.asarray(sh.get(keys[probe])).reshape(-1, w)
        assert_bits(got, want, "after the second Add, host get")
        # one SGD step on them (dyadic: exact)
        hp = ou.hyper("sgd", lr=ou.DYADIC_LR)
        ppu.set_optimizer(sh, hp)
        r = rng.integers(0, probe.size, size=1500)
        r[-1] = r[0]
        g = ou.dyadic_grads(rng, r.size, w, np.float32)
        sh.apply(tdev(keys[probe[r]], cuda), tdev(g, cuda))
        p, _ = dyadic_step(got, [], r, g, hp, 1, np.dtype(np.float32))
        assert_bits(np.asarray(sh.get(keys[probe])).reshape(-1, w), p, "after the step")
        assert not np.asarray(sh.get(absent)).any(), "an absent key reads non-zero after the step"
        assert sh.sparse_info()["count"] == n
        held(cuda, before)
        sh.sync()


# ============================================================== scalar shards
def scalar_keys(seed, kb, span, boundaries, per=400, probes=120):
    rng = np.random.default_rng(ou.case_seed("large-scalar", seed))
    return Keys(rng, kb, span, boundaries, per, probes), rng


def check_scalar(sh, ks, ref_get, what, cuda=None):
    q = ks.all if cuda is None else tdev(ks.all, cuda)
    want = ref_get(ks.all)  # (zero for a key no call wrote: the probes beside every boundary among them)
    assert_bits_equal(host(sh.get(q)), want, what)
    return want


def window(ks, lo, n):
    return ks.key(np.arange(lo, lo + n, dtype=np.int64))


# the option sets of tests/test_fuzz.py that change the sorted Add's tiles and grid, the Get's unroll,
# and the resident window on (auto: 224 MiB of a 16 GiB array) and off
ASSIGN_KNOBS = [{}, {"TILE_GRID": 1024}, {"TILE_SHIFT": 16}, {"GET_UNROLL": 4}, {"GET_UNROLL": 8}, {"RESIDENT_BYTES": 0},
                {"RESIDENT_BYTES": 0, "GET_UNROLL": 8}, {"EARLY": 1}, {"EARLY": 0}, {"UNROLL": 4}, {"NTP": 0}]


def test_whole_key_space_assign(cuda, oracle_mod):
    """pskv_shard_create(0, 2^32, float32): the Get (K1) and the sorted Add with a
    hint that holds, single (K2) and grouped (K2g: windows across element
    index 2^31 and up to key 0xFFFFFFFF, and sorted batches that are no
    windows, which take the tile mode), under every option set.  No stamp array
    is made (asserted by the memory held).  One shard serves every option set:
    the keys a set wrote are assigned zero again (one host Add) before the next."""
    import parameter_server_amd as ps

    span = 1 << 32
    before = need(cuda, 17)
    ks, rng = scalar_keys("assign", 0, span, [2**30, 2**31, 3 * 2**30])
    wins = [(2**31 - 1000, 2001), (span - 5000, 5000), (2**30 - 7, 1027), (0, 1024)]
    with ps.Shard(0, span, np.float32) as sh:
        assert sh.get_option("RESIDENT_BYTES") == -1 and sh.info()["resident_bytes"] > 0
        defaults = {name: sh.get_option(name) for knobs in ASSIGN_KNOBS for name in knobs}
        for ci, knobs in enumerate(ASSIGN_KNOBS):
            for name, v in {**defaults, **knobs}.items():
                sh.set_option(name, v)
            ref = oracle_mod.MapStorageRef(np.float32)
            wrote = []
            try:
                def add(batches, grouped):
                    dev = [(tdev(k, cuda), tdev(v, cuda)) for k, v in batches]
                    e0 = sh.get_option("EPOCH")
                    if grouped:
                        sh.add_grouped(dev, sorted_hint=True)
                    else:
                        sh.add(*dev[0], sorted_hint=True)
                    assert sh.get_option("EPOCH") == e0 + 1
                    for k, v in batches:
                        ref.add(k, v)
                        wrote.append(k)

                k = ks.draw(2500, distinct=True, sort=True)
                add([(k, unique_rows(ci, k.size, 1, np.float32).reshape(-1))], False)          # K2
                check_scalar(sh, ks, ref.get, f"{knobs} K2", cuda)
                ws = [window(ks, lo, n) for lo, n in wins]
                add([(k, unique_rows(ci + 50 + j, k.size, 1, np.float32).reshape(-1)) for j, k in enumerate(ws)], True)  # K2g, windows
                tiles = [ks.draw(900, distinct=True, sort=True) for _ in range(3)]
                add([(k, unique_rows(ci + 90 + j, k.size, 1, np.float32).reshape(-1)) for j, k in enumerate(tiles)], True)  # K2g, tiles
                check_scalar(sh, ks, ref.get, f"{knobs} K2g", cuda)
                for k in ws:  # the windows themselves, whole, through the device Get
                    assert_bits_equal(host(sh.get(tdev(k, cuda))), ref.get(k), f"{knobs} window from {int(k[0])}")
                want = check_scalar(sh, ks, ref.get, f"{knobs} host get")
                for b in ks.boundaries:  # unwritten probes on both sides of every boundary
                    zero = (want == 0) & ~ks.touched
                    assert (zero & (ks.offs < b)).any() and (zero & (ks.offs >= b)).any()
                # the keys around the windows' ends were not written
                edge = np.array([2**31 - 1001, 2**31 + 1001, span - 5001, 2**30 - 8, 2**30 - 7 + 1027, 1024], dtype=np.uint32)
                assert_bits_equal(sh.get(edge), ref.get(edge), f"{knobs} beside the windows")
            finally:
                ref.close()
            back = np.unique(np.concatenate(wrote))
            sh.add(back, np.zeros(back.size, dtype=np.float32))
            assert not sh.get(back).any()
        assert held(cuda, before) < 20 * GIB, "a stamp array was made"
        assert sh.get_option("EPOCH") > 0
        sh.sync()


ACC_KNOBS = [{}, {"RB_APPLY_LOG2": 13}, {"RB_BIN_BLOCK": 512}]


def test_whole_key_space_accumulate(cuda):
    """int32 sums (exact): K6/K7 over windows across element index 2^31 and up
    to key 0xFFFFFFFF, aligned and not, and K5 (GENERAL = 2) with the RB_* sets of
    tests/test_fuzz.py on keys repeated across the bands."""
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    span = 1 << 32
    before = need(cuda, 17)
    ks, rng = scalar_keys("accumulate", 0, span, [2**30, 2**31, 3 * 2**30])
    ref = tf.AccRef(np.int32)
    wins = [(2**31 - 1000, 2001), (span - 8192, 8192), (2**30 - 7, 1027), (2**31 - 100, 20_001), (span - 3, 3)]
    vals = lambda n: rng.integers(-2**31, 2**31, size=n).astype(np.int32)  # noqa: E731
    with ps.Shard(0, span, np.int32, mode="accumulate", options={"GENERAL": 2}) as sh:
        sh.set_timing(True)
        for off in (0, 1):  # 16-byte aligned device buffers, and one element off
            ws = [(window(ks, lo, n), vals(n)) for lo, n in wins]
            sh.add_grouped([(tdev(k, cuda, off), tdev(v, cuda, off)) for k, v in ws], sorted_hint=True)
            for k, v in ws:
                ref.add(k, v)
            for k, _ in ws:
                ref.check(k, host(sh.get(tdev(k, cuda))), f"K7 window from {int(k[0])} offset {off}")
            edge = np.array([2**31 - 1001, 2**31 + 20_001 - 100, span - 8193, 2**30 - 8, 2**30 - 7 + 1027], dtype=np.uint32)
            ref.check(edge, sh.get(edge), "beside the windows")
        assert sh.kernel_time(_lib.PSKV_K_ACC_DENSE)["launches"] == 2
        for knobs in ACC_KNOBS:
            for name, v in {"RB_APPLY_LOG2": 0, "RB_BIN_BLOCK": 1024, **knobs}.items():
                sh.set_option(name, v)
            k = ks.draw(40_000)
            v = vals(k.size)
            sh.add(tdev(k, cuda), tdev(v, cuda))
            ref.add(k, v)
            # (a key no call wrote has no sum in the reference: it must read zero)
            ref.check(ks.all, host(sh.get(tdev(ks.all, cuda))), f"K5 {knobs}")
        assert sh.kernel_time(_lib.PSKV_K_RADIX)["launches"] >= len(ACC_KNOBS)
        held(cuda, before)
        sh.sync()


@pytest.mark.parametrize("base", ["low", "high"])
def test_scalar_shard_with_stamps_past_2_31(cuda, oracle_mod, base):
    """2^31 + 8192 float32 keys and their 17 GB of stamps: K4a/K4b (GENERAL = 0)
    and the replay behind a hint that does not hold, on keys around element
    index 2^31 (byte offset 2^33 of the parameters, 2^34 of the stamps) and
    around byte offset 2^32 of both arrays."""
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    span = 2**31 + 8192
    kb = 0 if base == "low" else 2**31 - 8192
    before = need(cuda, 25)
    ks, rng = scalar_keys(("stamps", base), kb, span, [2**29, 2**30, 2**31])
    ref = oracle_mod.MapStorageRef(np.float32)
    try:
        with ps.Shard(kb, kb + span, np.float32, options={"GENERAL": 0}) as sh:
            sh.set_timing(True)
            for c in range(2):
                k = ks.draw(6000)
                v = unique_rows(c, k.size, 1, np.float32).reshape(-1)
                sh.add(tdev(k, cuda), tdev(v, cuda))  # K4a / K4b
                ref.add(k, v)
                check_scalar(sh, ks, ref.get, f"K4 call {c}", cuda)
            assert sh.kernel_time(_lib.PSKV_K_GENERAL_COMMIT)["launches"] == 2
            assert held(cuda, before) > 24 * GIB, "no stamp array"
            for grouped in (False, True):  # a hint that does not hold: the replay
                ka, kc = ks.draw(3000), ks.draw(3000)
                va, vc = (unique_rows(7 + 2 * grouped + j, 3000, 1, np.float32).reshape(-1) for j in range(2))
                if grouped:
                    sh.add_grouped([(tdev(ka, cuda), tdev(va, cuda)), (tdev(kc, cuda), tdev(vc, cuda))], sorted_hint=True)
                    ref.add(ka, va)
                    ref.add(kc, vc)
                else:
                    sh.add(tdev(ka, cuda), tdev(va, cuda), sorted_hint=True)
                    ref.add(ka, va)
                check_scalar(sh, ks, ref.get, f"replay, grouped {grouped}")
            sh.sync()
    finally:
        ref.close()
