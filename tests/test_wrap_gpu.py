"""GPU tests of the stamp epoch's wrap-around (tests/wrap_util.py
has the seam's helpers).

Two kinds of cases.  The suite's seeded scenarios (scalar, row, sparse, growing
sparse, pooled-push and FTRL shards) run again on a Shard class that moves the
epoch to the wrap-around before every writing call, against the references
they always had, which know nothing about epochs.  The pointed cases put one
wrap-around exactly where a word of DESIGN.md §8o's table matters: the stamps
under a multi-group Add and a multi-group step, the stamps of a sparse shard
after a growth and an erase, the verification tag under a held replay and
under a K7 launch that has no replay behind it, the out-of-range tag, and the
sticky error word.
"""
import numpy as np
import pytest

import edge_util as eu
import opt_util as ou
import pooled_push_group_util as gu
import pooled_push_util as ppu
import sparse_grow_util as sgu
import sparse_util as su
import test_fuzz as tf
import test_ftrl_fuzz as tff
import test_pooled_push_fuzz as tppf
import test_pooled_push_grouped_fuzz as tppgf
import test_rows_fuzz as trf
import test_sparse_fuzz as tsf
import test_sparse_grow_fuzz as tsgf
import wrap_util as wu
from rows_util import RowOracle, ValueSource
from test_edge_gpu import check_edge_step, read_all, rows_of
from test_gpu_parity import assert_bits_equal, tdev
from test_opt_gpu import all_keys

pytestmark = pytest.mark.gpu

LAST = wu.LAST


def after(e0, groups):
    """The epoch `groups` launch groups after e0, each taken by itself."""
    e = e0
    for _ in range(groups):
        e = 1 if e == LAST else e + 1
    return e


# ====================================================== 1. option semantics
def test_epoch_option_semantics(cuda, monkeypatch):
    import parameter_server_amd as ps
    from parameter_server_amd import PskvError, _lib

    monkeypatch.setenv("PSKV_EPOCH", "77")  # no environment default
    k = np.arange(500, dtype=np.uint32)
    with ps.Shard(0, 1000, np.float32) as sh:
        assert wu.epoch(sh) == 0
        sh.add(tdev(k, cuda), tdev(k.astype(np.float32), cuda))
        e = wu.epoch(sh)
        assert e == 1
        sh.set_option("EPOCH", e)  # the current value is a valid one
        sh.set_option("EPOCH", e + 10)
        assert wu.epoch(sh) == e + 10
        for bad in (e + 9, 0, -1, LAST + 1, 1 << 40):
            with pytest.raises(PskvError) as ei:
                sh.set_option("EPOCH", bad)
            assert ei.value.code == _lib.PSKV_EINVAL
            assert wu.epoch(sh) == e + 10
        sh.add(tdev(k, cuda), tdev(k.astype(np.float32) + 1, cuda))
        assert wu.epoch(sh) == e + 11
        sh.set_option("EPOCH", LAST)
        assert wu.epoch(sh) == LAST
        with pytest.raises(PskvError):
            sh.set_option("EPOCH", LAST - 1)
        sh.add(tdev(k, cuda), tdev(k.astype(np.float32) + 2, cuda))
        assert wu.epoch(sh) == 1  # the wrap-around
        assert np.array_equal(sh.get(k), k.astype(np.float32) + 2)
        sh.sync()


# ====================================== 2. the suite's scenarios, epoch moved
@pytest.fixture
def moved(monkeypatch):
    """install(**kw) puts wrap_util's class in the place of parameter_server_amd.Shard."""
    import parameter_server_amd as ps

    base = ps.Shard

    def install(**kw):
        stats = kw.pop("stats", None) or wu.Stats()
        monkeypatch.setattr(ps, "Shard", wu.wrapping_shard_class(base, stats=stats, **kw))
        return stats

    return install


def groups_of(n, size):
    return [pytest.param(range(a, min(a + size, n)), id=f"{a}-{min(a + size, n) - 1}") for a in range(0, n, size)]


@pytest.mark.parametrize("seeds", groups_of(57, 6))  # every knob of test_fuzz.KNOBS three times
def test_scalar_scenarios(cuda, oracle_mod, moved, seeds):
    """test_fuzz's scenarios (every scalar Add path, host and device, right and
    wrong hints, single and multi-group, add_get with the replay folded and
    not, overflow keys) against its oracle; where the scenario is
    deterministic (assign, or int32 sums) also reply by reply against the same
    scenario without the moves."""
    wraps = 0
    for seed in seeds:
        _, dt, mode, kb, ke, knobs = tf._scenario(seed)
        runs = []
        for schedule in (wu.SCHEDULE, None):
            if schedule is None and not (mode == "assign" or dt is np.int32):
                continue
            rec = []
            stats = moved(schedule=schedule, record=rec)
            rng = tf._scenario(seed)[0]
            tf._run(cuda, oracle_mod, seed, rng, dt, mode, kb, ke, knobs)
            runs.append(rec)
            wraps += stats.wraps
        if len(runs) == 2:
            wu.same_records(runs[0], runs[1], f"seed {seed}: with the epoch moved against without")
    assert wraps >= len(seeds), f"{wraps} wrap-arounds in {len(seeds)} scenarios: the moves do not reach the shards"


@pytest.mark.parametrize("seeds", groups_of(40, 10))
def test_row_scenarios(cuda, oracle_mod, moved, seeds):
    stats = moved()
    for seed in seeds:
        trf.scenario(seed, cuda, oracle_mod)
    assert stats.wraps >= len(seeds)


@pytest.mark.parametrize("seeds", groups_of(40, 10))
def test_sparse_scenarios(cuda, oracle_mod, moved, seeds):
    """The sparse shard wraps; its dense twin (optimizer scenarios) never does."""
    stats = moved(only_sparse=True)
    for seed in seeds:
        if seed % 2 == 0:
            tsf.storage_scenario(seed, cuda, oracle_mod)
        else:
            tsf.optimizer_scenario(seed, cuda)
    assert stats.wraps >= len(seeds)


@pytest.mark.parametrize("seeds", groups_of(40, 10))
def test_growing_sparse_scenarios(cuda, moved, seeds):
    """Reserve, automatic growth and erase between the wrap-arounds."""
    stats = moved(only_sparse=True)
    for seed in seeds:
        sc = sgu.draw_scenario(seed)
        if sc["kind"] == "storage":
            tsgf.storage_scenario(sc, cuda)
        else:
            tsgf.optimizer_scenario(sc, cuda)
    assert stats.wraps >= len(seeds)


@pytest.mark.parametrize("seeds", groups_of(40, 10))
def test_pooled_push_scenarios(cuda, moved, seeds):
    stats = moved()
    for seed in seeds:
        tppf.scenario(seed, cuda)
    assert stats.wraps >= len(seeds)


@pytest.mark.parametrize("seeds", groups_of(30, 10))
def test_grouped_pooled_push_scenarios(cuda, moved, seeds):
    stats = moved()
    for seed in seeds:
        tppgf.scenario(seed, cuda)
    assert stats.wraps >= len(seeds)


@pytest.mark.parametrize("seeds", groups_of(20, 5))
def test_ftrl_scenarios(cuda, moved, seeds):
    stats = moved()
    for seed in seeds:
        tff.test_scenario(cuda, seed)
    assert stats.wraps >= len(seeds)


# ============================= 3. a multi-group Add with the wrap between groups
ADD_PATHS = ["stamps", "radix", "hint_holds", "hint_broken", "host", "unaligned"]


@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("path", ADD_PATHS)
def test_multi_group_assign_add_across_the_wrap(cuda, oracle_mod, path, d):
    """65 batches are two launch groups; batch 64 repeats batch 0's keys, so one
    key set lies in both, and every call draws from the same 300 keys (two of
    them outside the range, in the overflow table)."""
    import parameter_server_amd as ps

    kb, ke = 1000, 1298
    pool = np.concatenate([np.arange(kb, ke), [ke + 5, 0xFFFFFFF0]]).astype(np.uint32)
    rng = np.random.default_rng(ou.case_seed("wrap-add", path, d))
    src = ValueSource(np.float32, "assign", rng)
    options = {"stamps": {"GENERAL": 0}, "radix": {"GENERAL": 2}}.get(path)
    ref = oracle_mod.MapStorageRef(np.float32)

    def call(sh):
        batches = []
        for _ in range(65):
            if path == "hint_holds":  # strictly increasing, in range
                k = np.sort(rng.choice(pool[:-2], size=40, replace=False))
            else:
                k = rng.choice(pool, size=40)
            batches.append(k)
        batches[64] = batches[0].copy()
        batches = [(k, src.rows(k.size, 1).reshape(-1)) for k in batches]
        e0 = wu.epoch(sh)
        if path == "host":
            sh.add_grouped(batches)
        else:
            off = 1 if path == "unaligned" else 0
            sh.add_grouped([(tdev(k, cuda, off), tdev(v, cuda, off)) for k, v in batches],
                           sorted_hint=path.startswith("hint"))
        for k, v in batches:
            ref.add(k, v)
        assert_bits_equal(sh.get(pool), ref.get(pool), f"{path} d {d} from epoch {e0:#x}")
        return e0

    try:
        with ps.Shard(kb, ke, np.float32, overflow_slots=64, options=options) as sh:
            call(sh)  # the prefix, at small epochs
            assert wu.near_wrap(sh, d)
            e0 = call(sh)
            if path != "host":  # (host batches are staged together: their groups are the staging's)
                assert wu.epoch(sh) == after(e0, 2), "two launch groups"
            call(sh)
            call(sh)
            assert wu.epoch(sh) < 16
            sh.sync()
    finally:
        ref.close()


# ================================== 4. the held replay of pskv_add_get_grouped
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("hint_holds", [False, True], ids=["broken", "holds"])
@pytest.mark.parametrize("fold", [1, 0])
def test_add_get_across_the_wrap(cuda, oracle_mod, fold, hint_holds, d):
    """d = 1: the call after the move holds its replay at the last epoch
    (pend_epoch = 0xFFFFFFFF) and the next call is the first after the wrap;
    d = 2 and d = 0 put the wrap one call later and earlier.  Every pull is
    read through the call's own Get and through a later one."""
    import torch

    import parameter_server_amd as ps

    kb, ke = 5000, 5000 + 3000
    pool = np.concatenate([np.arange(kb, ke), [7, ke + 9]]).astype(np.uint32)
    rng = np.random.default_rng(ou.case_seed("wrap-addget", fold, hint_holds, d))
    src = ValueSource(np.float32, "assign", rng)
    ref = oracle_mod.MapStorageRef(np.float32)

    def call(sh, what):
        adds = []
        for _ in range(3):
            if hint_holds:
                k = np.sort(rng.choice(pool[:-2], size=1200, replace=False))
            else:
                k = rng.choice(pool, size=1200)  # unsorted, repeated and out-of-range keys: the replay runs
            adds.append((k, src.rows(k.size, 1).reshape(-1)))
        qs = [adds[0][0][:700].copy(), pool.copy()]
        outs = [torch.empty(q.size, dtype=torch.float32, device=cuda) for q in qs]
        sh.add_get_grouped([(tdev(k, cuda), tdev(v, cuda)) for k, v in adds],
                           [(tdev(q, cuda), o) for q, o in zip(qs, outs)], sorted_hint=True)
        for k, v in adds:
            ref.add(k, v)
        for q, o in zip(qs, outs):
            assert_bits_equal(o.cpu().numpy(), ref.get(q), f"{what}: the call's own Get")
        assert_bits_equal(sh.get(pool), ref.get(pool), f"{what}: a later Get")

    try:
        with ps.Shard(kb, ke, np.float32, overflow_slots=64, options={"FOLD_REPLAY": fold}) as sh:
            call(sh, "prefix 0")
            call(sh, "prefix 1")
            assert wu.near_wrap(sh, d)
            for i in range(3):
                e0 = wu.epoch(sh)
                call(sh, f"d {d} call {i} from epoch {e0:#x}")
                assert wu.epoch(sh) == after(e0, 1), "one launch group"
            assert wu.epoch(sh) == 3 - d
            sh.sync()
    finally:
        ref.close()


# ============================ 4b. a scalar shard's accumulate paths, int32 sums
ACC_PATHS = ["k5", "k4a_stamps", "k7_aligned", "k7_unaligned", "k7_host", "lookalike", "inline", "serve"]


@pytest.mark.parametrize("path", ACC_PATHS)
def test_accumulate_paths_across_the_wrap(cuda, path):
    """The selectors of test_edge_gpu's dense accumulate cases; the same call
    shape at small epochs, then with 0, 1 and 2 epochs left, on the same keys
    (two of them in the overflow table), the sums exact (int32).  The K7 paths
    read the verification tag, K4a writes the out-of-range tag; K5, the inline
    path and the request server use no epoch, and must not mind the moves."""
    import parameter_server_amd as ps

    rng = np.random.default_rng(ou.case_seed("wrap-acc", path))
    kb, rows = 1000, 40_000
    ke = kb + rows
    extra = np.array([ke + 7, 0xFFFFFFF0], dtype=np.uint32)
    options = {"k4a_stamps": {"GENERAL": "stamps"}, "k5": {"GENERAL": 2}, "inline": {"INLINE_ADD_CHUNKS": 8},
               "serve": {"SERVE": 1}}.get(path)
    windows = path.startswith("k7") or path == "lookalike"
    q = np.concatenate([all_keys(kb, ke), extra])
    ref = tf.AccRef(np.int32)
    vals = lambda n: rng.integers(-2**31, 2**31, size=n).astype(np.int32)  # noqa: E731

    def call(sh):
        if windows:
            batches = []
            for n in (1, 3, 1000, 8191, 8192, 20_001):
                first = kb + int(rng.integers(0, rows - n + 1))
                if path != "k7_unaligned":
                    first -= (first - kb) % 4
                batches.append(np.arange(first, first + n, dtype=np.int64).astype(np.uint32))
            batches.append(batches[-1][5000:15_000].copy())  # overlaps the window before it
            if path == "lookalike":  # still sorted at its ends: two keys swapped, one repeated
                k = batches[3]
                k[10], k[11] = k[11], k[10]
                k[500] = k[499]
            batches = [(k, vals(k.size)) for k in batches]
            if path == "k7_host":
                sh.add_grouped(batches)
            else:
                off = 1 if path == "k7_unaligned" else 0
                sh.add_grouped([(tdev(k, cuda, off), tdev(v, cuda, off)) for k, v in batches], sorted_hint=True)
        elif path in ("inline", "serve"):
            batches = []
            for _ in range(4):
                k = q[rng.integers(0, 600, size=2048 if path == "inline" else 256)]
                k[:2] = extra
                batches.append((k, vals(k.size)))
                sh.add(*batches[-1])
        else:
            k = q[rng.integers(0, q.size, size=45_000)]
            k[:4000] = q[7]  # a hot key
            batches = [(k, vals(k.size))]
            sh.add(tdev(k, cuda), tdev(batches[0][1], cuda))
        for k, v in batches:
            ref.add(k, v)
        ref.check(q, sh.get(q), f"{path} at epoch {wu.epoch(sh):#x}")

    with ps.Shard(kb, ke, np.int32, mode="accumulate", overflow_slots=64, options=options) as sh:
        call(sh)
        for d in (0, 1, 2, 0):
            # (the inline path and the request server take no epochs: once at the last one the shard stays there)
            assert wu.near_wrap(sh, d) or path in ("inline", "serve")
            call(sh)
            call(sh)
        sh.sync()


# ================================== 5. the verification tag and the oor tag
@pytest.mark.parametrize("e", [1, 3])
@pytest.mark.parametrize("path", ["k7_host", "k7_device", "k2_device", "k2g_device"])
def test_no_spurious_replay_after_the_wrap(cuda, oracle_mod, path, e):
    """A broken hint at epoch e leaves the tag e in flag[0].  After the wrap a
    call runs at epoch e again: K7 launched for host windows (nothing behind
    it) must not skip, and a hinted device call whose hint holds must give the
    right values without its replay running.  The replay's launch is queued
    either way (it decides on the device), so n_general_launches cannot tell;
    its time can: one workgroup replaying n keys takes 1 Ki keys per pass, an
    idle one reads a word.  Three launches of the same batches are timed: at
    epoch e after the wrap, at the next epoch, and with the hint broken on
    purpose; the first two must each stay below a quarter of the third (the
    replay of 800 passes against a launch that reads one word; measured on an
    MI355X: 1.36 to 1.60 ms against 0.004 to 0.008 ms)."""
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, rows, n = 64, 1_000_000, 800_000
    ke = kb + rows
    acc = path.startswith("k7")
    dt = np.int32 if acc else np.float32  # int32 sums are exact in any order
    rng = np.random.default_rng(ou.case_seed("wrap-flag", path, e))
    ref = tf.AccRef(np.int32) if acc else oracle_mod.MapStorageRef(dt)
    small = np.arange(kb, kb + 512, dtype=np.uint32)
    big = np.arange(kb + 1000, kb + 1000 + n, dtype=np.uint32)  # a window: sorted, dense, distinct
    check_keys = np.concatenate([small, big[:4096], big[-4096:]])

    def vals(k):
        return rng.integers(-1000, 1000, size=k.size).astype(dt)

    def dev_add(sh, k, v, hint=True):
        if path == "k2g_device" or (acc and path == "k7_device"):
            h = k.size // 2
            sh.add_grouped([(tdev(k[:h], cuda), tdev(v[:h], cuda)), (tdev(k[h:], cuda), tdev(v[h:], cuda))],
                           sorted_hint=hint)
        else:
            sh.add(tdev(k, cuda), tdev(v, cuda), sorted_hint=hint)
        ref.add(k, v)

    def filler(sh):  # one launch group, hint holds
        v = vals(small)
        dev_add(sh, small, v)

    def replay_ms(sh):
        sh.sync()
        return sh.kernel_time(_lib.PSKV_K_REPLAY)["total_ms"]

    try:
        with ps.Shard(kb, ke, dt, mode="accumulate" if acc else "assign") as sh:
            for _ in range(e - 1):
                filler(sh)
            broken = small[::-1].copy()  # decreasing: the hint is wrong, the verification tags flag[0] = e
            dev_add(sh, broken, vals(broken))
            assert wu.epoch(sh) == e
            assert wu.near_wrap(sh, 0)
            for _ in range(e - 1):
                filler(sh)
            assert wu.epoch(sh) == (e - 1 if e > 1 else LAST)
            v = vals(big)
            if path == "k7_host":
                h = n // 2
                sh.add_grouped([(big[:h], v[:h]), (big[h:], v[h:])])  # the CPU proves the windows: K7 alone
                ref.add(big, v)
            else:
                sh.set_timing(True, kernels=[_lib.PSKV_K_REPLAY])
                sh.reset_timing()
                dev_add(sh, big, v)
                at_e = replay_ms(sh)
            assert wu.epoch(sh) == e
            got = sh.get(check_keys)
            if acc:
                ref.check(check_keys, got, f"{path} at epoch {e} after the wrap")
            else:
                assert_bits_equal(got, ref.get(check_keys), f"{path} at epoch {e} after the wrap")
            if path != "k7_host":
                sh.reset_timing()
                dev_add(sh, big, vals(big))
                clean = replay_ms(sh)
                swapped = big.copy()
                swapped[[10, 11]] = swapped[[11, 10]]
                sh.reset_timing()
                dev_add(sh, swapped, vals(big))
                forced = replay_ms(sh)
                print(f"replay launch ms: at epoch {e} after the wrap {at_e:.4f}, next epoch {clean:.4f}, "
                      f"hint broken {forced:.4f}")
                assert clean < forced / 4, "the replay's time does not tell an idle launch from a running one"
                assert at_e < forced / 4, "the replay ran at the epoch of a tag from before the wrap"
                got = sh.get(check_keys)
                if acc:
                    ref.check(check_keys, got, "after the timed calls")
                else:
                    assert_bits_equal(got, ref.get(check_keys), "after the timed calls")
            sh.sync()
    finally:
        if not acc:
            ref.close()


@pytest.mark.parametrize("e", [1, 2])
def test_no_spurious_sticky_error_after_the_wrap(cuda, oracle_mod, e):
    """A device call drops an out-of-range row at epoch e (PSKV_ESTATE at sync,
    cleared); after the wrap a clean call at epoch e must leave sync clean."""
    import parameter_server_amd as ps
    from parameter_server_amd import PskvError, _lib

    kb, ke, w = 100, 100 + 3000, 3
    keys_all = all_keys(kb, ke)
    rng = np.random.default_rng(ou.case_seed("wrap-sticky", e))
    src = ValueSource(np.float32, "assign", rng)
    orc = RowOracle(oracle_mod, np.float32, "assign", w, kb, ke)

    def dev_add(sh, k, note=True):
        v = src.rows(k.size, w)
        sh.add(tdev(k, cuda), tdev(v, cuda))
        if note:
            orc.add(k, v)

    try:
        with ps.Shard(kb, ke, np.float32, width=w) as sh:
            for _ in range(e - 1):
                dev_add(sh, keys_all[rng.integers(0, ke - kb, size=2049)])
            bad = keys_all[rng.integers(0, ke - kb, size=2049)]
            bad[77] = ke + 1
            dev_add(sh, bad, note=False)
            assert wu.epoch(sh) == e
            with pytest.raises(PskvError) as ei:
                sh.sync()
            assert ei.value.code == _lib.PSKV_ESTATE
            sh.clear()
            sh.sync()
            dev_add(sh, keys_all)  # the refill
            assert wu.near_wrap(sh, 0)
            for _ in range(e):
                dev_add(sh, keys_all[rng.integers(0, ke - kb, size=2049)])
            assert wu.epoch(sh) == e
            sh.sync()  # PSKV_OK
            orc.check(keys_all, sh.get(keys_all), f"epoch {e} after the wrap")
            sh.sync()
    finally:
        for c in orc.cols:
            c.close()


@pytest.mark.parametrize("e", [1, 2])
def test_out_of_range_tag_after_the_wrap(cuda, oracle_mod, e):
    """K4a's out-of-range tag (flag[1]) of epoch e, then Adds at epoch e after
    the wrap, without and with out-of-range keys: the overflow table holds
    what the oracle holds."""
    import parameter_server_amd as ps

    kb, ke = 100, 100 + 3000
    pool = np.concatenate([all_keys(kb, ke), [5, ke + 3, 0xFFFFFFFF]]).astype(np.uint32)
    rng = np.random.default_rng(ou.case_seed("wrap-oor", e))
    src = ValueSource(np.float32, "assign", rng)
    ref = oracle_mod.MapStorageRef(np.float32)

    def dev_add(sh, k):
        v = src.rows(k.size, 1).reshape(-1)
        sh.add(tdev(k, cuda), tdev(v, cuda))
        ref.add(k, v)

    try:
        with ps.Shard(kb, ke, np.float32, overflow_slots=64, options={"GENERAL": 0}) as sh:
            for _ in range(e):
                dev_add(sh, rng.choice(pool, size=2049))  # out-of-range keys among them
            assert wu.epoch(sh) == e
            for with_oor in (False, True):
                assert wu.near_wrap(sh, 0)
                for _ in range(e):
                    dev_add(sh, rng.choice(pool if with_oor else pool[:-3], size=2049))
                assert wu.epoch(sh) == e
                assert_bits_equal(sh.get(pool), ref.get(pool), f"epoch {e} after the wrap, oor {with_oor}")
            sh.sync()
    finally:
        ref.close()


# ===================== 6. multi-group steps: the wrap is taken before the first
STEP_DS = [None, 2, 1, 0, 3]  # None: the prefix at small epochs


def _step_shape(kind):
    i = eu.KINDS.index(kind)
    return [1, 3, 4][i % 3], [np.float32, np.float64][i % 2]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("kind", eu.KINDS)
def test_grouped_step_across_the_wrap(cuda, kind, device):
    """pskv_apply_grouped of 65 batches (two launch groups) with 2, 1 and 0
    epochs left before the wrap, batch 64 on batch 0's keys; then a plain step
    on the same keys, which would see a stamp that outlived the wrap (the key
    takes no step) and a gradient scratch that was not put back to zero.  p,
    every state slot and the step counter after each."""
    import parameter_server_amd as ps

    w, dt = _step_shape(kind)
    kb, ke = 100, 140
    hp = eu.kind_hyper(kind)
    rng = np.random.default_rng(ou.case_seed("wrap-step", kind, device))
    keys_all = all_keys(kb, ke)
    grads = lambda n: (rng.standard_normal((n, w)) * 3).astype(dt)  # noqa: E731
    with ps.Shard(kb, ke, dt, width=w) as sh:
        eu.set_optimizer(sh, hp)
        sh.add(keys_all, rng.standard_normal((ke - kb, w)).astype(dt))
        steps = 0
        for d in STEP_DS:
            batches = [((kb + rng.integers(0, 12, size=3)).astype(np.uint32), grads(3)) for _ in range(65)]
            batches[64] = (batches[0][0].copy(), batches[64][1])
            cat_k = np.concatenate([k for k, _ in batches])
            cat_g = np.concatenate([g for _, g in batches])
            if d is not None:
                assert wu.near_wrap(sh, d)
            e0 = wu.epoch(sh)
            sent = [(tdev(k, cuda), tdev(g, cuda)) for k, g in batches] if device else batches
            check_edge_step(sh, keys_all, cat_k.astype(np.int64) - kb, cat_g, hp, lambda: sh.apply_grouped(sent),
                            f"{kind} d {d} grouped")
            if device:  # the whole call on one side of the wrap: with fewer than two epochs left it starts at 1
                assert wu.epoch(sh) == (2 if LAST - e0 < 2 else e0 + 2)
            k2, g2 = cat_k[::2].copy(), grads(cat_k[::2].size)
            e1 = wu.epoch(sh)
            check_edge_step(sh, keys_all, k2.astype(np.int64) - kb, g2, hp,
                            lambda: sh.apply(tdev(k2, cuda), tdev(g2, cuda)) if device else sh.apply(k2, g2),
                            f"{kind} d {d} the step after")
            if device:
                assert wu.epoch(sh) == after(e1, 1)
            steps += 2
            assert sh.step == steps
        sh.sync()


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("kind,nesterov", ppu.KINDS)
def test_grouped_pooled_push_across_the_wrap(cuda, kind, nesterov, device):
    """pskv_apply_pooled_grouped of more batches than one launch group holds."""
    import parameter_server_amd as ps

    i = ppu.KINDS.index((kind, nesterov))
    w, dt = [1, 3, 4][i % 3], np.dtype([np.float32, np.float64][i % 2])
    kb, ke = 2**31 - 30, 2**31 + 30
    hp = ppu.hyper(kind, nesterov, wd=0.01)
    ns = ou.SLOTS[kind]
    nb = gu.MAX_POOL_BATCHES + 2
    rng = np.random.default_rng(ou.case_seed("wrap-pooled", kind, nesterov, device))
    keys_all = all_keys(kb, ke)
    with ps.Shard(kb, ke, dt, width=w) as sh:
        ppu.set_optimizer(sh, hp)
        sh.add(keys_all, rng.standard_normal((ke - kb, w)).astype(dt))
        steps = 0
        for d in STEP_DS:
            batches = gu.draw_group(rng, [9] * nb, w, kb, ke, dt, c=steps)
            if d is not None:
                assert wu.near_wrap(sh, d)
            e0 = wu.epoch(sh)
            p, slots = read_all(sh, keys_all, ns)
            gu.apply_grouped(sh, batches, cuda if device else None)
            steps += 1
            pn, sn = read_all(sh, keys_all, ns)
            gu.check_step(p, slots, kb, batches, pn, sn, dt, hp, t=steps, msg=f"{kind} d {d} grouped push")
            if device:
                assert wu.epoch(sh) == (2 if LAST - e0 < 2 else e0 + 2)
            # the step after, on the same keys: a plain pooled push
            keys, off, bg, wts = batches[0]
            ppu.apply_pooled(sh, keys, off, bg, wts, cuda if device else None)
            steps += 1
            p2, s2 = read_all(sh, keys_all, ns)
            ppu.check_step(pn, sn, keys.astype(np.int64) - kb, wts, bg, ppu.bag_index(off), p2, s2, dt, hp, t=steps,
                           msg=f"{kind} d {d} the push after")
            assert sh.step == steps
        sh.sync()


# ================== 7. a sparse shard's stamps after a growth and after an erase
@pytest.mark.parametrize("kind", [None, "momentum", "ftrl"], ids=["assign", "momentum", "ftrl"])
@pytest.mark.parametrize("shape", ["reserve", "erase"])
def test_sparse_stamps_follow_the_capacity(cuda, oracle_mod, shape, kind):
    """Stamps on (almost) every slot of the capacity the shard has AFTER its
    rebuild, at epochs just below the wrap; then the wrap, and the same keys
    written again.  A reset sized by the capacity from before the rebuild
    leaves the stamps of the upper slots in place, and those keys take nothing
    any more."""
    import parameter_server_amd as ps

    w, dt = 3, np.dtype(np.float32)
    small, large = 64, 4096
    rng = np.random.default_rng(ou.case_seed("wrap-sparse", shape, kind))
    pool = su.key_pool(rng, large - 5)  # a count near the capacity
    src = ValueSource(dt, "assign", rng)
    orc = RowOracle(oracle_mod, dt, "assign", w, 0, 1 << 32)
    hp = eu.kind_hyper(kind) if kind else None

    def write(sh, k, device):
        """An assign Add, or a step checked from the shard's own state before it."""
        if kind is None:
            v = src.rows(k.size, w)
            sh.add(tdev(k, cuda), tdev(v, cuda)) if device else sh.add(k, v)
            orc.add(k, v)
            orc.check(pool, rows_of(sh.get(pool), w), f"{shape} after an Add at epoch {wu.epoch(sh):#x}")
            return
        g = (rng.standard_normal((k.size, w)) * 3).astype(dt)
        idx = np.searchsorted(sorted_pool, k)
        check_edge_step(sh, sorted_pool, idx, g, hp,
                        lambda: sh.apply(tdev(k, cuda), tdev(g, cuda)) if device else sh.apply(k, g),
                        f"{shape} {kind} step at epoch {wu.epoch(sh):#x}")

    sorted_pool = np.sort(pool)
    try:
        with ps.Shard.sparse(small if shape == "reserve" else large, dt, "assign", width=w) as sh:
            if kind:
                eu.set_optimizer(sh, hp)
            first = pool[:small - 4] if shape == "reserve" else pool
            v = src.rows(first.size, w)
            sh.add(tdev(first, cuda), tdev(v, cuda))  # stamps exist from here on
            orc.add(first, v)
            if shape == "reserve":
                sh.reserve(large)
                rest = pool[small - 4:]
                v = src.rows(rest.size, w)
                sh.add(tdev(rest, cuda), tdev(v, cuda))
                orc.add(rest, v)
            else:
                gone = pool[rng.permutation(pool.size)[:1000]]
                sh.erase(tdev(gone, cuda))
                z = np.zeros((gone.size, w), dtype=dt)
                orc.add(gone, z)  # an erased key reads as zeros, and is stored again below
                sh.add(gone, z)
            assert sh.sparse_info()["capacity"] == large and sh.sparse_info()["count"] == pool.size
            assert wu.near_wrap(sh, 1)
            write(sh, pool, True)      # the last epoch: a stamp on every stored slot
            assert wu.epoch(sh) == LAST
            write(sh, pool[::-1].copy(), True)   # the first after the wrap
            assert wu.epoch(sh) == 1
            write(sh, pool[rng.integers(0, pool.size, size=2049)], False)
            sh.sync()
    finally:
        for c in orc.cols:
            c.close()
