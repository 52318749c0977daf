"""GPU tests of row-valued shards (a fixed-width vector of values per key)
against the per-column oracle of tests/rows_util.py: column j of a width-W
shard behaves exactly like the reference storage fed (keys, vals[:, j]).

Bar: assign bit-exact, int32 accumulate exact, float accumulate within
    |gpu - ref64| <= 1.01 (m + 1) u (|p0| + sum|v_i|)
(tests/test_gpu_parity.py's bound; it holds for any summation order).
Pushed assign values are unique per (occurrence, column): a mixed row or a
wrong winner cannot compare equal.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

from rows_util import LAYOUTS, WIDTHS, RowOracle, ValueSource, key_patterns
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.int32, np.float32, np.float64]
MODES = ["assign", "accumulate"]
COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 4100]
# every tuning option of the pskv.h list, with a non-default value
OPTIONS = {"GENERAL": 2, "UNROLL": 4, "GET_UNROLL": 8, "NT": 0, "NTP": 0, "EARLY": 1, "PAGEABLE_DMA": 0,
           "DMA_MIN_BYTES": 0, "DMA_MIN_BYTES_GET": 0, "DMA_MIN_BYTES_PINNED": 0, "ZC_MAX_BYTES": 0,
           "FRAME_ZC_MAX_BYTES": 0, "INLINE": 0, "INLINE_ADD_CHUNKS": 4, "INLINE_GET_CHUNKS": 4, "ISPIN": 0,
           "SERVE": 1, "SERVE_IDLE_US": 100, "TILE_SHIFT": 12, "TILE_GRID": 1024, "RB_WBITS": 12, "RB_NBD": 7,
           "RB_TB": 8, "RB_APPLY_LOG2": 13, "RB_BIN_BLOCK": 512, "FOLD_REPLAY": 0,
           "SYNC_TIMEOUT_MS": 60000}


def rand_keys(rng, n, kb, ke, dup=True):
    hi = kb + max(1, (ke - kb) // 3) if dup else ke
    return rng.integers(kb, hi, size=n).astype(np.uint32)


def dget(sh, keys, cuda, offset=0):
    """Device Get; offset > 0: the output starts `offset` elements into a larger
    buffer (not 16-byte aligned: the element path)."""
    import torch

    dk = tdev(keys, cuda, offset)
    out = None
    if offset:
        from parameter_server_amd.shard import _torch_dtype

        buf = torch.empty(keys.size * sh.width + offset, dtype=_torch_dtype(sh.dtype), device=cuda)
        out = buf[offset:].view(keys.size, sh.width) if sh.width > 1 else buf[offset:]
    got = sh.get(dk, out=out)
    return got.cpu().numpy()


def run_every_path(sh, orc, src, rng, cuda, sizes):
    """Every entry point once, host and device, each Get checked at once."""
    kb, ke, w = orc.kb, orc.ke, orc.w
    size = itertools.cycle(sizes)
    # host add / get
    k = rand_keys(rng, next(size), kb, ke)
    v = src.rows(k.size, w)
    sh.add(k, v if rng.random() < 0.5 else v.reshape(-1))
    orc.add(k, v)
    q = rand_keys(rng, next(size), kb, ke, dup=False)
    orc.check(q, sh.get(q), "host get")
    # device add / get
    k = rand_keys(rng, next(size), kb, ke)
    v = src.rows(k.size, w)
    sh.add(tdev(k, cuda), tdev(v, cuda))
    orc.add(k, v)
    orc.check(q, dget(sh, q, cuda), "device get")
    # device views one element off alignment
    k = rand_keys(rng, next(size), kb, ke)
    v = src.rows(k.size, w)
    dv = tdev(v.reshape(-1), cuda, 1)
    sh.add(tdev(k, cuda, 1), dv.view(k.size, w) if w > 1 else dv)
    orc.add(k, v)
    orc.check(q, dget(sh, q, cuda, offset=1), "unaligned device get")
    # grouped, with an empty batch and a 1-key batch, duplicates across batches
    for device in (False, True):
        ks = [rand_keys(rng, n, kb, ke) for n in (next(size), 0, 1, next(size))]
        m = min(5, ks[0].size, ks[3].size)
        ks[3][:m] = ks[0][:m]
        vs = [src.rows(x.size, w) for x in ks]
        if device:
            sh.add_grouped([(tdev(a, cuda), tdev(b, cuda)) for a, b in zip(ks, vs)])
        else:
            sh.add_grouped(list(zip(ks, vs)))
        for a, b in zip(ks, vs):
            orc.add(a, b)
        qs = [rand_keys(rng, n, kb, ke, dup=False) for n in (1, next(size), 0)]
        if device:
            import torch

            outs = [torch.empty((x.size, w) if w > 1 else x.size, dtype=tdev(vs[0], cuda).dtype, device=cuda)
                    for x in qs]
            sh.get_grouped([(tdev(a, cuda), o) for a, o in zip(qs, outs)])
            outs = [o.cpu().numpy() for o in outs]
        else:
            outs = [np.empty((x.size, w) if w > 1 else x.size, dtype=orc.dt) for x in qs]
            sh.get_grouped(list(zip(qs, outs)))
        for a, o in zip(qs, outs):
            orc.check(a, o, f"get_grouped device={device}")
    # add_get_grouped: the Get sees the Add of the same call
    for device in (False, True):
        ks = [rand_keys(rng, n, kb, ke) for n in (next(size), 1, 0)]
        vs = [src.rows(x.size, w) for x in ks]
        qs = [ks[0].copy(), rand_keys(rng, next(size), kb, ke, dup=False)]
        if device:
            import torch

            outs = [torch.empty((x.size, w) if w > 1 else x.size, dtype=tdev(vs[0], cuda).dtype, device=cuda)
                    for x in qs]
            sh.add_get_grouped([(tdev(a, cuda), tdev(b, cuda)) for a, b in zip(ks, vs)],
                               [(tdev(a, cuda), o) for a, o in zip(qs, outs)])
            outs = [o.cpu().numpy() for o in outs]
        else:
            outs = [np.empty((x.size, w) if w > 1 else x.size, dtype=orc.dt) for x in qs]
            sh.add_get_grouped(list(zip(ks, vs)), list(zip(qs, outs)))
        for a, b in zip(ks, vs):
            orc.add(a, b)
        for a, o in zip(qs, outs):
            orc.check(a, o, f"add_get_grouped device={device}")
    sh.sync()


@pytest.mark.parametrize("layout", LAYOUTS, ids=["low", "mid"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_path_matches_the_per_column_oracle(cuda, oracle_mod, dtype, mode, width, layout):
    import parameter_server_amd as ps

    kb, ke = layout
    rng = np.random.default_rng(width * 1000 + kb % 977)
    orc = RowOracle(oracle_mod, dtype, mode, width, kb, ke)
    src = ValueSource(dtype, mode, rng)
    with ps.Shard(kb, ke, dtype, mode=mode, width=width) as sh:
        q = orc.all_keys()
        got = sh.get(q)  # never written: all-zero bits
        assert not np.ascontiguousarray(got).view(np.uint8).any()
        assert got.shape == ((q.size, width) if width > 1 else (q.size,))
        run_every_path(sh, orc, src, rng, cuda, [700, 65, 2049, 300, 1, 64])
        # the whole array
        orc.check(q, sh.dense_view().cpu().numpy(), "dense_view")
        assert tuple(sh.dense_view().shape) == ((ke - kb, width) if width > 1 else (ke - kb,))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mode", MODES)
def test_width_one_is_the_scalar_shard(cuda, oracle_mod, dtype, mode):
    """Shard(width=1) and a Shard made the old way give the same bits on the same calls."""
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[0]
    rng = np.random.default_rng(3)
    with ps.Shard(kb, ke, dtype, mode=mode, width=1) as a, ps.Shard(kb, ke, dtype, mode=mode) as b:
        assert a.info()["width"] == b.info()["width"] == 1
        for n in (1, 300, 2049):
            k = np.sort(rand_keys(rng, n, kb, ke))  # sorted: both shards sum in the same (K7) order
            v = rng.integers(-1000, 1000, size=n).astype(dtype)
            for sh in (a, b):
                sh.add(k, v)
                sh.add(tdev(k, cuda), tdev(v, cuda), sorted_hint=True)
        q = np.arange(kb, ke, dtype=np.uint32)
        ga, gb = a.get(q), b.get(q)
        assert ga.shape == gb.shape == (q.size,)
        assert np.array_equal(ga.view(np.uint8), gb.view(np.uint8))
        a.sync()
        b.sync()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("width", [3, 4, 33])
@pytest.mark.parametrize("mode", MODES)
def test_key_counts_and_patterns(cuda, oracle_mod, mode, width, n):
    """Counts that cross the lane-group, wave and 2048-key chunk boundaries x
    every key pattern, host and device; then the same keys again (the later
    call wins)."""
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[0]
    rng = np.random.default_rng(n * 7 + width)
    dtype = np.float32 if width != 4 else np.float64
    for name, k in key_patterns(rng, n, kb, ke).items():
        orc = RowOracle(oracle_mod, dtype, mode, width, kb, ke)
        src = ValueSource(dtype, mode, rng)
        with ps.Shard(kb, ke, dtype, mode=mode, width=width) as sh:
            for rnd in range(2):  # two calls in a row on the same keys
                v = src.rows(n, width)
                sh.add(tdev(k, cuda), tdev(v, cuda))
                orc.add(k, v)
                v = src.rows(n, width)
                sh.add(k[::-1].copy(), v)
                orc.add(k[::-1], v)
                orc.check(k, dget(sh, k, cuda), f"{name} round {rnd} device get")
            orc.check(orc.all_keys(), sh.get(orc.all_keys()), f"{name} host get of the whole range")
            sh.sync()


def test_duplicates_across_batches_of_one_grouped_call(cuda, oracle_mod):
    import parameter_server_amd as ps

    kb, ke = LAYOUTS[1]
    rng = np.random.default_rng(11)
    for mode in MODES:
        for width, dtype in ((5, np.int32), (16, np.float32), (64, np.float64)):
            orc = RowOracle(oracle_mod, dtype, mode, width, kb, ke)
            src = ValueSource(dtype, mode, rng)
            with ps.Shard(kb, ke, dtype, mode=mode, width=width) as sh:
                base = rand_keys(rng, 2100, kb, ke)
                ks = [base, base[::-1].copy(), base[:1].copy(), base[:0].copy(), base[500:700].copy()]
                vs = [src.rows(x.size, width) for x in ks]
                sh.add_grouped([(tdev(a, cuda), tdev(b, cuda)) for a, b in zip(ks, vs)])
                for a, b in zip(ks, vs):
                    orc.add(a, b)
                orc.check(orc.all_keys(), sh.dense_view().cpu().numpy(), f"{mode} W={width}")
                sh.sync()


@pytest.mark.parametrize("mode", MODES)
def test_device_add_with_out_of_range_keys_is_reported_at_sync(cuda, oracle_mod, mode):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, width = 1000, 4000, 4
    rng = np.random.default_rng(2)
    orc = RowOracle(oracle_mod, np.float32, mode, width, kb, ke)
    src = ValueSource(np.float32, mode, rng)
    with ps.Shard(kb, ke, np.float32, mode=mode, width=width) as sh:
        k = rand_keys(rng, 3000, kb, ke)
        bad = np.zeros(k.size, dtype=bool)
        bad[[0, 77, 2048, 2999]] = True
        k[bad] = [ke, 0xFFFFFFFF, kb - 1, ke]
        v = src.rows(k.size, width)
        sh.add(tdev(k, cuda), tdev(v, cuda))
        orc.add(k[~bad], v[~bad])
        q = orc.all_keys()
        orc.check(q, dget(sh, q, cuda), "in-range rows")
        oor = np.array([ke, 0xFFFFFFFF, kb - 1, 0], dtype=np.uint32)
        assert not dget(sh, oor, cuda).any() and not sh.get(oor).any()
        with pytest.raises(ps.PskvError) as e:
            sh.sync()
        assert e.value.code == _lib.PSKV_ESTATE
        assert "row shard" in str(e.value) and "out-of-range" in str(e.value)
        sh.clear()
        sh.sync()
        assert not sh.get(q).view(np.uint8).any()
        assert not sh.dense_view().cpu().numpy().view(np.uint8).any()


def test_host_add_with_an_out_of_range_key_is_refused(cuda, oracle_mod):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, width = 1000, 4000, 3
    rng = np.random.default_rng(4)
    with ps.Shard(kb, ke, np.float64, width=width) as sh:
        k = rand_keys(rng, 500, kb, ke)
        k[317] = ke + 5
        with pytest.raises(ps.PskvError) as e:
            sh.add(k, np.ones((k.size, width)))
        assert e.value.code == _lib.PSKV_EINVAL and str(ke + 5) in str(e.value)
        with pytest.raises(ps.PskvError) as e:
            sh.add_grouped([(k[:10].copy(), np.ones((10, width))), (k, np.ones((k.size, width)))])
        assert e.value.code == _lib.PSKV_EINVAL
        q = np.arange(kb, ke, dtype=np.uint32)
        assert not sh.get(q).view(np.uint8).any()  # nothing was applied
        # Gets of such keys: zero rows, host and device, and no error
        oor = np.array([ke, kb - 1, 0xFFFFFFFF], dtype=np.uint32)
        assert sh.get(oor).shape == (3, width) and not sh.get(oor).any()
        assert not dget(sh, oor, cuda).any()
        sh.sync()


def test_info_timing_and_options(cuda, oracle_mod):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    kb, ke, width = 0, 3000, 16
    rng = np.random.default_rng(8)
    for mode in MODES:
        orc = RowOracle(oracle_mod, np.float32, mode, width, kb, ke)
        src = ValueSource(np.float32, mode, rng)
        with ps.Shard(kb, ke, np.float32, mode=mode, width=width) as sh:
            info = sh.info()
            assert info["width"] == width and info["value_bytes"] == 4
            assert info["dense_bytes"] == (ke - kb) * width * 4
            sh.set_timing(True)
            run_every_path(sh, orc, src, rng, cuda, [300, 2049, 65])
            add_id = _lib.PSKV_K_ROW_COMMIT if mode == "assign" else _lib.PSKV_K_ROW_ACCUMULATE
            other = _lib.PSKV_K_ROW_ACCUMULATE if mode == "assign" else _lib.PSKV_K_ROW_COMMIT
            assert sh.kernel_time(_lib.PSKV_K_ROW_GATHER)["launches"] > 0
            assert sh.kernel_time(add_id)["launches"] > 0
            assert sh.kernel_time(add_id)["total_ms"] > 0
            assert sh.kernel_time(other)["launches"] == 0
            for kid in range(11):  # no scalar kernel runs on a row shard
                assert sh.kernel_time(kid)["launches"] == 0, _lib.KERNEL_NAMES[kid]
            sh.set_timing(False)
            # every option is accepted and echoed, and changes no result
            for name, value in OPTIONS.items():
                sh.set_option(name, value)
                assert sh.get_option(name) == value
            k = rand_keys(rng, 2500, kb, ke)
            v = src.rows(k.size, width)
            sh.add(tdev(k, cuda), tdev(v, cuda), sorted_hint=True)  # accepted, ignored
            orc.add(k, v)
            run_every_path(sh, orc, src, rng, cuda, [300, 2049, 65])
            orc.check(orc.all_keys(), sh.dense_view().cpu().numpy(), "after options")


def test_wrong_value_counts_raise(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd.storage import CheckError, HipStorage

    with ps.Shard(0, 100, np.float32, width=4) as sh:
        k = np.arange(5, dtype=np.uint32)
        with pytest.raises(ValueError):
            sh.add(k, np.ones(5 * 4 - 1, dtype=np.float32))
        with pytest.raises(ValueError):
            sh.add(k, np.ones((5, 3), dtype=np.float32))
        with pytest.raises(ValueError):
            sh.add(tdev(k, cuda), tdev(np.ones(5, dtype=np.float32), cuda))
        with pytest.raises(ValueError):
            sh.add_grouped([(k, np.ones(5, dtype=np.float32))])
    st = HipStorage(np.float32, 0, 100, width=4)
    try:
        with pytest.raises(CheckError) as e:
            st.SubAdd(k, np.ones(19, dtype=np.float32).view(np.uint8))
        assert "5" in str(e.value) and "19" in str(e.value)
    finally:
        st.close()


def test_python_storage_mirror_mf_rows(cuda):
    """An mf-shaped round on a width-10 storage: pull two latent rows (never
    written: zeros), push the updated rows, pull them back bit-exact."""
    from parameter_server_amd.storage import Flag, HipStorage, Message, typed

    st = HipStorage(np.float64, 0, 1 << 12, width=10)
    try:
        keys = np.array([17, 3001], dtype=np.uint32)
        g = Message()
        g.meta.flag, g.meta.sender, g.meta.recver, g.meta.model_id = Flag.kGet, 5, 200, 1
        g.AddData(keys)
        rep = st.Get(g)
        assert rep.meta.sender == 200 and rep.meta.recver == 5
        assert np.shares_memory(rep.data[0], g.data[0])  # reply keys alias the request
        rows = typed(rep.data[1], np.float64)
        assert rows.size == 20 and not rows.any()
        upd = np.random.default_rng(0).standard_normal((2, 10))
        a = Message()
        a.meta.flag = Flag.kAdd
        a.AddData(keys)
        a.AddData(upd)
        st.Add(a)
        rep = st.Get(g)
        assert np.array_equal(typed(rep.data[1], np.float64).view(np.uint64), upd.reshape(-1).view(np.uint64))
        assert np.shares_memory(rep.data[0], g.data[0])
        st.FinishIter()
    finally:
        st.close()


def test_cpp_rows_program(cuda):
    """tests/cpp/hip_storage_rows_test.cpp: the reference's three-key storage
    cases at width 4 through std::unique_ptr<AbstractStorage>, and the size
    check's abort in a child process."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_rows_test")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
