"""CPU tests of row-valued shards: the argument checks of pskv_shard_create_rows
(made before any device is looked up), the new exports, and the per-column
oracle the GPU tests check against (tests/rows_util.py), pinned by a direct
numpy restatement.  No kernel is launched here."""
import ctypes

import numpy as np

from rows_util import RowOracle


def _create_rows(key_begin, key_end, dtype, mode, width):
    from parameter_server_amd import _lib

    h = ctypes.c_void_p()
    rc = _lib.lib.pskv_shard_create_rows(0, key_begin, key_end, dtype, mode, width, 0, ctypes.byref(h))
    return rc, _lib.lib.pskv_last_error().decode(), h


def test_create_rows_rejects_bad_widths_before_the_device_lookup():
    from parameter_server_amd import _lib

    assert _lib.PSKV_MAX_WIDTH == 4096
    for key_begin, key_end, dtype, width in [(0, 1000, _lib.PSKV_F32, 0),
                                             (0, 1000, _lib.PSKV_F32, _lib.PSKV_MAX_WIDTH + 1),
                                             (0, 1 << 32, _lib.PSKV_F64, _lib.PSKV_MAX_WIDTH)]:
        rc, msg, h = _create_rows(key_begin, key_end, dtype, _lib.PSKV_ASSIGN, width)
        assert rc == _lib.PSKV_EINVAL, (width, rc, msg)
        assert "width" in msg, msg
        assert not h.value


def test_create_rows_width_one_fails_like_create_ex():
    from parameter_server_amd import _lib

    h = ctypes.c_void_p()
    rc_ex = _lib.lib.pskv_shard_create_ex(0, 0, 100, 7, _lib.PSKV_ASSIGN, 0, ctypes.byref(h))
    msg_ex = _lib.lib.pskv_last_error().decode()
    rc, msg, h2 = _create_rows(0, 100, 7, _lib.PSKV_ASSIGN, 1)
    assert rc == rc_ex == _lib.PSKV_EINVAL
    assert msg == msg_ex and "dtype" in msg
    assert not h.value and not h2.value


def test_width_of_a_null_shard_and_exports():
    from parameter_server_amd import _lib

    assert _lib.lib.pskv_shard_width(None) == 0
    assert {"pskv_shard_create_rows", "pskv_shard_width"} <= set(_lib.EXPORTED)
    assert (_lib.PSKV_K_ROW_GATHER, _lib.PSKV_K_ROW_COMMIT, _lib.PSKV_K_ROW_ACCUMULATE,
            _lib.PSKV_K_COUNT) == (11, 12, 13, 14)


def test_per_column_oracle_is_last_occurrences_row(oracle_mod):
    """50 keys with duplicates, W = 3: the oracle's rows are the rows of each
    key's LAST occurrence, zeros for a key never pushed."""
    rng = np.random.default_rng(5)
    w, kb, ke = 3, 100, 120
    keys = rng.integers(kb, ke - 2, size=50).astype(np.uint32)  # ke-2, ke-1 never pushed
    assert np.unique(keys).size < keys.size
    vals = (1 + np.arange(50 * w)).reshape(50, w).astype(np.float32)
    orc = RowOracle(oracle_mod, np.float32, "assign", w, kb, ke)
    orc.add(keys, vals)
    q = np.arange(kb, ke, dtype=np.uint32)
    want = np.zeros((q.size, w), dtype=np.float32)
    for i, k in enumerate(keys):  # sequential: a later occurrence overwrites the whole row
        want[int(k) - kb] = vals[i]
    got = orc.expect(q)
    assert np.array_equal(got, want)
    assert not got[-2:].any()
    orc.check(q, want)
    mixed = want.copy()
    dup = int(keys[0]) - kb
    mixed[dup, 1] += 1  # one column of one row from elsewhere: the checker must object
    try:
        orc.check(q, mixed)
    except AssertionError:
        pass
    else:
        raise AssertionError("the checker accepted a mixed row")


def test_per_column_oracle_accumulates(oracle_mod):
    rng = np.random.default_rng(6)
    w, kb, ke = 3, 10, 30
    keys = rng.integers(kb, ke, size=50).astype(np.uint32)
    vi = rng.integers(-2**31, 2**31, size=(50, w)).astype(np.int32)
    orc = RowOracle(oracle_mod, np.int32, "accumulate", w, kb, ke)
    orc.add(keys, vi)
    want = np.zeros((ke - kb, w), dtype=np.int64)
    np.add.at(want, keys.astype(np.int64) - kb, vi.astype(np.int64))
    want = (want & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    q = np.arange(kb, ke, dtype=np.uint32)
    assert np.array_equal(orc.expect(q), want)
    vf = rng.standard_normal((50, w)).astype(np.float32)
    orf = RowOracle(oracle_mod, np.float32, "accumulate", w, kb, ke)
    orf.add(keys, vf)
    ref, bound = orf.expect(q)
    direct = np.zeros((ke - kb, w))
    np.add.at(direct, keys.astype(np.int64) - kb, vf.astype(np.float64))
    assert np.allclose(ref, direct, rtol=0, atol=1e-12)
    orf.check(q, direct.astype(np.float32))
    assert (bound[np.bincount(keys - kb, minlength=ke - kb) == 0] == 0).all()
