"""Sparse shards (pskv_shard_create_sparse), the part that needs no GPU: the
exported symbols, the argument checks that come before any device lookup, and
the relabelling helper of tests/sparse_util.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sparse_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pskv.h")
NEW_SYMBOLS = ["pskv_shard_create_sparse", "pskv_sparse_info_get", "pskv_sparse_keys", "pskv_index_time"]
# include/pskv.h's values (the library is imported inside the tests, as everywhere
# in this suite: a GPU run must load torch's HIP runtime first)
PSKV_EINVAL, PSKV_I32, PSKV_F32, PSKV_F64, PSKV_ASSIGN, PSKV_ACCUMULATE, PSKV_HOST = -1, 0, 1, 2, 0, 1, 0
PSKV_MAX_WIDTH = 4096


class _Lazy:
    """_lib.X / lib.X resolved at use."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, attr):
        from parameter_server_amd import _lib as m

        return getattr(m if self._name == "_lib" else m.lib, attr)


_lib, lib = _Lazy("_lib"), _Lazy("lib")


def err():
    return lib.pskv_last_error().decode()


def create(capacity, dtype=PSKV_F32, mode=PSKV_ASSIGN, width=4, device=0):
    h = ctypes.c_void_p()
    rc = lib.pskv_shard_create_sparse(device, capacity, dtype, mode, width, ctypes.byref(h))
    if rc == 0:  # (only where a GPU is present)
        lib.pskv_shard_destroy(h)
    return rc


def test_symbols_exported_and_abi_version_unchanged():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pskv_\w+)", out))
    assert [s for s in NEW_SYMBOLS if s not in exported] == []
    assert [s for s in NEW_SYMBOLS if s not in _lib.EXPORTED] == []
    text = open(HEADER).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, text), s
    assert lib.pskv_abi_version() == 1
    assert re.search(r"#define PSKV_ABI_VERSION 1\b", text)


def test_timing_bits_and_kernel_ids_pinned():
    text = open(HEADER).read()
    assert re.search(r"#define PSKV_TIME_APPLY \(1u << 14\)", text)
    assert re.search(r"#define PSKV_TIME_POOLED \(1u << 15\)", text)
    assert re.search(r"#define PSKV_TIME_INDEX \(1u << 16\)", text)
    assert re.search(r"PSKV_K_COUNT = 14\b", text)
    assert _lib.PSKV_TIME_INDEX == 1 << 16 and _lib.PSKV_K_COUNT == 14


def test_info_structs_match_the_header():
    # pskv_info is ABI: a sparse shard reports through it unchanged
    assert ctypes.sizeof(_lib.PskvInfo) == 96
    assert ctypes.sizeof(_lib.PskvSparseInfo) == 40
    assert [f for f, _ in _lib.PskvSparseInfo._fields_] == ["size", "capacity", "count", "table_slots", "index_bytes"]


# device 12345 exists nowhere: a message that names the field proves the check
# came before the device was looked at
@pytest.mark.parametrize("kw,field", [
    (dict(capacity=0), "capacity"),
    (dict(capacity=2**31 - 1), "capacity"),
    (dict(capacity=2**40), "capacity"),
    (dict(capacity=8, width=0), "width"),
    (dict(capacity=8, width=PSKV_MAX_WIDTH + 1), "width"),
    (dict(capacity=8, dtype=3), "dtype"),
    (dict(capacity=8, dtype=-1), "dtype"),
    (dict(capacity=8, mode=2), "mode"),
    (dict(capacity=8, mode=-1), "mode"),
])
def test_creation_refuses_bad_arguments_before_the_device(kw, field):
    assert create(device=12345, **kw) == _lib.PSKV_EINVAL
    assert field in err() and "pskv_shard_create_sparse" in err(), err()


def test_creation_largest_arguments_reach_the_device_lookup():
    # every argument at its limit is accepted; what fails is the device
    assert create(device=12345, capacity=2**31 - 2, width=1, dtype=_lib.PSKV_I32) == _lib.PSKV_EINVAL
    assert "device" in err(), err()
    assert create(device=12345, capacity=1, width=_lib.PSKV_MAX_WIDTH, dtype=_lib.PSKV_F64,
                  mode=_lib.PSKV_ACCUMULATE) == _lib.PSKV_EINVAL
    assert "device" in err(), err()
    # the largest row arrays the other limits allow, (2^31 - 1) rows of 4096
    # doubles, are 2^46 - 2^15 bytes: the 2^46 limit of pskv_shard_create_rows
    # holds here by arithmetic, so no argument can trip it
    assert (2**31 - 1) * _lib.PSKV_MAX_WIDTH * 8 < 2**46
    assert create(device=12345, capacity=2**31 - 2, width=_lib.PSKV_MAX_WIDTH, dtype=_lib.PSKV_F64) == _lib.PSKV_EINVAL
    assert "device" in err(), err()


def test_creation_null_out():
    assert lib.pskv_shard_create_sparse(0, 8, _lib.PSKV_F32, _lib.PSKV_ASSIGN, 1, None) == _lib.PSKV_EINVAL
    assert "out" in err()


def test_info_and_keys_on_a_null_shard():
    info = _lib.PskvSparseInfo(ctypes.sizeof(_lib.PskvSparseInfo))
    assert lib.pskv_sparse_info_get(None, ctypes.byref(info)) == _lib.PSKV_EINVAL
    assert "null shard" in err()
    n = ctypes.c_uint64(77)
    buf = np.zeros(4, dtype=np.uint32)
    assert lib.pskv_sparse_keys(None, buf.ctypes.data, 4, ctypes.byref(n), _lib.PSKV_HOST) == _lib.PSKV_EINVAL
    assert "null shard" in err()
    assert lib.pskv_sparse_keys(None, buf.ctypes.data, 4, None, _lib.PSKV_HOST) == _lib.PSKV_EINVAL
    assert lib.pskv_sparse_keys(None, None, 4, ctypes.byref(n), _lib.PSKV_HOST) == _lib.PSKV_EINVAL
    assert lib.pskv_sparse_keys(None, buf.ctypes.data, 4, ctypes.byref(n), 0x10) == _lib.PSKV_EINVAL
    assert "flags" in err()
    assert lib.pskv_index_time(None, None, None, None) == _lib.PSKV_EINVAL


@pytest.mark.parametrize("size", [0, 39, 41, 104])
def test_info_wrong_size_names_the_field(size):
    info = _lib.PskvSparseInfo(size)
    assert lib.pskv_sparse_info_get(None, ctypes.byref(info)) == _lib.PSKV_EINVAL
    assert "size" in err(), err()
    assert lib.pskv_sparse_info_get(None, None) == _lib.PSKV_EINVAL


def test_relabelling_helper_self_test():
    assert su.self_test()


def test_relabelled_ranks_feed_the_row_oracle(oracle_mod):
    """The same pushes through raw keys (assign: MapStorageRef takes any key) and
    through ranks give the same rows: the relabelling changes names only."""
    from rows_util import RowOracle, ValueSource

    rng = np.random.default_rng(11)
    pool = su.key_pool(rng, 37)
    w = 3
    raw = RowOracle(oracle_mod, np.float32, "assign", w, 0, 1 << 32)
    byrank = RowOracle(oracle_mod, np.float32, "assign", w, 0, pool.size)
    acc = RowOracle(oracle_mod, np.int32, "accumulate", w, 0, pool.size)
    rl = su.Relabel(pool)
    src, asrc = ValueSource(np.float32, "assign", rng), ValueSource(np.int32, "accumulate", rng)
    total = np.zeros((pool.size, w), dtype=np.int64)
    for keys in su.pool_patterns(rng, 300, pool).values():
        v = src.rows(keys.size, w)
        raw.add(keys, v)
        byrank.add(rl.rank(keys), v)
        a = asrc.rows(keys.size, w)
        acc.add(rl.rank(keys), a)
        np.add.at(total, rl.rank(keys).astype(np.int64), a.astype(np.int64))
    assert np.array_equal(raw.expect(pool), byrank.expect(rl.rank(pool)))
    gone = su.absent_keys(rng, pool, 5)
    assert not raw.expect(gone).any()
    want = (total & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    assert np.array_equal(acc.expect(rl.rank(pool)), want[rl.rank(pool).astype(np.int64)])
