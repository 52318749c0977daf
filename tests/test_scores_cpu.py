"""CPU tests of the score pull (pskv_get_scores): the symbol and the refusals
that come before the handle.  No kernel is launched."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_exported_declared_and_bound():
    from parameter_server_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "parameter_server_amd", "libpskv.so")],
                         capture_output=True, text=True, check=True).stdout
    with open(os.path.join(ROOT, "include", "pskv.h")) as f:
        txt = f.read()
    assert "pskv_get_scores" in re.findall(r" T (pskv_\w+)", out)
    assert "pskv_get_scores" in _lib.EXPORTED and callable(_lib.lib.pskv_get_scores)
    assert re.search(r"^int pskv_get_scores\(pskv_shard\* s, const uint32_t\* keys, uint64_t n, const void\* queries,",
                     txt, re.M)
    assert "Score pulls" in txt and _lib.lib.pskv_abi_version() == 1


def test_arguments_are_checked_before_the_handle():
    from parameter_server_amd import _lib

    keys = np.arange(7, dtype=np.uint32)
    queries = np.full(3 * 4, 9.0, dtype=np.float32)
    out = np.full(7, 9.0, dtype=np.float32)
    good = np.array([0, 3, 3, 7], dtype=np.uint64)

    def call(k, n, off, nbags, q, o, flags):
        k, q, off, o = (a.ctypes.data if a is not None else None for a in (k, q, off, o))
        rc = _lib.lib.pskv_get_scores(None, k, n, q, off, nbags, o, flags)
        return rc, _lib.lib.pskv_last_error().decode()

    for flags in (_lib.PSKV_HOST, _lib.PSKV_DEVICE):
        rc, msg = call(keys, 7, good, 3, queries, out, flags)
        assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for off, bag, word in [(np.array([1, 3, 3, 7], dtype=np.uint64), 0, "offsets[0]"),
                           (np.array([0, 5, 4, 7], dtype=np.uint64), 1, "decrease"),
                           (np.array([0, 3, 3, 6], dtype=np.uint64), 2, "offsets[nbags]"),
                           (np.array([0, 3, 8, 8], dtype=np.uint64), 1, "past")]:
        rc, msg = call(keys, 7, off, 3, queries, out, _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL and "offsets" in msg and f"bag {bag}:" in msg and word in msg, msg
        assert "null shard" not in msg, msg
    rc, msg = call(keys, 7, np.array([1, 3, 3, 7], dtype=np.uint64), 3, queries, out, _lib.PSKV_DEVICE)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for flags in (0x8, 0x100, _lib.PSKV_DEVICE | _lib.PSKV_HOST_FRAME):
        rc, msg = call(keys, 7, good, 3, queries, out, flags)
        assert rc == _lib.PSKV_EINVAL and "flags" in msg, msg
    for args, word in [((None, 7, good, 3, queries, out), "null keys"), ((keys, 7, None, 3, queries, out), "null offsets"),
                       ((keys, 7, good, 3, None, out), "null queries"), ((keys, 7, good, 3, queries, None), "null out")]:
        rc, msg = call(*args, _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL and word in msg and "null shard" not in msg, msg
    # nbags == 0 (and n == 0): null pointers pass every check (with a shard: PSKV_OK, tests/test_scores_gpu.py)
    rc, msg = call(None, 0, None, 0, None, None, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    assert (queries == 9.0).all() and (out == 9.0).all()
