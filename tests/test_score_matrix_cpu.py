"""CPU tests of the score matrix pull (pskv_get_score_matrix): the symbol and
the refusals that come before the handle.  No kernel is launched."""
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
    assert "pskv_get_score_matrix" in re.findall(r" T (pskv_\w+)", out)
    assert "pskv_get_score_matrix" in _lib.EXPORTED and callable(_lib.lib.pskv_get_score_matrix)
    assert re.search(r"^int pskv_get_score_matrix\(pskv_shard\* s, const uint32_t\* keys, uint64_t n, "
                     r"const void\* queries, uint64_t nq,\s+void\* out, uint64_t out_stride, int flags\);", txt, re.M)
    assert "Score matrix pulls" in txt and _lib.lib.pskv_abi_version() == 1


def test_arguments_are_checked_before_the_handle():
    from parameter_server_amd import _lib

    keys = np.arange(7, dtype=np.uint32)
    queries = np.full(3 * 4, 9.0, dtype=np.float32)
    out = np.full(3 * 7, 9.0, dtype=np.float32)

    def call(k, n, q, nq, o, stride, flags):
        k, q, o = (a.ctypes.data if a is not None else None for a in (k, q, o))
        rc = _lib.lib.pskv_get_score_matrix(None, k, n, q, nq, o, stride, flags)
        return rc, _lib.lib.pskv_last_error().decode()

    for flags in (_lib.PSKV_HOST, _lib.PSKV_DEVICE):
        rc, msg = call(keys, 7, queries, 3, out, 7, flags)
        assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for flags in (0x8, 0x100, _lib.PSKV_DEVICE | _lib.PSKV_HOST_FRAME):
        rc, msg = call(keys, 7, queries, 3, out, 7, flags)
        assert rc == _lib.PSKV_EINVAL and "flags" in msg, msg
    for args, word in [((None, 7, queries, 3, out, 7), "null keys"), ((keys, 7, None, 3, out, 7), "null queries"),
                       ((keys, 7, queries, 3, None, 7), "null out"), ((keys, 7, queries, 3, out, 6), "out_stride 6 < n")]:
        for flags in (_lib.PSKV_HOST, _lib.PSKV_DEVICE):
            rc, msg = call(*args, flags)
            assert rc == _lib.PSKV_EINVAL and word in msg and "null shard" not in msg, msg
    # n == 0 and nq == 0: null pointers pass every check (with a shard: PSKV_OK, tests/test_score_matrix_gpu.py)
    rc, msg = call(None, 0, None, 0, None, 0, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    assert (queries == 9.0).all() and (out == 9.0).all()
