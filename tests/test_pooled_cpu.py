"""CPU tests of pooled pulls (pskv_get_pooled): the planner program
(tests/cpp/pooled_plan_test.cpp: the offsets check, the device clamp, the
long-bag chunks and the window rule), built with g++ and also run under the
host sanitizers as a stand-alone program, and the argument checks that
pskv_get_pooled makes before it looks at the handle.  No kernel is launched."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build_and_run(tmp_path, name, extra):
    src = os.path.join(ROOT, "tests", "cpp", "pooled_plan_test.cpp")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra,
                        "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "parameter_server_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
    return r.stdout


def test_pooled_plan(tmp_path):
    _build_and_run(tmp_path, "pooled_plan_test", [])


def test_pooled_plan_under_host_sanitizers(tmp_path):
    """The same host-only program with AddressSanitizer and UBSan: a stand-alone
    executable, nothing loaded into Python."""
    _build_and_run(tmp_path, "pooled_plan_test_san",
                   ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _call(keys, n, weights, offsets, nbags, out, flags):
    from parameter_server_amd import _lib

    def ptr(a):
        return a.ctypes.data if a is not None else None

    rc = _lib.lib.pskv_get_pooled(None, ptr(keys), n, ptr(weights), ptr(offsets), nbags, ptr(out), flags)
    return rc, _lib.lib.pskv_last_error().decode()


def test_get_pooled_checks_its_arguments_before_the_handle():
    from parameter_server_amd import _lib

    assert {"pskv_get_pooled", "pskv_pooled_time"} <= set(_lib.EXPORTED)
    assert _lib.PSKV_TIME_POOLED == 1 << 15 and _lib.PSKV_K_COUNT == 14
    keys = np.arange(7, dtype=np.uint32)
    out = np.full(3 * 4, 9.0, dtype=np.float32)
    good = np.array([0, 3, 3, 7], dtype=np.uint64)
    # every argument holds: only the null shard is left to object to
    rc, msg = _call(keys, 7, None, good, 3, out, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for off, bag, word in [(np.array([1, 3, 3, 7], dtype=np.uint64), 0, "offsets[0]"),
                           (np.array([0, 5, 4, 7], dtype=np.uint64), 1, "decrease"),
                           (np.array([0, 3, 3, 6], dtype=np.uint64), 2, "offsets[nbags]"),
                           (np.array([0, 3, 8, 8], dtype=np.uint64), 1, "past")]:
        rc, msg = _call(keys, 7, None, off, 3, out, _lib.PSKV_HOST)
        assert rc == _lib.PSKV_EINVAL, (off, rc, msg)
        assert "offsets" in msg and f"bag {bag}:" in msg and word in msg and "null shard" not in msg, msg
    # device offsets cannot be read: the same bad array gets as far as the handle
    rc, msg = _call(keys, 7, None, np.array([1, 3, 3, 7], dtype=np.uint64), 3, out, _lib.PSKV_DEVICE)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    for flags in (0x8, 0x100, _lib.PSKV_DEVICE | _lib.PSKV_HOST_FRAME):
        rc, msg = _call(keys, 7, None, good, 3, out, flags)
        assert rc == _lib.PSKV_EINVAL and "flags" in msg, msg
    rc, msg = _call(None, 7, None, good, 3, out, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null keys" in msg, msg
    rc, msg = _call(keys, 7, None, None, 3, out, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null offsets" in msg, msg
    rc, msg = _call(keys, 7, None, good, 3, None, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null out" in msg, msg
    # no bag: the null pointers are fine, the null shard is named
    rc, msg = _call(None, 0, None, None, 0, None, _lib.PSKV_HOST)
    assert rc == _lib.PSKV_EINVAL and "null shard" in msg, msg
    assert (out == 9.0).all()
    n, ms, el = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
    assert _lib.lib.pskv_pooled_time(None, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(el)) == _lib.PSKV_EINVAL
