"""CPU tests of the row initializer: the numpy restatement (tests/init_util.py)
against the published Philox4x32-10 known answers, and the argument checks of
pskv_shard_set_initializer / pskv_get_init that come before the handle."""
import ctypes
import math

import pytest

import init_util as iu

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(x) for x in iu.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("cfg,word", [
    (None, "cfg"), ((-1, 0, 0.0, 0.0), "kind"), ((4, 0, 0.0, 0.0), "kind"), ((1, 0, math.nan, 0.0), "a must"),
    ((3, 0, 0.0, math.inf), "b must"), ((2, 0, 1.0, 0.5), "a (lo)"), ((3, 0, 0.0, -1.0), "b (std)"),
], ids=["null", "kind-low", "kind-high", "nan-a", "inf-b", "uniform-order", "normal-std"])
def test_set_initializer_checks_come_before_the_handle(cfg, word):
    from parameter_server_amd import _lib

    arg = None if cfg is None else ctypes.byref(_lib.PskvInitializer(*cfg))
    rc = _lib.lib.pskv_shard_set_initializer(None, arg)
    msg = _lib.lib.pskv_last_error().decode()
    assert rc == _lib.PSKV_EINVAL and word in msg and "null shard" not in msg, msg


def test_a_valid_rule_reaches_the_handle_and_get_init_checks_its_arguments():
    from parameter_server_amd import _lib

    L = _lib.lib
    for cfg in [(0, 0, 0.0, 0.0), (1, 9, 0.01, 0.0), (2, 1 << 63, -1.0, -1.0), (3, 5, 1.0, 0.0)]:
        assert L.pskv_shard_set_initializer(None, ctypes.byref(_lib.PskvInitializer(*cfg))) == _lib.PSKV_EINVAL
        assert "null shard" in L.pskv_last_error().decode()
    buf = (ctypes.c_uint32 * 4)()
    for args, word in [((buf, 4, buf, 8), "flags"), ((None, 4, buf, 0), "null keys"), ((buf, 4, None, 1), "null keys"),
                       ((None, 0, None, 0), "null shard")]:
        keys, n, out, flags = args
        rc = L.pskv_get_init(None, ctypes.cast(keys, ctypes.c_void_p) if keys else None, n,
                             ctypes.cast(out, ctypes.c_void_p) if out else None, flags)
        assert rc == _lib.PSKV_EINVAL and word in L.pskv_last_error().decode(), L.pskv_last_error()
