"""Growth and erase of sparse shards (pskv_sparse_reserve, pskv_sparse_set_growth,
pskv_sparse_get_growth, pskv_sparse_erase), the part that needs no GPU: the
exported symbols, the argument checks that come before the handle is looked
at, the growth rule of tests/sparse_grow_util.py against a hand-written table,
and the fuzz scenarios' share of calls that are compared bit for bit."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sparse_grow_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pskv.h")
NEW_SYMBOLS = ["pskv_sparse_reserve", "pskv_sparse_set_growth", "pskv_sparse_get_growth", "pskv_sparse_erase"]
PSKV_DEVICE = 1


class _Lazy:
    """_lib.X / lib.X resolved at use (a GPU run must load torch's HIP runtime first)."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, attr):
        from parameter_server_amd import _lib as m

        return getattr(m if self._name == "_lib" else m.lib, attr)


_lib, lib = _Lazy("_lib"), _Lazy("lib")


def err():
    return lib.pskv_last_error().decode()


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


def test_header_lists_what_is_not_provided():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    assert "not provided: growth, deletion or eviction" not in text
    for words in ("shrinking", "growth requested from the device", "eviction policies", "tombstones", "64-bit keys"):
        assert words in text, words


@pytest.mark.parametrize("capacity", [0, 2**31 - 1, 2**31, 2**40, 2**64 - 1])
def test_reserve_refuses_a_bad_capacity_before_the_handle(capacity):
    assert lib.pskv_sparse_reserve(None, capacity) == _lib.PSKV_EINVAL
    assert "capacity" in err() and "null shard" not in err(), err()


def test_reserve_largest_capacity_reaches_the_handle():
    for capacity in (1, 2**31 - 2):
        assert lib.pskv_sparse_reserve(None, capacity) == _lib.PSKV_EINVAL
        assert "null shard" in err(), err()


@pytest.mark.parametrize("limit", [2**31 - 1, 2**32, 2**64 - 1])
def test_set_growth_refuses_a_limit_out_of_range_before_the_handle(limit):
    assert lib.pskv_sparse_set_growth(None, limit) == _lib.PSKV_EINVAL
    assert "max_capacity" in err() and "null shard" not in err(), err()


def test_set_growth_and_get_growth_on_a_null_shard():
    for limit in (0, 1, 2**31 - 2):
        assert lib.pskv_sparse_set_growth(None, limit) == _lib.PSKV_EINVAL
        assert "null shard" in err(), err()
    m, r = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.pskv_sparse_get_growth(None, ctypes.byref(m), ctypes.byref(r)) == _lib.PSKV_EINVAL
    assert "null shard" in err() and (m.value, r.value) == (7, 7)
    assert lib.pskv_sparse_get_growth(None, None, None) == _lib.PSKV_EINVAL


def test_erase_checks_flags_and_keys_before_the_handle():
    buf = np.zeros(4, dtype=np.uint32)
    for flags in (2, 4, 0x10, 3):  # PSKV_SORTED_HINT, PSKV_HOST_FRAME and unknown bits: PSKV_HOST or PSKV_DEVICE only
        assert lib.pskv_sparse_erase(None, buf.ctypes.data, 4, flags) == _lib.PSKV_EINVAL
        assert "flags" in err() and "null shard" not in err(), err()
    for flags in (_lib.PSKV_HOST, PSKV_DEVICE):
        assert lib.pskv_sparse_erase(None, None, 4, flags) == _lib.PSKV_EINVAL
        assert "keys" in err() and "null shard" not in err(), err()
        assert lib.pskv_sparse_erase(None, buf.ctypes.data, 4, flags) == _lib.PSKV_EINVAL
        assert "null shard" in err(), err()
        assert lib.pskv_sparse_erase(None, None, 0, flags) == _lib.PSKV_EINVAL  # (n == 0 still needs a shard)
        assert "null shard" in err(), err()


# (capacity, count, n, max) -> the capacity behind the call, written out by hand
RULE = [
    ((8, 0, 8, 0), 8),            # growth off
    ((8, 8, 100, 0), 8),
    ((8, 0, 8, 4100), 8),         # count + n == capacity: fits
    ((8, 0, 9, 4100), 16),        # one too many: doubling
    ((8, 8, 1, 4100), 16),
    ((8, 7, 1, 4100), 8),
    ((8, 0, 4100, 4100), 4100),   # straight to count + n
    ((8, 0, 5000, 4100), 4100),   # clamped by the limit
    ((8, 3, 14, 4100), 17),       # count + n beats doubling
    ((8, 3, 13, 4100), 16),       # doubling ties count + n
    ((100, 100, 1, 150), 150),    # doubling clamped
    ((100, 60, 41, 101), 101),
    ((4100, 4100, 37, 4100), 4100),  # at the limit: fixed
    ((16, 16, 600, 20), 20),
    ((2**30, 2**30, 1, 2**31 - 2), 2**31 - 2),
    ((1, 0, 1, 5), 1),
    ((1, 1, 1, 5), 2),
    ((8, 8, 0, 4100), 8),         # a call without keys does not grow
]


@pytest.mark.parametrize("case,want", RULE)
def test_growth_rule_against_the_hand_written_table(case, want):
    assert gu.grown_capacity(*case) == want


def test_capacity_model_follows_the_rule_along_a_call_sequence():
    """4100 keys in calls of 37 from capacity 8: the capacities depend on the
    call sequence alone (count + n against the capacity, then doubling)."""
    cm = gu.CapacityModel(8, 4100)
    seen = []
    for a in range(0, 4100, 37):
        cm.write(range(a, min(a + 37, 4100)))
        seen.append(cm.capacity)
    assert seen[:4] == [37, 74, 148, 148] and seen[-1] == 4100 and cm.count == 4100
    assert sorted(set(seen)) == [37, 74, 148, 296, 592, 1184, 2368, 4100] and cm.rebuilds == 8
    cm.erase([1, 2, 2, 5000])
    assert (cm.count, cm.capacity, cm.rebuilds) == (4098, 4100, 9)
    cm.erase([])
    assert cm.rebuilds == 9
    assert gu.table_slots(8) == 16 and gu.table_slots(20) == 64 and gu.table_slots(4100) == 16384


def _build_and_run(tmp_path, name, extra, args=()):
    """tests/cpp/sparse_plan_test.cpp (the rules of pskv_plan.h in C++), built with g++ and run."""
    src = os.path.join(ROOT, "tests", "cpp", "sparse_plan_test.cpp")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra,
                        "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "parameter_server_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    if not args:
        assert " 0 failed" in r.stdout
    return r.stdout


def test_sparse_plan(tmp_path):
    _build_and_run(tmp_path, "sparse_plan_test", [])


def test_sparse_plan_under_host_sanitizers(tmp_path):
    """The same host-only program with AddressSanitizer and UBSan: a stand-alone
    executable, nothing loaded into Python."""
    _build_and_run(tmp_path, "sparse_plan_test_san",
                   ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_sparse_plan_grid_against_the_python_model(tmp_path):
    """sparse_table_slots and sparse_grown_capacity as the library computes them
    against table_slots and grown_capacity of sparse_grow_util, the reference:
    capacity 1..33, count 0..capacity, n 0..70, max in {c, c + 1, 2c - 1, 2c, 4c}."""
    out = _build_and_run(tmp_path, "sparse_plan_grid", [], ["--grid", "1", "33", "70"])
    slots, grown = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "slots":
            slots[int(f[1])] = int(f[2])
        else:
            assert f[0] == "grow", line
            grown[tuple(int(x) for x in f[1:5])] = int(f[5])
    assert slots == {c: gu.table_slots(c) for c in range(1, 34)}
    want = {(c, count, n, m): gu.grown_capacity(c, count, n, m)
            for c in range(1, 34) for count in range(c + 1) for n in range(71)
            for m in (c, c + 1, 2 * c - 1, 2 * c, 4 * c)}
    assert grown.keys() == want.keys()
    assert [k for k in want if grown[k] != want[k]] == []


def test_fuzz_scenarios_compare_nine_calls_in_ten_bit_for_bit():
    """The model alone: 40 scenarios, what each call is and whether its result
    is order-dependent (duplicated keys in an accumulate Add or a step)."""
    scs = [gu.draw_scenario(seed) for seed in range(40)]
    assert gu.comparable_share(scs) >= 0.9, gu.comparable_share(scs)
    ops = set()
    for sc in scs:
        assert 8 <= sc["capacity"] <= 256
        summing = sc["kind"] == "optimizer" or sc["mode"] == "accumulate"
        for c in sc["calls"]:
            ops.add(c["op"])
            k = c.get("keys")
            assert k is None or k.size <= gu.FUZZ_MAX_KEYS
            assert c["count"] <= c["capacity"], (sc["seed"], c["op"])
            dup = k is not None and np.unique(k).size != k.size
            step_or_sum = c["op"].startswith("apply") or (summing and sc["kind"] == "storage" and c["op"].startswith("add"))
            assert c["order_dependent"] == bool(dup and step_or_sum), (sc["seed"], c["op"])
    assert {"reserve", "set_growth", "erase", "add", "add_grouped", "add_get_grouped", "get", "get_grouped", "get_pooled",
            "apply", "apply_grouped", "apply_pooled", "apply_pooled_grouped", "put_state", "get_state", "sync"} <= ops
    assert any(sc["calls"][-1]["rebuilds"] >= 3 for sc in scs)
    again = gu.draw_scenario(7)  # seeded: a scenario reruns identically
    assert [(c["op"], c["count"], c["capacity"]) for c in again["calls"]] == \
        [(c["op"], c["count"], c["capacity"]) for c in scs[7]["calls"]] and np.array_equal(again["pool"], scs[7]["pool"])
