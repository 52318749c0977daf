"""CPU tests of optimizer steps: the new exports, the argument checks that
need no device (pskv_shard_set_optimizer validates the configuration before it
looks at the handle), the float64 oracle of tests/opt_util.py pinned against a
per-key loop, the checker's teeth on the very inputs the GPU bound tests use,
and the exactness of the dyadic cases.  No kernel is launched here."""
import ctypes
import math
import os

import numpy as np
import pytest

import opt_util as ou
from rows_util import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pskv_shard_set_optimizer", "pskv_shard_get_optimizer", "pskv_apply", "pskv_apply_grouped",
       "pskv_get_state", "pskv_apply_time"]


def _last_error():
    from parameter_server_amd import _lib

    return _lib.lib.pskv_last_error().decode()


def test_new_symbols_are_exported_and_declared():
    from parameter_server_amd import _lib

    assert set(NEW) <= set(_lib.EXPORTED)
    header = open(os.path.join(ROOT, "include", "pskv.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(_lib.lib, name)
    assert "#define PSKV_TIME_APPLY (1u << 14)" in header
    assert _lib.PSKV_TIME_APPLY == 1 << 14
    assert (_lib.PSKV_OPT_NONE, _lib.PSKV_OPT_SGD, _lib.PSKV_OPT_ADAGRAD) == (0, 1, 2)


def test_kernel_ids_and_abi_version_are_unchanged():
    from parameter_server_amd import _lib

    assert _lib.PSKV_K_COUNT == 14
    assert _lib.lib.pskv_abi_version() == 1
    assert _lib.lib.pskv_kernel_time(None, 14, None, None, None) == _lib.PSKV_EINVAL


def test_null_shard_is_einval():
    from parameter_server_amd import _lib

    L = _lib.lib
    k = np.zeros(4, dtype=np.uint32)
    v = np.zeros(4, dtype=np.float32)
    b = (_lib.PskvBatch * 1)(_lib.PskvBatch(k.ctypes.data, v.ctypes.data, 4))
    cfg, nb = _lib.PskvOptimizer(), ctypes.c_uint64()
    calls = {
        "pskv_apply": lambda: L.pskv_apply(None, k.ctypes.data, v.ctypes.data, 4, 0),
        "pskv_apply_grouped": lambda: L.pskv_apply_grouped(None, b, 1, 0),
        "pskv_get_state": lambda: L.pskv_get_state(None, k.ctypes.data, 4, v.ctypes.data, 0),
        "pskv_shard_get_optimizer": lambda: L.pskv_shard_get_optimizer(None, ctypes.byref(cfg), ctypes.byref(nb)),
        "pskv_apply_time": lambda: L.pskv_apply_time(None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.PSKV_EINVAL, name
        msg = _last_error()
        assert name in msg and "null shard" in msg, msg


GOOD = dict(kind=2, lr=0.05, weight_decay=0.01, eps=1e-8, init_accum=0.1)


@pytest.mark.parametrize("field,value,kind", [
    ("kind", 3, None), ("kind", -1, None),
    ("lr", 0.0, 1), ("lr", -1.0, 1), ("lr", math.nan, 2), ("lr", math.inf, 2),
    ("weight_decay", -1.0, 1), ("weight_decay", math.nan, 2), ("weight_decay", math.inf, 1),
    ("eps", 0.0, 2), ("eps", -1.0, 2), ("eps", math.nan, 2),
    ("init_accum", -1.0, 2), ("init_accum", math.inf, 2),
])
def test_set_optimizer_reports_the_bad_field_without_a_shard(field, value, kind):
    from parameter_server_amd import _lib

    c = dict(GOOD)
    if kind is not None:
        c["kind"] = kind
    c[field] = value
    cfg = _lib.PskvOptimizer(c["kind"], c["lr"], c["weight_decay"], c["eps"], c["init_accum"])
    assert _lib.lib.pskv_shard_set_optimizer(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
    msg = _last_error()
    assert field in msg and "null shard" not in msg, msg


def test_set_optimizer_good_config_names_the_null_shard():
    from parameter_server_amd import _lib

    for c in (GOOD, dict(GOOD, kind=1, eps=0.0, init_accum=-1.0),  # SGD ignores eps / init_accum
              dict(kind=0, lr=0.0, weight_decay=-1.0, eps=0.0, init_accum=0.0)):  # NONE ignores all
        cfg = _lib.PskvOptimizer(c["kind"], c["lr"], c["weight_decay"], c["eps"], c["init_accum"])
        assert _lib.lib.pskv_shard_set_optimizer(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
        msg = _last_error()
        assert "null shard" in msg, msg
        for f in ("lr", "weight_decay", "eps", "init_accum", "kind"):
            assert f + " must" not in msg, msg
    assert _lib.lib.pskv_shard_set_optimizer(None, None) == _lib.PSKV_EINVAL
    assert "null configuration" in _last_error()


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
def test_oracle_matches_a_per_key_loop(kind):
    rng = np.random.default_rng(11)
    w, rows, lr, wd, eps = 3, 20, 0.05, 0.01, 1e-8
    idx = rng.integers(0, rows - 2, size=50)  # the last two rows are never touched
    assert np.unique(idx).size < idx.size
    grads = rng.standard_normal((50, w)) * 3
    p = rng.standard_normal((rows, w))
    h = np.full((rows, w), 0.1)
    ref = ou.step64(p, h, idx, grads, kind, lr, wd, eps)
    for k in range(rows):
        occ = [i for i in range(50) if idx[i] == k]
        assert ref["m"][k] == len(occ)
        if not occ:
            assert np.array_equal(ref["p"][k], p[k]) and np.array_equal(ref["h"][k], h[k])
            continue
        for j in range(w):
            g = sum(float(grads[i, j]) for i in occ)
            G = sum(abs(float(grads[i, j])) for i in occ)
            d = g + wd * p[k, j]
            if kind == "sgd":
                want_p, want_h = p[k, j] - lr * d, h[k, j]
            else:
                want_h = h[k, j] + d * d
                want_p = p[k, j] - lr * d / (math.sqrt(want_h) + eps)
            assert math.isclose(ref["p"][k, j], want_p, rel_tol=1e-13, abs_tol=1e-15)
            assert math.isclose(ref["G"][k, j], G, rel_tol=1e-13)
            if kind == "adagrad":
                assert math.isclose(ref["h"][k, j], want_h, rel_tol=1e-13)
    # the checker accepts the oracle's own result rounded to the value type
    for dt in (np.float32, np.float64):
        p_t, h_t = p.astype(dt), h.astype(dt)
        r = ou.step64(p_t, h_t, idx, grads.astype(dt), kind, lr, wd, eps)
        ou.check_step64(p_t, h_t, idx, grads.astype(dt), r["p"].astype(dt), r["h"].astype(dt), dt, kind, lr, wd, eps)
        moved = r["p"].astype(dt)
        moved[rows - 1, 0] += 1  # an untouched key changed: the checker must object
        assert ou.step_errors64(p_t, h_t, idx, grads.astype(dt), moved, r["h"].astype(dt), dt, kind, lr, wd, eps)


def _sequential(ref, p, h, idx, grads, rows, kind, lr, wd, eps):
    """The WRONG semantics at the keys `rows`: one step per occurrence, in call
    order (every other key as the oracle has it)."""
    pn, hn = ref["p"].copy(), ref["h"].copy()
    for k in rows:
        pk, hk = p[k:k + 1].astype(np.float64), h[k:k + 1].astype(np.float64)
        for i in np.flatnonzero(idx == k):
            r = ou.step64(pk, hk, [0], grads[i:i + 1], kind, lr, wd, eps)
            pk, hk = r["p"], r["h"]
        pn[k], hn[k] = pk[0], hk[0]
    return pn, hn


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_checker_rejects_wrong_semantics_on_the_gpu_tests_inputs(dt):
    """Every bound case of tests/test_opt_gpu.py that has a duplicated key: a
    result of m sequential steps, and a result with one loser's gradient
    dropped, both fall outside the tolerance at some duplicated key."""
    dt = np.dtype(dt)
    lr, eps = ou.BOUND_LR, ou.BOUND_EPS
    seen = 0
    for case in ou.bound_cases():
        li, n, w, pat, kind, wd = case
        kb, ke = LAYOUTS[li]
        p0, calls = ou.bound_steps(ou.case_seed(case, dt.name), kb, ke, n, w, pat, dt)
        p = p0.copy()
        h = np.full(p.shape, ou.BOUND_INIT_ACCUM, dtype=dt)
        for keys, grads in calls:
            idx = keys.astype(np.int64) - kb
            ref = ou.step64(p, h, idx, grads, kind, lr, wd, eps)
            good_p, good_h = ref["p"].astype(dt), ref["h"].astype(dt)
            ou.check_step64(p, h, idx, grads, good_p, good_h, dt, kind, lr, wd, eps, msg=str(case))
            dup = np.flatnonzero(ref["m"] > 1)
            if dup.size:
                seen += 1
                # (for SGD without weight decay m steps ARE one step on the sum; no such case is listed)
                sp, sh = _sequential(ref, p, h, idx, grads, dup[:4], kind, lr, wd, eps)
                assert ou.step_errors64(p, h, idx, grads, sp.astype(dt), sh.astype(dt), dt, kind, lr, wd, eps), \
                    f"sequential steps accepted: {case}"
                first = int(np.flatnonzero(idx == dup[0])[0])  # a loser: not the key's last occurrence
                keep = np.ones(idx.size, dtype=bool)
                keep[first] = False
                dr = ou.step64(p, h, idx[keep], grads[keep], kind, lr, wd, eps)
                assert ou.step_errors64(p, h, idx, grads, dr["p"].astype(dt), dr["h"].astype(dt), dt, kind, lr, wd,
                                      eps), f"a dropped loser accepted: {case}"
            p, h = good_p, good_h
    assert seen > 20


def test_dyadic_cases_are_exact_in_float32():
    """The float64 oracle's result of every dyadic SGD step is representable in
    float32, for up to 3 steps of up to 4100 occurrences of one key: the GPU's
    float32 (and float64) arithmetic then has nothing to round, whatever the
    order of the sums and with or without FMA contraction."""
    kb, ke = LAYOUTS[0]
    for n, w, pat in [(4100, 1, "all_equal"), (4100, 3, "dups_in_chunk"), (2049, 4, "dups_across_chunks"),
                      (2049, 16, "distinct"), (1, 33, "range_ends")]:
        p0, calls = ou.dyadic_steps(ou.case_seed(n, w, pat), kb, ke, n, w, pat, np.float32)
        p = p0.astype(np.float64)
        for keys, grads in calls:
            idx = keys.astype(np.int64) - kb
            assert np.array_equal(grads * 16, np.round(grads * 16)) and np.abs(grads).max() <= 8
            ref = ou.step64(p, None, idx, grads, "sgd", ou.DYADIC_LR)
            # every partial sum is a multiple of 2^-4 below 2^24 * 2^-4: exact in any order
            assert ref["G"].max() <= 4100 * 8 and ref["G"].max() * 16 < 2**24
            assert np.array_equal(ref["p"].astype(np.float32).astype(np.float64), ref["p"])
            assert np.array_equal(ref["p"] * 128, np.round(ref["p"] * 128))  # multiples of 2^-7
            assert np.abs(ref["p"]).max() * 128 < 2**24
            p = ref["p"]
