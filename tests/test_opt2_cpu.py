"""CPU tests of momentum and Adam steps: the new exports and constants, the
argument checks that need no device, the np.longdouble oracle of
tests/opt_util.py pinned against a per-key loop and (Adam) against
torch.optim.SparseAdam, the two conditions that bind the tolerances on the GPU
bound tests' own inputs, and the exactness of the dyadic momentum cases.  No
kernel is launched here."""
import ctypes
import math
import os

import numpy as np
import pytest

import opt_util as ou
from rows_util import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pskv_shard_set_optimizer_ex", "pskv_shard_get_optimizer_ex", "pskv_get_state_slot", "pskv_put_state",
       "pskv_get_step", "pskv_set_step"]


def _last_error():
    from parameter_server_amd import _lib

    return _lib.lib.pskv_last_error().decode()


def _cfg(**kw):
    from parameter_server_amd import _lib

    c = dict(size=ctypes.sizeof(_lib.PskvOptimizerEx), kind=4, lr=0.05, weight_decay=0.01, eps=1e-8, init_accum=0.1,
             momentum=0.9, nesterov=0, beta1=0.9, beta2=0.999)
    c.update(kw)
    return _lib.PskvOptimizerEx(c["size"], c["kind"], c["lr"], c["weight_decay"], c["eps"], c["init_accum"],
                                c["momentum"], c["nesterov"], c["beta1"], c["beta2"])


# ------------------------------------------------------- exports, constants
def test_new_symbols_are_exported_and_declared():
    from parameter_server_amd import _lib

    assert set(NEW) <= set(_lib.EXPORTED)
    header = open(os.path.join(ROOT, "include", "pskv.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(_lib.lib, name)
    assert (_lib.PSKV_OPT_MOMENTUM, _lib.PSKV_OPT_ADAM) == (3, 4)
    assert "PSKV_OPT_MOMENTUM = 3" in header and "PSKV_OPT_ADAM = 4" in header
    assert "} pskv_optimizer_ex;" in header
    for word in ("AdamW", "amsgrad", "per-key step counts"):  # what is not provided is said
        assert word in header, word
    # the struct as the C compiler lays it out: 4 + 4, 4 doubles, double, int (+ pad), 2 doubles
    assert ctypes.sizeof(_lib.PskvOptimizerEx) == 72
    assert _lib.PskvOptimizerEx.beta1.offset == 56


def test_kernel_ids_and_abi_version_are_unchanged():
    from parameter_server_amd import _lib

    assert _lib.PSKV_K_COUNT == 14
    assert _lib.lib.pskv_abi_version() == 1
    assert _lib.lib.pskv_kernel_time(None, 14, None, None, None) == _lib.PSKV_EINVAL
    header = open(os.path.join(ROOT, "include", "pskv.h")).read()
    assert "PSKV_K_COUNT = 14" in header and "#define PSKV_ABI_VERSION 1" in header


def test_null_shard_is_einval():
    from parameter_server_amd import _lib

    L = _lib.lib
    k = np.zeros(4, dtype=np.uint32)
    v = np.zeros(4, dtype=np.float32)
    cfg, out, nb, t = _cfg(), _lib.PskvOptimizerEx(), ctypes.c_uint64(), ctypes.c_uint64()
    calls = {
        "pskv_shard_set_optimizer_ex": lambda: L.pskv_shard_set_optimizer_ex(None, ctypes.byref(cfg)),
        "pskv_shard_get_optimizer_ex": lambda: L.pskv_shard_get_optimizer_ex(None, ctypes.byref(out),
                                                                             ctypes.byref(nb)),
        "pskv_get_state_slot": lambda: L.pskv_get_state_slot(None, 0, k.ctypes.data, 4, v.ctypes.data, 0),
        "pskv_put_state": lambda: L.pskv_put_state(None, 0, k.ctypes.data, v.ctypes.data, 4, 0),
        "pskv_get_step": lambda: L.pskv_get_step(None, ctypes.byref(t)),
        "pskv_set_step": lambda: L.pskv_set_step(None, 3),
    }
    assert set(calls) == set(NEW)
    for name, call in calls.items():
        assert call() == _lib.PSKV_EINVAL, name
        msg = _last_error()
        assert msg.startswith(name + ":") and "null shard" in msg, msg


@pytest.mark.parametrize("field,value,kind", [
    ("size", 0, 4), ("size", 40, 3), ("size", 80, 0),
    ("kind", 5, None), ("kind", -1, None),
    ("lr", 0.0, 3), ("lr", math.nan, 4), ("weight_decay", -1.0, 3), ("weight_decay", math.inf, 4),
    ("eps", 0.0, 4), ("eps", math.nan, 4), ("eps", -1.0, 2), ("init_accum", -1.0, 2),
    ("momentum", 1.0, 3), ("momentum", -0.1, 3), ("momentum", math.nan, 3),
    ("beta1", 1.0, 4), ("beta2", 1.0, 4), ("beta1", -0.5, 4), ("beta2", math.nan, 4),
    ("nesterov", 2, 3),
])
def test_set_optimizer_ex_reports_the_bad_field_without_a_shard(field, value, kind):
    from parameter_server_amd import _lib

    kw = {field: value}
    if kind is not None:
        kw["kind"] = kind
    cfg = _cfg(**kw)
    assert _lib.lib.pskv_shard_set_optimizer_ex(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
    msg = _last_error()
    assert field in msg and "null shard" not in msg, msg


def test_fields_a_kind_does_not_use_are_ignored():
    from parameter_server_amd import _lib

    for kw in (dict(kind=3, eps=0.0, init_accum=-1.0, beta1=2.0, beta2=math.nan),  # momentum: no eps, betas
               dict(kind=4, momentum=7.0, nesterov=9, init_accum=-1.0),  # Adam: no momentum fields
               dict(kind=1, eps=0.0, momentum=math.nan, nesterov=5, beta1=1.0),
               dict(kind=2, momentum=1.0, beta2=1.0),
               dict(kind=0, lr=0.0, weight_decay=-1.0, eps=0.0, momentum=1.0, beta1=1.0)):
        cfg = _cfg(**kw)
        assert _lib.lib.pskv_shard_set_optimizer_ex(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
        msg = _last_error()
        assert "null shard" in msg and " must" not in msg, msg
    assert _lib.lib.pskv_shard_set_optimizer_ex(None, None) == _lib.PSKV_EINVAL
    assert "null configuration" in _last_error()


def test_the_old_setter_still_refuses_the_new_kinds():
    from parameter_server_amd import _lib

    for kind in (3, 4):
        cfg = _lib.PskvOptimizer(kind, 0.05, 0.0, 1e-8, 0.0)
        assert _lib.lib.pskv_shard_set_optimizer(None, ctypes.byref(cfg)) == _lib.PSKV_EINVAL
        msg = _last_error()
        assert "kind" in msg and "null shard" not in msg, msg


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("kind,nesterov", [("momentum", False), ("momentum", True), ("adam", False)])
def test_oracle_matches_a_per_key_loop(kind, nesterov):
    rng = np.random.default_rng(12)
    w, rows, t = 3, 20, 3
    hp = ou.hyper(kind, wd=0.01, nesterov=nesterov)
    idx = rng.integers(0, rows - 2, size=50)  # the last two rows are never touched
    assert np.unique(idx).size < idx.size
    grads = rng.standard_normal((50, w)) * 3
    p = rng.standard_normal((rows, w))
    slots = [np.abs(rng.standard_normal((rows, w))) for _ in range(ou.SLOTS[kind])]
    ref = ou.step_ref(p, slots, idx, grads, hp, t)
    for k in range(rows):
        occ = [i for i in range(50) if idx[i] == k]
        assert ref["m"][k] == len(occ)
        if not occ:
            assert np.array_equal(ref["p"][k], p[k])
            for s, sn in zip(slots, ref["slots"]):
                assert np.array_equal(sn[k], s[k])
            continue
        for j in range(w):
            d = sum(float(grads[i, j]) for i in occ) + hp["wd"] * p[k, j]
            if kind == "momentum":
                v = hp["mu"] * slots[0][k, j] + d
                want_p = p[k, j] - hp["lr"] * ((d + hp["mu"] * v) if nesterov else v)
                want_s = [v]
            else:
                m = hp["beta1"] * slots[0][k, j] + (1 - hp["beta1"]) * d
                v = hp["beta2"] * slots[1][k, j] + (1 - hp["beta2"]) * d * d
                a = hp["lr"] / (1 - hp["beta1"]**t)
                b = 1 / math.sqrt(1 - hp["beta2"]**t)
                want_p = p[k, j] - a * m / (math.sqrt(v) * b + hp["eps"])
                want_s = [m, v]
            assert math.isclose(ref["p"][k, j], want_p, rel_tol=1e-12, abs_tol=1e-14)
            for sn, want in zip(ref["slots"], want_s):
                assert math.isclose(sn[k, j], want, rel_tol=1e-12, abs_tol=1e-14)
    # the checker accepts the oracle's own result rounded to the value type, and objects to a moved untouched key
    for dt in (np.float32, np.float64):
        p_t, s_t, g_t = p.astype(dt), [s.astype(dt) for s in slots], grads.astype(dt)
        r = ou.step_ref(p_t, s_t, idx, g_t, hp, t)
        got_p, got_s = r["p"].astype(dt), [s.astype(dt) for s in r["slots"]]
        ou.check_step(p_t, s_t, idx, g_t, got_p, got_s, dt, hp, t)
        for which in range(1 + len(got_s)):
            moved = [got_p.copy()] + [s.copy() for s in got_s]
            moved[which][rows - 1, 0] += 1
            assert ou.step_errors(p_t, s_t, idx, g_t, moved[0], moved[1:], dt, hp, t)


@pytest.mark.parametrize("coalesce", [False, True], ids=["distinct", "coalesced_duplicates"])
def test_adam_oracle_matches_torch_sparse_adam(coalesce):
    """torch.optim.SparseAdam, float64 on the CPU, weight_decay 0: an independent
    statement of the lazy rule (untouched rows keep p, m and v) and of the bias
    correction by the GLOBAL step.  Three steps over changing key sets.
    SparseAdam's denominator is (sqrt(v) + eps) b where the shard's (and dense
    torch Adam's) is sqrt(v) b + eps: SparseAdam with eps is exactly this rule
    with eps b(t), and that is what the oracle is given here."""
    import torch

    rng = np.random.default_rng(21 + coalesce)
    rows, w = 12, 3
    hp = ou.hyper("adam", lr=0.05, eps=1e-8, beta1=0.9, beta2=0.999)
    p0 = rng.standard_normal((rows, w))
    param = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.SparseAdam([param], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    p, slots = p0.copy(), ou.zero_slots("adam", p0.shape, np.float64)
    for t in (1, 2, 3):
        if coalesce:
            idx = rng.integers(0, rows - 3, size=9)  # duplicates: the sparse gradient sums them
            assert np.unique(idx).size < idx.size
        else:
            idx = rng.permutation(rows)[:5]
        grads = rng.standard_normal((idx.size, w))
        param.grad = torch.sparse_coo_tensor(torch.tensor(idx[None, :]), torch.tensor(grads), (rows, w)).coalesce()
        before = param.detach().numpy().copy()
        opt.step()
        ref = ou.step_ref(p, slots, idx, grads, dict(hp, eps=hp["eps"] * float(ou.bias_corrections(hp, t)[1])), t)
        untouched = np.setdiff1d(np.arange(rows), idx)
        assert np.array_equal(ref["p"][untouched], p[untouched])
        assert all(np.array_equal(sn[untouched], s[untouched]) for sn, s in zip(ref["slots"], slots))
        p, slots = ref["p"].astype(np.float64), [s.astype(np.float64) for s in ref["slots"]]
        st = opt.state[param]
        assert np.allclose(param.detach().numpy(), p, rtol=1e-12, atol=1e-14), t
        assert np.allclose(st["exp_avg"].numpy(), slots[0], rtol=1e-12, atol=1e-15), t
        assert np.allclose(st["exp_avg_sq"].numpy(), slots[1], rtol=1e-12, atol=1e-15), t
        assert np.array_equal(param.detach().numpy()[untouched], before[untouched])


# -------------------------------------------------------------- tolerances
def _walk(case, dt):
    """The bound case's three steps along the oracle: (t, p, slots, idx, grads, ref) per step."""
    kb, _ = LAYOUTS[case[0]]
    hp = ou.case_hyper(case)
    p0, calls = ou.bound_steps2(case, dt)
    p, slots = p0.copy(), ou.zero_slots(hp["kind"], p0.shape, dt)
    for t, (keys, grads) in enumerate(calls, 1):
        idx = keys.astype(np.int64) - kb
        pre = ou.prepare(p, slots, idx, grads, dt, hp, t)
        ref = pre[0]
        yield t, p, slots, idx, grads, pre, hp
        p, slots = ref["p"].astype(dt), [s.astype(dt) for s in ref["slots"]]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_an_emulation_of_the_kernel_order_passes_the_checker(dt):
    """Condition (a): on every bound case, the kernel's operation order in
    float32 / float64 numpy arithmetic -- the losers' rows added one by one in
    call order and in a random order, then the rule -- is inside the tolerances."""
    dt = np.dtype(dt)
    for case in ou.bound_cases2():
        rng = np.random.default_rng(ou.case_seed("perm", case))
        for t, p, slots, idx, grads, pre, hp in _walk(case, dt):
            for order in (None, rng):
                got_p, got_s = ou.emulate(p, slots, idx, grads, dt, hp, t, order)
                ou.check_step(p, slots, idx, grads, got_p, got_s, dt, hp, t, pre=pre, msg=f"{case} t {t}")


def _sequential(ref, p, slots, idx, grads, rows, hp, t):
    """The WRONG semantics at the keys `rows`: one step per occurrence, in call order."""
    pn, sn = ref["p"].copy(), [s.copy() for s in ref["slots"]]
    for k in rows:
        pk, sk = p[k:k + 1].astype(ou.F), [s[k:k + 1].astype(ou.F) for s in slots]
        for i in np.flatnonzero(idx == k):
            r = ou.step_ref(pk, sk, [0], grads[i:i + 1], hp, t)
            pk, sk = r["p"], r["slots"]
        pn[k] = pk[0]
        for s, x in zip(sn, sk):
            s[k] = x[0]
    return pn, sn


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_checker_rejects_wrong_semantics_on_the_gpu_tests_inputs(dt):
    """Condition (b): on every bound case and step with a duplicated key, a
    result of m sequential steps and a result with one loser's gradient dropped
    both fall outside the tolerance in at least one checked array."""
    dt = np.dtype(dt)
    seen = 0
    carried_by = set()
    for case in ou.bound_cases2():
        for t, p, slots, idx, grads, pre, hp in _walk(case, dt):
            ref = pre[0]
            ou.check_step(p, slots, idx, grads, ref["p"].astype(dt), [s.astype(dt) for s in ref["slots"]], dt, hp, t,
                          pre=pre, msg=str(case))
            dup = np.flatnonzero(ref["m"] > 1)
            if not dup.size:
                continue
            seen += 1
            sp, ss = _sequential(ref, p, slots, idx, grads, dup[:4], hp, t)
            bad = ou.step_errors(p, slots, idx, grads, sp.astype(dt), [s.astype(dt) for s in ss], dt, hp, t, pre=pre)
            assert bad, f"sequential steps accepted: {case} t {t}"
            carried_by |= {name for name, _ in bad}
            first = int(np.flatnonzero(idx == dup[0])[0])  # a loser: not the key's last occurrence
            keep = np.ones(idx.size, dtype=bool)
            keep[first] = False
            dr = ou.step_ref(p, slots, idx[keep], grads[keep], hp, t)
            bad = ou.step_errors(p, slots, idx, grads, dr["p"].astype(dt), [s.astype(dt) for s in dr["slots"]], dt,
                                 hp, t, pre=pre)
            assert bad, f"a dropped loser accepted: {case} t {t}"
            carried_by |= {name for name, _ in bad}
    assert seen > 100
    assert {"m", "v"} <= carried_by


# ---------------------------------------------------------- dyadic momentum
def _exact32(x):
    x = np.asarray(x, dtype=ou.F)
    return np.array_equal(x.astype(np.float32).astype(ou.F), x)


@pytest.mark.parametrize("nesterov", [False, True])
def test_dyadic_momentum_cases_are_exact_in_float32(nesterov):
    """momentum 0.5, lr 2^-3, no weight decay, opt_util's dyadic inputs, three
    steps, up to 4100 occurrences of one key: every partial sum of the
    gradients (in any order) and every intermediate of the rule -- mu v, the new
    v, the Nesterov sum, lr times it, the new p -- is representable in float32,
    so float32 and float64 arithmetic have nothing to round, with or without
    FMA contraction."""
    hp = ou.dyadic_hyper(nesterov)
    mu, lr = ou.F(hp["mu"]), ou.F(hp["lr"])
    for n, w, pat in [(4100, 1, "all_equal"), (4100, 3, "dups_in_chunk"), (2049, 4, "dups_across_chunks"),
                      (2049, 16, "distinct"), (1, 33, "range_ends"), (4100, 64, "all_equal")]:
        kb, _ = LAYOUTS[0]
        p0, calls = ou.dyadic_steps2(n, w, pat, 0, np.float32)
        assert len(calls) == 3
        p, v = p0.astype(ou.F), np.zeros(p0.shape, dtype=ou.F)
        for keys, grads in calls:
            idx = keys.astype(np.int64) - kb
            assert np.array_equal(grads * 16, np.round(grads * 16)) and np.abs(grads).max() <= 8
            ref = ou.step_ref(p, [v], idx, grads, hp)
            # every partial sum is a multiple of 2^-4 below 2^24 * 2^-4: exact in any order
            assert ref["G"].max() * 16 < 2**24
            d, vn = ref["d"], ref["slots"][0]
            step = d + mu * vn if nesterov else vn
            for x in (d, mu * v, vn, mu * vn, step, lr * step, ref["p"]):
                assert _exact32(x), (n, w, pat)
            p, v = ref["p"], vn
