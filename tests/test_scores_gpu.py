"""GPU tests of the score pull (Shard.get_scores): host and device path,
float32 and float64, row and sparse shards, against a plain reference in the
next wider precision.  Bound (the dot product in any order, with or without
fma): |got - ref| <= gamma_W * sum_j |q_j p_j|, gamma_W = W u / (1 - W u)."""
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from opt_util import case_seed
from rows_util import bits
from test_gpu_parity import tdev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = 7  # the first key of the row shards
WINDOW = 1024  # kScoreWindow
ROWS, UNWRITTEN = 64, 5  # the last rows are never written (a sparse shard: absent keys)
# an empty first bag, 1, 2, 7, an empty one, a bag that crosses a window edge, bags of one whose query rows pass
# the 32 KiB staging budget inside one window from W = 260 (f32: 31 rows), an empty last bag
LENS = [0, 1, 2, 7, 0, WINDOW + 3] + [1] * 40 + [0]


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def wide(x, like):
    if like.dtype != object:
        return x.astype(like.dtype)
    return np.array([Fraction(float(v)) for v in x], dtype=object)


def wide_dots(q, p):
    """sum_j q[i, j] p[i, j] and sum_j |q p| per position: float64 for float32; for float64 longdouble, or
    exact rationals where that is no wider.  256 positions at a time."""
    ld = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    dots, mags = [], []
    for i in range(0, len(q), 256):
        a, b = q[i: i + 256], p[i: i + 256]
        if q.dtype == np.float32 or ld:
            t = np.float64 if q.dtype == np.float32 else np.longdouble
            x = a.astype(t) * b.astype(t)
        else:
            x = np.array([[Fraction(float(u)) * Fraction(float(v)) for u, v in zip(r, s)] for r, s in zip(a, b)],
                         dtype=object).reshape(a.shape)
        dots.append(x.sum(axis=1))
        mags.append(np.abs(x).sum(axis=1))
    return np.concatenate(dots), np.concatenate(mags)


@functools.lru_cache(maxsize=None)
def case(dt, w):
    """Per (dtype, width), computed once: rows, the row of every position, offsets, queries, reference, tolerance."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(case_seed("scores", dt.name, w))
    p = rng.standard_normal((ROWS, w)).astype(dt)
    p[ROWS - UNWRITTEN:] = 0
    off = offsets_of(LENS)
    idx = rng.integers(0, ROWS, int(off[-1]))  # repeated keys
    idx[:UNWRITTEN] = np.arange(ROWS - UNWRITTEN, ROWS)
    q = rng.standard_normal((len(LENS), w)).astype(dt)
    ref, mag = wide_dots(q[np.repeat(np.arange(len(LENS)), LENS)], p[idx])
    u = 2.0 ** (-24 if dt == np.float32 else -53)
    return p, idx, off, q, ref, (w * u / (1 - w * u)) * mag


def make(dt, w, sparse, rng=None):
    """(shard, the key of every row): a row shard over [KB, KB + ROWS), or a sparse one over random keys."""
    import parameter_server_amd as ps

    if not sparse:
        return ps.Shard(KB, KB + ROWS, dt, width=w), np.arange(KB, KB + ROWS, dtype=np.uint32)
    K = np.unique(rng.integers(0, 2**32, 3 * ROWS, dtype=np.uint64))[:ROWS].astype(np.uint32)
    return ps.Shard.sparse(ROWS, dt, width=w), K[rng.permutation(ROWS)]


def scores(sh, keys, off, q, cuda, misalign=0):
    if cuda is None:
        return sh.get_scores(keys, off, q)
    import torch

    out = torch.full((keys.size + 2 + misalign,), 77.0, dtype=getattr(torch, q.dtype.name), device=cuda)
    view = out[1 + misalign: 1 + misalign + keys.size]
    sh.get_scores(tdev(keys, cuda), tdev(off.astype(np.int64), cuda), tdev(q.reshape(-1), cuda, offset=misalign), view)
    got = out.cpu().numpy()
    assert (got[: 1 + misalign] == 77.0).all() and (got[1 + misalign + keys.size:] == 77.0).all(), "guards"
    return got[1 + misalign: 1 + misalign + keys.size]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sparse", [False, True], ids=["row", "sparse"])
@pytest.mark.parametrize("w", [1, 3, 4, 20, 64, 260, 4096])
def test_scores_meet_the_wide_reference(cuda, w, sparse, device, dt):
    p, idx, off, q, ref, tol = case(np.dtype(dt).name, w)
    sh, K = make(dt, w, sparse, np.random.default_rng(case_seed("scores-keys", w)))
    with sh:
        sh.add(K[: ROWS - UNWRITTEN], p[: ROWS - UNWRITTEN])
        got = scores(sh, K[idx], off, q, cuda if device else None)
        sh.sync()
        err, tol = np.abs(wide(got, ref) - ref).astype(np.float64), tol.astype(np.float64)
        assert (err <= tol).all(), (np.argmax(err - tol), err.max())
        assert (bits(got[idx >= ROWS - UNWRITTEN]) == 0).all(), "a zero row scores +0"
        if sparse:
            assert sh.sparse_info()["count"] == ROWS - UNWRITTEN, "a read never inserts"


@pytest.mark.parametrize("w", [20, 260])
def test_the_bits_depend_on_row_query_and_width_alone(cuda, w):
    dt, m = np.float32, 2 * WINDOW + 70  # two windows lie inside the one bag
    rng = np.random.default_rng(case_seed("scores-bits", w))
    p = rng.standard_normal((ROWS, w)).astype(dt)
    q = rng.standard_normal((2, w)).astype(dt)
    idx = rng.integers(0, ROWS, m)
    a, Ka = make(dt, w, False)
    b, Kb = make(dt, w, True, rng)
    with a, b:
        a.add(Ka, p)
        b.add(Kb, p)
        one, each = offsets_of([m]), offsets_of([1] * m)
        want = scores(a, Ka[idx], one, q[:1], cuda)
        runs = {"twice": scores(a, Ka[idx], one, q[:1], cuda),
                "bags of one": scores(a, Ka[idx], each, np.repeat(q[:1], m, axis=0), cuda),
                "5 keys in front": scores(a, np.concatenate([Ka[:5], Ka[idx]]), offsets_of([5, m]), q[::-1], cuda)[5:],
                "queries and out off 16 bytes": scores(a, Ka[idx], one, q[:1], cuda, misalign=1),
                "host": scores(a, Ka[idx], one, q[:1], None),
                "sparse": scores(b, Kb[idx], one, q[:1], cuda),
                "sparse, host, bags of one": scores(b, Kb[idx], each, np.repeat(q[:1], m, axis=0), None)}
        for name, got in runs.items():
            assert np.array_equal(bits(got), bits(want)), f"{name}: {int((bits(got) != bits(want)).sum())} differ"


def test_the_call_only_reads(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    w, n = 8, WINDOW + 100
    rng = np.random.default_rng(case_seed("scores-reads"))
    p = rng.standard_normal((ROWS, w)).astype(np.float32)
    q = rng.standard_normal((3, w)).astype(np.float32)
    with ps.Shard(KB, KB + ROWS, np.float32, width=w) as sh, ps.Shard(KB, KB + ROWS, np.int32, width=w) as ints:
        K = np.arange(KB, KB + ROWS, dtype=np.uint32)
        sh.add(K, p)
        sh.sync()
        sh.set_timing(True)
        sh.reset_timing()
        dense = sh.dense_view().cpu().numpy().copy()
        before = {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)}
        gets = sh.info()["n_get_calls"]
        scores(sh, K[rng.integers(0, ROWS, n)], offsets_of([n - 9, 0, 9]), q, cuda)  # (checks the guards round out)
        sh.sync()
        assert sh.pooled_time()["launches"] == 1 and sh.pooled_time()["elements"] == n
        assert {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)} == before
        assert sh.apply_time()["launches"] == 0 and sh.info()["n_get_calls"] == gets + 1
        assert np.array_equal(bits(sh.dense_view().cpu().numpy()), bits(dense))
        # no bag, and three bags without a key: PSKV_OK, nothing written, nothing launched
        for path in (None, cuda):
            assert scores(sh, K[:0], offsets_of([]), q[:0], path).size == 0
            assert scores(sh, K[:0], offsets_of([0, 0, 0]), q, path).size == 0
        out = np.full(4, 9.0, dtype=np.float32)
        assert _lib.lib.pskv_get_scores(sh.handle, None, 0, None, None, 0, None, _lib.PSKV_HOST) == _lib.PSKV_OK
        assert sh.pooled_time()["launches"] == 1
        with pytest.raises(Exception, match="float shards only"):
            ints.get_scores(K[:4], offsets_of([4]), np.zeros(w, np.int32))
        with pytest.raises(Exception, match="out is untouched"):
            sh.get_scores(np.array([KB, KB + ROWS, KB, KB], dtype=np.uint32), offsets_of([4]), q[:1], out=out)
        assert (out == 9.0).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_push_then_scores_make_a_step(cuda, dt):
    """SGD, lr 1: row' = row - c_i q_b, so the score falls by c_i (q_b . q_b).  Bound: the reference's parts in
    the wide precision; gamma_W on both dot products, two roundings (product, difference) of the update per element."""
    import parameter_server_amd as ps

    dt, w, lens = np.dtype(dt), 20, [30, 20]
    rng = np.random.default_rng(case_seed("scores-step", dt.name))
    p = rng.standard_normal((ROWS, w)).astype(dt)
    q = rng.standard_normal((2, w)).astype(dt)
    c = rng.standard_normal(sum(lens)).astype(dt)
    idx, off = rng.permutation(ROWS)[: sum(lens)], offsets_of(lens)
    K = np.arange(KB, KB + ROWS, dtype=np.uint32)
    qi = q[np.repeat([0, 1], lens)]
    with ps.Shard(KB, KB + ROWS, dt, width=w) as sh:
        sh.set_optimizer("sgd", lr=1.0)
        sh.add(K, p)
        s0 = scores(sh, K[idx], off, q, cuda)
        sh.apply_pooled(tdev(K[idx], cuda), tdev(off.astype(np.int64), cuda), tdev(q.reshape(-1), cuda), tdev(c, cuda))
        s1 = scores(sh, K[idx], off, q, cuda)
        sh.sync()
    qq, _ = wide_dots(qi, qi)
    _, mag0 = wide_dots(qi, p[idx])
    u = 2.0 ** (-24 if dt == np.float32 else -53)
    g = w * u / (1 - w * u)
    cq = np.abs(c[:, None] * qi).astype(np.float64) * (1 + u)  # |c q_j|: the update's size per element
    _, mag1 = wide_dots(np.abs(qi).astype(np.float64), np.abs(p[idx]) + cq)  # a bound on sum_j |q_j row'_j|
    upd = (np.abs(qi) * (u * cq + u * (np.abs(p[idx]) + cq))).sum(axis=1)  # two roundings per element, times |q_j|
    tol = g * mag0 + g * mag1 * (1 + u) + upd
    err = np.abs(wide(s1, qq) - (wide(s0, qq) - wide(c, qq) * qq))
    assert (err <= tol).all(), (err.max(), tol.min())


def test_scores_through_hip_storage(cuda):
    """tests/cpp/hip_storage_scores_test.cpp: SubGetScores, a host and a device call, against a host loop."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_scores_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
