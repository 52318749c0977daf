"""GPU tests of the score matrix pull (Shard.get_score_matrix): host and device
path, float32 and float64, row and sparse shards, against the wide reference
of tests/test_scores_gpu.py.  Bound (the dot product in any order of correctly
rounded operations): |got - ref| <= gamma_W * sum_j |q_j p_j|, gamma_W = W u /
(1 - W u)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from opt_util import case_seed
from rows_util import bits
from test_gpu_parity import tdev
from test_scores_gpu import KB, ROWS, UNWRITTEN, make, wide, wide_dots

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS, QUERIES = 64, 64  # kMatKeys, kMatQueries
N = 2 * KEYS + 5        # two whole windows and a short one
NQ = QUERIES + 17       # a whole block, then a whole MFMA tile and a short one


@functools.lru_cache(maxsize=None)
def case(dt, w):
    """Per (dtype, width), computed once: rows, the row of every position, queries, reference, tolerance."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(case_seed("score-matrix", dt.name, w))
    p = rng.standard_normal((ROWS, w)).astype(dt)
    p[ROWS - UNWRITTEN:] = 0
    idx = rng.integers(0, ROWS, N)  # repeated keys
    idx[:UNWRITTEN] = np.arange(ROWS - UNWRITTEN, ROWS)
    q = rng.standard_normal((NQ, w)).astype(dt)
    per_row = [wide_dots(np.broadcast_to(qb, p.shape), p) for qb in q]  # each query against the 64 distinct rows
    ref = np.stack([r for r, _ in per_row])[:, idx]
    mag = np.stack([m for _, m in per_row])[:, idx]
    u = 2.0 ** (-24 if dt == np.float32 else -53)
    return p, idx, q, ref, (w * u / (1 - w * u)) * mag


def matrix(sh, keys, q, cuda, pad=3, misalign=0):
    """The (nq, n) scores, written into rows of n + pad elements with guard elements before, between and after."""
    n, nq, lead = keys.size, len(q), 1 + misalign
    stride = n + pad
    if cuda is None:
        buf = np.full(lead + nq * stride + 1, 77.0, dtype=q.dtype)
        sh.get_score_matrix(keys, q, out=buf[lead: lead + nq * stride].reshape(nq, stride)[:, :n])
    else:
        import torch

        t = torch.full((lead + nq * stride + 1,), 77.0, dtype=getattr(torch, q.dtype.name), device=cuda)
        sh.get_score_matrix(tdev(keys, cuda), tdev(q.reshape(-1), cuda, offset=misalign),
                            t[lead: lead + nq * stride].view(nq, stride)[:, :n])
        buf = t.cpu().numpy()
    body = buf[lead: lead + nq * stride].reshape(nq, stride)
    got = body[:, :n].copy()
    body[:, :n] = 77.0
    assert (buf == 77.0).all(), "guards"
    return got


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sparse", [False, True], ids=["row", "sparse"])
@pytest.mark.parametrize("w", [1, 3, 4, 20, 64, 260, 4096])
def test_matrix_meets_the_wide_reference(cuda, w, sparse, device, dt):
    p, idx, q, ref, tol = case(np.dtype(dt).name, w)
    sh, K = make(dt, w, sparse, np.random.default_rng(case_seed("score-matrix-keys", w)))
    with sh:
        sh.add(K[: ROWS - UNWRITTEN], p[: ROWS - UNWRITTEN])
        got = matrix(sh, K[idx], q, cuda if device else None)
        sh.sync()
        err, tol = np.abs(wide(got.reshape(-1), ref.reshape(-1)) - ref.reshape(-1)).astype(np.float64), \
            tol.reshape(-1).astype(np.float64)
        print(f"W {w}: largest err / bound {np.max(err[tol > 0] / tol[tol > 0]):.3f}")
        assert (err <= tol).all(), (np.argmax(err - tol), err.max())
        assert (bits(got[:, idx >= ROWS - UNWRITTEN]) == 0).all(), "a zero row gives a column of +0"
        if sparse:
            assert sh.sparse_info()["count"] == ROWS - UNWRITTEN, "a read never inserts"


@pytest.mark.parametrize("w", [20, 260])
def test_the_bits_depend_on_row_query_and_width_alone(cuda, w):
    dt = np.float32
    rng = np.random.default_rng(case_seed("score-matrix-bits", w))
    p = rng.standard_normal((ROWS, w)).astype(dt)
    q = rng.standard_normal((NQ, w)).astype(dt)
    idx = rng.integers(0, ROWS, N)
    kp, qp = rng.permutation(N), rng.permutation(NQ)
    # mat_split (pskv_plan.h): N = 133 keys are 3 windows, which want ceil(1024 / 3) = 342 query groups; NQ = 81 makes
    # 2 blocks in 2 groups of one, and 343 * 64 + 17 = 21969 queries make 344 blocks in 172 groups of two
    big = 343 * QUERIES + 17
    a, Ka = make(dt, w, False)
    b, Kb = make(dt, w, True, rng)
    with a, b:
        a.add(Ka, p)
        b.add(Kb, p)
        want = matrix(a, Ka[idx], q, cuda)
        runs = {"twice": (matrix(a, Ka[idx], q, cuda), want),
                "keys permuted": (matrix(a, Ka[idx[kp]], q, cuda), want[:, kp]),
                "queries permuted": (matrix(a, Ka[idx], q[qp], cuda), want[qp]),
                "queries and out off 16 bytes": (matrix(a, Ka[idx], q, cuda, misalign=1), want),
                "out_stride = n": (matrix(a, Ka[idx], q, cuda, pad=0), want),
                "host": (matrix(a, Ka[idx], q, None), want),
                "sparse": (matrix(b, Kb[idx], q, cuda), want),
                "groups of two blocks": (matrix(a, Ka[idx], q[np.arange(big) % NQ], cuda), want[np.arange(big) % NQ])}
        for qi, ki in [(0, 0), (15, 16), (63, 63), (64, 64), (NQ - 1, N - 1)]:
            runs[f"the pair ({qi}, {ki}) alone"] = (matrix(a, Ka[idx[ki: ki + 1]], q[qi: qi + 1], cuda),
                                                    want[qi: qi + 1, ki: ki + 1])
        for name, (got, ref) in runs.items():
            assert np.array_equal(bits(got), bits(ref)), f"{name}: {int((bits(got) != bits(ref)).sum())} differ"


def test_the_call_only_reads(cuda):
    import parameter_server_amd as ps
    from parameter_server_amd import _lib

    w, n, nq = 8, KEYS + 36, 5
    rng = np.random.default_rng(case_seed("score-matrix-reads"))
    p = rng.standard_normal((ROWS, w)).astype(np.float32)
    q = rng.standard_normal((nq, w)).astype(np.float32)
    with ps.Shard(KB, KB + ROWS, np.float32, width=w) as sh, ps.Shard(KB, KB + ROWS, np.int32, width=w) as ints:
        K = np.arange(KB, KB + ROWS, dtype=np.uint32)
        sh.add(K, p)
        sh.sync()
        sh.set_timing(True)
        sh.reset_timing()
        dense = sh.dense_view().cpu().numpy().copy()
        before = {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)}
        gets = sh.info()["n_get_calls"]
        matrix(sh, K[rng.integers(0, ROWS, n)], q, cuda)
        sh.sync()
        assert sh.pooled_time()["launches"] == 1 and sh.pooled_time()["elements"] == n * nq
        assert {k: sh.kernel_time(k) for k in range(_lib.PSKV_K_COUNT)} == before
        assert sh.apply_time()["launches"] == 0 and sh.info()["n_get_calls"] == gets + 1
        assert np.array_equal(bits(sh.dense_view().cpu().numpy()), bits(dense))
        # no key, or no query: PSKV_OK, nothing written (the guards), nothing launched
        for path in (None, cuda):
            assert matrix(sh, K[:0], q, path).shape == (nq, 0)
            assert matrix(sh, K[:4], q[:0], path).shape == (0, 4)
        assert sh.pooled_time()["launches"] == 1
        with pytest.raises(Exception, match="float shards only"):
            ints.get_score_matrix(K[:4], np.zeros((2, w), np.int32))
        out = np.full((2, 4), 9.0, dtype=np.float32)
        with pytest.raises(Exception, match="out is untouched"):
            sh.get_score_matrix(np.array([KB, KB + ROWS, KB, KB], dtype=np.uint32), q[:2], out=out)
        assert (out == 9.0).all()


def test_score_matrix_through_hip_storage(cuda):
    """tests/cpp/hip_storage_score_matrix_test.cpp: SubGetScoreMatrix, a host and a device call, against a host loop."""
    exe = os.path.join(ROOT, "parameter_server_amd", "bin", "hip_storage_score_matrix_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
