"""The row initializer (include/pskv.h, "Row initializers") restated in numpy:
Philox4x32-10 and the value formulas in float64.  This is the plain reference
of tests/test_init_cpu.py and tests/test_init_gpu.py.

NORMAL's bound: |got - (a + b z)| <= C * u_T * (|a| + |b| * rad), u_T the unit
roundoff of T (rows_util.U_ROUND).  float: C = 1 -- both sides evaluate in
double and differ only by where the one final rounding to float falls.
double: the device library's log, sin and cos against numpy's: the largest
ratio measured on the MI355X over the draws of tests/test_init_gpu.py is
C_F64_MEASURED; C is 4 times that (the draws do not reach the worst argument
of log and cos), and may never exceed 64: more is a wrong formula."""
import numpy as np

C_F64_MEASURED = 3.415  # float64, W = 1024, mean 0.25, std 2 (the largest of the widths' 1.15 .. 3.42)
C_NORMAL = {np.dtype(np.float32): 1.0, np.dtype(np.float64): 4 * C_F64_MEASURED}
assert max(C_NORMAL.values()) <= 64
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two.  Returns four uint64 arrays holding 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & M32 for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return c


def _u53(hi, lo):
    return (hi >> np.uint64(5)).astype(np.float64) * 2.0**26 + (lo >> np.uint64(6)).astype(np.float64)


def init_ref(keys, width, dt, kind, a=0.0, b=0.0, seed=0):
    """(rows, rad): rows (n, width) -- CONSTANT and UNIFORM in dt, exact bits;
    NORMAL the float64 value a + b z before its rounding to dt, rad alongside."""
    dt = np.dtype(dt)
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 1)
    per = 16 // dt.itemsize
    e = np.arange(width, dtype=np.uint64).reshape(1, -1)
    q, r = e // np.uint64(per), (e % np.uint64(per)).astype(np.int64)
    if kind == "constant":
        return np.full((keys.size, width), a, dtype=dt), None
    x = np.stack(philox4x32_10([keys + 0 * q, q + 0 * keys, 0, 0], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]))
    pick = lambda j: np.take_along_axis(x, np.broadcast_to(j, x.shape[1:])[None], 0)[0]  # noqa: E731
    if kind == "uniform":
        if dt.itemsize == 4:
            u = ((pick(r) >> np.uint64(8)).astype(np.float64) * 2.0**-24).astype(dt)
        else:
            u = _u53(pick(2 * r), pick(2 * r + 1)) * 2.0**-53
        return (u * dt.type(b - a)).astype(dt) + dt.type(a), None
    if dt.itemsize == 4:
        h = r // 2
        u1 = ((pick(2 * h) >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0**-24
        u2 = (pick(2 * h + 1) >> np.uint64(8)).astype(np.float64) * 2.0**-24
    else:
        u1 = (_u53(pick(0 * r), pick(0 * r + 1)) + 1.0) * 2.0**-53
        u2 = _u53(pick(0 * r + 2), pick(0 * r + 3)) * 2.0**-53
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    z = rad * np.where(r % 2 == 0, np.cos(ang), np.sin(ang))
    return a + b * z, np.broadcast_to(rad, z.shape)
