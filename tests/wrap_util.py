"""Helpers of the epoch wrap-around tests (tests/test_wrap_gpu.py).

A shard's stamp epoch is a uint32 that advances once per launch group
(DESIGN.md §8o); option EPOCH moves it forward, so `near_wrap(sh, d)` leaves
the shard d launch groups short of the last epoch, 0xFFFFFFFF: the group after
that one takes the wrap-around (the stamps and both tags reset, epoch 1).

`wrapping_shard_class` builds a Shard whose every writing call first moves the
epoch to 0xFFFFFFFF - d, d cycling through `schedule`: with d = 0 the wrap falls
before the call's first group, with 0 < d < G between two of its G groups, with
d = G right behind it (the next call takes it).  Every existing scenario that
makes its shards through `parameter_server_amd.Shard` runs unchanged on such a
class -- its reference knows nothing about epochs -- and, as its calls keep
hitting the same small key sets, every key is written on both sides of many
wrap-arounds.  `record`: every reply of the shard is appended to that list, for
the comparison of a run with the moves against one without.
"""
import numpy as np

LAST = 0xFFFFFFFF
WRITERS = ("add", "add_grouped", "add_get_grouped", "apply", "apply_grouped", "apply_pooled",
           "apply_pooled_grouped", "put_state")
SCHEDULE = (0, 1, 2, 0, 3, 1, 2, 0, 1)  # no period in common with an alternation of two or three calls


def epoch(sh):
    return sh.get_option("EPOCH")


def near_wrap(sh, d):
    """Leave `sh` d launch groups short of the last epoch; False (and nothing
    done) where the epoch is already beyond that."""
    v = LAST - int(d)
    if v < epoch(sh):
        return False
    sh.set_option("EPOCH", v)
    return True


class Stats:
    def __init__(self):
        self.calls = self.moves = self.wraps = 0


def _host_copy(x):
    return x.cpu().numpy().copy() if hasattr(x, "cpu") else np.array(x, copy=True)


def wrapping_shard_class(base, schedule=SCHEDULE, stats=None, record=None, only_sparse=False):
    """A subclass of `base` (parameter_server_amd.Shard) as the module docstring
    says.  schedule None: no moves (the recording twin).  only_sparse: a dense
    shard is left alone (the dense twin of a sparse shard stays a reference
    that never wraps)."""
    stats = stats if stats is not None else Stats()

    class WrappingShard(base):
        wrap_stats = stats

        def _around(self, name, *a, **kw):
            moved = False
            if schedule is not None and not (only_sparse and not self.is_sparse):
                n = getattr(self, "_wrap_calls", 0)
                self._wrap_calls = n + 1
                moved = near_wrap(self, schedule[n % len(schedule)])
            before = epoch(self)
            out = getattr(base, name)(self, *a, **kw)
            stats.calls += 1
            stats.moves += bool(moved)
            stats.wraps += epoch(self) < before
            return out

        def get(self, *a, **kw):
            out = base.get(self, *a, **kw)
            if record is not None:
                record.append(_host_copy(out))
            return out

        def get_state(self, *a, **kw):
            out = base.get_state(self, *a, **kw)
            if record is not None:
                record.append(_host_copy(out))
            return out

        def get_grouped(self, batches, *a, **kw):
            out = base.get_grouped(self, batches, *a, **kw)
            if record is not None and isinstance(batches, (list, tuple)):
                record.extend(_host_copy(o) for _, o in batches)
            return out

        def add_get_grouped(self, adds, gets, *a, **kw):
            out = self._around("add_get_grouped", adds, gets, *a, **kw)
            if record is not None and isinstance(gets, (list, tuple)):
                record.extend(_host_copy(o) for _, o in gets)
            return out

    def writer(name):
        def call(self, *a, **kw):
            return self._around(name, *a, **kw)
        call.__name__ = name
        return call

    for name in WRITERS:
        if name != "add_get_grouped":
            setattr(WrappingShard, name, writer(name))
    return WrappingShard


def same_records(a, b, what):
    """Two recordings of one scenario: the same replies, bit for bit."""
    assert len(a) == len(b), f"{what}: {len(a)} replies against {len(b)}"
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, i, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            u = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
            bad = np.flatnonzero(x.reshape(-1).view(u) != y.reshape(-1).view(u))
            raise AssertionError(f"{what}: reply {i} differs in {bad.size} of {x.size} values, first at "
                                 f"{bad[:3].tolist()}: {x.reshape(-1)[bad[0]]!r} against {y.reshape(-1)[bad[0]]!r}")
