"""Shard: Python handle on one HBM-resident parameter shard (pskv_shard).

Host inputs are numpy arrays (they stand for the zmq receive buffers the
reference storage sees, comm/mailbox.cpp:246-257); device inputs are torch
tensors on the shard's GPU (PyTorch only supplies memory and streams — every
byte of the Add/Get work is done by the HIP kernels in libpskv.so).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib

_NP_DTYPE = {_lib.PSKV_I32: np.dtype(np.int32), _lib.PSKV_F32: np.dtype(np.float32),
             _lib.PSKV_F64: np.dtype(np.float64)}
_DTYPE_CODE = {v: k for k, v in _NP_DTYPE.items()}


def dtype_code(dtype) -> int:
    try:
        import torch

        if isinstance(dtype, torch.dtype):
            dtype = {torch.int32: np.int32, torch.float32: np.float32, torch.float64: np.float64}[dtype]
    except ImportError:
        pass
    return _DTYPE_CODE[np.dtype(dtype)]


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def device_count() -> int:
    return int(lib.pskv_device_count())


class Shard:
    """A key range [key_begin, key_end) of uint32 keys held in HBM.

    mode "assign" is the reference semantics (last write wins, missing -> 0);
    "accumulate" is the gradient-reduction mode (param[k] += v).

    width > 1 makes a row shard: every key holds `width` values (an embedding
    row).  add takes values shaped (n, width) or flat n * width, get returns
    (n, width); counts stay in keys.  A row shard stores no key outside its
    range (include/pskv.h: the one limit).

    capacity > 0 (or Shard.sparse) makes a sparse shard instead: it owns every
    uint32 key and holds at most `capacity` distinct ones, at any width, its
    memory following capacity and not the key space (include/pskv.h, "Sparse
    shards").  key_begin, key_end and overflow_slots are not used.  reserve,
    set_growth and erase change what it holds room for; `capacity` follows
    reserve and load_state_dict, sparse_info()["capacity"] is always current."""

    def __init__(self, key_begin: int = 0, key_end: int = 1 << 32, dtype=np.float32,
                 mode: str = "assign", device: int = 0, overflow_slots: int = 0, options=None,
                 width: int = 1, capacity: int = 0):
        self.dtype = np.dtype(dtype) if not _is_torch(dtype) else _NP_DTYPE[dtype_code(dtype)]
        self.code = dtype_code(self.dtype)
        self.mode = {"assign": _lib.PSKV_ASSIGN, "accumulate": _lib.PSKV_ACCUMULATE}[mode]
        self.key_begin, self.key_end, self.device = int(key_begin), int(key_end), int(device)
        self.width = int(width)
        if not 0 <= self.width < 1 << 32:
            raise ValueError(f"width {width} out of range")
        h = ctypes.c_void_p()
        self.capacity = int(capacity)
        self.is_sparse = self.capacity != 0
        if self.is_sparse:
            if not 0 < self.capacity < 1 << 64:
                raise ValueError(f"capacity {capacity} out of range")
            self.key_begin, self.key_end = 0, 1 << 32
            check(lib.pskv_shard_create_sparse(self.device, self.capacity, self.code, self.mode, self.width,
                                               ctypes.byref(h)))
        else:
            check(lib.pskv_shard_create_rows(self.device, self.key_begin, self.key_end, self.code,
                                             self.mode, self.width, int(overflow_slots), ctypes.byref(h)))
        self._h = h
        for name, value in (options or {}).items():
            self.set_option(name, value)

    @classmethod
    def sparse(cls, capacity: int, dtype=np.float32, mode: str = "assign", device: int = 0, width: int = 1,
               options=None, max_capacity=None) -> "Shard":
        """A sparse shard of at most `capacity` distinct keys (pskv_shard_create_sparse).
        max_capacity: writing calls may grow it up to that many (set_growth)."""
        if int(capacity) == 0:
            raise ValueError("Shard.sparse: capacity must be positive")
        s = cls(dtype=dtype, mode=mode, device=device, options=options, width=width, capacity=capacity)
        if max_capacity is not None:
            try:
                s.set_growth(max_capacity)
            except Exception:
                s.close()
                raise
        return s

    # ------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.pskv_shard_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    # ------------------------------------------------------------ helpers
    def _host_keys(self, keys):
        return np.ascontiguousarray(keys, dtype=np.uint32)

    def _host_vals(self, vals, n):
        v = np.ascontiguousarray(vals, dtype=self.dtype)
        if v.size != n * self.width:
            if self.width > 1:
                raise ValueError(f"CHECK_EQ(keys.size() * width, vals.size()) failed: {n} * {self.width} vs {v.size}")
            raise ValueError(f"CHECK_EQ(keys.size(), vals.size()) failed: {n} vs {v.size}")
        return v

    def _check_dev_count(self, keys, vals):
        if vals.numel() != keys.numel() * self.width:
            if self.width > 1:
                raise ValueError(f"CHECK_EQ(keys.size() * width, vals.size()) failed: "
                                 f"{keys.numel()} * {self.width} vs {vals.numel()}")
            raise ValueError("CHECK_EQ(keys.size(), vals.size()) failed")

    # ------------------------------------------------------------ Add / Get
    def add(self, keys, vals, sorted_hint: bool = False, frame: bool = False):
        """Push one batch.  numpy -> host path; torch CUDA tensors -> device path.
        frame=True: host arrays that live in HostFrames are borrowed until the
        frames are freed (PSKV_HOST_FRAME): read in place, no wait."""
        if _is_torch(keys):
            self._check_dev(keys, vals)
            flags = _lib.PSKV_DEVICE | (_lib.PSKV_SORTED_HINT if sorted_hint else 0)
            self._check_dev_count(keys, vals)
            check(lib.pskv_add(self._h, keys.data_ptr(), vals.data_ptr(), keys.numel(), flags))
            return
        k = self._host_keys(keys)
        v = self._host_vals(vals, k.size)
        flags = _lib.PSKV_HOST_FRAME if frame else _lib.PSKV_HOST
        check(lib.pskv_add(self._h, k.ctypes.data, v.ctypes.data, k.size, flags))

    def get(self, keys, out=None, frame: bool = False):
        """Pull one batch.  numpy keys -> returns a numpy array (synchronous);
        torch keys -> fills/returns a torch tensor (stream-ordered)."""
        if _is_torch(keys):
            import torch

            if out is None:
                shape = (keys.numel(), self.width) if self.width > 1 else keys.numel()
                out = torch.empty(shape, dtype=_torch_dtype(self.dtype), device=keys.device)
            self._check_dev(keys, out)
            if self.width > 1:
                self._check_dev_count(keys, out)
            check(lib.pskv_get(self._h, keys.data_ptr(), keys.numel(), out.data_ptr(),
                               _lib.PSKV_DEVICE))
            return out
        k = self._host_keys(keys)
        if self.width > 1:
            if out is None:
                out = np.empty((k.size, self.width), dtype=self.dtype)
            elif not (isinstance(out, np.ndarray) and out.dtype == self.dtype and out.flags.c_contiguous
                      and out.size == k.size * self.width):
                raise ValueError("row shard: out must be a C-contiguous array of keys * width values")
        res = np.empty(k.size, dtype=self.dtype) if out is None else out
        flags = _lib.PSKV_HOST_FRAME if frame else _lib.PSKV_HOST
        check(lib.pskv_get(self._h, k.ctypes.data, k.size, res.ctypes.data, flags))
        return res

    def get_pooled(self, keys, offsets, weights=None, out=None):
        """One pooled row per bag (pskv_get_pooled): bag b is keys[offsets[b] :
        offsets[b+1]], its row sum_i weights[i] * row(keys[i]) (weights None:
        every weight one).  numpy inputs -> host path, returns a numpy array;
        torch tensors -> device path (offsets an int64 tensor), stream-ordered.
        Returns (nbags, width), or (nbags,) at width 1."""
        if _is_torch(keys):
            import torch

            if offsets.dtype != torch.int64 or offsets.numel() < 1:
                raise ValueError("get_pooled: device offsets must be an int64 tensor of nbags + 1 values")
            nbags = offsets.numel() - 1
            tdt = _torch_dtype(self.dtype)
            ts = [keys, offsets]
            if weights is not None:
                if weights.dtype != tdt or weights.numel() != keys.numel():
                    raise ValueError("get_pooled: weights must hold one value of the shard's dtype per key")
                ts.append(weights)
            if out is None:
                out = torch.empty((nbags, self.width) if self.width > 1 else nbags, dtype=tdt, device=keys.device)
            elif out.dtype != tdt or out.numel() != nbags * self.width:
                raise ValueError("get_pooled: out must hold nbags * width values of the shard's dtype")
            self._check_dev(*ts, out)
            check(lib.pskv_get_pooled(self._h, keys.data_ptr(), keys.numel(),
                                      weights.data_ptr() if weights is not None else None, offsets.data_ptr(),
                                      nbags, out.data_ptr(), _lib.PSKV_DEVICE))
            return out
        k = self._host_keys(keys)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.size < 1:
            raise ValueError("get_pooled: offsets must hold nbags + 1 values")
        nbags = off.size - 1
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=self.dtype)
            if w.size != k.size:
                raise ValueError(f"get_pooled: {w.size} weights for {k.size} keys")
        if out is None:
            out = np.empty((nbags, self.width) if self.width > 1 else nbags, dtype=self.dtype)
        elif not (isinstance(out, np.ndarray) and out.dtype == self.dtype and out.flags.c_contiguous
                  and out.size == nbags * self.width):
            raise ValueError("get_pooled: out must be a C-contiguous array of nbags * width values")
        check(lib.pskv_get_pooled(self._h, k.ctypes.data, k.size, w.ctypes.data if w is not None else None,
                                  off.ctypes.data, nbags, out.ctypes.data, _lib.PSKV_HOST))
        return out

    def pooled_time(self):
        """Pooled pulls timed as one operation each (pskv_pooled_time)."""
        n, ms, el = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
        check(lib.pskv_pooled_time(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(el)))
        return {"launches": n.value, "total_ms": ms.value, "elements": el.value}

    def prepare(self, batches, is_get: bool = False) -> "BatchSet":
        """Validate and pack a batch list once, for repeated grouped calls."""
        arr, keep, flags = self._batch_array(batches, is_get=is_get)
        return BatchSet(arr, len(batches), flags, keep)

    def add_grouped(self, batches, sorted_hint: bool = False, frame: bool = False):
        """batches: list of (keys, vals) (all torch-device or all numpy-host) or a BatchSet."""
        bs = batches if isinstance(batches, BatchSet) else self.prepare(batches)
        flags = bs.flags
        if sorted_hint and flags & _lib.PSKV_DEVICE:
            flags |= _lib.PSKV_SORTED_HINT
        if frame and not flags & _lib.PSKV_DEVICE:
            flags |= _lib.PSKV_HOST_FRAME
        check(lib.pskv_add_grouped(self._h, bs.arr, bs.n, flags))

    def get_grouped(self, batches, frame: bool = False):
        """batches: list of (keys, out) pairs (out filled in place) or a BatchSet."""
        bs = batches if isinstance(batches, BatchSet) else self.prepare(batches, is_get=True)
        flags = bs.flags
        if frame and not flags & _lib.PSKV_DEVICE:
            flags |= _lib.PSKV_HOST_FRAME
        check(lib.pskv_get_grouped(self._h, bs.arr, bs.n, flags))

    def add_get_grouped(self, adds, gets, sorted_hint: bool = False):
        """add_grouped(adds) then get_grouped(gets) in ONE call (pskv_add_get_grouped:
        the BSP model's flush then the Gets it releases, or a worker round's push
        then pull); the hint applies to the Adds.  adds / gets: batch lists or
        BatchSets."""
        ba = adds if isinstance(adds, BatchSet) else self.prepare(adds)
        bg = gets if isinstance(gets, BatchSet) else self.prepare(gets, is_get=True)
        if (ba.flags ^ bg.flags) & _lib.PSKV_DEVICE and ba.n and bg.n:
            raise ValueError("add_get_grouped: adds and gets must both be device or both host batches")
        flags = ba.flags if ba.n else bg.flags
        if sorted_hint and flags & _lib.PSKV_DEVICE:
            flags |= _lib.PSKV_SORTED_HINT
        check(lib.pskv_add_get_grouped(self._h, ba.arr, ba.n, bg.arr, bg.n, flags))

    # ------------------------------------------------------------ optimizer steps
    _OPT_KIND = {None: _lib.PSKV_OPT_NONE, "none": _lib.PSKV_OPT_NONE, "sgd": _lib.PSKV_OPT_SGD,
                 "adagrad": _lib.PSKV_OPT_ADAGRAD, "momentum": _lib.PSKV_OPT_MOMENTUM, "adam": _lib.PSKV_OPT_ADAM,
                 "ftrl": _lib.PSKV_OPT_FTRL}
    _OPT_NAME = {_lib.PSKV_OPT_NONE: None, _lib.PSKV_OPT_SGD: "sgd", _lib.PSKV_OPT_ADAGRAD: "adagrad",
                 _lib.PSKV_OPT_MOMENTUM: "momentum", _lib.PSKV_OPT_ADAM: "adam", _lib.PSKV_OPT_FTRL: "ftrl"}
    _OPT_SLOTS = {None: 0, "sgd": 0, "adagrad": 1, "momentum": 1, "adam": 2, "ftrl": 2}

    def set_optimizer(self, kind, lr: float = 0.0, weight_decay: float = 0.0, eps: float = 1e-10,
                      init_accum=None, momentum: float = 0.0, nesterov: bool = False,
                      beta1: float = 0.9, beta2: float = 0.999, l1: float = 0.0, l2: float = 0.0,
                      ftrl_beta: float = 1.0):
        """pskv_shard_set_optimizer(_ex, _cfg): kind "sgd", "adagrad", "momentum",
        "adam", "ftrl" or None.  The same kind again changes the hyper-parameters
        of later steps only (state and step count stay); another kind resets
        both.  init_accum None: 0.1 for "ftrl" (n must not start at 0 beside
        ftrl_beta = 0), else 0."""
        code = self._OPT_KIND[kind]
        if init_accum is None:
            init_accum = 0.1 if code == _lib.PSKV_OPT_FTRL else 0.0
        if code == _lib.PSKV_OPT_FTRL:
            cfg = _lib.PskvOptimizerCfg(ctypes.sizeof(_lib.PskvOptimizerCfg), code, float(lr), float(weight_decay),
                                        float(eps), float(init_accum), float(momentum), int(nesterov), float(beta1),
                                        float(beta2), float(l1), float(l2), float(ftrl_beta))
            check(lib.pskv_shard_set_optimizer_cfg(self._h, ctypes.byref(cfg)))
            return
        if code in (_lib.PSKV_OPT_MOMENTUM, _lib.PSKV_OPT_ADAM):
            cfg = _lib.PskvOptimizerEx(ctypes.sizeof(_lib.PskvOptimizerEx), code, float(lr), float(weight_decay),
                                       float(eps), float(init_accum), float(momentum), int(nesterov), float(beta1),
                                       float(beta2))
            check(lib.pskv_shard_set_optimizer_ex(self._h, ctypes.byref(cfg)))
            return
        cfg = _lib.PskvOptimizer(code, float(lr), float(weight_decay), float(eps), float(init_accum))
        check(lib.pskv_shard_set_optimizer(self._h, ctypes.byref(cfg)))

    def optimizer(self) -> dict:
        """The configuration, and `state_bytes`: what the optimizer holds in HBM
        beyond the dense array.  "momentum" adds momentum and nesterov, "adam"
        beta1 and beta2, "ftrl" l1, l2 and ftrl_beta."""
        cfg, nbytes = _lib.PskvOptimizerCfg(), ctypes.c_uint64()
        check(lib.pskv_shard_get_optimizer_cfg(self._h, ctypes.byref(cfg), ctypes.byref(nbytes)))
        d = {"kind": self._OPT_NAME[cfg.kind], "lr": cfg.lr, "weight_decay": cfg.weight_decay,
             "eps": cfg.eps, "init_accum": cfg.init_accum, "state_bytes": nbytes.value}
        if cfg.kind == _lib.PSKV_OPT_MOMENTUM:
            d.update(momentum=cfg.momentum, nesterov=bool(cfg.nesterov))
        elif cfg.kind == _lib.PSKV_OPT_ADAM:
            d.update(beta1=cfg.beta1, beta2=cfg.beta2)
        elif cfg.kind == _lib.PSKV_OPT_FTRL:
            d.update(l1=cfg.l1, l2=cfg.l2, ftrl_beta=cfg.ftrl_beta)
        return d

    def apply(self, keys, grads):
        """One optimizer step from one batch of (key, gradient-row) pairs, shaped
        as add's.  numpy -> host path; torch CUDA tensors -> device path."""
        if _is_torch(keys):
            self._check_dev(keys, grads)
            self._check_dev_count(keys, grads)
            check(lib.pskv_apply(self._h, keys.data_ptr(), grads.data_ptr(), keys.numel(), _lib.PSKV_DEVICE))
            return
        k = self._host_keys(keys)
        g = self._host_vals(grads, k.size)
        check(lib.pskv_apply(self._h, k.ctypes.data, g.ctypes.data, k.size, _lib.PSKV_HOST))

    def apply_grouped(self, batches):
        """ONE optimizer step over every batch: list of (keys, grads) or a BatchSet."""
        bs = batches if isinstance(batches, BatchSet) else self.prepare(batches)
        check(lib.pskv_apply_grouped(self._h, bs.arr, bs.n, bs.flags))

    def _pooled_push_batch(self, who, keys, offsets, bag_grads, weights):
        """The checks of one pooled push's four arrays (`who` opens the
        messages).  Returns (keys, weights, offsets, bag_grads pointers, n,
        nbags), the call's flags and the host arrays behind the pointers, which
        the caller keeps until its call has returned."""
        if _is_torch(keys):
            import torch

            if offsets.dtype != torch.int64 or offsets.numel() < 1:
                raise ValueError(f"{who}: device offsets must be an int64 tensor of nbags + 1 values")
            nbags = offsets.numel() - 1
            tdt = _torch_dtype(self.dtype)
            ts = [keys, offsets, bag_grads]
            if weights is not None:
                if weights.dtype != tdt or weights.numel() != keys.numel():
                    raise ValueError(f"{who}: weights must hold one value of the shard's dtype per key")
                ts.append(weights)
            if bag_grads.dtype != tdt or bag_grads.numel() != nbags * self.width:
                raise ValueError(f"{who}: bag_grads must hold nbags * width values of the shard's dtype")
            self._check_dev(*ts)
            return ((keys.data_ptr(), weights.data_ptr() if weights is not None else None, offsets.data_ptr(),
                     bag_grads.data_ptr(), keys.numel(), nbags), _lib.PSKV_DEVICE, None)
        k = self._host_keys(keys)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.size < 1:
            raise ValueError(f"{who}: offsets must hold nbags + 1 values")
        nbags = off.size - 1
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=self.dtype)
            if w.size != k.size:
                raise ValueError(f"{who}: {w.size} weights for {k.size} keys")
        g = np.ascontiguousarray(bag_grads, dtype=self.dtype)
        if g.size != nbags * self.width:
            raise ValueError(f"{who}: {g.size} bag gradient values for {nbags} bags of width {self.width}")
        return ((k.ctypes.data, w.ctypes.data if w is not None else None, off.ctypes.data, g.ctypes.data, k.size,
                 nbags), _lib.PSKV_HOST, (k, off, w, g))

    def apply_pooled(self, keys, offsets, bag_grads, weights=None):
        """One optimizer step from one gradient row per bag (pskv_apply_pooled):
        the gradient row of keys[i] is weights[i] * bag_grads[b], b the bag with
        offsets[b] <= i < offsets[b+1] (weights None: the bag's row itself).
        Arguments as get_pooled's, with bag_grads (nbags * width values) in the
        place of its output.  numpy -> host path; torch tensors -> device path
        (offsets an int64 tensor), stream-ordered."""
        (pk, pw, po, pg, n, nbags), flags, keep = self._pooled_push_batch("apply_pooled", keys, offsets, bag_grads,
                                                                          weights)
        check(lib.pskv_apply_pooled(self._h, pk, n, pw, po, nbags, pg, flags))
        del keep

    def apply_pooled_grouped(self, batches):
        """ONE optimizer step from several pooled pushes (pskv_apply_pooled_grouped):
        `batches` is a list of (keys, offsets, bag_grads) or (keys, offsets,
        bag_grads, weights), each shaped as apply_pooled's arguments; the step
        is the one apply_pooled would make of their concatenation.  All numpy
        -> host path; all torch tensors on the shard's device -> device path."""
        batches = [tuple(b) for b in batches]
        for b in batches:
            if len(b) not in (3, 4):
                raise ValueError("apply_pooled_grouped: a batch is (keys, offsets, bag_grads[, weights])")
        dev = [_is_torch(b[0]) for b in batches]
        if any(dev) and not all(dev):
            raise ValueError("apply_pooled_grouped: the batches must all be device or all host batches")
        arr = (_lib.PskvPoolBatch * max(len(batches), 1))()
        keep = []  # the host arrays behind the pointers, alive until the call returns
        flags = _lib.PSKV_HOST
        for i, b in enumerate(batches):
            (pk, pw, po, pg, n, nbags), flags, held = self._pooled_push_batch(
                f"apply_pooled_grouped: batch {i}", b[0], b[1], b[2], b[3] if len(b) == 4 else None)
            keep.append(held)
            arr[i] = _lib.PskvPoolBatch(pk, pw, po, pg, n, nbags)
        check(lib.pskv_apply_pooled_grouped(self._h, arr, len(batches), flags))
        del keep

    def get_state(self, keys, out=None, slot: int = 0):
        """The rows of `keys` in state slot `slot` (pskv_get_state_slot; Adagrad
        h, momentum v, Adam m and v, FTRL z and n), as get returns values."""
        if _is_torch(keys):
            import torch

            if out is None:
                shape = (keys.numel(), self.width) if self.width > 1 else keys.numel()
                out = torch.empty(shape, dtype=_torch_dtype(self.dtype), device=keys.device)
            self._check_dev(keys, out)
            self._check_dev_count(keys, out)
            check(lib.pskv_get_state_slot(self._h, int(slot), keys.data_ptr(), keys.numel(), out.data_ptr(),
                                          _lib.PSKV_DEVICE))
            return out
        k = self._host_keys(keys)
        if out is None:
            out = np.empty((k.size, self.width) if self.width > 1 else k.size, dtype=self.dtype)
        elif not (isinstance(out, np.ndarray) and out.dtype == self.dtype and out.flags.c_contiguous
                  and out.size == k.size * self.width):
            raise ValueError("get_state: out must be a C-contiguous array of keys * width values")
        check(lib.pskv_get_state_slot(self._h, int(slot), k.ctypes.data, k.size, out.ctypes.data, _lib.PSKV_HOST))
        return out

    def put_state(self, keys, vals, slot: int = 0):
        """Write state rows (pskv_put_state): shaped as add's, the last occurrence
        of a key wins with its whole row."""
        if _is_torch(keys):
            self._check_dev(keys, vals)
            self._check_dev_count(keys, vals)
            check(lib.pskv_put_state(self._h, int(slot), keys.data_ptr(), vals.data_ptr(), keys.numel(),
                                     _lib.PSKV_DEVICE))
            return
        k = self._host_keys(keys)
        v = self._host_vals(vals, k.size)
        check(lib.pskv_put_state(self._h, int(slot), k.ctypes.data, v.ctypes.data, k.size, _lib.PSKV_HOST))

    @property
    def step(self) -> int:
        """Optimizer steps since creation, clear or a kind change (pskv_get_step)."""
        t = ctypes.c_uint64()
        check(lib.pskv_get_step(self._h, ctypes.byref(t)))
        return t.value

    @step.setter
    def step(self, t: int):
        check(lib.pskv_set_step(self._h, int(t)))

    def state_dict(self) -> dict:
        """A checkpoint: the whole range's parameters, every state slot and the
        step count, as host arrays.  A sparse shard saves its stored keys
        ("keys") and their rows."""
        if self.is_sparse:
            keys = self.keys()
        else:
            keys = np.arange(self.key_begin, self.key_end, dtype=np.int64).astype(np.uint32)
        o = self.optimizer()
        d = {"p": self.get(keys), "slots": [self.get_state(keys, slot=i) for i in range(self._OPT_SLOTS[o["kind"]])],
             "t": self.step, "optimizer": o}
        if self.is_sparse:
            d["keys"] = keys
        return d

    def load_state_dict(self, d: dict):
        """Restore state_dict()'s checkpoint into a shard of the same range,
        width, dtype and optimizer kind (a sparse shard's: into a sparse shard
        with room for the saved keys)."""
        if self.is_sparse != ("keys" in d):
            raise ValueError("load_state_dict: a sparse shard's checkpoint goes into a sparse shard, a dense one's "
                             "into a dense one")
        if self.is_sparse:
            keys = np.ascontiguousarray(d["keys"], dtype=np.uint32)
        else:
            keys = np.arange(self.key_begin, self.key_end, dtype=np.int64).astype(np.uint32)
        kind = self.optimizer()["kind"]
        if len(d["slots"]) != self._OPT_SLOTS[kind]:
            raise ValueError(f"load_state_dict: {len(d['slots'])} state slots for optimizer {kind!r}")
        if self.is_sparse:
            # a checkpoint of more keys than the capacity: one reserve, within
            # the growth limit (a shard without growth drops what does not fit,
            # as before; keys stored beside the checkpoint's grow it on the way)
            limit, held = self.growth()["max_capacity"], int(np.unique(keys).size)
            if limit and held > self.sparse_info()["capacity"]:
                self.reserve(min(held, limit))
        self.add(keys, d["p"])
        for i, v in enumerate(d["slots"]):
            self.put_state(keys, v, slot=i)
        self.step = d["t"]

    # ------------------------------------------------------------ sparse shards
    def sparse_info(self) -> dict:
        """pskv_sparse_info_get: capacity, count (distinct keys held), table_slots
        and index_bytes of a sparse shard.  Waits for the shard's stream."""
        i = _lib.PskvSparseInfo(ctypes.sizeof(_lib.PskvSparseInfo))
        check(lib.pskv_sparse_info_get(self._h, ctypes.byref(i)))
        return {f: getattr(i, f) for f, _ in _lib.PskvSparseInfo._fields_ if f != "size"}

    def keys(self) -> np.ndarray:
        """The keys a sparse shard holds, in unspecified order (pskv_sparse_keys)."""
        n = ctypes.c_uint64()
        out = np.empty(max(self.sparse_info()["count"], 1), dtype=np.uint32)
        check(lib.pskv_sparse_keys(self._h, out.ctypes.data, out.size, ctypes.byref(n), _lib.PSKV_HOST))
        return out[:min(n.value, out.size)]

    def reserve(self, capacity: int):
        """Grow a sparse shard to hold `capacity` distinct keys (pskv_sparse_reserve):
        every stored key keeps its row and state; returns when done."""
        if not 0 <= int(capacity) < 1 << 64:
            raise ValueError(f"capacity {capacity} out of range")
        check(lib.pskv_sparse_reserve(self._h, int(capacity)))
        self.capacity = max(self.capacity, int(capacity))

    def set_growth(self, max_capacity: int):
        """Let writing calls grow the shard themselves, up to max_capacity
        distinct keys; 0 = fixed (pskv_sparse_set_growth).  A call that grows
        waits for the shard's stream."""
        if not 0 <= int(max_capacity) < 1 << 64:
            raise ValueError(f"max_capacity {max_capacity} out of range")
        check(lib.pskv_sparse_set_growth(self._h, int(max_capacity)))

    def growth(self) -> dict:
        """pskv_sparse_get_growth: max_capacity (0 = fixed) and the rebuilds done
        so far (reserve, automatic growth and erase each count one)."""
        m, r = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.pskv_sparse_get_growth(self._h, ctypes.byref(m), ctypes.byref(r)))
        return {"max_capacity": m.value, "rebuilds": r.value}

    def erase(self, keys):
        """Forget keys (pskv_sparse_erase): numpy keys or a device tensor, as get
        takes them.  A maintenance call: its cost follows the keys stored."""
        if _is_torch(keys):
            self._check_dev(keys)
            check(lib.pskv_sparse_erase(self._h, keys.data_ptr(), keys.numel(), _lib.PSKV_DEVICE))
            return
        k = self._host_keys(keys)
        check(lib.pskv_sparse_erase(self._h, k.ctypes.data, k.size, _lib.PSKV_HOST))

    def index_time(self):
        """A sparse shard's index launches, one operation per call (pskv_index_time)."""
        n, ms, el = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
        check(lib.pskv_index_time(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(el)))
        return {"launches": n.value, "total_ms": ms.value, "elements": el.value}

    def apply_time(self):
        """Optimizer steps timed as one operation each (pskv_apply_time)."""
        n, ms, el = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
        check(lib.pskv_apply_time(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(el)))
        return {"launches": n.value, "total_ms": ms.value, "elements": el.value}

    def _batch_array(self, batches, is_get):
        arr = (_lib.PskvBatch * max(1, len(batches)))()
        keep = []
        dev = None
        for i, (k, v) in enumerate(batches):
            t = _is_torch(k)
            if dev is None:
                dev = t
            if t != dev:
                raise ValueError("mixed host/device batches in one grouped call")
            if t:
                self._check_dev(k, v)
                self._check_dev_count(k, v)
                keep += [k, v]
                arr[i] = _lib.PskvBatch(k.data_ptr(), v.data_ptr(), k.numel())
            else:
                kk = self._host_keys(k)
                if is_get:
                    if not (isinstance(v, np.ndarray) and v.dtype == self.dtype and v.flags.c_contiguous):
                        raise ValueError("get_grouped host outputs must be C-contiguous arrays of the shard dtype")
                    if self.width > 1 and v.size != kk.size * self.width:
                        raise ValueError("row shard: get_grouped outputs must hold keys * width values")
                    vv = v
                else:
                    vv = self._host_vals(v, kk.size)
                keep += [kk, vv]
                arr[i] = _lib.PskvBatch(kk.ctypes.data, vv.ctypes.data, kk.size)
        return arr, keep, (_lib.PSKV_DEVICE if dev else _lib.PSKV_HOST)

    def _check_dev(self, *ts):
        for t in ts:
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous():
                raise ValueError("device tensors must be contiguous and on the shard's GPU")

    # ------------------------------------------------------------ control
    _GENERAL = {"stamps": 0, "auto": 1, "radix": 2}

    def set_option(self, name: str, value):
        """pskv_set_option: a tuning / path option of this shard (include/pskv.h).
        GENERAL also takes "stamps" / "auto" / "radix"; booleans as 0 / 1."""
        if name == "GENERAL" and isinstance(value, str):
            value = self._GENERAL[value]
        check(lib.pskv_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64()
        check(lib.pskv_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def sync(self):
        check(lib.pskv_sync(self._h))

    def clear(self):
        check(lib.pskv_clear(self._h))

    def set_stream(self, stream_handle):
        """stream_handle: int hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or None."""
        check(lib.pskv_set_stream(self._h, stream_handle))

    def dense_ptr(self) -> int:
        return int(lib.pskv_dense_ptr(self._h) or 0)

    def info(self) -> dict:
        i = _lib.PskvInfo()
        check(lib.pskv_shard_info(self._h, ctypes.byref(i)))
        d = {f: getattr(i, f) for f, _ in _lib.PskvInfo._fields_}
        d["width"] = int(lib.pskv_shard_width(self._h))
        return d

    def set_timing(self, on, kernels=None):
        """on: bool; kernels: optional list of kernel ids (_lib.PSKV_K_*) to time."""
        if kernels is None:
            check(lib.pskv_set_timing(self._h, 1 if on else 0))
        else:
            mask = 0
            for k in kernels:
                mask |= 1 << k
            check(lib.pskv_set_timing_mask(self._h, mask if on else 0))

    def reset_timing(self):
        check(lib.pskv_reset_timing(self._h))

    def kernel_time(self, kernel: int):
        n, ms, el = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
        check(lib.pskv_kernel_time(self._h, kernel, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(el)))
        return {"launches": n.value, "total_ms": ms.value, "elements": el.value}

    def dense_view(self):
        """A torch tensor aliasing the dense HBM array (tests only; no copy)."""
        import torch

        if self.is_sparse:
            raise ValueError("dense_view: a sparse shard's row order is unspecified (use keys() and get())")
        n = self.key_end - self.key_begin
        ptr = self.dense_ptr()
        if self.width > 1:
            return _tensor_from_ptr(ptr, n * self.width, _torch_dtype(self.dtype), self.device).view(n, self.width)
        return _tensor_from_ptr(ptr, n, _torch_dtype(self.dtype), self.device)


class BatchSet:
    """A packed pskv_batch array (plus references keeping its buffers alive)."""

    def __init__(self, arr, n, flags, keep):
        self.arr, self.n, self.flags, self._keep = arr, n, flags, keep


def _torch_dtype(npdt):
    import torch

    return {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32,
            np.dtype(np.float64): torch.float64}[np.dtype(npdt)]


def _tensor_from_ptr(ptr, n, tdtype, device):
    """Wrap raw device memory as a torch tensor via __cuda_array_interface__."""
    import torch

    typestr = {torch.int32: "<i4", torch.float32: "<f4", torch.float64: "<f8"}[tdtype]

    class _Holder:
        __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False),
                                    "version": 2, "strides": None}

    with torch.cuda.device(device):
        return torch.as_tensor(_Holder(), device=f"cuda:{device}")


class HostFrame:
    """A page-locked host frame from the library's pool (pskv_host_alloc): the
    buffer a mailbox receives one message payload into (comm/mailbox.cpp:246-257).
    `array(dtype, n, offset)` views it as numpy; `free()` returns it (the pool
    holds it back until queued PSKV_HOST_FRAME reads of it have run)."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        check(lib.pskv_host_alloc(int(nbytes), ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def array(self, dtype, n: int, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        if self.ptr is None or offset < 0 or offset + n * dt.itemsize > self.nbytes:
            raise ValueError("view outside the frame")
        buf = (ctypes.c_char * (n * dt.itemsize)).from_address(self.ptr + offset)
        return np.frombuffer(buf, dtype=dt, count=n)

    def free(self):
        if self.ptr is not None:
            p, self.ptr = self.ptr, None
            check(lib.pskv_host_free(p))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


def host_pool_stats() -> dict:
    v = [ctypes.c_uint64() for _ in range(3)]
    check(lib.pskv_host_pool_stats(*[ctypes.byref(x) for x in v]))
    return {"live_bytes": v[0].value, "cached_bytes": v[1].value, "held_bytes": v[2].value}


def host_pool_trim():
    check(lib.pskv_host_pool_trim())


def range_slice(ranges, keys):
    """Mirror of RangePartitionManager::Slice through the product library
    (pskv_range_slice).  Returns [(range_index, start, length), ...]."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    nr = len(ranges)
    rb = np.ascontiguousarray([b for b, _ in ranges], dtype=np.uint64)
    re = np.ascontiguousarray([e for _, e in ranges], dtype=np.uint64)
    sr = np.empty(max(nr, 1), dtype=np.int32)
    ss = np.empty(max(nr, 1), dtype=np.uint64)
    sl = np.empty(max(nr, 1), dtype=np.uint64)
    ns = check(lib.pskv_range_slice(rb.ctypes.data, re.ctypes.data, nr, k.ctypes.data, k.size,
                                    sr.ctypes.data, ss.ctypes.data, sl.ctypes.data))
    return [(int(sr[i]), int(ss[i]), int(sl[i])) for i in range(ns)]


def jump_hash(keys, num_buckets: int) -> np.ndarray:
    """Bucket of every key under the reference's default partitioner
    (ConsistentHashingPartitionManager, base/consistent_hashing_partition_manager.hpp:81-89)
    through the product library (pskv_jump_hash).  int32 array, values in
    [0, num_buckets)."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    out = np.empty(k.size, dtype=np.int32)
    check(lib.pskv_jump_hash(k.ctypes.data, k.size, int(num_buckets), out.ctypes.data))
    return out
