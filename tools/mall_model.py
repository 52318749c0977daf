#!/usr/bin/env python3
"""A model of the Infinity Cache under the headline step's parameter traffic.

Not a measurement: an LRU of `cache` bytes over the parameter accesses of
bench.py's cfg-2 step (64 x 1M-key windows pushed, the free window slots
pulled, 16 window sets rotated), at window granularity (one 1M-key f32 window
= 4 MB = one cache entry).  The streamed keys, values and outputs are
non-temporal and are taken not to allocate, so they do not appear.  It answers
one question: what share of the step's parameter bytes does HBM serve under a
cache policy?

  today      K1's plain loads allocate, K2g's non-temporal stores do not
             (option NTP = 1, RESIDENT_BYTES = 0)
  resident   offsets [0, resident) of the dense array take plain loads and plain
             stores (both allocate; a dirty entry costs its write-back when it
             is evicted), every other parameter access is non-temporal and is
             served by HBM (option RESIDENT_BYTES)

A load that hits and a store that is absorbed cost HBM nothing; a load that
misses, a non-temporal access and the write-back of an evicted dirty entry cost
the entry's bytes.  DESIGN.md §7 ("Resident window") sets the model's figures
beside the measured ones.

Pure Python: parameter_server_amd/workload.py is loaded by path, so this runs
without the HIP library.

  python3 tools/mall_model.py
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 1_000_000
MIB = 1 << 20


def load_workload():
    spec = importlib.util.spec_from_file_location(
        "pskv_workload", os.path.join(ROOT, "parameter_server_amd", "workload.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def window_sets(sets=16, batches=64, batch=MB, key_space=100 * MB):
    """bench.py's cfg-2 plan (plan_rank / plan_pull at N = 1): per set, the
    pushed and the pulled window slots."""
    w = load_workload()
    out = []
    for r in range(sets):
        seed = w.set_seed(r, 1)
        push = w.dense_bases(batches, key_space, batch, seed=seed)
        pull = w.complement_windows(push, 0, key_space, batch, seed=seed + 7)
        out.append((sorted({int(b) // batch for b in push}), [int(b) // batch for b in pull]))
    return out


def hbm_share(resident=0, cache=256 * MIB, rotations=4, value_bytes=4, batch=MB, **plan):
    """Share of the parameter bytes of the last rotation's steps that HBM
    serves.  resident: bytes of the dense array from its start (0: today's
    policy); a window slot is resident when it lies wholly inside."""
    entry = batch * value_bytes
    cap = cache // entry
    res_slots = resident // entry
    sets = window_sets(batch=batch, **plan)
    lru = OrderedDict()  # slot -> dirty
    total = hbm = 0

    def touch(slot, dirty):
        nonlocal hbm
        was = lru.pop(slot, None)
        hit = was is not None
        lru[slot] = dirty or bool(was)
        if len(lru) > cap:
            _, was_dirty = lru.popitem(last=False)
            hbm += entry * bool(was_dirty)
        return hit

    for rot in range(rotations):
        if rot == rotations - 1:
            total = hbm = 0
        for push, pull in sets:
            for s in push:  # K2g
                total += entry
                if resident and s < res_slots:
                    touch(s, True)      # plain store: absorbed
                else:
                    hbm += entry        # non-temporal store
            for s in pull:  # K1
                total += entry
                if resident and s >= res_slots:
                    hbm += entry        # non-temporal load
                elif not touch(s, False):
                    hbm += entry        # plain load, a miss
    return hbm / total


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--cache-mib", type=int, default=256)
    p.add_argument("--resident-mb", type=int, nargs="*", default=[192, 224, 256])
    args = p.parse_args()
    cache = args.cache_mib * MIB
    rows = {"today": hbm_share(0, cache)}
    for r in args.resident_mb:
        rows[f"resident {r} MB"] = hbm_share(r * MB, cache)
    rows["resident 256 MB in a 224 MiB cache"] = hbm_share(256 * MB, 224 * MIB)
    print(json.dumps({k: round(v, 3) for k, v in rows.items()}, indent=1))


if __name__ == "__main__":
    main()
