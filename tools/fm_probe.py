"""The factorization-machine pooled calls against the round trips they replace
(DESIGN.md §8p): f32, device path, a table of ROWS rows (16 Mi by default), KEYS
distinct keys per call, 4 key draws in rotation, STEPS timed calls after WARMUP,
RUNS runs per leg, the legs alternating inside one process, HIP events around
the calls.  Adagrad (lr 0.05, eps 1e-8, init_accum 0.1) for the push.

  pull  fm         one pskv_get_pooled_fm (sum and pair)
        roundtrip  pskv_get of the n rows, then the segment arithmetic in torch
                   on the device: x = w[:, None] * rows, S and Q by index_add_
                   over the bags, pair = 0.5 * (S * S - Q).sum(1)
  push  fm         one pskv_apply_pooled_fm (bag_scale and bag_grads)
        roundtrip  pskv_get of the n rows and the segment sum S in torch, the
                   rows w (c S + bag_grads)[bag] - c[bag] w^2 p formed in torch,
                   then pskv_apply of the n * W rows

Bags of uniform length (--lengths, default 2,8,64), weighted and not.  No ratio
is promised; a case slower than its round trip is recorded as such.  Prints one
JSON document and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, sh, a, fn):
    """ms per call over the steps after the warm-up, HIP events around every call."""
    ms = 0.0
    for i in range(a.warmup + a.steps):
        if i == a.warmup:
            sh.sync()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i % 4)
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            ms += e0.elapsed_time(e1)
    sh.sync()
    torch.cuda.synchronize()
    return ms / a.steps


def run_width(ps, torch, a, w):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + w)
    res = {}
    with ps.Shard(0, a.rows, np.float32, mode="assign", width=w) as sh:
        sh.set_optimizer("adagrad", lr=0.05, eps=1e-8, init_accum=0.1)
        # small values: thousands of steps on the same rows stay finite
        sh.add(torch.arange(a.rows, device=dev, dtype=torch.int32),
               torch.randn((a.rows, w), generator=g, device=dev, dtype=torch.float32) * 0.01)
        keys = [torch.randperm(a.rows, generator=g, device=dev)[:a.keys].to(torch.int32) for _ in range(4)]
        wts = [torch.randn((a.keys,), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
        for m in [int(x) for x in a.lengths.split(",")]:
            nbags = a.keys // m
            off = torch.arange(nbags + 1, device=dev, dtype=torch.int64) * m
            bag = torch.arange(nbags, device=dev).repeat_interleave(m)
            cs = [torch.randn((nbags,), generator=g, device=dev, dtype=torch.float32) * 0.01 for _ in range(4)]
            bgs = [torch.randn((nbags, w), generator=g, device=dev, dtype=torch.float32) * 0.01 for _ in range(4)]
            for weighted in (False, True):
                def terms(i):
                    p = sh.get(keys[i]).reshape(a.keys, w)
                    return p, (p * wts[i][:, None] if weighted else p)

                def pull_roundtrip(i):
                    _, x = terms(i)
                    s = torch.zeros((nbags, w), device=dev).index_add_(0, bag, x)
                    q = torch.zeros((nbags, w), device=dev).index_add_(0, bag, x * x)
                    return s, 0.5 * (s * s - q).sum(1)

                def push_roundtrip(i):
                    p, x = terms(i)
                    t = cs[i][:, None] * torch.zeros((nbags, w), device=dev).index_add_(0, bag, x) + bgs[i]
                    wi = wts[i] if weighted else torch.ones_like(wts[i])
                    sh.apply(keys[i], wi[:, None] * t[bag] - (cs[i][bag] * wi * wi)[:, None] * p)

                legs = {
                    "pull": {"fm": lambda i: sh.get_pooled_fm(keys[i], off, wts[i] if weighted else None),
                             "roundtrip": pull_roundtrip},
                    "push": {"fm": lambda i: sh.apply_pooled_fm(keys[i], off, cs[i], wts[i] if weighted else None, bgs[i]),
                             "roundtrip": push_roundtrip},
                }
                for call, pair in legs.items():
                    runs = {leg: [] for leg in pair}
                    for _ in range(a.runs):
                        for leg, fn in pair.items():  # alternating
                            runs[leg].append(timed(torch, sh, a, fn))
                    entry = {leg: {"ms_per_call_runs": r, "median_ms": statistics.median(r), "spread_ms": max(r) - min(r)}
                             for leg, r in runs.items()}
                    entry["fm_over_roundtrip"] = entry["fm"]["median_ms"] / entry["roundtrip"]["median_ms"]
                    res.setdefault(call, {}).setdefault("bags_of_%d" % m, {})["weighted" if weighted else "unweighted"] = entry
                    print(f"W={w} {call} bags of {m} weighted={weighted}: fm {entry['fm']['median_ms']:.4f} ms, roundtrip "
                          f"{entry['roundtrip']['median_ms']:.4f} ms, ratio {entry['fm_over_roundtrip']:.3f}", flush=True)
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--lengths", default="2,8,64")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import parameter_server_amd as ps

    doc = {"what": "tools/fm_probe.py: pskv_get_pooled_fm and pskv_apply_pooled_fm against the pskv_get + torch segment "
                   "arithmetic (+ pskv_apply) round trips they replace (DESIGN.md 8p)",
           "dtype": "float32", "optimizer": "adagrad lr 0.05 eps 1e-8 init_accum 0.1", "rows": a.rows,
           "keys_per_call": a.keys, "key_draw": "distinct", "steps": a.steps, "warmup": a.warmup, "runs_per_leg": a.runs,
           "device": torch.cuda.get_device_name(0), "library": os.path.relpath(ps._lib.LIB_PATH, ROOT),
           "notes": ["medians of HIP events around the call(s); 4 key draws in rotation, legs alternating",
                     "fm_over_roundtrip below 1: the in-shard call is faster"],
           "widths": {}}
    for w in [int(x) for x in a.widths.split(",")]:
        doc["widths"][str(w)] = run_width(ps, torch, a, w)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
