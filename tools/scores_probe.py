"""The score pull against the round trip it replaces: f32,
device path, a row shard of KEYS rows (1 Mi by default) and KEYS distinct keys
per call (a permutation: the shard holds exactly them), 4 key draws in
rotation, STEPS timed calls after WARMUP, RUNS runs per leg, the legs
alternating inside one process, HIP events around the calls.

  scores     one pskv_get_scores
  roundtrip  pskv_get of the n rows into a device buffer, then
             (rows * q[bag]).sum(-1) in torch on the device
  get        the pskv_get alone

Bags of uniform length (--lengths, default 1,8,64; 0: one bag of all keys).
No ratio is promised; a case slower than its round trip is recorded as such.
algorithmic_bytes: keys, rows, the query rows as staged (one per bag and
window it reaches) and scores; divide by the kernel's time from a separate
kernel trace.  Prints one JSON document and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 1024  # kScoreWindow (pskv_plan.h)


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
    g.manual_seed(9876 + w)
    res = {}
    with ps.Shard(0, a.keys, np.float32, mode="assign", width=w) as sh:
        sh.add(torch.arange(a.keys, device=dev, dtype=torch.int32),
               torch.randn((a.keys, w), generator=g, device=dev, dtype=torch.float32))
        keys = [torch.randperm(a.keys, generator=g, device=dev).to(torch.int32) for _ in range(4)]
        out = torch.empty(a.keys, device=dev, dtype=torch.float32)
        for m in [int(x) for x in a.lengths.split(",")]:
            m = m or a.keys
            nbags = a.keys // m
            off = torch.arange(nbags + 1, device=dev, dtype=torch.int64) * m
            bag = torch.arange(nbags, device=dev).repeat_interleave(m)
            q = torch.randn((nbags, w), generator=g, device=dev, dtype=torch.float32)
            legs = {"scores": lambda i: sh.get_scores(keys[i], off, q, out),
                    "roundtrip": lambda i: (sh.get(keys[i]).reshape(a.keys, w) * q[bag]).sum(-1),
                    "get": lambda i: sh.get(keys[i])}
            if a.only:
                legs = {a.only: legs[a.only]}
            runs = {leg: [] for leg in legs}
            for _ in range(a.runs):
                for leg, fn in legs.items():  # alternating
                    runs[leg].append(timed(torch, sh, a, fn))
            entry = {leg: {"ms_per_call_runs": r, "median_ms": statistics.median(r), "spread_ms": max(r) - min(r)}
                     for leg, r in runs.items()}
            if not a.only:
                rt = entry["roundtrip"]
                entry["scores_over_roundtrip"] = entry["scores"]["median_ms"] / rt["median_ms"]
                entry["roundtrip_spread_over_median"] = rt["spread_ms"] / rt["median_ms"]
                entry["scores_over_get"] = entry["scores"]["median_ms"] / entry["get"]["median_ms"]
            staged = nbags + (a.keys + WINDOW - 1) // WINDOW - 1 if m < a.keys else (a.keys + WINDOW - 1) // WINDOW
            entry["algorithmic_bytes"] = a.keys * 4 + a.keys * w * 4 + staged * w * 4 + a.keys * 4
            res["one_bag" if m == a.keys else "bags_of_%d" % m] = entry
            print(f"W={w} bags of {m}: " + ", ".join(f"{leg} {e['median_ms']:.4f} ms" for leg, e in entry.items()
                                                      if isinstance(e, dict)), flush=True)
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--lengths", default="1,8,64,0")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default=None, help="time one leg alone (a kernel trace of `scores`)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import parameter_server_amd as ps

    doc = {"what": "tools/scores_probe.py: pskv_get_scores against the pskv_get + torch round trip it replaces and "
                   "against pskv_get alone (DESIGN.md 8r)",
           "dtype": "float32", "rows": a.keys, "keys_per_call": a.keys, "key_draw": "a permutation of the shard's keys",
           "steps": a.steps, "warmup": a.warmup, "runs_per_leg": a.runs, "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(ps._lib.LIB_PATH, ROOT),
           "notes": ["medians of HIP events around the call(s); 4 key draws in rotation, legs alternating",
                     "scores_over_roundtrip below 1 by more than roundtrip_spread_over_median: the in-shard call is faster"],
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
