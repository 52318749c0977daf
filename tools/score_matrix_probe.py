"""The score matrix pull against the round trips it replaces:
f32, device path, a row shard of ROWS rows (1 Mi by default), n distinct keys
per call (the head of a permutation), 4 key draws in rotation, STEPS timed
calls after WARMUP, RUNS runs per leg, the legs alternating inside one
process, HIP events around the calls.

  matrix     one pskv_get_score_matrix into an (nq, n) device matrix
  roundtrip  pskv_get of the n rows into a device buffer, then
             torch.matmul(q, rows.T) on the device: the yardstick, on code
             this call does not touch
  repeated   pskv_get_scores with the keys repeated nq times, one bag per
             query (only while n * nq <= --repeat-limit positions)

Cases whose out passes --max-out-bytes are skipped.  No ratio is promised; a
case slower than its round trip is recorded as such.  algorithmic_bytes: keys,
rows once, queries once and scores; flops: 2 n nq W; divide by the kernel's
time from a separate kernel trace.  Prints one JSON document and writes it to
--out.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.scores_probe import timed  # noqa: E402


def run_width(ps, torch, a, w):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + w)
    res = {}
    with ps.Shard(0, a.rows, np.float32, mode="assign", width=w) as sh:
        sh.add(torch.arange(a.rows, device=dev, dtype=torch.int32),
               torch.randn((a.rows, w), generator=g, device=dev, dtype=torch.float32))
        perms = [torch.randperm(a.rows, generator=g, device=dev).to(torch.int32) for _ in range(4)]
        for n in [int(x) for x in a.keys.split(",")]:
            keys = [p[:n].contiguous() for p in perms]
            for nq in [int(x) for x in a.queries.split(",")]:
                name = f"n={n},nq={nq}"
                if n * nq * 4 > a.max_out_bytes:
                    res[name] = {"skipped": "out passes --max-out-bytes"}
                    continue
                q = torch.randn((nq, w), generator=g, device=dev, dtype=torch.float32)
                out = torch.empty((nq, n), device=dev, dtype=torch.float32)
                legs = {"matrix": lambda i: sh.get_score_matrix(keys[i], q, out),
                        "roundtrip": lambda i: torch.matmul(q, sh.get(keys[i]).reshape(n, w).T, out=out)}
                if n * nq <= a.repeat_limit:
                    rep = [k.repeat(nq) for k in keys]
                    off = torch.arange(nq + 1, device=dev, dtype=torch.int64) * n
                    flat = out.view(-1)
                    legs["repeated"] = lambda i: sh.get_scores(rep[i], off, q, flat)
                if a.only:
                    legs = {a.only: legs[a.only]}
                runs = {leg: [] for leg in legs}
                for _ in range(a.runs):
                    for leg, fn in legs.items():  # alternating
                        runs[leg].append(timed(torch, sh, a, fn))
                entry = {leg: {"ms_per_call_runs": r, "median_ms": statistics.median(r), "spread_ms": max(r) - min(r)}
                         for leg, r in runs.items()}
                if not a.only:
                    rt, m = entry["roundtrip"], entry["matrix"]["median_ms"]
                    entry["matrix_over_roundtrip"] = m / rt["median_ms"]
                    entry["roundtrip_spread_over_median"] = rt["spread_ms"] / rt["median_ms"]
                    entry["clears_the_spread"] = abs(1 - entry["matrix_over_roundtrip"]) > \
                        entry["roundtrip_spread_over_median"]
                    if "repeated" in entry:
                        entry["matrix_over_repeated"] = m / entry["repeated"]["median_ms"]
                entry["algorithmic_bytes"] = n * 4 + n * w * 4 + nq * w * 4 + n * nq * 4
                entry["flops"] = 2 * n * nq * w
                res[name] = entry
                print(f"W={w} {name}: " + ", ".join(f"{leg} {e['median_ms']:.4f} ms" for leg, e in entry.items()
                                                     if isinstance(e, dict)), flush=True)
                del out, q
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--widths", default="16,64,256")
    ap.add_argument("--keys", default="1024,16384,262144")
    ap.add_argument("--queries", default="16,256,4096")
    ap.add_argument("--max-out-bytes", type=int, default=2 << 30)
    ap.add_argument("--repeat-limit", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default=None, help="time one leg alone (a kernel trace of `matrix`)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import parameter_server_amd as ps

    doc = {"what": "tools/score_matrix_probe.py: pskv_get_score_matrix against the pskv_get + torch.matmul round trip "
                   "it replaces and against pskv_get_scores with repeated keys (DESIGN.md 8s)",
           "dtype": "float32", "rows": a.rows, "key_draw": "the first n of a permutation of the shard's keys",
           "steps": a.steps, "warmup": a.warmup, "runs_per_leg": a.runs, "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(ps._lib.LIB_PATH, ROOT),
           "notes": ["medians of HIP events around the call(s); 4 key draws in rotation, legs alternating",
                     "matrix_over_roundtrip below 1 by more than roundtrip_spread_over_median: the in-shard call is faster"],
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
