"""Pooled pushes against the round trip they replace: f32, device
path, a table of ROWS rows (16 Mi by default), KEYS keys per call, 4 key draws
in rotation, STEPS timed calls after WARMUP, RUNS runs per leg, the legs
alternating inside one process.  Adagrad, lr 0.05, eps 1e-8, init_accum 0.1.

  --leg pooled     one pskv_apply_pooled: the library's timer (pskv_apply_time)
                   and HIP events around the call
  --leg roundtrip  what a worker does without it: the rows expanded on the
                   device in torch (bag_grads.repeat_interleave(lens, 0), times
                   weights[:, None] when weighted), then pskv_apply of the
                   n * W rows; HIP events around both
  --leg apply      pskv_apply alone on rows expanded beforehand: the step
                   without the expansion, a floor (the library's timer)
  (default: all three, alternating)

The roundtrip and apply legs run pskv_apply, which a pooled push does not
change; run them on a build of the parent commit (PSKV_LIB_PATH) to compare
across builds.

Bag shapes: uniform lengths (--lengths, default 1,8,64) and the skewed draw of
tools/pooled_probe.py.  Weighted and unweighted.  Keys: distinct, and a draw
with 8 occurrences per key.

Prints one JSON document and writes it to --out.  The condition it evaluates:
at W = 16 and W = 64, uniform lengths 8 and 64, weighted and not, the pooled
push's median (events) is not above the round trip's by more than the larger
run-to-run spread of the two.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pooled_probe import bag_offsets  # noqa: E402


def draw_keys(torch, g, dev, rows, n, occurrences):
    """n keys of [0, rows): distinct, or n / occurrences distinct keys each `occurrences` times, shuffled."""
    distinct = torch.randperm(rows, generator=g, device=dev)[:n // occurrences]
    k = distinct.repeat(occurrences)
    return k[torch.randperm(k.numel(), generator=g, device=dev)].to(torch.int32)


def run_width(ps, torch, a, w, legs):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(9876 + w)
    shapes = [("uniform", int(x)) for x in a.lengths.split(",")] + [("skewed",)]
    res = {}
    with ps.Shard(0, a.rows, np.float32, mode="assign", width=w) as sh:
        sh.set_optimizer("adagrad", lr=0.05, eps=1e-8, init_accum=0.1)
        sh.set_timing(True)
        for occ in (1, 8):
            keys = [draw_keys(torch, g, dev, a.rows, a.keys, occ) for _ in range(4)]
            wts = [torch.randn((a.keys,), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
            for shape in shapes:
                off, nbags = bag_offsets(torch, dev, a.keys, shape, a.skew_bags, a.skew_len)
                lens = off[1:] - off[:-1]
                bgs = [torch.randn((nbags, w), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
                name = "uniform_%d" % shape[1] if shape[0] == "uniform" else "skewed_8_with_%dx%d" % (a.skew_bags, a.skew_len)
                for weighted in (False, True):
                    def expand(i):
                        rows = bgs[i % 4].repeat_interleave(lens, 0)
                        return rows * wts[i % 4][:, None] if weighted else rows

                    pre = [expand(i) for i in range(4)] if "apply" in legs else None
                    runs = {leg: [] for leg in legs}
                    lib_runs = []
                    for _ in range(a.runs):
                        for leg in legs:  # alternating
                            ev_ms = 0.0
                            for i in range(a.warmup + a.steps):
                                if i == a.warmup:
                                    sh.sync()
                                    torch.cuda.synchronize()
                                    sh.reset_timing()
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                if leg == "pooled":
                                    sh.apply_pooled(keys[i % 4], off, bgs[i % 4], wts[i % 4] if weighted else None)
                                elif leg == "roundtrip":
                                    sh.apply(keys[i % 4], expand(i))
                                else:
                                    sh.apply(keys[i % 4], pre[i % 4])
                                e1.record()
                                e1.synchronize()
                                if i >= a.warmup:
                                    ev_ms += e0.elapsed_time(e1)
                            sh.sync()
                            torch.cuda.synchronize()
                            t = sh.apply_time()
                            assert t["launches"] == a.steps and t["elements"] == a.steps * a.keys, t
                            if leg == "pooled":
                                lib_runs.append(t["total_ms"] / a.steps)
                            runs[leg].append((t["total_ms"] if leg == "apply" else ev_ms) / a.steps)
                    entry = {leg: {"ms_per_call_runs": r, "median_ms": statistics.median(r), "spread_ms": max(r) - min(r)}
                             for leg, r in runs.items()}
                    if lib_runs:
                        entry["pooled"]["library_timer_median_ms"] = statistics.median(lib_runs)
                    if "pooled" in entry and "roundtrip" in entry:
                        p, r = entry["pooled"], entry["roundtrip"]
                        entry["pooled_over_roundtrip"] = p["median_ms"] / r["median_ms"]
                        entry["not_slower_than_roundtrip"] = bool(
                            p["median_ms"] <= r["median_ms"] + max(p["spread_ms"], r["spread_ms"]))
                    if lib_runs and "apply" in entry:
                        entry["pooled_over_apply"] = entry["pooled"]["library_timer_median_ms"] / entry["apply"]["median_ms"]
                    key = "distinct" if occ == 1 else "8_per_key"
                    res.setdefault(key, {}).setdefault(name, {"bags": nbags})["weighted" if weighted else "unweighted"] = entry
                    print(f"W={w} {key} {name} weighted={weighted}: " +
                          ", ".join(f"{leg} {e['median_ms']:.4f} ms" for leg, e in entry.items() if isinstance(e, dict)),
                          flush=True)
                    del pre
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="pooled,roundtrip,apply", help="comma list of pooled | roundtrip | apply")
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--lengths", default="1,8,64")
    ap.add_argument("--skew-bags", type=int, default=4)
    ap.add_argument("--skew-len", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.leg.split(",")
    if any(leg not in ("pooled", "roundtrip", "apply") for leg in legs):
        ap.error("--leg takes pooled, roundtrip, apply")
    import torch

    import parameter_server_amd as ps

    doc = {"what": "tools/pooled_push_probe.py: pskv_apply_pooled against the device expansion + pskv_apply round trip "
                   "it replaces and against pskv_apply alone (DESIGN.md 8g)",
           "legs": legs, "dtype": "float32", "optimizer": "adagrad lr 0.05 eps 1e-8 init_accum 0.1", "rows": a.rows,
           "keys_per_call": a.keys, "steps": a.steps, "warmup": a.warmup, "runs_per_leg": a.runs,
           "device": torch.cuda.get_device_name(0), "library": os.path.relpath(ps._lib.LIB_PATH, ROOT),
           "notes": ["pooled and roundtrip medians: HIP events around the call(s); apply: the library's timer; "
                     "pooled.library_timer_median_ms: the library's timer of the pooled push",
                     "the expansion is bag_grads.repeat_interleave(lens, 0), times weights[:, None] when weighted"],
           "condition": "at W = 16 and W = 64, uniform lengths 8 and 64, weighted and not, on either key draw: the pooled "
                        "push's median is not above the round trip's by more than the larger run-to-run spread of the two",
           "widths": {}}
    for w in [int(x) for x in a.widths.split(",")]:
        doc["widths"][str(w)] = run_width(ps, torch, a, w, legs)
    if "pooled" in legs and "roundtrip" in legs:
        met = {}
        for draw in ("distinct", "8_per_key"):
            verdicts = [doc["widths"][w][draw][s][k]["not_slower_than_roundtrip"]
                        for w in ("16", "64") if w in doc["widths"]
                        for s in ("uniform_8", "uniform_64") if s in doc["widths"][w][draw]
                        for k in ("unweighted", "weighted")]
            met[draw] = bool(verdicts) and all(verdicts)
        doc["condition_met_per_key_draw"] = met
        doc["condition_met"] = all(met.values())
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
