"""Pooled pulls against the round trip they replace: f32, device
path, a table of ROWS rows (16 Mi by default: the dense array exceeds the
256 MiB Infinity Cache from W = 16 on and equals it at W = 4), KEYS uniformly
random keys per call, 4 distinct key draws in rotation, STEPS timed calls after
WARMUP, RUNS runs per leg, the legs alternating inside one process.

  --leg pooled     pskv_get_pooled, the library's own timer (pskv_pooled_time)
  --leg get        pskv_get of the same keys, k_row_gather's timer: the bytes a
                   pooled pull reads, written out in full
  --leg roundtrip  that Get plus a torch segment sum on the device (the weights
                   multiplied in first), HIP events around both: what a worker
                   does today, and what the pooled pull replaces
  (default: all three, alternating)

Bag shapes: uniform lengths (--lengths, default 1,8,64) and one skewed draw of
the same KEYS keys, bags of 8 with --skew-bags bags of --skew-len keys among
them.  Weighted and unweighted.  One host-path figure (--host) against a host
Get of the same keys, wall clock.

Prints one JSON document and writes it to --out.  The condition it evaluates:
at W = 16 and W = 64, uniform lengths 8 and 64, the pooled pull's median is not
above the round trip's by more than the larger run-to-run spread of the two.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bag_offsets(torch, dev, nkeys, shape, skew_bags, skew_len):
    """int64 device offsets of the shape: ("uniform", L) or ("skewed",)."""
    if shape[0] == "uniform":
        length = shape[1]
        off = np.arange(0, nkeys + 1, length, dtype=np.int64)
        if off[-1] != nkeys:
            off = np.append(off, nkeys)
    else:
        rest = nkeys - skew_bags * skew_len
        lens = np.full(rest // 8, 8, dtype=np.int64)
        if rest % 8:
            lens = np.append(lens, rest % 8)
        at = np.linspace(0, lens.size, skew_bags + 2, dtype=np.int64)[1:-1]  # spread among the short bags
        lens = np.insert(lens, at, skew_len)
        off = np.concatenate([[0], np.cumsum(lens)])
    assert off[-1] == nkeys
    return torch.from_numpy(off).to(dev), int(off.size - 1)


def segment_sum(torch, rows, wts, off, lengths):
    if wts is not None:
        rows = rows * wts[:, None]
    return torch.segment_reduce(rows, "sum", lengths=lengths, axis=0, unsafe=True)


def run_width(ps, torch, a, w, legs, doc):
    from parameter_server_amd import _lib

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + w)
    keys = [torch.randint(0, a.rows, (a.keys,), generator=g, device=dev, dtype=torch.int64).to(torch.int32)
            for _ in range(4)]
    wts = [torch.randn((a.keys,), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
    rows_out = torch.empty((a.keys, w), dtype=torch.float32, device=dev)
    shapes = [("uniform", int(x)) for x in a.lengths.split(",")] + [("skewed",)]
    res = {}
    with ps.Shard(0, a.rows, np.float32, mode="assign", width=w) as sh:
        for i in range(4):  # pull rows that were written
            sh.add(keys[i], torch.randn((a.keys, w), generator=g, device=dev, dtype=torch.float32))
        sh.set_timing(True)
        for shape in shapes:
            off, nbags = bag_offsets(torch, dev, a.keys, shape, a.skew_bags, a.skew_len)
            lengths = off[1:] - off[:-1]
            pooled_out = torch.empty((nbags, w), dtype=torch.float32, device=dev)
            name = "uniform_%d" % shape[1] if shape[0] == "uniform" else "skewed_8_with_%dx%d" % (a.skew_bags, a.skew_len)
            for weighted in (False, True):
                runs = {leg: [] for leg in legs}
                for _ in range(a.runs):
                    for leg in legs:  # alternating
                        ev_ms = 0.0
                        for i in range(a.warmup + a.steps):
                            if i == a.warmup:
                                sh.sync()
                                torch.cuda.synchronize()
                                sh.reset_timing()
                            k, wt = keys[i % 4], (wts[i % 4] if weighted else None)
                            if leg == "pooled":
                                sh.get_pooled(k, off, wt, out=pooled_out)
                            elif leg == "get":
                                sh.get(k, out=rows_out)
                            else:
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                sh.get(k, out=rows_out)
                                segment_sum(torch, rows_out, wt, off, lengths)
                                e1.record()
                                e1.synchronize()
                                if i >= a.warmup:
                                    ev_ms += e0.elapsed_time(e1)
                        sh.sync()
                        torch.cuda.synchronize()
                        if leg == "pooled":
                            t = sh.pooled_time()
                            assert t["launches"] == a.steps, t
                            ms = t["total_ms"]
                        elif leg == "get":
                            t = sh.kernel_time(_lib.PSKV_K_ROW_GATHER)
                            assert t["launches"] == a.steps, t
                            ms = t["total_ms"]
                        else:
                            ms = ev_ms
                        runs[leg].append(ms / a.steps)
                entry = {}
                for leg, r in runs.items():
                    entry[leg] = {"ms_per_call_runs": r, "median_ms": statistics.median(r), "spread_ms": max(r) - min(r),
                                  "row_payload_TBps": a.keys * w * 4 / (statistics.median(r) / 1e3) / 1e12}
                if "pooled" in entry and "roundtrip" in entry:
                    p, r = entry["pooled"], entry["roundtrip"]
                    entry["pooled_over_roundtrip"] = p["median_ms"] / r["median_ms"]
                    entry["not_slower_than_roundtrip"] = bool(
                        p["median_ms"] <= r["median_ms"] + max(p["spread_ms"], r["spread_ms"]))
                if "pooled" in entry and "get" in entry:
                    entry["pooled_over_get"] = entry["pooled"]["median_ms"] / entry["get"]["median_ms"]
                res.setdefault(name, {"bags": nbags})["weighted" if weighted else "unweighted"] = entry
                print(f"W={w} {name} weighted={weighted}: " +
                      ", ".join(f"{leg} {e['median_ms']:.4f} ms" for leg, e in entry.items() if isinstance(e, dict)),
                      flush=True)
        if a.host and w == a.host_width:
            hk = keys[0].cpu().numpy().view(np.uint32)
            hoff = np.arange(0, a.keys + 1, 8, dtype=np.uint64)
            best = {}
            for leg in ("pooled", "get"):
                ts = []
                for _ in range(4):
                    t0 = time.perf_counter()
                    sh.get_pooled(hk, hoff) if leg == "pooled" else sh.get(hk)
                    ts.append((time.perf_counter() - t0) * 1e3)
                best[leg + "_ms_calls"] = ts
                best[leg + "_ms_min_after_first"] = min(ts[1:])
            doc["host_path"] = {"width": w, "keys": a.keys, "bag_length": 8, "wall_clock": best}
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="pooled,get,roundtrip", help="comma list of pooled | get | roundtrip")
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--lengths", default="1,8,64")
    ap.add_argument("--skew-bags", type=int, default=4)
    ap.add_argument("--skew-len", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also one host-path figure at --host-width")
    ap.add_argument("--host-width", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.leg.split(",")
    if any(leg not in ("pooled", "get", "roundtrip") for leg in legs):
        ap.error("--leg takes pooled, get, roundtrip")
    import torch

    import parameter_server_amd as ps

    doc = {"what": "tools/pooled_probe.py: pskv_get_pooled against pskv_get and against the Get + device segment-sum "
                   "round trip it replaces (DESIGN.md 8f)",
           "legs": legs, "dtype": "float32", "rows": a.rows, "keys_per_call": a.keys, "steps": a.steps,
           "warmup": a.warmup, "runs_per_leg": a.runs, "device": torch.cuda.get_device_name(0),
           "notes": ["pooled and get: the library's timers (kernels only); roundtrip: HIP events around the Get and the "
                     "torch segment sum (torch.segment_reduce; weighted: an elementwise multiply first)",
                     "at W = 4 the dense array (rows * 16 B) equals the 256 MiB Infinity Cache, it does not exceed it",
                     "row_payload_TBps counts keys * W * 4 bytes of rows read per call"],
           "condition": "at W = 16 and W = 64, uniform lengths 8 and 64: the pooled pull's median is not above the round "
                        "trip's by more than the larger run-to-run spread of the two",
           "widths": {}}
    for w in [int(x) for x in a.widths.split(",")]:
        doc["widths"][str(w)] = run_width(ps, torch, a, w, legs, doc)
    if "pooled" in legs and "roundtrip" in legs:
        verdicts = [doc["widths"][w][s][k]["not_slower_than_roundtrip"]
                    for w in ("16", "64") if w in doc["widths"]
                    for s in ("uniform_8", "uniform_64") if s in doc["widths"][w]
                    for k in ("unweighted", "weighted")]
        doc["condition_met"] = bool(verdicts) and all(verdicts)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
