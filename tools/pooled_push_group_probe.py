"""Grouped pooled pushes against the round trips they replace:
f32, device path, a table of ROWS rows (16 Mi by default), Adagrad (lr 0.05,
eps 1e-8, init_accum 0.1), BATCHES batches (8) of KEYS keys each (128 Ki: 1 Mi
keys per call), uniform bags of 8 and 64, weighted and not, distinct keys over
the whole call and 8 occurrences per key, 4 draws in rotation, STEPS timed
calls after WARMUP, RUNS runs per leg, the legs alternating inside one process.
HIP events around everything a leg does per call.

  --leg grouped    one pskv_apply_pooled_grouped of the BATCHES batches
  --leg concat     the exact workaround it replaces, on the same build: torch.cat
                   of the batches' keys, weights and bag rows, the offsets shifted
                   by the keys before each batch and concatenated on the device,
                   then one pskv_apply_pooled
  --leg expanded   every batch's rows expanded on the device
                   (bag_grads.repeat_interleave(lens, 0), times weights[:, None]
                   when weighted), then one pskv_apply_grouped of the n * W rows
  (default: all three, alternating)

One process per width (--widths 16, then --widths 64, each under its own time
limit), then --merge A.json B.json --out C.json puts the documents together and
evaluates the condition: in every case, grouped's median is not above concat's
by more than the larger run-to-run spread of the two.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("grouped", "concat", "expanded")
CONDITION = ("in every case (W, key draw, bag length, weighted or not): the grouped call's median is not above the "
             "concat round trip's by more than the larger run-to-run spread of the two")


def draw_keys(torch, g, dev, rows, n, occurrences):
    """n keys of [0, rows): distinct, or n / occurrences distinct keys each `occurrences` times, shuffled."""
    distinct = torch.randperm(rows, generator=g, device=dev)[:n // occurrences]
    k = distinct.repeat(occurrences)
    return k[torch.randperm(k.numel(), generator=g, device=dev)].to(torch.int32)


def run_width(ps, torch, a, w, legs):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + w)
    nb, n = a.batches, a.keys
    res = {}
    with ps.Shard(0, a.rows, np.float32, mode="assign", width=w) as sh:
        sh.set_optimizer("adagrad", lr=0.05, eps=1e-8, init_accum=0.1)
        sh.set_timing(True)
        for occ in (1, 8):
            # the key draw spans the whole call: a key's occurrences fall into any of the batches
            keys = [draw_keys(torch, g, dev, a.rows, nb * n, occ).view(nb, n) for _ in range(4)]
            wts = [torch.randn((nb, n), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
            for length in [int(x) for x in a.lengths.split(",")]:
                off = torch.arange(0, n + 1, length, device=dev, dtype=torch.int64)
                assert int(off[-1]) == n, "the bag length must divide the batch"
                nbags = off.numel() - 1
                lens = off[1:] - off[:-1]
                shifts = [off[1:] + j * n for j in range(nb)]
                bgs = [torch.randn((nb, nbags, w), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
                for weighted in (False, True):
                    def batch(i, j):
                        return keys[i % 4][j], off, bgs[i % 4][j], wts[i % 4][j] if weighted else None

                    def call(leg, i):
                        if leg == "grouped":
                            sh.apply_pooled_grouped([batch(i, j) for j in range(nb)])
                        elif leg == "concat":
                            k = torch.cat([keys[i % 4][j] for j in range(nb)])
                            b = torch.cat([bgs[i % 4][j] for j in range(nb)])
                            ws = torch.cat([wts[i % 4][j] for j in range(nb)]) if weighted else None
                            o = torch.cat([off[:1]] + shifts)
                            sh.apply_pooled(k, o, b, ws)
                        else:
                            rows = []
                            for j in range(nb):
                                r = bgs[i % 4][j].repeat_interleave(lens, 0)
                                rows.append(r * wts[i % 4][j][:, None] if weighted else r)
                            sh.apply_grouped([(keys[i % 4][j], rows[j]) for j in range(nb)])

                    runs = {leg: [] for leg in legs}
                    lib = {leg: [] for leg in legs}
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
                                call(leg, i)
                                e1.record()
                                e1.synchronize()
                                if i >= a.warmup:
                                    ev_ms += e0.elapsed_time(e1)
                            sh.sync()
                            torch.cuda.synchronize()
                            t = sh.apply_time()
                            assert t["launches"] == a.steps and t["elements"] == a.steps * nb * n, t
                            runs[leg].append(ev_ms / a.steps)
                            lib[leg].append(t["total_ms"] / a.steps)
                    entry = {leg: {"ms_per_call_runs": r, "median_ms": statistics.median(r), "spread_ms": max(r) - min(r),
                                   "library_timer_median_ms": statistics.median(lib[leg])}
                             for leg, r in runs.items()}
                    if "grouped" in entry and "concat" in entry:
                        p, r = entry["grouped"], entry["concat"]
                        entry["grouped_over_concat"] = p["median_ms"] / r["median_ms"]
                        entry["not_slower_than_concat"] = bool(
                            p["median_ms"] <= r["median_ms"] + max(p["spread_ms"], r["spread_ms"]))
                    if "grouped" in entry and "expanded" in entry:
                        entry["grouped_over_expanded"] = entry["grouped"]["median_ms"] / entry["expanded"]["median_ms"]
                    key = "distinct" if occ == 1 else "8_per_key"
                    res.setdefault(key, {}).setdefault("uniform_%d" % length, {"bags_per_batch": nbags})[
                        "weighted" if weighted else "unweighted"] = entry
                    print(f"W={w} {key} bags of {length} weighted={weighted}: " +
                          ", ".join(f"{leg} {e['median_ms']:.4f} ms (library {e['library_timer_median_ms']:.4f})"
                                    for leg, e in entry.items() if isinstance(e, dict)), flush=True)
    torch.cuda.synchronize()
    return res


def verdict(doc):
    cases = [e for w in doc["widths"].values() for draw in w.values() for shape in draw.values()
             for e in shape.values() if isinstance(e, dict) and "not_slower_than_concat" in e]
    if cases:
        doc["cases"] = len(cases)
        doc["cases_not_slower_than_concat"] = sum(e["not_slower_than_concat"] for e in cases)
        doc["condition_met"] = all(e["not_slower_than_concat"] for e in cases)
    return doc


def write(doc, out):
    txt = json.dumps(doc, indent=1)
    print(txt)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=",".join(LEGS), help="comma list of " + " | ".join(LEGS))
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--keys", type=int, default=1 << 17, help="keys per batch")
    ap.add_argument("--widths", default="16,64")
    ap.add_argument("--lengths", default="8,64")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None, help="documents of single widths to put together (no GPU)")
    a = ap.parse_args()
    if a.merge:
        docs = [json.load(open(p)) for p in a.merge]
        doc = docs[0]
        for d in docs[1:]:
            doc["widths"].update(d["widths"])
        write(verdict(doc), a.out)
        return
    legs = a.leg.split(",")
    if any(leg not in LEGS for leg in legs):
        ap.error("--leg takes " + ", ".join(LEGS))
    import torch

    import parameter_server_amd as ps

    doc = {"what": "tools/pooled_push_group_probe.py: pskv_apply_pooled_grouped against the device concatenation + "
                   "pskv_apply_pooled round trip it replaces and against the device expansion + pskv_apply_grouped "
                   "(DESIGN.md 8h)",
           "legs": legs, "dtype": "float32", "optimizer": "adagrad lr 0.05 eps 1e-8 init_accum 0.1", "rows": a.rows,
           "batches_per_call": a.batches, "keys_per_batch": a.keys, "steps": a.steps, "warmup": a.warmup,
           "runs_per_leg": a.runs, "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(ps._lib.LIB_PATH, ROOT),
           "notes": ["medians: HIP events around everything the leg does per call (concat: the torch.cat calls and the "
                     "pooled push; expanded: the expansions and the grouped apply); library_timer_median_ms: the "
                     "library's timer of the step alone (pskv_apply_time)",
                     "a key draw spans the whole call: a key's occurrences fall into any of its batches"],
           "condition": CONDITION, "widths": {}}
    for w in [int(x) for x in a.widths.split(",")]:
        doc["widths"][str(w)] = run_width(ps, torch, a, w, legs)
    write(verdict(doc), a.out)


if __name__ == "__main__":
    main()
