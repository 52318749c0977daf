"""A server-side Adagrad step against the round trip it replaces (DESIGN.md
§8c): f32, device path, a table of ROWS rows of width W, KEYS uniformly random
DISTINCT keys per call, 4 key draws in rotation, STEPS timed calls after
WARMUP.  Every call is timed twice: by the library's own timers and by HIP
events around the whole step (on the legacy default stream, which the shard's
blocking stream orders against).

  --leg apply      one pskv_apply per call; --kind adagrad (default), momentum,
                   adam or ftrl selects the rule (momentum 0.9,
                   Adam's betas 0.9 / 0.999; §8i: FTRL-Proximal with l1 0.5,
                   l2 0.01, ftrl_beta 1)
                   --dups D: a call of the same size with D occurrences per
                   key (KEYS / D distinct keys, shuffled): prices the loser atomics
  --leg roundtrip  what a worker must do without optimizer steps for the same
                   update: get the rows, the Adagrad arithmetic in torch on the
                   device (h in a torch tensor indexed by the keys), add
                   (assign) the new rows.  It uses only Get and Add, so with
                   --tree it runs on a checkout and build from before
                   pskv_apply existed (the baseline).
  --tree PATH      import parameter_server_amd from this checkout (built)
                   instead of the one the script lies in

Prints one JSON document and writes it to --out.

  --merge OUT.json RUN.json ...
                   no GPU: collect run documents; per leg and width the median
                   and the spread (max - min) over its runs, and the condition:
                   at W = 16 and W = 64 the apply step (events, median) takes no
                   longer than the round trip; a difference inside the larger of
                   the two spreads counts as equal.  profiles/apply_probe.json
                   is the output of this mode.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD, EPS, INIT_ACCUM = 0.05, 0.0, 1e-8, 0.1
MOMENTUM, BETA1, BETA2 = 0.9, 0.9, 0.999
L1, L2, FTRL_BETA = 0.5, 0.01, 1.0


def run_width(ps, torch, leg, w, rows, nkeys, steps, warmup, dups, kind="adagrad"):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + w)
    draws = []
    for _ in range(4):
        d = torch.randperm(rows, generator=g, device=dev)[:nkeys // dups]
        if dups > 1:
            d = d.repeat(dups)[torch.randperm(d.numel() * dups, generator=g, device=dev)]
        draws.append(d)
    keys = [d.to(torch.int32) for d in draws]
    grads = [torch.randn((keys[0].numel(), w), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    with ps.Shard(0, rows, np.float32, width=w) as sh:
        for i in range(4):  # the rows start written
            sh.add(keys[i], grads[(i + 1) % 4])
        if leg == "apply" and kind == "adagrad":
            sh.set_optimizer("adagrad", lr=LR, weight_decay=WD, eps=EPS, init_accum=INIT_ACCUM)
        elif leg == "apply" and kind == "momentum":
            sh.set_optimizer("momentum", lr=LR, weight_decay=WD, momentum=MOMENTUM)
        elif leg == "apply" and kind == "ftrl":
            sh.set_optimizer("ftrl", lr=LR, weight_decay=WD, l1=L1, l2=L2, ftrl_beta=FTRL_BETA, init_accum=INIT_ACCUM)
        elif leg == "apply":
            sh.set_optimizer("adam", lr=LR, weight_decay=WD, eps=EPS, beta1=BETA1, beta2=BETA2)
        else:
            h = torch.full((rows, w), INIT_ACCUM, dtype=torch.float32, device=dev)
            p = torch.empty((keys[0].numel(), w), dtype=torch.float32, device=dev)
        nk = 0
        while True:  # every kernel id this build knows
            try:
                sh.kernel_time(nk)
            except ps.PskvError:
                break
            nk += 1
        sh.set_timing(True)
        for i in range(warmup + steps):
            if i == warmup:
                sh.sync()
                torch.cuda.synchronize()
                sh.reset_timing()
            k, gr = keys[i % 4], grads[i % 4]
            if i >= warmup:
                ev[i - warmup][0].record()
            if leg == "apply":
                sh.apply(k, gr)
            else:
                sh.get(k, out=p)
                k64 = draws[i % 4]
                d = gr + WD * p if WD else gr
                hk = h[k64] + d * d
                h[k64] = hk
                sh.add(k, p - LR * d / (hk.sqrt() + EPS))
            if i >= warmup:
                ev[i - warmup][1].record()
        sh.sync()
        torch.cuda.synchronize()
        event_ms = [a.elapsed_time(b) for a, b in ev]
        if leg == "apply":
            t = sh.apply_time()
            lib_ms, launches = t["total_ms"], t["launches"]
        else:
            ts = [sh.kernel_time(k) for k in range(nk)]
            lib_ms, launches = sum(t["total_ms"] for t in ts), sum(t["launches"] for t in ts)
    payload = keys[0].numel() * w * 4
    per = statistics.median(event_ms)
    return {
        "event_ms_median": per,
        "event_ms_min": min(event_ms),
        "event_ms_max": max(event_ms),
        "library_timer_ms_per_call": lib_ms / steps,
        "timed_operations_per_call": launches / steps,
        # apply: keys + g in, p and h in and out; the gradient scratch is only read when a key repeats
        "gradient_payload_GBps": payload / (per / 1e3) / 1e9,
    }


def merge(paths):
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append(json.load(f))
    doc = {"what": "tools/apply_probe.py --merge: one server-side Adagrad step (pskv_apply) against the Get + torch "
                   "arithmetic + assign Add round trip it replaces (DESIGN.md 8c)",
           "setup": {k: runs[0][k] for k in ("dtype", "rows", "keys_per_call", "steps", "warmup", "device")},
           "hyper_parameters": {"lr": LR, "weight_decay": WD, "eps": EPS, "init_accum": INIT_ACCUM},
           "condition": "at W = 16 and W = 64 the apply step takes no longer than the round trip, each at the median "
                        "of its runs' event medians; a difference inside the larger of the two spreads counts as equal",
           "runs": runs, "summary": {}, "condition_met": True}
    legs = {}
    for r in runs:
        name = r["leg"] if r["dups"] == 1 else f"{r['leg']}_dups{r['dups']}"
        if r.get("kind", "adagrad") != "adagrad":
            name += "_" + r["kind"]
        if r.get("label"):
            name += "@" + r["label"]
        for w, x in r["widths"].items():
            legs.setdefault(name, {}).setdefault(w, []).append(x)
    for name, ws in legs.items():
        doc["summary"][name] = {}
        for w, xs in ws.items():
            e = [x["event_ms_median"] for x in xs]
            t = [x["library_timer_ms_per_call"] for x in xs]
            doc["summary"][name][w] = {"runs": len(xs), "event_ms": statistics.median(e), "event_ms_spread": max(e) - min(e),
                                       "library_timer_ms": statistics.median(t),
                                       "library_timer_ms_spread": max(t) - min(t)}
    base, new = "apply@parent", "apply@new"
    if base in legs and new in legs:
        # the regression guard of DESIGN.md §8d: the edited kernel's Adagrad step against the parent build's
        doc["what"] = ("tools/apply_probe.py --merge: one server-side step (pskv_apply) per kind; the Adagrad leg on a "
                       "build of the parent commit (label parent) and on this build (label new), alternating "
                       "(DESIGN.md 8d)")
        doc["condition"] = ("at each width this build's Adagrad step takes no longer than the parent build's, each at the "
                            "median of its runs' event medians; a difference inside the larger of the two spreads "
                            "counts as equal")
        doc["adagrad_new_over_parent"] = {}
        doc["adagrad_guard_met"] = True
        for w in legs[new]:
            n, b = doc["summary"][new][w], doc["summary"][base][w]
            slack = max(n["event_ms_spread"], b["event_ms_spread"])
            doc["adagrad_new_over_parent"][w] = round(n["event_ms"] / b["event_ms"], 3)
            doc["adagrad_guard_met"] = doc["adagrad_guard_met"] and n["event_ms"] <= b["event_ms"] + slack
        doc["condition_met"] = doc["adagrad_guard_met"]
        for k, streams in (("apply_momentum", 6), ("apply_adam", 8)):
            for name in (k, k + "@new"):
                if name in legs:
                    doc[k + "_over_parent_adagrad"] = {
                        w: round(doc["summary"][name][w]["event_ms"] / doc["summary"][base][w]["event_ms"], 3)
                        for w in legs[name]}
                    doc[k + "_model"] = round(streams / 6, 3)
    if "apply_adam@parent" in legs and "apply_adam@new" in legs:
        # the regression guard of DESIGN.md §8i: Adagrad (above) and Adam, parent build against this build
        doc["adam_new_over_parent"] = {}
        doc["adam_guard_met"] = True
        for w in legs["apply_adam@new"]:
            n, b = doc["summary"]["apply_adam@new"][w], doc["summary"]["apply_adam@parent"][w]
            slack = max(n["event_ms_spread"], b["event_ms_spread"])
            doc["adam_new_over_parent"][w] = round(n["event_ms"] / b["event_ms"], 3)
            doc["adam_guard_met"] = doc["adam_guard_met"] and n["event_ms"] <= b["event_ms"] + slack
        doc["condition_met"] = bool(doc["condition_met"]) and doc["adam_guard_met"]
    if "apply_ftrl@new" in legs and "apply_adam@new" in legs:
        # FTRL against Adam on one build: both move eight dense-sized streams of the touched rows (model 1);
        # reported, not gated
        doc["ftrl_over_adam"] = {}
        doc["ftrl_model"] = 1.0
        doc["ftrl_minus_adam_inside_spread"] = {}
        for w in legs["apply_ftrl@new"]:
            f, a = doc["summary"]["apply_ftrl@new"][w], doc["summary"]["apply_adam@new"][w]
            doc["ftrl_over_adam"][w] = round(f["event_ms"] / a["event_ms"], 3)
            doc["ftrl_minus_adam_inside_spread"][w] = bool(
                abs(f["event_ms"] - a["event_ms"]) <= max(f["event_ms_spread"], a["event_ms_spread"]))
    if "apply" in legs and "roundtrip" in legs:
        doc["apply_over_roundtrip"] = {}
        for w in legs["apply"]:
            a, r = doc["summary"]["apply"][w], doc["summary"]["roundtrip"].get(w)
            if not r:
                continue
            doc["apply_over_roundtrip"][w] = round(a["event_ms"] / r["event_ms"], 3)
            if w in ("16", "64"):
                slack = max(a["event_ms_spread"], r["event_ms_spread"])
                doc["condition_met"] = doc["condition_met"] and a["event_ms"] <= r["event_ms"] + slack
    elif base not in legs or new not in legs:
        doc["condition_met"] = None
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["apply", "roundtrip"])
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="OUT.json RUN.json ...")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--commit", default="", help="the commit the tree was built from (recorded)")
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--dups", type=int, default=1)
    ap.add_argument("--kind", choices=["adagrad", "momentum", "adam", "ftrl"], default="adagrad",
                    help="the apply leg's optimizer")
    ap.add_argument("--label", default="", help="kept in the run document; --merge keeps labelled runs apart")
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        txt = json.dumps(merge(a.merge[1:]), indent=1)
        with open(a.merge[0], "w") as f:
            f.write(txt + "\n")
        print(txt)
        return
    if not a.leg:
        ap.error("--leg or --merge is required")
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import parameter_server_amd as ps

    doc = {"leg": a.leg, "kind": a.kind, "label": a.label, "dups": a.dups, "commit": a.commit, "dtype": "float32", "rows": a.rows, "keys_per_call": a.keys,
           "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "widths": {}}
    for w in [int(x) for x in a.widths.split(",")]:
        r = run_width(ps, torch, a.leg, w, a.rows, a.keys, a.steps, a.warmup, a.dups, a.kind)
        doc["widths"][str(w)] = r
        print(f"W={w} {a.leg} dups={a.dups}: events {r['event_ms_median']:.4f} ms, library timers "
              f"{r['library_timer_ms_per_call']:.4f} ms", flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
