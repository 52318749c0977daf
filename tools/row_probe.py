"""Row-valued shards against the flattening they replace (DESIGN.md "Row-valued
shards"): f32, device path, a table of ROWS rows (at the default 16 Mi rows the
dense array exceeds the 256 MiB Infinity Cache from W = 16 on and equals it at
W = 4), KEYS uniformly random keys pushed and pulled per step,
4 distinct key draws in rotation.  Times Get, assign Add and accumulate Add
with the library's own kernel timers.

  --leg row   a width-W shard (this library's row form)
  --leg flat  the same logical traffic as scalar keys k * W + j on a scalar
              shard of ROWS * W keys, through the unsorted device Add and Get:
              the workaround.  It uses only the scalar API, so the same script
              runs on a build from before row shards existed (the baseline).

Prints one JSON document and writes it to --out.

  --merge ROW.json FLAT.json [--extra NAME=PATH ...]
              no GPU: put a row-leg and a flattened-leg document side by side
              with the ratios row / flattened and whether the condition holds
              (at W = 16 and W = 64 no operation's row form takes longer);
              further runs (a repeat, another option) ride along under NAME.
              profiles/rows_probe.json is the output of this mode.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(sh, ids):
    """Sum of the timed kernels' time per call, and the launches behind it."""
    tot, launches = 0.0, 0
    for k in ids:
        t = sh.kernel_time(k)
        tot += t["total_ms"]
        launches += t["launches"]
    return tot, launches


def run_leg(ps, torch, leg, w, rows, nkeys, steps, warmup, options):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + w)
    draws = [torch.randint(0, rows, (nkeys,), generator=g, device=dev, dtype=torch.int64) for _ in range(4)]
    vals = [torch.randn((nkeys, w), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
    if leg == "row":
        keys = [d.to(torch.int32) for d in draws]
        pv = vals
        mk = lambda mode: ps.Shard(0, rows, np.float32, mode=mode, width=w, options=options)  # noqa: E731
        out = torch.empty((nkeys, w), dtype=torch.float32, device=dev)
    else:
        j = torch.arange(w, device=dev, dtype=torch.int64)
        keys = [(d[:, None] * w + j[None, :]).reshape(-1).to(torch.int32) for d in draws]  # < 2^31
        pv = [v.reshape(-1) for v in vals]
        mk = lambda mode: ps.Shard(0, rows * w, np.float32, mode=mode, options=options)  # noqa: E731
        out = torch.empty(nkeys * w, dtype=torch.float32, device=dev)
    del draws
    res = {}
    for op in ("get", "assign", "accumulate"):
        with mk("accumulate" if op == "accumulate" else "assign") as sh:
            nk = 0
            while True:  # every kernel id this build knows
                try:
                    sh.kernel_time(nk)
                except ps.PskvError:
                    break
                nk += 1
            ids = list(range(nk))
            if op == "get":  # pull rows that were written
                for i in range(4):
                    sh.add(keys[i], pv[i])
            sh.set_timing(True)
            for i in range(warmup + steps):
                if i == warmup:
                    sh.sync()
                    sh.reset_timing()
                if op == "get":
                    sh.get(keys[i % 4], out=out)
                else:
                    sh.add(keys[i % 4], pv[i % 4])
            sh.sync()
            ms, launches = timed_ms(sh, ids)
            per = ms / steps
            payload = nkeys * w * 4
            res[op] = {
                "ms_per_call": per,
                "kernel_launches_per_call": launches / steps,
                "row_payload_GBps": payload / (per / 1e3) / 1e9,
                # keys read + rows read + rows written (Add: the read-modify-write of the table)
                "algorithmic_GBps": ((keys[0].numel() * 4) + 2 * payload) / (per / 1e3) / 1e9,
            }
        torch.cuda.synchronize()
    return res


def merge(row_path, flat_path, extras, flat_commit):
    with open(row_path) as f:
        row = json.load(f)
    with open(flat_path) as f:
        flat = json.load(f)
    doc = {"what": "tools/row_probe.py --merge: a row-valued shard against the flattened scalar form it replaces "
                   "(DESIGN.md 8b)",
           "setup": {k: row[k] for k in ("dtype", "rows", "keys_per_call", "steps", "warmup", "device")},
           "notes": ["each leg is one run of `steps` timed calls",
                     "kernel_launches_per_call counts timed kernel ids: the row assign is 1.0 although two kernels "
                     "run (k_general_mark + k_row_commit are timed as the one id PSKV_K_ROW_COMMIT)",
                     "at W = 4 the dense array (rows * 16 B) equals the 256 MiB Infinity Cache, it does not exceed it"],
           "condition": "at W = 16 and W = 64 the row form of Get, assign Add and accumulate Add takes no longer than "
                        "the flattened form",
           "flattened_leg_commit": flat_commit,
           "context_only": {"guide_random_row_register_gather_TBps": 5.5, "guide_float_atomic_added_bytes_TBps": 1.3},
           "row": row["widths"], "flattened": flat["widths"], "ratio_row_over_flattened": {}, "condition_met": True}
    for w, ops in row["widths"].items():
        r = {op: round(ops[op]["ms_per_call"] / flat["widths"][w][op]["ms_per_call"], 3) for op in ops}
        doc["ratio_row_over_flattened"][w] = r
        if w in ("16", "64"):
            doc["condition_met"] = doc["condition_met"] and all(v <= 1 for v in r.values())
    for e in extras:
        name, path = e.split("=", 1)
        with open(path) as f:
            x = json.load(f)
        doc[name] = {"leg": x["leg"], "options": x.get("options", {}), "widths": x["widths"]}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["row", "flat"])
    ap.add_argument("--merge", nargs=2, metavar=("ROW.json", "FLAT.json"))
    ap.add_argument("--extra", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--flat-commit", default="", help="--merge: the commit the flattened leg was built from")
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="a shard option (pskv_set_option), e.g. NT=0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        txt = json.dumps(merge(a.merge[0], a.merge[1], a.extra, a.flat_commit), indent=1)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    if not a.leg:
        ap.error("--leg or --merge is required")
    import torch

    import parameter_server_amd as ps

    options = {n: int(v) for n, v in (o.split("=") for o in a.option)}
    doc = {"leg": a.leg, "options": options, "dtype": "float32", "rows": a.rows, "keys_per_call": a.keys, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "widths": {}}
    for w in [int(x) for x in a.widths.split(",")]:
        doc["widths"][str(w)] = run_leg(ps, torch, a.leg, w, a.rows, a.keys, a.steps, a.warmup, options)
        print(f"W={w} {a.leg}: " + ", ".join(f"{op} {r['ms_per_call']:.4f} ms" for op, r in doc["widths"][str(w)].items()),
              flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
