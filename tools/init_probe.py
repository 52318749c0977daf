"""What a row initializer costs: f32, device path, W = 4 / 16 / 64.

  step_steady   an Adagrad step (pskv_apply) on a sparse shard that holds KEYS
                keys, none of the call's keys new: row kernels + index launches,
                by the library's timers.  With a rule set, the index operation
                includes k_row_init_new's two-word launch.
  step_all_new  the same step on an emptied shard: every key of the call is new
                (pskv_clear before each call, outside the timers)
  dense_fill    pskv_clear of a dense row shard of ROWS rows: host clock around
                the call (it returns when the fill is done), in GB/s of rows

  --kinds zero            uses only calls a build from before initializers has:
                          run from such a checkout it is the parent's leg
  --kinds zero,uniform,normal
  --merge OUT A.json B.json ...   no GPU: the documents side by side, with the ratios

A probe, not a threshold: nothing asserts these numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_sparse(ps, kind, capacity, w):
    sh = ps.Shard.sparse(capacity, np.float32, "assign", width=w)
    if kind != "zero":
        sh.set_initializer(kind, -0.01 if kind == "uniform" else 0.0, 0.01, seed=1)
    sh.set_optimizer("adagrad", lr=0.05, eps=1e-8, init_accum=0.1)
    return sh


def step_ms(sh, steps):
    return (sh.apply_time()["total_ms"] + sh.index_time()["total_ms"]) / steps, sh.index_time()["total_ms"] / steps


def run(ps, torch, kind, w, a):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(99 + w)
    uniq = torch.unique(torch.randint(-2**31, 2**31, (a.keys + a.keys // 8 + 64,), generator=g, device=dev))[:a.keys]
    assert uniq.numel() == a.keys
    keys = [uniq[torch.randperm(a.keys, generator=g, device=dev)].to(torch.int32).contiguous() for _ in range(2)]
    grads = torch.randn((a.keys, w), generator=g, device=dev, dtype=torch.float32)
    res = {}
    for leg in ("step_steady", "step_all_new"):
        with make_sparse(ps, kind, 2 * a.keys, w) as sh:
            sh.apply(keys[0], grads)
            sh.sync()
            sh.set_timing(True)
            for i in range(a.warmup + a.steps):
                if leg == "step_all_new":
                    sh.clear()
                if i == a.warmup:
                    sh.sync()
                    sh.reset_timing()
                sh.apply(keys[i % 2], grads)
            sh.sync()
            ms, index_ms = step_ms(sh, a.steps)
            res[leg] = {"ms_per_step": ms, "index_ms_per_step": index_ms}
    with ps.Shard(0, a.rows, np.float32, width=w) as sh:
        if kind != "zero":
            sh.set_initializer(kind, -0.01 if kind == "uniform" else 0.0, 0.01, seed=1)
        times = []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sh.clear()
            times.append(time.perf_counter() - t0)
        t = float(np.median(times[a.warmup:]))
        res["dense_fill"] = {"ms": t * 1e3, "GBps": a.rows * w * 4 / t / 1e9}
    return res


def merge(paths):
    docs = [json.load(open(p)) for p in paths]
    out = {"what": "tools/init_probe.py --merge (DESIGN.md 8q)", "runs": docs, "ratios": {}}
    new = next((d for d in docs if "normal" in d["kinds"]), None)
    if new:
        for w, k in new["kinds"]["normal"].items():
            z = new["kinds"]["zero"][w]
            out["ratios"][w] = {leg: round(k[leg]["ms_per_step"] / z[leg]["ms_per_step"], 3)
                                for leg in ("step_steady", "step_all_new")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="zero,uniform,normal")
    ap.add_argument("--merge", nargs="+", metavar="JSON")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_probe.json"))
    a = ap.parse_args()
    if a.merge:
        doc = merge(a.merge)
    else:
        import torch

        import parameter_server_amd as ps

        doc = {"label": a.label, "dtype": "float32", "keys_per_step": a.keys, "dense_rows": a.rows, "steps": a.steps,
               "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kinds": {}}
        for kind in a.kinds.split(","):
            doc["kinds"][kind] = {}
            for w in [int(x) for x in a.widths.split(",")]:
                doc["kinds"][kind][str(w)] = r = run(ps, torch, kind, w, a)
                print(f"{a.label} {kind} W={w}: " + json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
