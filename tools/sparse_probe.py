"""A sparse shard against the dense row shard it stands on: f32,
device path, KEYS uniformly random distinct uint32 keys, 4 orders of them in
rotation.  Times a Get, an assign Add and an Adagrad step (pskv_apply) per
width with the library's own timers.

  --leg sparse  a sparse shard of CAPACITY slots that already holds the keys;
                the time of a call is its row kernels plus its index launches
                (pskv_index_time), whose share is reported
  --leg dense   the dense row shard [0, CAPACITY) fed, position by position, a
                slot number in place of the key: distinct random rows of
                [0, KEYS), which is where a sparse shard that took the keys in
                one call keeps them.  This is the work a build from before
                sparse shards can already do -- the floor -- and the leg uses
                only calls such a build has.

Prints one JSON document and writes it to --out.

  --merge SPARSE.json DENSE.json
                no GPU: both documents side by side with the ratios sparse /
                dense and the index's share of the sparse time.
                profiles/sparse_probe.json is the output of this mode.

A probe, not a threshold: nothing asserts these numbers.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ("get", "assign", "apply_adagrad")


def kernel_ids(ps, sh):
    n = 0
    while True:  # every kernel id this build knows
        try:
            sh.kernel_time(n)
        except ps.PskvError:
            return list(range(n))
        n += 1


def run_leg(ps, torch, leg, w, capacity, nkeys, steps, warmup, options):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(4321 + w)
    if leg == "sparse":
        # distinct uniformly random uint32 keys (as int32 bits): draw with room to spare, keep the first nkeys distinct
        draw = torch.randint(-2**31, 2**31, (nkeys + nkeys // 8 + 64,), generator=g, device=dev, dtype=torch.int64)
        uniq = torch.unique(draw)
        uniq = uniq[torch.randperm(uniq.numel(), generator=g, device=dev)][:nkeys]
        assert uniq.numel() == nkeys, "not enough distinct keys drawn"
        base = uniq.to(torch.int32)
    else:
        base = torch.randperm(nkeys, generator=g, device=dev).to(torch.int32)
    keys = [base[torch.randperm(nkeys, generator=g, device=dev)].contiguous() for _ in range(4)]
    vals = [torch.randn((nkeys, w), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
    out = torch.empty((nkeys, w), dtype=torch.float32, device=dev)
    res = {}
    for op in OPS:
        if leg == "sparse":
            sh = ps.Shard.sparse(capacity, np.float32, "assign", width=w, options=options)
        else:
            sh = ps.Shard(0, capacity, np.float32, mode="assign", width=w, options=options)
        with sh:
            if op == "apply_adagrad":
                sh.set_optimizer("adagrad", lr=0.05, eps=1e-8, init_accum=0.1)
            sh.add(keys[0], vals[0])  # the shard holds the keys (and their rows) before anything is timed
            sh.sync()
            if leg == "sparse":
                assert sh.sparse_info()["count"] == nkeys
            ids = kernel_ids(ps, sh)
            sh.set_timing(True)
            for i in range(warmup + steps):
                if i == warmup:
                    sh.sync()
                    sh.reset_timing()
                if op == "get":
                    sh.get(keys[i % 4], out=out)
                elif op == "assign":
                    sh.add(keys[i % 4], vals[i % 4])
                else:
                    sh.apply(keys[i % 4], vals[i % 4])
            sh.sync()
            rows_ms = sum(sh.kernel_time(k)["total_ms"] for k in ids) + sh.apply_time()["total_ms"]
            index_ms = sh.index_time()["total_ms"] if leg == "sparse" else 0.0
            per = (rows_ms + index_ms) / steps
            payload = nkeys * w * 4
            res[op] = {"ms_per_call": per, "row_kernels_ms_per_call": rows_ms / steps,
                       "index_ms_per_call": index_ms / steps, "index_share": index_ms / (rows_ms + index_ms),
                       "row_payload_GBps": payload / (per / 1e3) / 1e9}
        torch.cuda.synchronize()
    return res


def merge(sparse_path, dense_path):
    with open(sparse_path) as f:
        sp = json.load(f)
    with open(dense_path) as f:
        dn = json.load(f)
    doc = {"what": "tools/sparse_probe.py --merge: a sparse shard against the dense row shard fed slot numbers "
                   "(DESIGN.md 8k)",
           "setup": {k: sp[k] for k in ("dtype", "capacity", "keys_per_call", "steps", "warmup", "device")},
           "notes": ["each leg is one run of `steps` timed calls; a probe, no test asserts these numbers",
                     "the sparse time of a call = its row kernels + its index launches (insert for the writing "
                     "calls, translate for all), each timed as the library times them",
                     "byte model of the index per key: 4 B of key read, one random 64 B line of the table at least, "
                     "4 B of slot id written (and read again by the row kernels)"],
           "sparse": sp["widths"], "dense": dn["widths"], "ratio_sparse_over_dense": {}, "index_share_of_sparse": {}}
    for w, ops in sp["widths"].items():
        doc["ratio_sparse_over_dense"][w] = {op: round(ops[op]["ms_per_call"] / dn["widths"][w][op]["ms_per_call"], 3)
                                             for op in ops}
        doc["index_share_of_sparse"][w] = {op: round(ops[op]["index_share"], 3) for op in ops}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["sparse", "dense"])
    ap.add_argument("--merge", nargs=2, metavar=("SPARSE.json", "DENSE.json"))
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="a shard option (pskv_set_option), e.g. NT=0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        txt = json.dumps(merge(a.merge[0], a.merge[1]), indent=1)
    else:
        if not a.leg:
            ap.error("--leg or --merge is required")
        import torch

        import parameter_server_amd as ps

        options = {n: int(v) for n, v in (o.split("=") for o in a.option)}
        doc = {"leg": a.leg, "options": options, "dtype": "float32", "capacity": a.capacity, "keys_per_call": a.keys,
               "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "widths": {}}
        for w in [int(x) for x in a.widths.split(",")]:
            doc["widths"][str(w)] = run_leg(ps, torch, a.leg, w, a.capacity, a.keys, a.steps, a.warmup, options)
            print(f"W={w} {a.leg}: " + ", ".join(f"{op} {r['ms_per_call']:.4f} ms (index {r['index_share']:.0%})"
                                                 for op, r in doc["widths"][str(w)].items()), flush=True)
        txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
