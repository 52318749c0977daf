"""Growth and erase of a sparse shard: f32, Adagrad state (one
state slot), KEYS uniformly random distinct uint32 keys stored, per width.

  (a) reserve   pskv_sparse_reserve of a shard that holds KEYS keys at capacity
                KEYS, to 2 * KEYS
  (b) erase     pskv_sparse_erase of a random 10 % of the KEYS stored keys
                (device list)
  (c) step      an Adagrad step (pskv_apply, device path) of the KEYS stored
                keys at capacity 4 * KEYS, with growth enabled but never firing
                against the same step with growth off -- the work a build from
                before growth can already do.  The two shards alternate, round
                by round, in one run.

(a) and (b) are host calls that return when the device is done: a host clock
around the call, the device idle before it.  Their floor, timed the same way in
the same run: plain device-to-device copies of the surviving row and state
bytes plus a memset of the new table.  The floor leaves out what the rebuild
also does -- the random 8-byte table stores, slot_keys, the start values of the
free rows, the zeroed gradient scratch and stamp array, the allocations -- so
the ratio is reported, not asserted.  (c): the library's own timers (the step's
row kernels plus its index launches) and the host clock per call.

Prints one JSON document and writes it to --out (profiles/sparse_grow_probe.json).
A probe, not a threshold: nothing asserts these numbers.
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


def table_bytes(capacity):
    return max(16, 1 << (2 * capacity - 1).bit_length()) * 8


def draw_keys(torch, g, dev, nkeys):
    draw = torch.randint(-2**31, 2**31, (nkeys + nkeys // 8 + 64,), generator=g, device=dev, dtype=torch.int64)
    uniq = torch.unique(draw)
    uniq = uniq[torch.randperm(uniq.numel(), generator=g, device=dev)][:nkeys]
    assert uniq.numel() == nkeys, "not enough distinct keys drawn"
    return uniq.to(torch.int32).contiguous()


def clock(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def floor_ms(torch, dev, rows, w, arrays, new_capacity):
    """`arrays` device-to-device copies of rows x w f32 and a memset of the new table."""
    src = [torch.empty((rows, w), dtype=torch.float32, device=dev).normal_() for _ in range(arrays)]
    dst = [torch.empty((rows, w), dtype=torch.float32, device=dev) for _ in range(arrays)]
    table = torch.empty(table_bytes(new_capacity) // 8, dtype=torch.int64, device=dev)

    def run():
        for s, d in zip(src, dst):
            d.copy_(s)
        table.zero_()

    run()  # warm
    return clock(torch, run)


def stored_shard(ps, torch, keys, w, capacity, g, dev, max_capacity=None):
    sh = ps.Shard.sparse(capacity, np.float32, "assign", width=w, max_capacity=max_capacity)
    sh.set_optimizer("adagrad", lr=0.05, eps=1e-8, init_accum=0.1)
    sh.apply(keys, torch.randn((keys.numel(), w), generator=g, device=dev, dtype=torch.float32))
    sh.sync()
    assert sh.sparse_info()["count"] == keys.numel()
    return sh


def run_width(ps, torch, w, nkeys, reps, steps, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(8765 + w)
    keys = draw_keys(torch, g, dev, nkeys)
    res = {}
    # (a) reserve KEYS -> 2 KEYS, a fresh shard per repetition
    times, floors = [], []
    for _ in range(reps):
        with stored_shard(ps, torch, keys, w, nkeys, g, dev) as sh:
            times.append(clock(torch, lambda: sh.reserve(2 * nkeys)))
            assert sh.sparse_info()["capacity"] == 2 * nkeys and sh.sparse_info()["count"] == nkeys
        floors.append(floor_ms(torch, dev, nkeys, w, 2, 2 * nkeys))
    res["reserve"] = {"ms": times, "floor_ms": floors, "median_ms": statistics.median(times),
                      "median_floor_ms": statistics.median(floors),
                      "ratio_to_floor": statistics.median(times) / statistics.median(floors)}
    # (b) erase a random 10 %
    times, floors = [], []
    for _ in range(reps):
        gone = keys[torch.randperm(nkeys, generator=g, device=dev)[: nkeys // 10]].contiguous()
        with stored_shard(ps, torch, keys, w, nkeys, g, dev) as sh:
            times.append(clock(torch, lambda: sh.erase(gone)))
            assert sh.sparse_info()["count"] == nkeys - nkeys // 10
        floors.append(floor_ms(torch, dev, nkeys - nkeys // 10, w, 2, nkeys))
    res["erase_10pct"] = {"ms": times, "floor_ms": floors, "median_ms": statistics.median(times),
                          "median_floor_ms": statistics.median(floors),
                          "ratio_to_floor": statistics.median(times) / statistics.median(floors)}
    # (c) the step with growth on (never firing) against growth off, alternating
    order = [keys[torch.randperm(nkeys, generator=g, device=dev)].contiguous() for _ in range(4)]
    grads = [torch.randn((nkeys, w), generator=g, device=dev, dtype=torch.float32) for _ in range(4)]
    rounds = {"off": [], "on": []}
    with stored_shard(ps, torch, keys, w, 4 * nkeys, g, dev) as off, \
            stored_shard(ps, torch, keys, w, 4 * nkeys, g, dev, max_capacity=8 * nkeys) as on:
        for sh in (off, on):
            sh.set_timing(True)
        for _ in range(reps):
            for name, sh in (("off", off), ("on", on)):
                for i in range(warmup):
                    sh.apply(order[i % 4], grads[i % 4])
                sh.sync()
                sh.reset_timing()
                t0 = time.perf_counter()
                for i in range(steps):
                    sh.apply(order[i % 4], grads[i % 4])
                sh.sync()
                host = (time.perf_counter() - t0) * 1e3 / steps
                rounds[name].append({"timers_ms_per_call": (sh.apply_time()["total_ms"] + sh.index_time()["total_ms"]) / steps,
                                     "host_ms_per_call": host})
        assert on.growth()["rebuilds"] == 0 and on.sparse_info()["capacity"] == 4 * nkeys
    ratio = [a["timers_ms_per_call"] / b["timers_ms_per_call"] for a, b in zip(rounds["on"], rounds["off"])]
    res["step_growth_on_over_off"] = {"rounds": rounds, "ratio_timers": ratio,
                                      "ratio_host": [a["host_ms_per_call"] / b["host_ms_per_call"]
                                                     for a, b in zip(rounds["on"], rounds["off"])],
                                      "mean_ratio_timers": statistics.mean(ratio)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--widths", default="4,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import parameter_server_amd as ps

    doc = {"what": "tools/sparse_grow_probe.py: reserve, erase and the growth check of a sparse shard (DESIGN.md 8l)",
           "setup": {"dtype": "float32", "optimizer": "adagrad", "keys": a.keys, "reps": a.reps, "steps": a.steps,
                     "warmup": a.warmup, "device": torch.cuda.get_device_name(0)},
           "notes": ["reserve and erase: host clock around the blocking call, the device idle before it",
                     "floor: device-to-device copies of the surviving rows (parameters and the one state slot) plus a "
                     "memset of the new table, timed the same way in the same run; the rebuild's table stores, slot_keys, "
                     "start values of the free rows, zeroed scratch arrays and allocations are not in it",
                     "step: growth on with a limit that never fires against growth off, the two shards alternating"],
           "widths": {}}
    for w in [int(x) for x in a.widths.split(",")]:
        doc["widths"][str(w)] = r = run_width(ps, torch, w, a.keys, a.reps, a.steps, a.warmup)
        print(f"W={w}: reserve {r['reserve']['median_ms']:.3f} ms ({r['reserve']['ratio_to_floor']:.2f}x floor), "
              f"erase {r['erase_10pct']['median_ms']:.3f} ms ({r['erase_10pct']['ratio_to_floor']:.2f}x floor), "
              f"step on/off {r['step_growth_on_over_off']['mean_ratio_timers']:.4f}", flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
