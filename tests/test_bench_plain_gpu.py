"""A plain bench.py run (no --full) end to end on one GPU, at a reduced window
count: the result line carries the headline alone, and --dump-outputs writes
what the last timed step handed back — compared here with a torch model of the
shard replaying the same warm-up and timed steps (sequential last-write-wins
slice assigns; never-written keys read 0)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(cuda, tmp_path):
    import torch

    import bench

    J, B, R, steps, warmup = 8, 1_000_000, 3, 4, 1
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--batches", str(J), "--batch-keys", str(B), "--sets", str(R), "--dump-outputs", str(out)]
    r = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert res["metric"] == bench.METRIC and res["unit"] == "GB/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["n_gpus"] == 1 and res["steps"] == steps and res["warmup"] == warmup
    assert res["value"] > 0 and res["ms_per_step"] > 0
    # value = the steps' algorithmic bytes over the steps' time
    assert res["value"] == pytest.approx(res["config"]["bytes_per_step_per_gpu"] / res["ms_per_step"] / 1e6, rel=1e-6)
    assert res["config"]["push_pull_overlap_keys"] == 0 and res["config"]["window_sets"] == R
    for k in ("roofline", "zipf_sparse", "extra", "cpu_baseline"):  # --full's
        assert k not in res
    assert sorted(os.listdir(out)) == ["param_sample.npy", "pull_values.npy"]
    pulled, params = np.load(out / "pull_values.npy"), np.load(out / "param_sample.npy")
    assert pulled.dtype == np.float32 and params.dtype == np.float32
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 10 ** 6

    # the model: the run's step order (max(warmup, R) warm-up steps, then the timed ones, both from step 0)
    dev = torch.device(cuda)
    sets = [bench.make_set(0, 1, J, B, dev, s) for s in range(R)]
    ref = torch.zeros(100_000_000, dtype=torch.float32, device=dev)
    for i in list(range(max(warmup, R))) + list(range(steps)):
        for (_, first, n), (_, v) in zip(sets[i % R]["slices"], sets[i % R]["batches"]):
            ref[first:first + n] = v
    last = sets[(steps - 1) % R]
    want = torch.cat([ref[first:first + n] for _, first, n in last["pull"]])
    pos = bench.dump_positions(want.numel())
    assert pos is not None and want.numel() > bench.DUMP_MAX_ELEMS  # the sampled branch
    want = want[torch.from_numpy(pos).to(dev)].cpu().numpy()
    assert np.array_equal(pulled.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(pulled) > 0  # windows pushed by the other sets' steps are among the pulls
    keys = torch.from_numpy(bench.dump_param_keys(0, 100_000_000)).to(dev)
    assert np.array_equal(params.view(np.uint32), ref[keys].cpu().numpy().view(np.uint32))
    assert np.count_nonzero(params) > 0
