"""bench.py's plain run and its --dump-outputs: the result line of a plain run, the arrays of its last timed step, and
that two runs with the same arguments write the same arrays, with or without --full.  The sampler of large outputs runs
without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS, ROOT


def test_dump_sample_is_whole_when_small_and_a_fixed_spread_sample_when_large():
    import bench
    t = torch.rand(4, 5, 6)
    s = bench._dump_sample(t, 120, 1)
    assert s.shape == t.shape and s.dtype == torch.float32 and torch.equal(s, t)
    assert s.data_ptr() != t.data_ptr()                          # a copy: the next step may overwrite the original
    assert torch.equal(bench._dump_sample(t.to(torch.bfloat16), 120, 1), t.to(torch.bfloat16).float())
    big = torch.arange(1_000_003, dtype=torch.float64)
    a, b = bench._dump_sample(big, 1000, 5), bench._dump_sample(big, 1000, 5)
    assert a.shape == (1000,) and a.dtype == torch.float32 and torch.equal(a, b)
    idx = a.double()                                             # the values are their own positions
    assert bool((idx[1:] > idx[:-1]).all()) and idx[0] < 1001 and idx[-1] > 1_000_003 - 1001
    assert not torch.equal(a, bench._dump_sample(big, 1000, 6))


def _bench_run(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "512",
           "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    out = _bench_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["value"] > 0 and abs(out["value"] - 512 * 1e3 / out["ms_per_step"]) <= 2e-3 * out["value"]
    for k in ("roofline", "kernels", "forward", "exact_f32", "cpu_baseline"):     # --full only
        assert k not in out, k
    names = {"loss", "Y"} | {"param_" + k for k in PARAM_KEYS}
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["Y"].shape == (512, 24, 102) and a["param_gru.weight_ih_l0"].shape == (306, 442)
    assert abs(float(a["loss"]) - out["loss"]) <= 1e-6
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in names) <= 64 << 20
    _bench_run(tmp_path / "b")                                   # same arguments: same inputs, same outputs
    full = _bench_run(tmp_path / "c", "--full", "--no-traffic", "--no-secondary", "--no-cpu-baseline")
    assert full["full"] is True and "roofline" in full and full["loss"] == out["loss"]   # --full: same steps, more figures
    for n in names:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / (n + ".npy"))), n
        assert np.array_equal(a[n], np.load(tmp_path / "c" / (n + ".npy"))), n
