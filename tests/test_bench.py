"""bench.py's plain run and --dump-outputs: the result line of a plain run, and the dumped arrays of its last
timed step (the CPU test covers the sampling of long arrays, the -m gpu test the values themselves)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_sampling(tmp_path):
    import torch
    import bench
    env = SimpleNamespace(torch=torch, world=1, rank=0)
    n_long = bench.DUMP_SAMPLE + 12345
    arrays = {"values": torch.arange(n_long, dtype=torch.float64), "leaf": torch.arange(7, dtype=torch.int32) - 3}
    bench.dump_outputs(env, str(tmp_path / "a"), arrays)
    bench.dump_outputs(env, str(tmp_path / "b"), arrays)
    leaf = np.load(tmp_path / "a" / "leaf.npy")
    assert leaf.dtype == np.float64 and np.array_equal(leaf, np.arange(7) - 3)        # short arrays whole, ids exact
    v = np.load(tmp_path / "a" / "values.npy")
    assert v.dtype == np.float64 and len(v) == bench.DUMP_SAMPLE                      # long arrays: a sample ...
    assert (np.diff(v) > 0).all() and v[0] >= 0 and v[-1] < n_long                   # ... of distinct entries, in order
    assert np.array_equal(v, np.load(tmp_path / "b" / "values.npy"))                  # ... the same in every run
    # several ranks: one file per rank, the sample shrinks with the world so that all ranks stay within the budget
    bench.dump_outputs(SimpleNamespace(torch=torch, world=4, rank=2), str(tmp_path / "c"), arrays)
    assert sorted(os.listdir(tmp_path / "c")) == ["leaf_rank2.npy", "values_rank2.npy"]
    assert len(np.load(tmp_path / "c" / "values_rank2.npy")) == bench.DUMP_SAMPLE // 4


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(orc, tmp_path):
    """C1 (N = 512 Gaussian, M = 10k targets): a plain run prints the headline line only, with the asked-for
    number of timed steps, and its dumped values / weights are the oracle's interpolant on the same clouds."""
    out_dir = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "C1", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["config"]["config"] == "C1"
    assert "cpu_baseline" not in line and not line["extra"].get("other_configs")       # the rest is --full's
    assert sorted(os.listdir(out_dir)) == ["values.npy", "weights.npy"]
    vals, w = np.load(out_dir / "values.npy"), np.load(out_dir / "weights.npy")
    assert vals.dtype == np.float64 and vals.shape == (10_000,) and w.shape == (512,)
    n, dim = 512, 2
    eps = orc.gaussian_eps(n, dim)
    x = orc.synth_centres(n, dim)
    y = orc.synth_targets(0, 10_000, dim)
    want = orc.rbf_eval(0, eps, x, orc.rbf_solve(0, eps, x, orc.synth_response(x)), y)
    assert np.abs(vals - want).max() / np.abs(want).max() < 1e-8
    # the dumped weights are the ones the dumped values were swept with
    again = orc.rbf_eval(0, eps, x, w, y)
    assert np.abs(vals - again).max() / np.abs(again).max() < 1e-10
