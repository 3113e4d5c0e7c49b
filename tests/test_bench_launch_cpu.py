"""CPU test (-m "not gpu") of bench.py's launcher path: `python bench.py --gpus 2` with no launcher around it must
start the ranks itself (python -m torch.distributed.run as a CHILD, never exec), and relay exactly one JSON line.
--stub swaps the HIP step for a stand-in so that the plumbing (rendezvous on 127.0.0.1, barrier, max over ranks,
rank-0 line, weak / strong batch split) runs on gloo ranks here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--steps", "3", "--warmup", "1", *flags],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("scaling,per_rank", [("weak", 8), ("strong", 4), (None, 4)])
def test_self_launch_two_ranks(scaling, per_rank):
    """the default is BASELINE config 4's shape: a GLOBAL batch of 8 frames over the ranks (strong scaling)"""
    r = _run("--gpus", "2", *(("--scaling", scaling) if scaling else ()))
    scaling = scaling or "strong"
    assert r["n_gpus"] == 2 and r["ranks"] == 2 and r["steps"] == 3 and r["warmup"] == 1
    assert r["scaling"] == scaling and r["config"]["frames_per_gpu"] == per_rank
    assert r["config"]["global_batch"] == 2 * per_rank and r["value"] > 0


def test_single_rank_needs_no_launcher():
    r = _run()
    assert r["n_gpus"] == 1 and r["config"]["frames_per_gpu"] == 8


def test_dump_outputs_are_float32_and_repeatable(tmp_path):
    """--dump-outputs DIR: the last timed step's loss / parameters / gradients as .npy, identical from run to run"""
    runs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = _run("--dump-outputs", str(d))
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        runs.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert set(runs[0]) == {"loss.npy", "parameters.npy", "gradients.npy"}
    for name, a in runs[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        assert np.array_equal(a, runs[1][name]), name


def test_full_is_off_by_default():
    """a plain run measures the headline alone; the side measurements come with --full"""
    sys.path.insert(0, ROOT)
    import bench
    assert not bench.parse_args(["--steps", "3"]).full
    a = bench.parse_args(["--full", "--no-side-runs"])
    assert a.full and a.no_side_runs and not a.no_op_table and not a.no_cpu_baseline


def test_dump_outputs_samples_large_arrays_within_the_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    big = {"a": torch.arange(30 << 20, dtype=torch.float32), "b": torch.ones(5, 7, dtype=torch.float64)}
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), big)
    total = sum(os.path.getsize(tmp_path / "0" / f) for f in os.listdir(tmp_path / "0"))
    assert total <= bench.DUMP_BYTES
    a0, a1 = np.load(tmp_path / "0" / "a.npy"), np.load(tmp_path / "1" / "a.npy")
    assert a0.dtype == np.float32 and np.array_equal(a0, a1) and (np.diff(a0) >= 0).all()   # the same sorted sample each time
    assert a0.size < (30 << 20)
    assert np.array_equal(np.load(tmp_path / "0" / "b.npy"), np.ones((5, 7), np.float32))
