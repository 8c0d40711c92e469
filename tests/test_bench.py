"""bench.py command line: the result line, --dump-outputs and --full.

The benchmark is started as a process because its command line is what is
under test; sizes are tiny so a run is dominated by interpreter start-up.
"""

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")

# 4.125 Mi bf16 elements: just above the 4 Mi-element threshold at which a
# dump becomes a seeded sample, and not a power of two
SIZE_MIB = "8.25"
STEPS = 3


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_bench(*extra):
    env = os.environ.copy()
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR"):
        env.pop(k, None)
    env["MASTER_PORT"] = str(free_port())
    proc = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS),
         "--warmup", "1", "--size-mib", SIZE_MIB, *extra],
        env=env, cwd=REPO, timeout=120, stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    return json.loads(proc.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    dirs = [str(tmp_path_factory.mktemp("dump")) for _ in range(2)]
    recs = [run_bench("--dump-outputs", d) for d in dirs]
    return dirs, recs


def check_record(rec):
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in rec
    assert rec["metric"] == "allreduce_fwdbwd_algbw_GBps"
    assert rec["unit"] == "GB/s" and rec["dtype"] == "bf16"
    assert rec["higher_is_better"] is True
    assert rec["steps"] == STEPS
    assert rec["ms_per_step"] > 0
    # value is 2 * bytes / t_step in GB/s, from the same timing
    nbytes = int(float(SIZE_MIB) * 1024 * 1024 // 2) * 2
    expect = 2 * nbytes / (rec["ms_per_step"] * 1e-3) / 1e9
    assert rec["value"] == pytest.approx(expect, rel=0.05)


def test_plain_run_record(two_runs):
    _, recs = two_runs
    for rec in recs:
        check_record(rec)
        # secondary measurements only run with --full
        assert "n1_default_path_ms" not in rec["config"]


def test_dump_outputs_repeatable(two_runs):
    dirs, _ = two_runs
    names = sorted(os.listdir(dirs[0]))
    assert names == ["allreduce_out.npy", "input_grad.npy"]
    assert sorted(os.listdir(dirs[1])) == names
    total = 0
    for name in names:
        a = np.load(os.path.join(dirs[0], name))
        b = np.load(os.path.join(dirs[1], name))
        assert a.dtype == np.float32 and a.size == 1 << 22
        assert np.array_equal(a, b)
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    # world 1, SUM: the result is the (random normal) input, its adjoint
    # hands the all-ones seed back
    out = np.load(os.path.join(dirs[0], "allreduce_out.npy"))
    assert np.isfinite(out).all() and 0.9 < out.std() < 1.1
    assert (np.load(os.path.join(dirs[0], "input_grad.npy")) == 1).all()


@pytest.mark.parametrize("steps,warmup", [(1, 0), (4, 2), (7, 0)])
def test_steps_sets_timed_step_calls(steps, warmup):
    import torch
    import torch.distributed as dist

    import bench

    mine = not dist.is_initialized()
    if mine:
        dist.init_process_group(
            "gloo", init_method=f"tcp://127.0.0.1:{free_port()}",
            rank=0, world_size=1)
    try:
        calls = []

        def step_fn():
            calls.append(len(calls))
            return {"call": calls[-1]}

        elapsed, outputs = bench.time_steps(
            step_fn, steps, warmup, torch.device("cpu"))
    finally:
        if mine:
            dist.destroy_process_group()
    assert len(calls) == warmup + steps
    # what is handed back is what the last timed call returned
    assert outputs == {"call": warmup + steps - 1}
    assert elapsed > 0


@pytest.mark.gpu
def test_full_adds_default_path_timing():
    rec = run_bench("--full")
    check_record(rec)
    assert rec["config"]["n1_default_path_ms"] > 0
    assert "n1_note" in rec["config"]
