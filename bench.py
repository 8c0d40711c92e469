#!/usr/bin/env python3
"""Flagship benchmark: autograd-transparent Allreduce fwd+bwd on a 1 GiB
bf16 tensor per GPU (BASELINE.json config #2 — the headline metric:
"Allreduce algbw GB/s + grad-step wallclock, 1GiB bf16 tensor").

One step = forward Allreduce(SUM) of the 1 GiB tensor + backward through
its autograd node (the adjoint Allreduce of a 1 GiB gradient) — i.e. the
full autodiff-transparent round trip, 2 GiB of collective payload per GPU
per step. The reported value is the WHOLE-JOB algorithmic bandwidth:
  value = n_gpus * 2 * bytes / t_step      [GB/s, higher is better]
`vs_baseline` is null: the reference publishes no numbers.

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W          # single GPU
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N ...      # N ranks, RCCL

Other BASELINE configs are reachable with --config {allreduce,linreg,
ring,alltoall} for self-measurement; the driver uses the default.

A plain run sets up, warms up, times the steps and prints the JSON line.
--full adds the secondary measurements (today: the N=1 default-path
timing recorded next to the headline). --dump-outputs DIR writes what the
last timed step returned to its caller as DIR/<name>.npy; inputs are
seeded, so two builds can be compared output for output.
"""

import argparse
import json
import os
import time

import torch

SEED = 20240229
# --dump-outputs: arrays above this many elements are written as a fixed
# seeded sample (4 Mi float32 = 16 MiB each; every config returns at most
# three arrays, so a dump stays under 64 MB)
DUMP_MAX_ELEMS = 1 << 22
DUMP_MAX_BYTES = 64 * 1000 * 1000


def setup_world(args):
    # Time REAL communication even at N=1: force_full_path disables the
    # world-1 local fast paths so the timed region contains an actual
    # ncclAllReduce / grouped RCCL exchange (cost parity with the local
    # slab-kernel path was measured in profiles/microbench_final.txt;
    # rocprof on this bench shows the RCCL kernels). Set before the
    # extension reads its config.
    os.environ.setdefault("MPI4TORCH_AMD_FORCE_FULL_PATH", "1")
    if "WORLD_SIZE" not in os.environ:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = os.environ.get("MASTER_PORT", "29400")
        os.environ["RANK"] = "0"
        os.environ["WORLD_SIZE"] = "1"
        os.environ["LOCAL_RANK"] = "0"
    import torch.distributed as dist

    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")
    import mpi4torch_amd as m4a

    m4a.init()
    return m4a, rank, world, device


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def time_steps(step_fn, steps, warmup, device):
    """Wall time of `steps` calls of step_fn, each run to completion.

    Every step ends in a device synchronize. The collectives run on side
    streams and mark their buffers with recordStream, so the caching
    allocator cannot reuse a step's tensors before the device has finished
    it. A host that queues steps without waiting therefore takes fresh
    device memory for every queued step, and ms_per_step then measures
    allocation and depends on --steps. With the synchronize the working
    set is fixed after warm-up and ms_per_step does not depend on the
    number of steps (measurements: profiles/bench_steps_stability.md).
    """
    import torch.distributed as dist

    for _ in range(warmup):
        step_fn()
        sync(device)
    dist.barrier()
    sync(device)
    t0 = time.perf_counter()
    # only the last step's return value is kept, so the steps before it
    # free their results exactly as a caller that drops them would
    for _ in range(steps - 1):
        step_fn()
        sync(device)
    outputs = step_fn()
    sync(device)
    elapsed = time.perf_counter() - t0
    dist.barrier()
    # MAX over ranks
    t = torch.tensor([elapsed], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item()), outputs


def dump_outputs(outputs, out_dir):
    """Write each tensor of `outputs` as <out_dir>/<name>.npy (float32, or
    float64 for double tensors). Large tensors are reduced to the same
    seeded sample of flat indices in every run."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, x in outputs.items():
        x = x.detach().reshape(-1)
        if x.numel() > DUMP_MAX_ELEMS:
            g = torch.Generator().manual_seed(SEED)
            idx = torch.randint(0, x.numel(), (DUMP_MAX_ELEMS,), generator=g)
            idx = idx.sort().values.to(x.device)
            if x.element_size() == 1:  # fp8: gather the raw bytes
                x = x.view(torch.uint8)[idx].view(x.dtype)
            else:
                x = x[idx]
        x = x.to(torch.float64 if x.dtype == torch.float64 else torch.float32)
        a = x.cpu().numpy()
        total += a.nbytes
        assert total <= DUMP_MAX_BYTES, "dump exceeds 64 MB"
        np.save(os.path.join(out_dir, name + ".npy"), a)


def bench_allreduce(m4a, comm, device, args):
    n_elems = int(args.size_mib * 1024 * 1024 // 2)  # bf16 = 2 bytes
    dtype = torch.bfloat16 if device.type == "cuda" else torch.bfloat16
    t = torch.randn(n_elems, dtype=torch.float32, device=device).to(dtype)
    t.requires_grad_()
    grad_seed = torch.ones(n_elems, dtype=dtype, device=device)

    def step():
        t.grad = None
        r = comm.Allreduce(t, m4a.MPI_SUM)
        r.backward(grad_seed)
        return {"allreduce_out": r, "input_grad": t.grad}

    elapsed, outputs = time_steps(step, args.steps, args.warmup, device)
    t_step = elapsed / args.steps

    config = {
        "model": "allreduce_1GiB_bf16_fwd_bwd",
        "tensor_mib": args.size_mib,
        "global_batch": None,
        "seq_len": None,
        "parallelism": f"dp{comm.size}",
    }
    if args.full and comm.size == 1 and device.type == "cuda":
        # The timed region holds a REAL ncclAllReduce (force_full_path);
        # at nranks=1 RCCL implements it as an internal copy whose speed
        # varies wildly across boxes (profiles/rccl_1rank_box_variance.md:
        # 1.15-9.2 ms/GiB measured for identical code). Record the
        # framework's DEFAULT world-1 path alongside so the record is
        # self-explanatory; the N>1 numbers are the real communication.
        m4a = __import__("mpi4torch_amd")
        m4a._C.force_full_path(False)
        try:
            fp_elapsed, _ = time_steps(step, 5, 2, device)
            config["n1_default_path_ms"] = round(fp_elapsed / 5 * 1e3, 3)
            config["n1_note"] = (
                "value times RCCL's nranks=1 internal copy "
                "(box-variable; see profiles/rccl_1rank_box_variance.md); "
                "n1_default_path_ms is the framework's default world-1 "
                "path on the same box")
        finally:
            m4a._C.force_full_path(True)

    nbytes = n_elems * 2
    return {
        "metric": "allreduce_fwdbwd_algbw_GBps",
        "value": comm.size * 2 * nbytes / t_step / 1e9,
        "unit": "GB/s",
        "config": config,
    }, t_step, outputs


def bench_linreg(m4a, comm, device, args):
    # BASELINE config #3: data-parallel linear regression, per-rank local
    # loss + allreduce (reference examples/simple_linear_regression.py)
    from mpi4torch_amd.models.linreg import DistributedLinReg

    n, f = 1 << 20, 32
    model = DistributedLinReg(comm, n_features=f).to(device)
    x = torch.randn(n, f, device=device)
    y = torch.randn(n, device=device)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        loss = model.loss(x, y)
        loss.backward()
        opt.step()
        out = {"loss": loss}
        for i, p in enumerate(model.parameters()):
            out[f"param{i}"] = p
        return out

    elapsed, outputs = time_steps(step, args.steps, args.warmup, device)
    t_step = elapsed / args.steps
    return {
        "metric": "linreg_steps_per_s",
        "value": comm.size * args.steps / elapsed,
        "unit": "steps/s*gpus",
        "config": {
            "model": "dp_linreg",
            "global_batch": n * comm.size,
            "seq_len": None,
            "parallelism": f"dp{comm.size}",
        },
    }, t_step, outputs


def bench_ring(m4a, comm, device, args):
    # BASELINE config #4: 256 MiB ring exchange with autograd WaitHandles
    n = 256 * 1024 * 1024 // 4  # fp32
    t = torch.randn(n, device=device).requires_grad_()
    grad_seed = torch.ones(n, device=device)
    rank, world = comm.rank, comm.size

    def step():
        t.grad = None
        req = comm.Isend(t, (rank + 1) % world, 0)
        req2 = comm.Irecv(
            m4a.JoinDummies(torch.empty_like(t), [req.dummy]),
            (rank + world - 1) % world,
            0,
        )
        res = comm.Wait(m4a.JoinDummiesHandle(req, [req2.dummy]))
        res2 = comm.Wait(m4a.JoinDummiesHandle(req2, [res]))
        res2.backward(grad_seed)
        return {"ring_out": res2, "input_grad": t.grad}

    elapsed, outputs = time_steps(step, args.steps, args.warmup, device)
    t_step = elapsed / args.steps
    nbytes = n * 4
    return {
        "metric": "ring_exchange_fwdbwd_GBps",
        "value": comm.size * 2 * nbytes / t_step / 1e9,
        "unit": "GB/s",
        "config": {
            "model": "ring_256MiB_fp32_fwd_bwd",
            "global_batch": None,
            "seq_len": None,
            "parallelism": f"ring{comm.size}",
        },
    }, t_step, outputs


def bench_alltoall(m4a, comm, device, args):
    # BASELINE config #5: 4096x4096 fp8 shards, expert-parallel pattern
    world = comm.size
    rows = 4096 * world
    t32 = torch.randn(rows, 4096, device=device)
    dtype = torch.float8_e4m3fn if device.type == "cuda" else torch.float8_e4m3fn
    t = t32.to(dtype).requires_grad_()
    grad_seed = torch.ones(4096, 4096 * world, device=device).to(dtype)

    # EP pattern: every rank knows the routing table, so use the
    # explicit-counts form — no host count exchanges in the timed loop
    counts = [4096] * world

    def step():
        t.grad = None
        r = comm.Alltoallv(t, 1, 0, counts, counts)
        r.backward(grad_seed)
        return {"alltoall_out": r, "input_grad": t.grad}

    elapsed, outputs = time_steps(step, args.steps, args.warmup, device)
    t_step = elapsed / args.steps
    nbytes = rows * 4096
    return {
        "metric": "alltoall_fp8_fwdbwd_GBps",
        "value": comm.size * 2 * nbytes / t_step / 1e9,
        "unit": "GB/s",
        "config": {
            "model": "alltoall_4096x4096_fp8",
            "global_batch": None,
            "seq_len": None,
            "parallelism": f"ep{comm.size}",
        },
    }, t_step, outputs


BENCHES = {
    "allreduce": bench_allreduce,
    "linreg": bench_linreg,
    "ring": bench_ring,
    "alltoall": bench_alltoall,
}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--config", default="allreduce", choices=sorted(BENCHES))
    p.add_argument("--size-mib", type=float, default=1024.0,
                   help="allreduce tensor size per GPU (MiB)")
    p.add_argument("--all-configs", action="store_true",
                   help="run every BASELINE config; write all JSON records "
                        "to gpurun_out/bench_all.jsonl, print the headline "
                        "(allreduce) line last")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (N=1 "
                        "default-path timing next to the headline)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the arrays the last timed step returned as "
                        "DIR/<name>.npy (seeded sample of large ones)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    m4a, rank, world, device = setup_world(args)
    comm = m4a.COMM_WORLD
    assert comm.size == world

    def run_config(name):
        # every config starts from the same seed, so its inputs are the
        # same in every run with the same arguments, --all-configs or not
        torch.manual_seed(SEED + rank)
        return BENCHES[name](m4a, comm, device, args)

    extra_records = []
    if args.all_configs:
        for name in ("linreg", "ring", "alltoall"):
            r, ts, _ = run_config(name)
            r["ms_per_step"] = round(ts * 1e3, 3)
            extra_records.append(r)
        args.config = "allreduce"
    result, t_step, outputs = run_config(args.config)
    if args.dump_outputs and rank == 0:
        dump_outputs(outputs, args.dump_outputs)
    # RCCL's version banner is written through C stdio, which is fully
    # buffered on a pipe and flushes at exit — AFTER our JSON. Flush it now
    # so the JSON line is the last thing on stdout.
    try:
        import ctypes

        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    if rank == 0:
        out = {
            "metric": result["metric"],
            "value": round(result["value"], 3),
            "unit": result["unit"],
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(t_step * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # the reference publishes no numbers
            "dtype": "bf16" if args.config == "allreduce" else
                     ("fp8" if args.config == "alltoall" else "fp32"),
            "data": "synthetic",
            "config": result["config"],
        }
        if extra_records:
            # --all-configs: persist every config's record (headline
            # included) for the profiles/ archive; stdout still carries
            # exactly ONE JSON line (the driver's contract)
            os.makedirs("gpurun_out", exist_ok=True)
            with open("gpurun_out/bench_all.jsonl", "w") as f:
                for r in extra_records:
                    f.write(json.dumps({**r, "n_gpus": world}) + "\n")
                f.write(json.dumps(out) + "\n")
        print(json.dumps(out), flush=True)

    import torch.distributed as dist

    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
