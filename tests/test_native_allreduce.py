"""native_allreduce geometry on the CPU transport (worlds 2, 5, 7).

MPI4TORCH_AMD_ALLREDUCE=native sends bf16/fp16/fp32 arithmetic Allreduce
through the two-shot engine on gloo too: block exchange without a self pair
(P-1 staging slots), local reduce of own block + staged copies, allgather of
the reduced blocks. The CPU local reduce has the kernel's semantics (fp32
accumulation in rank order, one rounding to the tensor dtype), so the result
must equal, bit for bit, a reference built from an Allgather of the inputs.

MIN/MAX follow fminf/fmaxf on the GPU (as the fp8 reduce kernel does), which
differ from torch.minimum/maximum only on NaN: inputs here are NaN-free.
"""

import torch

from spmd import run_spmd

DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _reference(comm, x, opname):
    """fp32 rank-order accumulation of every rank's x, one cast at the end."""
    world = comm.size
    allx = comm.Allgather(x.float().reshape(1, -1), 0)
    acc = allx[0]
    for r in range(1, world):
        if opname == "sum":
            acc = acc + allx[r]
        elif opname == "prod":
            acc = acc * allx[r]
        elif opname == "min":
            acc = torch.minimum(acc, allx[r])
        else:
            acc = torch.maximum(acc, allx[r])
    return acc.to(x.dtype)


def _native_worker(rank, world):
    import os

    os.environ["MPI4TORCH_AMD_ALLREDUCE"] = "native"
    import mpi4torch_amd as m

    m._C.reload_config()
    comm = m.COMM_WORLD
    ops = (("sum", m.MPI_SUM), ("prod", m.MPI_PROD), ("min", m.MPI_MIN),
           ("max", m.MPI_MAX))
    gen = torch.Generator().manual_seed(1234 + rank)
    for n in (1, world - 1, 4 * world, 4 * world + 3, 16 * world + 5):
        for dtype in DTYPES:
            for opname, op in ops:
                x = torch.randn(n, generator=gen)
                if opname == "prod":
                    x = 1.0 + 0.25 * x  # keep the product in range
                else:
                    x = x * (rank + 1)
                x = x.to(dtype)
                want = _reference(comm, x, opname)
                got = comm.Allreduce(x, op)
                assert got.dtype == dtype and got.shape == x.shape
                assert torch.equal(_bits(got), _bits(want)), (n, dtype, opname)

    # autograd: the adjoint of the sum-allreduce is the sum-allreduce of the
    # incoming gradients, through the same engine
    for n in (4 * world + 3, 16 * world + 5):
        for dtype in DTYPES:
            x = torch.randn(n, generator=gen).to(dtype).requires_grad_()
            g = (torch.randn(n, generator=gen) * (rank + 1)).to(dtype)
            y = comm.Allreduce(x, m.MPI_SUM)
            y.backward(g)
            want = _reference(comm, g, "sum")
            assert torch.equal(_bits(x.grad), _bits(want)), (n, dtype)

    # 2-d input keeps its shape; dtypes outside the engine still reduce
    x2 = (torch.randn(3, 2 * world + 1, generator=gen)).to(torch.bfloat16)
    got2 = comm.Allreduce(x2, m.MPI_SUM)
    assert got2.shape == x2.shape
    assert torch.equal(_bits(got2.reshape(-1)),
                       _bits(_reference(comm, x2.reshape(-1), "sum")))
    ti = torch.arange(5, dtype=torch.int64) + rank
    assert (comm.Allreduce(ti, m.MPI_SUM)
            == world * torch.arange(5) + world * (world - 1) // 2).all()


def test_native_allreduce_ws2():
    run_spmd(2, _native_worker)


def test_native_allreduce_ws5():
    run_spmd(5, _native_worker)


def test_native_allreduce_ws7():
    run_spmd(7, _native_worker)


def _knob_worker(rank, world):
    import os

    import mpi4torch_amd as m

    comm = m.COMM_WORLD
    x = (torch.arange(40, dtype=torch.float32) * (rank + 1)).to(torch.bfloat16)
    outs = []
    for mode in ("auto", "native", "rccl"):
        os.environ["MPI4TORCH_AMD_ALLREDUCE"] = mode
        m._C.reload_config()
        outs.append(comm.Allreduce(x, m.MPI_MAX))
    want = (torch.arange(40, dtype=torch.float32) * world).to(torch.bfloat16)
    for o in outs:
        assert torch.equal(o, want)
    os.environ["MPI4TORCH_AMD_ALLREDUCE"] = "bogus"
    try:
        m._C.reload_config()
    except RuntimeError as e:
        assert "MPI4TORCH_AMD_ALLREDUCE" in str(e)
    else:
        raise AssertionError("bad MPI4TORCH_AMD_ALLREDUCE value accepted")
    finally:
        os.environ["MPI4TORCH_AMD_ALLREDUCE"] = "auto"
        m._C.reload_config()


def test_allreduce_engine_knob_ws2():
    run_spmd(2, _knob_worker)
