"""AllgatherCompressed(wire="mxfp4"): the mxfp4 composite against a numpy
float64 oracle written from the format definition, the op at worlds 2 and 3
on gloo, autograd, the error checks and FSDP's param_compression="mxfp4".

Every comparison is exact (bytes), NaN by position.
"""

import copy

import numpy as np
import pytest
import torch

import mpi4torch_amd as m
from spmd import run_spmd
from test_compressed import _rand_input
from test_reducescatter_compressed import (oracle_reducescatter,
                                           _nan_aware_bytes_equal,
                                           _bytes_equal)
from test_allgather_compressed import (_same_on_all_ranks, _net, _data,
                                       _unit_flat, _capture_full_buffers)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


# ------------------------------ the oracle --------------------------------

def oracle_quantize(x):
    """flat tensor -> (payload [G*16] u8, scales [G] u8), in float64."""
    v = x.reshape(-1).to(torch.float64).numpy()
    G = -(-v.size // 32)
    xg = np.zeros(G * 32)
    xg[:v.size] = v
    xg = xg.reshape(G, 32)
    finite = np.isfinite(xg).all(1)
    xg[~finite] = 0.0
    amax = np.abs(xg).max(1)
    # the smallest integer E in [-127, 127] with amax * 2^-E <= 6, by search
    E = np.full(G, -127)
    while True:
        up = (amax * 2.0 ** -E > 6.0) & (E < 127)
        if not up.any():
            break
        E[up] += 1
    E[amax == 0] = 0
    y = xg * (2.0 ** -E)[:, None]
    # nearest grid point; of two equally near ones the code with low bit 0
    dist = np.abs(np.abs(y)[..., None] - GRID)
    lo = dist.argmin(-1)
    hi = 7 - dist[..., ::-1].argmin(-1)
    code = np.where(lo % 2 == 0, lo, hi)
    nib = (code | (np.signbit(y) << 3)).astype(np.uint8)
    nib[~finite] = 0
    pay = nib[:, 0::2] | (nib[:, 1::2] << 4)
    sc = np.where(finite, E + 127, 255).astype(np.uint8)
    return torch.from_numpy(pay.reshape(-1)), torch.from_numpy(sc)


def oracle_dequantize(pay, sc, dtype):
    """payload [G*16], scales [G] -> [G*32] of dtype."""
    p = pay.numpy().reshape(-1, 16)
    nib = np.stack([p & 15, p >> 4], -1).reshape(-1, 32)
    v = np.where(nib & 8, -GRID[nib & 7], GRID[nib & 7])
    s = sc.numpy().astype(np.int64)
    d = v * (2.0 ** np.clip(s - 127, -127, 127))[:, None]
    d[s == 255] = np.nan
    with np.errstate(over="ignore"):
        f32 = torch.from_numpy(d.astype(np.float32))    # exact, or +-inf
    return f32.reshape(-1).to(dtype)


def oracle_codec(x):
    """cast(dq(q(x))) of one rank's tensor, in its own shape."""
    xc = x.contiguous()
    d = oracle_dequantize(*oracle_quantize(xc), xc.dtype)
    return d[:xc.numel()].view(xc.shape)


def oracle_allgather(xs, axis):
    return torch.cat([oracle_codec(x) for x in xs], dim=axis)


def all_finite_values(dtype):
    """Every finite value of a 16-bit dtype, in groups of 32 whose first
    element is an anchor: 0 (the values set the scale themselves), 6 (E = 0:
    all 8 codes, every tie and both signed zeros occur), and two more."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = v[torch.isfinite(v)]
    v = torch.cat([v, v.new_zeros(-v.numel() % 31)]).view(-1, 31)
    return torch.cat([
        torch.cat([torch.full((v.shape[0], 1), a, dtype=dtype), v], 1)
        for a in (0.0, 6.0, 3.0 * 2.0 ** -10, 448.0)]).reshape(-1)


def scale_boundary_values():
    """Groups whose amax is m = 0.75 exactly (mantissa field 0x400000) or
    one of its two fp32 neighbours, at exponent fields from the subnormal
    range to the top; the other elements are fractions of it."""
    bits = [(e << 23) + 0x400000 + d
            for e in (0, 1, 2, 3, 100, 127, 128, 253, 254) for d in (-1, 0, 1)]
    amax = torch.tensor(bits, dtype=torch.int32).view(torch.float32)
    frac = torch.linspace(-1, 1, 32, dtype=torch.float32)
    return (amax[:, None] * frac[None, :]).reshape(-1)


def special_values():
    x = torch.linspace(-5, 5, 4 * 32).view(4, 32).clone()
    x[0] = 0.0                      # a zero group
    x[1, 3] = float("inf")
    x[2, 31] = float("nan")
    x[3, 0] = -0.0
    return x.reshape(-1)


def all_wire_bytes():
    """Every scale byte over every payload byte: 4096 groups."""
    pay = torch.arange(256, dtype=torch.uint8).repeat(256)
    sc = torch.arange(256, dtype=torch.uint8).repeat_interleave(16)
    return pay, sc


VALUE_SETS = {
    "bf16": lambda: all_finite_values(torch.bfloat16),
    "fp16": lambda: all_finite_values(torch.float16),
    "boundary": scale_boundary_values,
    "special": special_values,
}


@pytest.fixture(scope="module")
def C():
    return m._C


# ------------------------- composite vs the oracle ------------------------

@pytest.mark.parametrize("name", sorted(VALUE_SETS))
def test_quantize_values(C, name):
    x = VALUE_SETS[name]()
    pay, sc = C._mx4_quantize(x)
    opay, osc = oracle_quantize(x)
    assert torch.equal(sc, osc)
    assert torch.equal(pay, opay)
    if name == "bf16":
        g = pay.view(-1, 16)[x.view(-1, 32)[:, 0] == 6.0]
        nibs = torch.cat([g & 15, g >> 4]).unique()
        assert nibs.tolist() == list(range(16))      # all codes, both signs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_quantize_lengths(C, n, dtype):
    x = _rand_input(n, dtype, seed=n)
    pay, sc = C._mx4_quantize(x)
    assert pay.numel() == 16 * sc.numel() == 16 * ((n + 31) // 32)
    opay, osc = oracle_quantize(x)
    assert torch.equal(sc, osc) and torch.equal(pay, opay)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_all_bytes(C, dtype):
    pay, sc = all_wire_bytes()
    out = C._mx4_dequantize_blocks(pay, sc, 1, 1, 32 * sc.numel(), dtype)
    assert out.shape == (1, 1, 32 * sc.numel()) and out.dtype == dtype
    _nan_aware_bytes_equal(out.view(-1), oracle_dequantize(pay, sc, dtype))


# ------------------------------ SPMD worlds -------------------------------

def _spmd_worker(rank, world):
    comm = m.COMM_WORLD
    for shape, axis, dtype in [((4099,), 0, torch.float32),
                               ((3, 5, 7), 1, torch.bfloat16)]:
        n = int(np.prod(shape))
        xs = [_rand_input(n, dtype, seed=7 * n + r).view(shape)
              for r in range(world)]
        out = comm.AllgatherCompressed(xs[rank], axis, wire="mxfp4")
        _bytes_equal(out, oracle_allgather(xs, axis))
        assert _same_on_all_ranks(comm, out)
        # the default wire is untouched by the keyword
        _bytes_equal(comm.AllgatherCompressed(xs[rank], axis, wire="mxfp8"),
                     comm.AllgatherCompressed(xs[rank], axis))
        assert not torch.equal(out, comm.AllgatherCompressed(xs[rank], axis))

    # backward: ReducescatterCompressed (mxfp8) of the gradient
    ws = [_rand_input(3 * 40 * world, torch.float32, seed=90 + r)
          .view(3, 40 * world) for r in range(world)]
    x = _rand_input(120, torch.float32, seed=rank).view(3, 40).requires_grad_()
    (comm.AllgatherCompressed(x, 1, wire="mxfp4") * ws[rank]).sum().backward()
    _bytes_equal(x.grad, oracle_reducescatter(ws, 1, rank))

    with pytest.raises(RuntimeError,
                       match="equal counts.*Allgather handles variable"):
        comm.AllgatherCompressed(torch.ones(3, 5 + rank), 1, wire="mxfp4")
    with pytest.raises(ValueError, match="wire"):
        comm.AllgatherCompressed(torch.ones(3), 0, wire="mxfp6")


def _fsdp_worker(rank, world):
    from mpi4torch_amd.parallel import FullyShardedDataParallel

    comm = m.COMM_WORLD
    torch.manual_seed(3)
    base = _net()
    net = copy.deepcopy(base)
    holder = {}
    captured = _capture_full_buffers(net, holder)
    fsdp = FullyShardedDataParallel(net, param_compression="mxfp4",
                                    grad_compression="mxfp8")
    holder["fsdp"] = fsdp
    opt = torch.optim.SGD(fsdp.shard_parameters(), lr=0.05)
    for step in range(3):
        loss = (fsdp(_data(rank, step)) ** 2).sum()
        if step == 0:
            for u, bmod in zip(fsdp._units, [base[0], base[2]]):
                sl = u.shard_len
                orig = _unit_flat(list(bmod.parameters()), u.padded)
                # the master shard keeps full precision
                _bytes_equal(u.shard.detach(), orig[rank * sl:(rank + 1) * sl])
                full = captured[u.module]
                _bytes_equal(full, oracle_allgather(
                    [orig[r * sl:(r + 1) * sl] for r in range(world)], 0))
                assert _same_on_all_ranks(comm, full)
        fsdp.zero_grad()
        loss.backward()
        fsdp.finish_backward()
        assert all(bool(torch.isfinite(captured[u.module]).all())
                   and bool(torch.isfinite(u.shard.grad).all())
                   for u in fsdp._units)
        opt.step()
        fsdp.refresh_shards()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("worker", [_spmd_worker, _fsdp_worker])
def test_spmd(worker, world):
    run_spmd(world, worker)


# -------------------------------- world 1 ---------------------------------

def test_world1_changes_nothing():
    from mpi4torch_amd.parallel import FullyShardedDataParallel

    x = torch.randn(100)
    y = m.COMM_WORLD.AllgatherCompressed(x, wire="mxfp4")
    assert y.data_ptr() != x.data_ptr()
    _bytes_equal(y, x)
    with pytest.raises(ValueError, match="wire"):
        m.COMM_WORLD.AllgatherCompressed(x, 0, wire="fp4")
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        FullyShardedDataParallel(_net().double(), param_compression="mxfp4")
    torch.manual_seed(3)
    base = _net()
    outs = []
    for opt in ("mxfp4", None):
        model = FullyShardedDataParallel(copy.deepcopy(base),
                                         param_compression=opt)
        outs.append(model(_data(0)).detach())
    _bytes_equal(outs[0], outs[1])
