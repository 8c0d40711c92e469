"""AllgatherCompressed(wire="mxfp6-e2m3"): the mxfp6 composite against a numpy
float64 oracle written from the format definition, the op at worlds 2 and 3
on gloo, autograd, the error checks and FSDP's param_compression.

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
WIRE = "mxfp6-e2m3"
# sign<<5 | e<<3 | m, bias 1: m/8 for e = 0, (1 + m/8) * 2^(e-1) above
GRID = np.array([m_ / 8 if e == 0 else (1 + m_ / 8) * 2.0 ** (e - 1)
                 for e in range(4) for m_ in range(8)])


# ------------------------------ the oracle --------------------------------

def oracle_pack(codes):
    """codes [G, 32] -> payload [G*24]: code i in bits 6i..6i+5 of the group,
    bit 0 the LSB of byte 0."""
    bits = (codes[..., None] >> np.arange(6)) & 1
    return torch.from_numpy(np.packbits(
        bits.reshape(-1, 192).astype(np.uint8), axis=1,
        bitorder="little").reshape(-1))


def oracle_quantize(x):
    """flat tensor -> (payload [G*24] u8, scales [G] u8), in float64."""
    v = x.reshape(-1).to(torch.float64).numpy()
    G = -(-v.size // 32)
    xg = np.zeros(G * 32)
    xg[:v.size] = v
    xg = xg.reshape(G, 32)
    finite = np.isfinite(xg).all(1)
    xg[~finite] = 0.0
    amax = np.abs(xg).max(1)
    # the smallest integer E in [-127, 127] with amax * 2^-E <= 7.5, by search
    E = np.full(G, -127)
    while True:
        up = (amax * 2.0 ** -E > 7.5) & (E < 127)
        if not up.any():
            break
        E[up] += 1
    E[amax == 0] = 0
    y = xg * (2.0 ** -E)[:, None]
    # nearest grid point; of two equally near ones the even code
    dist = np.abs(np.abs(y)[..., None] - GRID)
    lo = dist.argmin(-1)
    hi = 31 - dist[..., ::-1].argmin(-1)
    code = np.where(lo % 2 == 0, lo, hi) | (np.signbit(y) << 5)
    code[~finite] = 0
    sc = np.where(finite, E + 127, 255).astype(np.uint8)
    return oracle_pack(code), torch.from_numpy(sc)


def oracle_dequantize(pay, sc, dtype):
    """payload [G*24], scales [G] -> [G*32] of dtype."""
    bits = np.unpackbits(pay.numpy().reshape(-1, 24), axis=1,
                         bitorder="little").reshape(-1, 32, 6)
    code = (bits << np.arange(6)).sum(-1)
    v = np.where(code & 32, -GRID[code & 31], GRID[code & 31])
    s = sc.numpy().astype(np.int64)
    d = v * (2.0 ** np.clip(s - 127, -127, 127))[:, None]
    d[s == 255] = np.nan
    with np.errstate(over="ignore"):
        f32 = torch.from_numpy(d.astype(np.float32))    # exact, or +-inf
    return f32.reshape(-1).to(dtype)


def composite_codec(x):
    """cast(dq(q(x))) of one rank's tensor by the composite, in its shape."""
    xc = x.contiguous()
    d = m._C._mx6_dequantize_blocks(*m._C._mx6_quantize(xc), 1, 1, xc.numel(),
                                    xc.dtype)
    return d.view(xc.shape)


def all_finite_values(dtype):
    """Every finite value of a 16-bit dtype, in groups of 32 whose first
    element is an anchor: 0 (the values set the scale themselves), 7.5
    (E = 0: all 64 codes occur), and two more."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = v[torch.isfinite(v)]
    v = torch.cat([v, v.new_zeros(-v.numel() % 31)]).view(-1, 31)
    return torch.cat([
        torch.cat([torch.full((v.shape[0], 1), a, dtype=dtype), v], 1)
        for a in (0.0, 7.5, 3.0 * 2.0 ** -10, 448.0)]).reshape(-1)


def tie_values():
    """Under an anchor of 7.5 (E = 0): each of the 31 midpoints between two
    neighbouring grid values and its two fp32 neighbours, in both signs."""
    mid = torch.from_numpy((GRID[:-1] + GRID[1:]) / 2).float()
    bits = mid.view(torch.int32)
    v = torch.stack([bits - 1, bits, bits + 1]).view(torch.float32).view(-1)
    v = torch.cat([v, -v, v.new_zeros(-2 * v.numel() % 31)]).view(-1, 31)
    return torch.cat([torch.full((v.shape[0], 1), 7.5), v], 1).reshape(-1)


def scale_boundary_values():
    """Groups whose amax is m = 0.9375 exactly (mantissa field 0x700000) or
    one of its two fp32 neighbours, at exponent fields from the subnormal
    range to the top; the other elements are fractions of it."""
    bits = [(e << 23) + 0x700000 + d
            for e in (0, 1, 2, 3, 100, 127, 128, 253, 254) for d in (-1, 0, 1)]
    amax = torch.tensor(bits, dtype=torch.int32).view(torch.float32)
    frac = torch.linspace(-1, 1, 32, dtype=torch.float32)
    return (amax[:, None] * frac[None, :]).reshape(-1)


def special_values():
    x = torch.linspace(-7, 7, 5 * 32).view(5, 32).clone()
    x[0] = 0.0                      # a zero group
    x[1, 3] = float("inf")
    x[2, 31] = float("nan")
    x[3, 0] = -0.0
    x[4, 5], x[4, 6] = -0.01, 0.01  # rounds to zero, the sign kept
    return x.reshape(-1)


def all_wire_codes():
    """Every code at every position under every scale byte: group s of 64
    holds code (i + s) % 64 at position i; 256 * 64 groups."""
    codes = (np.arange(32)[None, :] + np.arange(64)[:, None]) % 64
    pay = oracle_pack(codes).repeat(256)
    sc = torch.arange(256, dtype=torch.uint8).repeat_interleave(64)
    return pay, sc


VALUE_SETS = {
    "bf16": lambda: all_finite_values(torch.bfloat16),
    "fp16": lambda: all_finite_values(torch.float16),
    "ties": tie_values,
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
    pay, sc = C._mx6_quantize(x)
    opay, osc = oracle_quantize(x)
    assert torch.equal(sc, osc)
    assert torch.equal(pay, opay)
    if name == "special":
        assert sc[1:3].tolist() == [255, 255] and not pay[24:72].any()
        d = oracle_dequantize(pay, sc, torch.float32)[4 * 32 + 5:4 * 32 + 7]
        assert d.tolist() == [0.0, 0.0]
        assert torch.signbit(d).tolist() == [True, False]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 16, 31, 32, 33])
def test_quantize_lengths(C, n, dtype):
    x = _rand_input(n, dtype, seed=n)
    pay, sc = C._mx6_quantize(x)
    assert pay.numel() == 24 * sc.numel() == 24 * ((n + 31) // 32)
    opay, osc = oracle_quantize(x)
    assert torch.equal(sc, osc) and torch.equal(pay, opay)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_all_codes(C, dtype):
    pay, sc = all_wire_codes()
    out = C._mx6_dequantize_blocks(pay, sc, 1, 1, 32 * sc.numel(), dtype)
    assert out.shape == (1, 1, 32 * sc.numel()) and out.dtype == dtype
    _nan_aware_bytes_equal(out.view(-1), oracle_dequantize(pay, sc, dtype))


def test_error_between_the_siblings(C):
    """Relative RMS error on a fixed N(0,1) bf16 tensor: mxfp6 lies strictly
    below mxfp4 (an ordering, not a threshold)."""
    x = torch.randn(65536 * 32,
                    generator=torch.Generator().manual_seed(0)).bfloat16()
    n, ref = x.numel(), x.double()
    err = {w: float(((dq(*q(x), 1, 1, n, x.dtype).view(-1).double() - ref)
                     .norm() / ref.norm()))
           for w, q, dq in (("mx6", C._mx6_quantize, C._mx6_dequantize_blocks),
                            ("mx4", C._mx4_quantize, C._mx4_dequantize_blocks))}
    print("relative RMS error", err)
    assert err["mx6"] < err["mx4"]


# ------------------------------ SPMD worlds -------------------------------

def _spmd_worker(rank, world):
    comm = m.COMM_WORLD
    for shape, axis, dtype in [((4099,), 0, torch.float32),
                               ((3, 5, 7), 1, torch.bfloat16)]:
        n = int(np.prod(shape))
        xs = [_rand_input(n, dtype, seed=7 * n + r).view(shape)
              for r in range(world)]
        out = comm.AllgatherCompressed(xs[rank], axis, wire=WIRE)
        _bytes_equal(out, torch.cat([composite_codec(x) for x in xs], axis))
        assert _same_on_all_ranks(comm, out)
        for other in ("mxfp8", "mxfp4"):
            assert not torch.equal(
                out, comm.AllgatherCompressed(xs[rank], axis, wire=other))

    # backward: ReducescatterCompressed (mxfp8) of the gradient
    ws = [_rand_input(3 * 40 * world, torch.float32, seed=90 + r)
          .view(3, 40 * world) for r in range(world)]
    x = _rand_input(120, torch.float32, seed=rank).view(3, 40).requires_grad_()
    (comm.AllgatherCompressed(x, 1, wire=WIRE) * ws[rank]).sum().backward()
    _bytes_equal(x.grad, oracle_reducescatter(ws, 1, rank))

    with pytest.raises(RuntimeError,
                       match="equal counts.*Allgather handles variable"):
        comm.AllgatherCompressed(torch.ones(3, 5 + rank), 1, wire=WIRE)
    for refused in ("mxfp6", "fp6"):
        with pytest.raises(ValueError, match="wire.*mxfp8.*mxfp6-e2m3.*mxfp4"):
            comm.AllgatherCompressed(torch.ones(3), 0, wire=refused)


def _fsdp_worker(rank, world):
    from mpi4torch_amd.parallel import FullyShardedDataParallel

    comm = m.COMM_WORLD
    torch.manual_seed(3)
    base = _net()
    net = copy.deepcopy(base)
    holder = {}
    captured = _capture_full_buffers(net, holder)
    fsdp = FullyShardedDataParallel(net, param_compression=WIRE)
    holder["fsdp"] = fsdp
    opt = torch.optim.SGD(fsdp.shard_parameters(), lr=0.05)
    loss = (fsdp(_data(rank, 0)) ** 2).sum()
    for u, bmod in zip(fsdp._units, [base[0], base[2]]):
        sl = u.shard_len
        orig = _unit_flat(list(bmod.parameters()), u.padded)
        # the master shard keeps full precision
        _bytes_equal(u.shard.detach(), orig[rank * sl:(rank + 1) * sl])
        full = captured[u.module]
        _bytes_equal(full, torch.cat(
            [composite_codec(orig[r * sl:(r + 1) * sl])
             for r in range(world)]))
        assert _same_on_all_ranks(comm, full)
    fsdp.zero_grad()
    loss.backward()
    fsdp.finish_backward()
    assert all(bool(torch.isfinite(u.shard.grad).all()) for u in fsdp._units)
    opt.step()
    fsdp.refresh_shards()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("worker", [_spmd_worker, _fsdp_worker])
def test_spmd(worker, world):
    run_spmd(world, worker)


# -------------------------------- world 1 ---------------------------------

def test_world1_changes_nothing():
    from mpi4torch_amd.parallel import FullyShardedDataParallel
    from mpi4torch_amd.utils import mxfp6_allgather_wire_bytes, trace

    x = torch.randn(100)
    for comm in (m.COMM_WORLD, trace(m.COMM_WORLD)):
        y = comm.AllgatherCompressed(x, 0, wire=WIRE)
        assert y.data_ptr() != x.data_ptr()
        _bytes_equal(y, x)
    with pytest.raises(ValueError, match="wire"):
        trace(m.COMM_WORLD).AllgatherCompressed(x, 0, "mxfp6")
    assert mxfp6_allgather_wire_bytes(33, 3) == 2 * 25 * 2
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        FullyShardedDataParallel(_net().double(), param_compression=WIRE)
    for refused in ({"param_compression": "mxfp6"},
                    {"grad_compression": WIRE}):
        with pytest.raises(ValueError, match="compression must be"):
            FullyShardedDataParallel(_net(), **refused)
