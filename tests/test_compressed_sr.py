"""Stochastic rounding on the mxfp8 gradient reductions: the composite against
an oracle written from the rule in float64 and numpy integers (it does not
call the extension; the scale byte is the round-to-nearest oracle's),
unbiasedness with derived bounds, the ops on gloo worlds against the chain of
debug ops, rejections, one DDP step.
"""

import copy
import os

import numpy as np
import pytest
import torch

import mpi4torch_amd as m  # module-level so TorchScript resolves m.MPI_Communicator
from spmd import run_spmd
from test_compressed import (DTYPES, _Net, _bytes_equal, _ddp_data, _groups,
                             _rand_input, _with_specials, oracle_quantize)

C = m._C
SEEDS = [0, 2 ** 40 + 3]
N0S = [0, 2 ** 33 - 64]   # the second makes the pair index cross 2^32


def oracle_key(seed, stream, rank):
    M = 2 ** 64 - 1

    def mix(z):
        z = (z + 0x9e3779b97f4a7c15) & M
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
        return z ^ (z >> 31)

    z = mix(mix(mix(seed & M) ^ stream) ^ rank)
    return z & 0xffffffff, z >> 32


def oracle_bits(key, n0, count):
    def h(x):
        x = x ^ (x >> 16)
        x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> 15)
        x = x * np.uint32(0x846ca68b)
        return x ^ (x >> 16)

    n = np.arange(count, dtype=np.uint64) + np.uint64(n0)
    j = n >> np.uint64(1)
    lo = (j & np.uint64(0xffffffff)).astype(np.uint32)
    hi = (j >> np.uint64(32)).astype(np.uint32)
    w = h((h(lo ^ np.uint32(key[0])) + hi) ^ np.uint32(key[1]))
    r = np.where((n & np.uint64(1)) != 0, w >> 16, w & np.uint32(0xffff))
    return torch.from_numpy(r.astype(np.int64))


def oracle_quantize_sr(x, seed, stream, rank, n0):
    """flat x -> (payload, scales, finite [G, 1], y [G, 32] float64, ulp)"""
    sc = oracle_quantize(x)[1]
    finite = (sc != 255).unsqueeze(1)
    E = torch.where(finite, sc.int().unsqueeze(1) - 127, 0)
    y = torch.ldexp(torch.where(finite, _groups(x), 0.0), -E).double()
    e = torch.where(y == 0, -6, (torch.frexp(y)[1] - 1).clamp_min(-6))
    ulp = torch.ldexp(torch.ones((), dtype=torch.float64), e - 3)
    t = y.abs() / ulp
    r = oracle_bits(oracle_key(seed, stream, rank), n0, y.numel()).view_as(y)
    up = t - t.floor() >= (65536 - r).double() / 65536
    q = torch.copysign((t.floor() + up) * ulp, y).float()
    pay = q.to(torch.float8_e4m3fn).view(torch.uint8)
    return torch.where(finite, pay, 0).reshape(-1), sc, finite, y, ulp


def _inputs(n, dtype):
    xs = [_with_specials(_rand_input(n, dtype, seed=n, scale=s))
          for s in (1.0, 3e4)]
    # the clamped E = -127 region; fp16 cannot hold it and keeps the fp32 one
    tiny = _rand_input(n, torch.float32, seed=n + 1, scale=4e-38)
    xs.append(tiny if dtype == torch.float16 else tiny.to(dtype))
    x = _rand_input(n, dtype, seed=n + 2)
    if n >= 192:
        x[35], x[160] = -0.0, float("nan")   # the NaN in a group of its own
    return xs + [x]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n0", N0S)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [1, 33, 4099])
def test_composite_matches_oracle_and_rounds_to_a_neighbour(n, seed, n0, dtype):
    for x in _inputs(n, dtype):
        p, s = C._mx8_quantize_sr(x, seed, 1, 3, n0)
        po, so, finite, y, ulp = oracle_quantize_sr(x, seed, 1, 3, n0)
        _bytes_equal(s, so)
        _bytes_equal(p, po)
        q = p.view(torch.float8_e4m3fn).double().view_as(y)
        ok = finite.expand_as(y)
        assert bool(((q - y).abs() < ulp)[ok].all())
        assert bool((q.abs() <= 448)[ok].all())
        assert torch.equal(torch.signbit(q)[ok], torch.signbit(y)[ok])
        assert not bool(p.view_as(y)[~ok].any())   # a 255 group is zeros


# ------------------------------ unbiasedness -------------------------------

K = 256


def _quarter_ulp_input():
    """4096 fp32 elements (fl + 0.25) * ulp on the E = 0 grid: element 0 of
    every group lies in [256, 448), the others run over all binades and the
    subnormals. Returns (x, ulp)."""
    i = torch.arange(4096).view(128, 32)
    e = i % 14 - 6
    fl = torch.where(e == -6, i // 14 % 16, 8 + i // 14 % 8)
    e[:, 0], fl[:, 0] = 8, 8 + torch.arange(128) % 5
    ulp = torch.ldexp(torch.ones(()), e - 3)
    sign = 1 - i // 7 % 2 * 2
    return (sign * (fl + 0.25) * ulp).reshape(-1), ulp.reshape(-1)


def _check_unbiased(x, ulp, quantize_k):
    """z = (mean_k dq(q_k) - x) / ulp. One draw's error has variance at most
    1/4 ulp^2 and a bias of at most 2^-16 ulp, hence six-sigma bounds."""
    acc = torch.zeros(x.numel(), dtype=torch.float64)
    for k in range(K):
        p, s = quantize_k(k)
        assert int(s.min()) == 127 and int(s.max()) == 127
        acc += C._mx8_dequantize(p, s, x.numel(), torch.float32).double()
    z = (acc / K - x.double()) / ulp.double() * torch.sign(x).double()
    print("mean z", float(z.mean()), "max |z|", float(z.abs().max()))
    assert abs(float(z.mean())) <= 6 * 0.5 / (K * 4096) ** 0.5 + 2.0 ** -16
    assert float(z.abs().max()) <= 6 * 0.5 / K ** 0.5 + 2.0 ** -16


def test_quantize_is_unbiased_where_round_to_nearest_is_not():
    x, ulp = _quarter_ulp_input()
    p, s = C._mx8_quantize(x)
    z = (C._mx8_dequantize(p, s, 4096, torch.float32) - x) / ulp
    assert torch.equal(z * torch.sign(x), torch.full((4096,), -0.25))
    _check_unbiased(x, ulp, lambda k: C._mx8_quantize_sr(x, k, 0, 0, 0))


def test_reduce_is_unbiased_at_p4():
    x, ulp = _quarter_ulp_input()
    whole = torch.sign(x) * (x.abs() / ulp).floor() * ulp
    qs = [C._mx8_quantize(c) for c in
          (whole, x - whole, torch.zeros(4096), torch.zeros(4096))]
    pay, sc = (torch.stack([q[i] for q in qs]) for i in (0, 1))
    total = sum(C._mx8_dequantize(p, s, 4096, torch.float32) for p, s in qs)
    assert torch.equal(total, x)  # the four copies sum to x exactly
    _check_unbiased(x, ulp, lambda k: C._mx8_reduce_sr(pay, sc, k, 1, 0, 0))


# ------------------------------ gloo worlds --------------------------------

def _rank_input(r, n, dtype, salt=0):
    return _with_specials(_rand_input(n, dtype, seed=100 * salt + r + 1))


def _allreduce_chain(xs, seed, stream0):
    qs = [C._mx8_quantize_sr(x, seed, stream0, r, 0) for r, x in enumerate(xs)]
    p, s = C._mx8_reduce_sr(torch.stack([q[0] for q in qs]),
                            torch.stack([q[1] for q in qs]), seed,
                            stream0 + 1, 0, 0)
    return C._mx8_dequantize(p, s, xs[0].numel(), xs[0].dtype)


def _ops_worker(rank, world):
    comm = m.COMM_WORLD
    seed, n = 2 ** 40 + 3, 4099
    for dtype in (torch.float32, torch.bfloat16):
        xs = [_rank_input(r, n, dtype) for r in range(world)]
        x = xs[rank].clone().requires_grad_()
        out = comm.AllreduceCompressed(x, seed=seed)
        # the chain is the same computation on every rank, so equality with
        # it is also identity across ranks
        _bytes_equal(out.detach(), _allreduce_chain(xs, seed, 0))
        assert not torch.equal(
            torch.nan_to_num(out.detach()),
            torch.nan_to_num(comm.AllreduceCompressed(xs[rank])))
        # another split of the groups over the ranks: one more group
        pad = torch.cat([xs[rank], torch.zeros(32, dtype=dtype)])
        assert ((n + 31) // 32) % world != ((n + 63) // 32) % world
        _bytes_equal(comm.AllreduceCompressed(pad, seed=seed)[:n],
                     out.detach())
        gs = [_rank_input(r, n, dtype, salt=1) for r in range(world)]
        out.backward(gs[rank])
        _bytes_equal(x.grad, _allreduce_chain(gs, seed, 2))
        for L in (37, 64):   # a block per launch, and one launch
            xs = [_rank_input(r, world * L, dtype, salt=L)
                  for r in range(world)]
            Gb = (L + 31) // 32
            qs = [C._mx8_quantize_sr(x[rank * L:(rank + 1) * L], seed, 0, r,
                                     rank * Gb * 32)
                  for r, x in enumerate(xs)]
            want = C._mx8_reduce_to(torch.stack([q[0] for q in qs]),
                                    torch.stack([q[1] for q in qs]), L, dtype)
            _bytes_equal(comm.ReducescatterCompressed(xs[rank], 0, seed=seed),
                         want)


@pytest.mark.parametrize("world", [2, 3])
def test_ops_equal_the_chain_of_debug_ops(world):
    run_spmd(world, _ops_worker)


def _desync_worker(rank, world):
    os.environ["MPI4TORCH_AMD_DEBUG"] = "1"
    import mpi4torch_amd as m

    for call in (lambda s: m.COMM_WORLD.AllreduceCompressed(
                     torch.ones(64), seed=s),
                 lambda s: m.COMM_WORLD.ReducescatterCompressed(
                     torch.ones(64), 0, seed=s)):
        call(5)
        with pytest.raises(RuntimeError, match="desync"):
            call(5 + rank)


def test_rejections():
    from mpi4torch_amd.parallel import DistributedDataParallel

    with pytest.raises(RuntimeError, match="type .int."):
        m.COMM_WORLD.AllreduceCompressed(torch.ones(64), seed=1.5)
    with pytest.raises(RuntimeError, match="type .int."):
        m.COMM_WORLD.ReducescatterCompressed(torch.ones(64), 0, seed="7")
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        DistributedDataParallel(_Net().double(), grad_compression="mxfp8-sr")
    with pytest.raises(ValueError, match="grad_compression"):
        DistributedDataParallel(_Net(), grad_compression="mxfp4-sr")
    run_spmd(2, _desync_worker)


def _ddp_worker(rank, world):
    from mpi4torch_amd.parallel import DistributedDataParallel

    torch.manual_seed(3)
    net = _Net()
    ref = copy.deepcopy(net)
    ddp = DistributedDataParallel(net, bucket_cap_mb=0,   # bucket per param
                                  grad_compression="mxfp8-sr",
                                  compression_seed=11)
    c = 0
    for step in range(2):
        for model in (ddp, ref):
            model.zero_grad(set_to_none=True)
            (model(_ddp_data(rank + step)) ** 2).sum().backward()
        ddp.finish_gradient_sync()
        want = {id(p): q.grad for p, q in
                zip(net.parameters(), ref.parameters())}
        for b in ddp._buckets:
            flat = torch.cat([want[id(p)].reshape(-1) for p in b.params])
            red = m.COMM_WORLD.AllreduceCompressed(flat, seed=11 + c) / world
            _bytes_equal(torch.cat([p.grad.reshape(-1) for p in b.params]),
                         red)
            c += 1
    assert c == 2 * len(ddp._buckets) > 2


def test_ddp_step_uses_consecutive_seeds_ws2():
    run_spmd(2, _ddp_worker)
