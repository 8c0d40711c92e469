"""ReducescatterCompressed (mxfp8 wire, no requantization): the reduce_to
composite against the pure-torch oracle, the derived accuracy bound, SPMD
worlds on gloo, autograd, error checks, ZeRO-2 gradient compression.

Rank j's result is
    cast(((dq(q(b_0[j])) + dq(q(b_1[j]))) + ... + dq(q(b_{P-1}[j]))))
with b_r[j] rank r's block j flattened in row-major order of the output
shape, q/dq the codec of test_compressed.py (groups of 32 start at the
block's first element), the sum in fp32 in rank order and one RNE cast.
"""

import copy

import pytest
import torch

import mpi4torch_amd as m  # module-level so TorchScript resolves m.MPI_Communicator
from spmd import run_spmd
from test_compressed import (oracle_quantize, oracle_dequantize_groups,
                             _groups, _rand_input, _with_specials,
                             UNIT_ROUNDOFF)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


# ------------------------------ the oracle --------------------------------

def oracle_reduce_to(blocks):
    """Every rank's copy of one block (flat, same dtype) -> what its owner
    keeps: fp32 rank-order sum of the dequantized copies, one cast."""
    n = blocks[0].numel()
    S = None
    for b in blocks:
        d = oracle_dequantize_groups(*oracle_quantize(b))
        S = d if S is None else S + d
    return S.reshape(-1)[:n].to(blocks[0].dtype)


def _axis_block(x, axis, j, world):
    c = x.shape[axis] // world
    return x.narrow(axis, j * c, c).contiguous()


def oracle_reducescatter(xs, axis, j):
    """All ranks' inputs -> what ReducescatterCompressed returns on rank j."""
    world = len(xs)
    blocks = [_axis_block(x, axis, j, world) for x in xs]
    return oracle_reduce_to([b.reshape(-1) for b in blocks]).view(
        blocks[0].shape)


def reducescatter_bound(blocks, out):
    """Per-element bound on |out - sum_r x_r| (derived, not tuned): the one
    quantization obeys |q(x) - x| <= |x|/16 + amax_group * 2^-17 (see
    allreduce_bound; its second-quantization term is gone), the P-1 fp32
    adds lose at most (P-1) * 2^-24 * sum_r |dq(q(x_r))|, and the output
    rounding is |out| * u."""
    n = blocks[0].numel()
    P = len(blocks)
    bound = torch.zeros(_groups(blocks[0]).shape, dtype=torch.float64)
    mag = torch.zeros_like(bound)
    for x in blocks:
        g = _groups(x).double()
        bound += g.abs() / 16 + g.abs().amax(dim=1, keepdim=True) * 2.0 ** -17
        mag += oracle_dequantize_groups(*oracle_quantize(x)).double().abs()
    bound += (P - 1) * 2.0 ** -24 * mag
    bound = bound.reshape(-1)[:n]
    return bound + out.reshape(-1).double().abs() * UNIT_ROUNDOFF[out.dtype]


def _nan_aware_bytes_equal(a, b):
    """NaNs at the same positions, everything else byte for byte."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype,
                                                       a.shape, b.shape)
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb)
    assert torch.equal(a[~na].view(torch.uint8), b[~nb].view(torch.uint8))


def _bytes_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype,
                                                       a.shape, b.shape)
    assert torch.equal(a.contiguous().view(torch.uint8),
                       b.contiguous().view(torch.uint8))


def _stack_q(C, xs):
    qs = [C._mx8_quantize(x) for x in xs]
    return torch.stack([q[0] for q in qs]), torch.stack([q[1] for q in qs])


@pytest.fixture(scope="module")
def C():
    return m._C


# ------------------------- composite vs the oracle ------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1e-6, 3e4])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4099])
def test_reduce_to_matches_oracle(C, n, scale, dtype):
    for P in (1, 2, 5, 8):
        xs = [_with_specials(_rand_input(n, dtype, seed=97 * r + n + 1,
                                         scale=scale))
              if r != 1 else _rand_input(n, dtype, seed=5, scale=scale)
              for r in range(P)]
        pay, sc = _stack_q(C, xs)
        out = C._mx8_reduce_to(pay, sc, n, dtype)
        assert out.dtype == dtype and out.shape == (n,)
        _nan_aware_bytes_equal(out, oracle_reduce_to(xs))
        if P == 1:
            _nan_aware_bytes_equal(
                out, C._mx8_dequantize(pay[0], sc[0], n, dtype))


@pytest.mark.parametrize("P", [1, 5])
def test_reduce_to_clamped_exponent_region(C, P):
    """Groups whose amax is tiny or an fp32 subnormal: E clamps at -127 and
    the dequantized values and their sums are fp32 subnormals."""
    n = 32 * 40 + 7
    xs = [_rand_input(n, torch.float32, seed=400 + r, scale=4e-38)
          for r in range(P)]
    assert bool((xs[0].abs() < 2.0 ** -126).any())
    pay, sc = _stack_q(C, xs)
    assert int(sc[0].min()) == 0                         # E = -127 reached
    out = C._mx8_reduce_to(pay, sc, n, torch.float32)
    _bytes_equal(out, oracle_reduce_to(xs))
    assert bool((out != 0).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_to_nan_group_is_local(C, dtype):
    """A 255 scale in any one copy makes exactly that group NaN."""
    n, P = 4099, 5
    for bad_rank in (0, 3, P - 1):
        xs = [_rand_input(n, dtype, seed=20 + r) for r in range(P)]
        xs[bad_rank][5 * 32 + 9] = float("inf")
        pay, sc = _stack_q(C, xs)
        assert int(sc[bad_rank][5]) == 255
        out = C._mx8_reduce_to(pay, sc, n, dtype)
        assert bool(torch.isnan(out[5 * 32:6 * 32]).all())
        assert bool(torch.isfinite(out[:5 * 32]).all())
        assert bool(torch.isfinite(out[6 * 32:]).all())
        _nan_aware_bytes_equal(out, oracle_reduce_to(xs))


def test_reduce_to_out_argument(C):
    n = 33
    xs = [_rand_input(n, torch.bfloat16, seed=r) for r in range(3)]
    pay, sc = _stack_q(C, xs)
    buf = torch.full((n + 8,), 7.0, dtype=torch.bfloat16)
    out = C._mx8_reduce_to(pay, sc, n, torch.bfloat16, out=buf)
    assert out.data_ptr() == buf.data_ptr() and out.shape == (n,)
    _bytes_equal(buf[:n], oracle_reduce_to(xs))
    assert bool((buf[n:] == 7.0).all())
    with pytest.raises(RuntimeError, match="expects uint8 payload"):
        C._mx8_reduce_to(pay, sc, 65, torch.bfloat16)


def _accuracy_scales(dtype):
    # fp16 inputs overflow at 3e4
    return [1.0, 1e-6] if dtype == torch.float16 else [1.0, 1e-6, 3e4]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 2, 5, 8])
def test_accuracy_bound(C, P, dtype):
    n = 4099
    for scale in _accuracy_scales(dtype):
        xs = [_rand_input(n, dtype, seed=31 * r + P, scale=scale)
              for r in range(P)]
        pay, sc = _stack_q(C, xs)
        out = C._mx8_reduce_to(pay, sc, n, dtype)
        exact = sum(x.double() for x in xs)
        bound = reducescatter_bound(xs, out)
        err = (out.double() - exact).abs()
        ratio = (err / bound.clamp(min=1e-300)).max().item()
        print(f"P={P} scale={scale} {dtype}: worst error/bound = {ratio:.3f}")
        # no element is excluded
        assert bool(torch.isfinite(out).all())
        assert bool((err <= bound).all()), ratio


# ------------------------------ SPMD worlds -------------------------------

def _spmd_input(shape, dtype, rank, tag):
    n = 1
    for d in shape:
        n *= d
    return _rand_input(n, dtype, seed=2000 * (tag + 1) + rank,
                       scale=(1.0, 1e-6, 3e4)[tag % 3]
                       if dtype != torch.float16 else 1.0).view(shape)


def _spmd_worker(rank, world):
    comm = m.COMM_WORLD
    cases = [
        ("L1", 1, torch.float32),
        ("L33", 33, torch.float32),     # partial group, block bases off 16 B
        ("L96", 96, torch.float32),     # L % 32 == 0: one flat quantize
        ("L4099_bf16", 4099, torch.bfloat16),
        ("L4099_f16", 4099, torch.float16),
    ]
    for tag, (name, L, dtype) in enumerate(cases):
        xs = [_spmd_input((L * world,), dtype, r, tag) for r in range(world)]
        out = comm.ReducescatterCompressed(xs[rank], 0)
        assert out.dtype == dtype and out.shape == (L,), name
        _bytes_equal(out, oracle_reducescatter(xs, 0, rank))

    # 2-D input reduced along axis 1 (before > 1: rank-major packing)
    xs = [_rand_input(3 * 40 * world, torch.float32, seed=50 + r)
          .view(3, 40 * world) for r in range(world)]
    out = comm.ReducescatterCompressed(xs[rank], 1)
    assert out.shape == (3, 40)
    _bytes_equal(out, oracle_reducescatter(xs, 1, rank))
    # negative axis wraps
    _bytes_equal(comm.ReducescatterCompressed(xs[rank], -1), out)

    # non-contiguous input (a transposed view), axis 0
    xs = [_rand_input(12 * 8 * world, torch.float32, seed=60 + r)
          .view(12, 8 * world).t() for r in range(world)]
    assert not xs[rank].is_contiguous()
    out = comm.ReducescatterCompressed(xs[rank], 0)
    assert out.shape == (8, 12)
    _bytes_equal(out, oracle_reducescatter(xs, 0, rank))

    # one inf on the last rank inside block k: only rank k's group holding
    # it is NaN, everything else on every rank is finite
    L, k = 4099, world // 2
    xs = [_rand_input(L * world, torch.float32, seed=70 + r)
          for r in range(world)]
    xs[world - 1][k * L + 40] = float("inf")
    out = comm.ReducescatterCompressed(xs[rank], 0)
    want = oracle_reducescatter(xs, 0, rank)
    _nan_aware_bytes_equal(out, want)
    if rank == k:
        assert bool(torch.isnan(out[32:64]).all())
        assert bool(torch.isfinite(out[:32]).all())
        assert bool(torch.isfinite(out[64:]).all())
    else:
        assert bool(torch.isfinite(out).all())

    # backward: the adjoint is the uncompressed allgather, so x.grad is
    # exactly the concatenation of every rank's weights
    ws = [_rand_input(3 * 40, torch.float32, seed=90 + r).view(3, 40)
          for r in range(world)]
    x = _rand_input(3 * 40 * world, torch.float32,
                    seed=80 + rank).view(3, 40 * world).requires_grad_()
    y = comm.ReducescatterCompressed(x, 1)
    (y * ws[rank]).sum().backward()
    _bytes_equal(x.grad, torch.cat(ws, dim=1))

    # the functional wrapper and the tracing passthrough reach the same op
    from mpi4torch_amd import ops
    from mpi4torch_amd.utils import trace

    xs = [_rand_input(33 * world, torch.float32, seed=110 + r)
          for r in range(world)]
    want = oracle_reducescatter(xs, 0, rank)
    _bytes_equal(ops.reducescatter_compressed(xs[rank]), want)
    _bytes_equal(ops.reducescatter_compressed(xs[rank], axis=0), want)
    traced = trace(comm)
    _bytes_equal(traced.ReducescatterCompressed(xs[rank], 0), want)
    assert [r.op for r in traced.trace_records()] == [
        "ReducescatterCompressed"]

    # unequal counts are refused on every rank before anything is sent
    with pytest.raises(RuntimeError, match="equal counts"):
        comm.ReducescatterCompressed(torch.ones(world + 1), 0)


@pytest.mark.parametrize("world", [2, 5, 7])
def test_spmd(world):
    run_spmd(world, _spmd_worker)


def _debug_collectives_worker(rank, world):
    """The op goes through the collective-desync detector: matching calls
    pass, a rank with another shape is reported."""
    import os

    comm = m.COMM_WORLD
    os.environ["MPI4TORCH_AMD_DEBUG"] = "1"
    m._C.reload_config()
    try:
        x = _rand_input(100, torch.float32, seed=rank)
        assert comm.ReducescatterCompressed(x, 0).shape == (50,)
        with pytest.raises(RuntimeError, match="desync"):
            comm.ReducescatterCompressed(torch.ones(64 + 2 * rank), 0)
    finally:
        os.environ.pop("MPI4TORCH_AMD_DEBUG")
        m._C.reload_config()


def test_spmd_debug_collectives_ws2():
    run_spmd(2, _debug_collectives_worker)


# ---------------------- single-process surface checks ---------------------

def test_error_checks_and_world1():
    comm = m.COMM_WORLD
    x = torch.randn(100)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.ReducescatterCompressed(torch.ones(4, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.ReducescatterCompressed(
            torch.ones(4).to(torch.float8_e4m3fn), 0)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.ReducescatterCompressed(torch.ones(4, dtype=torch.float64))
    # zero-numel input gives an empty tensor of the output shape
    e = comm.ReducescatterCompressed(torch.empty(0, 3), 0)
    assert e.shape == (0, 3) and e.dtype == torch.float32
    e = comm.ReducescatterCompressed(torch.empty(4, 0), 0)
    assert e.shape == (4, 0)
    # a world of one compresses nothing: exact clone, axis defaults to 0
    y = comm.ReducescatterCompressed(x)
    assert y.data_ptr() != x.data_ptr()
    _bytes_equal(y, x)
    # and backward is the identity
    xg = torch.randn(6, 4, requires_grad=True)
    w = torch.randn(6, 4)
    (comm.ReducescatterCompressed(xg, 1) * w).sum().backward()
    _bytes_equal(xg.grad, w)


def _unequal_counts_worker(rank, world):
    comm = m.COMM_WORLD
    with pytest.raises(RuntimeError,
                       match="equal counts.*Reducescatter handles variable"):
        comm.ReducescatterCompressed(torch.ones(3, 5), 1)


def test_unequal_counts_ws2():
    run_spmd(2, _unequal_counts_worker)


def test_scriptable():
    @torch.jit.script
    def fn(comm: m.MPI_Communicator, t: torch.Tensor) -> torch.Tensor:
        return (comm.ReducescatterCompressed(t, 0) +
                comm.ReducescatterCompressed(t))

    t = torch.randn(40)
    torch.testing.assert_close(fn(m.COMM_WORLD, t), 2 * t, rtol=0, atol=0)


def test_wire_bytes_helper():
    from mpi4torch_amd.utils import (mxfp8_reducescatter_wire_bytes,
                                     mxfp8_wire_bytes)

    assert mxfp8_reducescatter_wire_bytes(4099 * 5, 5) == 4 * 33 * 129
    assert mxfp8_reducescatter_wire_bytes(32 * 8, 8) == 7 * 33
    assert mxfp8_reducescatter_wire_bytes(100, 1) == 0
    # it is the size of what one rank sends: its copy of the other blocks
    x = torch.randn(4099 * 5)
    sent = 0
    for j in range(1, 5):
        p, s = m._C._mx8_quantize(x[j * 4099:(j + 1) * 4099].contiguous())
        sent += p.numel() + s.numel()
    assert sent == mxfp8_reducescatter_wire_bytes(4099 * 5, 5)
    # half of the compressed allreduce's exchange + allgather
    n = 32 * 8 * 1000
    assert 2 * mxfp8_reducescatter_wire_bytes(n, 8) == \
        2 * 7 * mxfp8_wire_bytes(n) // 8


# ---------------------------------- ZeRO-2 --------------------------------

class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.trunk = torch.nn.Linear(8, 24)
        self.head = torch.nn.Linear(24, 5)
        self.extra = torch.nn.Linear(8, 5)

    def forward(self, x):
        return self.head(torch.tanh(self.trunk(x))) + self.extra(x)


def _data(rank, step=0):
    g = torch.Generator().manual_seed(300 + rank + 1000 * step)
    return torch.randn(6, 8, generator=g)


def _same_on_all_ranks(comm, t):
    v = t.contiguous().view(torch.uint8).to(torch.int32)
    return torch.equal(comm.Allreduce(v, m.MPI_MAX),
                       comm.Allreduce(v, m.MPI_MIN))


def _bucket_flat(sdp, b, what):
    """The bucket's parameters (or their grads), flattened and zero-padded
    to shard_len * P like the class does."""
    P = sdp.comm.size
    flat = torch.zeros(b.shard_len * P)
    parts = [(q if what == "param" else q.grad).detach().reshape(-1)
             for q in b.params]
    torch.cat(parts, out=flat[:sum(b.numels)])
    return flat


def _zero2_worker(rank, world):
    from mpi4torch_amd.parallel.sharded_ddp import ShardedDataParallel

    comm = m.COMM_WORLD
    torch.manual_seed(3)
    base = _Net()
    comp_net, plain_net = copy.deepcopy(base), copy.deepcopy(base)
    comp = ShardedDataParallel(comp_net, torch.optim.SGD, lr=1.0,
                               grad_compression="mxfp8")
    plain = ShardedDataParallel(plain_net, torch.optim.SGD, lr=1.0)
    assert comp.grad_compression == "mxfp8"
    assert plain.grad_compression is None
    assert [b.shard_len for b in comp._buckets] == \
        [b.shard_len for b in plain._buckets]

    # every rank's local gradients, rebuilt locally from the shared seeds,
    # in the bucket's own parameter order
    pname = {id(p): n for n, p in comp_net.named_parameters()}
    local = []
    for r in range(world):
        net = copy.deepcopy(base)
        (net(_data(r)) ** 2).sum().backward()
        local.append({n: p.grad.clone() for n, p in net.named_parameters()})
    old = {id(b): _bucket_flat(comp, b, "param") for b in comp._buckets}

    for sdp in (comp, plain):
        (sdp(_data(rank)) ** 2).sum().backward()
        sdp.step()

    for b, bp in zip(comp._buckets, plain._buckets):
        sl = b.shard_len
        total = sum(b.numels)
        flats = []
        for r in range(world):
            f = torch.zeros(sl * world)
            torch.cat([local[r][pname[id(q)]].reshape(-1) for q in b.params],
                      out=f[:total])
            flats.append(f)
        shards = [[f[j * sl:(j + 1) * sl] for f in flats]
                  for j in range(world)]
        reduced = torch.cat([oracle_reduce_to(s) for s in shards])
        # SGD without momentum at lr=1 is one add_: old - grad, and the grad
        # is the oracle's shard divided by P
        want = old[id(b)] - reduced / world
        got = _bucket_flat(comp, b, "param")
        _bytes_equal(got[:total], want[:total])
        assert _same_on_all_ranks(comm, got)
        # within the derived bound (averaged) of the uncompressed run, and
        # not identical to it: compression really happened
        ref = _bucket_flat(plain, bp, "param")
        bound = torch.cat([reducescatter_bound(s, oracle_reduce_to(s))
                           for s in shards]) / world
        err = (got.double() - ref.double()).abs()
        assert bool((err <= bound).all()), (err / bound).max().item()
        assert float(err.max()) > 0.0
        # the full gradients were freed
        assert all(q.grad is None for q in b.params)

    # no_sync accumulation followed by a synchronized backward
    before = _bucket_flat(comp, comp._buckets[0], "param")
    with comp.no_sync():
        (comp(_data(rank, 1)) ** 2).sum().backward()
    acc = comp_net.trunk.weight.grad.clone()
    assert all(b.reduced is None and b.handle is None for b in comp._buckets)
    (comp(_data(rank, 2)) ** 2).sum().backward()
    assert all(b.reduced is not None for b in comp._buckets)
    assert float(acc.abs().max()) > 0.0
    comp.step()
    after = _bucket_flat(comp, comp._buckets[0], "param")
    assert _same_on_all_ranks(comm, after)
    assert not torch.equal(before, after)

    # grad_compression=None changes nothing: bit for bit against a second
    # uncompressed instance
    a_net, b_net = copy.deepcopy(base), copy.deepcopy(base)
    a = ShardedDataParallel(a_net, torch.optim.SGD, lr=1.0)
    bb = ShardedDataParallel(b_net, torch.optim.SGD, lr=1.0,
                             grad_compression=None)
    for sdp in (a, bb):
        (sdp(_data(rank)) ** 2).sum().backward()
        assert all(b.reduced is None and b.handle is not None
                   for b in sdp._buckets)
        sdp.step()
    for pa, pb in zip(a_net.parameters(), b_net.parameters()):
        _bytes_equal(pa.detach(), pb.detach())
    _bytes_equal(_bucket_flat(a, a._buckets[0], "param"),
                 _bucket_flat(plain, plain._buckets[0], "param"))


@pytest.mark.parametrize("world", [2, 3])
def test_zero2_grad_compression(world):
    run_spmd(world, _zero2_worker)


def test_zero2_bad_arguments_and_world1():
    from mpi4torch_amd.parallel.sharded_ddp import ShardedDataParallel

    with pytest.raises(ValueError, match="grad_compression"):
        ShardedDataParallel(_Net(), torch.optim.SGD, lr=1.0,
                            grad_compression="fp4")
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        ShardedDataParallel(_Net().double(), torch.optim.SGD, lr=1.0,
                            grad_compression="mxfp8")
    # a world of one has no wire: the option is accepted and changes nothing
    torch.manual_seed(3)
    base = _Net()
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    sdps = [ShardedDataParallel(nets[0], torch.optim.SGD, lr=1.0,
                                grad_compression="mxfp8"),
            ShardedDataParallel(nets[1], torch.optim.SGD, lr=1.0)]
    for sdp in sdps:
        (sdp(_data(0)) ** 2).sum().backward()
        sdp.step()
    for pa, pb in zip(nets[0].parameters(), nets[1].parameters()):
        _bytes_equal(pa.detach(), pb.detach())
    assert not torch.equal(nets[0].trunk.weight, base.trunk.weight)
