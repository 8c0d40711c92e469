"""AllgatherCompressed (mxfp8 wire): the dequantize_blocks composite against
the pure-torch oracle, SPMD worlds on gloo, autograd, error checks, the
Python surface and the two FSDP compression options.

Every rank's result is the concatenation along the axis of
    cast(dq(q(x_r)))
over all ranks r, its own block included, with x_r rank r's contiguous
tensor flattened in row-major order and q/dq the codec of test_compressed.py
(groups of 32 start at the rank's first element).
"""

import copy

import pytest
import torch

import mpi4torch_amd as m  # module-level so TorchScript resolves m.MPI_Communicator
from spmd import run_spmd
from test_compressed import (oracle_quantize, oracle_dequantize_groups,
                             _rand_input)
from test_reducescatter_compressed import (oracle_reducescatter,
                                           _nan_aware_bytes_equal,
                                           _bytes_equal)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GEOMS = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 4099), (3, 40), (3, 41),
         (7, 4)]


# ------------------------------ the oracle --------------------------------

def oracle_codec(x):
    """cast(dq(q(x))) of one rank's tensor, in its own shape."""
    xc = x.contiguous()
    d = oracle_dequantize_groups(*oracle_quantize(xc.reshape(-1)))
    return d.reshape(-1)[:xc.numel()].to(xc.dtype).view(xc.shape)


def oracle_allgather(xs, axis):
    """All ranks' inputs -> what AllgatherCompressed returns on every rank."""
    return torch.cat([oracle_codec(x) for x in xs], dim=axis)


def _inputs(n, dtype, seed, scale=1.0):
    """randn * scale * rand(groups, 1): per-group magnitudes spread over the
    e4m3 range, plus the special groups when there is room for them."""
    g = torch.Generator().manual_seed(seed)
    G = (n + 31) // 32
    x = torch.randn(G, 32, generator=g) * scale * torch.rand(G, 1, generator=g)
    if G >= 8:
        x[1, 7] = 0.0                      # an exact-zero element
        x[2] = 0.0                         # an all-zero group
        x[3] = x[3].clamp(-1, 1)
        x[3, 5] = 448.0 * 2.0 ** -3        # amax exactly 448 * 2^j
        x[4, 9] = float("inf")             # one inf -> scale 255 group
        x[5, 0] = float("nan")
    return x.reshape(-1)[:n].to(dtype).contiguous()


def _stack_oracle_q(xs):
    qs = [oracle_quantize(x) for x in xs]
    return torch.stack([q[0] for q in qs]), torch.stack([q[1] for q in qs])


@pytest.fixture(scope="module")
def C():
    return m._C


# ------------------------- composite vs the oracle ------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1e-6, 3e4])
@pytest.mark.parametrize("geom", GEOMS)
def test_dequantize_blocks_matches_oracle(C, geom, scale, dtype):
    rows, row_elems = geom
    L = rows * row_elems
    for P in (1, 2, 5):
        xs = [_inputs(L, dtype, seed=97 * r + L + 1, scale=scale)
              if r != 1 else _rand_input(L, dtype, seed=5, scale=scale)
              for r in range(P)]
        pay, sc = _stack_oracle_q(xs)
        out = C._mx8_dequantize_blocks(pay, sc, rows, row_elems, dtype)
        assert out.dtype == dtype and out.shape == (rows, P, row_elems)
        want = torch.stack([oracle_codec(x).view(rows, row_elems)
                            for x in xs], dim=1)
        _nan_aware_bytes_equal(out, want)
        if L >= 256:
            flat = out[:, 0, :].reshape(-1)
            assert bool(torch.isnan(flat[4 * 32:6 * 32]).all())
        # the composite quantizer feeds it the same bytes
        q = C._mx8_quantize(xs[0])
        assert torch.equal(q[0], pay[0]) and torch.equal(q[1], sc[0])


@pytest.mark.parametrize("P", [1, 5])
def test_dequantize_blocks_clamped_exponent_region(C, P):
    """Groups whose amax is tiny or an fp32 subnormal: E clamps at -127 and
    the dequantized values are fp32 subnormals."""
    rows, row_elems = 3, 429                  # L = 32*40 + 7
    L = rows * row_elems
    xs = [_rand_input(L, torch.float32, seed=400 + r, scale=4e-38)
          for r in range(P)]
    assert bool((xs[0].abs() < 2.0 ** -126).any())
    pay, sc = _stack_oracle_q(xs)
    assert int(sc[0].min()) == 0                         # E = -127 reached
    out = C._mx8_dequantize_blocks(pay, sc, rows, row_elems, torch.float32)
    want = torch.stack([oracle_codec(x).view(rows, row_elems) for x in xs],
                       dim=1)
    _bytes_equal(out, want)
    assert bool((out != 0).any())


def test_dequantize_blocks_out_argument(C):
    rows, row_elems, P = 3, 11, 3
    xs = [_rand_input(33, torch.bfloat16, seed=r) for r in range(P)]
    pay, sc = _stack_oracle_q(xs)
    want = torch.stack([oracle_codec(x).view(rows, row_elems) for x in xs],
                       dim=1)
    buf = torch.full((99 + 8,), 7.0, dtype=torch.bfloat16)
    out = C._mx8_dequantize_blocks(pay, sc, rows, row_elems, torch.bfloat16,
                                   out=buf)
    assert out.data_ptr() == buf.data_ptr()
    assert out.shape == (rows, P, row_elems)
    _bytes_equal(buf[:99].view(rows, P, row_elems), want)
    assert bool((buf[99:] == 7.0).all())
    with pytest.raises(RuntimeError, match="expects uint8 payload"):
        C._mx8_dequantize_blocks(pay, sc, 5, 13, torch.bfloat16)


# ------------------------------ SPMD worlds -------------------------------

def _same_on_all_ranks(comm, t):
    """Uncompressed Allgather of the bytes: every rank's copy equals ours."""
    mine = t.contiguous().view(-1).view(torch.uint8)
    allb = comm.Allgather(mine, 0).view(comm.size, -1)
    return all(torch.equal(allb[r], mine) for r in range(comm.size))


def _spmd_worker(rank, world):
    comm = m.COMM_WORLD
    cases = [
        ("L1", (1,), torch.float32),
        ("L33", (33,), torch.float32),        # partial group per block
        ("L96", (96,), torch.float32),        # one flat stream
        ("L4099_bf16", (4099,), torch.bfloat16),
        ("L4099_f16", (4099,), torch.float16),
        ("3d_30", (2, 3, 5), torch.float32),  # L = 30
        ("3d_32", (4, 2, 4), torch.bfloat16),  # L = 32
        ("3d_96", (4, 3, 8), torch.float16),  # L = 96
        ("3d_105", (3, 5, 7), torch.float32),
    ]
    for tag, (name, shape, dtype) in enumerate(cases):
        n = 1
        for d in shape:
            n *= d
        scale = (1.0, 1e-6, 3e4)[tag % 3] if dtype != torch.float16 else 1.0
        xs = [_rand_input(n, dtype, seed=2000 * (tag + 1) + r,
                          scale=scale).view(shape) for r in range(world)]
        for axis in range(len(shape)):
            out = comm.AllgatherCompressed(xs[rank], axis)
            want = oracle_allgather(xs, axis)
            assert out.dtype == dtype and out.shape == want.shape, name
            _bytes_equal(out, want)
            assert _same_on_all_ranks(comm, out), name
    # negative axis wraps, axis defaults to 0
    _bytes_equal(comm.AllgatherCompressed(xs[rank], -1),
                 oracle_allgather(xs, 2))
    _bytes_equal(comm.AllgatherCompressed(xs[rank]), oracle_allgather(xs, 0))

    # non-contiguous input (a transposed view): quantized in the row-major
    # order of its own shape
    xs = [_rand_input(12 * 8, torch.float32, seed=60 + r).view(12, 8).t()
          for r in range(world)]
    assert not xs[rank].is_contiguous()
    out = comm.AllgatherCompressed(xs[rank], 1)
    assert out.shape == (8, 12 * world)
    _bytes_equal(out, oracle_allgather(xs, 1))

    # one NaN on rank k: only the group holding it, in rank k's block, is
    # NaN, on every rank
    L, k = 4099, world // 2
    xs = [_rand_input(L, torch.float32, seed=70 + r) for r in range(world)]
    xs[k][40] = float("nan")
    out = comm.AllgatherCompressed(xs[rank], 0)
    _nan_aware_bytes_equal(out, oracle_allgather(xs, 0))
    nan = torch.isnan(out)
    assert bool(nan[k * L + 32:k * L + 64].all())
    assert int(nan.sum()) == 32

    # backward: ReducescatterCompressed of the gradient. With per-rank
    # weights w_r the gradient on rank r is the compressed reduce-scatter
    # of the weights.
    ws = [_rand_input(3 * 40 * world, torch.float32, seed=90 + r)
          .view(3, 40 * world) for r in range(world)]
    x = _rand_input(3 * 40, torch.float32,
                    seed=80 + rank).view(3, 40).requires_grad_()
    y = comm.AllgatherCompressed(x, 1)
    assert y.grad_fn.name() == "M4AAllgatherCompressedBackward"
    (y * ws[rank]).sum().backward()
    _bytes_equal(x.grad, oracle_reducescatter(ws, 1, rank))
    # 1-D, L not a multiple of 32
    ws = [_rand_input(33 * world, torch.bfloat16, seed=95 + r)
          for r in range(world)]
    x = _rand_input(33, torch.bfloat16, seed=85 + rank).requires_grad_()
    (comm.AllgatherCompressed(x, 0) * ws[rank]).sum().backward()
    _bytes_equal(x.grad, oracle_reducescatter(ws, 0, rank))

    # the functional wrapper and the tracing passthrough reach the same op
    from mpi4torch_amd import ops
    from mpi4torch_amd.utils import trace

    xs = [_rand_input(33, torch.float32, seed=110 + r) for r in range(world)]
    want = oracle_allgather(xs, 0)
    _bytes_equal(ops.allgather_compressed(xs[rank]), want)
    _bytes_equal(ops.allgather_compressed(xs[rank], axis=0), want)
    traced = trace(comm)
    _bytes_equal(traced.AllgatherCompressed(xs[rank], 0), want)
    assert [r.op for r in traced.trace_records()] == ["AllgatherCompressed"]

    # zero-numel input gives an empty tensor of the output shape
    e = comm.AllgatherCompressed(torch.empty(2, 0), 0)
    assert e.shape == (2 * world, 0)
    e = comm.AllgatherCompressed(torch.empty(0, 3), 0)
    assert e.shape == (0, 3)


@pytest.mark.parametrize("world", [2, 5, 7])
def test_spmd(world):
    run_spmd(world, _spmd_worker)


def _unequal_counts_worker(rank, world):
    comm = m.COMM_WORLD
    with pytest.raises(RuntimeError,
                       match="equal counts.*Allgather handles variable"):
        comm.AllgatherCompressed(torch.ones(3, 5 + rank), 1)
    # the world is still in step afterwards
    out = comm.AllgatherCompressed(torch.full((3,), float(rank)), 0)
    assert out.tolist() == [0.0] * 3 + [1.0] * 3


def test_unequal_counts_ws2():
    run_spmd(2, _unequal_counts_worker)


def _debug_collectives_worker(rank, world):
    """The op goes through the collective-desync detector: matching calls
    pass, a rank with another off-axis shape is reported."""
    import os

    comm = m.COMM_WORLD
    os.environ["MPI4TORCH_AMD_DEBUG"] = "1"
    m._C.reload_config()
    try:
        x = _rand_input(100, torch.float32, seed=rank)
        assert comm.AllgatherCompressed(x, 0).shape == (200,)
        with pytest.raises(RuntimeError, match="desync"):
            comm.AllgatherCompressed(torch.ones(4, 3 + rank), 0)
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
        comm.AllgatherCompressed(torch.ones(4, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.AllgatherCompressed(torch.ones(4).to(torch.float8_e4m3fn), 0)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.AllgatherCompressed(torch.ones(4, dtype=torch.float64))
    e = comm.AllgatherCompressed(torch.empty(0, 3), 0)
    assert e.shape == (0, 3) and e.dtype == torch.float32
    # a world of one compresses nothing: exact clone, axis defaults to 0
    y = comm.AllgatherCompressed(x)
    assert y.data_ptr() != x.data_ptr()
    _bytes_equal(y, x)
    # and backward is the identity
    xg = torch.randn(6, 4, requires_grad=True)
    w = torch.randn(6, 4)
    (comm.AllgatherCompressed(xg, 1) * w).sum().backward()
    _bytes_equal(xg.grad, w)


def test_scriptable():
    @torch.jit.script
    def fn(comm: m.MPI_Communicator, t: torch.Tensor) -> torch.Tensor:
        return (comm.AllgatherCompressed(t, 0) +
                comm.AllgatherCompressed(t))

    t = torch.randn(40)
    torch.testing.assert_close(fn(m.COMM_WORLD, t), 2 * t, rtol=0, atol=0)


def test_tracing_wrapper_world1():
    from mpi4torch_amd.utils import trace

    traced = trace(m.COMM_WORLD)
    t = torch.randn(5, 3)
    _bytes_equal(traced.AllgatherCompressed(t, 1), t)
    assert [r.op for r in traced.trace_records()] == ["AllgatherCompressed"]


def test_wire_bytes_helper():
    from mpi4torch_amd.utils import mxfp8_allgather_wire_bytes

    # (world-1) * 33 * ceil(numel/32), counted by hand
    assert mxfp8_allgather_wire_bytes(1, 2) == 33
    assert mxfp8_allgather_wire_bytes(32, 2) == 33
    assert mxfp8_allgather_wire_bytes(33, 8) == 7 * 66
    assert mxfp8_allgather_wire_bytes(4099, 5) == 4 * 33 * 129
    assert mxfp8_allgather_wire_bytes(4099, 5) == 17028
    assert mxfp8_allgather_wire_bytes(100, 1) == 0
    # it is the size of what one rank receives: every other rank's stream
    p, s = m._C._mx8_quantize(torch.randn(4099))
    assert 4 * (p.numel() + s.numel()) == mxfp8_allgather_wire_bytes(4099, 5)


# ----------------------------------- FSDP ---------------------------------

def _net():
    # 216 and 125 parameters: shard_len 108 / 63 at world 2, 72 / 42 at
    # world 3 — never a multiple of 32
    return torch.nn.Sequential(torch.nn.Linear(8, 24), torch.nn.Tanh(),
                               torch.nn.Linear(24, 5))


def _data(rank, step=0):
    g = torch.Generator().manual_seed(300 + rank + 1000 * step)
    return torch.randn(6, 8, generator=g)


def _unit_flat(tensors, padded):
    flat = torch.zeros(padded)
    parts = [t.detach().reshape(-1) for t in tensors]
    torch.cat(parts, out=flat[:sum(p.numel() for p in parts)])
    return flat


def _capture_full_buffers(net, holder):
    """Forward hooks registered BEFORE the FSDP wrapper's: they run while
    the unit is still materialized and keep a copy of its full buffer."""
    captured = {}

    def hook(module, inputs, output):
        captured[module] = holder["fsdp"]._by_module[module].flat.clone()

    for mod in net.children():
        if any(True for _ in mod.parameters()):
            mod.register_forward_hook(hook)
    return captured


def _fsdp_worker(rank, world):
    from mpi4torch_amd.parallel import FullyShardedDataParallel

    comm = m.COMM_WORLD
    torch.manual_seed(3)
    base = _net()
    units_of = lambda net: [net[0], net[2]]

    # ---- param_compression: every rank computes with dq(q(shard_r)) -------
    net = copy.deepcopy(base)
    holder = {}
    captured = _capture_full_buffers(net, holder)
    fsdp = FullyShardedDataParallel(net, param_compression="mxfp8")
    holder["fsdp"] = fsdp
    assert fsdp.param_compression == "mxfp8" and fsdp.grad_compression is None
    assert all(u.shard_len % 32 != 0 for u in fsdp._units)
    fsdp(_data(rank))
    for u, bmod in zip(fsdp._units, units_of(base)):
        sl = u.shard_len
        orig = _unit_flat(list(bmod.parameters()), u.padded)
        # the master shard keeps full precision
        _bytes_equal(u.shard.detach(), orig[rank * sl:(rank + 1) * sl])
        want = oracle_allgather(
            [orig[r * sl:(r + 1) * sl] for r in range(world)], 0)
        full = captured[u.module]
        _bytes_equal(full, want)
        assert _same_on_all_ranks(comm, full)
        assert not torch.equal(full, orig)    # compression really happened
        # nothing was prefetched: the op has no non-blocking variant
        assert u.prefetch_handle is None
        u.start_materialize()
        assert u.prefetch_handle is None

    # ---- grad_compression: shard.grad is the compressed reduce-scatter ----
    local = []
    for r in range(world):
        ref = copy.deepcopy(base)
        (ref(_data(r)) ** 2).sum().backward()
        local.append(units_of(ref))
    net = copy.deepcopy(base)
    fsdp = FullyShardedDataParallel(net, grad_compression="mxfp8")
    assert fsdp.grad_compression == "mxfp8" and fsdp.param_compression is None
    (fsdp(_data(rank)) ** 2).sum().backward()
    assert all(u.grad_reduced is not None and u.grad_handle is None
               for u in fsdp._units)
    fsdp.finish_backward()
    plain_net = copy.deepcopy(base)
    plain = FullyShardedDataParallel(plain_net)
    (plain(_data(rank)) ** 2).sum().backward()
    assert all(u.grad_reduced is None and u.grad_handle is not None
               for u in plain._units)
    plain.finish_backward()
    for i, (u, up) in enumerate(zip(fsdp._units, plain._units)):
        gflats = [_unit_flat([p.grad for p in local[r][i].parameters()],
                             u.padded) for r in range(world)]
        want = oracle_reducescatter(gflats, 0, rank) / world
        _bytes_equal(u.shard.grad, want.to(u.shard.dtype))
        assert u.grad_reduced is None
        # compression really happened
        assert not torch.equal(u.shard.grad, up.shard.grad)

    # ---- both options: a few optimizer steps ------------------------------
    net = copy.deepcopy(base)
    holder = {}
    captured = _capture_full_buffers(net, holder)
    fsdp = FullyShardedDataParallel(net, param_compression="mxfp8",
                                    grad_compression="mxfp8")
    holder["fsdp"] = fsdp
    opt = torch.optim.SGD(fsdp.shard_parameters(), lr=0.05)
    prev = None
    for step in range(3):
        loss = (fsdp(_data(rank, step)) ** 2).sum()
        fsdp.zero_grad()
        loss.backward()
        fsdp.finish_backward()
        fulls = [captured[u.module] for u in fsdp._units]
        for f in fulls:
            assert bool(torch.isfinite(f).all())
            assert _same_on_all_ranks(comm, f)
        if prev is not None:
            assert not any(torch.equal(a, b) for a, b in zip(prev, fulls))
        prev = fulls
        opt.step()
        fsdp.refresh_shards()


@pytest.mark.parametrize("world", [2, 3])
def test_fsdp_compression(world):
    run_spmd(world, _fsdp_worker)


def test_fsdp_bad_arguments_and_world1():
    from mpi4torch_amd.parallel import FullyShardedDataParallel

    with pytest.raises(ValueError, match="param_compression"):
        FullyShardedDataParallel(_net(), param_compression="fp4")
    with pytest.raises(ValueError, match="grad_compression"):
        FullyShardedDataParallel(_net(), grad_compression="mxfp4")
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        FullyShardedDataParallel(_net().double(), param_compression="mxfp8")
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        FullyShardedDataParallel(_net().double(), grad_compression="mxfp8")
    # a world of one has no wire: the options are accepted and change nothing
    torch.manual_seed(3)
    base = _net()
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    models = [FullyShardedDataParallel(nets[0], param_compression="mxfp8",
                                       grad_compression="mxfp8"),
              FullyShardedDataParallel(nets[1])]
    outs = []
    for model in models:
        opt = torch.optim.SGD(model.shard_parameters(), lr=0.1)
        for step in range(2):
            y = model(_data(0, step))
            model.zero_grad()
            (y ** 2).sum().backward()
            model.finish_backward()
            opt.step()
            model.refresh_shards()
        outs.append(model(_data(0, 5)).detach())
    _bytes_equal(outs[0], outs[1])
    for ua, ub in zip(models[0]._units, models[1]._units):
        _bytes_equal(ua.shard.detach(), ub.shard.detach())
    assert not torch.equal(models[0]._units[0].shard.detach()[:8 * 24],
                           base[0].weight.detach().reshape(-1))
