"""AlltoallCompressed (mxfp8 wire): the quantize_blocks composite against the
pure-torch oracle, SPMD worlds on gloo, autograd, error checks, the Python
surface, the Ulysses helpers and the transformer block's option.

On rank `me` the block of the result that came from rank r is
    cast(dq(q(flat(contiguous(x_r.narrow(scatteraxis, me*n, n))))))
with n the scatter-axis size over the world size and q/dq the codec of
test_compressed.py (groups of 32 start at the block's first element); the
blocks are concatenated along the gather axis in rank order.
"""

import itertools

import pytest
import torch

import mpi4torch_amd as m  # module-level so TorchScript resolves m.MPI_Communicator
from spmd import run_spmd
from test_compressed import oracle_quantize, _rand_input
from test_reducescatter_compressed import (_nan_aware_bytes_equal,
                                           _bytes_equal)
from test_allgather_compressed import oracle_codec, _inputs

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GEOMS = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 4099), (3, 40), (3, 41),
         (7, 4)]


# ------------------------------ the oracle --------------------------------

def oracle_alltoall(xs, gatheraxis, scatteraxis):
    """All ranks' inputs -> what AlltoallCompressed returns, per rank."""
    P = len(xs)
    gatheraxis %= xs[0].dim()
    scatteraxis %= xs[0].dim()
    n = xs[0].shape[scatteraxis] // P
    return [torch.cat([oracle_codec(x.narrow(scatteraxis, me * n, n))
                       for x in xs], dim=gatheraxis) for me in range(P)]


def _blocks_input(blocks, rows, row_elems):
    """P flat blocks of rows*row_elems elements -> the flat
    [rows][P][row_elems] tensor whose block p they are."""
    return torch.stack([b.view(rows, row_elems) for b in blocks],
                       dim=1).contiguous().view(-1)


@pytest.fixture(scope="module")
def C():
    return m._C


# ------------------------- composite vs the oracle ------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1e-6, 3e4])
@pytest.mark.parametrize("geom", GEOMS)
def test_quantize_blocks_matches_oracle(C, geom, scale, dtype):
    rows, row_elems = geom
    L = rows * row_elems
    Gb = (L + 31) // 32
    for P in (1, 2, 5):
        blocks = [_inputs(L, dtype, seed=97 * r + L + 1, scale=scale)
                  if r != 1 else
                  _rand_input(L, dtype, seed=5, scale=scale).contiguous()
                  for r in range(P)]
        x = _blocks_input(blocks, rows, row_elems)
        pay, sc = C._mx8_quantize_blocks(x, P, rows, row_elems)
        assert pay.dtype == torch.uint8 and pay.shape == (P, Gb * 32)
        assert sc.dtype == torch.uint8 and sc.shape == (P, Gb)
        for p in range(P):
            want_p, want_s = oracle_quantize(blocks[p])
            assert torch.equal(sc[p], want_s), (p, P)
            assert torch.equal(pay[p], want_p), (p, P)   # padding included
        if L >= 256:
            assert int(sc[0, 4]) == 255 and int(sc[0, 5]) == 255
            assert not bool(pay[0, 4 * 32:6 * 32].any())
        if L % 32:
            assert not bool(pay[:, L:].any())             # zero padding


@pytest.mark.parametrize("P", [1, 5])
def test_quantize_blocks_clamped_exponent_region(C, P):
    """Groups whose amax is tiny or an fp32 subnormal: E clamps at -127."""
    rows, row_elems = 3, 429                  # L = 32*40 + 7
    L = rows * row_elems
    blocks = [_rand_input(L, torch.float32, seed=400 + r,
                          scale=4e-38).contiguous() for r in range(P)]
    assert bool((blocks[0].abs() < 2.0 ** -126).any())
    pay, sc = C._mx8_quantize_blocks(_blocks_input(blocks, rows, row_elems),
                                     P, rows, row_elems)
    assert int(sc[0].min()) == 0                         # E = -127 reached
    assert bool(pay.any())
    for p in range(P):
        want_p, want_s = oracle_quantize(blocks[p])
        assert torch.equal(sc[p], want_s) and torch.equal(pay[p], want_p)


def test_quantize_blocks_out_arguments(C):
    rows, row_elems, P = 3, 11, 3             # L = 33, Gb = 2
    blocks = [_rand_input(33, torch.bfloat16, seed=r).contiguous()
              for r in range(P)]
    x = _blocks_input(blocks, rows, row_elems)
    want = C._mx8_quantize_blocks(x, P, rows, row_elems)
    pbuf = torch.full((P * 64 + 8,), 0xAB, dtype=torch.uint8)
    sbuf = torch.full((P * 2 + 8,), 0xAB, dtype=torch.uint8)
    pay, sc = C._mx8_quantize_blocks(x, P, rows, row_elems,
                                     payload_out=pbuf, scales_out=sbuf)
    assert pay.data_ptr() == pbuf.data_ptr() and pay.shape == (P, 64)
    assert sc.data_ptr() == sbuf.data_ptr() and sc.shape == (P, 2)
    assert torch.equal(pbuf[:P * 64].view(P, 64), want[0])
    assert torch.equal(sbuf[:P * 2].view(P, 2), want[1])
    assert bool((pbuf[P * 64:] == 0xAB).all())
    assert bool((sbuf[P * 2:] == 0xAB).all())
    # an input view with an offset base
    y = torch.cat([torch.zeros(1, dtype=x.dtype), x])[1:]
    got = C._mx8_quantize_blocks(y, P, rows, row_elems)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(RuntimeError, match="rows\\*nblocks\\*row_elems"):
        C._mx8_quantize_blocks(x, P, 5, 13)
    with pytest.raises(RuntimeError, match="at least P\\*Gb\\*32"):
        C._mx8_quantize_blocks(x, P, rows, row_elems, payload_out=pbuf[:100],
                               scales_out=sbuf)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        C._mx8_quantize_blocks(torch.ones(99, dtype=torch.int32), P, rows,
                               row_elems)


def test_pack_blocks_hook(C):
    """_pack_blocks (the microbenchmark's yardstick) is the rank-major pack:
    quantizing its staging block by block gives quantize_blocks' bytes."""
    rows, P, row_elems = 3, 4, 40
    x = _rand_input(rows * P * row_elems, torch.float32, seed=7).contiguous()
    stage = torch.empty_like(x)
    C._pack_blocks(x.view(rows, P, row_elems), stage)
    assert torch.equal(stage.view(P, rows, row_elems),
                       x.view(rows, P, row_elems).permute(1, 0, 2))
    pay, sc = C._mx8_quantize_blocks(x, P, rows, row_elems)
    for p in range(P):
        q = C._mx8_quantize(stage.view(P, -1)[p])
        assert torch.equal(q[0], pay[p]) and torch.equal(q[1], sc[p])
    with pytest.raises(RuntimeError, match="debug_pack_blocks expects"):
        C._pack_blocks(x.view(rows, P, row_elems), stage[:-1])


# ------------------------------ SPMD worlds -------------------------------

def _check_pair(comm, rank, world, shape, dtype, gaxis, saxis, seed,
                scale=1.0):
    """Forward against the oracle; backward against the oracle all-to-all
    of the weights with the axes swapped."""
    n = 1
    for d in shape:
        n *= d
    xs = [_rand_input(n, dtype, seed=seed + r, scale=scale).view(shape)
          for r in range(world)]
    want = oracle_alltoall(xs, gaxis, saxis)
    x = xs[rank].clone().requires_grad_()
    y = comm.AlltoallCompressed(x, gaxis, saxis)
    assert y.grad_fn.name() == "M4AAlltoallCompressedBackward"
    assert y.dtype == dtype and y.shape == want[rank].shape, (shape, gaxis,
                                                              saxis)
    _bytes_equal(y.detach(), want[rank])
    ws = [_rand_input(n, dtype, seed=seed + 500 + r, scale=scale)
          .view(want[r].shape) for r in range(world)]
    y.backward(ws[rank])
    gwant = oracle_alltoall(ws, saxis, gaxis)
    assert x.grad.shape == tuple(shape)
    _bytes_equal(x.grad, gwant[rank])


def _spmd_worker(rank, world):
    comm = m.COMM_WORLD
    P = world
    # every ordered pair of distinct axes of a 3-D input
    shape = (2 * P, 3 * P, P)
    for i, (g, s) in enumerate(itertools.permutations(range(3), 2)):
        _check_pair(comm, rank, world, shape, torch.float32, g, s,
                    seed=1000 + 10 * i, scale=(1.0, 1e-6, 3e4)[i % 3])
    # the 4-D Ulysses shape, sequence <-> heads
    for dtype in DTYPES:
        _check_pair(comm, rank, world, (2, 3, P * 2, 8), dtype, 1, 2,
                    seed=2000)
    # groups straddling rows: the send side is [3][P][40]
    _check_pair(comm, rank, world, (3, P * 5, 8), torch.bfloat16, 0, 1,
                seed=3000)
    _check_pair(comm, rank, world, (3, P * 5, 8), torch.float32, 2, 1,
                seed=3100, scale=3e4)
    # an odd row length: the send side is [3][P][41]
    _check_pair(comm, rank, world, (3, P * 41), torch.float16, 0, 1,
                seed=4000)
    _check_pair(comm, rank, world, (3, P * 41), torch.float32, 0, 1,
                seed=4100, scale=1e-6)
    # a block of one element
    _check_pair(comm, rank, world, (1, P), torch.float32, 0, 1, seed=4200)

    # negative axes wrap
    xs = [_rand_input(3 * P * 8, torch.float32, seed=50 + r).view(3, P, 8)
          for r in range(world)]
    _bytes_equal(comm.AlltoallCompressed(xs[rank], -3, -2),
                 oracle_alltoall(xs, 0, 1)[rank])

    # non-contiguous input (a transposed view): blocks are taken in the
    # row-major order of its own shape
    xs = [_rand_input(12 * 4 * P, torch.float32, seed=60 + r)
          .view(12, 4 * P).t() for r in range(world)]
    assert not xs[rank].is_contiguous()
    out = comm.AlltoallCompressed(xs[rank], 1, 0)
    assert out.shape == (4, 12 * P)
    _bytes_equal(out, oracle_alltoall(xs, 1, 0)[rank])

    # one NaN on rank k, in the block that goes to rank 0: only the group
    # holding it is NaN, and only there
    L, k = 4099, world // 2
    xs = [_rand_input(P * L, torch.float32, seed=70 + r).view(1, P * L)
          for r in range(world)]
    xs[k][0, 40] = float("nan")
    out = comm.AlltoallCompressed(xs[rank], 0, 1)
    _nan_aware_bytes_equal(out, oracle_alltoall(xs, 0, 1)[rank])
    nan = torch.isnan(out)
    if rank == 0:
        assert bool(nan[k, 32:64].all()) and int(nan.sum()) == 32
    else:
        assert int(nan.sum()) == 0

    # the functional wrapper and the tracing passthrough reach the same op
    from mpi4torch_amd import ops
    from mpi4torch_amd.utils import trace

    xs = [_rand_input(3 * P * 11, torch.float32, seed=110 + r)
          .view(3, P * 11) for r in range(world)]
    want = oracle_alltoall(xs, 0, 1)[rank]
    _bytes_equal(ops.alltoall_compressed(xs[rank], 0, 1), want)
    traced = trace(comm)
    _bytes_equal(traced.AlltoallCompressed(xs[rank], 0, 1), want)
    assert [r.op for r in traced.trace_records()] == ["AlltoallCompressed"]

    # zero-numel input gives an empty tensor of the output shape
    e = comm.AlltoallCompressed(torch.empty(2, 0, 3 * P), 0, 2)
    assert e.shape == (2 * P, 0, 3)
    e = comm.AlltoallCompressed(torch.empty(0, P), 0, 1)
    assert e.shape == (0, 1)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_spmd(world):
    run_spmd(world, _spmd_worker)


def _errors_worker(rank, world):
    comm = m.COMM_WORLD
    with pytest.raises(RuntimeError,
                       match="equal counts.*multiple of the world size.*"
                             "Alltoall/Alltoallv handle variable"):
        comm.AlltoallCompressed(torch.ones(3, 5), 0, 1)
    with pytest.raises(RuntimeError,
                       match="equal counts.*same size on the gather axis.*"
                             "Alltoall/Alltoallv handle variable"):
        comm.AlltoallCompressed(torch.ones(3 + rank, 4), 0, 1)
    with pytest.raises(RuntimeError,
                       match="two different axes.*Alltoall handles the "
                             "same-axis repartition"):
        comm.AlltoallCompressed(torch.ones(4, 4), 1, -1)
    # the world is still in step afterwards
    out = comm.AlltoallCompressed(torch.full((1, 2), float(rank)), 0, 1)
    assert out.tolist() == [[0.0], [1.0]]


def test_errors_ws2():
    run_spmd(2, _errors_worker)


def _debug_collectives_worker(rank, world):
    """The op goes through the collective-desync detector: matching calls
    pass, a rank with another off-axis shape is reported."""
    import os

    comm = m.COMM_WORLD
    os.environ["MPI4TORCH_AMD_DEBUG"] = "1"
    m._C.reload_config()
    try:
        x = _rand_input(3 * 8, torch.float32, seed=rank).view(3, 8)
        assert comm.AlltoallCompressed(x, 0, 1).shape == (6, 4)
        with pytest.raises(RuntimeError, match="desync"):
            comm.AlltoallCompressed(torch.ones(4, 2, 3 + rank), 0, 1)
    finally:
        os.environ.pop("MPI4TORCH_AMD_DEBUG")
        m._C.reload_config()


def test_spmd_debug_collectives_ws2():
    run_spmd(2, _debug_collectives_worker)


# ---------------------- single-process surface checks ---------------------

def test_error_checks_and_world1():
    comm = m.COMM_WORLD
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.AlltoallCompressed(torch.ones(4, 4, dtype=torch.int32), 0, 1)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.AlltoallCompressed(torch.ones(4, 4, dtype=torch.float64), 0, 1)
    with pytest.raises(RuntimeError,
                       match="two different axes.*Alltoall handles the "
                             "same-axis repartition"):
        comm.AlltoallCompressed(torch.ones(4, 4), 0, 0)
    with pytest.raises(RuntimeError, match="two different axes"):
        comm.AlltoallCompressed(torch.ones(4, 4), 1, -1)
    e = comm.AlltoallCompressed(torch.empty(0, 3), 0, 1)
    assert e.shape == (0, 3) and e.dtype == torch.float32
    # a world of one compresses nothing: exact clone
    x = torch.randn(7, 13)
    y = comm.AlltoallCompressed(x, 0, 1)
    assert y.data_ptr() != x.data_ptr()
    _bytes_equal(y, x)
    # and backward is the identity
    xg = torch.randn(6, 4, requires_grad=True)
    w = torch.randn(6, 4)
    comm.AlltoallCompressed(xg, 1, 0).backward(w)
    _bytes_equal(xg.grad, w)


def test_scriptable():
    @torch.jit.script
    def fn(comm: m.MPI_Communicator, t: torch.Tensor) -> torch.Tensor:
        return comm.AlltoallCompressed(t, 0, 1)

    t = torch.randn(5, 8)
    torch.testing.assert_close(fn(m.COMM_WORLD, t), t, rtol=0, atol=0)


def test_tracing_wrapper_world1():
    from mpi4torch_amd.utils import trace

    traced = trace(m.COMM_WORLD)
    t = torch.randn(5, 3)
    _bytes_equal(traced.AlltoallCompressed(t, 1, 0), t)
    assert [r.op for r in traced.trace_records()] == ["AlltoallCompressed"]


def test_wire_bytes_helper():
    from mpi4torch_amd.utils import alltoall_compressed_wire_bytes

    # (P-1) * 33 * ceil(numel/P/32), counted by hand: blocks of 4099
    # elements are 129 groups of 33 bytes, three of them leave the rank
    assert alltoall_compressed_wire_bytes(4099 * 4, 4) == 3 * 33 * 129
    assert alltoall_compressed_wire_bytes(4099 * 4, 4) == 12771
    assert alltoall_compressed_wire_bytes(64, 2) == 33
    assert alltoall_compressed_wire_bytes(66, 2) == 66
    assert alltoall_compressed_wire_bytes(100, 1) == 0
    # it is the size of what one rank sends: every block but its own
    p, s = m._C._mx8_quantize_blocks(torch.randn(4099 * 4), 4, 1, 4099)
    assert 3 * (p[0].numel() + s[0].numel()) == 12771


# ------------------------------ Ulysses helpers ---------------------------

def _ulysses_worker(rank, world):
    from mpi4torch_amd.parallel import (seq_to_head, head_to_seq,
                                        ulysses_reshard)

    comm = m.COMM_WORLD
    P = world
    b, s_loc, h, d = 2, 3, 2 * P, 8
    for dtype in (torch.float32, torch.bfloat16):
        ts = [_rand_input(b * s_loc * h * d, dtype, seed=700 + r)
              .view(b, s_loc, h, d) for r in range(world)]
        first = oracle_alltoall(ts, 1, 2)
        out = seq_to_head(ts[rank], compression="mxfp8")
        assert out.shape == (b, s_loc * P, h // P, d)
        _bytes_equal(out, first[rank])
        back = head_to_seq(out, compression="mxfp8")
        assert back.shape == (b, s_loc, h, d)
        _bytes_equal(back, oracle_alltoall(first, 2, 1)[rank])
        _bytes_equal(ulysses_reshard(ts[rank], 1, 2, h // P,
                                     compression="mxfp8"), first[rank])
    # compression=None is the uncompressed path, byte for byte
    t = ts[rank].float()
    plain = comm.Alltoallv(t, 1, 2, [h // P] * P, [s_loc] * P)
    assert torch.equal(t, head_to_seq(plain))          # a pure permutation
    _bytes_equal(seq_to_head(t), plain)
    _bytes_equal(seq_to_head(t, compression=None), plain)
    _bytes_equal(head_to_seq(plain, compression=None), t)
    _bytes_equal(ulysses_reshard(t, 1, 2, h // P, compression=None), plain)
    # backward through both compressed reshards
    x = t.clone().requires_grad_()
    w = _rand_input(t.numel(), torch.float32, seed=800 + rank).view(t.shape)
    head_to_seq(seq_to_head(x, compression="mxfp8"),
                compression="mxfp8").backward(w)
    ws = [_rand_input(t.numel(), torch.float32, seed=800 + r).view(t.shape)
          for r in range(world)]
    _bytes_equal(x.grad,
                 oracle_alltoall(oracle_alltoall(ws, 1, 2), 2, 1)[rank])
    with pytest.raises(ValueError, match="must be None or 'mxfp8'"):
        seq_to_head(t, compression="fp4")
    with pytest.raises(ValueError, match="must be None or 'mxfp8'"):
        head_to_seq(t, compression="mxfp4")
    with pytest.raises(ValueError, match="must be None or 'mxfp8'"):
        ulysses_reshard(t, 1, 2, h // P, compression="e5m2")
    with pytest.raises(ValueError, match="equal counts"):
        ulysses_reshard(t, 1, 2, h // P + 1, compression="mxfp8")


@pytest.mark.parametrize("world", [2, 4])
def test_ulysses_helpers(world):
    run_spmd(world, _ulysses_worker)


def test_ulysses_helpers_world1():
    from mpi4torch_amd.parallel import seq_to_head, head_to_seq

    t = torch.randn(2, 3, 4, 8)
    _bytes_equal(seq_to_head(t, compression="mxfp8"), t)
    _bytes_equal(head_to_seq(t, compression="mxfp8"), t)
    with pytest.raises(ValueError, match="must be None or 'mxfp8'"):
        seq_to_head(t, compression="fp8")


# --------------------------- the transformer block ------------------------

class _Recorder:
    """A communicator stand-in that keeps what AlltoallCompressed saw."""

    def __init__(self, comm):
        self._comm = comm
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._comm, name)

    def AlltoallCompressed(self, t, gatheraxis, scatteraxis):
        out = self._comm.AlltoallCompressed(t, gatheraxis, scatteraxis)
        self.calls.append((t.detach().clone(), gatheraxis, scatteraxis,
                           out.detach().clone()))
        return out


def _transformer_worker(rank, world):
    from mpi4torch_amd.models.transformer import UlyssesTransformerBlock

    comm = m.COMM_WORLD
    d_model, n_heads, B, S_local = 16, 2 * world, 2, 4
    torch.manual_seed(5)
    block = UlyssesTransformerBlock(d_model, n_heads, compression="mxfp8")
    assert block.compression == "mxfp8"
    rec = _Recorder(comm)
    block.comm = rec
    torch.manual_seed(40 + rank)
    x = torch.randn(B, S_local, d_model, requires_grad=True)
    y = block(x)
    loss = (y ** 2).sum()
    loss.backward()
    assert bool(torch.isfinite(loss))
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for p in block.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    # forward saw two compressed reshards: q/k/v in, attention out
    assert [(c[1], c[2]) for c in rec.calls[:2]] == [(1, 3), (2, 1)]
    qkv_in, _, _, qkv_out = rec.calls[0]
    assert qkv_in.shape == (B, S_local, 3, n_heads, d_model // n_heads)
    every = comm.Allgather(qkv_in.unsqueeze(0), 0)
    want = oracle_alltoall([every[r] for r in range(world)], 1, 3)[rank]
    _bytes_equal(qkv_out, want)
    assert not torch.equal(
        qkv_out, comm.Alltoallv(qkv_in, 1, 3, [n_heads // world] * world,
                                [S_local] * world))   # it really compressed

    # the option off: the module is what it is without the argument
    torch.manual_seed(5)
    off = UlyssesTransformerBlock(d_model, n_heads, compression=None)
    torch.manual_seed(5)
    plain = UlyssesTransformerBlock(d_model, n_heads)
    assert off.compression is None
    sd_off, sd_plain = off.state_dict(), plain.state_dict()
    assert list(sd_off) == list(sd_plain)
    for k in sd_off:
        _bytes_equal(sd_off[k], sd_plain[k])
    outs = []
    for blk in (off, plain):
        xi = x.detach().clone().requires_grad_()
        yi = blk(xi)
        (yi ** 2).sum().backward()
        outs.append((yi.detach(), xi.grad))
    _bytes_equal(outs[0][0], outs[1][0])
    _bytes_equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError, match="must be None or 'mxfp8'"):
        UlyssesTransformerBlock(d_model, n_heads, compression="fp4")


def test_transformer_block_ws2():
    run_spmd(2, _transformer_worker)
