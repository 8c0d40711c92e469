"""AlltoallPairwiseCompressed (mxfp8 wire, fused slice permutes): the segments
composites against the pure-torch oracle, SPMD worlds on gloo, autograd,
error checks, the Python surface and the MoE layer's option.

With xs = x_r.index_select(axis, send_order_r) (or x_r), the piece rank `me`
receives from rank r is
    cast(dq(q(flat(contiguous(xs.narrow(axis, sdispl_r[me], M[r][me]))))))
with M the count matrix (M[r][j] = what r sends to j) and q/dq the codec of
test_compressed.py (groups of 32 start at the block's first element). The
pieces are concatenated along the axis in rank order into y, and the result
is y or, with recv_order, out.index_copy_(axis, recv_order, y).
"""

import pytest
import torch

import mpi4torch_amd as m  # module-level so TorchScript resolves m.MPI_Communicator
from spmd import run_spmd
from test_compressed import oracle_quantize, _rand_input
from test_reducescatter_compressed import (_nan_aware_bytes_equal,
                                           _bytes_equal)
from test_allgather_compressed import oracle_codec, _inputs

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MAX_SEGS = int(m._C._MX8_MAX_SEGS_PER_LAUNCH)
# (rows, after, counts)
GEOMS = [
    (1, 32, [3, 0, 2, 1, 4]),      # flat-coincident, with an empty block
    (1, 4, [1, 9, 0, 7]),          # the smallest fp32 vector slice
    (1, 8, [1, 9, 0, 7]),          # the smallest 16-bit vector slice
    (1, 40, [2, 3, 1]),
    (3, 8, [5, 0, 2, 6]),          # rows > 1
    (2, 41, [1, 3, 2]),            # the twins
    (1, 1, [31, 33, 1]),
    (1, 4096, [1, 2]),             # long slices
    (1, 8, [i % 4 for i in range(MAX_SEGS + 1)]),   # more than one launch
]


# ------------------------------ the oracle --------------------------------

def _displs(counts):
    d, out = 0, []
    for c in counts:
        out.append(d)
        d += c
    return out


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _codec(x):
    return oracle_codec(x) if x.numel() else x.clone()


def oracle_segments_quantize(x3, counts, order):
    """[rows, S, after] -> per-segment (payload, scales) or None if empty."""
    xs = x3 if order is None else x3.index_select(1, order)
    out = []
    for d, c in zip(_displs(counts), counts):
        blk = xs[:, d:d + c].contiguous().view(-1)
        out.append(oracle_quantize(blk) if blk.numel() else None)
    return out


def oracle_segments_codec(x3, counts, send_order, recv_order):
    """What quantize_segments -> dequantize_segments gives for [rows, S,
    after]: every segment through the codec, then the scatter."""
    xs = x3 if send_order is None else x3.index_select(1, send_order)
    y = torch.cat([_codec(xs[:, d:d + c])
                   for d, c in zip(_displs(counts), counts)], dim=1)
    if recv_order is None:
        return y
    out = torch.empty_like(y)
    out.index_copy_(1, recv_order, y)
    return out


def oracle_pairwise(xs, axis, M, sorders, rorders):
    """All ranks' inputs -> what AlltoallPairwiseCompressed returns, per
    rank. M[r][j] = slices rank r sends to rank j."""
    P = len(xs)
    gathered = [x if o is None else x.index_select(axis, o)
                for x, o in zip(xs, sorders)]
    outs = []
    for me in range(P):
        y = torch.cat([_codec(gathered[r].narrow(axis, _displs(M[r])[me],
                                                 M[r][me]))
                       for r in range(P)], dim=axis)
        if rorders[me] is not None:
            out = torch.empty_like(y)
            out.index_copy_(axis, rorders[me], y)
            y = out
        outs.append(y)
    return outs


@pytest.fixture(scope="module")
def C():
    return m._C


def _flat(rows, after, counts, dtype, seed, scale=1.0):
    return _inputs(rows * sum(counts) * after, dtype, seed=seed, scale=scale)


# ------------------------- composite vs the oracle ------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}x{len(g[2])}")
def test_segments_composite_matches_oracle(C, geom, permute, dtype):
    rows, after, counts = geom
    S = sum(counts)
    for scale in (1.0, 1e-6, 3e4):
        if dtype == torch.float16 and scale > 1.0:
            scale = 30.0
        x = _flat(rows, after, counts, dtype, seed=S + after, scale=scale)
        order = _perm(S, seed=S) if permute else None
        pay, sc = C._mx8_quantize_segments(x, rows, after, counts,
                                           order=order)
        want = oracle_segments_quantize(x.view(rows, S, after), counts, order)
        G = [(rows * c * after + 31) // 32 for c in counts]
        assert pay.dtype == torch.uint8 and pay.shape == (32 * sum(G),)
        assert sc.dtype == torch.uint8 and sc.shape == (sum(G),)
        goff = 0
        for p, w in enumerate(want):
            if w is not None:
                assert torch.equal(sc[goff:goff + G[p]], w[1]), p
                assert torch.equal(pay[32 * goff:32 * (goff + G[p])], w[0]), p
            goff += G[p]
        rorder = _perm(S, seed=S + 1) if permute else None
        got = C._mx8_dequantize_segments(pay, sc, rows, after, counts, dtype,
                                         order=rorder)
        assert got.shape == (rows, S, after) and got.dtype == dtype
        _nan_aware_bytes_equal(
            got, oracle_segments_codec(x.view(rows, S, after), counts, order,
                                       rorder))


def test_segments_clamped_exponent_region(C):
    """Groups whose amax is tiny or an fp32 subnormal: E clamps at -127."""
    rows, after, counts = 3, 8, [5, 0, 2, 6]
    S = sum(counts)
    x = _rand_input(rows * S * after, torch.float32, seed=400,
                    scale=4e-38).contiguous()
    assert bool((x.abs() < 2.0 ** -126).any())
    order = _perm(S, seed=3)
    pay, sc = C._mx8_quantize_segments(x, rows, after, counts, order=order)
    assert int(sc.min()) == 0 and bool(pay.any())
    want = [w for w in oracle_segments_quantize(x.view(rows, S, after),
                                                counts, order) if w]
    assert torch.equal(pay, torch.cat([w[0] for w in want]))
    assert torch.equal(sc, torch.cat([w[1] for w in want]))
    got = C._mx8_dequantize_segments(pay, sc, rows, after, counts,
                                     torch.float32, order=order)
    _bytes_equal(got, oracle_segments_codec(x.view(rows, S, after), counts,
                                            order, order))


def test_segments_out_arguments(C):
    rows, after, counts = 3, 11, [1, 0, 2]
    S = 3
    x = _rand_input(rows * S * after, torch.bfloat16, seed=1).contiguous()
    order = torch.tensor([2, 0, 1])
    want = C._mx8_quantize_segments(x, rows, after, counts, order=order)
    NG = want[1].numel()
    assert NG == 2 + 3
    pbuf = torch.full((NG * 32 + 8,), 0xAB, dtype=torch.uint8)
    sbuf = torch.full((NG + 8,), 0xAB, dtype=torch.uint8)
    pay, sc = C._mx8_quantize_segments(x, rows, after, counts, order=order,
                                       payload_out=pbuf, scales_out=sbuf)
    assert pay.data_ptr() == pbuf.data_ptr() and sc.data_ptr() == sbuf.data_ptr()
    assert torch.equal(pbuf[:NG * 32], want[0]) and torch.equal(sbuf[:NG], want[1])
    assert bool((pbuf[NG * 32:] == 0xAB).all()) and bool((sbuf[NG:] == 0xAB).all())
    ref = C._mx8_dequantize_segments(pay, sc, rows, after, counts,
                                     torch.bfloat16, order=order)
    obuf = torch.full((rows * S * after + 5,), 7.0, dtype=torch.bfloat16)
    got = C._mx8_dequantize_segments(pay, sc, rows, after, counts,
                                     torch.bfloat16, order=order, out=obuf)
    assert got.data_ptr() == obuf.data_ptr()
    _bytes_equal(obuf[:rows * S * after].view(rows, S, after), ref)
    assert bool((obuf[rows * S * after:] == 7.0).all())
    with pytest.raises(RuntimeError, match="rows\\*S\\*after"):
        C._mx8_quantize_segments(x, 2, 5, counts)
    with pytest.raises(RuntimeError, match="sum\\(counts\\) must equal"):
        C._mx8_quantize_segments(x, rows, after, [1, 1])
    with pytest.raises(RuntimeError, match="sum\\(counts\\) entries"):
        C._mx8_quantize_segments(x, rows, after, counts, order=order[:2])
    with pytest.raises(RuntimeError, match="at least"):
        C._mx8_quantize_segments(x, rows, after, counts, payload_out=pbuf[:9],
                                 scales_out=sbuf)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        C._mx8_quantize_segments(torch.ones(99, dtype=torch.int32), rows,
                                 after, counts)


# ------------------------------ SPMD worlds -------------------------------

def _count_matrix(P, seed):
    """M[r][j]: what rank r sends to rank j, the same on every rank. The
    last rank sends nothing to anyone, rank 0 sends nothing to itself and
    three slices to rank 1."""
    g = torch.Generator().manual_seed(seed)
    M = torch.randint(0, 5, (P, P), generator=g)
    M[P - 1, :] = 0
    M[0, 0] = 0
    M[0, 1] = 3
    return M.tolist()


def _column(M, j):
    return [row[j] for row in M]


def _check_case(comm, rank, world, shape_of, axis, dtype, seed, use_s, use_r,
                scale=1.0):
    M = _count_matrix(world, seed)
    S = [sum(M[r]) for r in range(world)]
    R = [sum(_column(M, r)) for r in range(world)]
    xs = []
    for r in range(world):
        shape = shape_of(S[r])
        n = 1
        for d in shape:
            n *= d
        xs.append(_rand_input(n, dtype, seed=seed + r, scale=scale)
                  .contiguous().view(shape))
    so = [_perm(S[r], seed + 50 + r) if use_s else None for r in range(world)]
    ro = [_perm(R[r], seed + 70 + r) if use_r else None for r in range(world)]
    want = oracle_pairwise(xs, axis, M, so, ro)
    x = xs[rank].clone().requires_grad_()
    y = comm.AlltoallPairwiseCompressed(x, axis, M[rank], _column(M, rank),
                                        send_order=so[rank],
                                        recv_order=ro[rank])
    assert y.grad_fn.name() == "M4AAlltoallPairwiseCompressedBackward"
    _bytes_equal(y.detach(), want[rank])
    # recv_counts=[] has them exchanged on the host: the same result
    y2 = comm.AlltoallPairwiseCompressed(xs[rank], axis, M[rank], [],
                                         so[rank], ro[rank])
    _bytes_equal(y2, want[rank])
    # backward: the same op with counts and orders swapped
    ws = [_rand_input(want[r].numel(), dtype, seed=seed + 500 + r,
                      scale=scale).contiguous().view(want[r].shape)
          for r in range(world)]
    y.backward(ws[rank])
    MT = [_column(M, r) for r in range(world)]
    gwant = oracle_pairwise(ws, axis, MT, ro, so)
    assert x.grad.shape == xs[rank].shape
    _bytes_equal(x.grad, gwant[rank])


def _spmd_worker(rank, world):
    comm = m.COMM_WORLD
    shapes = [(lambda s: (s, 40), 0), (lambda s: (3, s, 8), 1),
              (lambda s: (s, 5), 0)]
    i = 0
    for shape_of, axis in shapes:
        for use_s, use_r in ((False, False), (True, False), (False, True),
                             (True, True)):
            _check_case(comm, rank, world, shape_of, axis,
                        DTYPES[i % 3], seed=1000 + 10 * i, use_s=use_s,
                        use_r=use_r, scale=(1.0, 1e-6, 30.0)[i % 3])
            i += 1
    # negative axis wraps
    _check_case(comm, rank, world, lambda s: (3, s, 8), -2, torch.float32,
                seed=3000, use_s=True, use_r=True)

    # one NaN on rank 0, in the block that goes to rank 1: only the group
    # holding it is NaN, and only on the rank that receives it
    M = _count_matrix(world, 77)
    xs = [_rand_input(sum(M[r]) * 40, torch.float32, seed=70 + r)
          .contiguous().view(sum(M[r]), 40) for r in range(world)]
    d01 = _displs(M[0])[1]
    xs[0][d01 + 1, 0] = float("nan")          # block element 40: group 1
    out = comm.AlltoallPairwiseCompressed(xs[rank], 0, M[rank],
                                          _column(M, rank))
    want = oracle_pairwise(xs, 0, M, [None] * world, [None] * world)[rank]
    _nan_aware_bytes_equal(out, want)
    nan = torch.isnan(out)
    if rank == 1:
        assert int(nan.sum()) == 32
        assert bool(nan.view(-1)[32:64].all())   # rank 0's piece comes first
    else:
        assert int(nan.sum()) == 0

    # the functional wrapper and the tracing passthrough reach the same op
    from mpi4torch_amd import ops
    from mpi4torch_amd.utils import trace

    so = _perm(sum(M[rank]), 5 + rank)
    want = oracle_pairwise(
        xs, 0, M, [_perm(sum(M[r]), 5 + r) for r in range(world)],
        [None] * world)[rank]
    _nan_aware_bytes_equal(
        ops.alltoall_pairwise_compressed(xs[rank], 0, M[rank],
                                         send_order=so), want)
    traced = trace(comm)
    _nan_aware_bytes_equal(
        traced.AlltoallPairwiseCompressed(xs[rank], 0, M[rank],
                                          _column(M, rank), send_order=so),
        want)
    assert [r.op for r in traced.trace_records()] == [
        "AlltoallPairwiseCompressed"]

    # a zero-width slice gives an empty tensor of the output shape
    e = comm.AlltoallPairwiseCompressed(torch.empty(sum(M[rank]), 0), 0,
                                        M[rank], _column(M, rank))
    assert e.shape == (sum(_column(M, rank)), 0)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_spmd(world):
    run_spmd(world, _spmd_worker)


def _debug_collectives_worker(rank, world):
    import os

    comm = m.COMM_WORLD
    os.environ["MPI4TORCH_AMD_DEBUG"] = "1"
    m._C.reload_config()
    try:
        x = _rand_input(2 * 8, torch.float32, seed=rank).view(2, 8)
        assert comm.AlltoallPairwiseCompressed(x, 0, [1, 1], [1, 1]).shape \
            == (2, 8)
        with pytest.raises(RuntimeError, match="desync"):
            comm.AlltoallPairwiseCompressed(torch.ones(2, 3 + rank), 0,
                                            [1, 1], [1, 1])
    finally:
        os.environ.pop("MPI4TORCH_AMD_DEBUG")
        m._C.reload_config()


def test_spmd_debug_collectives_ws2():
    run_spmd(2, _debug_collectives_worker)


# ---------------------- single-process surface checks ---------------------

def test_error_checks():
    comm = m.COMM_WORLD
    f = comm.AlltoallPairwiseCompressed
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        f(torch.ones(4, 4, dtype=torch.int32), 0, [4], [4])
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        f(torch.ones(4, 4, dtype=torch.float64), 0, [4], [4])
    with pytest.raises(RuntimeError, match="send_counts must have world_size"):
        f(torch.ones(4, 4), 0, [2, 2], [4])
    with pytest.raises(RuntimeError, match="recv_counts must have world_size"):
        f(torch.ones(4, 4), 0, [4], [2, 2])
    with pytest.raises(RuntimeError, match="sum of send_counts \\(3\\) must "
                                           "equal the axis size \\(4\\)"):
        f(torch.ones(4, 4), 0, [3], [3])
    good = torch.arange(4)
    with pytest.raises(RuntimeError, match="send_order must be a 1-D tensor "
                                           "of length 4"):
        f(torch.ones(4, 4), 0, [4], [4], send_order=good[:3])
    with pytest.raises(RuntimeError, match="recv_order must be a 1-D tensor "
                                           "of length 4"):
        f(torch.ones(4, 4), 0, [4], [4], recv_order=good.view(2, 2))
    with pytest.raises(RuntimeError, match="send_order must be an int64"):
        f(torch.ones(4, 4), 0, [4], [4], send_order=good.int())
    with pytest.raises(RuntimeError, match="recv_order must be on the "
                                           "tensor's device"):
        f(torch.ones(4, 4), 0, [4], [4], recv_order=good.to("meta"))
    with pytest.raises(RuntimeError, match="send_order must be a "
                                           "permutation of 0..3"):
        f(torch.ones(4, 4), 0, [4], [4], send_order=torch.tensor([0, 1, 1, 3]))
    with pytest.raises(RuntimeError, match="recv_order must be a "
                                           "permutation of 0..3"):
        f(torch.ones(4, 4), 0, [4], [4], recv_order=torch.tensor([0, 1, 2, 4]))
    with pytest.raises(RuntimeError, match="recv_order must be a "
                                           "permutation"):
        f(torch.ones(4, 4), 0, [4], [4], recv_order=torch.tensor([0, 1, 2, -1]))


def test_moe_compression_argument():
    from mpi4torch_amd.models.moe import ExpertParallelMoE

    for bad in ("fp4", "mxfp4", True):
        with pytest.raises(ValueError, match="ExpertParallelMoE: compression "
                                             "must be None or 'mxfp8'"):
            ExpertParallelMoE(8, 2, compression=bad)
    layer = ExpertParallelMoE(32, 2, compression="mxfp8").double()
    with pytest.raises(TypeError, match="float32, bfloat16 or float16 "
                                        "parameters"):
        layer(torch.randn(4, 32, dtype=torch.float64))


def test_world1_default_is_the_exact_permutation():
    comm = m.COMM_WORLD
    # 1/3 is not an e4m3 multiple of any power of two: the codec would move it
    x = torch.full((6, 40), 1.0 / 3.0) * torch.arange(1, 7).view(6, 1)
    assert not torch.equal(oracle_codec(x), x)
    so, ro = _perm(6, 1), _perm(6, 2)
    y = comm.AlltoallPairwiseCompressed(x, 0, [6], [6])
    assert y.data_ptr() != x.data_ptr()
    _bytes_equal(y, x)
    want = torch.empty_like(x)
    want.index_copy_(0, ro, x.index_select(0, so))
    _bytes_equal(comm.AlltoallPairwiseCompressed(x, 0, [6], [], so, ro), want)
    _bytes_equal(comm.AlltoallPairwiseCompressed(x, 0, [6], [6],
                                                 send_order=so), x[so])
    # backward is the inverse permutation, exact
    xg = x.clone().requires_grad_()
    w = torch.randn(6, 40)
    comm.AlltoallPairwiseCompressed(xg, 0, [6], [6], so, ro).backward(w)
    gwant = torch.empty_like(w)
    gwant.index_copy_(0, so, w.index_select(0, ro))
    _bytes_equal(xg.grad, gwant)
    # axis 1 of a 3-D tensor
    t = torch.randn(2, 6, 3)
    _bytes_equal(comm.AlltoallPairwiseCompressed(t, 1, [6], [6], so, None),
                 t[:, so])


def test_world1_forced_full_path_runs_the_codec():
    comm = m.COMM_WORLD
    x = (torch.full((6, 40), 1.0 / 3.0) * torch.arange(1, 7).view(6, 1))
    so, ro = _perm(6, 1), _perm(6, 2)
    m._C.force_full_path(True)
    try:
        y = comm.AlltoallPairwiseCompressed(x, 0, [6], [6], so, ro)
    finally:
        m._C.force_full_path(False)
    want = oracle_pairwise([x], 0, [[6]], [so], [ro])[0]
    _bytes_equal(y, want)
    assert not torch.equal(y, x)


def test_scriptable():
    @torch.jit.script
    def fn(comm: m.MPI_Communicator, t: torch.Tensor,
           order: torch.Tensor) -> torch.Tensor:
        a = comm.AlltoallPairwiseCompressed(t, 0, [5], [5], order, None)
        return comm.AlltoallPairwiseCompressed(a, 0, [5], [5])

    t = torch.randn(5, 8)
    order = _perm(5, 3)
    torch.testing.assert_close(fn(m.COMM_WORLD, t, order), t[order], rtol=0,
                               atol=0)


def test_tracing_wrapper_world1():
    from mpi4torch_amd.utils import trace

    traced = trace(m.COMM_WORLD)
    t = torch.randn(5, 3)
    order = _perm(5, 4)
    _bytes_equal(traced.AlltoallPairwiseCompressed(t, 0, [5], [5],
                                                   recv_order=order),
                 torch.empty_like(t).index_copy_(0, order, t))
    assert [r.op for r in traced.trace_records()] == [
        "AlltoallPairwiseCompressed"]


def test_wire_bytes_helper(C):
    from mpi4torch_amd.utils import mxfp8_alltoall_pairwise_wire_bytes as wb

    # 3 slices of 40 -> 120 elements -> 4 groups; 1 slice -> 2 groups
    assert wb([3, 0, 1], 40, 1) == 33 * 4 + 33 * 2
    assert wb([3, 0, 1], 40, 0) == 33 * 2
    assert wb([7], 40, 0) == 0
    assert wb([0, 0], 40, 1) == 0
    # it is the size of the tensors the composite produces for the peers
    counts, rows, after, rank = [2, 5, 0, 1], 3, 7, 1
    x = torch.randn(rows * sum(counts) * after)
    pay, sc = C._mx8_quantize_segments(x, rows, after, counts)
    G = [(rows * c * after + 31) // 32 for c in counts]
    assert pay.numel() + sc.numel() == 33 * sum(G)
    assert wb(counts, rows * after, rank) == 33 * (sum(G) - G[rank])


# --------------------------------- the MoE --------------------------------

def _moe_reference_forward(layer, x):
    """ExpertParallelMoE.forward with the oracle codec applied to x_sorted
    before an uncompressed dispatch and to the expert output before an
    uncompressed combine. With d_model == 32 every group is one token row,
    so the codec of the whole tensor is the codec of every block."""
    comm = layer.comm
    N, D = x.shape
    assert D == 32
    P = comm.size
    gates = torch.softmax(layer.router(x), dim=-1)
    expert = torch.argmax(gates, dim=-1)
    gate = gates.gather(1, expert.unsqueeze(1)).squeeze(1)
    owner = expert // layer.experts_per_rank
    order = torch.argsort(owner, stable=True)
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(N)
    x_sorted = _codec(x.index_select(0, order))
    send_counts = torch.bincount(owner, minlength=P).tolist()
    recv_counts = layer._recv_counts(send_counts)
    dispatched = comm.AlltoallPairwise(x_sorted, 0, send_counts, recv_counts)
    eid = comm.AlltoallPairwise(
        expert.index_select(0, order).to(torch.float64).unsqueeze(1), 0,
        send_counts, recv_counts).squeeze(1).long()
    local_eid = eid - comm.rank * layer.experts_per_rank
    out = torch.zeros_like(dispatched)
    for e in range(layer.experts_per_rank):
        mask = local_eid == e
        if bool(mask.any()):
            idx = mask.nonzero(as_tuple=True)[0]
            out = out.index_copy(
                0, idx, layer.experts[e](dispatched.index_select(0, idx)))
    combined = comm.AlltoallPairwise(_codec(out), 0, recv_counts, send_counts)
    return combined.index_select(0, inverse) * gate.unsqueeze(1)


def _moe_worker(rank, world):
    from mpi4torch_amd.models.moe import ExpertParallelMoE

    d_model, n_experts, N = 32, 2 * world, 24
    torch.manual_seed(5)
    layer = ExpertParallelMoE(d_model, n_experts, d_hidden=16,
                              compression="mxfp8")
    assert layer.compression == "mxfp8"
    torch.manual_seed(40 + rank)
    x = torch.randn(N, d_model, requires_grad=True)
    y = layer(x)
    with torch.no_grad():
        want = _moe_reference_forward(layer, x)
    assert torch.equal(y.detach(), want)
    (y ** 2).sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    assert bool(torch.isfinite(layer.router.weight.grad).all())
    assert bool(layer.router.weight.grad.abs().sum() > 0)
    populated = 0
    for p in layer.experts.parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all())
            populated += int(p.grad.abs().sum() > 0)
    assert populated > 0

    # the option off: the layer is what it is without the argument
    torch.manual_seed(5)
    off = ExpertParallelMoE(d_model, n_experts, d_hidden=16, compression=None)
    torch.manual_seed(5)
    plain = ExpertParallelMoE(d_model, n_experts, d_hidden=16)
    assert off.compression is None and plain.compression is None
    with torch.no_grad():
        a, b = off(x), plain(x)
    assert torch.equal(a, b)
    assert not torch.equal(a, y.detach())          # it really compressed


def test_moe_ws2():
    run_spmd(2, _moe_worker)
