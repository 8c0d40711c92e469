"""AlltoallPairwiseCompressedIndexed on the CPU: the mx8_dequantize_combine
composite against a plain reference (the numpy float64 oracle's dequantize,
then a Python loop of ordered fp32 adds), the table builder on out-of-contract
input, the op's checks, its backward, the exact world of one, and
ExpertParallelMoE(top_k=2). The GPU file feeds the same cases to the kernel.
"""

import numpy as np
import pytest
import torch

import mpi4torch_amd as m
import mx8_oracles as mo
from spmd import run_spmd
from test_alltoall_pairwise_compressed import _codec

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (after, counts, fan)
GEOMS = [
    (4, [1, 9, 0, 7], 2),      # smallest fp32 chunk; the twin for 16-bit
    (8, [1, 9, 0, 7], 3),      # L_p % 32 != 0 (goff padding), an empty segment
    (40, [2, 3, 1], 2),        # slices that start mid-group
    (41, [1, 3, 2], 2),        # the twin
    (1, [31, 33, 1], 8),       # the twin
    (4096, [1, 2], 2),
    (8, [i % 4 for i in range(33)], 3),
]
GEOM_IDS = [f"{g[0]}x{len(g[1])}x{g[2]}" for g in GEOMS]


def wire(after, counts, seed):
    """Random payload and scale bytes of the segments: no NaN codes, scales
    within 2^+-7 of one so that sums round but stay finite."""
    G = sum((c * after + 31) // 32 for c in counts)
    g = torch.Generator().manual_seed(seed)
    pay = torch.randint(0, 256, (G * 32,), generator=g, dtype=torch.uint8)
    pay[(pay & 0x7f) == 0x7f] = 0x31
    sc = torch.randint(120, 135, (G,), generator=g, dtype=torch.uint8)
    return pay, sc


def fan_index(R, fan, seed):
    """(index, out_size): destinations with fan sources, with fewer and with
    none, the sources of a destination scattered over the stream."""
    idx = torch.arange(R) // fan
    if R % fan == 0:
        idx[R - 1] = idx[R - 1] + 1
    out_size = int(idx.max()) + 2
    n = torch.bincount(idx, minlength=out_size)
    assert bool((n == fan).any() and ((n > 0) & (n < fan)).any()
                and (n == 0).any())
    return idx[torch.randperm(R, generator=torch.Generator()
                              .manual_seed(seed))], out_size


def reference(pay, sc, after, counts, index, out_size, fan, dtype):
    rows, goff = [], 0
    for c in counts:
        G = (c * after + 31) // 32
        if c:
            d = mo._f32(mo.dequantize(pay[32 * goff:32 * (goff + G)].numpy(),
                                      sc[goff:goff + G].numpy()))
            rows += list(torch.from_numpy(d).view(-1)[:c * after]
                         .view(c, after))
        goff += G
    acc = torch.zeros(out_size, after)
    seen = [0] * out_size
    for i, s in enumerate(index.tolist()):
        if 0 <= s < out_size and seen[s] < fan:
            acc[s] = rows[i] if seen[s] == 0 else acc[s] + rows[i]
            seen[s] += 1
    return acc.to(dtype)


def nan_case():
    """(8, [1, 9, 0, 7], 3) with a 255 scale on segment 1's first group and
    the two NaN payload codes in segment 3."""
    after, counts, fan = GEOMS[1]
    pay, sc = wire(after, counts, 77)
    sc[1] = 255
    pay[32 * 4 + 5], pay[32 * 4 + 9] = 0x7f, 0xff
    return (pay, sc, after, counts) + fan_index(sum(counts), fan, 78) + (fan,)


def order_probe():
    """Destination 0 adds (1, 2^25, -2^25) and gives 0, destination 1 adds
    (-2^25, 2^25, 1) and gives 1; every other order swaps an outcome."""
    x = np.zeros((6, 32), dtype=np.float32)
    x[:, 0] = [1.0, 2.0 ** 25, -2.0 ** 25, -2.0 ** 25, 2.0 ** 25, 1.0]
    pay, sc = mo.quantize(x)
    return (torch.from_numpy(pay), torch.from_numpy(sc), 32, [4, 2],
            torch.tensor([0, 0, 0, 1, 1, 1]), 2, 3)


def dropped_case():
    """Entries of -1 and out_size, and a fourth source for a destination of
    fan 3: all dropped."""
    after, counts, fan = GEOMS[1]
    pay, sc = wire(after, counts, 5)
    index, out_size = fan_index(sum(counts), fan, 6)
    index[2], index[7] = -1, out_size
    index[index == 3] = 0
    assert int((index == 0).sum()) > fan
    return pay, sc, after, counts, index, out_size, fan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_composite_matches_reference(geom, dtype):
    after, counts, fan = geom
    pay, sc = wire(after, counts, after)
    index, out_size = fan_index(sum(counts), fan, after + 1)
    got = m._C._mx8_dequantize_combine(pay, sc, after, counts, index, out_size,
                                       fan, dtype)
    mo.nan_aware_equal(got, reference(pay, sc, after, counts, index, out_size,
                                      fan, dtype))


@pytest.mark.parametrize("case", [nan_case, order_probe, dropped_case])
def test_composite_special_cases(case):
    pay, sc, after, counts, index, out_size, fan = case()
    want = reference(pay, sc, after, counts, index, out_size, fan,
                     torch.float32)
    out = torch.full((out_size * after + 8,), 7.0)
    got = m._C._mx8_dequantize_combine(pay, sc, after, counts, index, out_size,
                                       fan, torch.float32, out=out)
    mo.nan_aware_equal(got, want)
    assert bool((out[out_size * after:] == 7.0).all())
    if case is nan_case:
        assert 0 < int(torch.isnan(want).sum()) <= 34
    if case is order_probe:
        assert (float(want[0, 0]), float(want[1, 0])) == (0.0, 1.0)


def test_error_checks():
    f = m.COMM_WORLD.AlltoallPairwiseCompressedIndexed
    x, i4 = torch.ones(4, 4), torch.tensor([0, 1, 1, 3])
    for match, args, kw in [
        ("out_size is required with a recv_index", (x, 0, [4], [4]),
         dict(recv_index=i4)),
        ("every dimension before the axis must have size 1",
         (torch.ones(2, 4, 4), 1, [4], [4]), dict(recv_index=i4, out_size=4)),
        ("a slice occurs 2 times in send_index, more than max_repeat = 1",
         (x, 0, [4], [4]), dict(send_index=i4)),
        ("a slice occurs 2 times in recv_index", (x, 0, [4], [4]),
         dict(recv_index=i4, out_size=4)),
        ("recv_index entries must lie in \\[0, 3\\)", (x, 0, [4], [4]),
         dict(recv_index=i4, out_size=3, max_repeat=2)),
        ("send_index must be a 1-D tensor of length 4", (x, 0, [4], [4]),
         dict(send_index=i4[:3])),
        ("recv_index must be a 1-D tensor of length 4", (x, 0, [4], [4]),
         dict(recv_index=i4.view(2, 2), out_size=4)),
        ("send_index must be an int64", (x, 0, [4], [4]),
         dict(send_index=i4.int())),
        ("recv_index must be on the tensor's device", (x, 0, [4], [4]),
         dict(recv_index=i4.to("meta"), out_size=4)),
        ("without a send_index the sum of send_counts \\(3\\) must equal the "
         "axis size \\(4\\)", (x, 0, [3], [3]), {}),
        ("float32, bfloat16 and float16", (x.double(), 0, [4], [4]), {}),
        ("Indexed: send_counts must have world_size entries",
         (x, 0, [2, 2], [4]), {}),
        ("Indexed: recv_counts must have world_size entries",
         (x, 0, [4], [2, 2]), {}),
        ("Indexed: negative send count -1", (x, 0, [-1], [4]), {}),
        ("Indexed: negative recv count -2", (x, 0, [4], [-2]), {}),
        ("Indexed: max_repeat must be >= 1, got 0", (x, 0, [4], [4]),
         dict(max_repeat=0)),
        ("Indexed: out_size must be >= 0, got -1", (x, 0, [4], [4]),
         dict(out_size=-1)),
    ]:
        with pytest.raises(RuntimeError, match=match):
            f(*args, **kw)
    # the kernel binding under the combine tail
    pay, sc = wire(8, [4], 1)
    for match, args in [
        ("_mx8_dequantize_combine: after and fan must be >= 1 and out_size "
         ">= 0", (pay, sc, 8, [4], i4, 4, 0, torch.float32)),
        ("_mx8_dequantize_combine expects flat contiguous uint8 payload "
         "\\[32\\*sum\\(G\\)\\] and scales \\[sum\\(G\\)\\]",
         (pay[:-1], sc, 8, [4], i4, 4, 2, torch.float32)),
        ("_mx8_dequantize_combine: index must be a contiguous int64 tensor "
         "of sum\\(counts\\) entries on the payload's device",
         (pay, sc, 8, [4], i4[:3], 4, 2, torch.float32)),
    ]:
        with pytest.raises(RuntimeError, match=match):
            m._C._mx8_dequantize_combine(*args)


def _grad_case(comm, rank, world):
    """Top-2 dispatch and combine with data-dependent counts: autograd through
    the op is, byte for byte, the op on the gradient with swapped arguments."""
    g = torch.Generator().manual_seed(50 + rank)
    N, D, k = 11, 40, 2
    owner = torch.randint(0, world, (N * k,), generator=g)
    order = torch.argsort(owner, stable=True)
    tok = order // k
    send = torch.bincount(owner, minlength=world).tolist()
    x = torch.randn(N, D, generator=g, requires_grad=True)
    f = comm.AlltoallPairwiseCompressedIndexed
    y = f(x, 0, send, [], send_index=tok, max_repeat=k)
    recv = send if world == 1 else [int(v) for v in comm.Allgather(
        torch.tensor([send], dtype=torch.float64), 0)[:, rank]]
    assert y.shape == (sum(recv), D)
    w = torch.randn(y.shape, generator=g)
    gx, = torch.autograd.grad(y, x, w)
    want = f(w, 0, recv, send, recv_index=tok, out_size=N, max_repeat=k)
    assert torch.equal(gx.view(torch.int32), want.view(torch.int32))
    yd = y.detach().requires_grad_()
    z = f(yd, 0, recv, send, recv_index=tok, out_size=N, max_repeat=k)
    v = torch.randn(N, D, generator=g)
    gy, = torch.autograd.grad(z, yd, v)
    want = f(v, 0, send, recv, send_index=tok, max_repeat=k)
    assert torch.equal(gy.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(z.detach(), k * x.detach())   # the codec ran


def _grad_worker(rank, world):
    _grad_case(m.COMM_WORLD, rank, world)


def test_backward_is_the_swapped_op_world1_full_path():
    m._C.force_full_path(True)
    try:
        _grad_case(m.COMM_WORLD, 0, 1)
    finally:
        m._C.force_full_path(False)


def test_backward_is_the_swapped_op_ws2():
    run_spmd(2, _grad_worker)


def test_world1_default_is_exact():
    f = m.COMM_WORLD.AlltoallPairwiseCompressedIndexed
    x = torch.full((5, 40), 1.0 / 3.0) * torch.arange(1, 6).view(5, 1)
    tok = torch.tensor([4, 0, 0, 2, 4, 4])
    y = f(x, 0, [6], [6], send_index=tok, max_repeat=3)
    assert torch.equal(y, x[tok])
    z = f(y.bfloat16(), 0, [6], [6], recv_index=tok, out_size=6, max_repeat=3)
    want = torch.zeros(6, 40)
    want[0] = y.bfloat16()[1].float() + y.bfloat16()[2].float()
    want[2] = y[3]
    want[4] = (y.bfloat16()[0].float() + y.bfloat16()[4].float()
               + y.bfloat16()[5].float())
    assert torch.equal(z.view(torch.int16), want.bfloat16().view(torch.int16))


class _CodecComm:
    """A communicator whose AlltoallPairwise sends token rows through the
    oracle codec first (d_model == 32: every row is one group)."""

    def __init__(self, comm):
        self.size, self.rank, self._comm = comm.size, comm.rank, comm

    def AlltoallPairwise(self, t, axis, send, recv):
        t = _codec(t) if t.shape[1] == 32 else t
        return self._comm.AlltoallPairwise(t, axis, send, recv)


def _layers(**kw):
    from mpi4torch_amd.models.moe import ExpertParallelMoE

    out = []
    for compression in (None, "mxfp8"):
        torch.manual_seed(5)
        out.append(ExpertParallelMoE(32, 4, d_hidden=16,
                                     compression=compression, **kw))
    return out


def test_moe_top2_world1_is_bit_exact():
    plain, mx8 = _layers(top_k=2)
    x = torch.randn(24, 32, generator=torch.Generator().manual_seed(1))
    grads = []
    for layer in (plain, mx8):
        xg = x.clone().requires_grad_()
        y = layer(xg)
        (y ** 2).sum().backward()
        grads.append([y.detach(), xg.grad] +
                     [p.grad for p in layer.parameters()])
    assert all(g is not None for g in grads[1])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_moe_top2_full_path_matches_codec_reference():
    """test_moe_ws2's comparison for top-1, exact equality with the layer
    whose uncompressed transfers carry oracle-coded rows, at top_k=2."""
    plain, mx8 = _layers(top_k=2)
    plain.comm = _CodecComm(plain.comm)
    x = torch.randn(24, 32, generator=torch.Generator().manual_seed(2))
    m._C.force_full_path(True)
    try:
        with torch.no_grad():
            want = plain(x)
        xg = x.clone().requires_grad_()
        y = mx8(xg)
        (y ** 2).sum().backward()
    finally:
        m._C.force_full_path(False)
    assert torch.equal(y.detach(), want)
    with torch.no_grad():
        assert not torch.equal(_layers(top_k=2)[0](x), want)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all())
               for p in mx8.parameters())
    assert bool(torch.isfinite(xg.grad).all())


def test_moe_top1_is_the_layer_without_the_argument():
    x = torch.randn(24, 32, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        for a, b in zip(_layers(top_k=1), _layers()):
            assert torch.equal(a(x), b(x))
    from mpi4torch_amd.models.moe import ExpertParallelMoE
    with pytest.raises(ValueError, match="top_k must lie in"):
        ExpertParallelMoE(32, 4, top_k=5)
