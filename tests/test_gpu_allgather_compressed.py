"""GPU (MI355X) tests for AllgatherCompressed: the gfx950
mx8_dequantize_blocks kernel against the CPU torch composite, byte for byte,
and the full pipeline at world size 1 under force_full_path.

The composite (csrc/ops.cpp) is the semantic definition; tests/
test_allgather_compressed.py pins it to an independent pure-torch oracle on
the CPU.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (rows, row_elems): the single flat stream (1,32); a partial last group per
# block; groups straddling rows on the vector path (3,40) (5,36) (4,1000);
# the smallest vector row, (7,4) for fp32 and (7,8) for 16-bit ((7,4) takes
# the general twin for 16-bit, with rows shorter than a chunk); the odd-row
# general twin (3,41), whose segments have head, chunk and tail parts
GEOMS = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 4099), (1, 32 * 257 + 5),
         (3, 40), (3, 41), (5, 36), (7, 4), (7, 8), (2, 4096), (4, 1000)]


@pytest.fixture(scope="module")
def world1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29557")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    import torch.distributed as dist

    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    import mpi4torch_amd as m

    m.init()
    return m


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


def _blocks(C, L, P, seed0, mixed=True):
    """P quantized blocks of L elements with mixed per-block scales; the
    special groups (255 scales included) sit in every block but block 1."""
    qs = []
    for r in range(P):
        scale = (1.0, 1e-6, 3e4)[r % 3] if mixed and L > 33 else 1.0
        x = _inputs(L, torch.float32, seed=seed0 + 100 * r, scale=scale)
        if r == 1:
            x = torch.nan_to_num(x, nan=0.5, posinf=1.0)
        qs.append(C._mx8_quantize(x))
    return torch.stack([q[0] for q in qs]), torch.stack([q[1] for q in qs])


def _match(out, ref):
    """NaNs at the same positions, the finite part byte for byte (signed
    zeros included)."""
    assert out.dtype == ref.dtype and out.shape == ref.shape
    torch.testing.assert_close(out, ref, rtol=0, atol=0, equal_nan=True)
    fin = ~torch.isnan(ref)
    assert torch.equal(out[fin].view(torch.uint8), ref[fin].view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("geom", GEOMS)
def test_dequantize_blocks_kernel_matches_composite(world1, geom, P, dtype):
    C = world1._C
    rows, row_elems = geom
    L = rows * row_elems
    pay, sc = _blocks(C, L, P, seed0=L)
    ref = C._mx8_dequantize_blocks(pay, sc, rows, row_elems, dtype)
    out = C._mx8_dequantize_blocks(pay.cuda(), sc.cuda(), rows, row_elems,
                                   dtype)
    assert out.is_cuda and out.dtype == dtype
    assert out.shape == (rows, P, row_elems)
    _match(out.cpu(), ref)
    if L >= 256:
        flat = ref[:, 0, :].reshape(-1)
        assert bool(torch.isnan(flat[4 * 32:6 * 32]).all())
        assert not bool(torch.isnan(flat[6 * 32:]).any())
    if rows == 1:
        # one row: every block is the dequantize kernel's, bit for bit
        for r in range(P):
            deq = C._mx8_dequantize(pay[r].cuda(), sc[r].cuda(), L, dtype)
            _match(out[0, r].cpu(), deq.cpu())


@pytest.mark.parametrize("P", [1, 5])
def test_dequantize_blocks_clamped_exponent_region(world1, P):
    """Groups of magnitude ~1e-38: E clamps at -127 and the dequantized
    values are fp32 subnormals (ldexpf)."""
    C = world1._C
    rows, row_elems = 3, 429               # L = 32*40 + 7, general twin
    L = rows * row_elems
    g = torch.Generator().manual_seed(17)
    xs = [(torch.randn(41, 32, generator=g) * 4e-38 *
           torch.rand(41, 1, generator=g)).reshape(-1)[:L].contiguous()
          for _ in range(P)]
    assert bool((xs[0].abs() < 2.0 ** -126).any())
    qs = [C._mx8_quantize(x) for x in xs]
    assert int(qs[0][1].min()) == 0  # E = -127 reached
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    for r_, re_ in ((rows, row_elems), (1, L), (9, 143)):
        ref = C._mx8_dequantize_blocks(pay, sc, r_, re_, torch.float32)
        assert bool((ref != 0).any())
        out = C._mx8_dequantize_blocks(pay.cuda(), sc.cuda(), r_, re_,
                                       torch.float32)
        assert torch.equal(out.cpu().view(torch.uint8), ref.view(torch.uint8))
    # and on the vector path: L = 1280, rows of 320
    pay, sc = pay[:, :1280].contiguous(), sc[:, :40].contiguous()
    ref = C._mx8_dequantize_blocks(pay, sc, 4, 320, torch.float32)
    out = C._mx8_dequantize_blocks(pay.cuda(), sc.cuda(), 4, 320,
                                   torch.float32)
    assert torch.equal(out.cpu().view(torch.uint8), ref.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", [(1, 33), (3, 40), (3, 41),
                                  (1, 32 * 257 + 5)])
def test_dequantize_blocks_writes_exactly_n(world1, geom, dtype):
    """Dequantize into a buffer with a canary tail: nothing may be written
    past the last element (each block's partial last group holds 32 payload
    bytes)."""
    C = world1._C
    P = 5
    rows, row_elems = geom
    L = rows * row_elems
    N = P * L
    Gb = (L + 31) // 32
    pay, sc = _blocks(C, L, P, seed0=11)
    ref = C._mx8_dequantize_blocks(pay, sc, rows, row_elems, dtype)
    ref = ref.reshape(-1)
    buf = torch.full((N + 64,), 7.0, dtype=dtype, device="cuda")
    out = C._mx8_dequantize_blocks(pay.cuda(), sc.cuda(), rows, row_elems,
                                   dtype, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    assert out.shape == (rows, P, row_elems)
    _match(buf[:N].cpu(), ref)
    assert bool((buf[N:] == 7.0).all()), "wrote past N"
    # through the general twin (output base not 16-byte aligned)
    buf2 = torch.full((N + 65,), 7.0, dtype=dtype, device="cuda")
    assert buf2[1:].data_ptr() % 16 != 0
    C._mx8_dequantize_blocks(pay.cuda(), sc.cuda(), rows, row_elems, dtype,
                             out=buf2[1:])
    _match(buf2[1:N + 1].cpu(), ref)
    assert bool((buf2[N + 1:] == 7.0).all()) and float(buf2[0]) == 7.0
    # and with the payload base off by one byte
    pbuf = torch.empty(P * Gb * 32 + 1, dtype=torch.uint8, device="cuda")
    pv = pbuf[1:].view(P, Gb * 32)
    pv.copy_(pay)
    assert pv.data_ptr() % 16 != 0
    buf3 = torch.full((N + 64,), 7.0, dtype=dtype, device="cuda")
    C._mx8_dequantize_blocks(pv, sc.cuda(), rows, row_elems, dtype, out=buf3)
    _match(buf3[:N].cpu(), ref)
    assert bool((buf3[N:] == 7.0).all()), "wrote past N"


def _composite_codec(C, x):
    """dq(q(x)) with the CPU composite: what the full path computes at world
    size 1."""
    xc = x.detach().cpu().contiguous()
    p, s = C._mx8_quantize(xc)
    return C._mx8_dequantize(p, s, xc.numel(), xc.dtype).view(xc.shape)


def _composite_reducescatter_w1(C, x):
    """reduce_to(quant(x)) with the CPU composite: the backward at world
    size 1."""
    xc = x.detach().cpu().contiguous()
    p, s = C._mx8_quantize(xc)
    return C._mx8_reduce_to(p.unsqueeze(0), s.unsqueeze(0), xc.numel(),
                            xc.dtype).view(xc.shape)


def _full_path(m, x, w, axis):
    m._C.force_full_path(True)
    try:
        y = m.COMM_WORLD.AllgatherCompressed(x, axis)
        y.backward(w)
        torch.cuda.synchronize()
    finally:
        m._C.force_full_path(False)
    assert y.is_cuda and y.dtype == x.dtype and y.shape == x.shape
    _match(y.detach().cpu(), _composite_codec(m._C, x))
    # backward: the compressed reduce-scatter of w at world 1
    _match(x.grad.cpu(), _composite_reducescatter_w1(m._C, w))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1 << 16, (1 << 16) + 3, 33])
def test_full_path_world1(world1, n, dtype):
    x = _inputs(n, dtype, seed=n).cuda().requires_grad_()
    w = _inputs(n, dtype, seed=n + 9).cuda()
    _full_path(world1, x, w, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_path_world1_2d_axis1(world1, dtype):
    """before > 1: rows of 40 elements, groups straddling the rows."""
    x = _inputs(3 * 40, dtype, seed=4).view(3, 40).cuda().requires_grad_()
    w = _inputs(3 * 40, dtype, seed=5).view(3, 40).cuda()
    _full_path(world1, x, w, 1)


def test_world1_default_is_exact_clone(world1):
    m = world1
    comm = m.COMM_WORLD
    x = _inputs(4099, torch.bfloat16, seed=2).cuda()
    y = comm.AllgatherCompressed(x, 0)
    assert y.data_ptr() != x.data_ptr()
    assert torch.equal(y.cpu().view(torch.uint8), x.cpu().view(torch.uint8))
