"""GPU (MI355X) tests for ReducescatterCompressed: the gfx950 mx8_reduce_to
kernel against the CPU torch composite, byte for byte, and the full
pipeline at world size 1 under force_full_path.

The composite (csrc/ops.cpp) is the semantic definition; tests/
test_reducescatter_compressed.py pins it to an independent pure-torch
oracle on the CPU.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SIZES = [1, 31, 32, 33, 4096, 4099, 32 * 257 + 5]


@pytest.fixture(scope="module")
def world1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29554")
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


def _copies(C, n, P, seed0, mixed=True):
    """P quantized copies with mixed per-copy scales; the special groups
    (255 scales included) sit in every copy but copy 1."""
    qs = []
    for r in range(P):
        scale = (1.0, 1e-6, 3e4)[r % 3] if mixed and n > 33 else 1.0
        x = _inputs(n, torch.float32, seed=seed0 + 100 * r, scale=scale)
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
@pytest.mark.parametrize("P", [1, 2, 5, 8])
@pytest.mark.parametrize("n", SIZES)
def test_reduce_to_kernel_matches_composite(world1, n, P, dtype):
    C = world1._C
    pay, sc = _copies(C, n, P, seed0=n)
    ref = C._mx8_reduce_to(pay, sc, n, dtype)
    out = C._mx8_reduce_to(pay.cuda(), sc.cuda(), n, dtype)
    assert out.is_cuda and out.dtype == dtype and out.shape == (n,)
    _match(out.cpu(), ref)
    if n >= 256:
        assert bool(torch.isnan(ref[4 * 32:5 * 32]).all())
        # (a finite sum past the fp16 range is +-inf, never NaN)
        assert not bool(torch.isnan(ref[6 * 32:]).any())
    if P == 1:
        # one copy: the dequantize kernel, bit for bit
        deq = C._mx8_dequantize(pay[0].cuda(), sc[0].cuda(), n, dtype)
        _match(out.cpu(), deq.cpu())


@pytest.mark.parametrize("P", [1, 5])
def test_reduce_to_clamped_exponent_region(world1, P):
    """Groups of magnitude ~1e-38: E clamps at -127 and the dequantized
    values and their sums are fp32 subnormals (ldexpf, fp32 adds)."""
    C = world1._C
    n = 32 * 40 + 7
    g = torch.Generator().manual_seed(17)
    xs = [(torch.randn(41, 32, generator=g) * 4e-38 *
           torch.rand(41, 1, generator=g)).reshape(-1)[:n].contiguous()
          for _ in range(P)]
    assert bool((xs[0].abs() < 2.0 ** -126).any())
    qs = [C._mx8_quantize(x) for x in xs]
    assert int(qs[0][1].min()) == 0  # E = -127 reached
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    ref = C._mx8_reduce_to(pay, sc, n, torch.float32)
    assert bool((ref != 0).any())
    out = C._mx8_reduce_to(pay.cuda(), sc.cuda(), n, torch.float32)
    assert torch.equal(out.cpu().view(torch.uint8), ref.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 33, 4099, 32 * 257 + 5])
def test_reduce_to_writes_exactly_n(world1, n, dtype):
    """Reduce into a buffer with a canary tail: nothing may be written past
    element n (the partial last group holds 32 payload bytes per copy)."""
    C = world1._C
    P = 5
    G = (n + 31) // 32
    pay, sc = _copies(C, n, P, seed0=11)
    ref = C._mx8_reduce_to(pay, sc, n, dtype)
    buf = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")
    out = C._mx8_reduce_to(pay.cuda(), sc.cuda(), n, dtype, out=buf)
    assert out.data_ptr() == buf.data_ptr() and out.shape == (n,)
    _match(buf[:n].cpu(), ref)
    assert bool((buf[n:] == 7.0).all()), "wrote past N"
    # through the scalar path (output base not 16-byte aligned)
    buf2 = torch.full((n + 65,), 7.0, dtype=dtype, device="cuda")
    assert buf2[1:].data_ptr() % 16 != 0
    C._mx8_reduce_to(pay.cuda(), sc.cuda(), n, dtype, out=buf2[1:])
    _match(buf2[1:n + 1].cpu(), ref)
    assert bool((buf2[n + 1:] == 7.0).all()) and float(buf2[0]) == 7.0
    # and with the payload base off by one byte
    pbuf = torch.empty(P * G * 32 + 1, dtype=torch.uint8, device="cuda")
    pv = pbuf[1:].view(P, G * 32)
    pv.copy_(pay)
    assert pv.data_ptr() % 16 != 0
    buf3 = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")
    C._mx8_reduce_to(pv, sc.cuda(), n, dtype, out=buf3)
    _match(buf3[:n].cpu(), ref)
    assert bool((buf3[n:] == 7.0).all()), "wrote past N"


def _composite_reducescatter_w1(C, x):
    """reduce_to(quant(x)) with the CPU composite: what the full path
    computes at world size 1."""
    xc = x.detach().cpu().contiguous()
    p, s = C._mx8_quantize(xc)
    return C._mx8_reduce_to(p.unsqueeze(0), s.unsqueeze(0), xc.numel(),
                            xc.dtype).view(xc.shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1 << 16, (1 << 16) + 3, 33])
def test_full_path_world1(world1, n, dtype):
    m = world1
    comm = m.COMM_WORLD
    x = _inputs(n, dtype, seed=n).cuda().requires_grad_()
    w = _inputs(n, dtype, seed=n + 9).cuda()
    m._C.force_full_path(True)
    try:
        y = comm.ReducescatterCompressed(x, 0)
        y.backward(w)
        torch.cuda.synchronize()
    finally:
        m._C.force_full_path(False)
    assert y.is_cuda and y.dtype == dtype and y.shape == x.shape
    torch.testing.assert_close(y.detach().cpu(),
                               _composite_reducescatter_w1(m._C, x),
                               rtol=0, atol=0, equal_nan=True)
    # backward: the uncompressed allgather, so the gradient is w exactly
    # (NaN positions of w included)
    gw, cw = x.grad.cpu(), w.cpu()
    assert torch.equal(torch.isnan(gw), torch.isnan(cw))
    fin = ~torch.isnan(cw)
    assert torch.equal(gw[fin].view(torch.uint8), cw[fin].view(torch.uint8))


def test_full_path_world1_2d_axis1(world1):
    """before > 1 at world 1: the rank-major packing is the identity."""
    m = world1
    x = _inputs(3 * 40, torch.float32, seed=4).view(3, 40).cuda()
    m._C.force_full_path(True)
    try:
        y = m.COMM_WORLD.ReducescatterCompressed(x, 1)
        torch.cuda.synchronize()
    finally:
        m._C.force_full_path(False)
    assert y.shape == (3, 40)
    torch.testing.assert_close(y.cpu(), _composite_reducescatter_w1(m._C, x),
                               rtol=0, atol=0, equal_nan=True)


def test_world1_default_is_exact_clone(world1):
    m = world1
    comm = m.COMM_WORLD
    x = _inputs(4099, torch.bfloat16, seed=2).cuda()
    y = comm.ReducescatterCompressed(x, 0)
    assert y.data_ptr() != x.data_ptr()
    assert torch.equal(y.cpu().view(torch.uint8), x.cpu().view(torch.uint8))
