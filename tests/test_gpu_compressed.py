"""GPU (MI355X) tests for the mxfp8 compressed allreduce: each gfx950 codec
kernel against the CPU torch composite, byte for byte, and the full
pipeline at world size 1 under force_full_path.

The composite (csrc/ops.cpp) is the semantic definition; tests/
test_compressed.py pins it to an independent pure-torch oracle on the CPU.
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
    os.environ.setdefault("MASTER_PORT", "29553")
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


def _bytes_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_quantize_kernel_matches_composite(world1, n, dtype):
    C = world1._C
    for scale in (1.0, 1e-6, 3e4):
        x = _inputs(n, dtype, seed=n, scale=scale)
        p_ref, s_ref = C._mx8_quantize(x)
        p, s = C._mx8_quantize(x.cuda())
        assert p.is_cuda and p.dtype == torch.uint8 and s.dtype == torch.uint8
        _bytes_equal(s.cpu(), s_ref)
        _bytes_equal(p.cpu(), p_ref)


@pytest.mark.parametrize("P", [1, 5])
def test_kernels_clamped_exponent_region(world1, P):
    """Groups of magnitude ~1e-38 (amax tiny or an fp32 subnormal): E clamps
    at -127 and dequantized values are fp32 subnormals, which the kernels
    must produce and consume exactly (ldexpf, fp32 adds)."""
    C = world1._C
    n = 32 * 40 + 7
    g = torch.Generator().manual_seed(17)
    xs = [(torch.randn(41, 32, generator=g) * 4e-38 *
           torch.rand(41, 1, generator=g)).reshape(-1)[:n].contiguous()
          for _ in range(P)]
    assert bool((xs[0].abs() < 2.0 ** -126).any())
    qs = [C._mx8_quantize(x) for x in xs]
    assert int(qs[0][1].min()) == 0  # E = -127 reached
    for x, (p_ref, s_ref) in zip(xs, qs):
        p, s = C._mx8_quantize(x.cuda())
        _bytes_equal(s.cpu(), s_ref)
        _bytes_equal(p.cpu(), p_ref)
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    p_ref, s_ref = C._mx8_reduce(pay, sc)
    p, s = C._mx8_reduce(pay.cuda(), sc.cuda())
    _bytes_equal(s.cpu(), s_ref)
    _bytes_equal(p.cpu(), p_ref)
    ref = C._mx8_dequantize(p_ref, s_ref, n, torch.float32)
    assert bool((ref != 0).any())
    out = C._mx8_dequantize(p, s, n, torch.float32)
    _bytes_equal(out.cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_kernel_misaligned_input(world1, dtype):
    C = world1._C
    big = _inputs(4099 + 1, dtype, seed=3).cuda()
    x = big[1:]  # contiguous, base pointer not 16-byte aligned
    assert x.data_ptr() % 16 != 0
    p_ref, s_ref = C._mx8_quantize(x.cpu())
    p, s = C._mx8_quantize(x)
    _bytes_equal(s.cpu(), s_ref)
    _bytes_equal(p.cpu(), p_ref)


@pytest.mark.parametrize("P", [1, 2, 5, 8])
@pytest.mark.parametrize("n", SIZES)
def test_reduce_kernel_matches_composite(world1, n, P):
    C = world1._C
    qs = [C._mx8_quantize(_inputs(n, torch.float32, seed=100 * r + n,
                                  scale=(1.0, 1e-6, 3e4)[r % 3] if n > 33
                                  else 1.0))
          for r in range(P)]
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    p_ref, s_ref = C._mx8_reduce(pay, sc)
    p, s = C._mx8_reduce(pay.cuda(), sc.cuda())
    _bytes_equal(s.cpu(), s_ref)
    _bytes_equal(p.cpu(), p_ref)


def test_reduce_kernel_misaligned(world1):
    C = world1._C
    n, P = 4099, 5
    G = (n + 31) // 32
    qs = [C._mx8_quantize(_inputs(n, torch.float32, seed=7 + r))
          for r in range(P)]
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    p_ref, s_ref = C._mx8_reduce(pay, sc)
    # payload base off by one byte: the scalar path
    buf = torch.empty(P * G * 32 + 1, dtype=torch.uint8, device="cuda")
    pv = buf[1:].view(P, G * 32)
    pv.copy_(pay)
    assert pv.data_ptr() % 16 != 0
    p, s = C._mx8_reduce(pv, sc.cuda())
    _bytes_equal(s.cpu(), s_ref)
    _bytes_equal(p.cpu(), p_ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_dequantize_kernel_matches_composite(world1, n, dtype):
    C = world1._C
    x = _inputs(n, dtype, seed=n + 1)
    p, s = C._mx8_quantize(x)
    ref = C._mx8_dequantize(p, s, n, dtype)
    out = C._mx8_dequantize(p.cuda(), s.cuda(), n, dtype)
    assert out.is_cuda and out.dtype == dtype and out.shape == (n,)
    torch.testing.assert_close(out.cpu(), ref, rtol=0, atol=0, equal_nan=True)
    # the finite part byte for byte (signed zeros included)
    fin = ~torch.isnan(ref)
    _bytes_equal(out.cpu()[fin], ref[fin])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 33, 4099, 32 * 257 + 5])
def test_dequantize_writes_exactly_n(world1, n, dtype):
    """Dequantize into a buffer with a canary tail: nothing may be written
    past element n (the partial last group holds 32 payload bytes)."""
    C = world1._C
    x = _inputs(n, dtype, seed=11)
    p, s = C._mx8_quantize(x)
    ref = C._mx8_dequantize(p, s, n, dtype)
    buf = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")
    out = C._mx8_dequantize(p.cuda(), s.cuda(), n, dtype, out=buf)
    assert out.data_ptr() == buf.data_ptr() and out.shape == (n,)
    torch.testing.assert_close(buf[:n].cpu(), ref, rtol=0, atol=0,
                               equal_nan=True)
    assert bool((buf[n:] == 7.0).all()), "wrote past N"
    # and through the scalar path (output base not 16-byte aligned)
    buf2 = torch.full((n + 65,), 7.0, dtype=dtype, device="cuda")
    C._mx8_dequantize(p.cuda(), s.cuda(), n, dtype, out=buf2[1:])
    torch.testing.assert_close(buf2[1:n + 1].cpu(), ref, rtol=0, atol=0,
                               equal_nan=True)
    assert bool((buf2[n + 1:] == 7.0).all()) and float(buf2[0]) == 7.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_kernel_misaligned_payload(world1, dtype):
    C = world1._C
    n = 4099
    G = (n + 31) // 32
    x = _inputs(n, dtype, seed=5)
    p, s = C._mx8_quantize(x)
    ref = C._mx8_dequantize(p, s, n, dtype)
    buf = torch.empty(G * 32 + 1, dtype=torch.uint8, device="cuda")
    pv = buf[1:]
    pv.copy_(p)
    out = C._mx8_dequantize(pv, s.cuda(), n, dtype)
    torch.testing.assert_close(out.cpu(), ref, rtol=0, atol=0, equal_nan=True)


def _composite_allreduce_w1(C, x):
    """dequant(reduce(quant(x))) with the CPU composite: what the full path
    computes at world size 1."""
    xc = x.detach().cpu().contiguous()
    p, s = C._mx8_quantize(xc)
    rp, rs = C._mx8_reduce(p.unsqueeze(0), s.unsqueeze(0))
    return C._mx8_dequantize(rp, rs, xc.numel(), xc.dtype).view(xc.shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1 << 16, (1 << 16) + 3, 33])
def test_full_path_world1(world1, n, dtype):
    m = world1
    comm = m.COMM_WORLD
    x = _inputs(n, dtype, seed=n).cuda().requires_grad_()
    w = _inputs(n, dtype, seed=n + 9).cuda()
    m._C.force_full_path(True)
    try:
        y = comm.AllreduceCompressed(x)
        y.backward(w)
        torch.cuda.synchronize()
    finally:
        m._C.force_full_path(False)
    assert y.is_cuda and y.dtype == dtype and y.shape == x.shape
    torch.testing.assert_close(y.detach().cpu(),
                               _composite_allreduce_w1(m._C, x),
                               rtol=0, atol=0, equal_nan=True)
    # backward: the gradient goes through the same compressed pipeline
    torch.testing.assert_close(x.grad.cpu(),
                               _composite_allreduce_w1(m._C, w),
                               rtol=0, atol=0, equal_nan=True)


def test_world1_default_is_exact_clone(world1):
    m = world1
    comm = m.COMM_WORLD
    x = _inputs(4099, torch.bfloat16, seed=2).cuda()
    y = comm.AllreduceCompressed(x, m.MPI_SUM)
    assert y.data_ptr() != x.data_ptr()
    _bytes_equal(y.cpu(), x.cpu())
