"""GPU (MI355X) tests for stochastic rounding on the mxfp8 wire: the two _sr
kernels (vector and any-alignment twin) against the CPU composite, byte for
byte, and the full pipelines at world size 1 under force_full_path.

The composite (csrc/ops.cpp) is the semantic definition; tests/
test_compressed_sr.py pins it to an independent oracle on the CPU.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
N0S = [0, 2 ** 33 - 64]   # the second makes the pair index cross 2^32
SEED = 2 ** 40 + 3


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
        x[1, 8] = -0.0
        x[2] = 0.0                         # an all-zero group
        x[3] = x[3].clamp(-1, 1)
        x[3, 5] = 448.0 * 2.0 ** -3        # amax exactly 448 * 2^j
        x[4, 9] = float("inf")             # one inf -> scale 255 group
        x[5, 0] = float("nan")
        x[6] *= 1e-38                      # the clamped E = -127 region
    return x.reshape(-1)[:n].to(dtype).contiguous()


def _bytes_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _both_equal(got, want):
    for g, w in zip(got, want):
        assert g.is_cuda
        _bytes_equal(g.cpu(), w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n0", N0S)
@pytest.mark.parametrize("n", [1, 31, 33, 4099, 32 * 257 + 5])
def test_quantize_sr_kernel_matches_composite(world1, n, n0, dtype):
    C = world1._C
    for scale in (1.0, 3e4):
        x = _inputs(n, dtype, seed=n, scale=scale)
        _both_equal(C._mx8_quantize_sr(x.cuda(), SEED, 2, 1, n0),
                    C._mx8_quantize_sr(x, SEED, 2, 1, n0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_sr_kernel_misaligned_base(world1, dtype):
    C = world1._C
    x = _inputs(4099 + 1, dtype, seed=3).cuda()[1:]
    assert x.data_ptr() % 16 != 0          # takes the twin
    _both_equal(C._mx8_quantize_sr(x, SEED, 0, 0, N0S[1]),
                C._mx8_quantize_sr(x.cpu(), SEED, 0, 0, N0S[1]))


def _reduce_case(C, P, n, n0, misaligned):
    qs = [C._mx8_quantize(_inputs(n, torch.float32, seed=n + r,
                                  scale=(1.0, 3e4, 1e-6)[r % 3]))
          for r in range(P)]
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    want = C._mx8_reduce_sr(pay, sc, SEED, 1, 0, n0)
    dpay = pay.cuda()
    if misaligned:
        dpay = torch.cat([dpay.new_zeros(1), dpay.reshape(-1)])[1:].view_as(pay)
        assert dpay.data_ptr() % 16 != 0   # takes the twin
    _both_equal(C._mx8_reduce_sr(dpay, sc.cuda(), SEED, 1, 0, n0), want)


@pytest.mark.parametrize("n0", N0S)
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("P", [1, 5])
def test_reduce_sr_kernel_matches_composite(world1, P, n, n0):
    _reduce_case(world1._C, P, n, n0, misaligned=False)


def test_reduce_sr_kernel_misaligned_base(world1):
    _reduce_case(world1._C, 5, 4099, N0S[1], misaligned=True)


def _chain_w1(C, x, stream0):
    p, s = C._mx8_quantize_sr(x.detach().cpu(), SEED, stream0, 0, 0)
    p, s = C._mx8_reduce_sr(p[None], s[None], SEED, stream0 + 1, 0, 0)
    return C._mx8_dequantize(p, s, x.numel(), x.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [33, 4096, 2 ** 16 + 3])   # 4096: one launch
def test_full_path_world1(world1, n, dtype):
    m = world1
    C, comm = m._C, m.COMM_WORLD
    x = _inputs(n, dtype, seed=n).cuda().requires_grad_()
    w = _inputs(n, dtype, seed=n + 9).cuda()
    C.force_full_path(True)
    try:
        y = comm.AllreduceCompressed(x, seed=SEED)
        y.backward(w)
        rs = comm.ReducescatterCompressed(x.detach(), 0, seed=SEED)
        rne = comm.AllreduceCompressed(x.detach())
        torch.cuda.synchronize()
    finally:
        C.force_full_path(False)
    same = dict(rtol=0, atol=0, equal_nan=True)
    torch.testing.assert_close(y.detach().cpu(), _chain_w1(C, x, 0), **same)
    torch.testing.assert_close(x.grad.cpu(), _chain_w1(C, w, 2), **same)
    p, s = C._mx8_quantize_sr(x.detach().cpu(), SEED, 0, 0, 0)
    torch.testing.assert_close(
        rs.cpu(), C._mx8_reduce_to(p[None], s[None], n, dtype), **same)
    # seed=None is still round to nearest
    xc = x.detach().cpu()
    p, s = C._mx8_reduce(*(t[None] for t in C._mx8_quantize(xc)))
    torch.testing.assert_close(rne.cpu(), C._mx8_dequantize(p, s, n, dtype),
                               **same)
