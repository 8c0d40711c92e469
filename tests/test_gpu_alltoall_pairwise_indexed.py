"""GPU (MI355X) tests for AlltoallPairwiseCompressedIndexed: the gfx950
mx8_dequantize_combine kernels, fed payload and scale bytes directly, against
the plain reference of test_alltoall_pairwise_indexed.py (numpy float64
dequantize, Python loop of ordered fp32 adds, one cast), exactly and with NaN
by position; then the op and the top-2 MoE layer at world size 1 under
force_full_path.
"""

import pytest
import torch

import mx8_oracles as mo
from test_alltoall_pairwise_indexed import (DTYPES, GEOMS, GEOM_IDS, wire,
                                            fan_index, reference, nan_case,
                                            order_probe, dropped_case)
from test_gpu_alltoall_pairwise_compressed import world1  # noqa: F401

pytestmark = pytest.mark.gpu


def run(C, pay, sc, after, counts, index, out_size, fan, dtype, poff=0,
        ooff=0):
    """The kernel between canaries: payload base off by poff bytes, out base
    off by ooff elements. Returns the result on the CPU."""
    n = out_size * after
    pg = torch.cat([torch.zeros(poff, dtype=torch.uint8), pay]).cuda()[poff:]
    obuf = torch.full((ooff + n + 16,), float("nan"), dtype=dtype,
                      device="cuda")
    got = C._mx8_dequantize_combine(pg, sc.cuda(), after, counts, index.cuda(),
                                    out_size, fan, dtype, out=obuf[ooff:])
    assert got.data_ptr() == obuf.data_ptr() + ooff * obuf.element_size()
    assert bool(torch.isnan(obuf[:ooff]).all()), "output underrun"
    assert bool(torch.isnan(obuf[ooff + n:]).all()), "output overrun"
    return obuf[ooff:ooff + n].cpu().view(out_size, after)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_kernel_matches_reference(world1, geom, dtype):  # noqa: F811
    after, counts, fan = geom
    pay, sc = wire(after, counts, after)
    index, out_size = fan_index(sum(counts), fan, after + 1)
    want = reference(pay, sc, after, counts, index, out_size, fan, dtype)
    assert not bool(torch.isnan(want).any())     # so NaN canaries can tell
    for poff, ooff in ((0, 0), (1, 0), (0, 1)):  # vector body, then the twin
        got = run(world1._C, pay, sc, after, counts, index, out_size, fan,
                  dtype, poff, ooff)
        mo.nan_aware_equal(got, want, (poff, ooff))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [nan_case, order_probe, dropped_case])
def test_kernel_special_cases(world1, case, dtype):  # noqa: F811
    pay, sc, after, counts, index, out_size, fan = case()
    want = reference(pay, sc, after, counts, index, out_size, fan, dtype)
    got = world1._C._mx8_dequantize_combine(
        pay.cuda(), sc.cuda(), after, counts, index.cuda(), out_size, fan,
        dtype).cpu()
    mo.nan_aware_equal(got, want)
    if case is dropped_case:                     # canaries, both kernels
        for poff, ooff in ((0, 0), (1, 1)):
            mo.nan_aware_equal(run(world1._C, pay, sc, after, counts, index,
                                   out_size, fan, dtype, poff, ooff), want)


def test_grid_wrap(world1):  # noqa: F811
    """More chunks than the capped grid has threads, ending in a partial
    wave: fp32 slices of one chunk, two sources each but for the last."""
    out_size = 4096 * 256 + 37
    R = 2 * out_size - 1
    pay, sc = wire(4, [R], 9)
    d = torch.from_numpy(mo._f32(mo.dequantize(pay.numpy(), sc.numpy())))
    d = torch.cat([d.view(-1)[:R * 4], torch.zeros(4)]).view(out_size, 2, 4)
    want = d[:, 0] + d[:, 1]
    want[-1] = d[-1, 0]                          # one source: assigned
    got = run(world1._C, pay, sc, 4, [R], torch.arange(R) // 2, out_size, 2,
              torch.float32)
    mo.nan_aware_equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_path_world1(world1, dtype):  # noqa: F811
    """Dispatch then combine through the op on the GPU is the composition of
    the CPU debug bindings, forward and backward."""
    m, C = world1, world1._C
    N, D, k = 37, 40, 2
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, D, generator=g).to(dtype)
    w = torch.randn(N, D, generator=g).to(dtype)
    tok = torch.argsort(torch.randint(0, 4, (N * k,), generator=g),
                        stable=True) // k

    def composite(t):
        p, s = C._mx8_quantize_segments(t.view(-1), 1, D, [N * k], order=tok)
        y = C._mx8_dequantize_segments(p, s, 1, D, [N * k], dtype)
        p, s = C._mx8_quantize_segments(y.view(-1), 1, D, [N * k])
        return C._mx8_dequantize_combine(p, s, D, [N * k], tok, N, k, dtype)

    xg, tg = x.cuda().requires_grad_(), tok.cuda()
    f = m.COMM_WORLD.AlltoallPairwiseCompressedIndexed
    C.force_full_path(True)
    try:
        y = f(xg, 0, [N * k], [N * k], send_index=tg, max_repeat=k)
        z = f(y, 0, [N * k], [N * k], recv_index=tg, out_size=N, max_repeat=k)
        z.backward(w.cuda())
        torch.cuda.synchronize()
    finally:
        C.force_full_path(False)
    assert z.is_cuda and z.dtype == dtype and z.shape == (N, D)
    mo.nan_aware_equal(z.detach().cpu(), composite(x))
    mo.nan_aware_equal(xg.grad.cpu(), composite(w))


def test_moe_top2_gpu(world1):  # noqa: F811
    from mpi4torch_amd.models.moe import ExpertParallelMoE

    torch.manual_seed(5)
    layer = ExpertParallelMoE(64, 4, compression="mxfp8", top_k=2).cuda()
    x = torch.randn(50, 64, device="cuda", requires_grad=True)
    world1._C.force_full_path(True)
    try:
        y = layer(x)
        (y ** 2).sum().backward()
        torch.cuda.synchronize()
    finally:
        world1._C.force_full_path(False)
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    assert bool(torch.isfinite(x.grad).all())
    for p in layer.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
