"""GPU (MI355X) tests for AlltoallPairwiseCompressedWeighted: its three gfx950
kernels, fed bytes directly, on the case lists and references of
test_alltoall_pairwise_weighted.py; then the op and the gate_at="combine" MoE
layer at world size 1 under force_full_path."""

import pytest
import torch

import mx8_oracles as mo
from test_alltoall_pairwise_indexed import wire
from test_alltoall_pairwise_weighted import (COMBINE, QUANT, QUANT_IDS, gen,
                                             reference, combine_case,
                                             quant_case, rowdot_case,
                                             check_rowdot, op_case, moe_layer,
                                             full_path)
from test_gpu_alltoall_pairwise_compressed import world1  # noqa: F401
from test_gpu_mx8_edges import _off_by_one

pytestmark = pytest.mark.gpu
OFFSETS = ((0, 0), (1, 0), (0, 1))               # vector body, then the twin


def shifted(t, off):
    return _off_by_one(t) if off else t.cuda()


def canaried(n, dtype, off, fill=float("nan")):
    """(buffer, check): n elements at offset `off` between canaries."""
    buf = torch.full((off + n + 16,), fill, dtype=dtype, device="cuda")
    same = torch.isnan if fill != fill else (lambda t: t == fill)

    def check(what=""):
        assert bool(same(buf[:off]).all()), ("underrun", what)
        assert bool(same(buf[off + n:]).all()), ("overrun", what)
        return buf[off:off + n].cpu()
    return buf, check


def combine(C, pay, sc, after, counts, index, w, out_size, fan, dtype, poff=0,
            ooff=0):
    buf, check = canaried(out_size * after, dtype, ooff)
    C._mx8_dequantize_combine_weighted(
        shifted(pay, poff), sc.cuda(), after, counts, index.cuda(), w.cuda(),
        out_size, fan, dtype, out=buf[ooff:])
    return check((poff, ooff)).view(out_size, after)


@pytest.mark.parametrize("name", COMBINE)
def test_combine_kernel(world1, name):  # noqa: F811
    *a, dtype = combine_case(name)
    want = reference(*a, dtype)
    for poff, ooff in OFFSETS:
        mo.nan_aware_equal(combine(world1._C, *a, dtype, poff, ooff), want,
                           (poff, ooff))


def test_combine_grid_wrap(world1):  # noqa: F811
    """More chunks than the capped grid has threads, ending in a partial
    wave: fp32 slices of one chunk, two sources each but for the last."""
    out_size = 4096 * 256 + 37
    R = 2 * out_size - 1
    pay, sc = wire(4, [R], 9)
    w = torch.randn(R, generator=gen(3))
    d = torch.from_numpy(mo._f32(mo.dequantize(pay.numpy(), sc.numpy())))
    d = w.view(R, 1) * d.view(-1)[:R * 4].view(R, 4)
    d = torch.cat([d, torch.zeros(1, 4)]).view(out_size, 2, 4)
    want = d[:, 0] + d[:, 1]
    want[-1] = d[-1, 0]                          # one source: assigned
    got = combine(world1._C, pay, sc, 4, [R], torch.arange(R) // 2, w,
                  out_size, 2, torch.float32)
    mo.nan_aware_equal(got, want)


@pytest.mark.parametrize("after,counts,dtype", QUANT, ids=QUANT_IDS)
def test_quantize_kernel(world1, after, counts, dtype):  # noqa: F811
    x, index, w, pay, sc = quant_case(after, counts, dtype)
    for xoff, poff in OFFSETS:
        pbuf, pcheck = canaried(pay.size, torch.uint8, poff, 0xAB)
        sbuf, scheck = canaried(sc.size, torch.uint8, 0, 0xAB)
        world1._C._mx8_quantize_segments_weighted(
            shifted(x.view(-1), xoff), after, counts, w.cuda(),
            order=index.cuda(), payload_out=pbuf[poff:], scales_out=sbuf)
        mo.bytes_equal(pcheck((xoff, poff)), pay, (xoff, poff))
        mo.bytes_equal(scheck((xoff, poff)), sc, (xoff, poff))


def rowdot(C, pay, sc, after, counts, index, g, poff=0):
    buf, check = canaried(sum(counts), torch.float32, 8)
    C._mx8_dequantize_rowdot(shifted(pay, poff), sc.cuda(), after, counts,
                             index.cuda(), g.cuda(), out=buf[8:])
    return check(poff)


# bf16 chunks per slice 1, 5, 8 (LPS 8), 9 (16), 20 (32), 64, 65 (64), 129 and
# 512 (more than one trip, the first with a ragged last); 41 takes the twin
@pytest.mark.parametrize("after,dtype", [
    (8, torch.bfloat16), (40, torch.bfloat16), (64, torch.bfloat16),
    (72, torch.float16), (160, torch.bfloat16), (512, torch.bfloat16),
    (520, torch.bfloat16), (1032, torch.bfloat16), (4096, torch.bfloat16),
    (4096, torch.float32), (20, torch.float32), (41, torch.bfloat16)])
def test_rowdot_kernel(world1, after, dtype):  # noqa: F811
    pay, sc, counts, index, g, ref, bound = rowdot_case(after, 37, dtype)
    got = rowdot(world1._C, pay, sc, after, counts, index, g)
    check_rowdot(got, ref, bound)
    assert torch.equal(got.view(torch.int32), rowdot(
        world1._C, pay, sc, after, counts, index, g).view(torch.int32))
    check_rowdot(rowdot(world1._C, pay, sc, after, counts, index, g, 1), ref,
                 bound)                          # the twin


def test_rowdot_grid_wrap(world1):  # noqa: F811
    """More slices than the capped grid sweeps at once, a partial last wave."""
    *a, ref, bound = rowdot_case(8, 4096 * 32 + 37, torch.bfloat16)
    pay, sc, counts, index, g = a
    check_rowdot(rowdot(world1._C, pay, sc, 8, counts, index, g), ref, bound)


def test_op_full_path_world1(world1):  # noqa: F811
    gw, ref, bound = full_path(
        world1, lambda: op_case(world1.COMM_WORLD, 0, 1, "cuda"))
    assert bool(((gw.double() - ref.double()).abs() <= bound).all())


def test_moe_gate_at_combine_gpu(world1):  # noqa: F811
    layer = moe_layer("cuda")
    x = torch.randn(24, 32, device="cuda", requires_grad=True)
    y = full_path(world1, lambda: layer(x))
    full_path(world1, (y ** 2).sum().backward)
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    for p in [x] + list(layer.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert float(layer.router.weight.grad.abs().max()) > 0
