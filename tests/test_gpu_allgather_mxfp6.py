"""GPU (MI355X) tests for the mxfp6 wire of AllgatherCompressed: the gfx950
mx6_quantize and mx6_dequantize_blocks kernels and their twins against the
CPU torch composite, byte for byte, and the full pipeline at world size 1
under force_full_path.

The composite (csrc/ops.cpp) is the semantic definition; tests/
test_allgather_mxfp6.py pins it to an independent float64 oracle on the CPU.
"""

import pytest
import torch

from test_allgather_mxfp6 import VALUE_SETS, WIRE, all_wire_codes
from test_gpu_allgather_compressed import world1, _match  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CANARY = 0xA5
WRAP = 4096 * 256          # lane slots of one full grid


def _quantize_with_canaries(C, x, in_off=0, pay_off=0):
    """Kernel quantize of x placed in_off elements into its buffer, payload
    written pay_off bytes into a canary-filled buffer; returns the bytes
    after checking that nothing else was written."""
    G = (x.numel() + 31) // 32
    xb = torch.zeros(x.numel() + in_off, dtype=x.dtype, device="cuda")
    xb[in_off:] = x
    pb = torch.full((pay_off + G * 24 + 64,), CANARY, dtype=torch.uint8,
                    device="cuda")
    sb = torch.full((G + 64,), CANARY, dtype=torch.uint8, device="cuda")
    pay, sc = C._mx6_quantize(xb[in_off:], payload_out=pb[pay_off:],
                              scales_out=sb)
    assert pay.data_ptr() == pb.data_ptr() + pay_off
    assert bool((pb[:pay_off] == CANARY).all())
    assert bool((pb[pay_off + G * 24:] == CANARY).all())
    assert bool((sb[G:] == CANARY).all())
    return pay.cpu(), sc.cpu()


@pytest.fixture(scope="module")
def value_refs(world1):
    """name -> (values, composite payload, composite scales), computed once."""
    C = world1._C
    return {k: (x, *C._mx6_quantize(x))
            for k, x in ((k, f()) for k, f in VALUE_SETS.items())}


@pytest.mark.parametrize("offs", [(0, 0), (1, 0), (0, 1)],
                         ids=["vector", "in_off", "pay_off"])
@pytest.mark.parametrize("name", sorted(VALUE_SETS))
def test_quantize_values(world1, value_refs, name, offs):
    x, rpay, rsc = value_refs[name]
    pay, sc = _quantize_with_canaries(world1._C, x, *offs)
    assert torch.equal(sc, rsc)
    assert torch.equal(pay, rpay)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 16, 31, 32, 33, 32 * 32 + 16,
                               16 * (WRAP + 70) + 3])
def test_quantize_geometry(world1, n, dtype):
    C = world1._C
    g = torch.Generator().manual_seed(n)
    G = (n + 31) // 32
    x = (torch.randn(G, 32, generator=g) *
         torch.rand(G, 1, generator=g)).reshape(-1)[:n].to(dtype)
    rpay, rsc = C._mx6_quantize(x)
    pay, sc = _quantize_with_canaries(C, x)
    assert torch.equal(sc, rsc) and torch.equal(pay, rpay)
    if n < WRAP:
        pay, sc = _quantize_with_canaries(C, x, in_off=1, pay_off=1)
        assert torch.equal(sc, rsc) and torch.equal(pay, rpay)


def _dequantize_with_canaries(C, pay, sc, P, rows, row_elems, dtype,
                              out_off=0, pay_off=0):
    total = rows * P * row_elems
    pb = torch.zeros(pay.numel() + pay_off, dtype=torch.uint8, device="cuda")
    pb[pay_off:] = pay.reshape(-1)
    ob = torch.full((out_off + total + 32,), 7.0, dtype=dtype, device="cuda")
    out = C._mx6_dequantize_blocks(pb[pay_off:], sc.cuda(), P, rows,
                                   row_elems, dtype, out=ob[out_off:])
    assert out.shape == (rows, P, row_elems)
    assert out.data_ptr() == ob.data_ptr() + out_off * ob.element_size()
    assert bool((ob[:out_off] == 7.0).all())
    assert bool((ob[out_off + total:] == 7.0).all())
    return out.cpu()


@pytest.mark.parametrize("out_off", [0, 1], ids=["vector", "twin"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_all_codes(world1, dtype, out_off):
    C = world1._C
    pay, sc = all_wire_codes()
    n = 32 * sc.numel()
    ref = C._mx6_dequantize_blocks(pay, sc, 1, 1, n, dtype)
    out = _dequantize_with_canaries(C, pay, sc, 1, 1, n, dtype,
                                    out_off=out_off)
    _match(out, ref)


def _wire(P, L, seed):
    """Random payload bytes under scales around 127, with a 255, a 0 and a
    254 scale where there is room."""
    g = torch.Generator().manual_seed(seed)
    Gb = (L + 31) // 32
    pay = torch.randint(0, 256, (P, Gb * 24), dtype=torch.uint8, generator=g)
    sc = torch.randint(100, 150, (P, Gb), dtype=torch.uint8, generator=g)
    if Gb >= 3:
        sc[0, 1], sc[-1, 0], sc[-1, 2] = 255, 0, 254
    return pay, sc


# (1,48) a partial group of whole chunks; (3,48) a group straddling rows;
# (7,16) (7,8) (7,4) rows of two chunks, one chunk and, for the 16-bit
# dtypes, less than one, which takes the twin; (1,33) (4,43) rows that start
# at elements 0, 43, 86, 129 and so at all four bit phases; (2,7) head- and
# tail-only rows; (3,24) an odd Gb, so the blocks' scale bases are misaligned
@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("geom", [(1, 32), (1, 48), (3, 48), (7, 16), (7, 8),
                                  (7, 4), (1, 33), (4, 43), (2, 7), (3, 24)])
def test_dequantize_blocks_geometry(world1, geom, P):
    C = world1._C
    rows, row_elems = geom
    pay, sc = _wire(P, rows * row_elems, seed=rows * row_elems + P)
    for dtype in DTYPES:
        ref = C._mx6_dequantize_blocks(pay, sc, P, rows, row_elems, dtype)
        for out_off, pay_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
            out = _dequantize_with_canaries(C, pay, sc, P, rows, row_elems,
                                            dtype, out_off, pay_off)
            _match(out, ref)


@pytest.mark.parametrize("row_elems", [16 * (WRAP // 2 + 37),
                                       8 * (WRAP // 2 + 37) + 3],
                         ids=["vector", "twin"])
def test_dequantize_blocks_grid_wrap(world1, row_elems):
    C = world1._C
    pay, sc = _wire(2, row_elems, seed=5)
    ref = C._mx6_dequantize_blocks(pay, sc, 2, 1, row_elems, torch.bfloat16)
    out = _dequantize_with_canaries(C, pay, sc, 2, 1, row_elems,
                                    torch.bfloat16)
    _match(out, ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,axis", [((33,), 0), ((1 << 16,), 0),
                                        (((1 << 16) + 3,), 0), ((3, 40), 1)])
def test_full_path_world1(world1, shape, axis, dtype):
    m = world1
    C = m._C
    g = torch.Generator().manual_seed(shape[0])
    x = torch.randn(shape, generator=g).to(dtype)
    rows = 1 if axis == 0 else shape[0]
    ref = C._mx6_dequantize_blocks(*C._mx6_quantize(x), 1, rows,
                                   x.numel() // rows, dtype).view(shape)
    xd = x.cuda()
    clone = m.COMM_WORLD.AllgatherCompressed(xd, axis, wire=WIRE)
    assert clone.data_ptr() != xd.data_ptr() and torch.equal(clone, xd)
    C.force_full_path(True)
    try:
        out = m.COMM_WORLD.AllgatherCompressed(xd, axis, wire=WIRE)
    finally:
        C.force_full_path(False)
    _match(out.cpu(), ref)
    assert not torch.equal(out.cpu(), x)
