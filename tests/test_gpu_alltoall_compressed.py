"""GPU (MI355X) tests for AlltoallCompressed: the gfx950 mx8_quantize_blocks
kernel against the CPU torch composite, byte for byte, a one-GPU emulation
of a P-rank all-to-all, and the full pipeline at world size 1 under
force_full_path.

The composite (csrc/ops.cpp) is the semantic definition; tests/
test_alltoall_compressed.py pins it to an independent pure-torch oracle on
the CPU.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (rows, row_elems): the flat path (1,32); a partial last group per block on
# the general twin (1,1) (1,31) (1,33) (1,4099) (1,32*257+5); groups
# straddling rows on the vector path, with a partial last group (3,40),
# (5,36) (fp32 only; 16-bit takes the twin) and without (4,1000) (2,4096);
# the smallest vector row, (7,4) for fp32 and (7,8) for 16-bit ((7,4) takes
# the general twin for 16-bit, with rows shorter than a chunk); the odd-row
# general twin (3,41)
GEOMS = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 4099), (1, 32 * 257 + 5),
         (3, 40), (3, 41), (5, 36), (7, 4), (7, 8), (2, 4096), (4, 1000)]


@pytest.fixture(scope="module")
def world1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29558")
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


def _blocks_input(L, P, rows, row_elems, dtype, seed0):
    """(flat [rows][P][row_elems] input, its P contiguous blocks) with mixed
    per-block scales; the special groups sit in every block but block 1."""
    blocks = []
    for r in range(P):
        scale = (1.0, 1e-6, 3e4)[r % 3] if L > 33 else 1.0
        if dtype == torch.float16 and scale > 1.0:
            scale = 30.0                   # 3e4 * randn leaves the fp16 range
        x = _inputs(L, torch.float32, seed=seed0 + 100 * r, scale=scale)
        if r == 1:
            x = torch.nan_to_num(x, nan=0.5, posinf=1.0)
        blocks.append(x.to(dtype).contiguous())
    x = torch.stack([b.view(rows, row_elems) for b in blocks], dim=1)
    return x.contiguous().view(-1), blocks


def _eq(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a, b)


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
def test_quantize_blocks_kernel_matches_composite(world1, geom, P, dtype):
    C = world1._C
    rows, row_elems = geom
    L = rows * row_elems
    Gb = (L + 31) // 32
    x, blocks = _blocks_input(L, P, rows, row_elems, dtype, seed0=L)
    p_ref, s_ref = C._mx8_quantize_blocks(x, P, rows, row_elems)
    pay, sc = C._mx8_quantize_blocks(x.cuda(), P, rows, row_elems)
    assert pay.is_cuda and pay.dtype == torch.uint8 and sc.dtype == torch.uint8
    assert pay.shape == (P, Gb * 32) and sc.shape == (P, Gb)
    _eq(sc.cpu(), s_ref)
    _eq(pay.cpu(), p_ref)
    if L >= 256:
        assert int(s_ref[0, 4]) == 255 and int(s_ref[0, 5]) == 255
        assert not bool(p_ref[0, 4 * 32:6 * 32].any())
    # every block is the quantize kernel's on its contiguous copy
    for r in range(P):
        q = C._mx8_quantize(blocks[r].cuda())
        _eq(pay[r].cpu(), q[0].cpu())
        _eq(sc[r].cpu(), q[1].cpu())


@pytest.mark.parametrize("P", [1, 5])
def test_quantize_blocks_clamped_exponent_region(world1, P):
    """Groups of magnitude ~1e-38 (amax tiny or an fp32 subnormal): E clamps
    at -127 and the scaled values are exact (ldexpf)."""
    C = world1._C
    L = 3 * 429                            # 32*40 + 7
    g = torch.Generator().manual_seed(17)
    blocks = [(torch.randn(41, 32, generator=g) * 4e-38 *
               torch.rand(41, 1, generator=g)).reshape(-1)[:L].contiguous()
              for _ in range(P)]
    assert bool((blocks[0].abs() < 2.0 ** -126).any())
    # the general twin (3x429, 9x143) and the vector path (4x320)
    for rows, row_elems in ((3, 429), (9, 143), (4, 320)):
        n = rows * row_elems
        x = torch.stack([b[:n].view(rows, row_elems) for b in blocks],
                        dim=1).contiguous().view(-1)
        p_ref, s_ref = C._mx8_quantize_blocks(x, P, rows, row_elems)
        assert int(s_ref[0].min()) == 0    # E = -127 reached
        assert bool(p_ref.any())
        pay, sc = C._mx8_quantize_blocks(x.cuda(), P, rows, row_elems)
        _eq(sc.cpu(), s_ref)
        _eq(pay.cpu(), p_ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", [(1, 33), (3, 40), (3, 41),
                                  (1, 32 * 257 + 5)])
def test_quantize_blocks_writes_exactly_what_it_owns(world1, geom, dtype):
    """Quantize into buffers with a 64-byte canary tail: nothing may be
    written past P*Gb*32 payload bytes and P*Gb scale bytes."""
    C = world1._C
    P = 5
    rows, row_elems = geom
    L = rows * row_elems
    Gb = (L + 31) // 32
    NP, NS = P * Gb * 32, P * Gb
    x, _ = _blocks_input(L, P, rows, row_elems, dtype, seed0=11)
    p_ref, s_ref = C._mx8_quantize_blocks(x, P, rows, row_elems)

    def run(xg, poff=0):
        pbuf = torch.full((poff + NP + 64,), 0xAB, dtype=torch.uint8,
                          device="cuda")
        sbuf = torch.full((NS + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        pay, sc = C._mx8_quantize_blocks(xg, P, rows, row_elems,
                                         payload_out=pbuf[poff:],
                                         scales_out=sbuf)
        assert pay.data_ptr() == pbuf.data_ptr() + poff
        assert sc.data_ptr() == sbuf.data_ptr()
        assert pay.shape == (P, Gb * 32) and sc.shape == (P, Gb)
        _eq(pbuf[poff:poff + NP].cpu().view(P, Gb * 32), p_ref)
        _eq(sbuf[:NS].cpu().view(P, Gb), s_ref)
        assert bool((pbuf[poff + NP:] == 0xAB).all()), "payload overrun"
        assert bool((pbuf[:poff] == 0xAB).all()), "payload underrun"
        assert bool((sbuf[NS:] == 0xAB).all()), "scales overrun"

    xg = x.cuda()
    assert xg.data_ptr() % 16 == 0
    run(xg)
    # through the general twin: the input an x[1:] view (base off 16 bytes)
    shifted = torch.cat([x[:1], x]).cuda()[1:]
    assert shifted.data_ptr() % 16 != 0
    run(shifted)
    # and with the payload base off by one byte
    run(xg, poff=1)


# --------------- one-GPU emulation of a P-rank all-to-all -----------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [((3, 5 * 8), 0, 1), ((2, 3, 5 * 2, 8), 1, 2)])
def test_emulated_alltoall_matches_oracle(world1, case, dtype):
    """Quantize every rank's input on the GPU, hand receiver `me` block `me`
    of each as its staging, dequantize on the GPU: the result is the CPU
    oracle's for that rank."""
    from test_alltoall_compressed import oracle_alltoall

    C = world1._C
    P = 5
    shape, gaxis, saxis = case
    numel = 1
    for d in shape:
        numel *= d
    xs = [_inputs(numel, dtype, seed=30 + r,
                  scale=(1.0, 1e-6, 3e4)[r % 3]).view(shape) for r in range(P)]
    want = oracle_alltoall(xs, gaxis, saxis)
    n = shape[saxis] // P
    before_s = 1
    for d in shape[:saxis]:
        before_s *= d
    row_s = numel // before_s // P
    bshape = list(shape)
    bshape[saxis] = n
    before_g = 1
    for d in bshape[:gaxis]:
        before_g *= d
    row_g = numel // P // before_g
    qs = [C._mx8_quantize_blocks(x.cuda().view(-1), P, before_s, row_s)
          for x in xs]
    for me in (0, 3):
        stg_pay = torch.stack([q[0][me] for q in qs])
        stg_sc = torch.stack([q[1][me] for q in qs])
        out = C._mx8_dequantize_blocks(stg_pay, stg_sc, before_g, row_g,
                                       dtype)
        assert out.is_cuda
        _match(out.cpu().view(want[me].shape), want[me])


# ------------------- the full pipeline at world size 1 --------------------

def _composite_codec(C, x):
    """dq(q(x)) with the CPU composite: what the full path computes at world
    size 1, where the one block is the whole tensor."""
    xc = x.detach().cpu().contiguous()
    p, s = C._mx8_quantize(xc)
    return C._mx8_dequantize(p, s, xc.numel(), xc.dtype).view(xc.shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [((3, 40), 0, 1), ((3, 40), 1, 0),
                                  ((2, 3, 4, 8), 1, 2), ((256, 257), 0, 1)])
def test_full_path_world1(world1, case, dtype):
    m = world1
    shape, gaxis, saxis = case
    numel = 1
    for d in shape:
        numel *= d
    x = _inputs(numel, dtype, seed=numel).view(shape).cuda().requires_grad_()
    w = _inputs(numel, dtype, seed=numel + 9).view(shape).cuda()
    m._C.force_full_path(True)
    try:
        y = m.COMM_WORLD.AlltoallCompressed(x, gaxis, saxis)
        y.backward(w)
        torch.cuda.synchronize()
    finally:
        m._C.force_full_path(False)
    assert y.is_cuda and y.dtype == dtype and y.shape == x.shape
    _match(y.detach().cpu(), _composite_codec(m._C, x))
    _match(x.grad.cpu(), _composite_codec(m._C, w))


def test_world1_default_is_exact_clone(world1):
    m = world1
    comm = m.COMM_WORLD
    x = _inputs(4099 * 2, torch.bfloat16, seed=2).view(2, 4099).cuda()
    y = comm.AlltoallCompressed(x, 0, 1)
    assert y.data_ptr() != x.data_ptr()
    assert torch.equal(y.cpu().view(torch.uint8), x.cpu().view(torch.uint8))
