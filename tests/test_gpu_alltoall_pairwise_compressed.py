"""GPU (MI355X) tests for AlltoallPairwiseCompressed: the gfx950
mx8_quantize_segments / mx8_dequantize_segments kernels against the CPU torch
composite, byte for byte; canaries around every buffer; out-of-range index
entries; a one-GPU emulation of a 5-rank pairwise exchange; the full pipeline
and the MoE layer at world size 1 under force_full_path.

The composite (csrc/ops.cpp) is the semantic definition; tests/
test_alltoall_pairwise_compressed.py pins it to an independent pure-torch
oracle on the CPU.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MAX_SEGS = 32
# (rows, after, counts): see the CPU file. (1,4,..) is the smallest vector
# slice for fp32 and takes the twin for the 16-bit dtypes; (2,41,..) and
# (1,1,..) take the twins for every dtype; (1,32,..) without an index is one
# flat stream.
GEOMS = [
    (1, 32, [3, 0, 2, 1, 4]),
    (1, 4, [1, 9, 0, 7]),
    (1, 8, [1, 9, 0, 7]),
    (1, 40, [2, 3, 1]),
    (3, 8, [5, 0, 2, 6]),
    (2, 41, [1, 3, 2]),
    (1, 1, [31, 33, 1]),
    (1, 4096, [1, 2]),
    (1, 8, [i % 4 for i in range(MAX_SEGS + 1)]),
]


@pytest.fixture(scope="module")
def world1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29559")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    import torch.distributed as dist

    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    import mpi4torch_amd as m

    m.init()
    assert int(m._C._MX8_MAX_SEGS_PER_LAUNCH) == MAX_SEGS
    return m


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _eq(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.shape, b.shape)
    assert torch.equal(a.contiguous().view(torch.uint8),
                       b.contiguous().view(torch.uint8))


def _match(a, b):
    """NaNs at the same positions, everything else byte for byte."""
    from test_reducescatter_compressed import _nan_aware_bytes_equal

    _nan_aware_bytes_equal(a, b)


def _flat(rows, after, counts, dtype, seed):
    from test_allgather_compressed import _inputs

    n = rows * sum(counts) * after
    scale = (1.0, 1e-6, 30.0)[seed % 3]
    return _inputs(n, dtype, seed=seed, scale=scale)


# --------------------- kernels vs composite, byte for byte ----------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("geom", GEOMS,
                         ids=lambda g: f"{g[0]}x{g[1]}x{len(g[2])}")
def test_segments_kernels_match_composite(world1, geom, permute, dtype):
    C = world1._C
    rows, after, counts = geom
    S = sum(counts)
    x = _flat(rows, after, counts, dtype, seed=S + after)
    so = _perm(S, S) if permute else None
    ro = _perm(S, S + 1) if permute else None
    p_ref, s_ref = C._mx8_quantize_segments(x, rows, after, counts, order=so)
    p, s = C._mx8_quantize_segments(
        x.cuda(), rows, after, counts,
        order=so.cuda() if permute else None)
    assert p.is_cuda and s.is_cuda
    _eq(s.cpu(), s_ref)
    _eq(p.cpu(), p_ref)
    want = C._mx8_dequantize_segments(p_ref, s_ref, rows, after, counts,
                                      dtype, order=ro)
    got = C._mx8_dequantize_segments(
        p_ref.cuda(), s_ref.cuda(), rows, after, counts, dtype,
        order=ro.cuda() if permute else None)
    assert got.is_cuda and got.shape == (rows, S, after)
    _match(got.cpu(), want)


# --------------------------------- canaries -------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("geom", [(3, 8, [5, 0, 2, 6]), (1, 40, [2, 3, 1]),
                                  (2, 41, [1, 3, 2])])
def test_segments_canaries(world1, geom, permute, dtype):
    """Guard bytes around payload, scales and output stay as they were, with
    aligned bases (the vector kernels) and with the payload base off by one
    byte / the input and output base off by one element (the twins)."""
    from test_compressed import _rand_input

    C = world1._C
    rows, after, counts = geom
    S = sum(counts)
    n = rows * S * after
    x = _rand_input(n, dtype, seed=11 + S).contiguous()
    so = _perm(S, 5) if permute else None
    ro = _perm(S, 6) if permute else None
    sog = so.cuda() if permute else None
    rog = ro.cuda() if permute else None
    p_ref, s_ref = C._mx8_quantize_segments(x, rows, after, counts, order=so)
    NP, NS = p_ref.numel(), s_ref.numel()
    o_ref = C._mx8_dequantize_segments(p_ref, s_ref, rows, after, counts,
                                       dtype, order=ro)

    def run_q(xg, poff):
        pbuf = torch.full((poff + NP + 64,), 0xAB, dtype=torch.uint8,
                          device="cuda")
        sbuf = torch.full((NS + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        pay, sc = C._mx8_quantize_segments(xg, rows, after, counts, order=sog,
                                           payload_out=pbuf[poff:],
                                           scales_out=sbuf)
        assert pay.data_ptr() == pbuf.data_ptr() + poff
        assert sc.data_ptr() == sbuf.data_ptr()
        _eq(pbuf[poff:poff + NP].cpu(), p_ref)
        _eq(sbuf[:NS].cpu(), s_ref)
        assert bool((pbuf[poff + NP:] == 0xAB).all()), "payload overrun"
        assert bool((pbuf[:poff] == 0xAB).all()), "payload underrun"
        assert bool((sbuf[NS:] == 0xAB).all()), "scales overrun"

    def run_d(poff, ooff):
        pg = torch.cat([torch.zeros(poff, dtype=torch.uint8),
                        p_ref]).cuda()[poff:]
        # NaN is the sentinel: the inputs have none, so with a permutation
        # (or no order) every output slice is written and none is left
        obuf = torch.full((ooff + n + 16,), float("nan"), dtype=dtype,
                          device="cuda")
        got = C._mx8_dequantize_segments(pg, s_ref.cuda(), rows, after, counts,
                                         dtype, order=rog, out=obuf[ooff:])
        assert got.data_ptr() == obuf.data_ptr() + ooff * obuf.element_size()
        head = obuf[ooff:ooff + n].cpu()
        assert not bool(torch.isnan(head).any()), "a slice was not written"
        _eq(head.view(rows, S, after), o_ref)
        assert bool(torch.isnan(obuf[ooff + n:]).all()), "output overrun"
        assert bool(torch.isnan(obuf[:ooff]).all()), "output underrun"

    xg = x.cuda()
    assert xg.data_ptr() % 16 == 0
    run_q(xg, 0)
    shifted = torch.cat([x[:1], x]).cuda()[1:]
    assert shifted.data_ptr() % 16 != 0
    run_q(shifted, 0)
    run_q(xg, 1)
    run_d(0, 0)
    run_d(1, 0)
    run_d(0, 1)


# ---------------------------- out-of-range index --------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geom", [(1, 8, [1, 9, 0, 7]), (3, 8, [5, 0, 2, 6]),
                                  (2, 5, [1, 3, 2])])
def test_out_of_range_index_is_zeros_and_dropped(world1, geom, dtype):
    """One entry equal to S and one negative. The launch is valid: the
    kernels compare every entry with S before they form an address. The send
    side reads such a slice as zeros, the receive side drops it."""
    from test_compressed import _rand_input

    C = world1._C
    rows, after, counts = geom
    S = sum(counts)
    n = rows * S * after
    x = _rand_input(n, dtype, seed=21 + S).contiguous()
    order = _perm(S, 9)
    bad = order.clone()
    bad[1] = S
    bad[S - 2] = -1
    ok = (bad >= 0) & (bad < S)
    # send side: the composite on the gathered tensor with those slices zero
    xs = x.view(rows, S, after).index_select(1, order).clone()
    xs[:, ~ok] = 0
    p_ref, s_ref = C._mx8_quantize_segments(xs.view(-1), rows, after, counts)
    NP, NS = p_ref.numel(), s_ref.numel()
    pbuf = torch.full((NP + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((NS + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    C._mx8_quantize_segments(x.cuda(), rows, after, counts, order=bad.cuda(),
                             payload_out=pbuf, scales_out=sbuf)
    _eq(pbuf[:NP].cpu(), p_ref)
    _eq(sbuf[:NS].cpu(), s_ref)
    assert bool((pbuf[NP:] == 0xAB).all()) and bool((sbuf[NS:] == 0xAB).all())
    # receive side: valid slices land, the two others are dropped
    y = C._mx8_dequantize_segments(p_ref, s_ref, rows, after, counts, dtype)
    want = torch.full((rows, S, after), float("nan"), dtype=dtype)
    want[:, bad[ok]] = y[:, ok]
    obuf = torch.full((16 + n + 16,), float("nan"), dtype=dtype,
                      device="cuda")
    C._mx8_dequantize_segments(p_ref.cuda(), s_ref.cuda(), rows, after,
                               counts, dtype, order=bad.cuda(), out=obuf[16:])
    _match(obuf[16:16 + n].cpu().view(rows, S, after), want)
    assert int(torch.isnan(want[0, :, 0]).sum()) == 2
    assert bool(torch.isnan(obuf[:16]).all())
    assert bool(torch.isnan(obuf[16 + n:]).all())


# ------------- one-GPU emulation of a 5-rank pairwise exchange ------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("orders", [False, True])
@pytest.mark.parametrize("case", [(1, 40), (3, 8)])
def test_emulated_pairwise_matches_oracle(world1, case, orders, dtype):
    """Quantize every emulated rank's segments on the GPU, route payload and
    scale slices to receiver `me` by hand, dequantize there on the GPU: the
    result is the CPU oracle's for that rank."""
    from test_alltoall_pairwise_compressed import (_count_matrix, _column,
                                                   oracle_pairwise)
    from test_allgather_compressed import _inputs

    C = world1._C
    P = 5
    rows, after = case
    M = _count_matrix(P, 31)
    S = [sum(M[r]) for r in range(P)]
    R = [sum(_column(M, r)) for r in range(P)]
    xs = [_inputs(rows * S[r] * after, dtype, seed=30 + r,
                  scale=(1.0, 1e-6, 30.0)[r % 3]).view(rows, S[r], after)
          for r in range(P)]
    so = [_perm(S[r], 40 + r) if orders else None for r in range(P)]
    ro = [_perm(R[r], 50 + r) if orders else None for r in range(P)]
    want = oracle_pairwise(xs, 1, M, so, ro)
    qs, goffs = [], []
    for r in range(P):
        qs.append(C._mx8_quantize_segments(
            xs[r].cuda().view(-1), rows, after, M[r],
            order=so[r].cuda() if orders else None))
        G = [(rows * c * after + 31) // 32 for c in M[r]]
        goffs.append([sum(G[:j]) for j in range(P + 1)])
    for me in (1, 4):
        stg_pay = torch.cat([qs[r][0][32 * goffs[r][me]:32 * goffs[r][me + 1]]
                             for r in range(P)])
        stg_sc = torch.cat([qs[r][1][goffs[r][me]:goffs[r][me + 1]]
                            for r in range(P)])
        out = C._mx8_dequantize_segments(
            stg_pay, stg_sc, rows, after, _column(M, me), dtype,
            order=ro[me].cuda() if orders else None)
        assert out.is_cuda
        _match(out.cpu(), want[me])


# ------------------- the full pipeline at world size 1 --------------------

def _composite(C, x, axis, so, ro):
    """What the full path computes at world size 1, with the CPU composite."""
    xc = x.detach().cpu().contiguous()
    rows = 1
    for d in xc.shape[:axis]:
        rows *= d
    S = xc.shape[axis]
    after = xc.numel() // (rows * S)
    p, s = C._mx8_quantize_segments(xc.view(-1), rows, after, [S], order=so)
    return C._mx8_dequantize_segments(p, s, rows, after, [S], xc.dtype,
                                      order=ro).view(xc.shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [((37, 40), 0), ((3, 10, 8), 1)])
def test_full_path_world1(world1, case, dtype):
    from test_allgather_compressed import _inputs

    m = world1
    shape, axis = case
    numel = 1
    for d in shape:
        numel *= d
    S = shape[axis]
    x = _inputs(numel, dtype, seed=numel).view(shape).cuda().requires_grad_()
    w = _inputs(numel, dtype, seed=numel + 9).view(shape).cuda()
    so, ro = _perm(S, 1), _perm(S, 2)
    m._C.force_full_path(True)
    try:
        y = m.COMM_WORLD.AlltoallPairwiseCompressed(
            x, axis, [S], [S], send_order=so.cuda(), recv_order=ro.cuda())
        y.backward(w)
        torch.cuda.synchronize()
    finally:
        m._C.force_full_path(False)
    assert y.is_cuda and y.dtype == dtype and y.shape == x.shape
    _match(y.detach().cpu(), _composite(m._C, x, axis, so, ro))
    _match(x.grad.cpu(), _composite(m._C, w, axis, ro, so))


def test_world1_default_is_the_exact_permutation(world1):
    from test_allgather_compressed import _inputs

    m = world1
    x = _inputs(50 * 64, torch.bfloat16, seed=2).view(50, 64).cuda()
    so, ro = _perm(50, 3).cuda(), _perm(50, 4).cuda()
    y = m.COMM_WORLD.AlltoallPairwiseCompressed(x, 0, [50], [50], so, ro)
    want = torch.empty_like(x)
    want.index_copy_(0, ro, x.index_select(0, so))
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


# ------------------------------- MoE on the GPU ---------------------------

def test_moe_gpu_matches_cpu_composite(world1):
    """ExpertParallelMoE(compression="mxfp8") on the GPU against the same
    layer on the CPU, both under force_full_path so both run the codec.

    The two runs share every byte of the input and the weights, and the
    dispatch is bit-identical (the codec sees the same x). The router, the
    experts and the gate run on different GEMM / erf / exp implementations,
    so the expert output differs by rounding: two fp32 GEMMs of K <= 256
    (256 * 2^-24 = 1.5e-5 each, relative to the operand magnitudes) plus
    GELU and softmax, bounded here by TIGHT = 1e-4 * (|want| + max|want|).
    That rounding can move an expert output across an e4m3 rounding point of
    the combine codec; the element then differs by one step of its group's
    grid, at most amax/7 (the top binade of e4m3 has spacing 32 and the
    scaled amax is above 224). A flip needs the value within ~1e-5 of a
    midpoint of a grid whose relative spacing is at least 2^-4, so about
    3e-4 of the elements at worst: one percent is allowed."""
    from mpi4torch_amd.models.moe import ExpertParallelMoE

    m = world1
    d_model, N = 64, 50
    torch.manual_seed(5)
    cpu_layer = ExpertParallelMoE(d_model, 4, compression="mxfp8")
    gpu_layer = ExpertParallelMoE(d_model, 4, compression="mxfp8")
    gpu_layer.load_state_dict(cpu_layer.state_dict())
    gpu_layer.cuda()
    x = torch.randn(N, d_model)
    xg = x.cuda().requires_grad_()
    m._C.force_full_path(True)
    try:
        with torch.no_grad():
            want = cpu_layer(x)
        got = gpu_layer(xg)
        (got ** 2).sum().backward()
        torch.cuda.synchronize()
    finally:
        m._C.force_full_path(False)
    with torch.no_grad():
        plain = ExpertParallelMoE(d_model, 4)
        plain.load_state_dict(cpu_layer.state_dict())
        assert not torch.equal(plain(x), want)       # the codec really ran
    got = got.detach().cpu()
    valid = ~torch.isnan(want)
    assert bool(valid.any())
    assert not bool(torch.isnan(got[valid]).any())
    diff = (got - want).abs()[valid]
    top = want[valid].abs().max()
    tight = 1e-4 * (want[valid].abs() + top)
    loose = top / 7 + tight
    print("moe gpu-vs-cpu: max diff", float(diff.max()), "over tight",
          int((diff > tight).sum()), "of", diff.numel())
    assert bool((diff <= loose).all())
    assert int((diff > tight).sum()) <= diff.numel() // 100
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    for p in gpu_layer.router.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert any(p.grad is not None and bool(p.grad.abs().sum() > 0)
               for p in gpu_layer.experts.parameters())
