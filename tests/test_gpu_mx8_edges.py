"""GPU (MI355X) tests that pin the mxfp8 codec kernels (csrc/mx8_kernels.hip)
on their value domain and past one grid.

Value domain: every 16-bit input under anchors that put it in the e4m3
subnormal and underflow range, the amax rule at every fp32 exponent, exact
round-to-nearest-even ties, all 256 x 256 wire bytes through dequantize, all
byte pairs through reduce / reduce_to under eight scale pairs, a rank-order
probe and a finite sum that overflows. The reference is the numpy float64
oracle of mx8_oracles.py, which test_mx8_oracles.py pins to the torch oracle
and the C++ composite on the CPU. Each case runs through the vector kernel
and through its twin (base off by one element or byte, or an odd row), and
through the separate copies of the codec in the _blocks and _segments
kernels. Every comparison is exact; NaN compares by position.

Grid wrap: grid_for caps a launch at 4096 workgroups of 256 lanes, the
_blocks kernels cap grid.x at 4096 / nblocks and the segments kernels at
4096 / nsegs (at least 1). Each kernel body runs once at the smallest size
whose lane slots exceed the capped grid, so the grid-stride loop takes a
second trip that ends in a partial wave, against the CPU composite.
"""

import functools
import os

import numpy as np
import pytest
import torch

import mx8_oracles as mo
from test_mx8_oracles import (check_anchored_coverage, check_boundary_coverage,
                              check_dequant_all_coverage, check_ties_coverage)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALVES = [torch.float16, torch.bfloat16]

# launch geometry of csrc/mx8_kernels.hip
GRID_CAP = 4096      # grid_for / xcap / seg_grid: workgroups per launch
WG = 256             # lanes per workgroup
LPG = {torch.float32: 8, torch.bfloat16: 4, torch.float16: 4}  # lanes/group
EPL = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}  # elems/chunk


@pytest.fixture(scope="module")
def world1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29561")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    import torch.distributed as dist

    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    import mpi4torch_amd as m

    m.init()
    return m


def _off_by_one(t):
    """A contiguous GPU copy of the flat CPU tensor t whose base is one
    element (one byte for uint8) past a 16-byte boundary: the twins' path."""
    v = torch.cat([t[:1], t]).cuda()[1:]
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _both_bases(t):
    g = t.cuda()
    assert g.data_ptr() % 16 == 0
    return [("vector", g), ("twin", _off_by_one(t))]


# =============================== value domain ==============================

# ---- 1. quantize ----------------------------------------------------------

def _quantize_case(name):
    if name == "boundary":
        check_boundary_coverage()
        return mo.fp32_amax_boundary()[0]
    if name == "ties":
        check_ties_coverage()
        return mo.fp32_ties()[0]
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[name]
    check_anchored_coverage(dtype)
    return mo.anchored_sweep(dtype)


@pytest.mark.parametrize("case", ["fp16", "bf16", "boundary", "ties"])
def test_quantize_values(world1, case):
    C = world1._C
    x = _quantize_case(case)
    p_ref, s_ref = mo.quantize(mo.groups(x))
    for path, xg in _both_bases(x):
        p, s = C._mx8_quantize(xg)
        mo.bytes_equal(s.cpu(), s_ref, f"{case} {path} scales")
        mo.bytes_equal(p.cpu(), p_ref, f"{case} {path} payload")


# ---- 2. dequantize --------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_all_wire_bytes(world1, dtype):
    C = world1._C
    pay, sc = mo.dequant_all()
    want, _, _ = check_dequant_all_coverage(dtype)
    for path, pg in _both_bases(pay):
        out = C._mx8_dequantize(pg, sc.cuda(), 65536, dtype)
        mo.nan_aware_equal(out.cpu(), want, f"{dtype} {path}")


# ---- 3 / 4. reduce and reduce_to on every byte pair -----------------------

def _pair_views(pay):
    """[P, n] CPU payload -> [(path, GPU [P, n])], aligned and off by one
    byte"""
    P, n = pay.shape
    flat = pay.reshape(-1)
    return [(path, g.view(P, n)) for path, g in _both_bases(flat)]


@pytest.mark.parametrize("pair", mo.SCALE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_reduce_all_byte_pairs(world1, pair):
    C = world1._C
    pay, sc = mo.reduce_pairs(*pair)
    p_ref, s_ref = mo.reduce(pay.numpy(), sc.numpy())
    for path, pg in _pair_views(pay):
        p, s = C._mx8_reduce(pg, sc.cuda())
        mo.bytes_equal(s.cpu(), s_ref, f"{pair} {path} scales")
        mo.bytes_equal(p.cpu(), p_ref, f"{pair} {path} payload")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair", mo.SCALE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_reduce_to_all_byte_pairs(world1, pair, dtype):
    C = world1._C
    pay, sc = mo.reduce_pairs(*pair)
    want = mo.reduce_to(pay.numpy(), sc.numpy(), 65536, dtype)
    for path, pg in _pair_views(pay):
        out = C._mx8_reduce_to(pg, sc.cuda(), 65536, dtype)
        mo.nan_aware_equal(out.cpu(), want, f"{pair} {dtype} {path}")


# ---- 5. rank order --------------------------------------------------------

@pytest.mark.parametrize("P", [3, 5])
def test_reduce_sums_in_rank_order(world1, P):
    C = world1._C
    pay, sc = mo.rank_order_probe(P)
    # the probe discriminates: the oracle gives 0 in rank order and 1.0
    # with the last two live copies exchanged (2^25, -2^25, 1); the CPU
    # suite checks every permutation
    outcomes = mo.rank_order_outcomes(P)
    assert outcomes[tuple(range(P))] == (0.0, 0.0)
    live = (0, 1, 2) if P == 3 else (0, 2, 4)
    swapped = list(range(P))
    swapped[live[1]], swapped[live[2]] = live[2], live[1]
    assert outcomes[tuple(swapped)][0] == 1.0
    assert all(1.0 in v for k, v in outcomes.items()
               if sorted([c for c in k if c in live][:2]) != list(live[:2]))
    zero = torch.zeros(64, dtype=torch.float32)
    for path, pg in _pair_views(pay):
        y = C._mx8_reduce_to(pg, sc.cuda(), 64, torch.float32)
        mo.nan_aware_equal(y.cpu(), zero, f"reduce_to {path}")
        p, s = C._mx8_reduce(pg, sc.cuda())
        mo.bytes_equal(p.cpu(), np.zeros(64, dtype=np.uint8), path)
        mo.bytes_equal(s.cpu(), np.full(2, 127, dtype=np.uint8), path)
        d = C._mx8_dequantize(p, s, 64, torch.float32)
        mo.nan_aware_equal(d.cpu(), zero, f"reduce + dequantize {path}")


# ---- 6. a finite sum that overflows ---------------------------------------

def test_reduce_finite_sum_overflows(world1):
    C = world1._C
    pay, sc = mo.overflow_probe()
    p_ref, s_ref = mo.reduce(pay.numpy(), sc.numpy())
    assert s_ref.tolist() == [255] and not p_ref.any()
    for path, pg in _pair_views(pay):
        p, s = C._mx8_reduce(pg, sc.cuda())
        mo.bytes_equal(s.cpu(), s_ref, path)
        mo.bytes_equal(p.cpu(), p_ref, path)
        for dtype in (torch.float32, torch.bfloat16):
            want = mo.reduce_to(pay.numpy(), sc.numpy(), 32, dtype)
            assert float(want[0]) == float("inf")
            assert float(want[1]) == mo.OVERFLOW_FINITE
            y = C._mx8_reduce_to(pg, sc.cuda(), 32, dtype).cpu()
            assert not bool(torch.isnan(y).any())
            mo.nan_aware_equal(y, want, f"{dtype} {path}")


# ---- 7. the relatives of quantize -----------------------------------------

def _relative_input(name):
    if name == "ties":
        return mo.fp32_ties()[0]
    return mo.anchored_sweep({"fp16": torch.float16,
                              "bf16": torch.bfloat16}[name])


@pytest.mark.parametrize("odd", [False, True], ids=["vector", "odd-row"])
@pytest.mark.parametrize("case", ["fp16", "bf16", "ties"])
def test_quantize_blocks_values(world1, case, odd):
    """nblocks = 2, rows = 3; a row length that is 8 modulo 32 (the vector
    body, groups straddle rows) or odd (the one-thread-per-group twin)."""
    C = world1._C
    x = _relative_input(case)
    t, row_elems, streams = mo.as_blocks(
        x, 2, 3, 1 if odd else 8, 2 if odd else 32)
    p_ref, s_ref = mo.quantize_streams(list(streams))
    tg = t.cuda()
    assert tg.data_ptr() % 16 == 0
    p, s = C._mx8_quantize_blocks(tg, 2, 3, row_elems)
    mo.bytes_equal(s.cpu(), s_ref, f"{case} scales")
    mo.bytes_equal(p.cpu(), p_ref, f"{case} payload")


@pytest.mark.parametrize("case", ["fp16", "bf16", "ties"])
def test_quantize_segments_values(world1, case):
    """rows = 1, after = 8, counts [5, 0, rest], slices gathered through an
    order: MODE 1 of the vector body, then the twin (base off by one)."""
    C = world1._C
    x = _relative_input(case)
    t, counts, order, segs = mo.as_segments(x, 8, 5, seed=3)
    p_ref, s_ref = mo.quantize_streams(segs)
    for path, tg in _both_bases(t):
        p, s = C._mx8_quantize_segments(tg, 1, 8, counts, order=order.cuda())
        mo.bytes_equal(s.cpu(), s_ref, f"{case} {path} scales")
        mo.bytes_equal(p.cpu(), p_ref, f"{case} {path} payload")


# ---- 8. the relatives of dequantize ---------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_elems", [16384, 16383])
def test_dequantize_blocks_all_wire_bytes(world1, row_elems, dtype):
    """nblocks = 2, rows = 2 over the 2 x 1024 groups of dequant_all. Rows
    of 16384 take the vector body; rows of 16383 leave the last group of a
    block padded (30 elements) and take the shifted twin."""
    C = world1._C
    pay, sc = mo.dequant_all()
    full, _, _ = check_dequant_all_coverage(dtype)
    L = 2 * row_elems
    assert (L + 31) // 32 == 1024
    want = (full.view(2, 32768)[:, :L].reshape(2, 2, row_elems)
            .transpose(0, 1).contiguous())
    out = C._mx8_dequantize_blocks(pay.view(2, 32768).cuda(),
                                   sc.view(2, 1024).cuda(), 2, row_elems,
                                   dtype)
    assert out.shape == (2, 2, row_elems)
    mo.nan_aware_equal(out.cpu(), want, f"{dtype} {row_elems}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_segments_all_wire_bytes(world1, dtype):
    """rows = 1, after = 8, counts [5, 0, 8184] over the 2048 groups of
    dequant_all (segment 0: two groups, the second partial), slices
    scattered through an order; then the twin (payload off by one byte)."""
    C = world1._C
    pay, sc = mo.dequant_all()
    full, _, _ = check_dequant_all_coverage(dtype)
    counts = [5, 0, 8184]
    S = sum(counts)
    assert 2 + (8184 * 8) // 32 == 2048
    stream = torch.cat([full[:40], full[64:]]).view(S, 8)
    order = torch.randperm(S, generator=torch.Generator().manual_seed(8))
    want = torch.empty(1, S, 8, dtype=dtype)
    want[0, order] = stream
    for path, pg in _both_bases(pay):
        out = C._mx8_dequantize_segments(pg, sc.cuda(), 1, 8, counts, dtype,
                                         order=order.cuda())
        assert out.shape == (1, S, 8)
        mo.nan_aware_equal(out.cpu(), want, f"{dtype} {path}")


# ================================= grid wrap ===============================
#
# The launch grid cannot be observed from Python; each threshold below is
# derived from the launch code:
#   grid_for(work)   = min(ceil(work / 256), 4096) workgroups, so a flat
#                      kernel loops twice when work > 4096 * 256 lane slots;
#   xcap             = max(4096 / nblocks, 1) workgroups in grid.x of a
#                      _blocks launch (grid.y = block), so a block loops twice
#                      when its lane slots exceed 256 * xcap;
#   seg_grid(work,n) = the same with the number of segments of the launch.
# Inputs are the sibling _inputs helper's: randn * scale * rand(G, 1) with
# the special groups (zero, amax 448 * 2^-3, inf, NaN).

SLOTS = GRID_CAP * WG


def _inputs(n, dtype, seed, scale=1.0):
    from test_gpu_compressed import _inputs as sibling

    return sibling(n, dtype, seed, scale)


def _C_cpu():
    import mpi4torch_amd as m

    return m._C


@functools.lru_cache(maxsize=None)
def _flat_case(dtype, groups_over):
    """(x, payload, scales, dequantized) on the CPU for N = 32 * groups + 7
    elements, groups = groups_over: the composite's results."""
    C = _C_cpu()
    N = 32 * groups_over + 7
    x = _inputs(N, dtype, seed=groups_over % 1000, scale=3.0)
    p, s = C._mx8_quantize(x)
    d = C._mx8_dequantize(p, s, N, dtype)
    assert bool(torch.isnan(d).any()) and int(s.max()) == 255
    return x, p, s, d


# lane slots of the vector body: nfull * LPG (quantize and dequantize)
FLAT_GROUPS = {torch.float32: 131072 + 5, torch.bfloat16: 262144 + 5}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_grid_wraps(world1, dtype):
    C = world1._C
    nfull = FLAT_GROUPS[dtype]
    assert nfull * LPG[dtype] > SLOTS                 # a second trip
    assert (nfull * LPG[dtype] - SLOTS) % 64 != 0     # ends in a partial wave
    x, p_ref, s_ref, _ = _flat_case(dtype, nfull)
    assert x.numel() % 32 == 7                        # and a scalar tail
    p, s = C._mx8_quantize(x.cuda())
    mo.bytes_equal(s.cpu(), s_ref, "scales")
    mo.bytes_equal(p.cpu(), p_ref, "payload")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dequantize_grid_wraps(world1, dtype):
    C = world1._C
    nfull = FLAT_GROUPS[dtype]
    assert nfull * LPG[dtype] > SLOTS
    assert (nfull * LPG[dtype] - SLOTS) % 64 != 0
    x, p_ref, s_ref, d_ref = _flat_case(dtype, nfull)
    N = x.numel()
    buf = torch.full((N + 64,), 7.0, dtype=dtype, device="cuda")
    C._mx8_dequantize(p_ref.cuda(), s_ref.cuda(), N, dtype, out=buf)
    mo.nan_aware_equal(buf[:N].cpu(), d_ref)
    assert bool((buf[N:] == 7.0).all()), "wrote past N"


@functools.lru_cache(maxsize=None)
def _copies_case(G):
    """Two quantized copies of G groups (the last one partial, 7 elements):
    copy 0 from _inputs, copy 1 the same stream rotated by 1031 groups, so
    groups of different magnitude and the special groups meet."""
    C = _C_cpu()
    N = 32 * (G - 1) + 7
    p, s = C._mx8_quantize(_inputs(N, torch.float32, seed=G % 1000, scale=3.0))
    pay = torch.stack([p, p.view(G, 32).roll(1031, 0).reshape(-1)])
    sc = torch.stack([s, s.roll(1031, 0)])
    return pay.contiguous(), sc.contiguous(), N


def test_reduce_grid_wraps(world1):
    C = world1._C
    n = 524288 + 5
    assert n * 2 > SLOTS and (n * 2 - SLOTS) % 64 != 0   # 2 lanes per group
    pay, sc, _ = _copies_case(n + 1)
    pay = pay[:, :n * 32].contiguous()
    sc = sc[:, :n].contiguous()
    p_ref, s_ref = _C_cpu()._mx8_reduce(pay, sc)
    assert int(s_ref.max()) == 255 and int(s_ref.min()) < 255
    p, s = C._mx8_reduce(pay.cuda(), sc.cuda())
    mo.bytes_equal(s.cpu(), s_ref, "scales")
    mo.bytes_equal(p.cpu(), p_ref, "payload")


# lanes per group of the reduce_to body: 4 for fp32, 2 for the 16-bit dtypes
REDUCE_TO_LPG = {torch.float32: 4, torch.bfloat16: 2}
REDUCE_TO_GROUPS = {torch.float32: 262144 + 5, torch.bfloat16: 524288 + 5}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reduce_to_grid_wraps(world1, dtype):
    C = world1._C
    nfull = REDUCE_TO_GROUPS[dtype]
    assert nfull * REDUCE_TO_LPG[dtype] > SLOTS
    assert (nfull * REDUCE_TO_LPG[dtype] - SLOTS) % 64 != 0
    pay, sc, _ = _copies_case(524288 + 5 + 1)
    G = nfull + 1
    N = 32 * nfull + 7
    pay = pay[:, :G * 32].contiguous()
    sc = sc[:, :G].contiguous()
    want = _C_cpu()._mx8_reduce_to(pay, sc, N, dtype)
    assert bool(torch.isnan(want).any())
    buf = torch.full((N + 64,), 7.0, dtype=dtype, device="cuda")
    C._mx8_reduce_to(pay.cuda(), sc.cuda(), N, dtype, out=buf)
    mo.nan_aware_equal(buf[:N].cpu(), want)
    assert bool((buf[N:] == 7.0).all()), "wrote past N"


# The one-thread-per-group twins: G groups > 4096 * 256 lanes, bf16 (67 MB),
# every base off by one element or byte.
TWIN_GROUPS = (1 << 20) + 5 + 1     # the last group holds 7 elements


@functools.lru_cache(maxsize=None)
def _twin_case():
    C = _C_cpu()
    N = 32 * (TWIN_GROUPS - 1) + 7
    x = _inputs(N, torch.bfloat16, seed=77, scale=3.0)
    p, s = C._mx8_quantize(x)
    return x, p, s


def test_scalar_twins_quantize_dequantize_grid_wrap(world1):
    C = world1._C
    assert TWIN_GROUPS > SLOTS and (TWIN_GROUPS - SLOTS) % 64 != 0
    x, p_ref, s_ref = _twin_case()
    N = x.numel()
    p, s = C._mx8_quantize(_off_by_one(x))
    mo.bytes_equal(s.cpu(), s_ref, "scales")
    mo.bytes_equal(p.cpu(), p_ref, "payload")
    del p, s
    want = _C_cpu()._mx8_dequantize(p_ref, s_ref, N, torch.bfloat16)
    out = C._mx8_dequantize(_off_by_one(p_ref), s_ref.cuda(), N,
                            torch.bfloat16)
    mo.nan_aware_equal(out.cpu(), want)


def test_scalar_twins_reduce_reduce_to_grid_wrap(world1):
    C = world1._C
    G = TWIN_GROUPS
    assert G > SLOTS and (G - SLOTS) % 64 != 0
    x, p0, s0 = _twin_case()
    N = x.numel()
    pay = torch.stack([p0, p0.view(G, 32).roll(1031, 0).reshape(-1)])
    sc = torch.stack([s0, s0.roll(1031, 0)]).contiguous()
    pg = _off_by_one(pay.reshape(-1)).view(2, G * 32)
    p_ref, s_ref = _C_cpu()._mx8_reduce(pay, sc)
    p, s = C._mx8_reduce(pg, sc.cuda())
    mo.bytes_equal(s.cpu(), s_ref, "scales")
    mo.bytes_equal(p.cpu(), p_ref, "payload")
    del p, s
    want = _C_cpu()._mx8_reduce_to(pay, sc, N, torch.bfloat16)
    out = C._mx8_reduce_to(pg, sc.cuda(), N, torch.bfloat16)
    mo.nan_aware_equal(out.cpu(), want)


# ---- _blocks --------------------------------------------------------------

def _blocks_wrap(C, dtype, nblocks, rows, row_elems, seed):
    n = rows * nblocks * row_elems
    x = _inputs(n, dtype, seed=seed, scale=3.0)
    p_ref, s_ref = _C_cpu()._mx8_quantize_blocks(x, nblocks, rows, row_elems)
    assert int(s_ref.max()) == 255
    xg = x.cuda()
    assert xg.data_ptr() % 16 == 0
    p, s = C._mx8_quantize_blocks(xg, nblocks, rows, row_elems)
    mo.bytes_equal(s.cpu(), s_ref, "scales")
    mo.bytes_equal(p.cpu(), p_ref, "payload")
    del p, s, xg
    want = _C_cpu()._mx8_dequantize_blocks(p_ref, s_ref, rows, row_elems,
                                           dtype)
    buf = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")
    C._mx8_dequantize_blocks(p_ref.cuda(), s_ref.cuda(), rows, row_elems,
                             dtype, out=buf)
    mo.nan_aware_equal(buf[:n].cpu().view(rows, nblocks, row_elems), want)
    assert bool((buf[n:] == 7.0).all()), "wrote past the output"


@pytest.mark.parametrize("nblocks,row_elems",
                         [(64, 21860), (4096, 344), (5000, 344)])
def test_blocks_vector_grid_wraps(world1, nblocks, row_elems):
    """fp32, rows = 3: the lane slots of one block (Gb * 8 on the quantize
    side, L / 4 chunks on the dequantize side) exceed 256 * xcap. 4096
    blocks leave grid.x = 1; 5000 blocks take the 4096 / nblocks == 0
    branch of xcap."""
    rows, dtype = 3, torch.float32
    xcap = max(GRID_CAP // nblocks, 1)
    L = rows * row_elems
    assert row_elems % EPL[dtype] == 0
    chunks = L // EPL[dtype]
    assert chunks > WG * xcap and (chunks - WG * xcap) % 64 != 0
    assert (L + 31) // 32 * LPG[dtype] > WG * xcap
    assert L % 32 != 0                      # a partial last group per block
    _blocks_wrap(world1._C, dtype, nblocks, rows, row_elems, seed=nblocks)


def test_blocks_twins_grid_wrap(world1):
    """bf16, 4096 blocks, rows = 3, an odd row of 2733: the quantize twin
    has one lane per group, Gb = 257 > 256 * 1; the shifted dequantize twin
    has rows * (row_elems / 8 + 2) = 1029 lane slots."""
    nblocks, rows, row_elems, dtype = 4096, 3, 2733, torch.bfloat16
    xcap = max(GRID_CAP // nblocks, 1)
    assert row_elems % EPL[dtype] != 0
    assert (rows * row_elems + 31) // 32 > WG * xcap
    assert rows * (row_elems // EPL[dtype] + 2) > WG * xcap
    _blocks_wrap(world1._C, dtype, nblocks, rows, row_elems, seed=5)


# ---- _segments ------------------------------------------------------------

def _segments_wrap(C, dtype, rows, after, counts, permute):
    S = sum(counts)
    n = rows * S * after
    x = _inputs(n, dtype, seed=S % 1000, scale=3.0)
    gen = torch.Generator().manual_seed(S)
    so = torch.randperm(S, generator=gen) if permute else None
    ro = torch.randperm(S, generator=gen) if permute else None
    Cc = _C_cpu()
    p_ref, s_ref = Cc._mx8_quantize_segments(x, rows, after, counts, order=so)
    assert int(s_ref.max()) == 255
    p, s = C._mx8_quantize_segments(x.cuda(), rows, after, counts,
                                    order=so.cuda() if permute else None)
    mo.bytes_equal(s.cpu(), s_ref, "scales")
    mo.bytes_equal(p.cpu(), p_ref, "payload")
    want = Cc._mx8_dequantize_segments(p_ref, s_ref, rows, after, counts,
                                       dtype, order=ro)
    buf = torch.full((n + 64,), 7.0, dtype=dtype, device="cuda")
    C._mx8_dequantize_segments(p_ref.cuda(), s_ref.cuda(), rows, after, counts,
                               dtype, order=ro.cuda() if permute else None,
                               out=buf)
    mo.nan_aware_equal(buf[:n].cpu().view(rows, S, after), want)
    assert bool((buf[n:] == 7.0).all()), "wrote past the output"


@pytest.mark.parametrize("rows,big,permute",
                         [(1, 16400, False), (1, 16400, True),
                          (3, 5500, True)],
                         ids=["mode0", "mode1", "mode2"])
def test_segments_vector_grid_wraps(world1, rows, big, permute):
    """fp32, after = 8 (two chunks per slice), 32 segments: grid.x is capped
    at 4096 / 32 = 128 workgroups and sized for the largest segment, whose
    chunks exceed 256 * 128. No order is MODE 0 (the 31 one-slice segments
    keep the launch off the flat-stream shortcut), an order with rows = 1 is
    MODE 1, with rows = 3 MODE 2."""
    dtype, after = torch.float32, 8
    counts = [big] + [1] * 31
    assert len(counts) == int(world1._C._MX8_MAX_SEGS_PER_LAUNCH)
    xcap = GRID_CAP // len(counts)
    chunks = rows * big * (after // EPL[dtype])
    assert chunks > WG * xcap and (chunks - WG * xcap) % 64 != 0
    assert (1 * after) % 32 != 0            # not one flat stream
    _segments_wrap(world1._C, dtype, rows, after, counts, permute)


@pytest.mark.parametrize("permute", [False, True])
def test_segments_twins_grid_wrap(world1, permute):
    """bf16, after = 41 (no multiple of 8: the one-thread-per-group twins),
    rows = 1: the largest segment has 32800 groups > 256 * 128."""
    dtype, after, rows = torch.bfloat16, 41, 1
    counts = [25600] + [1] * 31
    xcap = GRID_CAP // len(counts)
    assert after % EPL[dtype] != 0
    G = (rows * counts[0] * after + 31) // 32
    assert G > WG * xcap and (G - WG * xcap) % 64 != 0
    _segments_wrap(world1._C, dtype, rows, after, counts, permute)
