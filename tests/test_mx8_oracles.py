"""The mxfp8 value-domain sweeps on the CPU: the numpy float64 oracle of
mx8_oracles.py, the torch oracle of test_compressed.py and the C++ composite
(csrc/ops.cpp) agree on every input builder, byte for byte (outputs: NaN at
the same positions, every other element byte for byte), and each builder
still covers the edge it was built for. The GPU kernel tests
(test_gpu_mx8_edges.py) run the same builders through the gfx950 kernels
against the numpy oracle, so they inherit a checked reference.
"""

import functools

import numpy as np
import pytest
import torch

import mx8_oracles as mo
from test_compressed import (oracle_dequantize_groups, oracle_quantize,
                             oracle_reduce)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALVES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def C():
    import mpi4torch_amd as m

    return m._C


def _quantize_three_way(C, x):
    pn, sn = mo.quantize(mo.groups(x))
    pt, st = oracle_quantize(x)
    pc, sc = C._mx8_quantize(x)
    mo.bytes_equal(st, sn, "torch oracle scales")
    mo.bytes_equal(pt, pn, "torch oracle payload")
    mo.bytes_equal(sc, sn, "composite scales")
    mo.bytes_equal(pc, pn, "composite payload")
    return pn, sn


# ----------------------------- coverage facts ------------------------------
#
# Shared with the GPU file: each asserts, on the oracle's output, that the
# builder still reaches the edge it exists for.

@functools.lru_cache(maxsize=None)
def check_anchored_coverage(dtype):
    x = mo.anchored_sweep(dtype)
    e = mo.encode(mo.groups(x))
    code = e["payload"] & 0x7f
    sub = int(((code > 0) & (code < 8)).sum())
    nz = x.float().numpy() != 0
    zeros = int(((code == 0) & nz & np.isfinite(x.float().numpy())
                 & (np.repeat(e["scales"], 32) != 255)).sum())
    assert sub > 1000, sub
    assert zeros > 1000, zeros
    assert (e["payload"] == 0x00).any() and (e["payload"] == 0x80).any()
    # a nonzero input encoded as -0
    assert ((e["payload"] == 0x80) & nz).any()
    sub_tie = int((e["tie"] & (e["y"] < 2.0 ** -6)).sum())
    assert sub_tie >= 1, sub_tie
    # the underflow edge: y == 2^-10, the midpoint between 0 and the
    # smallest subnormal
    assert (e["tie"] & (e["y"] == 2.0 ** -10)).any()
    assert int((e["scales"] == 255).sum()) == 4
    return sub, zeros, sub_tie


def check_boundary_coverage():
    x, index = mo.fp32_amax_boundary()
    _, s = mo.quantize(mo.groups(x))
    s = s.astype(np.int64)
    assert s.min() == 0 and s.max() == 247
    assert set(range(248)) <= set(s.tolist())
    for e in range(1, 255):
        at, above = s[index[(e, 0x600000)]], s[index[(e, 0x600001)]]
        # m <= 0.875 takes k-9, one step above takes k-8: the scale bytes
        # differ by exactly one wherever the clamp at E = -127 leaves room,
        # i.e. (e-126)-9 >= -127; below that both clamp to byte 0
        if e >= 8:
            assert above - at == 1, (e, at, above)
            assert s[index[(e, 0x5fffff)]] == at
            assert s[index[(e, 0x7fffff)]] == above
        else:
            assert at == 0 and above == 0, (e, at, above)
    for f in (1, 0x400000, 0x7fffff):
        assert s[index[(0, f)]] == 0


def check_ties_coverage():
    x, mid, dn, up = mo.fp32_ties()
    e = mo.encode(mo.groups(x))
    tie = e["tie"].reshape(-1)
    code = e["payload"]
    assert mid.size == 2 * (6 * 126 + int((mo.MID < 56).sum()))
    assert tie[mid].all()
    assert not tie[dn].any() and not tie[up].any()
    assert (code[dn] != code[up]).all()
    # the midpoint goes to the even one of the two
    assert ((code[mid] == code[dn]) | (code[mid] == code[up])).all()
    assert (code[mid] % 2 == 0).all()
    # exactly the midpoints are ties (the anchors and the padding are not)
    assert int(tie.sum()) == mid.size
    scales = set(e["scales"].tolist())
    assert scales == {E + 127 for E in mo.TIE_EXPONENTS}


@functools.lru_cache(maxsize=None)
def check_dequant_all_coverage(dtype):
    pay, sc = mo.dequant_all()
    want = mo.cast(mo.dequantize(pay.numpy(), sc.numpy()), dtype)
    nan = int(torch.isnan(want).sum())
    inf = int(torch.isinf(want).sum())
    assert nan == 766, nan      # 256 under scale 255 + 2 NaN codes x 255
    if dtype == torch.float16:
        assert inf > 560, inf
    else:
        assert inf == 560, inf
    return want, nan, inf


# ------------------------------ the builders -------------------------------

def test_e4m3_table_is_the_format():
    assert mo.E4M3.size == 127 and mo.E4M3[0] == 0 and mo.E4M3[-1] == 448
    assert mo.E4M3[1] == 2.0 ** -9 and mo.E4M3[8] == 2.0 ** -6
    assert (np.diff(mo.E4M3) > 0).all()
    t = (torch.arange(127, dtype=torch.int32).to(torch.uint8)
         .view(torch.float8_e4m3fn).to(torch.float64).numpy())
    assert np.array_equal(t, mo.E4M3)


@pytest.mark.parametrize("dtype", HALVES)
def test_anchored_sweep(C, dtype):
    x = mo.anchored_sweep(dtype)
    assert x.dtype == dtype and 190_000 < x.numel() < 300_000
    sub, zeros, sub_tie = check_anchored_coverage(dtype)
    print(dtype, "elements", x.numel(), "subnormal codes", sub,
          "zeros from nonzero", zeros, "subnormal ties", sub_tie)
    _quantize_three_way(C, x)


def test_fp32_amax_boundary(C):
    x, _ = mo.fp32_amax_boundary()
    check_boundary_coverage()
    _quantize_three_way(C, x)


def test_fp32_ties(C):
    x, _, _, _ = mo.fp32_ties()
    check_ties_coverage()
    _quantize_three_way(C, x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequant_all(C, dtype):
    pay, sc = mo.dequant_all()
    want, nan, inf = check_dequant_all_coverage(dtype)
    print(dtype, "NaN", nan, "inf", inf)
    mo.nan_aware_equal(
        oracle_dequantize_groups(pay, sc).reshape(-1).to(dtype), want,
        "torch oracle")
    mo.nan_aware_equal(C._mx8_dequantize(pay, sc, 65536, dtype), want,
                       "composite")


@pytest.mark.parametrize("pair", mo.SCALE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_reduce_pairs(C, pair):
    pay, sc = mo.reduce_pairs(*pair)
    pn, sn = mo.reduce(pay.numpy(), sc.numpy())
    pt, st, _ = oracle_reduce(list(pay), list(sc))
    pc, scc = C._mx8_reduce(pay, sc)
    mo.bytes_equal(st, sn, "torch oracle scales")
    mo.bytes_equal(pt, pn, "torch oracle payload")
    mo.bytes_equal(scc, sn, "composite scales")
    mo.bytes_equal(pc, pn, "composite payload")
    for dtype in DTYPES:
        want = mo.reduce_to(pay.numpy(), sc.numpy(), 65536, dtype)
        mo.nan_aware_equal(C._mx8_reduce_to(pay, sc, 65536, dtype), want,
                           f"composite reduce_to {dtype}")


def test_reduce_pairs_reach_their_edges():
    def scales_of(pair):
        pay, sc = mo.reduce_pairs(*pair)
        return mo.reduce(pay.numpy(), sc.numpy())[1]

    assert (scales_of((255, 127)) == 255).all()
    s = scales_of((254, 120))               # fp32 overflow to inf
    assert (s == 255).any() and (s != 255).any()
    assert scales_of((0, 0)).min() == 0     # fp32 subnormal sums
    # a finite sum that overflows: 240 * 2^120 plus bytes 64..95 (up to
    # 30 * 2^120) passes 2^128 although every term is finite
    pay, sc = mo.reduce_pairs(247, 247)
    g = 0x77 * 8 + 2
    terms = np.stack([mo.dequantize(pay[r].numpy(), sc[r].numpy())[g]
                      for r in range(2)])
    assert np.isfinite(mo._f32(terms)).all()
    assert scales_of((247, 247))[g] == 255


@pytest.mark.parametrize("P", [3, 5])
def test_rank_order_probe(C, P):
    pay, sc = mo.rank_order_probe(P)
    # the probe discriminates: rank order (and its one equivalent, the first
    # two live copies swapped, a + b == b + a) gives 0 in both groups, every
    # other order of the copies gives 1.0 in one of them
    live = [c for c in range(P) if bool(pay[c].any())]
    assert len(live) == 3 and pay.shape == (P, 64)
    outcomes = mo.rank_order_outcomes(P)
    for perm, got in outcomes.items():
        seq = [p for p in perm if p in live]
        if sorted(seq[:2]) == live[:2]:
            assert got == (0.0, 0.0), (perm, got)
        else:
            assert 1.0 in got and set(got) <= {0.0, 1.0}, (perm, got)
    swapped = list(range(P))
    swapped[live[1]], swapped[live[2]] = live[2], live[1]
    assert outcomes[tuple(swapped)][0] == 1.0     # 2^25, -2^25, 1
    # composite and torch oracle in rank order
    y = C._mx8_reduce_to(pay, sc, 64, torch.float32)
    assert float(y[0]) == 0.0 and float(y[32]) == 0.0
    assert not bool(y.view(torch.int32).any())    # +0.0 everywhere
    p, s = C._mx8_reduce(pay, sc)
    mo.bytes_equal(p, np.zeros(64, dtype=np.uint8))
    mo.bytes_equal(s, np.full(2, 127, dtype=np.uint8))
    pn, sn = mo.reduce(pay.numpy(), sc.numpy())
    mo.bytes_equal(p, pn)
    mo.bytes_equal(s, sn)
    pt, st, _ = oracle_reduce(list(pay), list(sc))
    mo.bytes_equal(pt, pn)
    mo.bytes_equal(st, sn)


def test_overflow_probe(C):
    pay, sc = mo.overflow_probe()
    assert int(sc[0, 0]) == 120 + 127 and int(pay[0, 0]) == 0x77  # 240
    pn, sn = mo.reduce(pay.numpy(), sc.numpy())
    assert sn.tolist() == [255] and not pn.any()
    p, s = C._mx8_reduce(pay, sc)
    mo.bytes_equal(p, pn)
    mo.bytes_equal(s, sn)
    pt, st, _ = oracle_reduce(list(pay), list(sc))
    mo.bytes_equal(pt, pn)
    mo.bytes_equal(st, sn)
    for dtype in (torch.float32, torch.bfloat16):
        want = mo.reduce_to(pay.numpy(), sc.numpy(), 32, dtype)
        assert float(want[0]) == float("inf")
        assert float(want[1]) == mo.OVERFLOW_FINITE
        assert not bool(torch.isnan(want).any())
        mo.nan_aware_equal(C._mx8_reduce_to(pay, sc, 32, dtype), want)


# ------------------- the _blocks and _segments composites ------------------

def _relative_inputs():
    return [("fp16", mo.anchored_sweep(torch.float16)),
            ("bf16", mo.anchored_sweep(torch.bfloat16)),
            ("ties", mo.fp32_ties()[0])]


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_quantize_blocks_composite_is_quantize_of_each_block(C, which, odd):
    name, x = _relative_inputs()[which]
    t, row_elems, streams = mo.as_blocks(
        x, 2, 3, 1 if odd else 8, 2 if odd else 32)
    assert row_elems % 2 == 1 if odd else row_elems % 32 == 8
    p, s = C._mx8_quantize_blocks(t, 2, 3, row_elems)
    for r in range(2):
        pr, sr = C._mx8_quantize(streams[r].contiguous())
        mo.bytes_equal(p[r], pr, f"{name} block {r} payload")
        mo.bytes_equal(s[r], sr, f"{name} block {r} scales")
    pn, sn = mo.quantize_streams(list(streams))
    mo.bytes_equal(p, pn, f"{name} oracle payload")
    mo.bytes_equal(s, sn, f"{name} oracle scales")


@pytest.mark.parametrize("which", [0, 1, 2])
def test_quantize_segments_composite_is_quantize_of_each_segment(C, which):
    name, x = _relative_inputs()[which]
    t, counts, order, segs = mo.as_segments(x, 8, 5, seed=which)
    p, s = C._mx8_quantize_segments(t, 1, 8, counts, order=order)
    qs = [C._mx8_quantize(g.contiguous()) for g in segs if g.numel()]
    mo.bytes_equal(p, torch.cat([q[0] for q in qs]), f"{name} payload")
    mo.bytes_equal(s, torch.cat([q[1] for q in qs]), f"{name} scales")
    pn, sn = mo.quantize_streams(segs)
    mo.bytes_equal(p, pn, f"{name} oracle payload")
    mo.bytes_equal(s, sn, f"{name} oracle scales")
