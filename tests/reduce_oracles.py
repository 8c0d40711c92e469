"""Plain CPU references for the local reduce kernels, shared by the GPU
kernel tests (test_gpu_kernel_edges.py) and the CPU transport tests
(test_reduce_contracts.py). Nothing here calls into the package: every
reference is torch/numpy on CPU tensors, so the kernels and the CPU
composites are both checked against the same independent statement of the
contract.
"""

import functools

import torch

FP8_ENCODINGS = (torch.float8_e4m3fn, torch.float8_e5m2)
FP8_OPS = ("sum", "prod", "min", "max")  # kernel op codes 0..3

PAIRLOC_DTYPES = (torch.float32, torch.float64, torch.float16,
                  torch.bfloat16, torch.int8, torch.uint8, torch.int16,
                  torch.int32, torch.int64)


# ------------------------------- fp8 reduce --------------------------------
#
# Contract: out = torch cast of ((s0 o s1) o s2)... accumulated in fp32 in
# rank order. The cast turns a finite overflow into NaN (e4m3fn) or +-inf
# (e5m2); MIN/MAX propagate NaN (torch.minimum/maximum). Bytes must match
# wherever the reference is not NaN; where it is NaN any NaN byte will do.
#
# One corner is left open by the definition itself: torch.minimum/maximum
# of two zeros of opposite sign returns either zero depending on operand
# order and on whether the element falls in the vectorized body or the
# scalar tail of the CPU loop. Where a MIN/MAX result is zero and the
# sources hold zeros of both signs, a zero byte of either sign is accepted.

def fp8_fold(src_bytes, enc, opname):
    """src_bytes: uint8 [P, n] on CPU. Returns the reference as
    (bytes uint8 [n], is_nan bool [n], zero_sign_free bool [n])."""
    f = src_bytes.view(enc).float()
    acc = f[0].clone()
    for r in range(1, f.shape[0]):
        if opname == "sum":
            acc = acc + f[r]
        elif opname == "prod":
            acc = acc * f[r]
        elif opname == "min":
            acc = torch.minimum(acc, f[r])
        else:
            acc = torch.maximum(acc, f[r])
    ref8 = acc.to(enc)
    nan = torch.isnan(ref8.float())
    free = torch.zeros_like(nan)
    if opname in ("min", "max"):
        free = ((ref8.float() == 0) & (src_bytes == 0x00).any(0)
                & (src_bytes == 0x80).any(0))
    return ref8.view(torch.uint8), nan, free


def fp8_check(got_bytes, enc, ref, what):
    """Assert every element of got_bytes (uint8 [n], CPU) against ref from
    fp8_fold. Returns the share of elements that were compared byte for
    byte."""
    want, nan, free = ref
    assert got_bytes.shape == want.shape, what
    got_nan = torch.isnan(got_bytes.view(enc).float())
    bad_nan = nan & ~got_nan
    assert not bad_nan.any(), (
        what, "want NaN", _first(bad_nan), int(got_bytes[_first(bad_nan)]))
    bad_zero = free & ((got_bytes & 0x7F) != 0)
    assert not bad_zero.any(), (
        what, "want a zero", _first(bad_zero),
        int(got_bytes[_first(bad_zero)]))
    exact = ~nan & ~free
    bad = exact & (got_bytes != want)
    assert not bad.any(), (
        what, "index", _first(bad), "got", int(got_bytes[_first(bad)]),
        "want", int(want[_first(bad)]))
    return exact.sum().item() / max(want.numel(), 1)


def _first(mask):
    return int(mask.nonzero()[0])


def fp8_pair_sources(extra=0):
    """All 65536 byte pairs: source 0 = i // 256, source 1 = i % 256, plus
    `extra` more pairs so the length is no multiple of 16."""
    i = torch.arange(65536 + extra) % 65536
    return torch.stack([(i // 256).to(torch.uint8), (i % 256).to(torch.uint8)])


@functools.lru_cache(maxsize=None)
def fp8_pair_reference(enc, opname, extra=0):
    return fp8_fold(fp8_pair_sources(extra), enc, opname)


# ---------------------------- MINLOC / MAXLOC ------------------------------
#
# Contract: a NaN value wins for both ops (as torch.min/torch.max do) and
# its location is the smallest location among the NaN entries. Otherwise
# the extreme value wins, ties to the smallest location; -0.0 and +0.0 tie
# (which zero is returned is free, so values compare with ==). Integral
# locations compare exactly over the whole int64 range.

def pairloc_oracle(stacked, maxloc):
    """stacked: [P, n, 2] CPU tensor. A direct loop over ranks. Returns
    (best value, best location), float dtypes as float64 (exact for every
    supported float dtype), integral dtypes as int64."""
    wide = torch.float64 if stacked.dtype.is_floating_point else torch.int64
    v = stacked[..., 0].to(wide)
    loc = stacked[..., 1].to(wide)
    bv, bl = v[0].clone(), loc[0].clone()
    for r in range(1, v.shape[0]):
        x, y = v[r], loc[r]
        xn, bn = torch.isnan(x), torch.isnan(bv)
        gt = (x > bv) if maxloc else (x < bv)
        better = (xn & ~bn) | (~xn & ~bn & gt)
        tie = (xn & bn) | (~xn & ~bn & (x == bv))
        take = better | (tie & (y < bl))
        bv = torch.where(take, x, bv)
        bl = torch.where(take, y, bl)
    return bv, bl


def pairloc_check(got, stacked, maxloc, what):
    wide = torch.float64 if stacked.dtype.is_floating_point else torch.int64
    assert got.dtype == stacked.dtype and got.shape == stacked.shape[1:], what
    bv, bl = pairloc_oracle(stacked, maxloc)
    gv, gl = got[..., 0].to(wide), got[..., 1].to(wide)
    okv = (gv == bv) | (torch.isnan(gv) & torch.isnan(bv))
    assert okv.all(), (what, "value at", _first(~okv),
                       gv[_first(~okv)].item(), bv[_first(~okv)].item())
    okl = gl == bl
    assert okl.all(), (what, "location at", _first(~okl),
                       gl[_first(~okl)].item(), bl[_first(~okl)].item())


def _perm_locations(P, n, gen):
    # per-column random permutation of 0..P-1
    return torch.rand(P, n, generator=gen).argsort(0)


def pairloc_cases(dtype, P, n, seed):
    """Yields (name, stacked [P, n, 2]) for one dtype. Values come from a
    handful of levels so ties (and NaNs) occur in most columns; locations
    are a per-column permutation of 0..P-1 times 7, exact in every dtype."""
    gen = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        levels = [float("-inf"), -1.0, -0.0, 0.0, 1.0, float("inf")]
        sets = [("ties", levels), ("nan", levels + [float("nan")] * 2)]
    else:
        info = torch.iinfo(dtype)
        levels = sorted({info.min, min(info.max, max(info.min, -1)), 0, 1,
                         info.max})
        sets = [("ties", levels)]
    for name, lv in sets:
        table = torch.tensor(lv, dtype=torch.float64 if dtype.is_floating_point
                             else torch.int64)
        idx = torch.randint(0, len(lv), (P, n), generator=gen)
        vals = table[idx].to(dtype)
        locs = (_perm_locations(P, n, gen) * 7).to(dtype)
        yield name, torch.stack([vals, locs], dim=-1)
    if dtype == torch.int64:
        # locations a double cannot tell apart, values tied in most columns
        vals = torch.randint(0, 2, (P, n), generator=gen)
        locs = (1 << 62) + _perm_locations(P, n, gen)
        yield "loc2^62", torch.stack([vals, locs], dim=-1)
