"""Plain numpy float64 reference of the mxfp8 codec and the deterministic
input builders of its value-domain tests, shared by the CPU suite
(test_mx8_oracles.py) and the GPU kernel tests (test_gpu_mx8_edges.py).
Nothing here calls into the package or uses torch's fp8 cast: the e4m3fn
table comes from the format definition and rounding is a search over its
midpoints, so the composite in csrc/ops.cpp, the torch oracle of
test_compressed.py and the kernels are all checked against an independent
statement of the contract. torch only carries the tensors and performs the
final cast to the output dtype.

Codec: groups of 32 elements; amax = m * 2^k (frexp, m in [0.5, 1));
E = k-9 if m <= 0.875 else k-8, clamped to [-127, 127], 0 for an all-zero
group; payload = RNE e4m3fn of x * 2^-E; scale byte = E + 127. A group with
an inf or NaN has scale 255 and a zero payload.
"""

import functools
import itertools

import numpy as np
import torch

# The 127 non-negative finite e4m3fn values (code 127 is NaN) and the 126
# midpoints between neighbours.
E4M3 = np.array([(m / 8.0) * 2.0 ** -6 if e == 0
                 else (1 + m / 8.0) * 2.0 ** (e - 7)
                 for e in range(16) for m in range(8)][:127])
MID = (E4M3[1:] + E4M3[:-1]) / 2
# all 256 codes as signed float64, NaN for 0x7f / 0xff
DECODE = np.concatenate([E4M3, [np.nan], -E4M3, [np.nan]])

SCALE_PAIRS = ((127, 127), (127, 130), (130, 127), (0, 0), (0, 3),
               (247, 247), (254, 120), (255, 127))


# ------------------------------- the oracle --------------------------------

def groups(x):
    """flat torch tensor -> [G, 32] float32 numpy, zero-padded"""
    n = x.numel()
    G = (n + 31) // 32
    xp = np.zeros(G * 32, dtype=np.float32)
    xp[:n] = x.reshape(-1).to(torch.float32).numpy()
    return xp.reshape(G, 32)


def encode(xg):
    """[G, 32] float32 -> dict with payload u8 [G*32], scales u8 [G], the
    scaled magnitudes y f64 [G, 32] and tie bool [G, 32] (y on a midpoint);
    y and tie are zero / False in non-finite groups."""
    xg = np.asarray(xg, dtype=np.float32)
    x = xg.astype(np.float64)
    fin = np.isfinite(x).all(1)
    ax = np.where(fin[:, None], np.abs(x), 0.0)
    amax = ax.max(1)
    mant, k = np.frexp(amax)
    E = np.where(mant <= 0.875, k - 9, k - 8)
    E = np.where(amax == 0, 0, E).clip(-127, 127).astype(np.int64)
    y = np.ldexp(ax, -E[:, None])          # exact: a power-of-two scale
    assert y.max(initial=0.0) <= 448.0
    lo = np.searchsorted(MID, y, side="left")   # MID[lo-1] < y <= MID[lo]
    tie = (lo < 126) & (y == MID[np.minimum(lo, 125)])
    code = np.where(tie & (lo % 2 == 1), lo + 1, lo).astype(np.uint8)
    code |= np.signbit(xg).astype(np.uint8) << 7
    code = np.where(fin[:, None], code, 0).astype(np.uint8)
    scales = np.where(fin, E + 127, 255).astype(np.uint8)
    return {"payload": code.reshape(-1), "scales": scales, "y": y,
            "tie": tie & fin[:, None]}


def quantize(xg):
    e = encode(xg)
    return e["payload"], e["scales"]


def dequantize(payload, scales):
    """u8 [G*32], u8 [G] -> float64 [G, 32]: value * 2^(s-127); the NaN
    codes and scale 255 give NaN."""
    payload = np.asarray(payload, dtype=np.uint8)
    scales = np.asarray(scales, dtype=np.uint8)
    v = DECODE[payload.reshape(scales.size, 32)]
    d = np.ldexp(v, scales.astype(np.int64)[:, None] - 127)
    return np.where((scales == 255)[:, None], np.nan, d)


def _f32(d):
    # the products are exact in fp32 or overflow to inf
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(d).astype(np.float32)


def cast(d, dtype, numel=None):
    """float64/float32 array -> flat torch tensor of `dtype`, through
    float32 and torch's .to(dtype)."""
    t = torch.from_numpy(np.ascontiguousarray(_f32(d)).reshape(-1))
    if numel is not None:
        t = t[:numel]
    return t.to(dtype)


def _rank_sum(payloads, scales):
    payloads, scales = np.asarray(payloads), np.asarray(scales)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = _f32(dequantize(payloads[0], scales[0]))
        for r in range(1, payloads.shape[0]):
            acc = acc + _f32(dequantize(payloads[r], scales[r]))
    assert acc.dtype == np.float32
    return acc


def reduce(payloads, scales):
    """u8 [P, G*32], u8 [P, G] -> (payload, scales): float32 adds in rank
    order, then quantize."""
    return quantize(_rank_sum(payloads, scales))


def reduce_to(payloads, scales, numel, dtype):
    return cast(_rank_sum(payloads, scales), dtype, numel)


def nan_aware_equal(got, want, what=""):
    """torch tensors: NaN at the same positions, every other element byte
    for byte (signed zeros and infinities included)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (
        what, got.dtype, want.dtype, got.shape, want.shape)
    got, want = got.contiguous().view(-1), want.contiguous().view(-1)
    ng, nw = torch.isnan(got), torch.isnan(want)
    assert torch.equal(ng, nw), (what, "NaN positions differ",
                                 int((ng != nw).nonzero()[0]))
    bits = {4: torch.int32, 2: torch.int16}[got.element_size()]
    bad = (got.view(bits) != want.view(bits)) & ~nw
    assert not bool(bad.any()), (
        what, "index", int(bad.nonzero()[0]),
        "got", float(got[int(bad.nonzero()[0])]),
        "want", float(want[int(bad.nonzero()[0])]))


def bytes_equal(got, want, what=""):
    """uint8 torch tensor against a numpy/torch reference"""
    if isinstance(want, np.ndarray):
        want = torch.from_numpy(want)
    got, want = got.contiguous().view(-1), want.contiguous().view(-1)
    assert got.dtype == torch.uint8 and want.dtype == torch.uint8, what
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), (
        what, int(bad.sum()), "bytes differ, first at",
        int(bad.nonzero()[0]), "got", int(got[int(bad.nonzero()[0])]),
        "want", int(want[int(bad.nonzero()[0])]))


# ------------------------------ input builders -----------------------------
#
# Every builder is cached and its result is shared: treat it as read-only.

_NONFINITE = {torch.float16: (0x7c00, 0xfc00, 0x7e00, 0xfe01),
              torch.bfloat16: (0x7f80, 0xff80, 0x7fc0, 0xffc1)}


def _next_up(v, dtype):
    t = torch.tensor(v, dtype=dtype)
    return float((t.view(torch.int16) + 1).view(dtype))


def anchors(dtype):
    a = [1.0, 1.75, _next_up(1.75, dtype),
         float((torch.tensor(2.0, dtype=dtype).view(torch.int16) - 1)
               .view(dtype)),
         1.75 * 2.0 ** -10, 2.0 ** 10]
    if dtype == torch.bfloat16:
        a += [2.0 ** -120, 1.5 * 2.0 ** 120, 2.0 ** -126]
    return a


@functools.lru_cache(maxsize=None)
def anchored_sweep(dtype):
    """Every finite 16-bit pattern v with |v| <= A, 31 per group, the anchor
    A in the 32nd position (which moves with the anchor), for each anchor;
    then one group per non-finite class (+inf, -inf, quiet NaN, negative
    NaN). Flat tensor of `dtype`, a whole number of groups."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype)
    vf = v[torch.isfinite(v.float())]
    mags = vf.float().abs()
    out = []
    for j, A in enumerate(anchors(dtype)):
        assert float(torch.tensor(A, dtype=dtype)) == A  # representable
        sel = vf[mags <= A]
        n = sel.numel()
        G = (n + 30) // 31
        pad = torch.zeros(G * 31, dtype=dtype)
        pad[:n] = sel
        g = torch.empty(G, 32, dtype=dtype)
        pos = j * 5 % 32
        g[:, [i for i in range(32) if i != pos]] = pad.view(G, 31)
        g[:, pos] = A
        out.append(g)
    special = torch.ones(4, 32, dtype=dtype)
    for j, pat in enumerate(_NONFINITE[dtype]):
        special[j, 7 * j + 3] = torch.tensor(
            pat - 65536 if pat >= 32768 else pat,
            dtype=torch.int16).view(dtype)
    assert not bool(torch.isfinite(special.float()).all(1).any())
    out.append(special)
    return torch.cat(out).reshape(-1).contiguous()


BOUNDARY_MANTISSAS = (0x5fffff, 0x600000, 0x600001, 0, 0x7fffff)


@functools.lru_cache(maxsize=None)
def fp32_amax_boundary():
    """(x, index): for every fp32 exponent field 1..254 one group per amax
    mantissa in BOUNDARY_MANTISSAS, each group also holding -amax/3 and
    amax*2^-12; then exponent field 0 with mantissas 1, 0x400000, 0x7fffff.
    index[(field, mantissa)] is the group number."""
    rows, index = [], {}
    cases = [(e, f) for f in BOUNDARY_MANTISSAS for e in range(1, 255)]
    cases += [(0, f) for f in (1, 0x400000, 0x7fffff)]
    for g, (e, f) in enumerate(cases):
        a = np.array([(e << 23) | f], dtype=np.uint32).view(np.float32)[0]
        row = np.zeros(32, dtype=np.float32)
        row[(3 + g) % 32] = a
        row[(4 + g) % 32] = -a / np.float32(3)
        row[(5 + g) % 32] = a * np.float32(2.0 ** -12)
        rows.append(row)
        index[(e, f)] = g
    return torch.from_numpy(np.stack(rows).reshape(-1)), index


TIE_EXPONENTS = (-127, -126, -1, 0, 64, 119)


@functools.lru_cache(maxsize=None)
def fp32_ties():
    """(x, mid, down, up): for each E in TIE_EXPONENTS groups anchored at
    448 * 2^E whose elements are all 126 table midpoints times 2^E, each
    with its fp32 neighbours towards zero and away from it, in both signs;
    then the clamped case, anchor 448 * 2^-130 (E clamps to -127, the amax
    scales to 56) with the midpoints below 56. mid/down/up are index arrays
    into x, aligned entry by entry."""
    chunks, mid_i, dn_i, up_i = [], [], [], []
    base = 0
    for c, (E, anchor_exp) in enumerate(
            [(E, E) for E in TIE_EXPONENTS] + [(-127, -130)]):
        anchor = np.float32(np.ldexp(448.0, anchor_exp))
        m64 = np.ldexp(MID, E)
        m = m64.astype(np.float32)
        assert np.array_equal(m.astype(np.float64), m64)  # representable
        up = np.nextafter(m, np.float32(np.inf))
        dn = np.nextafter(m, np.float32(0))
        keep = up <= anchor
        assert keep.sum() == (126 if anchor_exp == E else int((MID < 56).sum()))
        tri = np.stack([m, dn, up], 1)[keep]          # [K, 3]
        vals = np.concatenate([tri, -tri]).reshape(-1)   # sign-major
        K = vals.size
        G = (K + 30) // 31
        pos = (c * 5 + 3) % 32
        slots = np.array([i for i in range(32) if i != pos])
        g = np.zeros((G, 32), dtype=np.float32)
        g[:, pos] = anchor
        flat = (np.arange(G)[:, None] * 32 + slots[None, :]).reshape(-1)[:K]
        g.reshape(-1)[flat] = vals
        where = (base + flat).reshape(-1, 3)
        mid_i.append(where[:, 0])
        dn_i.append(where[:, 1])
        up_i.append(where[:, 2])
        chunks.append(g.reshape(-1))
        base += G * 32
    return (torch.from_numpy(np.concatenate(chunks)),
            np.concatenate(mid_i), np.concatenate(dn_i), np.concatenate(up_i))


@functools.lru_cache(maxsize=None)
def dequant_all():
    """(payload u8 [65536], scales u8 [2048]): 256 scale bytes x 256 payload
    bytes, 8 groups per scale holding bytes 0..255."""
    pay = torch.arange(256, dtype=torch.int32).to(torch.uint8).repeat(256)
    sc = (torch.arange(256, dtype=torch.int32).to(torch.uint8)
          .repeat_interleave(8))
    return pay.contiguous(), sc.contiguous()


@functools.lru_cache(maxsize=None)
def reduce_pairs(s0, s1):
    """(payload u8 [2, 65536], scales u8 [2, 2048]): all byte pairs, copy 0
    byte idx // 256 under scale s0, copy 1 byte idx % 256 under scale s1."""
    i = torch.arange(65536, dtype=torch.int32)
    pay = torch.stack([(i // 256).to(torch.uint8), (i % 256).to(torch.uint8)])
    sc = torch.stack([torch.full((2048,), s0, dtype=torch.uint8),
                      torch.full((2048,), s1, dtype=torch.uint8)])
    return pay.contiguous(), sc.contiguous()


def _stack_quantized(copies):
    """list of [G, 32] float32 arrays -> (payload u8 [P, G*32], scales u8
    [P, G]) as torch tensors, quantized by the oracle"""
    qs = [quantize(c) for c in copies]
    return (torch.from_numpy(np.stack([q[0] for q in qs])),
            torch.from_numpy(np.stack([q[1] for q in qs])))


@functools.lru_cache(maxsize=None)
def rank_order_probe(P=3):
    """(payload [P, 64], scales [P, 2]). Group 0 holds 2^25, 1, -2^25 at
    element 0 of the first, middle and last copy: fp32 adds in rank order
    give (2^25 + 1) - 2^25 = 0, an order that brings 2^25 and -2^25 together
    first gives 1. Group 1 holds 1, 2^25, -2^25 in the same copies, which
    gives 1 for the orders group 0 cannot tell from rank order (the reversed
    one among them). With P = 5 copies 1 and 3 are all zero. Every value is
    an e4m3 code times a power of two, so quantization is exact."""
    assert P in (3, 5)
    live = (0, 1, 2) if P == 3 else (0, 2, 4)
    copies = [np.zeros((2, 32), dtype=np.float32) for _ in range(P)]
    for c, v0, v1 in zip(live, (2.0 ** 25, 1.0, -2.0 ** 25),
                         (1.0, 2.0 ** 25, -2.0 ** 25)):
        copies[c][0, 0] = v0
        copies[c][1, 0] = v1
    return _stack_quantized(copies)


def rank_order_outcomes(P=3):
    """{permutation of the copies: (group 0 element 0, group 1 element 0)}
    of the oracle's reduce_to"""
    pay, sc = rank_order_probe(P)
    out = {}
    for perm in itertools.permutations(range(P)):
        y = reduce_to(pay.numpy()[list(perm)], sc.numpy()[list(perm)], 64,
                      torch.float32)
        out[perm] = (float(y[0]), float(y[32]))
    return out


OVERFLOW_FINITE = 32.0 * 2.0 ** 120


@functools.lru_cache(maxsize=None)
def overflow_probe():
    """(payload [2, 32], scales [2, 1]): two copies of 240 * 2^120 at
    element 0, whose fp32 sum overflows, and of 16 * 2^120 at element 1,
    whose sum is OVERFLOW_FINITE."""
    g = np.zeros((1, 32), dtype=np.float32)
    g[0, 0] = np.float32(240.0 * 2.0 ** 120)
    g[0, 1] = np.float32(16.0 * 2.0 ** 120)
    return _stack_quantized([g, g.copy()])


# ------------- the same values through the _blocks / _segments layouts -----

def as_blocks(x, nblocks, rows, row_residue, modulus):
    """Lay the flat stream x (a whole number of groups) out as the input of
    quantize_blocks: the groups are dealt to `nblocks` streams at group
    boundaries, every stream zero-padded to L = rows * row_elems with
    row_elems the smallest length that holds it and has row_elems % modulus
    == row_residue. Returns (flat [rows][nblocks][row_elems] tensor,
    row_elems, streams [nblocks, L]): block r of the tensor is streams[r],
    whose groups coincide with groups of x."""
    assert x.numel() % 32 == 0
    G = x.numel() // 32
    per = (G + nblocks - 1) // nblocks * 32
    row_elems = (per + rows - 1) // rows
    while row_elems % modulus != row_residue:
        row_elems += 1
    L = rows * row_elems
    streams = torch.zeros(nblocks, L, dtype=x.dtype)
    for r in range(nblocks):
        part = x[r * per:(r + 1) * per]
        streams[r, :part.numel()] = part
    t = streams.view(nblocks, rows, row_elems).transpose(0, 1).contiguous()
    return t.view(-1), row_elems, streams


def as_segments(x, after, head_slices, seed):
    """Lay the flat stream x (a whole number of groups) out as the input of
    quantize_segments with rows = 1, counts = [head_slices, 0, rest] and an
    order: segment 0 is the first head_slices * after elements of x,
    segment 2 all of x zero-padded to whole slices, and the slices are
    scattered through a random permutation. Returns (flat [1][S][after]
    tensor, counts, order, segment streams)."""
    assert x.numel() % 32 == 0
    rest = (x.numel() + after - 1) // after
    body = torch.zeros(rest * after, dtype=x.dtype)
    body[:x.numel()] = x
    head = x[:head_slices * after].clone()
    stream = torch.cat([head, body]).view(head_slices + rest, after)
    S = head_slices + rest
    order = torch.randperm(S, generator=torch.Generator().manual_seed(seed))
    t = torch.empty_like(stream)
    t[order] = stream          # stream slice j is tensor slice order[j]
    return (t.view(-1).contiguous(), [head_slices, 0, rest], order,
            [head, torch.empty(0, dtype=x.dtype), body])


def quantize_streams(streams):
    """Oracle payload and scales of a list of contiguous streams, each
    padded to whole groups, concatenated: what the _blocks and _segments
    kernels emit."""
    qs = [quantize(groups(s)) for s in streams if s.numel()]
    return (np.concatenate([q[0] for q in qs]),
            np.concatenate([q[1] for q in qs]))
