"""GPU tests of the four older kernel families in csrc/kernels.hip at their
edges: special values, ties, alignment phases and stray writes.

fp8 reduce is checked over every pair of input bytes; MINLOC/MAXLOC over
value sets made of ties, signed zeros, infinities and NaN; bitwise reduce on
both of its paths with more than one source; the slab copy over every
(source phase, destination phase) with guard bytes around each destination.
arith_reduce MIN/MAX are pinned to the fminf/fmaxf rule on inputs with NaN.

Every reference is plain torch/numpy on the CPU (tests/reduce_oracles.py),
never the package's own composite.
"""

import os

import numpy as np
import pytest
import torch

import reduce_oracles as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world1():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29551")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    import torch.distributed as dist

    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    import mpi4torch_amd as m

    m.init()
    return m


def _enc_id(enc):
    return str(enc).replace("torch.float8_", "")


# ------------------------------- fp8 reduce --------------------------------

def _fp8_run(m, src_bytes, enc, op, misalign=False):
    """src_bytes: uint8 [P, n] on CPU -> result bytes uint8 [n] on CPU."""
    P, n = src_bytes.shape
    if misalign:
        buf = torch.empty(P * n + 1, dtype=torch.uint8, device="cuda")
        stacked = buf[1:].view(P, n)  # contiguous, base off by one byte
        stacked.copy_(src_bytes)
        assert stacked.data_ptr() % 16 != 0
    else:
        stacked = src_bytes.cuda()
        assert stacked.data_ptr() % 16 == 0
    out = m._C._fp8_reduce(stacked.view(enc), op)
    assert out.dtype == enc and out.shape == (n,)
    return out.view(torch.uint8).cpu()


@pytest.mark.parametrize("opname", ro.FP8_OPS)
@pytest.mark.parametrize("enc", ro.FP8_ENCODINGS, ids=_enc_id)
def test_fp8_reduce_all_pairs(world1, enc, opname):
    m = world1
    op = ro.FP8_OPS.index(opname)
    ref = ro.fp8_pair_reference(enc, opname)
    ref3 = ro.fp8_pair_reference(enc, opname, 3)
    src, src3 = ro.fp8_pair_sources(), ro.fp8_pair_sources(3)
    # vector path; scalar path by length; scalar path by misaligned base
    share = ro.fp8_check(_fp8_run(m, src, enc, op), enc, ref,
                         (enc, opname, "vector"))
    ro.fp8_check(_fp8_run(m, src3, enc, op), enc, ref3,
                 (enc, opname, "n=65539"))
    ro.fp8_check(_fp8_run(m, src, enc, op, misalign=True), enc, ref,
                 (enc, opname, "misaligned"))
    # the loose NaN comparison must not swallow the test
    assert share >= 0.8, (enc, opname, share)


@pytest.mark.parametrize("enc", ro.FP8_ENCODINGS, ids=_enc_id)
def test_fp8_reduce_rank_order_single_rounding(world1, enc):
    m = world1
    gen = torch.Generator().manual_seed(4099)
    n = 4099
    for P in (3, 8):
        src = torch.randint(0, 256, (P, n), dtype=torch.uint8, generator=gen)
        for op, opname in enumerate(ro.FP8_OPS):
            ref = ro.fp8_fold(src, enc, opname)
            ro.fp8_check(_fp8_run(m, src, enc, op), enc, ref,
                         (enc, opname, P))


# --------------------------- arith_reduce with NaN -------------------------

ARITH_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _bits(t):
    return t.contiguous().view(
        {1: torch.uint8, 2: torch.int16, 4: torch.int32,
         8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("dtype", ARITH_DTYPES, ids=("bf16", "fp16", "fp32"))
def test_arith_reduce_minmax_nan(world1, dtype):
    """MIN/MAX follow fminf/fmaxf: a NaN source is skipped, the result is
    NaN only where every source is."""
    m = world1
    P = 5
    gen = torch.Generator().manual_seed(97)
    for n in (8, 4097):
        src = (torch.randn(P, n, generator=gen) * 3).to(dtype)
        src[torch.rand(P, n, generator=gen) < 0.01] = float("nan")
        src[:, 1] = float("nan")          # NaN in every source
        src[:, 2] = torch.arange(P).to(dtype)
        src[0, 2] = float("nan")          # NaN only in source 0
        for opname, op, fn in (("min", m.MPI_MIN, torch.fmin),
                               ("max", m.MPI_MAX, torch.fmax)):
            acc = src[0].float()
            for r in range(1, P):
                acc = fn(acc, src[r].float())
            want = acc.to(dtype)
            nan = torch.isnan(want)
            assert nan[1] and not nan[2]
            for me in (0, P - 1):
                rest = torch.cat([src[:me], src[me + 1:]])
                per_vec = 16 // src.element_size()
                slot = (n + per_vec - 1) // per_vec * per_vec
                slotted = torch.zeros(P - 1, slot, dtype=dtype, device="cuda")
                slotted[:, :n].copy_(rest)
                for staged in (rest.cuda(), slotted[:, :n]):
                    got = m._C._arith_reduce(src[me].cuda(), staged, me,
                                             op).cpu()
                    what = (dtype, n, opname, me, staged.stride(0))
                    assert torch.equal(torch.isnan(got), nan), what
                    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), what


# ---------------------------- MINLOC / MAXLOC ------------------------------

@pytest.mark.parametrize("dtype", ro.PAIRLOC_DTYPES,
                         ids=lambda d: str(d).replace("torch.", ""))
def test_pairloc_reduce_ties_nan(world1, dtype):
    m = world1
    for P in (1, 2, 6):
        for n in (1, 1027):
            for name, stacked in ro.pairloc_cases(dtype, P, n, seed=31 * P + n):
                for op in (0, 1):  # minloc, maxloc
                    got = m._C._pairloc_reduce(stacked.cuda(), op).cpu()
                    ro.pairloc_check(got, stacked, op == 1,
                                     (dtype, P, n, name, op))


# ----------------------------- bitwise reduce ------------------------------

_BIT_OPS = ((0, np.bitwise_and), (1, np.bitwise_or), (2, np.bitwise_xor))

# (dtype, elements, base off by one byte, takes the 16-byte path)
_BIT_CASES = (
    (torch.int32, 4096, False, True),    # 16384 B
    (torch.int64, 4098, False, True),    # 32784 B
    (torch.uint8, 1, False, False),
    (torch.uint8, 15, False, False),
    (torch.uint8, 16, False, True),
    (torch.uint8, 4097, False, False),
    (torch.int32, 4096, True, False),    # byte path by misalignment
)


@pytest.mark.parametrize("P", (1, 2, 5, 8))
def test_bitwise_reduce_both_paths(world1, P):
    m = world1
    rng = np.random.default_rng(1000 + P)
    for dtype, n, misalign, want_vec in _BIT_CASES:
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        raw = rng.integers(0, 256, (P, nbytes), dtype=np.uint8)  # all bits
        if misalign:
            # the kernel is dtype-blind, so the same bytes go in as uint8
            # (a wider dtype cannot be viewed at an odd byte offset)
            buf = torch.empty(P * nbytes + 1, dtype=torch.uint8, device="cuda")
            stacked = buf[1:].view(P, nbytes)
            stacked.copy_(torch.from_numpy(raw))
        else:
            stacked = torch.from_numpy(raw).cuda().view(dtype)
            assert stacked.shape == (P, n)
        chunk_b = stacked[0].numel() * stacked.element_size()
        vec = chunk_b % 16 == 0 and stacked.data_ptr() % 16 == 0
        assert vec == want_vec, (dtype, n, misalign)
        for op, fn in _BIT_OPS:
            out = m._C._bitwise_reduce(stacked, op)
            assert out.data_ptr() % 16 == 0  # else the byte path is taken
            assert out.dtype == stacked.dtype and out.shape == stacked.shape[1:]
            got = out.view(torch.uint8).cpu().numpy().reshape(-1)
            want = fn.reduce(raw, axis=0)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (dtype, n, misalign, P, op, int(bad[0]),
                                   int(got[bad[0]]), int(want[bad[0]]))


# -------------------------------- slab copy --------------------------------

_GUARD = 64
_FILL = 0xA5
_ROW_BYTES = (0, 1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257)


def _granule(delta, pdelta):
    """Which kernel launch_slab_copy picks: the 16/8/4-byte granule copy,
    or (1) the byte-window kernel for a sub-dword phase difference."""
    for g in (16, 8, 4):
        if delta % g == 0 and pdelta % g == 0:
            return g
    return 1


def _slab_run(m, slabs, rng):
    """slabs: list of (src_phase, dst_phase, before, row_b, src_pitch,
    dst_pitch). Lays every slab out in its own source and destination
    region (64 guard bytes around each), copies them all with one
    _slab_copy call and compares the WHOLE destination buffer with a numpy
    expectation. Returns the copy granule of every descriptor."""
    descs, soff, doff = [], _GUARD, 0
    for sp, dp, before, row_b, spitch, dpitch in slabs:
        s0 = (soff + 15) // 16 * 16 + sp
        d0 = (doff + _GUARD + 15) // 16 * 16 + dp
        rows = max(before - 1, 0)
        # (count, after_b) collapse into one row; split it where it divides
        count = 3 if row_b % 3 == 0 else 1
        descs.append((s0, d0, before, count, row_b // count, spitch, dpitch))
        soff = s0 + rows * spitch + row_b
        doff = d0 + rows * dpitch + row_b + _GUARD
    src_np = rng.integers(0, 256, soff + _GUARD, dtype=np.uint8)
    want = np.full(doff, _FILL, dtype=np.uint8)
    for s0, d0, before, count, after_b, spitch, dpitch in descs:
        row_b = count * after_b
        for b in range(before):
            want[d0 + b * dpitch:d0 + b * dpitch + row_b] = \
                src_np[s0 + b * spitch:s0 + b * spitch + row_b]
    src = torch.from_numpy(src_np).cuda()
    dst = torch.full((doff,), _FILL, dtype=torch.uint8, device="cuda")
    # offsets are phases only if the allocations start on a 16-byte line
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    m._C._slab_copy(src, dst, descs)
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    if bad.size:
        k = int(bad[0])
        owner = max(i for i, d in enumerate(descs) if d[1] - _GUARD <= k)
        raise AssertionError(("first wrong byte", k, int(got[k]),
                              int(want[k]), "slab", slabs[owner],
                              "desc", descs[owner], "wrong bytes", bad.size))
    return [_granule(d[0] - d[1], d[5] - d[6]) for d in descs]


@pytest.mark.parametrize("pdiff", (0, 1, 2, 4, 8, 16))
@pytest.mark.parametrize("before", (1, 3))
def test_slab_copy_all_phases(world1, before, pdiff):
    """Every (source phase, destination phase, row length) in one launch
    sequence, in an order that mixes copy granules."""
    m = world1
    rng = np.random.default_rng(16 * before + pdiff)
    slabs = []
    for sp in range(16):
        for dp in range(16):
            for k, row_b in enumerate(_ROW_BYTES):
                # pitches >= the row; the padding varies so the rows of one
                # slab start at different phases
                dpitch = row_b + (sp + dp + k) % 5
                slabs.append((sp, dp, before, row_b, dpitch + pdiff, dpitch))
    order = rng.permutation(len(slabs))
    slabs = [slabs[i] for i in order]
    gran = _slab_run(m, slabs, rng)
    # the order really splits the buckets of launch_slab_copy and really
    # puts more than one launch's worth (8) of unequal slabs in a bucket
    runs, start = [], 0
    for i in range(1, len(gran) + 1):
        if i == len(gran) or gran[i] != gran[start]:
            runs.append(i - start)
            start = i
    assert max(runs) > 8
    # a sub-dword pitch difference leaves only the byte-window kernel
    kernels = {0: {16, 8, 4, 1}, 1: {1}, 2: {1}, 4: {4, 1}, 8: {8, 4, 1},
               16: {16, 8, 4, 1}}[pdiff]
    assert set(gran) == kernels
    assert len(kernels) == 1 or len(runs) > 100


@pytest.mark.parametrize("phases", ((0, 0), (1, 6)))
def test_slab_copy_grid_wraps(world1, phases):
    """One row of 16 MiB + 3 B: one more 16-byte chunk than the 4096 x 256
    threads of the capped grid, so the grid-stride loop runs twice."""
    m = world1
    row_b = (16 << 20) + 3
    assert row_b // 16 + 1 > 4096 * 256
    rng = np.random.default_rng(7)
    _slab_run(m, [(phases[0], phases[1], 1, row_b, row_b, row_b)], rng)


def test_slab_copy_rejects_bad_descriptors(world1):
    m = world1
    src = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), _FILL, dtype=torch.uint8, device="cuda")
    bad = [
        [(0, 0, 1, 1, 257, 257, 257)],                 # row longer than both
        [(200, 0, 3, 1, 20, 20, 20)],                  # src runs past the end
        [(0, 200, 3, 1, 20, 20, 20)],                  # dst runs past the end
        [(-1, 0, 1, 1, 4, 4, 4)],                      # negative offset
        [(0, 0, 2, 1, 8, 8, 4)],                       # dst rows overlap
        [(0, 0, 1, 1, 32, 32, 32), (64, 16, 1, 1, 32, 32, 32)],  # dst overlap
        [(0, 0, 1, 1, 4, 4)],                          # short descriptor
    ]
    for descs in bad:
        with pytest.raises(RuntimeError):
            m._C._slab_copy(src, dst, descs)
    with pytest.raises(RuntimeError):
        m._C._slab_copy(dst, dst, [(0, 128, 1, 1, 8, 8, 8)])  # aliasing
    torch.cuda.synchronize()
    assert (dst == _FILL).all()  # nothing was launched
    m._C._slab_copy(src, dst, [(0, 8, 2, 2, 4, 16, 16)])
    want = torch.full((256,), _FILL, dtype=torch.uint8)
    want[8:16] = 0
    want[24:32] = 0
    assert torch.equal(dst.cpu(), want)
