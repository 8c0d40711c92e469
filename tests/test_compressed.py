"""AllreduceCompressed (mxfp8 wire): codec semantics, accuracy bound, SPMD
worlds on gloo, autograd, error checks, DDP gradient compression.

The oracle below is a pure-torch statement of the codec (torch.frexp,
torch.ldexp, .to(float8_e4m3fn)), written independently of the C++
composite in csrc/ops.cpp that defines the semantics for the kernels; the
two must agree byte for byte.
"""

import copy

import pytest
import torch

import mpi4torch_amd as m  # module-level so TorchScript resolves m.MPI_Communicator
from spmd import run_spmd

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
UNIT_ROUNDOFF = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8,
                 torch.float16: 2.0 ** -11}


# ------------------------------ the oracle --------------------------------

def _groups(x):
    """flat tensor -> [G, 32] fp32, zero-padded"""
    n = x.numel()
    G = (n + 31) // 32
    xp = torch.zeros(G * 32, dtype=torch.float32)
    xp[:n] = x.reshape(-1).to(torch.float32)
    return xp.view(G, 32)


def oracle_quantize_groups(xg):
    finite = torch.isfinite(xg).all(dim=1)
    amax = torch.where(finite, xg.abs().amax(dim=1), torch.zeros(()))
    mant, k = torch.frexp(amax)
    E = torch.where(mant <= 0.875, k - 9, k - 8)
    E = torch.where(amax == 0, torch.zeros_like(E), E).clamp(-127, 127)
    scaled = torch.ldexp(xg, (-E).unsqueeze(1))
    payload = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    payload = torch.where(finite.unsqueeze(1), payload,
                          torch.zeros_like(payload))
    scales = torch.where(finite, E + 127, torch.full_like(E, 255))
    return payload.reshape(-1), scales.to(torch.uint8)


def oracle_quantize(x):
    return oracle_quantize_groups(_groups(x))


def oracle_dequantize_groups(payload, scales):
    G = scales.numel()
    v = payload.view(G, 32).view(torch.float8_e4m3fn).to(torch.float32)
    d = torch.ldexp(v, (scales.to(torch.int32) - 127).unsqueeze(1))
    return torch.where((scales == 255).unsqueeze(1),
                       torch.full_like(d, float("nan")), d)


def oracle_reduce(payloads, scales):
    """P copies -> (payload, scales, S) with S the fp32 rank-order sum"""
    S = oracle_dequantize_groups(payloads[0], scales[0])
    for r in range(1, len(payloads)):
        S = S + oracle_dequantize_groups(payloads[r], scales[r])
    p, s = oracle_quantize_groups(S)
    return p, s, S


def oracle_allreduce(xs):
    """All ranks' inputs -> what AllreduceCompressed returns on every rank."""
    qs = [oracle_quantize(x) for x in xs]
    p, s, _ = oracle_reduce([q[0] for q in qs], [q[1] for q in qs])
    n = xs[0].numel()
    out = oracle_dequantize_groups(p, s).reshape(-1)[:n].to(xs[0].dtype)
    return out.view(xs[0].shape)


def allreduce_bound(xs, out):
    """Per-element bound on |out - sum_r x_r| (derived, not tuned): each of
    the two quantizations obeys |q(x) - x| <= |x|/16 + amax_group * 2^-17
    (half an ulp of a 3-bit mantissa; e4m3 subnormal half-spacing relative
    to a group maximum that scales above 224), plus the output rounding
    |out| * u."""
    n = xs[0].numel()
    bound = torch.zeros(_groups(xs[0]).shape, dtype=torch.float64)
    S = None
    for x in xs:
        g = _groups(x).double()
        bound += g.abs() / 16 + g.abs().amax(dim=1, keepdim=True) * 2.0 ** -17
        d = oracle_dequantize_groups(*oracle_quantize(x))
        S = d if S is None else S + d
    Sd = S.double()
    bound += Sd.abs() / 16 + Sd.abs().amax(dim=1, keepdim=True) * 2.0 ** -17
    bound = bound.reshape(-1)[:n]
    return bound + out.reshape(-1).double().abs() * UNIT_ROUNDOFF[out.dtype]


def _bytes_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype,
                                                       a.shape, b.shape)
    assert torch.equal(a.contiguous().view(torch.uint8),
                       b.contiguous().view(torch.uint8))


def _rand_input(n, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    G = (n + 31) // 32
    x = torch.randn(G, 32, generator=g) * scale * torch.rand(G, 1, generator=g)
    return x.reshape(-1)[:n].to(dtype)


def _with_specials(x):
    """Plant the special groups where the tensor has room for them."""
    x = x.clone()
    n = x.numel()
    if n >= 32 * 6:
        x[32 + 7] = 0.0                       # an exact-zero element
        x[64:96] = 0.0                        # an all-zero group
        x[96:128] = x[96:128].float().clamp(-1, 1).to(x.dtype)
        x[96 + 5] = 448.0 * 2.0 ** -3         # amax exactly 448 * 2^j
        x[128 + 9] = float("inf")             # one inf in a group
    return x


@pytest.fixture(scope="module")
def C():
    import mpi4torch_amd as m

    return m._C


# --------------------------- codec vs the oracle --------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1e-6, 3e4])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4099])
def test_codec_matches_oracle(C, n, scale, dtype):
    x = _with_specials(_rand_input(n, dtype, seed=n, scale=scale))
    p, s = C._mx8_quantize(x)
    po, so = oracle_quantize(x)
    assert p.dtype == torch.uint8 and s.dtype == torch.uint8
    _bytes_equal(s, so)
    _bytes_equal(p, po)
    y = C._mx8_dequantize(p, s, n, dtype)
    yo = oracle_dequantize_groups(po, so).reshape(-1)[:n].to(dtype)
    _bytes_equal(y, yo)
    for P in (1, 2, 5, 8):
        xs = [_with_specials(_rand_input(n, dtype, seed=97 * r + n + 1,
                                         scale=scale))
              if r != 1 else _rand_input(n, dtype, seed=5, scale=scale)
              for r in range(P)]
        qs = [C._mx8_quantize(t) for t in xs]
        rp, rs = C._mx8_reduce(torch.stack([q[0] for q in qs]),
                               torch.stack([q[1] for q in qs]))
        op_, os_, _ = oracle_reduce([q[0] for q in qs], [q[1] for q in qs])
        _bytes_equal(rs, os_)
        _bytes_equal(rp, op_)


@pytest.mark.parametrize("P", [1, 5])
def test_codec_clamped_exponent_region(C, P):
    """Groups whose amax is tiny or an fp32 subnormal: E clamps at -127,
    the scaled values sit below 448 and dequantized values are fp32
    subnormals. Composite and oracle must still agree byte for byte."""
    n = 32 * 40 + 7
    xs = [_rand_input(n, torch.float32, seed=400 + r, scale=4e-38)
          for r in range(P)]
    assert bool((xs[0].abs() < 2.0 ** -126).any())      # fp32 subnormals
    qs = [C._mx8_quantize(x) for x in xs]
    for x, (p, s) in zip(xs, qs):
        po, so = oracle_quantize(x)
        _bytes_equal(s, so)
        _bytes_equal(p, po)
    assert int(qs[0][1].min()) == 0                      # E = -127 reached
    rp, rs = C._mx8_reduce(torch.stack([q[0] for q in qs]),
                           torch.stack([q[1] for q in qs]))
    op_, os_, _ = oracle_reduce([q[0] for q in qs], [q[1] for q in qs])
    _bytes_equal(rs, os_)
    _bytes_equal(rp, op_)
    y = C._mx8_dequantize(rp, rs, n, torch.float32)
    _bytes_equal(y, oracle_dequantize_groups(op_, os_).reshape(-1)[:n])
    assert bool((y != 0).any())


def test_codec_special_groups(C):
    x = _with_specials(_rand_input(4099, torch.float32, seed=1))
    p, s = C._mx8_quantize(x)
    p = p.view(-1, 32)
    # all-zero group: E = 0, zero payload
    assert int(s[2]) == 127 and int(p[2].max()) == 0
    # exact-zero element encodes as 0x00
    assert int(p[1, 7]) == 0
    # amax = 448 * 2^-3 exactly: E = -3 and the element is e4m3 max (0x7e)
    assert int(s[3]) == 127 - 3 and int(p[3, 5]) == 0x7E
    # one step above 448 * 2^j the exponent moves up
    x2 = x.clone()
    x2[96 + 5] = torch.nextafter(torch.tensor(56.0), torch.tensor(100.0))
    assert int(C._mx8_quantize(x2)[1][3]) == 127 - 2
    # an inf: scale 255, zero payload, NaN for the whole group
    assert int(s[4]) == 255 and int(p[4].max()) == 0
    y = C._mx8_dequantize(p.reshape(-1), s, 4099, torch.float32)
    assert bool(torch.isnan(y[128:160]).all())
    assert bool(torch.isfinite(y[:128]).all())
    assert bool(torch.isfinite(y[160:]).all())
    # a 255 group in any copy poisons the reduced group
    q2 = C._mx8_quantize(_rand_input(4099, torch.float32, seed=2))
    rp, rs = C._mx8_reduce(torch.stack([q2[0], p.reshape(-1)]),
                           torch.stack([q2[1], s]))
    assert int(rs[4]) == 255 and int(rp.view(-1, 32)[4].max()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1e-6, 3e4])
@pytest.mark.parametrize("P", [1, 2, 5, 8])
def test_accuracy_bound(C, P, scale, dtype):
    n = 4099
    xs = [_rand_input(n, dtype, seed=31 * r + P, scale=scale)
          for r in range(P)]
    qs = [C._mx8_quantize(x) for x in xs]
    rp, rs = C._mx8_reduce(torch.stack([q[0] for q in qs]),
                           torch.stack([q[1] for q in qs]))
    out = C._mx8_dequantize(rp, rs, n, dtype)
    exact = sum(x.double() for x in xs)
    bound = allreduce_bound(xs, out)
    ok = torch.isfinite(torch.stack([x.float() for x in xs])).all(dim=0)
    if dtype == torch.float16:
        # fp16 cannot hold 3e4-scaled values: inputs that overflowed to inf
        # must come back as NaN groups, and sums beyond the fp16 range are
        # outside what an output-relative rounding term describes
        bad_groups = ~torch.isfinite(_groups(torch.stack(
            [x.float() for x in xs]).sum(0))).all(dim=1)
        in_bad = bad_groups.repeat_interleave(32)[:n]
        assert bool(torch.isnan(out[in_bad]).all())
        ok = ~in_bad & (exact.abs() + bound < 65504.0)
    err = (out.double() - exact).abs()
    ratio = (err[ok] / bound[ok].clamp(min=1e-300)).max().item()
    print(f"P={P} scale={scale} {dtype}: worst error/bound = {ratio:.3f}")
    # only fp16 may exclude elements, and only once values leave its range
    assert bool(ok.all()) or (dtype == torch.float16 and scale > 1
                              and bool(ok.any()))
    assert bool((err[ok] <= bound[ok]).all()), ratio


# ------------------------------ SPMD worlds -------------------------------

def _cases(world):
    return [
        ("n33", (33,), torch.float32),          # ranks owning zero groups
        ("equal", (32 * world * 3,), torch.float32),   # G % P == 0
        ("n4099_bf16", (4099,), torch.bfloat16),
        ("n4099_f16", (4099,), torch.float16),
        ("n1", (1,), torch.float32),
    ]


def _spmd_input(shape, dtype, rank, tag):
    n = 1
    for d in shape:
        n *= d
    return _rand_input(n, dtype, seed=1000 * tag + rank,
                       scale=(1.0, 1e-6, 3e4)[tag % 3]
                       if dtype != torch.float16 else 1.0).view(shape)


def _same_on_all_ranks(comm, t):
    import mpi4torch_amd as m

    v = t.contiguous().view(torch.uint8).to(torch.int32)
    hi = comm.Allreduce(v, m.MPI_MAX)
    lo = comm.Allreduce(v, m.MPI_MIN)
    return torch.equal(hi, lo)


def _spmd_worker(rank, world):
    import mpi4torch_amd as m

    comm = m.COMM_WORLD
    for tag, (name, shape, dtype) in enumerate(_cases(world)):
        xs = [_spmd_input(shape, dtype, r, tag) for r in range(world)]
        out = comm.AllreduceCompressed(xs[rank], m.MPI_SUM)
        want = oracle_allreduce(xs)
        assert out.dtype == dtype and out.shape == xs[rank].shape, name
        _bytes_equal(out, want)
        assert _same_on_all_ranks(comm, out), name

    # 2-D non-contiguous input
    xs = [_rand_input(12 * 40, torch.float32, seed=50 + r).view(12, 40).t()
          for r in range(world)]
    assert not xs[rank].is_contiguous()
    out = comm.AllreduceCompressed(xs[rank])
    assert out.shape == (40, 12)
    _bytes_equal(out, oracle_allreduce([x.contiguous() for x in xs]))

    # one inf on one rank: that group is NaN everywhere, the rest is finite
    xs = [_rand_input(4099, torch.float32, seed=70 + r) for r in range(world)]
    xs[world - 1][40] = float("inf")
    out = comm.AllreduceCompressed(xs[rank], m.MPI_SUM)
    _bytes_equal(out, oracle_allreduce(xs))
    assert bool(torch.isnan(out[32:64]).all())
    assert bool(torch.isfinite(out[:32]).all())
    assert bool(torch.isfinite(out[64:]).all())

    # backward: x.grad is the compressed allreduce of every rank's w
    ws = [_rand_input(4099, torch.float32, seed=90 + r) for r in range(world)]
    x = _rand_input(4099, torch.float32, seed=80 + rank).requires_grad_()
    y = comm.AllreduceCompressed(x, m.MPI_SUM)
    (y * ws[rank]).sum().backward()
    _bytes_equal(x.grad, oracle_allreduce(ws))

    # the functional wrapper and the tracing passthrough reach the same op
    from mpi4torch_amd import ops
    from mpi4torch_amd.utils import trace

    _bytes_equal(ops.allreduce_compressed(ws[rank]), oracle_allreduce(ws))
    traced = trace(comm)
    _bytes_equal(traced.AllreduceCompressed(ws[rank], m.MPI_SUM),
                 oracle_allreduce(ws))
    assert [r.op for r in traced.trace_records()] == ["AllreduceCompressed"]


@pytest.mark.parametrize("world", [2, 5, 7])
def test_spmd(world):
    run_spmd(world, _spmd_worker)


def _debug_collectives_worker(rank, world):
    """The op goes through the collective-desync detector like Allreduce:
    matching calls pass, a rank with another shape is reported."""
    import os

    import mpi4torch_amd as m

    comm = m.COMM_WORLD
    os.environ["MPI4TORCH_AMD_DEBUG"] = "1"
    m._C.reload_config()
    try:
        x = _rand_input(100, torch.float32, seed=rank)
        assert comm.AllreduceCompressed(x).shape == x.shape
        with pytest.raises(RuntimeError, match="desync"):
            comm.AllreduceCompressed(torch.ones(64 + rank))
    finally:
        os.environ.pop("MPI4TORCH_AMD_DEBUG")
        m._C.reload_config()


def test_spmd_debug_collectives_ws2():
    run_spmd(2, _debug_collectives_worker)


# ---------------------- single-process surface checks ---------------------

def test_error_checks_and_world1():
    import mpi4torch_amd as m

    comm = m.COMM_WORLD
    x = torch.randn(100)
    with pytest.raises(RuntimeError, match="MPI_SUM only"):
        comm.AllreduceCompressed(x, m.MPI_MAX)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.AllreduceCompressed(torch.ones(4, dtype=torch.int32), m.MPI_SUM)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.AllreduceCompressed(
            torch.ones(4).to(torch.float8_e4m3fn), m.MPI_SUM)
    with pytest.raises(RuntimeError, match="float32, bfloat16 and float16"):
        comm.AllreduceCompressed(torch.ones(4, dtype=torch.float64))
    # zero-numel input works
    e = comm.AllreduceCompressed(torch.empty(0, 3), m.MPI_SUM)
    assert e.shape == (0, 3)
    # a world of one compresses nothing: exact clone, op defaults to SUM
    y = comm.AllreduceCompressed(x)
    assert y.data_ptr() != x.data_ptr()
    _bytes_equal(y, x)


def test_scriptable():
    @torch.jit.script
    def fn(comm: m.MPI_Communicator, t: torch.Tensor) -> torch.Tensor:
        return comm.AllreduceCompressed(t, 2) + comm.AllreduceCompressed(t)

    t = torch.randn(40)
    torch.testing.assert_close(fn(m.COMM_WORLD, t), 2 * t, rtol=0, atol=0)


def test_wire_bytes_helper():
    from mpi4torch_amd.utils import mxfp8_wire_bytes

    assert mxfp8_wire_bytes(32) == 33
    assert mxfp8_wire_bytes(33) == 66
    assert mxfp8_wire_bytes(1 << 20) == 33 * (1 << 15)
    import mpi4torch_amd as m

    p, s = m._C._mx8_quantize(torch.randn(4099))
    assert p.numel() + s.numel() == mxfp8_wire_bytes(4099)


# ----------------------------------- DDP ----------------------------------

class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.trunk = torch.nn.Linear(8, 24)
        self.head = torch.nn.Linear(24, 5)
        self.extra = torch.nn.Linear(8, 5)

    def forward(self, x, use_extra=True):
        y = self.head(torch.tanh(self.trunk(x)))
        if use_extra:
            y = y + self.extra(x)
        return y


def _ddp_data(rank):
    g = torch.Generator().manual_seed(300 + rank)
    return torch.randn(6, 8, generator=g)


def _ddp_check(rank, world, find_unused, cap_mb):
    import mpi4torch_amd as m
    from mpi4torch_amd.parallel import DistributedDataParallel

    torch.manual_seed(3)
    base = _Net()
    used = [(r % 2 == 0) or not find_unused for r in range(world)]

    def run(net, r):
        net.zero_grad(set_to_none=True)
        (net(_ddp_data(r), used[r]) ** 2).sum().backward()

    # every rank's local gradients, rebuilt locally from the shared seeds
    names = [n for n, _ in base.named_parameters()]
    local = []
    for r in range(world):
        net = copy.deepcopy(base)
        run(net, r)
        local.append({n: (p.grad.clone() if p.grad is not None else None)
                      for n, p in net.named_parameters()})

    plain_net, comp_net = copy.deepcopy(base), copy.deepcopy(base)
    plain = DistributedDataParallel(plain_net, bucket_cap_mb=cap_mb,
                                    find_unused_parameters=find_unused)
    comp = DistributedDataParallel(comp_net, bucket_cap_mb=cap_mb,
                                   find_unused_parameters=find_unused,
                                   grad_compression="mxfp8")
    for ddp, net in ((plain, plain_net), (comp, comp_net)):
        (ddp(_ddp_data(rank), used[rank]) ** 2).sum().backward()
        ddp.finish_gradient_sync()

    comm = m.COMM_WORLD
    pname = {id(p): n for n, p in comp_net.named_parameters()}
    got = dict(comp_net.named_parameters())
    ref = dict(plain_net.named_parameters())
    for b in comp._buckets:
        bn = [pname[id(q)] for q in b.params
              if any(local[r][pname[id(q)]] is not None
                     for r in range(world))]
        assert bn, "every parameter is used on some rank"
        flats = [torch.cat([
            (local[r][n] if local[r][n] is not None
             else torch.zeros_like(got[n])).reshape(-1) for n in bn])
            for r in range(world)]
        out = torch.cat([got[n].grad.reshape(-1) for n in bn])
        want = torch.cat([ref[n].grad.reshape(-1) for n in bn])
        # bit-identical across ranks
        assert _same_on_all_ranks(comm, out)
        # the compressed gradient IS the oracle's allreduce, averaged
        _bytes_equal(out, oracle_allreduce(flats) * (1.0 / world))
        # within the derived bound (averaged) of the uncompressed DDP
        bound = allreduce_bound(flats, out * world) / world
        err = (out.double() - want.double()).abs()
        assert bool((err <= bound).all()), (bn, (err / bound).max().item())
        assert float(err.max()) > 0.0 or float(want.abs().max()) == 0.0
    assert set(names) == {n for n in got if got[n].grad is not None}


def _ddp_worker(rank, world):
    _ddp_check(rank, world, find_unused=False, cap_mb=1)   # one big bucket
    _ddp_check(rank, world, find_unused=False, cap_mb=0)   # bucket per param
    _ddp_check(rank, world, find_unused=True, cap_mb=0)
    _ddp_check(rank, world, find_unused=True, cap_mb=1)


@pytest.mark.parametrize("world", [2, 3])
def test_ddp_grad_compression(world):
    run_spmd(world, _ddp_worker)


def _ddp_no_sync_worker(rank, world):
    from mpi4torch_amd.parallel import DistributedDataParallel

    torch.manual_seed(3)
    net = _Net()
    ddp = DistributedDataParallel(net, grad_compression="mxfp8")
    # a backward entirely under no_sync fires nothing: finish is a no-op,
    # as it is without compression, and gradients stay local
    with ddp.no_sync():
        (ddp(_ddp_data(rank)) ** 2).sum().backward()
    local = net.trunk.weight.grad.clone()
    ddp.finish_gradient_sync()
    _bytes_equal(net.trunk.weight.grad, local)
    # the next synchronized backward reduces the accumulated gradients
    (ddp(_ddp_data(rank)) ** 2).sum().backward()
    ddp.finish_gradient_sync()
    assert _same_on_all_ranks(m.COMM_WORLD, net.trunk.weight.grad)


def test_ddp_grad_compression_no_sync_ws2():
    run_spmd(2, _ddp_no_sync_worker)


def test_ddp_bad_arguments():
    from mpi4torch_amd.parallel import DistributedDataParallel

    with pytest.raises(ValueError, match="grad_compression"):
        DistributedDataParallel(_Net(), grad_compression="fp4")
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        DistributedDataParallel(_Net().double(), grad_compression="mxfp8")
    ddp = DistributedDataParallel(_Net(), grad_compression="mxfp8")
    assert ddp.grad_compression == "mxfp8"
    assert DistributedDataParallel(_Net()).grad_compression is None
