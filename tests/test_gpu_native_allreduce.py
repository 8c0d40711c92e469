"""GPU tests of the arith_reduce kernel and of native_allreduce at world 1.

Kernel numerics are checked bit for bit against a torch reference with the
kernel's contract: sources combined in rank order, fp32 accumulation, one
round-to-nearest-even cast. MIN/MAX follow fminf/fmaxf; inputs with NaN are
in test_gpu_kernel_edges.py. The P = 1 instance is a raw bit copy and is
fed arbitrary bit patterns (NaN payloads, infinities, -0.0, subnormals).
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
SIZES = (1, 7, 8, 4097, (1 << 16) + 3)


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


def _bits(t):
    return t.contiguous().view(
        {1: torch.uint8, 2: torch.int16, 4: torch.int32,
         8: torch.int64}[t.element_size()])


def _ops(m):
    return (("sum", m.MPI_SUM), ("prod", m.MPI_PROD), ("min", m.MPI_MIN),
            ("max", m.MPI_MAX))


def _sources(nranks, n, dtype, opname, gen):
    x = torch.randn(nranks, n, device="cuda", generator=gen)
    if opname == "prod":
        x = 1.0 + 0.25 * x  # keep the product in range
    else:
        x = x * torch.arange(1, nranks + 1, device="cuda").unsqueeze(1)
    return x.to(dtype)


def _reference(src, opname):
    acc = src[0].float()
    for r in range(1, src.shape[0]):
        v = src[r].float()
        if opname == "sum":
            acc = acc + v
        elif opname == "prod":
            acc = acc * v
        elif opname == "min":
            acc = torch.minimum(acc, v)
        else:
            acc = torch.maximum(acc, v)
    return acc.to(src.dtype)


def _split(src, me, layout):
    """own = source `me`, staged = the others in rank order. 'packed' rows
    are n apart (vector path only when n fills whole vectors); 'slotted'
    rows start on 16-byte boundaries as native_allreduce lays them out
    (vector body + element tail); 'odd' puts own at an odd element offset
    of a larger buffer (general path)."""
    nranks, n = src.shape
    rest = torch.cat([src[:me], src[me + 1:]])
    per_vec = 16 // src.element_size()
    if layout == "slotted":
        slot = (n + per_vec - 1) // per_vec * per_vec
        buf = torch.zeros(max(nranks - 1, 1), slot, dtype=src.dtype,
                          device="cuda")
        staged = buf[:nranks - 1, :n]
        staged.copy_(rest)
    else:
        staged = rest.contiguous()
    if layout == "odd":
        big = torch.zeros(n + 5, dtype=src.dtype, device="cuda")
        own = big[3:3 + n]
        own.copy_(src[me])
    else:
        own = src[me].clone()
    return own, staged


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16", "fp32"))
def test_arith_reduce_kernel(world1, dtype):
    m = world1
    gen = torch.Generator(device="cuda").manual_seed(77)
    for nranks in (1, 2, 5, 8):
        for n in SIZES:
            for opname, op in _ops(m):
                src = _sources(nranks, n, dtype, opname, gen)
                want = _bits(_reference(src, opname))
                for me in sorted({0, nranks - 1}):
                    for layout in ("packed", "slotted"):
                        own, staged = _split(src, me, layout)
                        got = m._C._arith_reduce(own, staged, me, op)
                        assert got.dtype == dtype and got.shape == (n,)
                        assert torch.equal(_bits(got), want), (
                            nranks, n, opname, me, layout)
    # own block at an odd element offset of a larger buffer
    for nranks in (1, 5):
        for n in (7, 4097):
            for opname, op in _ops(m):
                src = _sources(nranks, n, dtype, opname, gen)
                own, staged = _split(src, nranks - 1, "odd")
                assert own.data_ptr() % 16 != 0
                got = m._C._arith_reduce(own, staged, nranks - 1, op)
                assert torch.equal(_bits(got), _bits(_reference(src, opname)))


class _forced:
    """force_full_path with a chosen MPI4TORCH_AMD_ALLREDUCE engine."""

    def __init__(self, m, engine=None):
        self.m, self.engine = m, engine

    def __enter__(self):
        if self.engine is not None:
            os.environ["MPI4TORCH_AMD_ALLREDUCE"] = self.engine
        self.m._C.reload_config()
        self.m._C.force_full_path(True)

    def __exit__(self, *exc):
        os.environ.pop("MPI4TORCH_AMD_ALLREDUCE", None)
        self.m._C.reload_config()
        self.m._C.force_full_path(False)


def _random_bits(n, dtype, gen):
    es = torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(0, 256, (n * es,), dtype=torch.uint8, device="cuda",
                        generator=gen)
    return raw.view(dtype)


def test_p1_bit_copy(world1):
    m = world1
    comm = m.COMM_WORLD
    gen = torch.Generator(device="cuda").manual_seed(5)
    with _forced(m):
        for dtype in (torch.bfloat16, torch.float32, torch.int32,
                      torch.float64):
            for n in (1 << 16, (1 << 16) + 3):
                x = _random_bits(n, dtype, gen)
                if dtype == torch.bfloat16:
                    # the pattern set really holds the awkward values
                    b = _bits(x).int() & 0xFFFF
                    assert ((b & 0x7F80) == 0x7F80).any()  # inf / NaN
                    assert ((b & 0x7F80) == 0).any()       # zero / subnormal
                y = comm.Allreduce(x, m.MPI_SUM)
                assert y.data_ptr() != x.data_ptr()
                assert torch.equal(_bits(y), _bits(x)), (dtype, n)
        # -0.0 explicitly
        z = torch.full((9,), -0.0, device="cuda", dtype=torch.bfloat16)
        assert (_bits(comm.Allreduce(z, m.MPI_SUM)) == -32768).all()


def _fwd_bwd(m, dtype, seed):
    comm = m.COMM_WORLD
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((1 << 16) + 3, device="cuda",
                    generator=gen).to(dtype).requires_grad_()
    g = torch.randn((1 << 16) + 3, device="cuda", generator=gen).to(dtype)
    y = comm.Allreduce(x, m.MPI_SUM)
    y.backward(g)
    torch.cuda.synchronize()
    return x.detach(), g, y.detach(), x.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16", "fp32"))
def test_forced_fwd_bwd_and_rccl_knob(world1, dtype):
    m = world1
    with _forced(m):
        x, g, y, gx = _fwd_bwd(m, dtype, 11)
    assert y.dtype == dtype and gx.dtype == dtype
    # world of one: forward is the input, backward is the gradient
    assert torch.equal(_bits(y), _bits(x))
    assert torch.equal(_bits(gx), _bits(g))
    with _forced(m, "rccl"):
        _, _, y_r, gx_r = _fwd_bwd(m, dtype, 11)
    assert torch.equal(_bits(y_r), _bits(y))
    assert torch.equal(_bits(gx_r), _bits(gx))


def test_forced_allreduce_graph_capture(world1):
    m = world1
    comm = m.COMM_WORLD
    with _forced(m):
        static_in = torch.rand((1 << 18) + 3, device="cuda").to(torch.bfloat16)
        x0 = static_in.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                comm.Allreduce(static_in, m.MPI_SUM)
        torch.cuda.current_stream().wait_stream(s)

        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_out = comm.Allreduce(static_in, m.MPI_SUM)
        for i in range(3):
            static_in.copy_(x0 * (i + 1))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(static_out), _bits(static_in))
