#!/usr/bin/env python3
"""CDNA4 kernel micro-benchmarks (1 GPU): effective HBM bandwidth of the
local-reduce and marshaling kernels vs the ~8 TB/s HBM3E peak.

Each kernel moves (nranks*N reads + N writes) or (N reads + N writes) —
reported GB/s counts actual bytes touched. Run on an MI355X box:
    python tools/kernel_microbench.py            # everything
    python tools/kernel_microbench.py --mx8      # only the mxfp8 codec section
    python tools/kernel_microbench.py --mx8-reduce-to   # only that part
    python tools/kernel_microbench.py --mx8-dequantize-blocks   # only that part
    python tools/kernel_microbench.py --mx8-quantize-blocks     # only that part
    python tools/kernel_microbench.py --mx8-segments            # only that part

The mxfp8 section times the three codec kernels and, in the same run and
alternating with it, the sibling fp8_reduce kernel at the same P and n, so
the ratio between the two is not a comparison across runs. Its last part
times the fused reduce-scatter tail mx8_reduce_to against the two-kernel
sequence it replaces (mx8_reduce then mx8_dequantize), again alternating.
The dequantize-blocks part does the same for the fused allgather tail
mx8_dequantize_blocks against P x mx8_dequantize into staging plus the slab
unpack that Allgather uses. The quantize-blocks part does the same for the
fused all-to-all head mx8_quantize_blocks against the axis pack into staging
plus mx8_quantize. The segments part does the same for the pairwise
all-to-all head and tail with a fused token permute, mx8_quantize_segments
and mx8_dequantize_segments, against index_select plus the flat codec kernel.
"""

import os
import sys

os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29581")
os.environ.setdefault("RANK", "0")
os.environ.setdefault("WORLD_SIZE", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

dist.init_process_group("gloo", rank=0, world_size=1)
import mpi4torch_amd as m

m.init()
assert torch.cuda.is_available()


def timeit(fn, iters=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def report(name, ms, nbytes):
    print(f"{name:34s} {ms*1e3:9.1f} us  {nbytes/ms/1e6:8.1f} GB/s", flush=True)


P = 8
N = 64 << 20  # 64M elements per chunk


def mx8_section(repeats=5):
    """mxfp8 codec kernels. Bytes are what each kernel actually moves:
    quantize N*esize in + 33N/32 out, reduce P*33n/32 in + 33n/32 out,
    dequantize the mirror of quantize. Every launch's working set is larger
    than the 256 MiB Infinity Cache (the same buffers are reused across
    iterations): quantize/dequantize run at 256Mi elements (>= 776 MiB per
    launch), the reduce at P x 64 MiB of payload (594 MiB)."""
    C = m._C
    NQ = 256 << 20
    med = lambda v: sorted(v)[len(v) // 2]

    def line(name, times, nbytes):
        t = med(times)
        print(f"{name:34s} {t*1e3:9.1f} us  {nbytes/t/1e6:8.1f} GB/s  "
              f"(min {min(times)*1e3:.1f} max {max(times)*1e3:.1f} us, "
              f"{len(times)} repeats)", flush=True)
        return t

    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16"),
                       (torch.float16, "fp16")):
        x = torch.randn(NQ, device="cuda")
        x.view(-1, 32).mul_(torch.rand(NQ // 32, 1, device="cuda"))
        x = x.to(dtype)
        es = x.element_size()
        wire = 33 * NQ // 32
        tq = [timeit(lambda: C._mx8_quantize(x)) for _ in range(repeats)]
        line(f"mx8_quantize {tag} N={NQ>>20}Mi", tq, NQ * es + wire)
        pay, sc = C._mx8_quantize(x)
        td = [timeit(lambda: C._mx8_dequantize(pay, sc, NQ, dtype))
              for _ in range(repeats)]
        line(f"mx8_dequantize {tag} N={NQ>>20}Mi", td, NQ * es + wire)
        del x, pay, sc

    # reduce vs its sibling, alternating, same P and n
    wire = 33 * N // 32
    src = torch.randn(P, N, device="cuda") * 0.2
    stk8 = src.to(torch.float8_e4m3fn)
    qs = [C._mx8_quantize(src[r]) for r in range(P)]
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    del src, qs
    t_new, t_sib = [], []
    for _ in range(repeats):
        t_sib.append(timeit(lambda: C._fp8_reduce(stk8, 0)))
        t_new.append(timeit(lambda: C._mx8_reduce(pay, sc)))
    a = line(f"fp8_reduce (sibling) P={P} n={N>>25}Mi grp", t_sib,
             (P + 1) * N)
    b = line(f"mx8_reduce P={P} n={N>>25}Mi groups", t_new, (P + 1) * wire)
    spread = (max(t_sib) - min(t_sib)) / med(t_sib)
    print(f"mx8_reduce / fp8_reduce time ratio {b/a:.3f} "
          f"(sibling spread {spread*100:.1f}% of its median; the mx8 kernel "
          f"moves 33/32 = 1.031x the bytes)", flush=True)

    # informational: codec overhead of the full pipeline at world size 1
    # (no wire at this size: self-exchange + three kernels + allgather)
    t = torch.randn(128 << 20, device="cuda").to(torch.bfloat16)  # 256 MiB
    comm = m.COMM_WORLD
    C.force_full_path(True)
    try:
        tc = [timeit(lambda: comm.AllreduceCompressed(t, m.MPI_SUM), iters=10)
              for _ in range(3)]
        ta = [timeit(lambda: comm.Allreduce(t, m.MPI_SUM), iters=10)
              for _ in range(3)]
    finally:
        C.force_full_path(False)
    line("w1 full-path AllreduceCompressed", tc, t.numel() * 2)
    line("w1 full-path Allreduce", ta, t.numel() * 2)


def mx8_reduce_to_section(repeats=5):
    """mx8_reduce_to per output dtype at the reduce's shape (P = 8 copies of
    n = 2Mi groups) against mx8_reduce + mx8_dequantize of the same block,
    alternating in the same run. Bytes of the fused kernel: P*33n/32 in +
    n*32*esize out (>= 656 MiB per launch, past the Infinity Cache); the
    pair moves 33n/32 more out and in again."""
    C = m._C
    med = lambda v: sorted(v)[len(v) // 2]
    n = N // 32
    src = torch.randn(P, N, device="cuda") * 0.2
    src.view(P, n, 32).mul_(torch.rand(P, n, 1, device="cuda"))
    qs = [C._mx8_quantize(src[r]) for r in range(P)]
    pay = torch.stack([q[0] for q in qs])
    sc = torch.stack([q[1] for q in qs])
    del src, qs

    def line(name, times, nbytes):
        t = med(times)
        print(f"{name:34s} {t*1e3:9.1f} us  {nbytes/t/1e6:8.1f} GB/s  "
              f"(min {min(times)*1e3:.1f} max {max(times)*1e3:.1f} us, "
              f"{len(times)} repeats)", flush=True)
        return t

    def pair(dtype):
        rp, rs = C._mx8_reduce(pay, sc)
        return C._mx8_dequantize(rp, rs, N, dtype)

    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16"),
                       (torch.float16, "fp16")):
        es = torch.empty(0, dtype=dtype).element_size()
        t_pair, t_fused = [], []
        for _ in range(repeats):
            t_pair.append(timeit(lambda: pair(dtype)))
            t_fused.append(timeit(lambda: C._mx8_reduce_to(pay, sc, N, dtype)))
        fused_b = P * 33 * n + n * 32 * es
        a = line(f"mx8_reduce+dequantize {tag} P={P}", t_pair,
                 fused_b + 2 * 33 * n)
        b = line(f"mx8_reduce_to {tag} P={P} n={n>>20}Mi grp", t_fused,
                 fused_b)
        spread = (max(t_pair) - min(t_pair)) / med(t_pair)
        print(f"mx8_reduce_to / pair time ratio {tag} {b/a:.3f} "
              f"(pair spread {spread*100:.1f}% of its median)", flush=True)


def mx8_dequantize_blocks_section(repeats=5):
    """mx8_dequantize_blocks per output dtype at P = 8 blocks against the
    sequence it replaces, alternating in the same run, for three geometries:
      (a) rows = 1, L % 32 == 0: one flat stream; against ONE mx8_dequantize
          over the same bytes (the fused launcher dispatches to that kernel);
      (b) rows = 8, row_elems*esize % 16 == 0, row_elems % 32 != 0 (groups
          straddle the rows, vector path); against P x mx8_dequantize into
          staging and the axis unpack of Allgather (_unpack_blocks: one
          move_axis_blocks call, one slab-copy launch);
      (c) rows = 1, odd L (scalar twin); against P x mx8_dequantize written
          straight to each block's place (one row needs no unpack; blocks
          1..P-1 start off 16 bytes and take that kernel's scalar twin).
    Every block holds ~32Mi elements, so one launch reads 264 MiB and writes
    512 MiB (16-bit) or 1 GiB (fp32), past the 256 MiB Infinity Cache. Bytes
    of the fused kernel: P*33*ceil(L/32) in + P*L*esize out; the sequence of
    (b) writes and reads P*L*esize once more."""
    C = m._C
    med = lambda v: sorted(v)[len(v) // 2]

    def line(name, times, nbytes):
        t = med(times)
        print(f"{name:40s} {t*1e3:9.1f} us  {nbytes/t/1e6:8.1f} GB/s  "
              f"(min {min(times)*1e3:.1f} max {max(times)*1e3:.1f} us, "
              f"{len(times)} repeats)", flush=True)
        return t

    def quantized(L):
        Gb = (L + 31) // 32
        pay = torch.empty(P, Gb * 32, dtype=torch.uint8, device="cuda")
        sc = torch.empty(P, Gb, dtype=torch.uint8, device="cuda")
        for r in range(P):
            x = torch.randn(L, device="cuda") * 0.2
            x.mul_(torch.rand(L, device="cuda"))
            q = C._mx8_quantize(x)
            pay[r].copy_(q[0])
            sc[r].copy_(q[1])
            del x, q
        return pay, sc

    base = 32 << 20
    geoms = (("a", 1, base), ("b", 8, base // 8 + 8), ("c", 1, base + 1))
    for tag_g, rows, row_elems in geoms:
        L = rows * row_elems
        Gb = (L + 31) // 32
        pay, sc = quantized(L)
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16"),
                           (torch.float16, "fp16")):
            es = torch.empty(0, dtype=dtype).element_size()
            out = torch.empty(P * L, dtype=dtype, device="cuda")
            fused = lambda: C._mx8_dequantize_blocks(pay, sc, rows, row_elems,
                                                     dtype, out=out)
            fused_b = P * 33 * Gb + P * L * es
            if tag_g == "a":
                pf, sf = pay.view(-1), sc.view(-1)
                seq = lambda: C._mx8_dequantize(pf, sf, P * L, dtype, out=out)
                seq_b, seq_name = fused_b, "1 x mx8_dequantize"
            elif tag_g == "b":
                stage = torch.empty(P * L, dtype=dtype, device="cuda")
                parts = [stage[r * L:(r + 1) * L] for r in range(P)]
                out3 = out.view(rows, P, row_elems)

                def seq():
                    for r in range(P):
                        C._mx8_dequantize(pay[r], sc[r], L, dtype,
                                          out=parts[r])
                    C._unpack_blocks(stage, out3)

                seq_b = fused_b + 2 * P * L * es
                seq_name = f"{P} x mx8_dequantize + unpack"
            else:
                parts = [out[r * L:(r + 1) * L] for r in range(P)]

                def seq():
                    for r in range(P):
                        C._mx8_dequantize(pay[r], sc[r], L, dtype,
                                          out=parts[r])

                seq_b, seq_name = fused_b, f"{P} x mx8_dequantize in place"
            t_seq, t_fused = [], []
            for _ in range(repeats):
                t_seq.append(timeit(seq))
                t_fused.append(timeit(fused))
            a = line(f"({tag_g}) {seq_name} {tag}", t_seq, seq_b)
            b = line(f"({tag_g}) mx8_dequantize_blocks {tag} "
                     f"{rows}x{row_elems}", t_fused, fused_b)
            spread = (max(t_seq) - min(t_seq)) / med(t_seq)
            print(f"({tag_g}) fused / sequence time ratio {tag} {b/a:.3f} "
                  f"(sequence min-max spread {spread*100:.1f}% of its "
                  f"median)", flush=True)
            del out
            if tag_g == "b":
                del stage, parts, out3
        del pay, sc

    # informational: codec overhead of the full pipeline at world size 1 (no
    # wire at this size: quantize + 1-rank allgather + fused tail)
    t = torch.randn(128 << 20, device="cuda").to(torch.bfloat16)  # 256 MiB
    comm = m.COMM_WORLD
    C.force_full_path(True)
    try:
        tc = [timeit(lambda: comm.AllgatherCompressed(t, 0), iters=10)
              for _ in range(3)]
        ta = [timeit(lambda: comm.Allgather(t, 0), iters=10)
              for _ in range(3)]
    finally:
        C.force_full_path(False)
    line("w1 full-path AllgatherCompressed", tc, t.numel() * 2)
    line("w1 full-path Allgather", ta, t.numel() * 2)


def mx8_quantize_blocks_section(repeats=5):
    """mx8_quantize_blocks per input dtype at P = 8 blocks against the
    sequence it replaces, alternating in the same run, for four geometries:
      (a)  rows = 1, L % 32 == 0: the input is one flat stream; against ONE
           mx8_quantize over the same bytes (the fused launcher dispatches
           to that kernel);
      (b)  rows = 8, row_elems = 4Mi+8 (groups straddle the rows, vector
           path); against the rank-major axis pack that ReducescatterCompressed
           uses (_pack_blocks: one move_axis_blocks call, one slab-copy
           launch) and ONE flat mx8_quantize of the staging (L % 32 == 0);
      (b') rows = 32768, row_elems = 1024: the Ulysses shape with short
           rows; against the same sequence;
      (c)  rows = 1, odd L (general twin); against P x mx8_quantize of the
           blocks in place (blocks 1..P-1 start off 16 bytes and take that
           kernel's scalar twin).
    Every block holds ~32Mi elements, so one launch reads 512 MiB (16-bit)
    or 1 GiB (fp32) and writes 264 MiB, past the 256 MiB Infinity Cache.
    Bytes of the fused kernel: P*L*esize in + P*33*ceil(L/32) out; the
    sequence of (b)/(b') writes and reads P*L*esize once more."""
    C = m._C
    med = lambda v: sorted(v)[len(v) // 2]

    def line(name, times, nbytes):
        t = med(times)
        print(f"{name:40s} {t*1e3:9.1f} us  {nbytes/t/1e6:8.1f} GB/s  "
              f"(min {min(times)*1e3:.1f} max {max(times)*1e3:.1f} us, "
              f"{len(times)} repeats)", flush=True)
        return t

    base = 32 << 20
    geoms = (("a", 1, base), ("b", 8, base // 8 + 8),
             ("b'", 32768, 1024), ("c", 1, base + 1))
    for tag_g, rows, row_elems in geoms:
        L = rows * row_elems
        Gb = (L + 31) // 32
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16"),
                           (torch.float16, "fp16")):
            x = torch.randn(P * L, device="cuda") * 0.2
            x.mul_(torch.rand(P * L, device="cuda"))
            x = x.to(dtype)
            es = x.element_size()
            fused = lambda: C._mx8_quantize_blocks(x, P, rows, row_elems)
            fused_b = P * L * es + P * 33 * Gb
            if tag_g == "a":
                seq = lambda: C._mx8_quantize(x)
                seq_b, seq_name = fused_b, "1 x mx8_quantize"
            elif tag_g in ("b", "b'"):
                stage = torch.empty(P * L, dtype=dtype, device="cuda")
                x3 = x.view(rows, P, row_elems)

                def seq():
                    C._pack_blocks(x3, stage)
                    return C._mx8_quantize(stage)

                seq_b = fused_b + 2 * P * L * es
                seq_name = "pack + 1 x mx8_quantize"
            else:
                parts = [x[r * L:(r + 1) * L] for r in range(P)]

                def seq():
                    for r in range(P):
                        C._mx8_quantize(parts[r])

                seq_b, seq_name = fused_b, f"{P} x mx8_quantize in place"
            t_seq, t_fused = [], []
            for _ in range(repeats):
                t_seq.append(timeit(seq))
                t_fused.append(timeit(fused))
            a = line(f"({tag_g}) {seq_name} {tag}", t_seq, seq_b)
            b = line(f"({tag_g}) mx8_quantize_blocks {tag} "
                     f"{rows}x{row_elems}", t_fused, fused_b)
            spread = (max(t_seq) - min(t_seq)) / med(t_seq)
            print(f"({tag_g}) fused / sequence time ratio {tag} {b/a:.3f} "
                  f"(sequence min-max spread {spread*100:.1f}% of its "
                  f"median; fused min-max {min(t_fused)*1e3:.1f}-"
                  f"{max(t_fused)*1e3:.1f} us)", flush=True)
            if tag_g in ("b", "b'"):
                del stage, x3
            del x

    # informational: codec and staging overhead of the full pipeline at
    # world size 1 (no wire at this size: fused head + self-exchange + fused
    # tail) on the Ulysses-like [rows, heads*dim] reshard of 256 MiB bf16
    t = torch.randn(32768, 4096, device="cuda").to(torch.bfloat16)
    comm = m.COMM_WORLD
    C.force_full_path(True)
    try:
        tc = [timeit(lambda: comm.AlltoallCompressed(t, 0, 1), iters=10)
              for _ in range(3)]
        ta = [timeit(lambda: comm.Alltoall(t, 0, 1, t.size(1)), iters=10)
              for _ in range(3)]
    finally:
        C.force_full_path(False)
    line("w1 full-path AlltoallCompressed", tc, t.numel() * 2)
    line("w1 full-path Alltoall", ta, t.numel() * 2)


def mx8_segments_section(repeats=5):
    """mx8_quantize_segments / mx8_dequantize_segments at the MoE token
    geometry, 128Ki tokens x 4096, P = 8 segments of uneven counts (one of
    them zero), bf16 and fp32, against the sequences they replace,
    alternating in the same run:
      send  index_select(0, order) + ONE flat mx8_quantize   vs the fused
            head reading tokens through the index;
      recv  ONE flat mx8_dequantize + index_select(0, inverse)   vs the
            fused tail writing tokens through the index;
      flat  the no-index segments launchers vs the flat kernels (every L_p
            is a multiple of 32 here, so they dispatch to those kernels).
    A row is 4096 elements, so every segment is a whole number of groups and
    the sequence's bytes are byte for byte the fused kernels'. One launch
    touches 1 GiB (bf16) or 2 GiB (fp32) of tokens plus 528 MiB of codec
    bytes, past the 256 MiB Infinity Cache. Bytes of a fused kernel:
    N*D*esize + 33*N*D/32 (+ 8N of index); the sequence moves N*D*esize
    twice more."""
    C = m._C
    med = lambda v: sorted(v)[len(v) // 2]

    def line(name, times, nbytes):
        t = med(times)
        print(f"{name:44s} {t*1e3:9.1f} us  {nbytes/t/1e9:6.2f} TB/s  "
              f"(min {min(times)*1e3:.1f} max {max(times)*1e3:.1f} us, "
              f"{len(times)} repeats)", flush=True)
        return t

    def versus(tag, seq_name, seq, seq_b, fused_name, fused, fused_b,
               same_kernel=False):
        t_seq, t_fused = [], []
        for _ in range(repeats):
            t_seq.append(timeit(seq))
            t_fused.append(timeit(fused))
        a = line(f"({tag}) {seq_name}", t_seq, seq_b)
        b = line(f"({tag}) {fused_name}", t_fused, fused_b)
        spread = (max(t_seq) - min(t_seq)) / med(t_seq)
        if same_kernel:
            inside = min(t_seq) <= b <= max(t_seq)
            verdict = ("inside the sequence min-max" if inside
                       else "OUTSIDE the sequence min-max")
        else:
            verdict = ("below the sequence minimum" if b < min(t_seq)
                       else "NOT below the sequence minimum")
        print(f"({tag}) fused / sequence time ratio {b/a:.3f} (sequence "
              f"min-max spread {spread*100:.1f}% of its median; fused median "
              f"{verdict}; fused min-max "
              f"{min(t_fused)*1e3:.1f}-{max(t_fused)*1e3:.1f} us)",
              flush=True)

    N, D = 128 << 10, 4096
    counts = [20000, 0, 12000, 24000, 8000, 30000, 17072, 20000]
    assert sum(counts) == N and len(counts) == P
    gen = torch.Generator(device="cuda").manual_seed(7)
    order = torch.randperm(N, device="cuda", generator=gen)
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(N, device="cuda")
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        x = torch.randn(N, D, device="cuda") * 0.2
        x.mul_(torch.rand(N, 1, device="cuda"))
        x = x.to(dtype)
        es = x.element_size()
        flat = x.view(-1)
        codec_b = 33 * (N * D // 32)
        fused_b = N * D * es + codec_b
        pay, sc = C._mx8_quantize(flat)

        versus(f"send {tag}", "index_select + 1 x mx8_quantize",
               lambda: C._mx8_quantize(x.index_select(0, order).view(-1)),
               fused_b + 2 * N * D * es,
               "mx8_quantize_segments, indexed",
               lambda: C._mx8_quantize_segments(flat, 1, D, counts,
                                                order=order),
               fused_b + 8 * N)
        versus(f"recv {tag}", "1 x mx8_dequantize + index_select",
               lambda: C._mx8_dequantize(pay, sc, N * D, dtype)
               .view(N, D).index_select(0, inverse),
               fused_b + 2 * N * D * es,
               "mx8_dequantize_segments, indexed",
               lambda: C._mx8_dequantize_segments(pay, sc, 1, D, counts,
                                                  dtype, order=order),
               fused_b + 8 * N)
        versus(f"flat-q {tag}", "1 x mx8_quantize",
               lambda: C._mx8_quantize(flat), fused_b,
               "mx8_quantize_segments, no index",
               lambda: C._mx8_quantize_segments(flat, 1, D, counts), fused_b,
               same_kernel=True)
        versus(f"flat-d {tag}", "1 x mx8_dequantize",
               lambda: C._mx8_dequantize(pay, sc, N * D, dtype), fused_b,
               "mx8_dequantize_segments, no index",
               lambda: C._mx8_dequantize_segments(pay, sc, 1, D, counts,
                                                  dtype), fused_b,
               same_kernel=True)
        del x, flat, pay, sc

    # informational: codec overhead at world size 1 (no wire at this size).
    comm = m.COMM_WORLD
    t = torch.randn(32768, 4096, device="cuda").to(torch.bfloat16)
    cnt = [t.size(0)]
    C.force_full_path(True)
    try:
        tc = [timeit(lambda: comm.AlltoallPairwiseCompressed(t, 0, cnt, cnt),
                     iters=10) for _ in range(3)]
        ta = [timeit(lambda: comm.AlltoallPairwise(t, 0, cnt, cnt), iters=10)
              for _ in range(3)]
        line("w1 full-path AlltoallPairwiseCompressed", tc, t.numel() * 2)
        line("w1 full-path AlltoallPairwise", ta, t.numel() * 2)
        del t
        from mpi4torch_amd.models.moe import ExpertParallelMoE

        tok = torch.randn(16384, 1024, device="cuda").to(torch.bfloat16)
        for comp in (None, "mxfp8"):
            torch.manual_seed(3)
            layer = ExpertParallelMoE(1024, 8, compression=comp)
            layer = layer.to(device="cuda", dtype=torch.bfloat16)

            def step():
                layer.zero_grad(set_to_none=True)
                layer(tok).float().pow(2).sum().backward()

            ts = [timeit(step, iters=5, warmup=2) for _ in range(3)]
            line(f"w1 full-path MoE fwd+bwd compression={comp}", ts,
                 tok.numel() * 2)
    finally:
        C.force_full_path(False)


if "--mx8-segments" in sys.argv:
    mx8_segments_section()
    dist.destroy_process_group()
    sys.exit(0)

if "--mx8-quantize-blocks" in sys.argv:
    mx8_quantize_blocks_section()
    dist.destroy_process_group()
    sys.exit(0)

if "--mx8-reduce-to" in sys.argv:
    mx8_reduce_to_section()
    dist.destroy_process_group()
    sys.exit(0)

if "--mx8-dequantize-blocks" in sys.argv:
    mx8_dequantize_blocks_section()
    dist.destroy_process_group()
    sys.exit(0)

if "--mx8" in sys.argv:
    mx8_section()
    mx8_reduce_to_section()
    mx8_dequantize_blocks_section()
    mx8_quantize_blocks_section()
    mx8_segments_section()
    dist.destroy_process_group()
    sys.exit(0)

# fp8 local reduce: P chunks fp8 -> 1 chunk fp8, fp32 accumulation
stk8 = (torch.randn(P, N, device="cuda") * 0.2).to(torch.float8_e4m3fn)
ms = timeit(lambda: m._C._fp8_reduce(stk8, 0))
report(f"fp8_reduce  P={P} N={N>>20}Mi", ms, (P + 1) * N)

# bitwise reduce: int32
stki = torch.randint(0, 1 << 30, (P, N // 4), device="cuda",
                     dtype=torch.int32)
ms = timeit(lambda: m._C._bitwise_reduce(stki, 2))
report(f"bitwise_reduce int32 P={P}", ms, (P + 1) * N)

# pairloc reduce: fp32 pairs
npairs = N // 8
stkp = torch.stack([torch.randn(P, npairs, device="cuda"),
                    torch.randint(0, 99, (P, npairs), device="cuda").float()],
                   dim=-1)
ms = timeit(lambda: m._C._pairloc_reduce(stkp, 0))
report(f"pairloc_reduce fp32 P={P}", ms, (P + 1) * npairs * 8)

# slab pack/unpack roundtrip via debug entry (counts partition the axis):
# before=4096 rows, axis=4096, after=16 fp32 -> 1 GiB tensor, 8 blocks
x = torch.randn(4096, 4096, 16, device="cuda")
counts = [512] * 8
ms = timeit(lambda: m._C._pack_roundtrip(x, 1, counts), iters=10)
report("slab pack+unpack 4 GiB moved", ms, 4 * x.numel() * 4)

# contiguous fast_clone path (nontemporal streaming copy) via Allreduce w1
t = torch.randn(N, device="cuda")
comm = m.COMM_WORLD
ms = timeit(lambda: comm.Allreduce(t, m.MPI_SUM))
report("w1 fast-path clone 64Mi fp32", ms, 2 * N * 4)
del stk8, stki, stkp, x, t

# arith_reduce, the local tail of native_allreduce. nranks=1 is the bit copy
# the N=1 flagship times (1 GiB bf16), alternated with the slab copy
# (fast_clone) at the same size; 8 x 128 MiB bf16 is the P=8 reduce.
g1 = torch.randn(512 << 20, device="cuda", dtype=torch.bfloat16)  # 1 GiB
none = g1.new_empty((0, g1.numel()))
t_red, t_slab = [], []
for _ in range(5):
    t_red.append(timeit(lambda: m._C._arith_reduce(g1, none, 0, m.MPI_SUM)))
    t_slab.append(timeit(lambda: comm.Allreduce(g1, m.MPI_SUM)))
med = lambda v: sorted(v)[len(v) // 2]
for name, ts in (("arith_reduce bf16 nranks=1 1GiB", t_red),
                 ("slab copy (fast_clone) bf16 1GiB", t_slab)):
    print(f"{name:34s} {med(ts)*1e3:9.1f} us  "
          f"{2 * g1.numel() * 2 / med(ts) / 1e6:8.1f} GB/s  "
          f"(min {min(ts)*1e3:.1f} max {max(ts)*1e3:.1f} us, 5 repeats)",
          flush=True)
del g1, none
nb = 64 << 20  # 128 MiB of bf16 per rank
own = torch.randn(nb, device="cuda", dtype=torch.bfloat16)
stg = torch.randn(P - 1, nb, device="cuda", dtype=torch.bfloat16)
ms = timeit(lambda: m._C._arith_reduce(own, stg, 0, m.MPI_SUM))
report(f"arith_reduce bf16 P={P} 128MiB", ms, (P + 1) * nb * 2)
del own, stg

mx8_section()
mx8_reduce_to_section()
mx8_dequantize_blocks_section()
mx8_quantize_blocks_section()
mx8_segments_section()

dist.destroy_process_group()
