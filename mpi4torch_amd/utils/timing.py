"""hipEvent-based collective timing + bandwidth math.

The reference has no tracing/profiling subsystem; on MI355X
per-collective timing is first-class because the headline metric is
Allreduce algbw over xGMI.
"""

import torch


def algbw_gbps(nbytes: int, seconds: float) -> float:
    """Algorithmic bandwidth: bytes moved through the collective per second."""
    return nbytes / seconds / 1e9 if seconds > 0 else 0.0


def busbw_gbps(nbytes: int, seconds: float, world: int, op: str = "allreduce") -> float:
    """Bus bandwidth (NCCL convention): algbw corrected by the op's traffic
    factor — what the links actually carry. Ring allreduce moves
    2(P-1)/P bytes per byte of payload per GPU."""
    a = algbw_gbps(nbytes, seconds)
    if world <= 1:
        return a
    if op == "allreduce":
        return a * 2 * (world - 1) / world
    if op in ("allgather", "reducescatter", "alltoall"):
        return a * (world - 1) / world
    return a


def mxfp8_wire_bytes(numel: int) -> int:
    """Bytes AllreduceCompressed puts on the wire for ``numel`` elements:
    32 e4m3 payload bytes plus one shared-exponent byte per group of 32
    (the partial last group is padded), i.e. 33/32 byte per element —
    1.94x fewer than bf16, 3.88x fewer than fp32."""
    return 33 * ((numel + 31) // 32)


def mxfp8_reducescatter_wire_bytes(numel: int, world: int) -> int:
    """Bytes one rank sends in ReducescatterCompressed of ``numel`` elements
    over ``world`` ranks: its copy of every other rank's block, each block
    of numel/world elements quantized on its own (33 bytes per group of 32,
    the partial last group padded). Half of the compressed allreduce."""
    block = -(-numel // world)
    return (world - 1) * 33 * ((block + 31) // 32)


def mxfp8_allgather_wire_bytes(numel: int, world: int) -> int:
    """Bytes one rank receives in AllgatherCompressed of its own tensor of
    ``numel`` elements over ``world`` ranks: every other rank's tensor as
    one mxfp8 stream (33 bytes per group of 32, the partial last group
    padded)."""
    return (world - 1) * 33 * ((numel + 31) // 32)


def alltoall_compressed_wire_bytes(numel: int, world: int) -> int:
    """Bytes one rank sends in AlltoallCompressed of its own tensor of
    ``numel`` elements over ``world`` ranks: every other rank's block of
    numel/world elements, each quantized on its own (33 bytes per group of
    32, the partial last group padded)."""
    block = -(-numel // world)
    return (world - 1) * 33 * ((block + 31) // 32)


def mxfp8_alltoall_pairwise_wire_bytes(send_counts, slice_elems: int,
                                       rank: int) -> int:
    """Bytes rank ``rank`` sends in AlltoallPairwiseCompressed:
    ``send_counts[p]`` slices of ``slice_elems`` elements (the product of
    every dimension but the axis) to each other rank p, each block quantized
    on its own (33 bytes per group of 32, the partial last group padded).
    The block that stays local is not counted."""
    return sum(33 * ((c * slice_elems + 31) // 32)
               for p, c in enumerate(send_counts) if p != rank)


class CollectiveTimer:
    """Times GPU regions with CUDA/HIP events (no host sync until query)."""

    def __init__(self):
        self._events = []  # (label, nbytes, start, end)

    def span(self, label: str, nbytes: int = 0):
        timer = self

        class _Span:
            def __enter__(self):
                self.s = torch.cuda.Event(enable_timing=True)
                self.e = torch.cuda.Event(enable_timing=True)
                self.s.record()
                return self

            def __exit__(self, *exc):
                self.e.record()
                timer._events.append((label, nbytes, self.s, self.e))

        return _Span()

    def results(self):
        """Synchronizes and returns [(label, ms, algbw_GBps)]."""
        torch.cuda.synchronize()
        out = []
        for label, nbytes, s, e in self._events:
            ms = s.elapsed_time(e)
            out.append((label, ms, algbw_gbps(nbytes, ms / 1e3)))
        return out

    def clear(self):
        self._events.clear()
