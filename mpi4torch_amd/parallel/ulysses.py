"""DeepSpeed-Ulysses-style sequence<->head resharding on Alltoall.

The reference's axis-aware Alltoall IS the Ulysses reshard primitive
(reference csrc/extension.cpp:917-987): moving a
[batch, seq/P, heads, dim] activation to [batch, seq, heads/P, dim] and
back is Alltoall(gatheraxis=seq, scatteraxis=heads, numelem=heads/P).
Because Alltoall is autograd-transparent, the backward reshards the
gradient the opposite way automatically — attention code using these
helpers needs no custom autograd.

compression="mxfp8" sends the activation over the block-scaled fp8 wire
instead (AlltoallCompressed: 33/64 of the bf16 bytes, 33/128 of the fp32
ones, quantized once per direction; the backward reshard travels compressed
too). The default None is the uncompressed path, unchanged.
"""

import torch

import mpi4torch_amd as m4a


def _check_compression(compression):
    if compression not in (None, "mxfp8"):
        raise ValueError(
            "mpi4torch_amd Ulysses: compression must be None or 'mxfp8', "
            f"got {compression!r}")


def ulysses_reshard(t: torch.Tensor, gather_axis: int, scatter_axis: int,
                    numelem: int, comm=None,
                    compression=None) -> torch.Tensor:
    """General reshard: gather `gather_axis` across ranks, scatter
    `scatter_axis`, keeping `numelem` slices of it locally. With
    compression="mxfp8" the counts must be equal (`numelem` is the
    scatter-axis size over the world size on every rank)."""
    _check_compression(compression)
    comm = comm if comm is not None else m4a.COMM_WORLD
    if compression is not None:
        if numelem * comm.size != t.size(scatter_axis):
            raise ValueError(
                "mpi4torch_amd Ulysses: compression='mxfp8' needs equal "
                f"counts: numelem ({numelem}) times the world size "
                f"({comm.size}) must equal the scatter-axis size "
                f"({t.size(scatter_axis)})")
        return comm.AlltoallCompressed(t, gather_axis, scatter_axis)
    return comm.Alltoall(t, gather_axis, scatter_axis, numelem)


def seq_to_head(t: torch.Tensor, comm=None, seq_axis: int = 1,
                head_axis: int = 2, compression=None) -> torch.Tensor:
    """[b, s/P, h, d] -> [b, s, h/P, d]: full sequence, sharded heads —
    the layout attention wants. Uses the explicit-counts Alltoallv (all
    counts are uniform and locally known), skipping the host exchanges;
    compression="mxfp8" uses AlltoallCompressed instead."""
    _check_compression(compression)
    comm = comm if comm is not None else m4a.COMM_WORLD
    heads = t.size(head_axis)
    assert heads % comm.size == 0, (
        f"head count {heads} must divide by world size {comm.size}")
    if compression is not None:
        return comm.AlltoallCompressed(t, seq_axis, head_axis)
    if comm.size == 1:
        return comm.Alltoall(t, seq_axis, head_axis, heads)
    target = [heads // comm.size] * comm.size
    source = [t.size(seq_axis)] * comm.size
    return comm.Alltoallv(t, seq_axis, head_axis, target, source)


def head_to_seq(t: torch.Tensor, comm=None, seq_axis: int = 1,
                head_axis: int = 2, compression=None) -> torch.Tensor:
    """[b, s, h/P, d] -> [b, s/P, h, d]: back to sequence sharding."""
    _check_compression(compression)
    comm = comm if comm is not None else m4a.COMM_WORLD
    seq = t.size(seq_axis)
    assert seq % comm.size == 0, (
        f"sequence length {seq} must divide by world size {comm.size}")
    if compression is not None:
        return comm.AlltoallCompressed(t, head_axis, seq_axis)
    if comm.size == 1:
        return comm.Alltoall(t, head_axis, seq_axis, seq)
    target = [seq // comm.size] * comm.size
    source = [t.size(head_axis)] * comm.size
    return comm.Alltoallv(t, head_axis, seq_axis, target, source)
