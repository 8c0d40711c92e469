"""The CPU side of the local-reduce contracts (no GPU needed).

The torch composites that serve the gloo transport are held to the same
plain references (tests/reduce_oracles.py) as the gfx950 kernels in
test_gpu_kernel_edges.py, so both transports return the same results for
NaN values, ties, 64-bit locations and fp8 overflow.
"""

import pytest
import torch

import reduce_oracles as ro
from spmd import run_spmd


@pytest.mark.parametrize("dtype", ro.PAIRLOC_DTYPES,
                         ids=lambda d: str(d).replace("torch.", ""))
def test_pairloc_composite_ties_nan(dtype):
    import mpi4torch_amd as m

    for P in (1, 2, 6):
        for n in (1, 1027):
            for name, stacked in ro.pairloc_cases(dtype, P, n, seed=31 * P + n):
                for op in (0, 1):  # minloc, maxloc
                    got = m._C._pairloc_reduce(stacked, op)
                    ro.pairloc_check(got, stacked, op == 1,
                                     (dtype, P, n, name, op))


def _fp8_pairs_worker(rank, world):
    # The fp8 branch of the hierarchical lowering only reduces at world > 1
    # (a world of one returns a clone), so the pair table is split over two
    # ranks: rank 0 holds byte i // 256, rank 1 byte i % 256.
    import os

    os.environ["MPI4TORCH_AMD_FORCE_HIERARCHICAL"] = "1"
    import mpi4torch_amd as m

    m._C.reload_config()
    comm = m.COMM_WORLD
    ops = {"sum": m.MPI_SUM, "prod": m.MPI_PROD, "min": m.MPI_MIN,
           "max": m.MPI_MAX}
    # 65536 splits into two vector-friendly halves, 65539 into odd blocks
    for extra in (0, 3):
        mine = ro.fp8_pair_sources(extra)[rank]
        for enc in ro.FP8_ENCODINGS:
            for opname in ro.FP8_OPS:
                got = comm.Allreduce(mine.view(enc), ops[opname])
                assert got.dtype == enc
                share = ro.fp8_check(
                    got.view(torch.uint8), enc,
                    ro.fp8_pair_reference(enc, opname, extra),
                    (enc, opname, extra))
                assert share >= 0.8, (enc, opname, share)


def test_fp8_allreduce_all_pairs_ws2():
    run_spmd(2, _fp8_pairs_worker)
