from .timing import (CollectiveTimer, algbw_gbps, busbw_gbps,
                     mxfp8_wire_bytes, mxfp8_reducescatter_wire_bytes,
                     mxfp8_allgather_wire_bytes,
                     alltoall_compressed_wire_bytes,
                     mxfp8_alltoall_pairwise_wire_bytes)
from .tracing import trace, TracedCommunicator, TraceRecord
from .checkpoint import (save_checkpoint, load_checkpoint,
                         save_sharded_checkpoint, load_sharded_checkpoint)
from .clip import clip_grad_norm_sharded

__all__ = [
    "CollectiveTimer",
    "algbw_gbps",
    "busbw_gbps",
    "mxfp8_wire_bytes",
    "mxfp8_reducescatter_wire_bytes",
    "mxfp8_allgather_wire_bytes",
    "alltoall_compressed_wire_bytes",
    "mxfp8_alltoall_pairwise_wire_bytes",
    "trace",
    "TracedCommunicator",
    "TraceRecord",
    "save_checkpoint",
    "load_checkpoint",
    "save_sharded_checkpoint",
    "load_sharded_checkpoint",
    "clip_grad_norm_sharded",
]
