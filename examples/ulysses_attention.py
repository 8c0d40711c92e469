"""Ulysses-style sequence-parallel attention via Alltoall resharding.

Each rank holds a sequence shard [B, S/P, H, D]; the two Alltoalls move it
to full-sequence/sharded-heads for attention and back. Both reshards are
autograd-transparent, so backward reshards gradients automatically.
--compression mxfp8 sends both reshards, and their backward, over the
block-scaled fp8 wire (AlltoallCompressed: 33/128 of the fp32 bytes).

Run: torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 2 \
        examples/ulysses_attention.py [--compression mxfp8]
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpi4torch_amd as m4a
from mpi4torch_amd.parallel import seq_to_head, head_to_seq

ap = argparse.ArgumentParser()
ap.add_argument("--compression", choices=["mxfp8"], default=None,
                help="send the reshards over the mxfp8 wire")
args = ap.parse_args()

device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
comm = m4a.COMM_WORLD

B, S, H, D = 2, 16 * comm.size, 4 * comm.size, 32
local = torch.randn(B, S // comm.size, H, D, device=device).requires_grad_()

q = seq_to_head(local, compression=args.compression)   # [B, S, H/P, D]
k, v = q, q
attn = torch.nn.functional.scaled_dot_product_attention(
    q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
).transpose(1, 2)
out = head_to_seq(attn.contiguous(),
                  compression=args.compression)        # [B, S/P, H, D]

out.sum().backward()
print(f"rank {comm.rank}: out {tuple(out.shape)}, grad norm "
      f"{float(local.grad.norm()):.3f}")
