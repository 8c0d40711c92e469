"""Expert-parallel mixture-of-experts layer on AlltoallPairwise.

The BASELINE config #5 pattern ("expert-parallel alltoall") as a working
layer: experts are sharded across ranks; each token is routed (top-1,
softmax-gated) to its expert's owner with one pairwise-count Alltoall,
processed, and combined back with the reverse Alltoall. Both transfers are
autograd-transparent, so router and expert gradients need no custom
backward — the dispatch's adjoint returns token gradients to their
senders automatically.

compression="mxfp8" sends the tokens over the block-scaled fp8 wire with
AlltoallPairwiseCompressed: the sort by destination rank is fused into the
quantize kernel on the way out (no x_sorted is materialised) and the inverse
permutation into the dequantize kernel on the way back, so the layer loses
two full passes over the tokens as well as wire bytes. Expert ids stay on the
uncompressed AlltoallPairwise because they must arrive exact. The default
None leaves the layer bit for bit as it was.

top_k > 1 routes every token to its k best experts (topk of the softmax
gates, not renormalised). The N*k assignments are sorted by owner; expert ids
and assignment gates travel uncompressed, the owner scales its expert output
by the received gate, and the combine sums a token's k results. With
compression="mxfp8" both transfers are AlltoallPairwiseCompressedIndexed: the
dispatch gathers token order // k while it quantizes and the combine adds the
k received rows of a token in fp32 while it dequantizes, so neither the
gathered tokens nor an [N*k, D] combine buffer is materialised. top_k=1 takes
the two top-1 paths above, untouched.

gate_at="combine" (top_k > 1 with compression="mxfp8" only) applies the gate
on the token's home rank instead: the combine is
AlltoallPairwiseCompressedWeighted with the gates as receive weights, so the
expert output is quantized ungated, the gate multiplies in fp32 inside the
kernel that sums, and the gates never travel. A layer step then has two token
transfers and the id transfer in forward and two token transfers in backward,
against three transfers each way with the default "owner", and the router's
gradient is a fused dot on the home rank.
"""

import torch

import mpi4torch_amd as m4a


class ExpertParallelMoE(torch.nn.Module):
    def __init__(self, d_model: int, n_experts: int, comm=None,
                 d_hidden: int = None, compression=None, top_k: int = 1,
                 gate_at: str = "owner"):
        super().__init__()
        if compression not in (None, "mxfp8"):
            raise ValueError(
                "mpi4torch_amd ExpertParallelMoE: compression must be None "
                f"or 'mxfp8', got {compression!r}")
        if not 1 <= top_k <= n_experts:
            raise ValueError(
                "mpi4torch_amd ExpertParallelMoE: top_k must lie in "
                f"[1, n_experts = {n_experts}], got {top_k!r}")
        if gate_at not in ("owner", "combine"):
            raise ValueError(
                "mpi4torch_amd ExpertParallelMoE: gate_at must be 'owner' or "
                f"'combine', got {gate_at!r}")
        if gate_at == "combine" and not (top_k > 1 and compression == "mxfp8"):
            raise ValueError(
                "mpi4torch_amd ExpertParallelMoE: gate_at='combine' needs "
                "top_k > 1 and compression='mxfp8' (the gate rides in the "
                f"weighted mxfp8 combine), got top_k={top_k!r}, "
                f"compression={compression!r}")
        self.compression = compression
        self.top_k = top_k
        self.gate_at = gate_at
        self.comm = comm if comm is not None else m4a.COMM_WORLD
        P = self.comm.size
        assert n_experts % P == 0, (
            f"n_experts {n_experts} must divide world size {P}")
        self.n_experts = n_experts
        self.experts_per_rank = n_experts // P
        d_hidden = d_hidden or 4 * d_model
        self.router = torch.nn.Linear(d_model, n_experts)
        # this rank's experts
        self.experts = torch.nn.ModuleList([
            torch.nn.Sequential(
                torch.nn.Linear(d_model, d_hidden),
                torch.nn.GELU(),
                torch.nn.Linear(d_hidden, d_model),
            )
            for _ in range(self.experts_per_rank)
        ])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [N, D] local tokens -> [N, D]."""
        if self.top_k > 1:
            return self._forward_topk(x)
        if self.compression is not None:
            return self._forward_compressed(x)
        N, D = x.shape
        P = self.comm.size
        logits = self.router(x)
        gates = torch.softmax(logits, dim=-1)
        expert = torch.argmax(gates, dim=-1)          # [N], global expert id
        gate = gates.gather(1, expert.unsqueeze(1)).squeeze(1)  # [N]
        owner = expert // self.experts_per_rank       # destination rank

        # sort tokens by destination rank (stable: preserves order per dest)
        order = torch.argsort(owner, stable=True)
        inverse = torch.empty_like(order)
        inverse[order] = torch.arange(N, device=x.device)
        x_sorted = x.index_select(0, order)
        send_counts = torch.bincount(owner, minlength=P).tolist()

        # one count-matrix exchange serves both transfers explicitly
        recv_counts = self._recv_counts(send_counts)

        # dispatch tokens and (gradient-free) expert ids to the owners
        dispatched = self.comm.AlltoallPairwise(x_sorted, 0, send_counts,
                                                recv_counts)
        eid_sorted = expert.index_select(0, order).to(torch.float64)
        eid = self.comm.AlltoallPairwise(
            eid_sorted.unsqueeze(1), 0, send_counts,
            recv_counts).squeeze(1).long()
        local_eid = eid - self.comm.rank * self.experts_per_rank

        # run this rank's experts on their token groups
        out = torch.zeros_like(dispatched)
        for e in range(self.experts_per_rank):
            mask = local_eid == e
            if bool(mask.any()):
                idx = mask.nonzero(as_tuple=True)[0]
                out = out.index_copy(
                    0, idx, self.experts[e](dispatched.index_select(0, idx)))

        # combine: the reverse pairwise transfer (counts transpose)
        combined = self.comm.AlltoallPairwise(out, 0, recv_counts,
                                              send_counts)

        y = combined.index_select(0, inverse)
        return y * gate.unsqueeze(1)

    def _check_mx8_params(self):
        ok = (torch.float32, torch.bfloat16, torch.float16)
        for name, p in self.named_parameters():
            if p.dtype not in ok:
                raise TypeError(
                    "mpi4torch_amd ExpertParallelMoE: compression='mxfp8' "
                    "needs float32, bfloat16 or float16 parameters, got "
                    f"{p.dtype} for {name}")

    def _run_experts(self, dispatched, local_eid):
        out = torch.zeros_like(dispatched)
        for e in range(self.experts_per_rank):
            mask = local_eid == e
            if bool(mask.any()):
                idx = mask.nonzero(as_tuple=True)[0]
                out = out.index_copy(
                    0, idx, self.experts[e](dispatched.index_select(0, idx)))
        return out

    def _forward_topk(self, x: torch.Tensor) -> torch.Tensor:
        """forward() for top_k > 1: N*k assignments, sorted by owner."""
        mx8 = self.compression is not None
        if mx8:
            self._check_mx8_params()
        N, D = x.shape
        P, k = self.comm.size, self.top_k
        gates = torch.softmax(self.router(x), dim=-1)
        gate, expert = gates.topk(k, dim=-1)          # [N, k] each
        expert = expert.reshape(-1)                   # assignment n*k + j
        owner = expert // self.experts_per_rank
        order = torch.argsort(owner, stable=True)     # assignments by owner
        tok = order // k                              # their tokens
        send_counts = torch.bincount(owner, minlength=P).tolist()
        recv_counts = self._recv_counts(send_counts)

        # dispatch: stream slice i is token tok[i]; a token travels k times
        if mx8:
            dispatched = self.comm.AlltoallPairwiseCompressedIndexed(
                x, 0, send_counts, recv_counts, send_index=tok, max_repeat=k)
        else:
            dispatched = self.comm.AlltoallPairwise(
                x.index_select(0, tok), 0, send_counts, recv_counts)
        # expert ids and gates must arrive exact: uncompressed. The gate
        # keeps its autograd path, so the router needs no custom backward.
        eid = self.comm.AlltoallPairwise(
            expert.index_select(0, order).to(torch.float64).unsqueeze(1), 0,
            send_counts, recv_counts).squeeze(1).long()
        if self.gate_at == "combine":
            # the gate stays home: it weights the k received rows of a token
            # in fp32 while the combine sums them
            local_eid = eid - self.comm.rank * self.experts_per_rank
            return self.comm.AlltoallPairwiseCompressedWeighted(
                self._run_experts(dispatched, local_eid), 0, recv_counts,
                send_counts, recv_index=tok,
                recv_weights=gate.reshape(-1).index_select(0, order),
                out_size=N, max_repeat=k)
        g = self.comm.AlltoallPairwise(
            gate.reshape(-1).index_select(0, order).unsqueeze(1), 0,
            send_counts, recv_counts)
        local_eid = eid - self.comm.rank * self.experts_per_rank

        # the owner applies the gate, which keeps the wire op linear
        out = self._run_experts(dispatched, local_eid) * g

        # combine: a token's k results are summed where they arrive
        if mx8:
            return self.comm.AlltoallPairwiseCompressedIndexed(
                out, 0, recv_counts, send_counts, recv_index=tok, out_size=N,
                max_repeat=k)
        combined = self.comm.AlltoallPairwise(out, 0, recv_counts,
                                              send_counts)
        inverse = torch.empty_like(order)
        inverse[order] = torch.arange(N * k, device=x.device)
        return combined.index_select(0, inverse).view(N, k, D).sum(1)

    def _forward_compressed(self, x: torch.Tensor) -> torch.Tensor:
        """forward() over the mxfp8 wire: both token permutes ride inside
        the codec kernels of AlltoallPairwiseCompressed."""
        self._check_mx8_params()
        P = self.comm.size
        logits = self.router(x)
        gates = torch.softmax(logits, dim=-1)
        expert = torch.argmax(gates, dim=-1)          # [N], global expert id
        gate = gates.gather(1, expert.unsqueeze(1)).squeeze(1)  # [N]
        owner = expert // self.experts_per_rank       # destination rank

        # sort tokens by destination rank (stable: preserves order per dest)
        order = torch.argsort(owner, stable=True)
        send_counts = torch.bincount(owner, minlength=P).tolist()
        recv_counts = self._recv_counts(send_counts)

        # dispatch: the quantize kernel gathers token order[i] as stream
        # slice i while it reads
        dispatched = self.comm.AlltoallPairwiseCompressed(
            x, 0, send_counts, recv_counts, send_order=order)
        # expert ids must arrive exact: uncompressed
        eid_sorted = expert.index_select(0, order).to(torch.float64)
        eid = self.comm.AlltoallPairwise(
            eid_sorted.unsqueeze(1), 0, send_counts,
            recv_counts).squeeze(1).long()
        local_eid = eid - self.comm.rank * self.experts_per_rank

        out = torch.zeros_like(dispatched)
        for e in range(self.experts_per_rank):
            mask = local_eid == e
            if bool(mask.any()):
                idx = mask.nonzero(as_tuple=True)[0]
                out = out.index_copy(
                    0, idx, self.experts[e](dispatched.index_select(0, idx)))

        # combine: the dequantize kernel scatters received slice i to token
        # order[i] while it writes — the inverse permutation
        y = self.comm.AlltoallPairwiseCompressed(
            out, 0, recv_counts, send_counts, recv_order=order)
        return y * gate.unsqueeze(1)

    def _recv_counts(self, send_counts):
        """Dispatch recv counts = my column of the P x P count matrix;
        one exchange serves dispatch, id transfer and combine (counts are
        data-dependent — recomputed every forward)."""
        P = self.comm.size
        if P == 1:
            return list(send_counts)
        t = torch.tensor(send_counts, dtype=torch.float64)
        mat = self.comm.Allgather(t.unsqueeze(0), 0)  # [P, P]
        return [int(v) for v in mat[:, self.comm.rank].tolist()]
