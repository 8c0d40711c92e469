"""AlltoallPairwiseCompressedWeighted on the CPU: its three composites against
plain references (the float64 oracle, loops of fp32 products and adds), the
op at world sizes 1 and 2, and ExpertParallelMoE(gate_at="combine"). The GPU
file feeds the same case lists to the kernels."""

import numpy as np
import pytest
import torch

import mpi4torch_amd as m
import mx8_oracles as mo
from spmd import run_spmd
from test_alltoall_pairwise_indexed import (DTYPES, GEOMS, GEOM_IDS, wire,
                                            fan_index, nan_case, dropped_case)

COMBINE = [f"{i}-{str(d)[6:]}" for i in GEOM_IDS for d in DTYPES] + [
    "nan", "dropped", "zero_on_nan", "contraction"]
# (after, counts): every vector / twin split, an empty segment, > 32 segments
QUANT = [(a, c, d) for a, c in [(4, [3, 0, 5, 2]), (8, [3, 0, 5, 2]),
                                (40, [3, 0, 5, 2]), (41, [3, 0, 5, 2]),
                                (8, [i % 4 for i in range(33)])]
         for d in DTYPES]
QUANT_IDS = [f"{a}x{len(c)}-{str(d)[6:]}" for a, c, d in QUANT]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def values(pay, sc, after, counts):
    """The received slices by the float64 oracle: fp32 [R, after]."""
    rows, goff = [torch.zeros(0, after)], 0
    for c in counts:
        G = (c * after + 31) // 32
        if c:
            d = mo._f32(mo.dequantize(pay[32 * goff:32 * (goff + G)].numpy(),
                                      sc[goff:goff + G].numpy()))
            rows.append(torch.from_numpy(d).view(-1)[:c * after]
                        .view(c, after))
        goff += G
    return torch.cat(rows)


def reference(pay, sc, after, counts, index, w, out_size, fan, dtype):
    v = values(pay, sc, after, counts)
    acc = torch.zeros(out_size, after)
    seen = [0] * out_size
    for i, s in enumerate(index.tolist()):
        if 0 <= s < out_size and seen[s] < fan:
            term = w[i] * v[i]                   # fp32 product, rounded
            acc[s] = term if seen[s] == 0 else acc[s] + term
            seen[s] += 1
    return acc.to(dtype)


def combine_case(name):
    """name -> (pay, sc, after, counts, index, w, out_size, fan, dtype): the
    indexed file's geometries and special cases with random weights;
    zero_on_nan has weight 0 on its NaN sources, which stay NaN (IEEE);
    contraction adds (1.125 + 2^-23) * -1 and fl((1 + 2^-23) * 1.125), which
    is exactly 0 where an FMA keeps the product's 2^-26."""
    if name == "contraction":
        assert float(np.float32(1 + 2.0 ** -23) * np.float32(1.125)
                     - np.float32(1.125 + 2.0 ** -23)) == 0.0
        pay, sc = mo.quantize(np.repeat(np.float32([[-1.0], [1.125]]), 32, 1))
        return (torch.from_numpy(pay), torch.from_numpy(sc), 32, [2],
                torch.tensor([0, 0]),
                torch.tensor([1.125 + 2.0 ** -23, 1 + 2.0 ** -23]), 1, 2,
                torch.float32)
    if "-" in name:
        after, counts, fan = GEOMS[GEOM_IDS.index(name.split("-")[0])]
        pay, sc = wire(after, counts, after)
        index, out_size = fan_index(sum(counts), fan, after + 1)
        dtype = getattr(torch, name.split("-")[1])
    else:
        pay, sc, after, counts, index, out_size, fan = (
            dropped_case if name == "dropped" else nan_case)()
        dtype = torch.float32
    w = torch.randn(sum(counts), generator=gen(after + 2))
    return (pay, sc, after, counts, index, w * (name != "zero_on_nan"),
            out_size, fan, dtype)


@pytest.mark.parametrize("name", COMBINE)
def test_combine_composite(name):
    *a, dtype = combine_case(name)
    want = reference(*a, dtype)
    if name == "zero_on_nan":
        assert 0 < int(torch.isnan(want).sum()) <= 34
    if name == "contraction":
        assert bool((want == 0).all())
    n = want.numel()
    out = torch.full((n + 8,), 7.0, dtype=dtype)
    got = m._C._mx8_dequantize_combine_weighted(*a, dtype, out=out)
    mo.nan_aware_equal(got, want)
    assert bool((out[n:] == 7.0).all())


def quant_case(after, counts, dtype):
    """(x [N, after], index, w, want payload, want scales): a repeated index,
    a -1 (zeros), a zero weight, and 2^5 on slice 1, which moves the amax of
    its groups across binades."""
    S, N = sum(counts), 7
    x = torch.randn(N, after, generator=gen(after)).to(dtype)
    index = torch.randint(0, N, (S,), generator=gen(after + 1))
    index[0], index[3], index[4] = 2, 2, -1
    w = torch.randn(S, generator=gen(after + 2))
    w[1], w[2] = 32.0, 0.0
    xs = np.where((index >= 0).numpy()[:, None],
                  x.float().numpy()[index.clamp_min(0).numpy()],
                  np.float32(0))
    prod = torch.from_numpy(w.numpy()[:, None] * xs)
    assert prod.dtype == torch.float32
    streams = [prod[sum(counts[:p]):sum(counts[:p + 1])].reshape(-1)
               for p in range(len(counts))]
    return (x, index, w) + mo.quantize_streams(streams)


@pytest.mark.parametrize("after,counts,dtype", QUANT, ids=QUANT_IDS)
def test_quantize_composite(after, counts, dtype):
    x, index, w, pay, sc = quant_case(after, counts, dtype)
    got = m._C._mx8_quantize_segments_weighted(x.view(-1), after, counts, w,
                                               order=index)
    mo.bytes_equal(got[0], pay)
    mo.bytes_equal(got[1], sc)


def dot_bound(v, g, ref, after):
    """gamma_n for any summation order, plus half an fp32 ulp of the result"""
    return ((after + 2) * 2.0 ** -24 * (v.double() * g.double()).abs().sum(1)
            + 2.0 ** -24 * ref.abs())


def rowdot_case(after, R, dtype):
    """(pay, sc, counts, index, g, ref f64 [R], bound [R]): slice 1 names no
    row (exactly 0), slice 2 lies in a 255-scale group (NaN)."""
    counts, out_size = [R - R // 3, 0, R // 3], 5
    pay, sc = wire(after, counts, 100 + after)
    sc[(2 * after) // 32] = 255
    index = torch.randint(0, out_size, (R,), generator=gen(after))
    index[1] = out_size
    g = torch.randn(out_size, after, generator=gen(after + 1)).to(dtype)
    v = values(pay, sc, after, counts)
    rows = g[index.clamp_max(out_size - 1)] * (index < out_size).view(R, 1)
    ref = (v.double() * rows.double()).sum(1)
    bound = dot_bound(v, rows, ref, after)
    ref[1] = bound[1] = 0
    return pay, sc, counts, index, g, ref, bound


def check_rowdot(got, ref, bound):
    nan = torch.isnan(ref)
    # the 255 group's own slices (four of them at after = 8), no others
    assert 1 <= int(nan.sum()) <= 4 and torch.equal(torch.isnan(got), nan)
    assert float(got[1]) == 0.0
    err = (got.double() - ref).abs()
    assert bool((err[~nan] <= bound[~nan]).all()), (err / bound).max()


@pytest.mark.parametrize("after", [8, 41, 520])
def test_rowdot_composite(after):
    pay, sc, counts, index, g, ref, bound = rowdot_case(after, 37,
                                                        torch.bfloat16)
    check_rowdot(m._C._mx8_dequantize_rowdot(pay, sc, after, counts, index,
                                             g), ref, bound)


def test_error_checks():
    f = m.COMM_WORLD.AlltoallPairwiseCompressedWeighted
    x, i4, w4 = torch.ones(4, 4), torch.tensor([0, 1, 1, 3]), torch.ones(4)
    for match, args, kw in [
        ("recv_weights need a recv_index", (x, 0, [4], [4]),
         dict(recv_weights=w4)),
        ("send_weights are not differentiable", (x, 0, [4], [4]),
         dict(send_weights=w4.clone().requires_grad_())),
        ("recv_weights must be a 1-D tensor of length 4", (x, 0, [4], [4]),
         dict(recv_index=i4, recv_weights=w4[:3], out_size=4, max_repeat=2)),
        ("send_weights must be float32 or the tensor's dtype",
         (x, 0, [4], [4]), dict(send_weights=w4.double())),
        ("recv_weights must be on the tensor's device", (x, 0, [4], [4]),
         dict(recv_index=i4, recv_weights=w4.to("meta"), out_size=4,
              max_repeat=2)),
        ("with weights every dimension before the axis must have size 1",
         (torch.ones(2, 4, 4), 1, [4], [4]), dict(send_weights=w4)),
        # the checks it shares with the Indexed op, under its own name
        ("Weighted: send_counts must have world_size entries",
         (x, 0, [2, 2], [4]), dict(send_weights=w4)),
        ("Weighted: recv_counts must have world_size entries",
         (x, 0, [4], [2, 2]), dict(send_weights=w4)),
        ("Weighted: negative send count -1", (x, 0, [-1], [4]),
         dict(send_weights=w4)),
        ("Weighted: negative recv count -2", (x, 0, [4], [-2]),
         dict(send_weights=w4)),
        ("Weighted: max_repeat must be >= 1, got 0", (x, 0, [4], [4]),
         dict(send_weights=w4, max_repeat=0)),
        ("Weighted: without a send_index the sum of send_counts \\(3\\) must "
         "equal the axis size \\(4\\)", (x, 0, [3], [3]),
         dict(send_weights=w4[:3])),
        ("Weighted: out_size is required with a recv_index", (x, 0, [4], [4]),
         dict(recv_index=i4, recv_weights=w4)),
        ("Weighted: out_size must be >= 0, got -1", (x, 0, [4], [4]),
         dict(send_weights=w4, out_size=-1)),
        ("Weighted: send_index must be a 1-D tensor of length 4",
         (x, 0, [4], [4]), dict(send_index=i4[:3], send_weights=w4)),
        ("Weighted: send_index must be an int64", (x, 0, [4], [4]),
         dict(send_index=i4.int(), send_weights=w4)),
        ("Weighted: recv_index must be on the tensor's device",
         (x, 0, [4], [4]),
         dict(recv_index=i4.to("meta"), recv_weights=w4, out_size=4)),
        ("Weighted: recv_index entries must lie in \\[0, 3\\)",
         (x, 0, [4], [4]),
         dict(recv_index=i4, recv_weights=w4, out_size=3, max_repeat=2)),
        ("Weighted: a slice occurs 2 times in send_index, more than "
         "max_repeat = 1", (x, 0, [4], [4]),
         dict(send_index=i4, send_weights=w4)),
    ]:
        with pytest.raises(RuntimeError, match=match):
            f(*args, **kw)


def op_case(comm, rank, world, device="cpu"):
    """A top-2 combine with gates through the op. Every rank's routing and
    rows come from its seed, so a rank rebuilds what it must have received:
    the forward is the debug bindings composed, gx the swapped send-weighted
    op. Returns gw, the composite's row dot of those bytes and the bound."""
    C, N, D, k = m._C, 11, 40, 2
    owners = [torch.randint(0, world, (N * k,), generator=gen(60 + r))
              for r in range(world)]
    sends = [torch.bincount(o, minlength=world).tolist() for o in owners]
    recvs = [[sends[q][r] for q in range(world)] for r in range(world)]
    ys = [torch.randn(sum(recvs[r]), D, generator=gen(160 + r))
          for r in range(world)]
    send, recv = sends[rank], recvs[rank]
    arrived = torch.cat([ys[p][sum(recvs[p][:rank]):sum(recvs[p][:rank + 1])]
                         for p in range(world)])
    g = gen(260 + rank)
    tok = (torch.argsort(owners[rank], stable=True) // k).to(device)
    y = ys[rank].to(device).requires_grad_()
    w = torch.rand(N * k, generator=g).to(device).requires_grad_()
    ct = torch.randn(N, D, generator=g).to(device)
    f = comm.AlltoallPairwiseCompressedWeighted
    z = f(y, 0, recv, [], recv_index=tok, recv_weights=w, out_size=N,
          max_repeat=k)
    gy, gw = torch.autograd.grad(z, (y, w), ct)
    want = f(ct, 0, send, recv, send_index=tok, send_weights=w.detach(),
             max_repeat=k)
    assert torch.equal(gy.view(torch.int32), want.view(torch.int32))
    p, s = C._mx8_quantize_segments(arrived.view(-1), 1, D, send)
    mo.nan_aware_equal(z.detach().cpu(), C._mx8_dequantize_combine_weighted(
        p, s, D, send, tok.cpu(), w.detach().cpu(), N, k, torch.float32))
    ref = C._mx8_dequantize_rowdot(p, s, D, send, tok.cpu(), ct.cpu())
    return gw.cpu(), ref, dot_bound(values(p, s, D, send), ct.cpu()[tok.cpu()],
                                    ref, D)


def full_path(mod, fn):
    mod._C.force_full_path(True)
    try:
        return fn()
    finally:
        mod._C.force_full_path(False)


def test_op_world1_full_path():
    gw, ref, _ = full_path(m, lambda: op_case(m.COMM_WORLD, 0, 1))
    assert torch.equal(gw, ref)


def moe_layer(device="cpu", **kw):
    from mpi4torch_amd.models.moe import ExpertParallelMoE
    torch.manual_seed(5)
    kw = dict(dict(top_k=2, compression="mxfp8", gate_at="combine"), **kw)
    return ExpertParallelMoE(32, 4, d_hidden=16, **kw).to(device)


def _ws2_worker(rank, world):
    gw, ref, _ = op_case(m.COMM_WORLD, rank, world)
    assert torch.equal(gw, ref)
    layer, calls, plain = moe_layer(), [], m.COMM_WORLD.AlltoallPairwise
    layer.comm.AlltoallPairwise = \
        lambda *a: calls.append(a[0].shape) or plain(*a)
    x = torch.randn(12, 32, generator=gen(rank), requires_grad=True)
    layer(x).sum().backward()
    assert len(calls) == 1 and calls[0][1] == 1     # the expert ids alone
    assert bool(torch.isfinite(layer.router.weight.grad).all())


def test_op_and_layer_ws2():
    run_spmd(2, _ws2_worker)


def test_world1_default_is_exact():
    """No codec at world 1: the fp32 weighted sum of the values, and both
    gradients on the values themselves."""
    f = m.COMM_WORLD.AlltoallPairwiseCompressedWeighted
    y = (torch.full((6, 40), 1.0 / 3.0) * torch.arange(1, 7).view(6, 1)) \
        .bfloat16().requires_grad_()
    tok = torch.tensor([4, 0, 0, 2, 4, 4])
    w = torch.tensor([0.3, 0.7, 0.11, 1.0, 0.5, 0.25], requires_grad=True)
    z = f(y, 0, [6], [6], recv_index=tok, recv_weights=w, out_size=6,
          max_repeat=3)
    yf, wd = y.detach().float(), w.detach()
    want = torch.zeros(6, 40)
    want[0] = wd[1] * yf[1] + wd[2] * yf[2]
    want[2] = wd[3] * yf[3]
    want[4] = wd[0] * yf[0] + wd[4] * yf[4] + wd[5] * yf[5]
    assert torch.equal(z.view(torch.int16), want.bfloat16().view(torch.int16))
    ct = torch.randn(6, 40, generator=gen(1)).bfloat16()
    gy, gw = torch.autograd.grad(z, (y, w), ct)
    assert torch.equal(gy, (wd.view(6, 1) * ct.float()[tok]).bfloat16())
    assert torch.equal(gw, (yf * ct.float()[tok]).sum(1))


def dense_top2(layer, x):
    """The layer's math, dense and in fp32, with no transfers: (y, S) with S
    the per-element sum of the magnitudes of the terms y adds up."""
    gate, expert = torch.softmax(layer.router(x), dim=-1).topk(2, dim=-1)
    acts = [e[1](e[0](x)) for e in layer.experts]
    outs = [e[2](a) for e, a in zip(layer.experts, acts)]
    mags = [a.abs() @ e[2].weight.abs().T + e[2].bias.abs()
            for e, a in zip(layer.experts, acts)]

    def mix(t):
        pick = torch.stack(t, 1).gather(
            1, expert.unsqueeze(2).expand(-1, -1, x.shape[1]))
        return (gate.unsqueeze(2) * pick).sum(1)
    return mix(outs), mix(mags).detach()


def test_moe_gate_at_combine_world1_matches_dense():
    """Output, x.grad and every parameter gradient against the dense
    reference under (n + 2) * 2^-24 * S, n = k * d_hidden = 32, S the
    per-element sum of the magnitudes of the terms of the element's last
    contraction in the reference: |delta|^T |a| for a weight, sum |delta| for
    a bias, |delta| |W| over the linears that read x (delta: the gradient at
    a linear's output, a: its input)."""
    layer = moe_layer()
    x = torch.randn(24, 32, generator=gen(1))
    xg, xr, seen = x.clone().requires_grad_(), x.clone().requires_grad_(), []
    (layer(xg) ** 2).sum().backward()
    got = [layer(xg).detach(), xg.grad] + [p.grad for p in layer.parameters()]
    layer.zero_grad()
    hooks = [mod.register_forward_hook(
        lambda mod, i, o: o.retain_grad() or seen.append((mod, i[0], o)))
        for mod in layer.modules() if isinstance(mod, torch.nn.Linear)]
    yr, S_y = dense_top2(layer, xr)
    (yr ** 2).sum().backward()
    [h.remove() for h in hooks]
    S = {}
    for mod, a, o in seen:
        S[mod.weight] = o.grad.abs().T @ a.detach().abs()
        S[mod.bias] = o.grad.abs().sum(0)
    S_x = sum(o.grad.abs() @ mod.weight.detach().abs()
              for mod, a, o in seen if a is xr)
    want = [yr.detach(), xr.grad] + [p.grad for p in layer.parameters()]
    mags = [S_y, S_x] + [S[p] for p in layer.parameters()]
    for a, b, s in zip(got, want, mags):
        assert bool(((a - b).abs() <= (2 * 16 + 2) * 2.0 ** -24 * s).all())


def test_moe_gate_at_owner_is_the_default_and_checks():
    from mpi4torch_amd.models.moe import ExpertParallelMoE
    x = torch.randn(24, 32, generator=gen(1))
    torch.manual_seed(5)                         # moe_layer's seed
    plain = ExpertParallelMoE(32, 4, d_hidden=16, top_k=2, compression="mxfp8")
    assert torch.equal(moe_layer(gate_at="owner")(x), plain(x))
    for kw in (dict(top_k=1, compression="mxfp8"), dict(top_k=2)):
        with pytest.raises(ValueError, match="gate_at='combine' needs"):
            ExpertParallelMoE(32, 4, gate_at="combine", **kw)
