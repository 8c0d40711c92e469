// Communicator: the TorchScript custom class at the center of
// mpi4torch_amd. Parity target: MPI_Comm_Wrapper in the reference
// (helmholtz-analytics/mpi4torch csrc/extension.cpp:140-187), with the
// communicator identified by a c10d group name instead of a raw MPI_Comm
// (sub-communicators arrive through torch.distributed groups rather than
// mpi4py Fortran handles, reference :168-171).
#pragma once

#include "common.hpp"

#include <ATen/ATen.h>
#include <torch/custom_class.h>

#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

namespace m4a {

struct Transport;

struct Communicator : torch::CustomClassHolder {
  explicit Communicator(std::string group_name);

  int64_t GetRank();
  int64_t GetSize();

  // Collectives (autograd-transparent; adjoints per SURVEY.md §3.3).
  at::Tensor Allreduce(const at::Tensor& input, int64_t op);
  // Block-scaled fp8 compressed allreduce (MI355X extension): the tensor
  // travels as mxfp8 (32 e4m3 bytes + one shared-exponent byte per 32
  // elements, 33/32 byte per element) through the hierarchical exchange +
  // fused gfx950 reduce kernel; values are quantized exactly twice at any
  // world size. MPI_SUM only; float32/bfloat16/float16 only. Backward:
  // AllreduceCompressed of the gradient (self-adjoint sum, straight-through
  // quantization). A world of one returns an exact clone.
  at::Tensor AllreduceCompressed(const at::Tensor& input, int64_t op);
  at::Tensor Bcast_(const at::Tensor& input, int64_t root);
  at::Tensor Reduce_(const at::Tensor& input, int64_t op, int64_t root);
  at::Tensor Gather(const at::Tensor& input, int64_t gatheraxis, int64_t root);
  at::Tensor Allgather(const at::Tensor& input, int64_t gatheraxis);
  // Adjoint pair of Allgather, exposed as a public collective (MI355X
  // extension; not in the reference API): elementwise-SUM across ranks,
  // then this rank keeps `numelem` slices of `axis` (per-rank counts may
  // differ). Backward: Allgather of the gradient. Enables ZeRO-style
  // gradient/optimizer sharding (parallel/zero.py).
  at::Tensor Reducescatter(const at::Tensor& input, int64_t axis,
                           int64_t numelem);
  // Sum reduce-scatter over the mxfp8 wire (MI355X extension): the axis is
  // split into GetSize() equal blocks, each block is quantized once in
  // groups of 32 that start at the block, block j travels to rank j, and
  // the fused gfx950 tail sums the copies in fp32 straight into the input
  // dtype (no requantization, no allgather: half the wire bytes of
  // AllreduceCompressed). float32/bfloat16/float16 only; the axis size
  // must be a multiple of the world size. Backward: uncompressed Allgather
  // of the gradient. A world of one returns an exact clone.
  at::Tensor ReducescatterCompressed(const at::Tensor& input, int64_t axis);
  // Allgather over the mxfp8 wire (MI355X extension): every rank's tensor
  // (equal sizes on `axis`) is quantized once in groups of 32 that start at
  // its first element, payload and scales are allgathered as bytes, and the
  // fused gfx950 tail dequantizes every block — the own one included, so
  // all ranks hold identical bytes — straight into its place along `axis`.
  // float32/bfloat16/float16 only. Backward: ReducescatterCompressed of the
  // gradient. A world of one returns an exact clone.
  at::Tensor AllgatherCompressed(const at::Tensor& input, int64_t axis);
  // Equal-count, two-axis all-to-all over the mxfp8 wire (MI355X
  // extension): the scatter axis is split into GetSize() equal blocks, a
  // fused gfx950 kernel quantizes every block in place (groups of 32 that
  // start at the block), block j travels to rank j in one grouped
  // exchange, and the fused tail dequantizes the received blocks, the own
  // one included, straight into place along the gather axis (equal sizes
  // on every rank). No pack or unpack pass; every value is quantized
  // exactly once. float32/bfloat16/float16 only; the two axes must differ.
  // Backward: AlltoallCompressed of the gradient with the axes swapped. A
  // world of one returns an exact clone.
  at::Tensor AlltoallCompressed(const at::Tensor& input, int64_t gatheraxis,
                                int64_t scatteraxis);
  at::Tensor Scatter(const at::Tensor& input, int64_t scatteraxis,
                     int64_t numelem, int64_t root);
  at::Tensor Alltoall(const at::Tensor& input, int64_t gatheraxis,
                      int64_t scatteraxis, int64_t numelem);
  // Explicit-counts variant (MI355X extension; not in the reference):
  // skips the two host count exchanges when the caller already knows every
  // rank's counts (expert-parallel routing). target_counts[j] = what rank j
  // keeps along scatteraxis; source_sizes[j] = rank j's current
  // gather/partition-axis size.
  at::Tensor Alltoallv(const at::Tensor& input, int64_t gatheraxis,
                       int64_t scatteraxis,
                       std::vector<int64_t> target_counts,
                       std::vector<int64_t> source_sizes);
  at::Tensor AlltoallvImpl(const at::Tensor& input, int64_t gatheraxis,
                           int64_t scatteraxis, int64_t numelem,
                           const std::vector<int64_t>& target_counts,
                           const std::vector<int64_t>& source_sizes);
  // Pairwise-count alltoall (MI355X extension): rank r sends
  // send_counts[j] slices of `axis` to rank j (arbitrary P x P count
  // matrix — the expert-parallel token dispatch, inexpressible as the
  // reference's interval repartition). recv_counts, if empty, are
  // exchanged over the host channel. Backward sends every received slice
  // back (the exact adjoint).
  at::Tensor AlltoallPairwise(const at::Tensor& input, int64_t axis,
                              std::vector<int64_t> send_counts,
                              std::vector<int64_t> recv_counts);

  // AlltoallPairwise over the mxfp8 wire with the slice permute fused into
  // the codec kernels (MI355X extension): the expert-parallel
  // dispatch/combine primitive. With xs = input.index_select(axis,
  // send_order) (or input), block j = xs[.., sdispl_j : +send_counts[j], ..]
  // is quantized once in groups of 32 that start at the block and travels to
  // rank j in one grouped exchange; the received blocks, the own one
  // included, are dequantized into y along `axis` in rank order, and the
  // result is y or, with recv_order, the tensor with
  // out.index_copy_(axis, recv_order, y). Neither permute is a pass of its
  // own: the gfx950 head gathers while it reads, the tail scatters while it
  // writes. float32/bfloat16/float16 only; the orders are int64 permutations
  // on the tensor's device. Backward: the same op on the gradient with
  // counts and orders swapped. A world of one returns the exact permutation.
  at::Tensor AlltoallPairwiseCompressed(
      const at::Tensor& input, int64_t axis, std::vector<int64_t> send_counts,
      std::vector<int64_t> recv_counts, c10::optional<at::Tensor> send_order,
      c10::optional<at::Tensor> recv_order);

  // Non-blocking allreduce (MI355X-first overlap primitive, not in the
  // reference API): returns a wait handle; no autograd through it — use
  // Allreduce for differentiable paths. Gradient bucketing (parallel/ddp)
  // is its main consumer.
  std::vector<at::Tensor> Iallreduce(const at::Tensor& input, int64_t op);
  // Non-blocking equal-count reduce-scatter (no autograd): this rank's
  // flat block of the elementwise sum. input.numel() must be
  // world_size * block; returns a wait handle for the [block] result.
  std::vector<at::Tensor> Ireducescatter(const at::Tensor& input, int64_t op);
  // Non-blocking equal-count flat allgather (no autograd): Wait yields the
  // rank-major concatenation [size * numel]. FSDP prefetch primitive.
  std::vector<at::Tensor> Iallgather(const at::Tensor& input);

  // Non-blocking p2p. Handle contract identical to the reference
  // (csrc/extension.cpp:1094-1107): [meta tensor, comm buffer, input].
  std::vector<at::Tensor> Isend(const at::Tensor& input, int64_t dest,
                                int64_t tag);
  std::vector<at::Tensor> Irecv(const at::Tensor& input, int64_t source,
                                int64_t tag);
  at::Tensor Wait(const std::vector<at::Tensor>& handle);

  // Channel-aware p2p used by the backward pass: adjoint transfers ride a
  // dedicated RCCL communicator/stream instead of the reference's tag+10
  // offset (csrc/extension.cpp:1161).
  std::vector<at::Tensor> IsendImpl(const at::Tensor& input, int64_t dest,
                                    int64_t tag, bool backward_channel);
  std::vector<at::Tensor> IrecvImpl(const at::Tensor& input, int64_t source,
                                    int64_t tag, bool backward_channel);

  const std::string& group_name() const { return group_name_; }

  // internal
  Transport& tr_for(const at::Tensor& t);
  Transport& cpu_tr();
  Transport& gpu_tr(int device);

 private:
  std::string group_name_;
  std::mutex mu_;
  std::shared_ptr<Transport> cpu_tr_;
  std::shared_ptr<Transport> gpu_tr_;
  int gpu_device_ = -1;
};

// JoinDummies free op (reference csrc/extension.cpp:989-1046).
at::Tensor join_dummies(const at::Tensor& loopthrough,
                        const std::vector<at::Tensor>& dummies);

// Debug/test entry points (tests/test_gpu.py): exercise the CDNA4 slab and
// bitwise-reduce kernels directly, without a multi-rank world.
at::Tensor debug_pack_roundtrip(const at::Tensor& input, int64_t axis,
                                std::vector<int64_t> counts);
// launch_slab_copy once over descs, each (src_off, dst_off, before, count,
// after_b, src_pitch_b, dst_pitch_b) in bytes into the flat uint8 tensors
// src and dst. Raises before launching if a descriptor leaves either tensor
// or two destination ranges overlap.
void debug_slab_copy(const at::Tensor& src, const at::Tensor& dst,
                     const std::vector<std::vector<int64_t>>& descs);
at::Tensor debug_bitwise_reduce(const at::Tensor& stacked, int64_t op);
at::Tensor debug_fp8_reduce(const at::Tensor& stacked, int64_t op);
// arith_reduce kernel: own [n] is source `me`, staged [nranks-1, n] holds
// the other ranks in order; op is an MPI_* arithmetic constant.
at::Tensor debug_arith_reduce(const at::Tensor& own, const at::Tensor& staged,
                              int64_t me, int64_t op);
// mxfp8 codec entry points: the torch composite for CPU tensors, the gfx950
// kernels for GPU tensors (tests compare the two byte for byte).
std::tuple<at::Tensor, at::Tensor> debug_mx8_quantize(const at::Tensor& x);
// payload [P, G*32], scales [P, G] -> (payload [G*32], scales [G])
std::tuple<at::Tensor, at::Tensor> debug_mx8_reduce(const at::Tensor& payload,
                                                    const at::Tensor& scales);
at::Tensor debug_mx8_dequantize(const at::Tensor& payload,
                                const at::Tensor& scales, int64_t numel,
                                at::ScalarType dtype,
                                const c10::optional<at::Tensor>& out);
// payload [P, G*32], scales [P, G] -> flat [numel] of dtype: the
// reduce-scatter tail (fp32 rank-order sum, one cast, no requantization)
at::Tensor debug_mx8_reduce_to(const at::Tensor& payload,
                               const at::Tensor& scales, int64_t numel,
                               at::ScalarType dtype,
                               const c10::optional<at::Tensor>& out);
// payload [P, Gb*32], scales [P, Gb], Gb = ceil(rows*row_elems/32) ->
// [rows, P, row_elems] of dtype: the allgather tail (block r dequantized
// into out[:, r, :])
at::Tensor debug_mx8_dequantize_blocks(const at::Tensor& payload,
                                       const at::Tensor& scales, int64_t rows,
                                       int64_t row_elems,
                                       at::ScalarType dtype,
                                       const c10::optional<at::Tensor>& out);
// flat contiguous x of rows*nblocks*row_elems elements seen as
// [rows, nblocks, row_elems] -> (payload [P, Gb*32], scales [P, Gb]): the
// all-to-all head (block p = mx8_quantize of the contiguous x[:, p, :]).
// With payload_out / scales_out (flat uint8) the results alias their heads.
std::tuple<at::Tensor, at::Tensor> debug_mx8_quantize_blocks(
    const at::Tensor& x, int64_t nblocks, int64_t rows, int64_t row_elems,
    const c10::optional<at::Tensor>& payload_out,
    const c10::optional<at::Tensor>& scales_out);
// flat contiguous x seen as [rows, S, after]; segment p = mx8_quantize of the
// contiguous xs[:, displ_p : displ_p + counts[p], :], xs = x gathered through
// `order` along the slice axis if given -> (payload [32*sum G_p], scales
// [sum G_p]): the pairwise all-to-all head. With payload_out / scales_out
// (flat uint8) the results alias their heads.
std::tuple<at::Tensor, at::Tensor> debug_mx8_quantize_segments(
    const at::Tensor& x, int64_t rows, int64_t after,
    std::vector<int64_t> counts, const c10::optional<at::Tensor>& order,
    const c10::optional<at::Tensor>& payload_out,
    const c10::optional<at::Tensor>& scales_out);
// the pairwise all-to-all tail: the segments' streams -> [rows, R, after] of
// dtype, R = sum(counts), received slice i at slice order[i] if an order is
// given. With `out` (flat, of dtype) the result aliases its head and slices
// the order does not name keep their contents.
at::Tensor debug_mx8_dequantize_segments(
    const at::Tensor& payload, const at::Tensor& scales, int64_t rows,
    int64_t after, std::vector<int64_t> counts, at::ScalarType dtype,
    const c10::optional<at::Tensor>& order,
    const c10::optional<at::Tensor>& out);
// staging: flat P rank-major blocks of [rows, row_elems]; out: contiguous
// [rows, P, row_elems]. The axis unpack of an equal-count Allgather.
void debug_unpack_blocks(const at::Tensor& staging, const at::Tensor& out);
// in: contiguous [rows, P, row_elems]; staging: flat P rank-major blocks of
// [rows, row_elems]. The axis pack of an equal-count Reducescatter.
void debug_pack_blocks(const at::Tensor& in, const at::Tensor& staging);
// stacked: [nranks, ..., 2] (value, location) pairs; op: 0=minloc 1=maxloc
at::Tensor debug_pairloc_reduce(const at::Tensor& stacked, int64_t op);

} // namespace m4a
