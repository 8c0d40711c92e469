// Autograd-transparent collectives for mpi4torch_amd.
//
// Every public op follows the skeleton of the reference
// (helmholtz-analytics/mpi4torch, csrc/extension.cpp:274-308):
//   grad_fn setup -> AutoDispatchBelowADInplaceOrView body -> set_history
// with the adjoint table:
//   Allreduce(SUM) <-> Allreduce(SUM)      (ref :254-308)
//   Bcast_ -> Reduce_(SUM, root)           (ref :310-365)
//   Reduce_ -> Bcast_                      (ref :367-464)
//   Gather <-> Scatter                     (ref :466-599, :736-884)
//   Allgather -> ReduceScatter             (ref :601-734; we FIX the known
//                                           wrong-root bug at ref :626-628)
//   Alltoall -> Alltoall (axes swapped)    (ref :886-987)
//   Isend/Irecv -> Wait; Wait -> reverse transfer on the backward channel
//                                          (ref :1048-1265; tag+10 becomes a
//                                           dedicated RCCL communicator)
//
// The communication itself is MI355X-native (csrc/transport.cpp): RCCL over
// xGMI for GPU tensors, gloo for CPU; axis marshaling that the reference did
// with MPI derived datatypes is done by the batched CDNA4 slab-copy kernel
// (csrc/kernels.hip) on the GPU and by strided tensor copies on CPU.

#include "ops.hpp"
#include "transport.hpp"
#include "kernels.hpp"

#include <torch/csrc/autograd/function.h>
#include <torch/csrc/autograd/functions/utils.h>
#include <torch/csrc/autograd/variable.h>
#include <ATen/core/TensorBody.h>
#include <ATen/WrapDimUtils.h>

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <mutex>
#include <tuple>

namespace m4a {

using at::Tensor;
using torch::autograd::Node;
using torch::autograd::variable_list;

// ---------------------------------------------------------------------------
// Communicator
// ---------------------------------------------------------------------------

Communicator::Communicator(std::string group_name)
    : group_name_(std::move(group_name)) {}

int64_t Communicator::GetRank() { return cpu_tr().rank(); }
int64_t Communicator::GetSize() { return cpu_tr().size(); }

Transport& Communicator::cpu_tr() {
  std::lock_guard<std::mutex> g(mu_);
  if (!cpu_tr_) {
    cpu_tr_ = group_name_.empty() ? make_local_transport()
                                  : make_c10d_transport(group_name_);
  }
  return *cpu_tr_;
}

Transport& Communicator::gpu_tr(int device) {
  std::lock_guard<std::mutex> g(mu_);
  if (!gpu_tr_) {
    if (group_name_.empty()) {
      // No distributed context: world of one, local fast paths.
      if (!cpu_tr_) cpu_tr_ = make_local_transport();
      return *cpu_tr_;
    }
    gpu_tr_ = make_rccl_transport(group_name_, device);
    gpu_device_ = device;
  }
  TORCH_CHECK(device == gpu_device_,
              "mpi4torch_amd: one GPU per process (torchrun model); "
              "communicator bound to device ", gpu_device_,
              " but got a tensor on device ", device);
  return *gpu_tr_;
}

Transport& Communicator::tr_for(const Tensor& t) {
  if (t.is_cuda() && !config().force_host_staging) {
    return gpu_tr((int)t.get_device());
  }
  return cpu_tr();
}

namespace {

// Host staging policy: mirrors the reference's MPIDeviceHelper
// (csrc/extension.cpp:61-104). On MI355X the default is the direct
// RCCL/xGMI path; staging exists only as the force_host_staging() debug
// toggle (the analog of deactivate_cuda_aware_mpi_support, ref :54-59).
struct DeviceStager {
  explicit DeviceStager(const Tensor& t)
      : orig_device_(t.device()),
        active_(t.is_cuda() && config().force_host_staging) {}
  Tensor to_comm(const Tensor& t) const {
    return active_ ? t.to(at::kCPU) : t;
  }
  Tensor from_comm(Tensor t) const {
    return active_ ? t.to(orig_device_) : std::move(t);
  }
  at::Device orig_device_;
  bool active_;
};

// --------------------------- axis geometry --------------------------------

struct AxisGeom {
  int64_t before = 1, axis = 0, after = 1, after_b = 0, esize = 0;
};

AxisGeom axis_geom(const Tensor& t, int64_t axis) {
  AxisGeom g;
  auto sizes = t.sizes();
  for (int64_t i = 0; i < axis; ++i) g.before *= sizes[i];
  g.axis = sizes[axis];
  for (int64_t i = axis + 1; i < (int64_t)sizes.size(); ++i)
    g.after *= sizes[i];
  g.esize = t.element_size();
  g.after_b = g.after * g.esize;
  return g;
}

hipStream_t current_gpu_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA((int)t.get_device())
      .stream();
}

// Copy slices of `full` along `axis` (at displs/counts) into flat contiguous
// `blocks` (pack=true) or back (pack=false). GPU: one batched CDNA4 slab
// kernel launch on the current stream; CPU: strided tensor copies. This is
// the MI355X-native replacement for MPI_Type_vector marshaling (reference
// csrc/extension.cpp:556-577). The optional [row_lo, row_hi) range limits
// the copy to a slice of the `before` dimension — one phase of the
// pipelined (chunked) exchange; defaults cover all rows.
void move_axis_blocks(const Tensor& full, int64_t axis,
                      const std::vector<int64_t>& displs,
                      const std::vector<int64_t>& counts,
                      std::vector<Tensor>& blocks, bool pack,
                      int64_t row_lo = 0, int64_t row_hi = -1) {
  const auto g = axis_geom(full, axis);
  if (row_hi < 0) row_hi = g.before;
  const int64_t rows = row_hi - row_lo;
  if (rows <= 0) return;
  if (full.is_cuda()) {
    std::vector<SlabDesc> descs;
    descs.reserve(counts.size());
    char* base = static_cast<char*>(full.data_ptr());
    for (size_t i = 0; i < counts.size(); ++i) {
      if (counts[i] == 0 || g.before * g.after == 0) continue;
      char* bp = static_cast<char*>(blocks[i].data_ptr());
      SlabDesc d;
      d.before = rows;
      d.count = counts[i];
      d.after_b = g.after_b;
      if (pack) {
        d.src = base + displs[i] * g.after_b + row_lo * g.axis * g.after_b;
        d.src_pitch_b = g.axis * g.after_b;
        d.dst = bp + row_lo * counts[i] * g.after_b;
        d.dst_pitch_b = counts[i] * g.after_b;
      } else {
        d.src = bp + row_lo * counts[i] * g.after_b;
        d.src_pitch_b = counts[i] * g.after_b;
        d.dst = base + displs[i] * g.after_b + row_lo * g.axis * g.after_b;
        d.dst_pitch_b = g.axis * g.after_b;
      }
      descs.push_back(d);
    }
    if (!descs.empty()) {
      launch_slab_copy(descs.data(), (int)descs.size(),
                       current_gpu_stream(full));
    }
  } else {
    if (g.before * g.after == 0) return;
    auto f3 = full.view({g.before, g.axis, g.after})
                  .narrow(0, row_lo, rows);
    for (size_t i = 0; i < counts.size(); ++i) {
      if (counts[i] == 0) continue;
      auto b3 = blocks[i].view({g.before, counts[i], g.after})
                    .narrow(0, row_lo, rows);
      if (pack) {
        b3.copy_(f3.narrow(1, displs[i], counts[i]));
      } else {
        f3.narrow(1, displs[i], counts[i]).copy_(b3);
      }
    }
  }
}

// NOTE on the count exchanges below: a "static shapes" cache keyed by a
// rank's OWN contribution was tried and removed — own-value repetition
// does not imply the other ranks repeat, so a partial cache hit splits
// the gloo exchange and deadlocks. The ~0.1 ms host round-trip per axis
// collective stays; it is off the critical path for multi-megabyte
// payloads.

// Contiguous copy through the nontemporal CDNA4 slab kernel: measured
// ~3-5% faster than at::clone for large tensors (L2-bypassing streams) and
// keeps the world-of-one identity paths on the native kernels.
Tensor fast_clone(const Tensor& in) {
  if (!in.is_cuda() || in.numel() == 0) return in.clone();
  auto out = at::empty_like(in);
  SlabDesc d;
  d.src = in.data_ptr();
  d.dst = out.data_ptr();
  d.before = 1;
  d.count = 1;
  d.after_b = in.numel() * in.element_size();
  d.src_pitch_b = d.after_b;
  d.dst_pitch_b = d.after_b;
  launch_slab_copy(&d, 1, current_gpu_stream(in));
  return out;
}

std::vector<int64_t> prefix_displs(const std::vector<int64_t>& counts) {
  std::vector<int64_t> d(counts.size(), 0);
  for (size_t i = 1; i < counts.size(); ++i) d[i] = d[i - 1] + counts[i - 1];
  return d;
}

// Phase count for the chunked pack->wire pipelining. MUST be computed
// from rank-shared quantities only (global logical payload), so every
// rank slices every pair block at identical offsets. Graph capture
// forces one phase (iexchange+wait cannot be captured).
int64_t phase_count(const Tensor& t, int64_t per_rank_bytes) {
  const int64_t c = config().pipeline_chunk_bytes;
  if (c <= 0) return 1;
  if (t.is_cuda()) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(current_gpu_stream(t), &st);
    if (st != hipStreamCaptureStatusNone) return 1;
  }
  return std::min<int64_t>(
      4, std::max<int64_t>(1, (per_rank_bytes + c - 1) / c));
}

// Phased exchange for the funnel collectives (Gather/Scatter/Allgather):
// every pair block shares the SAME row count (the common `before` of the
// marshaled layout); per-pair row lengths come in elements. pack_phase /
// unpack_phase (either may be null) marshal one [row_lo, row_hi) slice;
// each phase is one full-width grouped iexchange, so marshaling overlaps
// the previous phase's wire time.
void phased_funnel_exchange(
    Transport& tr, int64_t K, int64_t rows,
    const std::vector<Tensor>& sblocks, const std::vector<int>& speers,
    const std::vector<int64_t>& srowe, std::vector<Tensor>& rblocks,
    const std::vector<int>& rpeers, const std::vector<int64_t>& rrowe,
    const std::function<void(int64_t, int64_t)>& pack_phase,
    const std::function<void(int64_t, int64_t)>& unpack_phase) {
  auto bound = [&](int64_t k) { return rows * k / K; };
  auto slice = [](const Tensor& blk, int64_t lo, int64_t len) {
    auto flat = blk.view({-1});
    return len > 0 ? flat.narrow(0, lo, len) : flat.narrow(0, 0, 0);
  };
  std::vector<uint64_t> reqs((size_t)K);
  for (int64_t k = 0; k < K; ++k) {
    const int64_t b0 = bound(k), b1 = bound(k + 1);
    if (pack_phase) pack_phase(b0, b1);
    std::vector<Tensor> sk(sblocks.size()), rk(rblocks.size());
    for (size_t i = 0; i < sblocks.size(); ++i) {
      sk[i] = slice(sblocks[i], b0 * srowe[i], (b1 - b0) * srowe[i]);
    }
    for (size_t j = 0; j < rblocks.size(); ++j) {
      rk[j] = slice(rblocks[j], b0 * rrowe[j], (b1 - b0) * rrowe[j]);
    }
    reqs[(size_t)k] = tr.iexchange(sk, speers, rk, rpeers);
  }
  for (int64_t k = 0; k < K; ++k) {
    wait_request(reqs[(size_t)k]);
    if (unpack_phase) unpack_phase(bound(k), bound(k + 1));
  }
}

// ------------------------- reduction lowering -----------------------------

bool is_logical(int64_t op) { return op == kLAnd || op == kLOr || op == kLXor; }
bool is_bitwise(int64_t op) { return op == kBAnd || op == kBOr || op == kBXor; }
bool is_arith(int64_t op) {
  return op == kSum || op == kProd || op == kMin || op == kMax;
}

// Collective-desync detector (config().debug_collectives): compare a
// signature of this collective across all ranks over the host channel and
// fail with a description instead of deadlocking in RCCL/gloo.
struct SigHash {
  size_t h;
  explicit SigHash(const char* opname) : h(std::hash<std::string>()(opname)) {}
  void mix(int64_t v) {
    h ^= std::hash<int64_t>()(v) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
  }
};

void debug_compare_sig(const std::string& group, const char* opname,
                       SigHash& sig) {
  auto all =
      host_allgather_int64(group, (int64_t)(sig.h & 0x7fffffffffffffffll));
  for (size_t r = 1; r < all.size(); ++r) {
    TORCH_CHECK(all[r] == all[0],
                "mpi4torch_amd[debug]: collective desync detected at ", opname,
                " — rank ", r, " issued a different op/shape/dtype/arguments "
                "than rank 0. This would deadlock without "
                "MPI4TORCH_AMD_DEBUG=1.");
  }
}

// Full-shape variant: every dimension must agree across ranks
// (elementwise collectives: Allreduce, Bcast_, Reduce_, Reducescatter).
void debug_check_collective(const std::string& group, const char* opname,
                            const at::Tensor& t,
                            std::initializer_list<int64_t> args) {
  if (!config().debug_collectives || group.empty()) return;
  SigHash sig(opname);
  sig.mix((int64_t)t.scalar_type());
  for (auto s : t.sizes()) sig.mix(s);
  for (auto a : args) sig.mix(a);
  debug_compare_sig(group, opname, sig);
}

// Axis-collective variant: per-rank sizes along the listed axes
// legitimately differ (variable counts), so the signature covers dtype,
// ndim, every OTHER dimension, and the op arguments.
void debug_check_axis_collective(const std::string& group, const char* opname,
                                 const at::Tensor& t,
                                 std::initializer_list<int64_t> axes,
                                 std::initializer_list<int64_t> args) {
  if (!config().debug_collectives || group.empty()) return;
  SigHash sig(opname);
  sig.mix((int64_t)t.scalar_type());
  sig.mix(t.dim());
  for (int64_t i = 0; i < t.dim(); ++i) {
    bool skip = false;
    for (auto a : axes) skip = skip || a == i;
    sig.mix(skip ? -1 : t.size(i));
  }
  for (auto a : args) sig.mix(a);
  debug_compare_sig(group, opname, sig);
}

// Dtype-only variant: shapes are rank-local by contract (Scatter's
// non-root inputs are placeholders whose only binding property is the
// dtype the output is allocated with).
void debug_check_dtype_collective(const std::string& group,
                                  const char* opname, at::ScalarType dtype,
                                  std::initializer_list<int64_t> args) {
  if (!config().debug_collectives || group.empty()) return;
  SigHash sig(opname);
  sig.mix((int64_t)dtype);
  for (auto a : args) sig.mix(a);
  debug_compare_sig(group, opname, sig);
}

void check_op(int64_t op) {
  TORCH_CHECK(op >= kMax && op <= kMaxLoc, "invalid reduction op ", op);
}

bool is_pairloc(int64_t op) { return op == kMinLoc || op == kMaxLoc; }

bool native_reduce_dtype(const Transport& tr, at::ScalarType t) {
  if (tr.is_gpu()) {
    switch (t) {
      case at::kByte:
      case at::kChar:
      case at::kInt:
      case at::kLong:
      case at::kHalf:
      case at::kFloat:
      case at::kDouble:
      case at::kBFloat16:
        return true;
      case at::kFloat8_e4m3fn:
      case at::kFloat8_e5m2: {
        // Default: the hierarchical block exchange + fp32-accumulating
        // CDNA4 kernel (one quantization, ~numel staging). Opt into
        // RCCL-native fp8 rings with MPI4TORCH_AMD_NATIVE_FP8=1
        // (runtime-probed).
        static const bool want_native = []() {
          const char* e = std::getenv("MPI4TORCH_AMD_NATIVE_FP8");
          return e && e[0] == '1';
        }();
        return want_native &&
               const_cast<Transport&>(tr).fp8_reduce_supported(t);
      }
      default:
        return false;  // short/bool go through the upcast path
    }
  }
  // gloo (like RCCL) has no int16: kShort takes the int32 upcast path
  switch (t) {
    case at::kByte:
    case at::kChar:
    case at::kInt:
    case at::kLong:
    case at::kHalf:
    case at::kFloat:
    case at::kDouble:
    case at::kBFloat16:
      return true;
    default:
      return false;
  }
}

at::ScalarType upcast_for_reduce(at::ScalarType t) {
  switch (t) {
    case at::kBool: return at::kByte;
    case at::kShort: return at::kInt;
    case at::kFloat8_e4m3fn:
    case at::kFloat8_e5m2:
      return at::kFloat;
    default:
      TORCH_CHECK(false, "mpi4torch_amd: dtype ", t,
                  " not supported for reductions");
  }
}

// Elementwise allreduce with full op/dtype lowering. `in` contiguous.
bool w1_shortcut(const Transport& tr) {
  return tr.size() == 1 && !config().force_full_path;
}

std::vector<int> iota_peers_fwd(int n) {
  std::vector<int> p(n);
  for (int i = 0; i < n; ++i) p[i] = i;
  return p;
}

// Hierarchical GPU allreduce for ops RCCL cannot reduce on the wire
// (bitwise, fp8, minloc/maxloc): partition the flat tensor into P
// near-equal contiguous blocks (aligned to `unit` elements), exchange each
// rank's copy of block j to rank j in ONE grouped p2p launch, locally
// reduce the P copies of the owned block with the fused CDNA4 kernel, then
// allgather the reduced blocks (in place). Versus the round-1 design
// (allgather everything + local reduce) this caps staging at ~numel
// instead of P*numel and wire bytes at 2*(P-1)/P*numel instead of
// (P-1)*numel, while keeping the single-reduction property (each element
// is combined exactly once, fp8 quantized exactly once).
template <typename LocalReduce>
Tensor hierarchical_allreduce(Transport& tr, const Tensor& in, int64_t unit,
                              LocalReduce local_reduce) {
  const int P = tr.size();
  const int me = tr.rank();
  const int64_t N = in.numel();
  const int64_t nunits = N / unit;
  std::vector<int64_t> counts(P);
  for (int p = 0; p < P; ++p) {
    counts[p] = (nunits / P + (p < nunits % P ? 1 : 0)) * unit;
  }
  auto displs = prefix_displs(counts);
  auto flat = in.view({-1});
  auto out = at::empty_like(in);
  auto out_flat = out.view({-1});
  auto nz_narrow = [](const Tensor& t, int64_t off, int64_t len) {
    return len > 0 ? t.narrow(0, off, len) : t.narrow(0, 0, 0);
  };
  // phase 1: block exchange — my copy of block j goes to rank j
  auto staging = at::empty({(int64_t)P * counts[me]}, in.options());
  std::vector<Tensor> sends(P), recvs(P);
  for (int p = 0; p < P; ++p) {
    sends[p] = nz_narrow(flat, displs[p], counts[p]);
    recvs[p] = nz_narrow(staging, (int64_t)p * counts[me], counts[me]);
  }
  auto peers = iota_peers_fwd(P);
  tr.exchange(sends, peers, recvs, peers);
  // phase 2: fused local reduction of the P copies of the owned block
  auto myblock = nz_narrow(out_flat, displs[me], counts[me]);
  if (counts[me] > 0) local_reduce(staging, myblock, counts[me], P);
  // phase 3: allgather the reduced blocks. Equal counts on GPU: one RCCL
  // allgather, in place (myblock aliases out_flat at the rank-major
  // offset — the NCCL in-place convention). Unequal counts, or the CPU
  // test mode (gloo's allgather does not define input/output aliasing):
  // grouped p2p.
  if (nunits % P == 0 && tr.is_gpu()) {
    tr.allgather_equal(myblock, out_flat);
  } else {
    std::vector<Tensor> s2, r2;
    std::vector<int> sp, rp;
    for (int p = 0; p < P; ++p) {
      if (p == me) continue;
      if (counts[me] > 0) {
        s2.push_back(myblock);
        sp.push_back(p);
      }
      if (counts[p] > 0) {
        r2.push_back(out_flat.narrow(0, displs[p], counts[p]));
        rp.push_back(p);
      }
    }
    tr.exchange(s2, sp, r2, rp);
  }
  return out;
}

bool arith_float_dtype(at::ScalarType t) {
  return t == at::kFloat || t == at::kBFloat16 || t == at::kHalf;
}

int arith_dtype_code(at::ScalarType t) {
  return t == at::kFloat ? 0 : (t == at::kBFloat16 ? 1 : 2);
}

int arith_op_code(int64_t op) {
  return op == kSum ? 0 : (op == kProd ? 1 : (op == kMin ? 2 : 3));
}

// Torch-composite local reduce with the kernel's semantics (fp32
// accumulation in rank order, one rounding): the CPU path of
// native_allreduce. MIN/MAX inputs are NaN-free by contract — the kernel
// follows fminf/fmaxf, at::minimum/maximum propagate NaN.
Tensor arith_local_reduce(const std::vector<Tensor>& srcs, int kop,
                          at::ScalarType out_dtype) {
  auto acc = srcs[0].to(at::kFloat);
  for (size_t r = 1; r < srcs.size(); ++r) {
    auto v = srcs[r].to(at::kFloat);
    if (kop == 0) acc = acc + v;
    else if (kop == 1) acc = acc * v;
    else if (kop == 2) acc = at::minimum(acc, v);
    else acc = at::maximum(acc, v);
  }
  return acc.to(out_dtype);
}

// Two-shot allreduce on the framework's own reduce kernel: the same three
// phases as hierarchical_allreduce (block exchange, local reduce of the
// owned block, allgather), minus the work the result does not need:
//   * the rank's own block is never copied into staging — staging holds
//     P-1 slots, the grouped exchange carries no self pair, and the kernel
//     reads the own block straight from the input;
//   * at P == 1 there is no exchange, no staging and no allgather: the whole
//     operation is one kernel launch, in -> out, on the caller's current
//     stream (where every local reduce runs anyway), with no side-stream
//     hop and no event pair because there is no wire phase. That launch is
//     a typeless bit copy, so at P == 1 any dtype may come here.
// Blocks are multiples of 16 bytes so every block start stays
// vector-aligned; the last block takes the remainder.
Tensor native_allreduce(Transport& tr, const Tensor& in, int64_t op) {
  const int P = tr.size();
  const int me = tr.rank();
  const int64_t N = in.numel();
  auto out = at::empty_like(in);
  if (P == 1) {
    if (in.is_cuda()) {
      launch_arith_copy(in.data_ptr(), out.data_ptr(),
                        N * (int64_t)in.element_size(),
                        current_gpu_stream(in));
    } else {
      out.copy_(in);
    }
    return out;
  }
  TORCH_CHECK(arith_float_dtype(in.scalar_type()) && is_arith(op),
              "native_allreduce reduces bf16/fp16/fp32 with sum/prod/min/max");
  const int kop = arith_op_code(op);
  const int64_t unit = 16 / (int64_t)in.element_size();
  const int64_t nunits = N / unit;
  std::vector<int64_t> counts(P);
  for (int p = 0; p < P; ++p) {
    counts[p] = (nunits / P + (p < nunits % P ? 1 : 0)) * unit;
  }
  counts[P - 1] += N - nunits * unit;
  auto displs = prefix_displs(counts);
  auto flat = in.view({-1});
  auto out_flat = out.view({-1});
  const int64_t mine = counts[me];
  // slot stride rounded up to the vector so every slot starts aligned even
  // when the owned block carries the remainder
  const int64_t slot = (mine + unit - 1) / unit * unit;
  // phase 1: my copy of block j goes to rank j (j != me); the P-1 peer
  // copies of my block land in staging, rank order with me skipped
  auto staging = at::empty({(int64_t)(P - 1) * slot}, in.options());
  {
    std::vector<Tensor> sends, recvs;
    std::vector<int> speers, rpeers;
    for (int p = 0; p < P; ++p) {
      if (p == me) continue;
      if (counts[p] > 0) {
        sends.push_back(flat.narrow(0, displs[p], counts[p]));
        speers.push_back(p);
      }
      if (mine > 0) {
        recvs.push_back(
            staging.narrow(0, (int64_t)(p - (p > me ? 1 : 0)) * slot, mine));
        rpeers.push_back(p);
      }
    }
    tr.exchange(sends, speers, recvs, rpeers);
  }
  // phase 2: reduce own block + P-1 staged copies into out's block
  if (mine > 0) {
    auto own = flat.narrow(0, displs[me], mine);
    auto myblock = out_flat.narrow(0, displs[me], mine);
    if (in.is_cuda()) {
      launch_arith_reduce(own.data_ptr(), staging.data_ptr(), slot, P, me,
                          myblock.data_ptr(), mine, kop,
                          arith_dtype_code(in.scalar_type()),
                          current_gpu_stream(in));
    } else {
      std::vector<Tensor> srcs;
      for (int r = 0; r < P; ++r) {
        srcs.push_back(r == me ? own
                               : staging.narrow(
                                     0, (int64_t)(r - (r > me ? 1 : 0)) * slot,
                                     mine));
      }
      myblock.copy_(arith_local_reduce(srcs, kop, in.scalar_type()));
    }
  }
  // phase 3: allgather the reduced blocks — one in-place RCCL allgather
  // when the blocks are equal, grouped p2p otherwise and on gloo (whose
  // allgather does not define input/output aliasing)
  if (N % (unit * P) == 0 && tr.is_gpu()) {
    auto myblock = out_flat.narrow(0, displs[me], mine);
    tr.allgather_equal(myblock, out_flat);
  } else {
    std::vector<Tensor> s2, r2;
    std::vector<int> sp, rp;
    for (int p = 0; p < P; ++p) {
      if (p == me) continue;
      if (mine > 0) {
        s2.push_back(out_flat.narrow(0, displs[me], mine));
        sp.push_back(p);
      }
      if (counts[p] > 0) {
        r2.push_back(out_flat.narrow(0, displs[p], counts[p]));
        rp.push_back(p);
      }
    }
    tr.exchange(s2, sp, r2, rp);
  }
  return out;
}

// Engine selection for the dtypes the transport's allreduce can carry
// (Config::allreduce_engine, MPI4TORCH_AMD_ALLREDUCE).
bool use_native_allreduce(const Transport& tr, at::ScalarType t, int64_t op) {
  switch (config().allreduce_engine) {
    case Config::kAllreduceRccl:
      return false;
    case Config::kAllreduceNative:
      return arith_float_dtype(t) && is_arith(op);
    default:
      // a world of one only gets here under force_full_path on the GPU
      return tr.size() == 1 && tr.is_gpu();
  }
}

Tensor transport_or_native_allreduce(Transport& tr, const Tensor& in,
                                     int64_t op) {
  if (use_native_allreduce(tr, in.scalar_type(), op)) {
    return native_allreduce(tr, in, op);
  }
  auto out = at::empty_like(in);
  tr.allreduce(in, out, (RedOp)op);
  return out;
}

int pairloc_dtype_code(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return 0;
    case at::kDouble: return 1;
    case at::kHalf: return 2;
    case at::kBFloat16: return 3;
    case at::kChar: return 4;
    case at::kByte: return 5;
    case at::kShort: return 6;
    case at::kInt: return 7;
    case at::kLong: return 8;
    default:
      TORCH_CHECK(false, "mpi4torch_amd: MPI_MINLOC/MAXLOC unsupported for "
                  "dtype ", t);
  }
}

// Torch-composite pair arg-reduce over stk [n_chunks, n_pairs, 2]: the CPU
// path, same rule as the CDNA4 kernel (csrc/kernels.hpp). min/max propagate
// NaN, so a NaN value wins and the NaN entries are the ones whose locations
// compete. Integral locations stay int64: a double cannot tell neighbours
// above 2^53 apart.
Tensor pairloc_local_reduce(const Tensor& stk, int64_t kop,
                            at::ScalarType out_dtype) {
  auto vals = stk.select(2, 0);
  const bool fl = at::isFloatingType(vals.scalar_type());
  auto locs = stk.select(2, 1).to(fl ? at::kDouble : at::kLong);
  Tensor bestv =
      kop == 0 ? std::get<0>(vals.min(0)) : std::get<0>(vals.max(0));
  auto mask = vals.eq(bestv.unsqueeze(0));
  if (fl) {
    mask = mask.logical_or(
        vals.isnan().logical_and(bestv.isnan().unsqueeze(0)));
  }
  const at::Scalar never =
      fl ? at::Scalar(std::numeric_limits<double>::infinity())
         : at::Scalar(std::numeric_limits<int64_t>::max());
  auto masked = locs.masked_fill(mask.logical_not(), never);
  auto bestl = std::get<0>(masked.min(0)).to(out_dtype);
  return at::stack({bestv, bestl}, -1);
}

// MINLOC/MAXLOC (reference op table csrc/extension.cpp:204-252): tensors
// are (value, location) pairs along the LAST axis (size 2), the tensor
// analog of MPI's pair types (MPI_DOUBLE_INT etc.). Result per pair: the
// extreme value across ranks and its location, ties -> smallest location.
Tensor pairloc_lowered(Transport& tr, const Tensor& in, int64_t op) {
  const int kop = op == kMinLoc ? 0 : 1;
  const int P = tr.size();
  const int dt = pairloc_dtype_code(in.scalar_type());  // dtype validation
  if (tr.is_gpu() || config().force_hierarchical) {
    return hierarchical_allreduce(
        tr, in, /*unit=*/2,
        [&](const Tensor& stg, Tensor& blk, int64_t n, int nr) {
          if (blk.is_cuda()) {
            launch_pairloc_reduce(stg.data_ptr(), blk.data_ptr(), n / 2,
                                  nr, kop, dt, current_gpu_stream(in));
          } else {
            blk.copy_(pairloc_local_reduce(stg.view({nr, -1, 2}), kop,
                                           in.scalar_type())
                          .view({-1}));
          }
        });
  }
  // CPU: allgather + torch composite arg-reduce
  auto staging = at::empty({(int64_t)P * in.numel()}, in.options());
  tr.allgather_equal(in, staging);
  return pairloc_local_reduce(staging.view({P, -1, 2}), kop,
                              in.scalar_type())
      .view(in.sizes())
      .contiguous();
}

Tensor allreduce_lowered(Transport& tr, const Tensor& in, int64_t op) {
  if (in.numel() == 0) return in.clone();
  if (tr.size() == 1) {
    // force_full_path exercises the real machinery even alone:
    // native_allreduce for arithmetic ops (one pass of the framework's own
    // reduce kernel; MPI4TORCH_AMD_ALLREDUCE=rccl puts the degenerate
    // ncclAllReduce back), the hierarchical exchange+kernel path
    // for bitwise/fp8/pairloc (P=1 self-exchange -> kernel -> in-place
    // allgather). Everything else short-circuits to a device clone.
    const bool fp8_in = in.scalar_type() == at::kFloat8_e4m3fn ||
                        in.scalar_type() == at::kFloat8_e5m2;
    const bool full =
        config().force_full_path && tr.is_gpu() &&
        (is_bitwise(op) || is_pairloc(op) ||
         (is_arith(op) &&
          (native_reduce_dtype(tr, in.scalar_type()) || fp8_in)));
    if (!full) return fast_clone(in);
  }
  if (is_pairloc(op)) {
    return pairloc_lowered(tr, in, op);
  }
  if (is_logical(op)) {
    // land/lor/lxor lower to min/max/sum over 0/1 indicators; valid on any
    // dtype and on both transports (RCCL has no logical ops).
    auto ind = in.ne(0).to(at::kByte);
    auto red = transport_or_native_allreduce(
        tr, ind, op == kLAnd ? kMin : (op == kLOr ? kMax : kSum));
    if (op == kLXor) red = red.bitwise_and_(1);
    return red.ne(0).to(in.scalar_type());
  }
  if (is_bitwise(op)) {
    TORCH_CHECK(at::isIntegralType(in.scalar_type(), /*includeBool=*/true),
                "mpi4torch_amd: ", red_op_name(op),
                " requires an integral tensor");
    if (!tr.is_gpu() && !config().force_hierarchical) {
      auto out = at::empty_like(in);
      tr.allreduce(in, out, (RedOp)op);
      return out;
    }
    // RCCL has no bitwise reductions: hierarchical exchange + local CDNA4
    // reduce kernel (staging ~numel, not P*numel).
    const int kop = op == kBAnd ? 0 : (op == kBOr ? 1 : 2);
    const int64_t esize = in.element_size();
    return hierarchical_allreduce(
        tr, in, /*unit=*/1,
        [&](const Tensor& stg, Tensor& blk, int64_t n, int nr) {
          if (blk.is_cuda()) {
            launch_bitwise_reduce(stg.data_ptr(), blk.data_ptr(), n * esize,
                                  nr, kop, current_gpu_stream(in));
            return;
          }
          auto v = stg.view({nr, n});
          auto acc = v[0].clone();
          for (int64_t r = 1; r < nr; ++r) {
            if (kop == 0) acc.bitwise_and_(v[r]);
            else if (kop == 1) acc.bitwise_or_(v[r]);
            else acc.bitwise_xor_(v[r]);
          }
          blk.copy_(acc);
        });
  }
  TORCH_CHECK(is_arith(op));
  if (native_reduce_dtype(tr, in.scalar_type())) {
    return transport_or_native_allreduce(tr, in, op);
  }
  const bool fp8 = in.scalar_type() == at::kFloat8_e4m3fn ||
                   in.scalar_type() == at::kFloat8_e5m2;
  if (fp8 && (tr.is_gpu() || config().force_hierarchical)) {
    // fp8 stays fp8 on the wire: hierarchical block exchange + one fused
    // CDNA4 reduction per element with fp32 accumulators and a single
    // quantization (better numerics than a per-hop-quantizing ring, 4x
    // fewer wire bytes per hop than the fp32-upcast path, and — unlike
    // the round-1 full allgather — staging stays ~numel at any P).
    const int kop = op == kSum ? 0 : (op == kProd ? 1 : (op == kMin ? 2 : 3));
    const bool e5m2 = in.scalar_type() == at::kFloat8_e5m2;
    return hierarchical_allreduce(
        tr, in, /*unit=*/1,
        [&](const Tensor& stg, Tensor& blk, int64_t n, int nr) {
          if (blk.is_cuda()) {
            launch_fp8_reduce(stg.data_ptr(), blk.data_ptr(), n, nr, kop,
                              e5m2, current_gpu_stream(in));
            return;
          }
          auto v = stg.view({nr, n}).to(at::kFloat);
          auto acc = v[0];
          for (int64_t r = 1; r < nr; ++r) {
            if (kop == 0) acc = acc + v[r];
            else if (kop == 1) acc = acc * v[r];
            else if (kop == 2) acc = at::minimum(acc, v[r]);
            else acc = at::maximum(acc, v[r]);
          }
          blk.copy_(acc.to(in.scalar_type()));
        });
  }
  auto up = in.to(upcast_for_reduce(in.scalar_type()));
  return transport_or_native_allreduce(tr, up, op).to(in.scalar_type());
}

// ----------------------- mxfp8 compressed allreduce -----------------------
//
// Codec (normative; the gfx950 kernels in csrc/mx8_kernels.hip match this
// torch composite byte for byte): groups of 32 consecutive elements of the
// flat tensor, each 32 OCP e4m3fn payload bytes + one E8M0 scale byte.
//   quantize : amax over |x| in fp32. Non-finite group -> scale 255, zero
//              payload. amax == 0 -> E = 0. Else amax = m*2^k (frexp,
//              m in [0.5,1)): E = k-9 if m <= 0.875 else k-8, clamped to
//              [-127,127] — the smallest E with amax*2^-E <= 448. Scale
//              byte E+127; payload = RNE(x * 2^-E) (exact scaling, never
//              saturates).
//   dequant  : fp32(byte) * 2^E (exact); scale 255 -> NaN group.
//   reduce   : ((d_0 + d_1) + ...) in fp32 in rank order on dequantized
//              values, then quantize. A 255 input or non-finite sum gives a
//              255 group (NaN propagation does this in the composite).

// 2^e as fp32 for int32 e in [-127,127], built from bits (2^-127 is the
// subnormal 0x00400000) so no transcendental is involved.
Tensor mx8_pow2(const Tensor& e) {
  auto bits = at::where(e.ge(-126), (e + 127) * (1 << 23),
                        at::full_like(e, 0x00400000));
  return bits.to(at::kInt).contiguous().view(at::kFloat);
}

// xg: [G, 32] fp32 -> (payload [G, 32] u8, scales [G] u8)
std::pair<Tensor, Tensor> mx8_quantize_groups(const Tensor& xg) {
  auto finite = at::isfinite(xg).all(1);
  auto amax = xg.abs().amax(1).masked_fill(finite.logical_not(), 0);
  auto mk = at::frexp(amax);
  auto m = std::get<0>(mk);
  auto k = std::get<1>(mk).to(at::kInt);
  auto E = k - at::where(m.le(0.875), at::full_like(k, 9), at::full_like(k, 8));
  E = at::where(amax.eq(0), at::zeros_like(E), E).clamp(-127, 127);
  auto scaled = xg * mx8_pow2(-E).unsqueeze(1);
  auto pay = scaled.to(at::kFloat8_e4m3fn).view(at::kByte);
  pay = at::where(finite.unsqueeze(1), pay, at::zeros_like(pay));
  auto sc = at::where(finite, E + 127, at::full_like(E, 255)).to(at::kByte);
  return {pay.contiguous(), sc.contiguous()};
}

// payload [G, 32] u8, scales [G] u8 -> [G, 32] fp32
Tensor mx8_dequantize_groups(const Tensor& pay, const Tensor& sc) {
  auto v = pay.contiguous().view(at::kFloat8_e4m3fn).to(at::kFloat);
  auto E = (sc.to(at::kInt) - 127).clamp(-127, 127);
  auto d = v * mx8_pow2(E).unsqueeze(1);
  return at::where(sc.eq(255).unsqueeze(1),
                   at::full_like(d, std::numeric_limits<float>::quiet_NaN()),
                   d);
}

// The dtype code of kernels.hpp; `who` names the caller in the message.
int mx8_dtype_code(at::ScalarType t, const char* who = "mxfp8 compression") {
  switch (t) {
    case at::kFloat: return 0;
    case at::kBFloat16: return 1;
    case at::kHalf: return 2;
    default:
      TORCH_CHECK(false, "mpi4torch_amd: ", who, " supports float32, "
                  "bfloat16 and float16 tensors, got ", t);
  }
}

// The codec functions below take optional outputs: a caller's contiguous
// buffer of the result's shape (or longer, where noted) is written in place
// and returned; without one the result is allocated.
Tensor out_or_empty(const c10::optional<Tensor>& out, at::IntArrayRef sizes,
                    const at::TensorOptions& opts) {
  return out.has_value() ? *out : at::empty(sizes, opts);
}

// flat contiguous x -> (payload [G*32] u8, scales [G] u8), G = ceil(N/32)
std::pair<Tensor, Tensor> mx8_quantize(
    const Tensor& x, const c10::optional<Tensor>& payload_out = c10::nullopt,
    const c10::optional<Tensor>& scales_out = c10::nullopt) {
  const int dt = mx8_dtype_code(x.scalar_type());
  const int64_t N = x.numel();
  const int64_t G = (N + 31) / 32;
  auto bopts = x.options().dtype(at::kByte);
  auto pay = out_or_empty(payload_out, {G * 32}, bopts);
  auto sc = out_or_empty(scales_out, {G}, bopts);
  if (x.is_cuda()) {
    launch_mx8_quantize(x.data_ptr(), pay.data_ptr(), sc.data_ptr(), N, dt,
                        current_gpu_stream(x));
    return {pay, sc};
  }
  auto padded = at::zeros({G * 32}, x.options().dtype(at::kFloat));
  padded.narrow(0, 0, N).copy_(x.view({-1}));
  auto ps = mx8_quantize_groups(padded.view({G, 32}));
  if (!payload_out.has_value()) return {ps.first.view({-1}), ps.second};
  pay.copy_(ps.first.view({-1}));
  sc.copy_(ps.second);
  return {pay, sc};
}

// The CPU composites' sum: P copies, pin [P * n*32], sin [P * n] -> [n, 32]
// fp32, ((d_0 + d_1) + ...) in rank order on dequantized values.
Tensor mx8_sum_copies(const Tensor& pin, const Tensor& sin, int64_t n, int P) {
  auto pv = pin.view({P, n, 32});
  auto sv = sin.view({P, n});
  auto acc = mx8_dequantize_groups(pv[0], sv[0]);
  for (int r = 1; r < P; ++r) {
    acc = acc + mx8_dequantize_groups(pv[r], sv[r]);
  }
  return acc;
}

// P copies: pin [P * n*32], sin [P * n] -> pout [n*32], sout [n] (views ok)
void mx8_reduce(const Tensor& pin, const Tensor& sin, Tensor& pout,
                Tensor& sout, int64_t n, int P) {
  if (n == 0) return;
  if (pin.is_cuda()) {
    launch_mx8_reduce(pin.data_ptr(), sin.data_ptr(), pout.data_ptr(),
                      sout.data_ptr(), n, P, current_gpu_stream(pin));
    return;
  }
  auto ps = mx8_quantize_groups(mx8_sum_copies(pin, sin, n, P));
  pout.copy_(ps.first.view({-1}));
  sout.copy_(ps.second);
}

// payload [G*32], scales [G] -> flat [numel] of `dtype`
Tensor mx8_dequantize(const Tensor& pay, const Tensor& sc, int64_t numel,
                      at::ScalarType dtype,
                      const c10::optional<Tensor>& out_opt = c10::nullopt) {
  const int dt = mx8_dtype_code(dtype);
  if (pay.is_cuda()) {
    auto out = out_or_empty(out_opt, {numel}, pay.options().dtype(dtype));
    launch_mx8_dequantize(pay.data_ptr(), sc.data_ptr(), out.data_ptr(),
                          numel, dt, current_gpu_stream(pay));
    return out;
  }
  const int64_t G = sc.numel();
  auto d = mx8_dequantize_groups(pay.view({G, 32}), sc).view({-1});
  auto res = d.narrow(0, 0, numel).to(dtype);
  return out_opt.has_value() ? out_opt->copy_(res) : res;
}

// P copies: pin [P * G*32], sin [P * G], G = ceil(numel/32) -> flat [numel]
// of `dtype` (views ok). The reduce-scatter tail, normative here: fp32
// rank-order sum of the dequantized copies, then .to(dtype) — no
// requantization. A 255 scale in any copy makes that group NaN.
Tensor mx8_reduce_to(const Tensor& pin, const Tensor& sin, int64_t numel,
                     int P, at::ScalarType dtype,
                     const c10::optional<Tensor>& out_opt = c10::nullopt) {
  const int dt = mx8_dtype_code(dtype);
  if (pin.is_cuda()) {
    auto out = out_or_empty(out_opt, {numel}, pin.options().dtype(dtype));
    launch_mx8_reduce_to(pin.data_ptr(), sin.data_ptr(), out.data_ptr(),
                         numel, P, dt, current_gpu_stream(pin));
    return out;
  }
  auto acc = mx8_sum_copies(pin, sin, (numel + 31) / 32, P);
  auto res = acc.view({-1}).narrow(0, 0, numel).to(dtype);
  return out_opt.has_value() ? out_opt->copy_(res) : res;
}

// One grouped Transport::exchange of quantized groups. On either side peer
// p's piece is the groups [off[p], off[p] + cnt[p]) of (pay, sc): sent from
// there, or received into them. Payload and scales travel as two contiguous
// pieces per peer. Empty pieces are not listed: both transports skip them on
// both ends of a pair anyway.
struct Mx8Side {
  Tensor pay, sc;
  std::vector<int64_t> off, cnt;  // per peer, in groups
};

void mx8_exchange(Transport& tr, const Mx8Side& send, const Mx8Side& recv) {
  std::vector<Tensor> sends, recvs;
  std::vector<int> speers, rpeers;
  auto list = [](const Mx8Side& s, std::vector<Tensor>& bufs,
                 std::vector<int>& peers) {
    for (int p = 0; p < (int)s.cnt.size(); ++p) {
      if (s.cnt[p] == 0) continue;
      bufs.push_back(s.pay.narrow(0, s.off[p] * 32, s.cnt[p] * 32));
      bufs.push_back(s.sc.narrow(0, s.off[p], s.cnt[p]));
      peers.insert(peers.end(), 2, p);
    }
  };
  list(send, sends, speers);
  list(recv, recvs, rpeers);
  tr.exchange(sends, speers, recvs, rpeers);
}

// Equal blocks of Gb groups, block p for peer p: the exchange of
// mx8_reducescatter and mx8_alltoall. Returns the P received blocks.
std::pair<Tensor, Tensor> mx8_exchange_blocks(Transport& tr, const Tensor& pay,
                                              const Tensor& sc, int64_t Gb) {
  const int P = tr.size();
  auto stg_pay = at::empty({(int64_t)P * Gb * 32}, pay.options());
  auto stg_sc = at::empty({(int64_t)P * Gb}, sc.options());
  std::vector<int64_t> off(P), cnt(P, Gb);
  for (int p = 0; p < P; ++p) off[p] = (int64_t)p * Gb;
  mx8_exchange(tr, {pay, sc, off, cnt}, {stg_pay, stg_sc, off, cnt});
  return {stg_pay, stg_sc};
}

// The reduce-scatter sibling of mx8_allreduce, phases 1-2 only: `packed` is
// the rank-major packed input, P blocks of L elements (block p is what rank
// p keeps). Each block is quantized in groups of 32 that start at the
// block's first element, block p travels to rank p (payload and scales as
// two contiguous pieces per peer in ONE grouped call) and the P copies of
// the owned block are summed straight into the input dtype. Every value is
// quantized exactly once; nothing goes back on the wire. Staging is two
// buffers of ~33/32 * P*L bytes; the wire carries (P-1)*33*ceil(L/32) bytes
// per rank.
Tensor mx8_reducescatter(Transport& tr, const Tensor& packed, int64_t L) {
  const int P = tr.size();
  const int64_t Gb = (L + 31) / 32;
  auto bopts = packed.options().dtype(at::kByte);
  Tensor pay, sc;
  if (L % 32 == 0) {
    // block-relative groups coincide with flat groups: one launch
    auto q = mx8_quantize(packed);
    pay = q.first;
    sc = q.second;
  } else {
    // one launch per block; a block base off 16 bytes takes the scalar twin
    pay = at::empty({(int64_t)P * Gb * 32}, bopts);
    sc = at::empty({(int64_t)P * Gb}, bopts);
    for (int p = 0; p < P; ++p) {
      mx8_quantize(packed.narrow(0, (int64_t)p * L, L),
                   pay.narrow(0, (int64_t)p * Gb * 32, Gb * 32),
                   sc.narrow(0, (int64_t)p * Gb, Gb));
    }
  }
  auto stg = mx8_exchange_blocks(tr, pay, sc, Gb);
  return mx8_reduce_to(stg.first, stg.second, L, P, packed.scalar_type());
}

// P gathered blocks: pay [P * Gb*32], sc [P * Gb], Gb = ceil(L/32),
// L = rows*row_elems, groups starting at each block (views ok) ->
// [rows, P, row_elems] of `dtype`. The allgather tail, normative here:
//   out[b, r, j] = dq(block r)[b*row_elems + j].to(dtype)
// A 255 scale gives a NaN group in that block only.
Tensor mx8_dequantize_blocks(const Tensor& pay, const Tensor& sc, int P,
                             int64_t rows, int64_t row_elems,
                             at::ScalarType dtype,
                             const c10::optional<Tensor>& out_opt =
                                 c10::nullopt) {
  const int dt = mx8_dtype_code(dtype);
  TORCH_CHECK(P >= 1 && P <= 65535,
              "mpi4torch_amd: mx8_dequantize_blocks supports 1..65535 "
              "blocks, got ", P);
  auto out = out_or_empty(out_opt, {rows, (int64_t)P, row_elems},
                          pay.options().dtype(dtype));
  if (out.numel() == 0) return out;
  if (pay.is_cuda()) {
    launch_mx8_dequantize_blocks(pay.data_ptr(), sc.data_ptr(),
                                 out.data_ptr(), P, rows, row_elems, dt,
                                 current_gpu_stream(pay));
    return out;
  }
  const int64_t L = rows * row_elems;
  const int64_t Gb = (L + 31) / 32;
  auto pv = pay.view({P, Gb, 32});
  auto sv = sc.view({P, Gb});
  for (int r = 0; r < P; ++r) {
    auto d = mx8_dequantize_groups(pv[r], sv[r]).view({-1});
    out.select(1, r).copy_(
        d.narrow(0, 0, L).to(dtype).view({rows, row_elems}));
  }
  return out;
}

// The allgather of the family: `in` is this rank's contiguous tensor seen as
// [rows, row_elems] (rows = the dims before the gather axis). It is
// quantized once as one flat stream (groups start at its first element),
// payload and scales are allgathered as bytes (equal counts: the plain
// collective on both transports, no grouped p2p) and the fused tail
// dequantizes every block, the own one included, straight into
// [rows, P, row_elems]. Every rank decodes the same bytes, so results are
// identical across ranks. Staging is two byte buffers of ~33/32 * P*L; the
// wire carries (P-1)*33*ceil(L/32) bytes received per rank.
Tensor mx8_allgather(Transport& tr, const Tensor& in, int64_t rows,
                     int64_t row_elems) {
  const int P = tr.size();
  const int64_t Gb = (rows * row_elems + 31) / 32;
  auto q = mx8_quantize(in.view({-1}));
  auto bopts = in.options().dtype(at::kByte);
  auto all_pay = at::empty({(int64_t)P * Gb * 32}, bopts);
  auto all_sc = at::empty({(int64_t)P * Gb}, bopts);
  tr.allgather_equal(q.first, all_pay);
  tr.allgather_equal(q.second, all_sc);
  return mx8_dequantize_blocks(all_pay, all_sc, P, rows, row_elems,
                               in.scalar_type());
}

// `in`: contiguous, rows*P*row_elems elements seen as [rows, P, row_elems]
// -> (payload [P, Gb*32], scales [P, Gb]), Gb = ceil(rows*row_elems/32).
// The all-to-all head, normative here: block p is mx8_quantize of the
// contiguous copy of in[:, p, :], so its groups start at the block and its
// partial last group is zero-padded.
std::pair<Tensor, Tensor> mx8_quantize_blocks(
    const Tensor& in, int P, int64_t rows, int64_t row_elems,
    const c10::optional<Tensor>& payload_out = c10::nullopt,
    const c10::optional<Tensor>& scales_out = c10::nullopt) {
  const int dt = mx8_dtype_code(in.scalar_type());
  TORCH_CHECK(P >= 1 && P <= 65535,
              "mpi4torch_amd: mx8_quantize_blocks supports 1..65535 "
              "blocks, got ", P);
  const int64_t Gb = (rows * row_elems + 31) / 32;
  auto bopts = in.options().dtype(at::kByte);
  auto pay = out_or_empty(payload_out, {(int64_t)P, Gb * 32}, bopts);
  auto sc = out_or_empty(scales_out, {(int64_t)P, Gb}, bopts);
  if (pay.numel() == 0) return {pay, sc};
  if (in.is_cuda()) {
    launch_mx8_quantize_blocks(in.data_ptr(), pay.data_ptr(), sc.data_ptr(),
                               P, rows, row_elems, dt,
                               current_gpu_stream(in));
    return {pay, sc};
  }
  auto v = in.view({rows, (int64_t)P, row_elems});
  for (int p = 0; p < P; ++p) {
    auto q = mx8_quantize(v.select(1, p).contiguous().view({-1}));
    pay[p].copy_(q.first);
    sc[p].copy_(q.second);
  }
  return {pay, sc};
}

// The all-to-all of the family: `in` is this rank's contiguous tensor seen
// as [rows_s, P, row_s] (rows_s = the dims before the scatter axis, row_s =
// its share n of the scatter axis times the dims after it). Block p, what
// rank p keeps, is quantized in place in groups of 32 that start at the
// block; block p travels to rank p (payload and scales as two contiguous
// pieces per peer in ONE grouped call, the call shape of mx8_reducescatter)
// and the fused tail dequantizes the P received blocks, the own one
// included, straight into [rows_g, P, row_g] (the block shape split at the
// gather axis). No pack pass, no unpack pass, no per-block launch; every
// value is quantized exactly once. Staging is two pairs of byte buffers of
// ~33/32 * numel; the wire carries (P-1)*33*ceil(numel/P/32) bytes per rank.
Tensor mx8_alltoall(Transport& tr, const Tensor& in, int64_t rows_s,
                    int64_t row_s, int64_t rows_g, int64_t row_g) {
  const int P = tr.size();
  const int64_t Gb = (rows_s * row_s + 31) / 32;
  auto q = mx8_quantize_blocks(in, P, rows_s, row_s);
  auto stg = mx8_exchange_blocks(tr, q.first.view({-1}), q.second.view({-1}),
                                 Gb);
  return mx8_dequantize_blocks(stg.first, stg.second, P, rows_g, row_g,
                               in.scalar_type());
}

// Segment layout of the variable-count codec: segment p covers `counts[p]`
// stream slices from the prefix sum on, L_p = rows*counts[p]*after elements,
// G_p = ceil(L_p/32) groups from group goff_p = sum_{q<p} G_q on.
struct Mx8SegPlan {
  std::vector<Mx8SegDesc> segs;
  std::vector<int64_t> groups;  // G_p
  int64_t slices = 0;           // sum of counts
  int64_t total_groups = 0;     // sum of G_p
  std::vector<int64_t> goffs() const {
    std::vector<int64_t> o;
    for (const auto& s : segs) o.push_back(s.goff);
    return o;
  }
};

Mx8SegPlan mx8_seg_plan(const std::vector<int64_t>& counts, int64_t rows,
                        int64_t after) {
  Mx8SegPlan pl;
  pl.segs.reserve(counts.size());
  pl.groups.reserve(counts.size());
  for (int64_t c : counts) {
    TORCH_CHECK(c >= 0, "mpi4torch_amd: negative segment count ", c);
    const int64_t G = (rows * c * after + 31) / 32;
    pl.segs.push_back(Mx8SegDesc{pl.slices, c, pl.total_groups});
    pl.groups.push_back(G);
    pl.slices += c;
    pl.total_groups += G;
  }
  return pl;
}

// `in`: contiguous, seen as [rows, S, after]. The pairwise all-to-all head,
// normative here: with xs = in.index_select(1, order) if `order` is given,
// else in, segment p is mx8_quantize of the contiguous copy of
// xs[:, displ_p : displ_p + counts[p], :] — groups start at the segment, the
// partial last group is zero-padded. Returns (payload [32*sum G_p], scales
// [sum G_p]) with the segments' streams one after the other. sum(counts)
// must equal S without an order and the order's length with one.
std::pair<Tensor, Tensor> mx8_quantize_segments(
    const Tensor& in, int64_t rows, int64_t after,
    const std::vector<int64_t>& counts, const c10::optional<Tensor>& order,
    const c10::optional<Tensor>& payload_out = c10::nullopt,
    const c10::optional<Tensor>& scales_out = c10::nullopt) {
  const int dt = mx8_dtype_code(in.scalar_type());
  const auto pl = mx8_seg_plan(counts, rows, after);
  const int64_t S = rows * after > 0 ? in.numel() / (rows * after) : 0;
  auto bopts = in.options().dtype(at::kByte);
  auto pay = payload_out.has_value()
                 ? payload_out->narrow(0, 0, pl.total_groups * 32)
                 : at::empty({pl.total_groups * 32}, bopts);
  auto sc = scales_out.has_value() ? scales_out->narrow(0, 0, pl.total_groups)
                                   : at::empty({pl.total_groups}, bopts);
  if (pl.total_groups == 0) return {pay, sc};
  if (in.is_cuda()) {
    launch_mx8_quantize_segments(
        in.data_ptr(),
        order.has_value() ? order->data_ptr<int64_t>() : nullptr,
        pay.data_ptr(), sc.data_ptr(), pl.segs.data(), (int)pl.segs.size(),
        rows, S, after, dt, current_gpu_stream(in));
    return {pay, sc};
  }
  auto xs = in.view({rows, S, after});
  if (order.has_value()) xs = xs.index_select(1, *order);
  for (size_t p = 0; p < counts.size(); ++p) {
    if (pl.groups[p] == 0) continue;
    auto q = mx8_quantize(
        xs.narrow(1, pl.segs[p].displ, counts[p]).contiguous().view({-1}));
    pay.narrow(0, pl.segs[p].goff * 32, pl.groups[p] * 32).copy_(q.first);
    sc.narrow(0, pl.segs[p].goff, pl.groups[p]).copy_(q.second);
  }
  return {pay, sc};
}

// The pairwise all-to-all tail, normative here: segment p's stream (layout
// as above, R = sum(counts)) gives
//   y[:, displ_p : displ_p + counts[p], :] = dq(segment p)[:L_p].to(dtype)
// and the result [rows, R, after] is y without an order, else a tensor with
// out.index_copy_(1, order, y): received slice i lands at slice order[i].
// `out` (contiguous [rows, R, after]) is written in place when given; slices
// no order entry names keep their contents.
Tensor mx8_dequantize_segments(const Tensor& pay, const Tensor& sc,
                               int64_t rows, int64_t after,
                               const std::vector<int64_t>& counts,
                               const c10::optional<Tensor>& order,
                               at::ScalarType dtype,
                               const c10::optional<Tensor>& out_opt =
                                   c10::nullopt) {
  const int dt = mx8_dtype_code(dtype);
  const auto pl = mx8_seg_plan(counts, rows, after);
  auto out = out_opt.has_value()
                 ? *out_opt
                 : at::empty({rows, pl.slices, after},
                             pay.options().dtype(dtype));
  if (pl.total_groups == 0) return out;
  if (pay.is_cuda()) {
    launch_mx8_dequantize_segments(
        pay.data_ptr(), sc.data_ptr(),
        order.has_value() ? order->data_ptr<int64_t>() : nullptr,
        out.data_ptr(), pl.segs.data(), (int)pl.segs.size(), rows, pl.slices,
        after, dt, current_gpu_stream(pay));
    return out;
  }
  auto y = order.has_value() ? at::empty({rows, pl.slices, after},
                                         pay.options().dtype(dtype))
                             : out;
  for (size_t p = 0; p < counts.size(); ++p) {
    if (pl.groups[p] == 0) continue;
    const int64_t G = pl.groups[p];
    auto d = mx8_dequantize_groups(
                 pay.narrow(0, pl.segs[p].goff * 32, G * 32).view({G, 32}),
                 sc.narrow(0, pl.segs[p].goff, G))
                 .view({-1});
    y.narrow(1, pl.segs[p].displ, counts[p])
        .copy_(d.narrow(0, 0, rows * counts[p] * after)
                   .to(dtype)
                   .view({rows, counts[p], after}));
  }
  if (order.has_value()) out.index_copy_(1, *order, y);
  return out;
}

// The pairwise all-to-all of the family: `in` is this rank's contiguous
// tensor seen as [rows, S, after]. The fused head gathers slices through
// send_order while it quantizes segment p (what rank p receives) in groups of
// 32 that start at the segment; payload and scales travel as two contiguous
// pieces per peer in ONE grouped call, their sizes 32*G and G computed from
// the counts both ends know; the fused tail dequantizes the received
// segments, the own one included, straight into [rows, R, after], scattering
// slices through recv_order while it writes. No index_select pass on either
// side; every value is quantized exactly once. Both transports skip
// zero-length pieces on both ends of a pair, and so does this: an empty
// segment is not listed at all.
Tensor mx8_alltoall_pairwise(Transport& tr, const Tensor& in, int64_t rows,
                             int64_t after,
                             const std::vector<int64_t>& send_counts,
                             const std::vector<int64_t>& recv_counts,
                             const c10::optional<Tensor>& send_order,
                             const c10::optional<Tensor>& recv_order) {
  const auto sp = mx8_seg_plan(send_counts, rows, after);
  const auto rp = mx8_seg_plan(recv_counts, rows, after);
  auto q = mx8_quantize_segments(in, rows, after, send_counts, send_order);
  auto bopts = in.options().dtype(at::kByte);
  auto stg_pay = at::empty({rp.total_groups * 32}, bopts);
  auto stg_sc = at::empty({rp.total_groups}, bopts);
  mx8_exchange(tr, {q.first, q.second, sp.goffs(), sp.groups},
               {stg_pay, stg_sc, rp.goffs(), rp.groups});
  return mx8_dequantize_segments(stg_pay, stg_sc, rows, after, recv_counts,
                                 recv_order, in.scalar_type());
}

// The mxfp8 sibling of hierarchical_allreduce: quantize once, exchange each
// rank's copy of group-block j to rank j (payload and scales as two
// contiguous pieces per peer in ONE grouped call), fused
// dequantize-sum-requantize of the owned block, allgather payload + scales
// in place, dequantize. Values are quantized exactly twice at any P; every
// rank decodes the same bytes, so results are identical across ranks.
// Staging is ~33/32 * numel bytes twice (quantized input, P copies of the
// owned block), never P * numel.
Tensor mx8_allreduce(Transport& tr, const Tensor& in) {
  const int P = tr.size();
  const int me = tr.rank();
  const int64_t N = in.numel();
  const int64_t G = (N + 31) / 32;
  std::vector<int64_t> counts(P);
  for (int p = 0; p < P; ++p) counts[p] = G / P + (p < G % P ? 1 : 0);
  auto displs = prefix_displs(counts);
  auto nz_narrow = [](const Tensor& t, int64_t off, int64_t len) {
    return len > 0 ? t.narrow(0, off, len) : t.narrow(0, 0, 0);
  };
  auto q = mx8_quantize(in.view({-1}));
  const int64_t cm = counts[me];
  // phase 1: one grouped exchange carrying payload and scales
  auto bopts = in.options().dtype(at::kByte);
  auto stg_pay = at::empty({(int64_t)P * cm * 32}, bopts);
  auto stg_sc = at::empty({(int64_t)P * cm}, bopts);
  std::vector<int64_t> stg_off(P), stg_cnt(P, cm);
  for (int p = 0; p < P; ++p) stg_off[p] = (int64_t)p * cm;
  mx8_exchange(tr, {q.first, q.second, displs, counts},
               {stg_pay, stg_sc, stg_off, stg_cnt});
  // phase 2: fused reduce of the P copies of the owned groups
  auto out_pay = at::empty({G * 32}, bopts);
  auto out_sc = at::empty({G}, bopts);
  auto my_pay = nz_narrow(out_pay, displs[me] * 32, cm * 32);
  auto my_sc = nz_narrow(out_sc, displs[me], cm);
  mx8_reduce(stg_pay, stg_sc, my_pay, my_sc, cm, P);
  // phase 3: allgather payload + scales (equal counts on GPU: RCCL, in
  // place; otherwise grouped p2p — same split as hierarchical_allreduce)
  if (G % P == 0 && tr.is_gpu()) {
    tr.allgather_equal(my_pay, out_pay);
    tr.allgather_equal(my_sc, out_sc);
  } else {
    // the owned block to every other rank, every other rank's block back
    std::vector<int64_t> own_off(P, displs[me]), own_cnt(P, cm);
    auto their_cnt = counts;
    own_cnt[me] = their_cnt[me] = 0;
    mx8_exchange(tr, {out_pay, out_sc, own_off, own_cnt},
                 {out_pay, out_sc, displs, their_cnt});
  }
  return mx8_dequantize(out_pay, out_sc, N, in.scalar_type())
      .view(in.sizes());
}

// ------------------------- autograd node base -----------------------------

struct M4ANode : public Node {
  c10::intrusive_ptr<Communicator> comm;
  void release_variables() override {}
};

struct UnimplementedBackward : public M4ANode {
  std::string name() const override { return "M4AUnimplementedBackward"; }
  variable_list apply(variable_list&&) override {
    TORCH_CHECK(false,
                "mpi4torch_amd: backward is only implemented for MPI_SUM "
                "reductions (matching the reference, mpi4torch "
                "csrc/extension.cpp:189-202)");
  }
};

// Poison node installed on inputs of in-place collectives so a later use of
// the ORIGINAL variable (instead of the returned one) fails loudly in
// backward. Mirrors MPINoInplaceBackward (reference :395-403, :454-461).
struct NoInplaceBackward : public Node {
  std::string name() const override { return "M4ANoInplaceBackward"; }
  variable_list apply(variable_list&&) override {
    TORCH_CHECK(false,
                "mpi4torch_amd: reuse of a variable passed to an in-place "
                "collective is not supported; use the returned tensor");
  }
};

template <typename NodeT, typename... Args>
std::shared_ptr<NodeT> make_node(const c10::intrusive_ptr<Communicator>& comm,
                                 Args&&... args) {
  auto node = std::shared_ptr<NodeT>(new NodeT(std::forward<Args>(args)...),
                                     torch::autograd::deleteNode);
  node->comm = comm;
  return node;
}

void attach_history(const Tensor& result, const std::shared_ptr<Node>& node) {
  if (node) {
    torch::autograd::set_history(result, node);
  }
}

void poison_inplace_input(const Tensor& input) {
  // Only for non-leaf inputs — leaves are owned by AccumulateGrad
  // (reference :454-461 has the same restriction).
  if (input.grad_fn()) {
    auto node = std::shared_ptr<NoInplaceBackward>(
        new NoInplaceBackward(), torch::autograd::deleteNode);
    auto& input_nc = const_cast<Tensor&>(input);
    torch::autograd::set_history(input_nc, node);
  }
}

// The frame of a collective front-end. With an input that requires grad,
// make_grad_fn(comm) builds the backward node and its next edges are set
// here; body(tr, in, stager) runs below autograd on the staged contiguous
// input and returns the result still on the transport's side; the frame
// brings it back and attaches history.
template <typename MakeNode, typename Body>
Tensor collective_frame(Communicator& comm, const Tensor& input,
                        MakeNode&& make_grad_fn, Body&& body) {
  std::shared_ptr<Node> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_grad_fn(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(&comm));
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    return stager.from_comm(body(comm.tr_for(in), in, stager));
  }();
  attach_history(result, grad_fn);
  return result;
}

// The compressed collectives' input check; opname is the front-end's.
void check_mx8_input(const char* opname, const Tensor& t) {
  (void)mx8_dtype_code(t.scalar_type(), opname);
}

// World of one: nothing crosses a wire, so nothing is compressed and the
// result is an exact clone. force_full_path on a GPU runs the whole pipeline
// instead: the codec kernels around a self-exchange.
bool world1_shortcut(const Transport& tr, const Tensor& in) {
  return tr.size() == 1 && !(config().force_full_path && in.is_cuda());
}

} // namespace

// ---------------------------------------------------------------------------
// Allreduce (reference csrc/extension.cpp:254-308)
// ---------------------------------------------------------------------------

namespace {
struct AllreduceSumBackward : public M4ANode {
  std::string name() const override { return "M4AAllreduceSumBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // self-adjoint: d/dx of sum-allreduce is sum-allreduce
      out[0] = comm->Allreduce(grads[0], kSum);
    }
    return out;
  }
};
} // namespace

Tensor Communicator::Allreduce(const Tensor& input, int64_t op) {
  check_op(op);
  TORCH_CHECK(!is_pairloc(op) ||
                  (input.dim() >= 1 && input.size(-1) == 2),
              "mpi4torch_amd: MPI_MINLOC/MAXLOC operate on (value, "
              "location) pairs — the last axis must have size 2 (the "
              "tensor analog of MPI's pair types, reference "
              "csrc/extension.cpp:204-252)");
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    if (op == kSum) {
      grad_fn = make_node<AllreduceSumBackward>(
          c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this));
    } else {
      grad_fn = make_node<UnimplementedBackward>(
          c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this));
    }
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(in);
    debug_check_collective(group_name_, "Allreduce", in, {op});
    return stager.from_comm(allreduce_lowered(tr, in, op));
  }();
  attach_history(result, grad_fn);
  return result;
}

// ---------------------------------------------------------------------------
// AllreduceCompressed (MI355X extension; not in the reference API)
// ---------------------------------------------------------------------------

namespace {
struct AllreduceCompressedBackward : public M4ANode {
  std::string name() const override {
    return "M4AAllreduceCompressedBackward";
  }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // treated as the self-adjoint sum; quantization is straight-through,
      // and the gradient itself travels compressed
      out[0] = comm->AllreduceCompressed(grads[0], kSum);
    }
    return out;
  }
};
} // namespace

Tensor Communicator::AllreduceCompressed(const Tensor& input, int64_t op) {
  TORCH_CHECK(op == kSum,
              "mpi4torch_amd: AllreduceCompressed supports MPI_SUM only "
              "(got ", red_op_name(op), ")");
  check_mx8_input("AllreduceCompressed", input);
  return collective_frame(
      *this, input,
      [](auto comm) { return make_node<AllreduceCompressedBackward>(comm); },
      [&](Transport& tr, const Tensor& in, const DeviceStager&) {
        debug_check_collective(group_name_, "AllreduceCompressed", in, {op});
        if (in.numel() == 0) return in.clone();
        // full path: self-exchange, all three kernels, allgather
        if (world1_shortcut(tr, in)) return fast_clone(in);
        return mx8_allreduce(tr, in);
      });
}

// ---------------------------------------------------------------------------
// Bcast_ (reference csrc/extension.cpp:310-365)
// ---------------------------------------------------------------------------

namespace {
struct BcastInPlaceBackward : public M4ANode {
  explicit BcastInPlaceBackward(int64_t root) : root(root) {}
  std::string name() const override { return "M4ABcastInPlaceBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // adjoint of broadcast-from-root is reduce-to-root
      out[0] = comm->Reduce_(grads[0], kSum, root);
    }
    return out;
  }
  int64_t root;
};
} // namespace

Tensor Communicator::Bcast_(const Tensor& input, int64_t root) {
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_node<BcastInPlaceBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this), root);
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto t = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(t);
    debug_check_collective(group_name_, "Bcast_", t, {root});
    if (tr.size() > 1 && t.numel() > 0) tr.broadcast(t, (int)root);
    return stager.from_comm(std::move(t));
  }();
  attach_history(result, grad_fn);
  return result;
}

// ---------------------------------------------------------------------------
// Reduce_ (reference csrc/extension.cpp:367-464)
// ---------------------------------------------------------------------------

namespace {
struct ReduceSumInPlaceBackward : public M4ANode {
  explicit ReduceSumInPlaceBackward(int64_t root) : root(root) {}
  std::string name() const override { return "M4AReduceSumInPlaceBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // adjoint of reduce-to-root is broadcast-from-root
      out[0] = comm->Bcast_(grads[0], root);
    }
    return out;
  }
  int64_t root;
};
} // namespace

Tensor Communicator::Reduce_(const Tensor& input, int64_t op, int64_t root) {
  check_op(op);
  TORCH_CHECK(!is_pairloc(op) ||
                  (input.dim() >= 1 && input.size(-1) == 2),
              "mpi4torch_amd: MPI_MINLOC/MAXLOC operate on (value, "
              "location) pairs — the last axis must have size 2");
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    if (op == kSum) {
      grad_fn = make_node<ReduceSumInPlaceBackward>(
          c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this), root);
    } else {
      grad_fn = make_node<UnimplementedBackward>(
          c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this));
    }
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto t = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(t);
    debug_check_collective(group_name_, "Reduce_", t, {op, root});
    if (tr.size() > 1 && t.numel() > 0) {
      if (is_arith(op) && native_reduce_dtype(tr, t.scalar_type())) {
        tr.reduce(t, (RedOp)op, (int)root);
      } else {
        // lowered ops: compute the full allreduce, keep root's value
        auto red = allreduce_lowered(tr, t, op);
        t.copy_(red);
      }
      if (tr.rank() != (int)root) {
        // non-root result is defined as zeros (reference :443-447)
        t.zero_();
      }
    }
    return stager.from_comm(std::move(t));
  }();
  attach_history(result, grad_fn);
  if (grad_fn) poison_inplace_input(input);
  return result;
}

// ---------------------------------------------------------------------------
// JoinDummies (reference csrc/extension.cpp:989-1046)
// ---------------------------------------------------------------------------

namespace {
struct JoinDummiesBackward : public Node {
  std::string name() const override { return "M4AJoinDummiesBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1 + dummy_sizes.size());
    if (should_compute_output(0)) {
      out[0] = grads[0];
    }
    for (size_t i = 0; i < dummy_sizes.size(); ++i) {
      if (should_compute_output(i + 1)) {
        // dummies are pure DAG dependencies: their gradient is zero
        out[i + 1] = at::zeros(dummy_sizes[i], dummy_options[i]);
      }
    }
    return out;
  }
  std::vector<std::vector<int64_t>> dummy_sizes;
  std::vector<at::TensorOptions> dummy_options;
};
} // namespace

Tensor join_dummies(const Tensor& loopthrough,
                    const std::vector<Tensor>& dummies) {
  if (!torch::autograd::compute_requires_grad(dummies)) {
    // no dummy carries grad: pure passthrough (reference :1030-1033)
    return loopthrough;
  }
  auto grad_fn = std::shared_ptr<JoinDummiesBackward>(
      new JoinDummiesBackward(), torch::autograd::deleteNode);
  grad_fn->set_next_edges(
      torch::autograd::collect_next_edges(loopthrough, dummies));
  for (const auto& d : dummies) {
    grad_fn->dummy_sizes.push_back(d.sizes().vec());
    grad_fn->dummy_options.push_back(d.options());
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    return loopthrough.variable_data();
  }();
  attach_history(result, grad_fn);
  return result;
}

// ---------------------------------------------------------------------------
// Gather / Scatter (reference csrc/extension.cpp:466-599, 736-884)
// ---------------------------------------------------------------------------

namespace {
struct GatherBackward : public M4ANode {
  GatherBackward(int64_t axis, int64_t root, int64_t numelem)
      : axis(axis), root(root), numelem(numelem) {}
  std::string name() const override { return "M4AGatherBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // adjoint of axis-gather is axis-scatter; numelem captured at forward
      // (reference :483-495; input_metadata unusable per pytorch#79446)
      out[0] = comm->Scatter(grads[0], axis, numelem, root);
    }
    return out;
  }
  int64_t axis, root, numelem;
};

struct ScatterBackward : public M4ANode {
  ScatterBackward(int64_t axis, int64_t root, std::vector<int64_t> in_sizes,
                  at::TensorOptions in_options)
      : axis(axis), root(root), in_sizes(std::move(in_sizes)),
        in_options(in_options) {}
  std::string name() const override { return "M4AScatterBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      auto gathered = comm->Gather(grads[0], axis, root);
      if (comm->GetRank() == root) {
        out[0] = gathered;
      } else {
        // the non-root input contributed nothing; keep the DAG edge alive
        // with a zeros tensor of its shape (reference :752-767)
        out[0] = join_dummies(at::zeros(in_sizes, in_options), {gathered});
      }
    }
    return out;
  }
  int64_t axis, root;
  std::vector<int64_t> in_sizes;
  at::TensorOptions in_options;
};

// Carve a contiguous tensor into per-rank flat blocks. If `base` is given
// and before==1, blocks are zero-copy views of it at the axis offsets
// (skipping the pack/unpack kernel entirely); otherwise fresh flat buffers.
std::vector<Tensor> make_blocks(const Tensor& like, int64_t before,
                                int64_t after,
                                const std::vector<int64_t>& counts,
                                const std::vector<int64_t>& displs,
                                const Tensor* base) {
  std::vector<Tensor> blocks(counts.size());
  const bool direct = (base != nullptr) && before == 1;
  Tensor flat;
  if (direct) flat = base->view({-1});
  for (size_t i = 0; i < counts.size(); ++i) {
    const int64_t n = before * counts[i] * after;
    if (direct) {
      // zero-length slices may carry an offset past the end (empty overlap
      // intervals in same-axis Alltoall): clamp to a valid empty view
      blocks[i] = n == 0 ? flat.narrow(0, 0, 0)
                         : flat.narrow(0, displs[i] * after, n);
    } else {
      blocks[i] = at::empty({n}, like.options());
    }
  }
  return blocks;
}

std::vector<int> iota_peers(int n) {
  std::vector<int> p(n);
  for (int i = 0; i < n; ++i) p[i] = i;
  return p;
}
} // namespace

Tensor Communicator::Gather(const Tensor& input, int64_t gatheraxis,
                            int64_t root) {
  gatheraxis = at::maybe_wrap_dim(gatheraxis, input.dim());
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_node<GatherBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
        gatheraxis, root, input.size(gatheraxis));
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(in);
    if (w1_shortcut(tr)) return stager.from_comm(fast_clone(in));
    debug_check_axis_collective(group_name_, "Gather", in, {gatheraxis},
                                {gatheraxis, root});
    const auto g = axis_geom(in, gatheraxis);
    auto counts = host_allgather_int64(group_name_, g.axis);
    auto displs = prefix_displs(counts);
    const int64_t total = displs.back() + counts.back();
    const int me = tr.rank();

    auto newsizes = in.sizes().vec();
    // non-root output is empty along the gather axis (reference behavior:
    // recvcounts stay zero off-root, csrc/extension.cpp:540-554)
    newsizes[gatheraxis] = (me == (int)root) ? total : 0;
    auto out = at::empty(newsizes, in.options());

    // phased pipelining: rows = the common `before` (non-axis dims match
    // across ranks); each sender's contiguous slab rows land directly in
    // root's per-peer staging, unpacked phase by phase
    const int64_t K =
        g.before > 1
            ? phase_count(in, g.before * total * g.after *
                                  in.element_size() / tr.size())
            : 1;

    if (me == (int)root) {
      auto blocks = make_blocks(in, g.before, g.after, counts, displs, &out);
      std::vector<Tensor> sends{in};
      std::vector<int> speers{(int)root};
      auto rpeers = iota_peers(tr.size());
      if (K > 1) {
        std::vector<int64_t> srowe{g.axis * g.after};
        std::vector<int64_t> rrowe(counts.size());
        for (size_t i = 0; i < counts.size(); ++i) {
          rrowe[i] = counts[i] * g.after;
        }
        phased_funnel_exchange(
            tr, K, g.before, sends, speers, srowe, blocks, rpeers, rrowe,
            nullptr, [&](int64_t b0, int64_t b1) {
              move_axis_blocks(out, gatheraxis, displs, counts, blocks,
                               /*pack=*/false, b0, b1);
            });
      } else {
        tr.exchange(sends, speers, blocks, rpeers);
        if (g.before != 1) {
          move_axis_blocks(out, gatheraxis, displs, counts, blocks,
                           /*pack=*/false);
        }
      }
    } else {
      std::vector<Tensor> sends{in}, recvs;
      std::vector<int> speers{(int)root}, rpeers;
      if (K > 1) {
        std::vector<int64_t> srowe{g.axis * g.after}, rrowe;
        phased_funnel_exchange(tr, K, g.before, sends, speers, srowe, recvs,
                               rpeers, rrowe, nullptr, nullptr);
      } else {
        tr.exchange(sends, speers, recvs, rpeers);
      }
    }
    return stager.from_comm(std::move(out));
  }();
  attach_history(result, grad_fn);
  return result;
}

Tensor Communicator::Scatter(const Tensor& input, int64_t scatteraxis,
                             int64_t numelem, int64_t root) {
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_node<ScatterBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
        scatteraxis, root, input.sizes().vec(), input.options());
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(in);
    if (w1_shortcut(tr)) {
      TORCH_CHECK(numelem == in.size(at::maybe_wrap_dim(scatteraxis, in.dim())),
                  "Scatter: numelem must equal the axis size at world size 1");
      return stager.from_comm(fast_clone(in));
    }
    const int me = tr.rank();
    debug_check_dtype_collective(group_name_, "Scatter", in.scalar_type(),
                                 {scatteraxis, root});
    // root broadcasts [ndim, sizes...]: the shape contract for non-root
    // ranks whose input tensor is a placeholder (reference :788-796)
    std::vector<int64_t> meta;
    if (me == (int)root) {
      meta.push_back(in.dim());
      for (auto s : in.sizes()) meta.push_back(s);
    }
    meta = host_broadcast_int64(group_name_, meta, (int)root, -1);
    const int64_t ndim = meta[0];
    std::vector<int64_t> rootsizes(meta.begin() + 1, meta.begin() + 1 + ndim);
    const int64_t axis = at::maybe_wrap_dim(scatteraxis, ndim);

    auto counts = host_allgather_int64(group_name_, numelem);
    auto displs = prefix_displs(counts);
    const int64_t total = displs.back() + counts.back();
    TORCH_CHECK(total == rootsizes[axis], "Scatter: sum of per-rank numelem (",
                total, ") must equal the scatter-axis size (", rootsizes[axis],
                ")");

    auto outsizes = rootsizes;
    outsizes[axis] = counts[me];
    auto out = at::empty(outsizes, in.options());

    // phased pipelining (marshaled side = root's pack; receivers' out IS
    // the slab layout, so their phase slices are plain contiguous ranges).
    // `before` comes from the SHARED rootsizes, so non-root ranks compute
    // the same K and row geometry without touching their placeholder.
    int64_t before_c = 1, after_c = 1;
    for (int64_t d = 0; d < ndim; ++d) {
      if (d < axis) before_c *= rootsizes[d];
      else if (d > axis) after_c *= rootsizes[d];
    }
    const int64_t K =
        before_c > 1
            ? phase_count(in, before_c * rootsizes[axis] * after_c *
                                  in.element_size() / tr.size())
            : 1;

    if (me == (int)root) {
      TORCH_CHECK(in.sizes().vec() == rootsizes);
      const auto g = axis_geom(in, axis);
      auto blocks = make_blocks(in, g.before, g.after, counts, displs, &in);
      auto speers = iota_peers(tr.size());
      std::vector<Tensor> recvs{out};
      std::vector<int> rpeers{(int)root};
      if (K > 1) {
        std::vector<int64_t> srowe(counts.size());
        for (size_t j = 0; j < counts.size(); ++j) {
          srowe[j] = counts[j] * g.after;
        }
        std::vector<int64_t> rrowe{counts[me] * g.after};
        phased_funnel_exchange(
            tr, K, g.before, blocks, speers, srowe, recvs, rpeers, rrowe,
            [&](int64_t b0, int64_t b1) {
              move_axis_blocks(in, axis, displs, counts, blocks,
                               /*pack=*/true, b0, b1);
            },
            nullptr);
      } else {
        if (g.before != 1) {
          move_axis_blocks(in, axis, displs, counts, blocks, /*pack=*/true);
        }
        tr.exchange(blocks, speers, recvs, rpeers);
      }
    } else {
      std::vector<Tensor> sends, recvs{out};
      std::vector<int> speers, rpeers{(int)root};
      if (K > 1) {
        std::vector<int64_t> srowe;
        std::vector<int64_t> rrowe{counts[me] * after_c};
        phased_funnel_exchange(tr, K, before_c, sends, speers, srowe, recvs,
                               rpeers, rrowe, nullptr, nullptr);
      } else {
        tr.exchange(sends, speers, recvs, rpeers);
      }
    }
    return stager.from_comm(std::move(out));
  }();
  attach_history(result, grad_fn);
  return result;
}

// ---------------------------------------------------------------------------
// Allgather (reference csrc/extension.cpp:601-734). Backward implemented as
// a true reduce-scatter, fixing the reference's wrong-root adjoint bug
// (ref :626-628).
// ---------------------------------------------------------------------------

namespace {
struct AllgatherBackward : public M4ANode {
  AllgatherBackward(int64_t axis, std::vector<int64_t> counts)
      : axis(axis), counts(std::move(counts)) {}
  std::string name() const override { return "M4AAllgatherBackward"; }
  variable_list apply(variable_list&& grads) override;
  int64_t axis;
  std::vector<int64_t> counts;
};
} // namespace

Tensor Communicator::Allgather(const Tensor& input, int64_t gatheraxis) {
  gatheraxis = at::maybe_wrap_dim(gatheraxis, input.dim());
  std::shared_ptr<AllgatherBackward> grad_fn;
  const bool needs_grad = torch::autograd::compute_requires_grad(input);
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(in);
    if (w1_shortcut(tr)) {
      if (needs_grad) {
        grad_fn = make_node<AllgatherBackward>(
            c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(
                this),
            gatheraxis, std::vector<int64_t>{input.size(gatheraxis)});
      }
      return stager.from_comm(fast_clone(in));
    }
    debug_check_axis_collective(group_name_, "Allgather", in, {gatheraxis},
                                {gatheraxis});
    const auto g = axis_geom(in, gatheraxis);
    auto counts = host_allgather_int64(group_name_, g.axis);
    auto displs = prefix_displs(counts);
    const int64_t total = displs.back() + counts.back();
    const bool equal = std::all_of(counts.begin(), counts.end(),
                                   [&](int64_t c) { return c == counts[0]; });
    if (needs_grad) {
      grad_fn = make_node<AllgatherBackward>(
          c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
          gatheraxis, counts);
    }

    auto newsizes = in.sizes().vec();
    newsizes[gatheraxis] = total;
    auto out = at::empty(newsizes, in.options());

    // phased pipelining: every rank both sends and receives ~the whole
    // gathered tensor, so the per-rank payload is the global logical size
    const int64_t K =
        g.before > 1
            ? phase_count(in,
                          g.before * total * g.after * in.element_size())
            : 1;
    if (equal && g.before == 1) {
      auto out_flat = out.view({-1});
      tr.allgather_equal(in, out_flat);
    } else if (K > 1) {
      // grouped p2p with phases: senders' slab rows go straight into
      // per-peer staging; each phase's unpack overlaps the next phase's
      // wire (on the xGMI crossbar direct p2p moves the same bytes as
      // the allgather ring, spread over all links)
      auto blocks = make_blocks(in, g.before, g.after, counts, displs,
                                nullptr);
      std::vector<Tensor> sends((size_t)tr.size(), in);
      auto peers = iota_peers(tr.size());
      std::vector<int64_t> srowe((size_t)tr.size(), g.axis * g.after);
      std::vector<int64_t> rrowe(counts.size());
      for (size_t i = 0; i < counts.size(); ++i) {
        rrowe[i] = counts[i] * g.after;
      }
      phased_funnel_exchange(
          tr, K, g.before, sends, peers, srowe, blocks, peers, rrowe,
          nullptr, [&](int64_t b0, int64_t b1) {
            move_axis_blocks(out, gatheraxis, displs, counts, blocks,
                             /*pack=*/false, b0, b1);
          });
    } else if (equal && tr.is_gpu()) {
      auto staging = at::empty({total * g.before * g.after}, in.options());
      tr.allgather_equal(in, staging);
      auto blocks = make_blocks(in, g.before, g.after, counts, displs, nullptr);
      for (size_t r = 0; r < blocks.size(); ++r) {
        blocks[r] = staging.narrow(0, displs[r] * g.before * g.after,
                                   g.before * counts[r] * g.after);
      }
      move_axis_blocks(out, gatheraxis, displs, counts, blocks, /*pack=*/false);
    } else {
      // variable counts: grouped p2p exchange (every rank sends its whole
      // tensor to every peer), then axis unpack
      auto blocks = make_blocks(in, g.before, g.after, counts, displs, &out);
      std::vector<Tensor> sends(tr.size(), in);
      auto peers = iota_peers(tr.size());
      tr.exchange(sends, peers, blocks, peers);
      if (g.before != 1) {
        move_axis_blocks(out, gatheraxis, displs, counts, blocks,
                         /*pack=*/false);
      }
    }
    return stager.from_comm(std::move(out));
  }();
  if (grad_fn) {
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
    attach_history(result, grad_fn);
  }
  return result;
}

namespace {
variable_list AllgatherBackward::apply(variable_list&& grads) {
  variable_list out(1);
  if (!should_compute_output(0)) return out;
  auto& grad = grads[0];
  DeviceStager stager(grad);
  auto g_in = stager.to_comm(grad).contiguous();
  auto& tr = comm->tr_for(g_in);
  if (tr.size() == 1) {
    out[0] = grads[0];
    return out;
  }
  const auto g = axis_geom(g_in, axis);
  auto displs = prefix_displs(counts);
  const int me = tr.rank();
  const bool equal = std::all_of(counts.begin(), counts.end(),
                                 [&](int64_t c) { return c == counts[0]; });
  auto outsizes = g_in.sizes().vec();
  outsizes[axis] = counts[me];

  // True adjoint of allgather: reduce-scatter of the gradient slices.
  if (equal && tr.is_gpu() &&
      native_reduce_dtype(tr, g_in.scalar_type())) {
    auto res = at::empty(outsizes, g_in.options());
    if (g.before == 1) {
      auto res_flat = res.view({-1});
      tr.reduce_scatter_equal(g_in, res_flat, kSum);
    } else {
      // pack the gradient into rank-major blocks, then reduce-scatter
      const int64_t chunk = g.before * counts[0] * g.after;
      auto staging = at::empty({(int64_t)counts.size() * chunk}, g_in.options());
      std::vector<Tensor> blocks(counts.size());
      for (size_t r = 0; r < counts.size(); ++r) {
        blocks[r] = staging.narrow(0, (int64_t)r * chunk, chunk);
      }
      move_axis_blocks(g_in, axis, displs, counts, blocks, /*pack=*/true);
      auto res_flat = res.view({-1});
      tr.reduce_scatter_equal(staging, res_flat, kSum);
    }
    out[0] = stager.from_comm(std::move(res));
    return out;
  }
  // general path (CPU, variable counts, exotic dtypes): allreduce + slice
  auto red = allreduce_lowered(tr, g_in, kSum);
  out[0] = stager.from_comm(
      red.narrow(axis, displs[me], counts[me]).contiguous());
  return out;
}
} // namespace

// ---------------------------------------------------------------------------
// Reducescatter — Allgather's adjoint as a public op (MI355X extension).
// ---------------------------------------------------------------------------

namespace {
struct ReducescatterBackward : public M4ANode {
  explicit ReducescatterBackward(int64_t axis) : axis(axis) {}
  std::string name() const override { return "M4AReducescatterBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // every rank's input slice region sees exactly the gradient of the
      // rank that kept it: concat = allgather
      out[0] = comm->Allgather(grads[0], axis);
    }
    return out;
  }
  int64_t axis;
};
} // namespace

Tensor Communicator::Reducescatter(const Tensor& input, int64_t axis,
                                   int64_t numelem) {
  axis = at::maybe_wrap_dim(axis, input.dim());
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_node<ReducescatterBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
        axis);
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(in);
    if (w1_shortcut(tr)) {
      TORCH_CHECK(numelem == in.size(axis),
                  "Reducescatter: numelem must equal the axis size at "
                  "world size 1");
      return stager.from_comm(fast_clone(in));
    }
    // numelem is per-rank (variable counts) — it must NOT enter the
    // signature; the input tensor's full shape must match elementwise.
    debug_check_collective(group_name_, "Reducescatter", in, {axis});
    const auto g = axis_geom(in, axis);
    auto counts = host_allgather_int64(group_name_, numelem);
    auto displs = prefix_displs(counts);
    const int64_t total = displs.back() + counts.back();
    TORCH_CHECK(total == g.axis,
                "Reducescatter: sum of per-rank numelem (", total,
                ") must equal the axis size (", g.axis, ")");
    const int me = tr.rank();
    auto outsizes = in.sizes().vec();
    outsizes[axis] = counts[me];
    const bool equal = std::all_of(counts.begin(), counts.end(),
                                   [&](int64_t c) { return c == counts[0]; });
    if (equal && tr.is_gpu() && native_reduce_dtype(tr, in.scalar_type())) {
      auto res = at::empty(outsizes, in.options());
      auto res_flat = res.view({-1});
      if (g.before == 1) {
        tr.reduce_scatter_equal(in, res_flat, kSum);
      } else {
        const int64_t chunk = g.before * counts[0] * g.after;
        auto staging = at::empty({(int64_t)counts.size() * chunk},
                                 in.options());
        std::vector<Tensor> blocks(counts.size());
        for (size_t r = 0; r < counts.size(); ++r) {
          blocks[r] = staging.narrow(0, (int64_t)r * chunk, chunk);
        }
        move_axis_blocks(in, axis, displs, counts, blocks, /*pack=*/true);
        tr.reduce_scatter_equal(staging, res_flat, kSum);
      }
      return stager.from_comm(std::move(res));
    }
    // general path: allreduce then slice (CPU, variable counts, exotic
    // dtypes incl. fp8 via the lowered allreduce)
    auto red = allreduce_lowered(tr, in, kSum);
    return stager.from_comm(
        red.narrow(axis, displs[me], counts[me]).contiguous());
  }();
  attach_history(result, grad_fn);
  return result;
}

// ---------------------------------------------------------------------------
// ReducescatterCompressed (MI355X extension; not in the reference API)
// ---------------------------------------------------------------------------

namespace {
struct ReducescatterCompressedBackward : public M4ANode {
  explicit ReducescatterCompressedBackward(int64_t axis) : axis(axis) {}
  std::string name() const override {
    return "M4AReducescatterCompressedBackward";
  }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // exact adjoint of the sum; quantization is straight-through and the
      // gradient travels uncompressed
      out[0] = comm->Allgather(grads[0], axis);
    }
    return out;
  }
  int64_t axis;
};
} // namespace

Tensor Communicator::ReducescatterCompressed(const Tensor& input,
                                             int64_t axis) {
  check_mx8_input("ReducescatterCompressed", input);
  axis = at::maybe_wrap_dim(axis, input.dim());
  auto make_grad_fn = [&](auto comm) {
    return make_node<ReducescatterCompressedBackward>(comm, axis);
  };
  auto body = [&](Transport& tr, const Tensor& in,
                  const DeviceStager&) -> Tensor {
    const int P = tr.size();
    TORCH_CHECK(in.size(axis) % P == 0,
                "mpi4torch_amd: ReducescatterCompressed requires equal "
                "counts: the axis size (", in.size(axis), ") must be a "
                "multiple of the world size (", P, "); Reducescatter "
                "handles variable counts");
    debug_check_collective(group_name_, "ReducescatterCompressed", in, {axis});
    auto outsizes = in.sizes().vec();
    outsizes[axis] = in.size(axis) / P;
    if (in.numel() == 0) return at::empty(outsizes, in.options());
    // full path: quantize, self-exchange, mx8_reduce_to
    if (world1_shortcut(tr, in)) return fast_clone(in);
    const auto g = axis_geom(in, axis);
    const int64_t count = g.axis / P;
    const int64_t L = g.before * count * g.after;
    Tensor packed = in.view({-1});
    if (g.before != 1) {
      // rank-major packing, exactly as Reducescatter does
      packed = at::empty({(int64_t)P * L}, in.options());
      std::vector<int64_t> counts(P, count);
      auto displs = prefix_displs(counts);
      std::vector<Tensor> blocks(P);
      for (int p = 0; p < P; ++p) {
        blocks[p] = packed.narrow(0, (int64_t)p * L, L);
      }
      move_axis_blocks(in, axis, displs, counts, blocks, /*pack=*/true);
    }
    return mx8_reducescatter(tr, packed, L).view(outsizes);
  };
  return collective_frame(*this, input, make_grad_fn, body);
}

// ---------------------------------------------------------------------------
// AllgatherCompressed (MI355X extension; not in the reference API)
// ---------------------------------------------------------------------------

namespace {
struct AllgatherCompressedBackward : public M4ANode {
  explicit AllgatherCompressedBackward(int64_t axis) : axis(axis) {}
  std::string name() const override {
    return "M4AAllgatherCompressedBackward";
  }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // exact adjoint of the concatenation; quantization is
      // straight-through, and the gradient itself travels compressed
      out[0] = comm->ReducescatterCompressed(grads[0], axis);
    }
    return out;
  }
  int64_t axis;
};
} // namespace

Tensor Communicator::AllgatherCompressed(const Tensor& input, int64_t axis) {
  check_mx8_input("AllgatherCompressed", input);
  axis = at::maybe_wrap_dim(axis, input.dim());
  auto make_grad_fn = [&](auto comm) {
    return make_node<AllgatherCompressedBackward>(comm, axis);
  };
  auto body = [&](Transport& tr, const Tensor& in,
                  const DeviceStager&) -> Tensor {
    const int P = tr.size();
    // full path: quantize, 1-rank allgather, mx8_dequantize_blocks
    if (world1_shortcut(tr, in)) return fast_clone(in);
    debug_check_axis_collective(group_name_, "AllgatherCompressed", in,
                                {axis}, {axis});
    const auto g = axis_geom(in, axis);
    auto counts = host_allgather_int64(group_name_, g.axis);
    const bool equal = std::all_of(counts.begin(), counts.end(),
                                   [&](int64_t c) { return c == counts[0]; });
    TORCH_CHECK(equal,
                "mpi4torch_amd: AllgatherCompressed requires equal counts: "
                "every rank's tensor must have the same size on axis ", axis,
                " (this rank has ", g.axis, "); Allgather handles variable "
                "counts");
    auto outsizes = in.sizes().vec();
    outsizes[axis] = g.axis * P;
    if (in.numel() == 0) return at::empty(outsizes, in.options());
    return mx8_allgather(tr, in, g.before, g.axis * g.after).view(outsizes);
  };
  return collective_frame(*this, input, make_grad_fn, body);
}

// ---------------------------------------------------------------------------
// AlltoallCompressed (MI355X extension; not in the reference API)
// ---------------------------------------------------------------------------

namespace {
struct AlltoallCompressedBackward : public M4ANode {
  AlltoallCompressedBackward(int64_t gaxis, int64_t saxis)
      : gaxis(gaxis), saxis(saxis) {}
  std::string name() const override {
    return "M4AAlltoallCompressedBackward";
  }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // exact adjoint of the permutation: the axes swapped; quantization is
      // straight-through, and the gradient itself travels compressed
      out[0] = comm->AlltoallCompressed(grads[0], saxis, gaxis);
    }
    return out;
  }
  int64_t gaxis, saxis;
};
} // namespace

Tensor Communicator::AlltoallCompressed(const Tensor& input,
                                        int64_t gatheraxis,
                                        int64_t scatteraxis) {
  check_mx8_input("AlltoallCompressed", input);
  gatheraxis = at::maybe_wrap_dim(gatheraxis, input.dim());
  scatteraxis = at::maybe_wrap_dim(scatteraxis, input.dim());
  TORCH_CHECK(gatheraxis != scatteraxis,
              "mpi4torch_amd: AlltoallCompressed requires two different "
              "axes, got ", gatheraxis, " for both; Alltoall handles the "
              "same-axis repartition");
  auto make_grad_fn = [&](auto comm) {
    return make_node<AlltoallCompressedBackward>(comm, gatheraxis,
                                                 scatteraxis);
  };
  auto body = [&](Transport& tr, const Tensor& in,
                  const DeviceStager&) -> Tensor {
    const int P = tr.size();
    TORCH_CHECK(in.size(scatteraxis) % P == 0,
                "mpi4torch_amd: AlltoallCompressed requires equal counts: "
                "the scatter-axis size (", in.size(scatteraxis), ") must be "
                "a multiple of the world size (", P, "); Alltoall/Alltoallv "
                "handle variable counts");
    // full path: mx8_quantize_blocks, self-exchange, mx8_dequantize_blocks
    if (world1_shortcut(tr, in)) return fast_clone(in);
    debug_check_axis_collective(group_name_, "AlltoallCompressed", in,
                                {gatheraxis}, {gatheraxis, scatteraxis});
    const int64_t g = in.size(gatheraxis);
    auto counts = host_allgather_int64(group_name_, g);
    const bool equal = std::all_of(counts.begin(), counts.end(),
                                   [&](int64_t c) { return c == counts[0]; });
    TORCH_CHECK(equal,
                "mpi4torch_amd: AlltoallCompressed requires equal counts: "
                "every rank's tensor must have the same size on the gather "
                "axis ", gatheraxis, " (this rank has ", g, "); "
                "Alltoall/Alltoallv handle variable counts");
    const int64_t n = in.size(scatteraxis) / P;
    auto outsizes = in.sizes().vec();
    outsizes[scatteraxis] = n;
    outsizes[gatheraxis] = g * P;
    if (in.numel() == 0) return at::empty(outsizes, in.options());
    // send side: `in` as [before_s][P][n*after_s]; receive side: the block
    // shape (scatter axis at n, gather axis at g) split at the gather axis
    const auto gs = axis_geom(in, scatteraxis);
    int64_t before_g = 1, after_g = 1;
    for (int64_t d = 0; d < in.dim(); ++d) {
      const int64_t sz = d == scatteraxis ? n : in.size(d);
      if (d < gatheraxis) before_g *= sz;
      if (d > gatheraxis) after_g *= sz;
    }
    return mx8_alltoall(tr, in, gs.before, n * gs.after, before_g, g * after_g)
        .view(outsizes);
  };
  return collective_frame(*this, input, make_grad_fn, body);
}

// ---------------------------------------------------------------------------
// Alltoall (reference csrc/extension.cpp:886-987). Unlike the reference's
// composite of GetSize() successive Scatters (ref :940-981, which serializes
// P collectives), this is ONE grouped RCCL p2p exchange with fused CDNA4
// pack/unpack — the latency/SM-efficient form on xGMI.
// ---------------------------------------------------------------------------

namespace {
struct AlltoallvBackward : public M4ANode {
  AlltoallvBackward(int64_t gaxis, int64_t saxis,
                    std::vector<int64_t> tgt, std::vector<int64_t> src)
      : gaxis(gaxis), saxis(saxis), tgt(std::move(tgt)),
        src(std::move(src)) {}
  std::string name() const override { return "M4AAlltoallvBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // adjoint: axes swapped, count vectors swapped (the gradient flows
      // back to the original partition)
      out[0] = comm->Alltoallv(grads[0], saxis, gaxis, tgt, src);
    }
    return out;
  }
  int64_t gaxis, saxis;
  std::vector<int64_t> tgt, src;
};

struct AlltoallBackward : public M4ANode {
  AlltoallBackward(int64_t gaxis, int64_t saxis, int64_t numelem)
      : gaxis(gaxis), saxis(saxis), numelem(numelem) {}
  std::string name() const override { return "M4AAlltoallBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // adjoint of alltoall is alltoall with the axes swapped
      // (reference :903-915); numelem = original gather-axis size
      out[0] = comm->Alltoall(grads[0], saxis, gaxis, numelem);
    }
    return out;
  }
  int64_t gaxis, saxis, numelem;
};

} // namespace

Tensor Communicator::AlltoallvImpl(const Tensor& input, int64_t gatheraxis,
                                   int64_t scatteraxis, int64_t numelem,
                                   const std::vector<int64_t>& target_counts,
                                   const std::vector<int64_t>& source_sizes) {
  gatheraxis = at::maybe_wrap_dim(gatheraxis, input.dim());
  scatteraxis = at::maybe_wrap_dim(scatteraxis, input.dim());
  const bool explicit_counts = !target_counts.empty();
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    if (explicit_counts) {
      grad_fn = make_node<AlltoallvBackward>(
          c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
          gatheraxis, scatteraxis, source_sizes, target_counts);
    } else {
      grad_fn = make_node<AlltoallBackward>(
          c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
          gatheraxis, scatteraxis, input.size(gatheraxis));
    }
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(in);
    if (w1_shortcut(tr)) {
      const int64_t want = explicit_counts ? target_counts[0] : numelem;
      TORCH_CHECK(want == in.size(scatteraxis),
                  "Alltoall: numelem must equal the scatter-axis size at "
                  "world size 1");
      return stager.from_comm(fast_clone(in));
    }
    const int me = tr.rank();
    const int P = tr.size();
    debug_check_axis_collective(group_name_, "Alltoall", in,
                                {gatheraxis, scatteraxis},
                                {gatheraxis, scatteraxis, explicit_counts});

    // What each rank wants along the scatter axis. With explicit counts
    // (Alltoallv) both vectors are caller-provided and the two host
    // round-trips are skipped — the expert-parallel hot path, where every
    // rank already knows the routing table.
    std::vector<int64_t> scounts;
    if (explicit_counts) {
      TORCH_CHECK((int)target_counts.size() == P,
                  "Alltoallv: target_counts must have world_size entries");
      TORCH_CHECK((int)source_sizes.size() == P,
                  "Alltoallv: source_sizes must have world_size entries");
      scounts = target_counts;
    } else {
      scounts = host_allgather_int64(group_name_, numelem);
    }
    auto sdispls = prefix_displs(scounts);

    std::vector<int64_t> s_offs(P), s_lens(P);  // my send slices (in `in`)
    std::vector<int64_t> r_offs(P), r_lens(P);  // my recv slices (in `out`)
    std::vector<int64_t> outsizes = in.sizes().vec();
    int64_t send_axis = scatteraxis, recv_axis = gatheraxis;
    std::vector<int64_t> srcsz;  // per-rank source-axis sizes (shared)

    if (gatheraxis != scatteraxis) {
      const int64_t stotal = sdispls.back() + scounts.back();
      TORCH_CHECK(in.size(scatteraxis) == stotal,
                  "Alltoall: scatter-axis size (", in.size(scatteraxis),
                  ") must equal the sum of per-rank numelem (", stotal, ")");
      auto gsizes = explicit_counts
                        ? source_sizes
                        : host_allgather_int64(group_name_,
                                               in.size(gatheraxis));
      TORCH_CHECK(gsizes[me] == in.size(gatheraxis),
                  "Alltoallv: source_sizes[rank] must equal the local "
                  "gather-axis size");
      auto gdispls = prefix_displs(gsizes);
      for (int j = 0; j < P; ++j) {
        s_offs[j] = sdispls[j];
        s_lens[j] = scounts[j];
        r_offs[j] = gdispls[j];
        r_lens[j] = gsizes[j];
      }
      outsizes[gatheraxis] = gdispls.back() + gsizes.back();
      outsizes[scatteraxis] = scounts[me];
      srcsz = gsizes;
    } else {
      // same-axis repartition (reference :947-979): ranks hold chunks of a
      // global axis; redistribute to the partition given by numelem
      auto nsizes = explicit_counts
                        ? source_sizes
                        : host_allgather_int64(group_name_,
                                               in.size(gatheraxis));
      TORCH_CHECK(nsizes[me] == in.size(gatheraxis),
                  "Alltoallv: source_sizes[rank] must equal the local "
                  "axis size");
      auto ndispls = prefix_displs(nsizes);
      const int64_t totaln = ndispls.back() + nsizes.back();
      const int64_t totalm = sdispls.back() + scounts.back();
      TORCH_CHECK(totaln == totalm,
                  "Alltoall (same axis): global axis length mismatch (",
                  totaln, " vs ", totalm, ")");
      const int64_t my_lo = ndispls[me], my_hi = my_lo + nsizes[me];
      const int64_t tgt_lo = sdispls[me], tgt_hi = tgt_lo + scounts[me];
      for (int j = 0; j < P; ++j) {
        // send: my chunk ∩ rank j's target interval
        const int64_t slo = std::max(my_lo, sdispls[j]);
        const int64_t shi = std::min(my_hi, sdispls[j] + scounts[j]);
        s_offs[j] = slo - my_lo;
        s_lens[j] = std::max<int64_t>(0, shi - slo);
        // recv: rank j's chunk ∩ my target interval
        const int64_t rlo = std::max(ndispls[j], tgt_lo);
        const int64_t rhi = std::min(ndispls[j] + nsizes[j], tgt_hi);
        r_offs[j] = rlo - tgt_lo;
        r_lens[j] = std::max<int64_t>(0, rhi - rlo);
      }
      outsizes[gatheraxis] = scounts[me];
      srcsz = nsizes;
    }

    auto out = at::empty(outsizes, in.options());
    const auto gs = axis_geom(in, send_axis);
    const auto gr = axis_geom(out, recv_axis);
    const bool send_packed = gs.before != 1;
    const bool recv_packed = gr.before != 1;
    auto sblocks = make_blocks(in, gs.before, gs.after, s_lens, s_offs, &in);
    auto rblocks = make_blocks(out, gr.before, gr.after, r_lens, r_offs, &out);
    auto peers = iota_peers(P);

    // ---- chunked pack -> wire pipelining (VERDICT/TODO task: overlap the
    // CDNA4 marshaling kernels with the wire). The marshaled side's slab
    // rows are split into K phases; each phase is its own full-width
    // grouped exchange (all peers, all links — no loss of multi-link
    // concurrency) issued non-blockingly, so pack(k+1) and unpack(k) run
    // on the compute stream while phase k rides the collective stream.
    // K is derived from SHARED quantities only (global logical tensor
    // size, common non-axis dims), so every rank slices every pair block
    // at identical byte offsets. Supported: exactly one marshaled side
    // (different axes), or both (same axis — rows coincide); the rare
    // both-marshaled different-axis case falls back to one phase.
    // SHARED marshaling flags. The LOCAL gs.before/gr.before can differ
    // across ranks in the different-axis case (the other, rank-sized axis
    // may lie inside `before`; a rank whose extent there is 1 sees
    // before==1). The phasing DECISION and the per-pair geometry selection
    // must be identical on every rank, so they use `before` computed with
    // the rank-dependent axis at its MAX over the shared size vectors;
    // the local pack/unpack still use the local flags (a 1-row rank just
    // contributes empty phases, which both endpoints compute identically).
    int64_t send_before_shared = 1, recv_before_shared = 1;
    {
      const int64_t src_max =
          *std::max_element(srcsz.begin(), srcsz.end());
      const int64_t sc_max =
          *std::max_element(scounts.begin(), scounts.end());
      auto insz = in.sizes();
      for (int64_t d = 0; d < send_axis; ++d) {
        send_before_shared *=
            (d == recv_axis && send_axis != recv_axis) ? src_max : insz[d];
      }
      for (int64_t d = 0; d < recv_axis; ++d) {
        recv_before_shared *= (d == scatteraxis && send_axis != recv_axis)
                                  ? sc_max
                                  : outsizes[d];
      }
    }
    const bool send_m = send_before_shared > 1;
    const bool recv_m = recv_before_shared > 1;
    int64_t K = 1;
    if ((send_m || recv_m) &&
        (send_axis == recv_axis || send_m != recv_m)) {
      int64_t global_elems = 1;
      for (size_t d = 0; d < outsizes.size(); ++d) {
        global_elems *= (d == (size_t)scatteraxis)
                            ? (sdispls.back() + scounts.back())
                            : outsizes[d];
      }
      K = phase_count(in, global_elems / P * in.element_size());
    }

    if (K > 1) {
      const int me_ = me;
      // per-pair row geometry of the marshaled side, from shared data.
      // Branch selection uses the SHARED flags (send_m/recv_m), never the
      // local before values — a rank whose local before is 1 must still
      // speak the globally-agreed phase geometry.
      auto send_geom = [&](int j) -> std::pair<int64_t, int64_t> {
        if (send_axis == recv_axis || send_m) {
          return {gs.before, s_lens[j] * gs.after};
        }
        // recv side is the marshaled one: receiver j's rows (its out dims
        // = common outsizes with the scatter axis at scounts[j])
        int64_t before = 1, after = 1;
        for (int64_t d = 0; d < (int64_t)outsizes.size(); ++d) {
          const int64_t sz =
              (d == scatteraxis) ? scounts[j] : outsizes[d];
          if (d < recv_axis) before *= sz;
          else if (d > recv_axis) after *= sz;
        }
        return {before, srcsz[me_] * after};
      };
      auto recv_geom = [&](int i) -> std::pair<int64_t, int64_t> {
        if (send_axis == recv_axis || recv_m) {
          return {gr.before, r_lens[i] * gr.after};
        }
        // send side is the marshaled one: sender i's rows (its in dims =
        // mine with the gather axis at srcsz[i])
        int64_t before = 1, after = 1;
        auto insz = in.sizes();
        for (int64_t d = 0; d < (int64_t)insz.size(); ++d) {
          const int64_t sz = (d == recv_axis) ? srcsz[i] : insz[d];
          if (d < send_axis) before *= sz;
          else if (d > send_axis) after *= sz;
        }
        return {before, scounts[me_] * after};
      };
      auto bound = [&](int64_t rows, int64_t k) { return rows * k / K; };
      auto slice = [](const Tensor& blk, int64_t lo, int64_t len) {
        auto flat = blk.view({-1});
        return len > 0 ? flat.narrow(0, lo, len) : flat.narrow(0, 0, 0);
      };
      std::vector<uint64_t> reqs((size_t)K);
      for (int64_t k = 0; k < K; ++k) {
        if (send_packed) {
          move_axis_blocks(in, send_axis, s_offs, s_lens, sblocks, true,
                           bound(gs.before, k), bound(gs.before, k + 1));
        }
        std::vector<Tensor> sk(P), rk(P);
        for (int j = 0; j < P; ++j) {
          auto sg = send_geom(j);
          sk[j] = slice(sblocks[j], bound(sg.first, k) * sg.second,
                        (bound(sg.first, k + 1) - bound(sg.first, k)) *
                            sg.second);
          auto rg = recv_geom(j);
          rk[j] = slice(rblocks[j], bound(rg.first, k) * rg.second,
                        (bound(rg.first, k + 1) - bound(rg.first, k)) *
                            rg.second);
        }
        reqs[(size_t)k] = tr.iexchange(sk, peers, rk, peers);
      }
      for (int64_t k = 0; k < K; ++k) {
        wait_request(reqs[(size_t)k]);
        if (recv_packed) {
          move_axis_blocks(out, recv_axis, r_offs, r_lens, rblocks, false,
                           bound(gr.before, k), bound(gr.before, k + 1));
        }
      }
      return stager.from_comm(std::move(out));
    }

    if (send_packed) {
      move_axis_blocks(in, send_axis, s_offs, s_lens, sblocks, /*pack=*/true);
    }
    tr.exchange(sblocks, peers, rblocks, peers);
    if (recv_packed) {
      move_axis_blocks(out, recv_axis, r_offs, r_lens, rblocks,
                       /*pack=*/false);
    }
    return stager.from_comm(std::move(out));
  }();
  attach_history(result, grad_fn);
  return result;
}

Tensor Communicator::Alltoall(const Tensor& input, int64_t gatheraxis,
                              int64_t scatteraxis, int64_t numelem) {
  return AlltoallvImpl(input, gatheraxis, scatteraxis, numelem, {}, {});
}

Tensor Communicator::Alltoallv(const Tensor& input, int64_t gatheraxis,
                               int64_t scatteraxis,
                               std::vector<int64_t> target_counts,
                               std::vector<int64_t> source_sizes) {
  TORCH_CHECK(!target_counts.empty(),
              "Alltoallv: target_counts must not be empty");
  return AlltoallvImpl(input, gatheraxis, scatteraxis,
                       /*numelem=*/-1, target_counts, source_sizes);
}


// ---------------------------------------------------------------------------
// AlltoallPairwise — the expert-parallel dispatch/combine primitive
// (MI355X extension; the reference's same-axis Alltoall can only
// repartition contiguous global intervals, reference :947-979).
// ---------------------------------------------------------------------------

namespace {
struct AlltoallPairwiseBackward : public M4ANode {
  AlltoallPairwiseBackward(int64_t axis, std::vector<int64_t> send,
                           std::vector<int64_t> recv)
      : axis(axis), send(std::move(send)), recv(std::move(recv)) {}
  std::string name() const override { return "M4AAlltoallPairwiseBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // adjoint: return every received slice to its sender — the count
      // matrix transposes, i.e. swap send/recv vectors
      out[0] = comm->AlltoallPairwise(grads[0], axis, recv, send);
    }
    return out;
  }
  int64_t axis;
  std::vector<int64_t> send, recv;
};
} // namespace

Tensor Communicator::AlltoallPairwise(const Tensor& input, int64_t axis,
                                      std::vector<int64_t> send_counts,
                                      std::vector<int64_t> recv_counts) {
  axis = at::maybe_wrap_dim(axis, input.dim());
  auto& tr0 = cpu_tr();
  const int P = tr0.size();
  TORCH_CHECK((int)send_counts.size() == P,
              "AlltoallPairwise: send_counts must have world_size entries");
  if (recv_counts.empty() && P > 1) {
    // exchange the count matrix; my recv from j = j's send to me
    auto mat = host_allgather_int64_vec(group_name_, send_counts);
    recv_counts.resize(P);
    const int me = tr0.rank();
    for (int j = 0; j < P; ++j) recv_counts[j] = mat[(int64_t)j * P + me];
  }
  if (P == 1 && recv_counts.empty()) recv_counts = send_counts;
  TORCH_CHECK((int)recv_counts.size() == P,
              "AlltoallPairwise: recv_counts must have world_size entries");

  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_node<AlltoallPairwiseBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
        axis, send_counts, recv_counts);
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto in = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(in);
    auto s_displs = prefix_displs(send_counts);
    auto r_displs = prefix_displs(recv_counts);
    const int64_t s_total = s_displs.back() + send_counts.back();
    const int64_t r_total = r_displs.back() + recv_counts.back();
    TORCH_CHECK(in.size(axis) == s_total,
                "AlltoallPairwise: sum of send_counts (", s_total,
                ") must equal the axis size (", in.size(axis), ")");
    auto outsizes = in.sizes().vec();
    outsizes[axis] = r_total;
    auto out = at::empty(outsizes, in.options());
    if (tr.size() == 1 && !config().force_full_path) {
      // world of one: send_counts == recv_counts, identity
      out.copy_(in);
      return stager.from_comm(std::move(out));
    }
    debug_check_axis_collective(group_name_, "AlltoallPairwise", in, {axis},
                                {axis});
    const auto g = axis_geom(in, axis);
    auto sblocks = make_blocks(in, g.before, g.after, send_counts, s_displs,
                               &in);
    if (g.before != 1) {
      move_axis_blocks(in, axis, s_displs, send_counts, sblocks,
                       /*pack=*/true);
    }
    const auto gr = axis_geom(out, axis);
    auto rblocks = make_blocks(out, gr.before, gr.after, recv_counts,
                               r_displs, &out);
    auto peers = iota_peers(tr.size());
    tr.exchange(sblocks, peers, rblocks, peers);
    if (gr.before != 1) {
      move_axis_blocks(out, axis, r_displs, recv_counts, rblocks,
                       /*pack=*/false);
    }
    return stager.from_comm(std::move(out));
  }();
  attach_history(result, grad_fn);
  return result;
}

// ---------------------------------------------------------------------------
// AlltoallPairwiseCompressed (MI355X extension; not in the reference API):
// AlltoallPairwise over the mxfp8 wire with the token permute fused into the
// codec kernels — the expert-parallel dispatch/combine primitive.
// ---------------------------------------------------------------------------

namespace {
struct AlltoallPairwiseCompressedBackward : public M4ANode {
  AlltoallPairwiseCompressedBackward(int64_t axis, std::vector<int64_t> send,
                                     std::vector<int64_t> recv,
                                     c10::optional<Tensor> send_order,
                                     c10::optional<Tensor> recv_order)
      : axis(axis), send(std::move(send)), recv(std::move(recv)),
        send_order(std::move(send_order)),
        recv_order(std::move(recv_order)) {}
  std::string name() const override {
    return "M4AAlltoallPairwiseCompressedBackward";
  }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      // exact adjoint of gather -> exchange -> scatter for permutations:
      // counts and orders swap; quantization is straight-through, and the
      // gradient itself travels compressed
      out[0] = comm->AlltoallPairwiseCompressed(grads[0], axis, recv, send,
                                                recv_order, send_order);
    }
    return out;
  }
  int64_t axis;
  std::vector<int64_t> send, recv;
  c10::optional<Tensor> send_order, recv_order;
};

// Shape, dtype and device always; the permutation property on the CPU, and
// on the GPU only under the desync detector's debug mode (it costs a sync).
void check_pairwise_order(const char* which,
                          const c10::optional<Tensor>& order, int64_t len,
                          const Tensor& input) {
  if (!order.has_value()) return;
  const Tensor& o = *order;
  TORCH_CHECK(o.dim() == 1 && o.numel() == len,
              "AlltoallPairwiseCompressed: ", which, " must be a 1-D tensor "
              "of length ", len, " (the sum of its counts), got shape ",
              o.sizes());
  TORCH_CHECK(o.scalar_type() == at::kLong,
              "AlltoallPairwiseCompressed: ", which, " must be an int64 "
              "tensor, got ", o.scalar_type());
  TORCH_CHECK(o.device() == input.device(),
              "AlltoallPairwiseCompressed: ", which, " must be on the "
              "tensor's device ", input.device(), ", got ", o.device());
  if (len > 0 && (!o.is_cuda() || config().debug_collectives)) {
    const bool perm = std::get<0>(o.sort()).equal(
        at::arange(len, o.options()));
    TORCH_CHECK(perm, "AlltoallPairwiseCompressed: ", which, " must be a "
                "permutation of 0..", len - 1);
  }
}
} // namespace

Tensor Communicator::AlltoallPairwiseCompressed(
    const Tensor& input, int64_t axis, std::vector<int64_t> send_counts,
    std::vector<int64_t> recv_counts, c10::optional<Tensor> send_order,
    c10::optional<Tensor> recv_order) {
  check_mx8_input("AlltoallPairwiseCompressed", input);
  axis = at::maybe_wrap_dim(axis, input.dim());
  auto& tr0 = cpu_tr();
  const int P = tr0.size();
  TORCH_CHECK((int)send_counts.size() == P,
              "AlltoallPairwiseCompressed: send_counts must have world_size "
              "entries");
  if (recv_counts.empty() && P > 1) {
    // exchange the count matrix; my recv from j = j's send to me
    auto mat = host_allgather_int64_vec(group_name_, send_counts);
    recv_counts.resize(P);
    const int me = tr0.rank();
    for (int j = 0; j < P; ++j) recv_counts[j] = mat[(int64_t)j * P + me];
  }
  if (P == 1 && recv_counts.empty()) recv_counts = send_counts;
  TORCH_CHECK((int)recv_counts.size() == P,
              "AlltoallPairwiseCompressed: recv_counts must have world_size "
              "entries");
  int64_t s_total = 0, r_total = 0;
  for (int64_t c : send_counts) {
    TORCH_CHECK(c >= 0, "AlltoallPairwiseCompressed: negative send count ", c);
    s_total += c;
  }
  for (int64_t c : recv_counts) {
    TORCH_CHECK(c >= 0, "AlltoallPairwiseCompressed: negative recv count ", c);
    r_total += c;
  }
  TORCH_CHECK(input.size(axis) == s_total,
              "AlltoallPairwiseCompressed: sum of send_counts (", s_total,
              ") must equal the axis size (", input.size(axis), ")");
  check_pairwise_order("send_order", send_order, s_total, input);
  check_pairwise_order("recv_order", recv_order, r_total, input);

  auto make_grad_fn = [&](auto comm) {
    return make_node<AlltoallPairwiseCompressedBackward>(
        comm, axis, send_counts, recv_counts, send_order, recv_order);
  };
  auto body = [&](Transport& tr, const Tensor& in,
                  const DeviceStager& stager) -> Tensor {
    // the order tensors follow the input through the stager
    c10::optional<Tensor> so, ro;
    if (send_order.has_value()) {
      so = stager.to_comm(*send_order).contiguous().variable_data();
    }
    if (recv_order.has_value()) {
      ro = stager.to_comm(*recv_order).contiguous().variable_data();
    }
    auto outsizes = in.sizes().vec();
    outsizes[axis] = r_total;
    // World of one: the result is the exact permutation, under the rule of
    // the uncompressed collectives — force_full_path runs the whole pipeline
    // on either device: mx8_quantize_segments, self-exchange,
    // mx8_dequantize_segments.
    if (w1_shortcut(tr)) {
      auto y = so.has_value() ? in.index_select(axis, *so) : fast_clone(in);
      if (ro.has_value()) {
        auto out = at::empty(outsizes, in.options());
        out.index_copy_(axis, *ro, y);
        y = out;
      }
      return y;
    }
    debug_check_axis_collective(group_name_, "AlltoallPairwiseCompressed",
                                in, {axis}, {axis});
    const auto g = axis_geom(in, axis);
    if (g.before * g.after == 0) return at::empty(outsizes, in.options());
    return mx8_alltoall_pairwise(tr, in, g.before, g.after, send_counts,
                                 recv_counts, so, ro)
        .view(outsizes);
  };
  return collective_frame(*this, input, make_grad_fn, body);
}

// ---------------------------------------------------------------------------
// Isend / Irecv / Wait (reference csrc/extension.cpp:1048-1265). The handle
// is the same 3-tensor contract [meta, buffer, input]; the MPI_Request
// becomes an entry in the request table (hipEvent on the p2p stream / c10d
// Work); the reference's backward tag offset (tag+10, ref :1161) becomes a
// dedicated backward RCCL communicator+stream (Channel::P2PBwd).
// ---------------------------------------------------------------------------

namespace {

constexpr int64_t kIsendOp = 0;
constexpr int64_t kIrecvOp = 1;
constexpr int64_t kIallreduceOp = 2;

double ptr_hash(const void* p) {
  return (double)(0xFFFFFFFFull & std::hash<const void*>()(p));
}

struct NonBlockingBackward : public M4ANode {
  std::string name() const override { return "M4ANonBlockingBackward"; }
  variable_list apply(variable_list&& grads) override {
    variable_list out(1);
    if (should_compute_output(0)) {
      TORCH_CHECK(grads.size() == 3 && grads[0].defined() &&
                      grads[1].defined() && grads[2].defined(),
                  "mpi4torch_amd: backward reached Isend/Irecv without a "
                  "matching Wait in the graph");
      // the incoming gradients ARE a wait handle produced by WaitBackward's
      // reverse transfer; completing it yields the input gradient
      out[0] = comm->Wait({grads[0], grads[1], grads[2]});
    }
    return out;
  }
};

struct WaitBackward : public M4ANode {
  WaitBackward(int64_t op, int64_t peer, int64_t tag,
               std::vector<int64_t> buf_sizes, at::TensorOptions buf_options)
      : op(op), peer(peer), tag(tag), buf_sizes(std::move(buf_sizes)),
        buf_options(buf_options) {}
  std::string name() const override { return "M4AWaitBackward"; }
  variable_list apply(variable_list&& grads) override;
  int64_t op, peer, tag;
  std::vector<int64_t> buf_sizes;
  at::TensorOptions buf_options;
};

variable_list WaitBackward::apply(variable_list&& grads) {
  if (!(should_compute_output(0) || should_compute_output(1) ||
        should_compute_output(2))) {
    return variable_list(3);
  }
  // Bifurcation detection, as in the reference (ref :1196-1202): the buffer
  // slot of the handle must flow straight from Isend/Irecv; any arithmetic
  // on it would have cloned the buffer and detached the real transfer.
  auto next_node = next_edge(1).function;
  TORCH_CHECK(next_node && next_node->name() == "M4ANonBlockingBackward",
              "mpi4torch_amd: detected bifurcation in Wait-handle usage; "
              "the next node in the DAG should be M4ANonBlockingBackward "
              "but is ",
              next_node ? next_node->name() : "<null>",
              ". Only JoinDummiesHandle may be applied to a wait handle.");
  TORCH_CHECK(op != kIallreduceOp,
              "mpi4torch_amd: Iallreduce handles carry no gradient");
  if (op == kIsendOp) {
    // adjoint of send is receive (on the dedicated backward channel)
    auto buf = at::zeros(buf_sizes, buf_options);
    return comm->IrecvImpl(join_dummies(buf, grads), peer, tag,
                           /*backward_channel=*/true);
  }
  // adjoint of receive is send of the incoming gradient
  return comm->IsendImpl(grads[0], peer, tag, /*backward_channel=*/true);
}

} // namespace

std::vector<at::Tensor> Communicator::IsendImpl(const Tensor& input,
                                                int64_t dest, int64_t tag,
                                                bool backward_channel) {
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_node<NonBlockingBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this));
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto buf = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(buf);
    const Channel ch = backward_channel ? Channel::P2PBwd : Channel::P2P;
    uint64_t req = tr.isend(buf, (int)dest, (int)tag, ch);
    auto meta = at::empty({7}, at::TensorOptions().dtype(at::kDouble));
    auto* m = meta.data_ptr<double>();
    m[0] = (double)req;
    m[1] = (double)kIsendOp;
    m[2] = (double)dest;
    m[3] = (double)tag;
    m[4] = ptr_hash(buf.data_ptr());
    m[5] = (double)(int64_t)stager.orig_device_.type();
    m[6] = (double)stager.orig_device_.index();
    // [meta, live buffer, original input] — the buffer reference keeps the
    // transfer's memory alive until Wait (reference :1094-1107)
    return std::vector<Tensor>{meta, buf, input.variable_data()};
  }();
  if (grad_fn) {
    torch::autograd::set_history(result, grad_fn);
  }
  return result;
}

std::vector<at::Tensor> Communicator::IrecvImpl(const Tensor& input,
                                                int64_t source, int64_t tag,
                                                bool backward_channel) {
  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(input)) {
    grad_fn = make_node<NonBlockingBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this));
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(input));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    DeviceStager stager(input);
    auto buf = stager.to_comm(input).contiguous().variable_data();
    auto& tr = tr_for(buf);
    const Channel ch = backward_channel ? Channel::P2PBwd : Channel::P2P;
    uint64_t req = tr.irecv(buf, (int)source, (int)tag, ch);
    auto meta = at::empty({7}, at::TensorOptions().dtype(at::kDouble));
    auto* m = meta.data_ptr<double>();
    m[0] = (double)req;
    m[1] = (double)kIrecvOp;
    m[2] = (double)source;
    m[3] = (double)tag;
    m[4] = ptr_hash(buf.data_ptr());
    m[5] = (double)(int64_t)stager.orig_device_.type();
    m[6] = (double)stager.orig_device_.index();
    return std::vector<Tensor>{meta, buf, input.variable_data()};
  }();
  if (grad_fn) {
    torch::autograd::set_history(result, grad_fn);
  }
  return result;
}

std::vector<at::Tensor> Communicator::Iallreduce(const Tensor& input,
                                                 int64_t op) {
  check_op(op);
  TORCH_CHECK(!torch::autograd::compute_requires_grad(input),
              "mpi4torch_amd: Iallreduce does not support autograd; use "
              "Allreduce, or detach the input (gradient buckets are already "
              "grad tensors)");
  at::AutoDispatchBelowADInplaceOrView guard;
  DeviceStager stager(input);
  auto in = stager.to_comm(input).contiguous().variable_data();
  auto& tr = tr_for(in);
  TORCH_CHECK(is_arith(op) && native_reduce_dtype(tr, in.scalar_type()),
              "mpi4torch_amd: Iallreduce supports native arithmetic "
              "reductions only (op ", red_op_name(op), ", dtype ",
              in.scalar_type(), ")");
  auto out = at::empty_like(in);
  uint64_t req = tr.iallreduce(in, out, (RedOp)op);
  auto meta = at::empty({7}, at::TensorOptions().dtype(at::kDouble));
  auto* m = meta.data_ptr<double>();
  m[0] = (double)req;
  m[1] = (double)kIallreduceOp;
  m[2] = 0.0;
  m[3] = 0.0;
  m[4] = ptr_hash(out.data_ptr());
  m[5] = (double)(int64_t)stager.orig_device_.type();
  m[6] = (double)stager.orig_device_.index();
  return {meta, out, in};
}

std::vector<at::Tensor> Communicator::Ireducescatter(const Tensor& input,
                                                     int64_t op) {
  check_op(op);
  TORCH_CHECK(!torch::autograd::compute_requires_grad(input),
              "mpi4torch_amd: Ireducescatter does not support autograd");
  at::AutoDispatchBelowADInplaceOrView guard;
  DeviceStager stager(input);
  auto in = stager.to_comm(input).contiguous().variable_data();
  auto& tr = tr_for(in);
  TORCH_CHECK(in.numel() % tr.size() == 0,
              "Ireducescatter: numel must be divisible by world size");
  TORCH_CHECK(is_arith(op) && native_reduce_dtype(tr, in.scalar_type()),
              "mpi4torch_amd: Ireducescatter supports native arithmetic "
              "reductions only");
  auto out = at::empty({in.numel() / tr.size()}, in.options());
  uint64_t req = tr.ireduce_scatter(in, out, (RedOp)op);
  auto meta = at::empty({7}, at::TensorOptions().dtype(at::kDouble));
  auto* m = meta.data_ptr<double>();
  m[0] = (double)req;
  m[1] = (double)kIallreduceOp;  // same wait semantics: handle returns buffer
  m[2] = 0.0;
  m[3] = 0.0;
  m[4] = ptr_hash(out.data_ptr());
  m[5] = (double)(int64_t)stager.orig_device_.type();
  m[6] = (double)stager.orig_device_.index();
  return {meta, out, in};
}

std::vector<at::Tensor> Communicator::Iallgather(const Tensor& input) {
  TORCH_CHECK(!torch::autograd::compute_requires_grad(input),
              "mpi4torch_amd: Iallgather does not support autograd; use "
              "Allgather, or detach the input (FSDP parameter prefetch "
              "operates on detached shards)");
  at::AutoDispatchBelowADInplaceOrView guard;
  DeviceStager stager(input);
  auto in = stager.to_comm(input).contiguous().variable_data();
  auto& tr = tr_for(in);
  auto out = at::empty({(int64_t)tr.size() * in.numel()}, in.options());
  uint64_t req = tr.iallgather(in, out);
  auto meta = at::empty({7}, at::TensorOptions().dtype(at::kDouble));
  auto* m = meta.data_ptr<double>();
  m[0] = (double)req;
  m[1] = (double)kIallreduceOp;  // same wait semantics: handle returns buffer
  m[2] = 0.0;
  m[3] = 0.0;
  m[4] = ptr_hash(out.data_ptr());
  m[5] = (double)(int64_t)stager.orig_device_.type();
  m[6] = (double)stager.orig_device_.index();
  return {meta, out, in};
}

std::vector<at::Tensor> Communicator::Isend(const Tensor& input, int64_t dest,
                                            int64_t tag) {
  return IsendImpl(input, dest, tag, /*backward_channel=*/false);
}

std::vector<at::Tensor> Communicator::Irecv(const Tensor& input,
                                            int64_t source, int64_t tag) {
  return IrecvImpl(input, source, tag, /*backward_channel=*/false);
}

Tensor Communicator::Wait(const std::vector<Tensor>& handle) {
  TORCH_CHECK(handle.size() == 3,
              "mpi4torch_amd: Wait expects the 3-tensor handle returned by "
              "Isend/Irecv");
  const auto& meta = handle[0];
  TORCH_CHECK(meta.device().is_cpu() && meta.scalar_type() == at::kDouble &&
                  meta.numel() == 7,
              "mpi4torch_amd: corrupted wait handle metadata");
  const double* m = meta.data_ptr<double>();
  const uint64_t req = (uint64_t)m[0];
  const int64_t op = (int64_t)m[1];
  const int64_t peer = (int64_t)m[2];
  const int64_t tag = (int64_t)m[3];
  const c10::Device orig_device((c10::DeviceType)(int64_t)m[5],
                                (c10::DeviceIndex)(int64_t)m[6]);
  // Handle-bifurcation misuse detection via the buffer-pointer hash
  // (reference :1231-1237).
  TORCH_CHECK(m[4] == ptr_hash(handle[1].data_ptr()),
              "mpi4torch_amd: detected bifurcation in Wait-handle usage; "
              "modifying or consuming the handle by anything other than "
              "Wait/JoinDummiesHandle is prohibited");

  std::shared_ptr<M4ANode> grad_fn;
  if (torch::autograd::compute_requires_grad(handle)) {
    grad_fn = make_node<WaitBackward>(
        c10::intrusive_ptr<Communicator>::unsafe_reclaim_from_nonowning(this),
        op, peer, tag, handle[1].sizes().vec(), handle[1].options());
    grad_fn->set_next_edges(torch::autograd::collect_next_edges(handle));
  }
  auto result = [&]() {
    at::AutoDispatchBelowADInplaceOrView guard;
    wait_request(req);
    if (op == kIsendOp) {
      return handle[2].variable_data();
    }
    // kIrecvOp and kIallreduceOp both return the (possibly unstaged) buffer
    auto buf = handle[1];
    if (buf.device() != orig_device) {
      buf = buf.to(orig_device);
    }
    return buf.variable_data();
  }();
  attach_history(result, grad_fn);
  return result;
}


// ---------------------------------------------------------------------------
// Debug/test entry points: exercise the CDNA4 kernels directly on one GPU
// (world-size-independent numerics tests; see tests/test_gpu.py).
// ---------------------------------------------------------------------------

Tensor debug_pack_roundtrip(const Tensor& input, int64_t axis,
                            std::vector<int64_t> counts) {
  auto in = input.contiguous();
  axis = at::maybe_wrap_dim(axis, in.dim());
  const auto g = axis_geom(in, axis);
  auto displs = prefix_displs(counts);
  TORCH_CHECK(displs.back() + counts.back() == g.axis,
              "counts must partition the axis");
  auto blocks = make_blocks(in, g.before, g.after, counts, displs, nullptr);
  move_axis_blocks(in, axis, displs, counts, blocks, /*pack=*/true);
  auto out = at::zeros_like(in);
  move_axis_blocks(out, axis, displs, counts, blocks, /*pack=*/false);
  return out;
}

// The unpack Allgather runs after an equal-count gather with before > 1:
// staging holds P rank-major blocks of [rows, row_elems]; block r goes to
// out[:, r, :] (one move_axis_blocks call, one slab-copy launch on GPU).
void debug_unpack_blocks(const Tensor& staging, const Tensor& out) {
  TORCH_CHECK(out.dim() == 3 && out.is_contiguous() && staging.dim() == 1 &&
                  staging.is_contiguous() &&
                  staging.numel() == out.numel() &&
                  staging.scalar_type() == out.scalar_type() &&
                  staging.device() == out.device(),
              "debug_unpack_blocks expects flat staging [P*rows*row_elems] "
              "and a contiguous out [rows, P, row_elems] of the same dtype "
              "and device");
  const int64_t rows = out.size(0), P = out.size(1), re = out.size(2);
  if (out.numel() == 0) return;
  auto full = out.view({rows, P * re});
  std::vector<int64_t> counts((size_t)P, re);
  auto displs = prefix_displs(counts);
  std::vector<Tensor> blocks((size_t)P);
  for (int64_t r = 0; r < P; ++r) {
    blocks[(size_t)r] = staging.narrow(0, r * rows * re, rows * re);
  }
  move_axis_blocks(full, 1, displs, counts, blocks, /*pack=*/false);
}

// The mirror: the rank-major axis pack of an equal-count Reducescatter or
// Alltoall (the pass mx8_quantize_blocks makes unnecessary).
void debug_pack_blocks(const Tensor& in, const Tensor& staging) {
  TORCH_CHECK(in.dim() == 3 && in.is_contiguous() && staging.dim() == 1 &&
                  staging.is_contiguous() &&
                  staging.numel() == in.numel() &&
                  staging.scalar_type() == in.scalar_type() &&
                  staging.device() == in.device(),
              "debug_pack_blocks expects a contiguous in [rows, P, row_elems] "
              "and flat staging [P*rows*row_elems] of the same dtype and "
              "device");
  const int64_t rows = in.size(0), P = in.size(1), re = in.size(2);
  if (in.numel() == 0) return;
  auto full = in.view({rows, P * re});
  std::vector<int64_t> counts((size_t)P, re);
  auto displs = prefix_displs(counts);
  std::vector<Tensor> blocks((size_t)P);
  for (int64_t r = 0; r < P; ++r) {
    blocks[(size_t)r] = staging.narrow(0, r * rows * re, rows * re);
  }
  move_axis_blocks(full, 1, displs, counts, blocks, /*pack=*/true);
}

// One launch_slab_copy call over caller-chosen descriptors (byte offsets
// into two flat uint8 tensors). Every descriptor is bounds-checked on the
// host before anything is launched, so a wrong test raises instead of
// touching memory outside the tensors.
void debug_slab_copy(const Tensor& src, const Tensor& dst,
                     const std::vector<std::vector<int64_t>>& descs) {
  TORCH_CHECK(src.is_cuda() && dst.is_cuda() && src.device() == dst.device(),
              "debug_slab_copy is a GPU kernel test");
  TORCH_CHECK(src.scalar_type() == at::kByte && dst.scalar_type() == at::kByte &&
                  src.dim() == 1 && dst.dim() == 1 && src.is_contiguous() &&
                  dst.is_contiguous(),
              "debug_slab_copy expects flat contiguous uint8 tensors");
  constexpr int64_t kMaxBytes = int64_t(1) << 31;  // keeps the products exact
  TORCH_CHECK(src.numel() < kMaxBytes && dst.numel() < kMaxBytes);
  const char* sbase = static_cast<const char*>(src.data_ptr());
  char* dbase = static_cast<char*>(dst.data_ptr());
  TORCH_CHECK(sbase + src.numel() <= dbase || dbase + dst.numel() <= sbase,
              "debug_slab_copy: src and dst overlap");
  // [begin, end) of the bytes a slab spans on one side; empty slabs span
  // nothing but must still start inside the tensor
  auto span = [](int64_t off, int64_t before, int64_t row_b, int64_t pitch,
                 int64_t numel, size_t i, const char* side) {
    TORCH_CHECK(off >= 0 && off <= numel && before >= 0 && before <= numel &&
                    row_b >= 0 && row_b <= numel && pitch >= 0 &&
                    pitch <= numel,
                "debug_slab_copy: descriptor ", i, " out of range on ", side);
    if (before == 0 || row_b == 0) return std::make_pair(off, off);
    const int64_t end = off + (before - 1) * pitch + row_b;
    TORCH_CHECK(end <= numel, "debug_slab_copy: descriptor ", i,
                " runs past the end of ", side);
    return std::make_pair(off, end);
  };
  std::vector<SlabDesc> slabs;
  std::vector<std::pair<int64_t, int64_t>> dspans;
  slabs.reserve(descs.size());
  for (size_t i = 0; i < descs.size(); ++i) {
    const auto& t = descs[i];
    TORCH_CHECK(t.size() == 7,
                "debug_slab_copy: descriptor is (src_off, dst_off, before, "
                "count, after_b, src_pitch_b, dst_pitch_b)");
    const int64_t before = t[2], count = t[3], after_b = t[4];
    TORCH_CHECK(count >= 0 && after_b >= 0 &&
                    (count == 0 || after_b <= kMaxBytes / count),
                "debug_slab_copy: descriptor ", i, " row size out of range");
    const int64_t row_b = count * after_b;
    span(t[0], before, row_b, t[5], src.numel(), i, "src");
    const auto d = span(t[1], before, row_b, t[6], dst.numel(), i, "dst");
    TORCH_CHECK(before <= 1 || row_b == 0 || t[6] >= row_b,
                "debug_slab_copy: descriptor ", i, " dst rows overlap");
    if (d.second > d.first) dspans.push_back(d);
    SlabDesc s;
    s.src = sbase + t[0];
    s.dst = dbase + t[1];
    s.before = before;
    s.count = count;
    s.after_b = after_b;
    s.src_pitch_b = t[5];
    s.dst_pitch_b = t[6];
    slabs.push_back(s);
  }
  std::sort(dspans.begin(), dspans.end());
  for (size_t i = 1; i < dspans.size(); ++i) {
    TORCH_CHECK(dspans[i - 1].second <= dspans[i].first,
                "debug_slab_copy: destination ranges overlap");
  }
  TORCH_CHECK(slabs.size() < (size_t)std::numeric_limits<int>::max());
  if (slabs.empty()) return;
  launch_slab_copy(slabs.data(), (int)slabs.size(), current_gpu_stream(src));
}

Tensor debug_fp8_reduce(const Tensor& stacked, int64_t op) {
  TORCH_CHECK(stacked.is_cuda(), "debug_fp8_reduce is a GPU kernel test");
  TORCH_CHECK(stacked.dim() >= 2);
  TORCH_CHECK(stacked.scalar_type() == at::kFloat8_e4m3fn ||
              stacked.scalar_type() == at::kFloat8_e5m2);
  auto in = stacked.contiguous();
  const int64_t n = in.size(0);
  auto out = at::empty(in.sizes().slice(1).vec(), in.options());
  launch_fp8_reduce(in.data_ptr(), out.data_ptr(), out.numel(), (int)n,
                    (int)op, in.scalar_type() == at::kFloat8_e5m2,
                    current_gpu_stream(in));
  return out;
}

// own: [n] (any element alignment, e.g. an offset view of a larger buffer);
// staged: [nranks-1, n] with a contiguous last axis, row stride free.
Tensor debug_arith_reduce(const Tensor& own, const Tensor& staged, int64_t me,
                          int64_t op) {
  TORCH_CHECK(own.is_cuda() && staged.is_cuda(),
              "debug_arith_reduce is a GPU kernel test");
  TORCH_CHECK(own.dim() == 1 && staged.dim() == 2 &&
              staged.size(1) == own.size(0) &&
              staged.scalar_type() == own.scalar_type() &&
              own.stride(0) == 1 && (staged.size(1) <= 1 || staged.stride(1) == 1),
              "debug_arith_reduce expects own [n] and staged [nranks-1, n]");
  TORCH_CHECK(arith_float_dtype(own.scalar_type()) && is_arith(op));
  const int64_t nranks = staged.size(0) + 1;
  TORCH_CHECK(me >= 0 && me < nranks);
  auto out = at::empty({own.size(0)}, own.options());
  launch_arith_reduce(own.data_ptr(), staged.data_ptr(),
                      nranks > 1 ? staged.stride(0) : 0, (int)nranks, (int)me,
                      out.data_ptr(), own.size(0), arith_op_code(op),
                      arith_dtype_code(own.scalar_type()),
                      current_gpu_stream(own));
  return out;
}

namespace {
// The canary tests' caller buffers: the codec writes the first `need`
// elements in place. `what` names that count in the binding's message.
void check_canary_out(const char* binding, const Tensor& o, int64_t need,
                      at::ScalarType dtype, const at::Device& dev,
                      const char* what) {
  TORCH_CHECK(o.dim() == 1 && o.is_contiguous() && o.numel() >= need &&
                  o.scalar_type() == dtype && o.device() == dev,
              binding, ": out must be a flat contiguous tensor of the "
              "requested dtype with at least ", what, " elements");
}

void check_canary_wire(const char* binding, const Tensor& po, const Tensor& so,
                       int64_t groups, const at::Device& dev,
                       const char* what) {
  auto ok = [&](const Tensor& t, int64_t need) {
    return t.dim() == 1 && t.is_contiguous() &&
           t.scalar_type() == at::kByte && t.numel() >= need &&
           t.device() == dev;
  };
  TORCH_CHECK(ok(po, groups * 32) && ok(so, groups), binding,
              ": payload_out and scales_out must be flat contiguous uint8 "
              "tensors with at least ", what, " elements");
}
} // namespace

std::tuple<Tensor, Tensor> debug_mx8_quantize(const Tensor& x) {
  auto ps = mx8_quantize(x.contiguous().view({-1}));
  return std::make_tuple(ps.first, ps.second);
}

std::tuple<Tensor, Tensor> debug_mx8_reduce(const Tensor& payload,
                                            const Tensor& scales) {
  TORCH_CHECK(payload.dim() == 2 && scales.dim() == 2 &&
                  payload.scalar_type() == at::kByte &&
                  scales.scalar_type() == at::kByte &&
                  payload.size(0) == scales.size(0) &&
                  payload.size(1) == scales.size(1) * 32,
              "debug_mx8_reduce expects uint8 payload [P, G*32] and "
              "scales [P, G]");
  auto pin = payload.contiguous();
  auto sin = scales.contiguous();
  const int64_t P = sin.size(0), n = sin.size(1);
  TORCH_CHECK(P >= 1);
  auto pout = at::empty({n * 32}, pin.options());
  auto sout = at::empty({n}, sin.options());
  mx8_reduce(pin.view({-1}), sin.view({-1}), pout, sout, n, (int)P);
  return std::make_tuple(pout, sout);
}

Tensor debug_mx8_dequantize(const Tensor& payload, const Tensor& scales,
                            int64_t numel, at::ScalarType dtype,
                            const c10::optional<Tensor>& out) {
  TORCH_CHECK(payload.scalar_type() == at::kByte &&
                  scales.scalar_type() == at::kByte &&
                  payload.numel() == scales.numel() * 32 &&
                  numel >= 0 && numel <= payload.numel() &&
                  (numel + 31) / 32 == scales.numel(),
              "debug_mx8_dequantize expects uint8 payload [G*32], scales "
              "[G] and numel in (32*(G-1), 32*G]");
  auto pay = payload.contiguous().view({-1});
  auto sc = scales.contiguous().view({-1});
  if (!out.has_value()) return mx8_dequantize(pay, sc, numel, dtype);
  check_canary_out("debug_mx8_dequantize", *out, numel, dtype, pay.device(),
                   "numel");
  return mx8_dequantize(pay, sc, numel, dtype, out->narrow(0, 0, numel));
}

Tensor debug_mx8_reduce_to(const Tensor& payload, const Tensor& scales,
                           int64_t numel, at::ScalarType dtype,
                           const c10::optional<Tensor>& out) {
  TORCH_CHECK(payload.dim() == 2 && scales.dim() == 2 &&
                  payload.scalar_type() == at::kByte &&
                  scales.scalar_type() == at::kByte &&
                  payload.size(0) == scales.size(0) && scales.size(0) >= 1 &&
                  payload.size(1) == scales.size(1) * 32 && numel >= 0 &&
                  (numel + 31) / 32 == scales.size(1),
              "debug_mx8_reduce_to expects uint8 payload [P, G*32], scales "
              "[P, G] and numel in (32*(G-1), 32*G]");
  auto pin = payload.contiguous().view({-1});
  auto sin = scales.contiguous().view({-1});
  const int P = (int)scales.size(0);
  if (!out.has_value()) return mx8_reduce_to(pin, sin, numel, P, dtype);
  check_canary_out("debug_mx8_reduce_to", *out, numel, dtype, pin.device(),
                   "numel");
  return mx8_reduce_to(pin, sin, numel, P, dtype, out->narrow(0, 0, numel));
}

Tensor debug_mx8_dequantize_blocks(const Tensor& payload,
                                   const Tensor& scales, int64_t rows,
                                   int64_t row_elems, at::ScalarType dtype,
                                   const c10::optional<Tensor>& out) {
  TORCH_CHECK(payload.dim() == 2 && scales.dim() == 2 &&
                  payload.scalar_type() == at::kByte &&
                  scales.scalar_type() == at::kByte &&
                  payload.size(0) == scales.size(0) && scales.size(0) >= 1 &&
                  scales.size(0) <= 65535 &&
                  payload.size(1) == scales.size(1) * 32 && rows >= 1 &&
                  row_elems >= 1 &&
                  (rows * row_elems + 31) / 32 == scales.size(1),
              "debug_mx8_dequantize_blocks expects uint8 payload [P, Gb*32], "
              "scales [P, Gb] and rows*row_elems in (32*(Gb-1), 32*Gb]");
  auto pin = payload.contiguous().view({-1});
  auto sin = scales.contiguous().view({-1});
  const int P = (int)scales.size(0);
  if (!out.has_value()) {
    return mx8_dequantize_blocks(pin, sin, P, rows, row_elems, dtype);
  }
  const int64_t total = rows * P * row_elems;
  check_canary_out("debug_mx8_dequantize_blocks", *out, total, dtype,
                   pin.device(), "rows*P*row_elems");
  return mx8_dequantize_blocks(
      pin, sin, P, rows, row_elems, dtype,
      out->narrow(0, 0, total).view({rows, (int64_t)P, row_elems}));
}

std::tuple<Tensor, Tensor> debug_mx8_quantize_blocks(
    const Tensor& x, int64_t nblocks, int64_t rows, int64_t row_elems,
    const c10::optional<Tensor>& payload_out,
    const c10::optional<Tensor>& scales_out) {
  TORCH_CHECK(x.dim() == 1 && x.is_contiguous() && nblocks >= 1 &&
                  nblocks <= 65535 && rows >= 1 && row_elems >= 1 &&
                  x.numel() == rows * nblocks * row_elems,
              "debug_mx8_quantize_blocks expects a flat contiguous tensor of "
              "rows*nblocks*row_elems elements and 1..65535 blocks");
  TORCH_CHECK(payload_out.has_value() == scales_out.has_value(),
              "debug_mx8_quantize_blocks: payload_out and scales_out go "
              "together");
  const int P = (int)nblocks;
  if (!payload_out.has_value()) {
    auto ps = mx8_quantize_blocks(x, P, rows, row_elems);
    return std::make_tuple(ps.first, ps.second);
  }
  const int64_t Gb = (rows * row_elems + 31) / 32;
  check_canary_wire("debug_mx8_quantize_blocks", *payload_out, *scales_out,
                    nblocks * Gb, x.device(), "P*Gb*32 and P*Gb");
  auto ps = mx8_quantize_blocks(
      x, P, rows, row_elems,
      payload_out->narrow(0, 0, nblocks * Gb * 32).view({nblocks, Gb * 32}),
      scales_out->narrow(0, 0, nblocks * Gb).view({nblocks, Gb}));
  return std::make_tuple(ps.first, ps.second);
}

std::tuple<Tensor, Tensor> debug_mx8_quantize_segments(
    const Tensor& x, int64_t rows, int64_t after,
    std::vector<int64_t> counts, const c10::optional<Tensor>& order,
    const c10::optional<Tensor>& payload_out,
    const c10::optional<Tensor>& scales_out) {
  TORCH_CHECK(x.dim() == 1 && x.is_contiguous() && rows >= 1 && after >= 1 &&
                  x.numel() % (rows * after) == 0,
              "debug_mx8_quantize_segments expects a flat contiguous tensor "
              "of rows*S*after elements");
  TORCH_CHECK(payload_out.has_value() == scales_out.has_value(),
              "debug_mx8_quantize_segments: payload_out and scales_out go "
              "together");
  const auto pl = mx8_seg_plan(counts, rows, after);
  const int64_t S = x.numel() / (rows * after);
  if (order.has_value()) {
    TORCH_CHECK(order->dim() == 1 && order->numel() == pl.slices &&
                    order->scalar_type() == at::kLong &&
                    order->is_contiguous() && order->device() == x.device(),
                "debug_mx8_quantize_segments: order must be a contiguous "
                "int64 tensor of sum(counts) entries on x's device");
  } else {
    TORCH_CHECK(pl.slices == S, "debug_mx8_quantize_segments: sum(counts) "
                "must equal the number of slices ", S);
  }
  if (payload_out.has_value()) {
    check_canary_wire("debug_mx8_quantize_segments", *payload_out,
                      *scales_out, pl.total_groups, x.device(),
                      "32*sum(G) and sum(G)");
  }
  auto ps = mx8_quantize_segments(x, rows, after, counts, order, payload_out,
                                  scales_out);
  return std::make_tuple(ps.first, ps.second);
}

Tensor debug_mx8_dequantize_segments(const Tensor& payload,
                                     const Tensor& scales, int64_t rows,
                                     int64_t after,
                                     std::vector<int64_t> counts,
                                     at::ScalarType dtype,
                                     const c10::optional<Tensor>& order,
                                     const c10::optional<Tensor>& out) {
  TORCH_CHECK(rows >= 1 && after >= 1,
              "debug_mx8_dequantize_segments: rows and after must be >= 1");
  const auto pl = mx8_seg_plan(counts, rows, after);
  TORCH_CHECK(payload.dim() == 1 && scales.dim() == 1 &&
                  payload.is_contiguous() && scales.is_contiguous() &&
                  payload.scalar_type() == at::kByte &&
                  scales.scalar_type() == at::kByte &&
                  payload.numel() == pl.total_groups * 32 &&
                  scales.numel() == pl.total_groups &&
                  payload.device() == scales.device(),
              "debug_mx8_dequantize_segments expects flat contiguous uint8 "
              "payload [32*sum(G)] and scales [sum(G)]");
  if (order.has_value()) {
    TORCH_CHECK(order->dim() == 1 && order->numel() == pl.slices &&
                    order->scalar_type() == at::kLong &&
                    order->is_contiguous() &&
                    order->device() == payload.device(),
                "debug_mx8_dequantize_segments: order must be a contiguous "
                "int64 tensor of sum(counts) entries on the payload's "
                "device");
  }
  if (!out.has_value()) {
    return mx8_dequantize_segments(payload, scales, rows, after, counts, order,
                                   dtype);
  }
  const int64_t total = rows * pl.slices * after;
  check_canary_out("debug_mx8_dequantize_segments", *out, total, dtype,
                   payload.device(), "rows*R*after");
  auto head = out->narrow(0, 0, total).view({rows, pl.slices, after});
  return mx8_dequantize_segments(payload, scales, rows, after, counts, order,
                                 dtype, head);
}

Tensor debug_pairloc_reduce(const Tensor& stacked, int64_t op) {
  TORCH_CHECK(stacked.dim() >= 2 && stacked.size(-1) == 2,
              "debug_pairloc_reduce expects [nranks, ..., 2] pairs");
  auto in = stacked.contiguous();
  const int64_t n = in.size(0);
  auto out_sizes = in.sizes().slice(1).vec();
  if (in.is_cuda()) {
    auto out = at::empty(out_sizes, in.options());
    launch_pairloc_reduce(in.data_ptr(), out.data_ptr(), out.numel() / 2,
                          (int)n, (int)op,
                          pairloc_dtype_code(in.scalar_type()),
                          current_gpu_stream(in));
    return out;
  }
  // CPU composite (the gloo transport's path)
  return pairloc_local_reduce(in.view({n, -1, 2}), op, in.scalar_type())
      .view(out_sizes)
      .contiguous();
}

Tensor debug_bitwise_reduce(const Tensor& stacked, int64_t op) {
  TORCH_CHECK(stacked.is_cuda(), "debug_bitwise_reduce is a GPU kernel test");
  TORCH_CHECK(stacked.dim() >= 2);
  auto in = stacked.contiguous();
  const int64_t n = in.size(0);
  auto out = at::empty(in.sizes().slice(1).vec(), in.options());
  const int64_t chunk_bytes = out.numel() * out.element_size();
  launch_bitwise_reduce(in.data_ptr(), out.data_ptr(), chunk_bytes, (int)n,
                        (int)op, current_gpu_stream(in));
  return out;
}

} // namespace m4a
