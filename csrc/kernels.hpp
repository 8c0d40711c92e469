// Host-side declarations for the CDNA4 (gfx950) HIP kernels in kernels.hip.
// This header is torch-free so the device TU stays minimal.
#pragma once

#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace m4a {

// Describes one slab of a batched strided copy: the MI355X-native
// replacement for the reference's MPI derived-datatype marshaling
// (MPI_Type_vector + MPI_Type_create_resized, reference
// csrc/extension.cpp:556-577, 691-712, 839-861).
//
// Copies, for b in [0,before), c in [0,count):
//   dst[b*dst_pitch_b + c*after_b + 0..after_b) =
//   src[b*src_pitch_b + c*after_b + 0..after_b)
// All quantities in BYTES except `before`/`count` (row counts). Note the
// c-stride is after_b on BOTH sides by definition, so (count, after)
// collapse into one contiguous row of count*after_b bytes per b — the
// kernel exploits this and vectorizes rows with phase-aligned 16/8/4-byte
// granules plus bytewise head/tail.
struct SlabDesc {
  const void* src;
  void* dst;
  int64_t before;
  int64_t count;
  int64_t after_b;
  int64_t src_pitch_b;  // byte stride between consecutive `b` on src
  int64_t dst_pitch_b;  // byte stride between consecutive `b` on dst
};

// Max slabs handled by a single kernel launch (descriptor array is passed
// by value in kernel args). Larger batches loop over launches.
constexpr int kMaxSlabsPerLaunch = 8;

// Batched strided copy of `n` slabs on `stream`. Consecutive slabs that admit
// the same granule (16, 8 or 4 bytes by the src/dst phase and pitch
// difference, else the 16-byte byte-window kernel) share launches of <=8.
void launch_slab_copy(const SlabDesc* descs, int n, hipStream_t stream);

// Elementwise bitwise reduction across `nranks` contiguous chunks:
//   out[0..chunk_bytes) = op_{r<nranks} in[r*chunk_bytes ..]
// op: 0=AND 1=OR 2=XOR. Bitwise ops are byte-local, so this is
// dtype-independent (serves MPI_BAND/BOR/BXOR for every integer dtype;
// reference op table csrc/extension.cpp:204-252).
void launch_bitwise_reduce(const void* in, void* out, int64_t chunk_bytes,
                           int nranks, int op, hipStream_t stream);

// MINLOC/MAXLOC local arg-reduction across `nranks` contiguous chunks of
// (value, location) pairs (MPI pair-type semantics, reference op table
// csrc/extension.cpp:204-252): in is [nranks][n_pairs][2] (last axis =
// value, location in the same dtype), out is [n_pairs][2].
//   op 0 = MINLOC: smallest value, ties -> smallest location
//   op 1 = MAXLOC: largest value, ties -> smallest location
// A NaN value wins for both ops (torch.min/torch.max propagate it); its
// location is the smallest among the NaN entries. -0.0 and +0.0 tie.
// Locations compare exactly in their own dtype and must not be NaN.
// dtype codes: 0=f32 1=f64 2=f16 3=bf16 4=i8 5=u8 6=i16 7=i32 8=i64
void launch_pairloc_reduce(const void* in, void* out, int64_t n_pairs,
                           int nranks, int op, int dtype, hipStream_t stream);

// Fused fp8 local reduction with fp32 accumulation: elementwise
//   out[i] = op_{r<nranks} fp32(in[r*n + i])  quantized to fp8 ONCE.
// This is the MI355X fp8 allreduce tail (allgather + this kernel): one
// quantization instead of one per ring hop, fp32 accumulation throughout.
// The result is the torch cast of the fp32 rank-order accumulation: round to
// nearest even WITHOUT saturation, so a finite overflow gives NaN (e4m3fn,
// |acc| > 464) or +-inf (e5m2, |acc| >= 61440) and a loss scaler still sees
// it. MIN/MAX propagate NaN (at::minimum/at::maximum, unlike arith_reduce).
// op: 0=sum 1=prod 2=min 3=max; e5m2 selects the encoding.
void launch_fp8_reduce(const void* in, void* out, int64_t n_elems,
                       int nranks, int op, bool e5m2, hipStream_t stream);

// Arithmetic local reduction for bf16/fp16/fp32 that reads its sources where
// they lie (the tail of native_allreduce): source r is `own` for r == me,
// otherwise slot r (r < me) or r-1 (r > me) of `staged`, whose nranks-1
// slots are stride_elems apart. Sources combine in rank order; 16-bit dtypes
// accumulate in fp32 and round once (RNE); MIN/MAX follow fminf/fmaxf.
// op: 0=sum 1=prod 2=min 3=max. dtype codes: 0=f32 1=bf16 2=f16.
// nranks == 1 is launch_arith_copy of the own block (staged is not read).
// Any n_elems and any alignment: 16-byte vectors when every pointer and the
// slot stride allow it (tail elements by one extra work item), one element
// per thread otherwise.
void launch_arith_reduce(const void* own, const void* staged,
                         int64_t stride_elems, int nranks, int me, void* out,
                         int64_t n_elems, int op, int dtype,
                         hipStream_t stream);
// The nranks == 1 instance: raw bit copy of nbytes (no float conversion, so
// it serves every dtype), one 16-byte nontemporal move per thread.
void launch_arith_copy(const void* src, void* dst, int64_t nbytes,
                       hipStream_t stream);

// mxfp8 codec (csrc/mx8_kernels.hip): groups of 32 consecutive elements ->
// 32 OCP e4m3fn payload bytes + one E8M0 scale byte (255 = non-finite
// group). The rule is defined by the torch composite in csrc/ops.cpp; the
// kernels match it byte for byte. dtype codes: 0=f32 1=bf16 2=f16.
//
// Quantize n_elems elements: payload gets ceil(n/32)*32 bytes (the partial
// last group is zero-padded), scales ceil(n/32) bytes.
void launch_mx8_quantize(const void* in, void* payload, void* scales,
                         int64_t n_elems, int dtype, hipStream_t stream);
// Reduce nranks copies of n_groups groups: payload_in [nranks][n_groups*32],
// scales_in [nranks][n_groups]. Sum in rank order on dequantized fp32
// values, one requantization.
void launch_mx8_reduce(const void* payload_in, const void* scales_in,
                       void* payload_out, void* scales_out, int64_t n_groups,
                       int nranks, hipStream_t stream);
// Dequantize into exactly n_elems elements of the given dtype (RNE).
void launch_mx8_dequantize(const void* payload, const void* scales, void* out,
                           int64_t n_elems, int dtype, hipStream_t stream);
// Reduce nranks mxfp8 copies of ceil(n_elems/32) groups straight into
// n_elems elements of `dtype` (0=f32 1=bf16 2=f16): fp32 rank-order sum of
// dequantized values, one RNE cast, no requantization. Writes exactly
// n_elems elements. Input layout as launch_mx8_reduce with
// n_groups = ceil(n_elems/32). nranks == 1 is launch_mx8_dequantize.
void launch_mx8_reduce_to(const void* payload_in, const void* scales_in,
                          void* out, int64_t n_elems, int nranks, int dtype,
                          hipStream_t stream);
// The allgather tail: nblocks mxfp8 streams, each of L = rows*row_elems
// elements with groups that start at the block, dequantized straight into
// place.
// payload [nblocks][Gb*32], scales [nblocks][Gb], Gb = ceil(rows*row_elems/32)
// out [rows][nblocks][row_elems] contiguous, of `dtype` (0=f32 1=bf16 2=f16):
//   out[b][r][j] = cast(dq(block r))[b*row_elems + j]
// Writes exactly rows*nblocks*row_elems elements. nblocks <= 65535 (grid.y).
void launch_mx8_dequantize_blocks(const void* payload, const void* scales,
                                  void* out, int nblocks, int64_t rows,
                                  int64_t row_elems, int dtype,
                                  hipStream_t stream);
// The all-to-all head, the mirror of the above on the send side: the
// contiguous in [rows][nblocks][row_elems] of `dtype` is read in place and
// block r, the stream of L = rows*row_elems elements in[b][r][j] in (b, j)
// order, is quantized in groups of 32 that start at the block:
//   payload [nblocks][Gb*32], scales [nblocks][Gb], Gb = ceil(L/32)
// byte for byte what launch_mx8_quantize gives on a contiguous copy of each
// block (zero-padded partial last group included). Writes exactly
// nblocks*Gb*33 bytes. nblocks <= 65535 (grid.y).
void launch_mx8_quantize_blocks(const void* in, void* payload, void* scales,
                                int nblocks, int64_t rows, int64_t row_elems,
                                int dtype, hipStream_t stream);

// One segment of the variable-count codec kernels below: `count` slices of
// the stream side starting at slice `displ`, whose mxfp8 stream starts at
// group `goff` (payload byte 32*goff, scale byte goff).
struct Mx8SegDesc {
  int64_t displ;
  int64_t count;
  int64_t goff;
};

// Max segments handled by a single launch of the segments kernels (the
// descriptors are passed by value in the kernel arguments, 24 bytes each).
// Larger batches loop over launches.
constexpr int kMaxMx8SegsPerLaunch = 32;

// The pairwise all-to-all head: the variable-count, optionally indexed
// sibling of launch_mx8_quantize_blocks. `in` is [rows][S][after] contiguous
// of `dtype`. Segment p is the stream of L_p = rows*count_p*after elements
// in[b][slice(displ_p + c)][a] in (b, c, a) order, where slice(s) = idx[s]
// with an index and s without one; it is quantized in groups of 32 that start
// at the segment, G_p = ceil(L_p/32) groups to payload + 32*goff_p and
// scales + goff_p, byte for byte what launch_mx8_quantize gives on a
// contiguous copy of the segment (zero-padded partial last group included).
// The caller guarantees displ_p + count_p <= S without an index and <= the
// length of idx with one; an idx entry outside [0, S) reads as a slice of
// zeros. A segment with count 0 writes nothing.
void launch_mx8_quantize_segments(const void* in, const int64_t* idx,
                                  void* payload, void* scales,
                                  const Mx8SegDesc* segs, int nsegs,
                                  int64_t rows, int64_t S, int64_t after,
                                  int dtype, hipStream_t stream);
// The pairwise all-to-all tail, the mirror of the above: segment p's stream
// is dequantized into out[b][slice(displ_p + c)][a] of the contiguous
// [rows][S][after] output of `dtype`. Writes exactly L_p elements per
// segment; an idx entry outside [0, S) drops its slice.
void launch_mx8_dequantize_segments(const void* payload, const void* scales,
                                    const int64_t* idx, void* out,
                                    const Mx8SegDesc* segs, int nsegs,
                                    int64_t rows, int64_t S, int64_t after,
                                    int dtype, hipStream_t stream);

} // namespace m4a
