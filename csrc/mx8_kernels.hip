// mxfp8 codec kernels for gfx950: the compressed-allreduce wire format.
//
// Format: groups of 32 consecutive elements; each group is 32 OCP e4m3fn
// payload bytes plus one E8M0 scale byte (33/32 byte per element). The
// codec rule is normative and defined by the torch composite in
// csrc/ops.cpp (mx8_quantize_groups / mx8_dequantize_groups); these kernels
// reproduce it bit for bit:
//   * amax over |x| is taken on the IEEE bit patterns (monotone for finite
//     values; anything >= 0x7f800000 is inf/NaN -> scale 255, zero payload);
//   * the shared exponent E comes from the exponent/mantissa fields
//     (frexp arithmetic, no log2f): amax = m*2^k, m in [0.5,1):
//     E = k-9 if m <= 0.875 else k-8, clamped to [-127,127];
//   * scaling is ldexpf (exact power-of-two scale), the conversion is the
//     hardware RNE f32->e4m3 of hip_fp8.h, which cannot saturate because
//     amax*2^-E <= 448 by construction.
//
// Nine streaming kernels, all 256-thread workgroups, grid-stride, 16-byte
// accesses on the wide side, nontemporal (every byte is touched once):
//   quantize   : 8 lanes x 16 B per fp32 group, 4 lanes x 16 B per 16-bit
//                group; amax crosses the lanes with 3 / 2 xor-shuffles;
//                payload leaves as packed dwords; scale bytes are gathered
//                across the wave so one lane stores four at once.
//   reduce     : sibling of fp8_reduce_kernel — dwordx4 payload loads
//                (16 elements per lane, 2 lanes per group), 16 fp32
//                accumulators, P copies summed in rank order on dequantized
//                values, requantization fused (amax crosses the lane pair).
//   dequantize : mirror of quantize; writes exactly N elements.
//   reduce_to  : the reduce-scatter tail — the reduce kernel without its
//                requantization: P copies summed in rank order straight
//                into N elements of the output dtype, 32 output bytes per
//                lane (two 16-byte stores).
//   dequantize_blocks : the allgather tail — the dequantize kernel's lane
//                layout over P gathered blocks at once (grid.y = block),
//                every 16-byte chunk stored straight at its place in the
//                [rows][P][row_elems] output.
//   quantize_blocks : the all-to-all head, its mirror — the quantize
//                kernel's lane layout over the P blocks of a
//                [rows][P][row_elems] input read in place (grid.y = block),
//                one mxfp8 stream per block out.
//   quantize_segments / dequantize_segments : the pairwise all-to-all head
//                and tail — the two _blocks layouts over segments of
//                variable slice counts (grid.y = segment, descriptors by
//                value), optionally gathering / scattering slices through
//                an int64 index while they read / write.
//   dequantize_combine : the top-k tail — received slices that name the same
//                output slice are summed there in table order in fp32 and
//                cast once; flat grid over the output chunks, the sources'
//                loads issued four at a time (see there).
// and the three kernels of the gated top-k combine:
//   dequantize_combine_weighted : dequantize_combine with an fp32 weight per
//                table entry, product rounded before the add;
//   quantize_segments_weighted : quantize_segments (rows == 1) of slices
//                scaled by an fp32 weight each, the head of its backward;
//   dequantize_rowdot : the weights' gradient, one dot product per received
//                slice over a group of 8 to 64 lanes; the one reduction here.
// Each of them has a twin for any slice length and alignment.
// quantize and reduce also exist with stochastic rounding (launch_mx8_*_sr):
// the same kernels under another rounding policy, see "rounding policies".
// The first four have a one-thread-per-group scalar twin for base pointers
// that miss the vector alignment (e.g. a contiguous x[1:] view); the partial
// last group of their vector kernels goes through the same scalar group
// routine. dequantize_blocks has a general twin that still stores aligned
// 16-byte chunks (see there); quantize_blocks has a one-thread-per-group twin
// with element-wise index mapping; the segments kernels have
// one-thread-per-group twins on both sides.
//
// What the kernels share is written once:
//   quant_lane / dequant_lane : one lane's part of a group in the vector
//                kernels of either direction (flat, _blocks, _segments);
//   quantize_stream / dequantize_stream : the vector body of the _blocks and
//                _segments kernels, templated on the map from a stream chunk
//                to its place in the tensor (BlockMap, SegMap); the kernels
//                themselves only pick the stream that grid.y names;
//   sum_copies : the rank-order sum of reduce and reduce_to;
//   SegCursor  : the (b, c, a) walk of the two segments twins.
// The mxfp4 wire of AllgatherCompressed (e2m1 nibbles under the same groups
// and scale byte) has its quantize and dequantize_blocks kernels at the end
// of this file, with its rule; the mxfp6 wire (e2m3 codes, 24 payload bytes
// per group) follows it.
// On the host, by_dtype / by_width / by_width_mode turn the run-time dtype,
// index width and segment mode into template arguments, grid2d is the capped
// 2-D grid, and launch_segments_t is both segments launchers.

#include <hip/hip_runtime.h>
#include <hip/hip_fp8.h>
#include <type_traits>
#include "kernels.hpp"

namespace m4a {

namespace {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef unsigned char u8;

constexpr unsigned kInfBits = 0x7f800000u;
constexpr unsigned kQNaNBits = 0x7fc00000u;

enum { kF32 = 0, kBF16 = 1, kF16 = 2 };

template <int K> struct Elem { using type = float; };
template <> struct Elem<kBF16> { using type = unsigned short; };
template <> struct Elem<kF16> { using type = unsigned short; };

__device__ inline float e4m3_to_f32(u8 b) {
  __hip_fp8_e4m3 v;
  v.__x = b;
  return float(v);
}

__device__ inline u8 f32_to_e4m3(float f) {
  __hip_fp8_e4m3 v(f);
  return v.__x;
}

// ---- element <-> f32 ----------------------------------------------------

template <int K>
__device__ inline float elem_to_f32(typename Elem<K>::type e);
template <>
__device__ inline float elem_to_f32<kF32>(float e) { return e; }
template <>
__device__ inline float elem_to_f32<kBF16>(unsigned short e) {
  return __uint_as_float((unsigned)e << 16);
}
template <>
__device__ inline float elem_to_f32<kF16>(unsigned short e) {
  return (float)__builtin_bit_cast(_Float16, e);
}

// RNE to the output dtype (bf16: the usual bias trick, NaN -> 0x7fc0)
template <int K>
__device__ inline typename Elem<K>::type f32_to_elem(float f);
template <>
__device__ inline float f32_to_elem<kF32>(float f) { return f; }
template <>
__device__ inline unsigned short f32_to_elem<kBF16>(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > kInfBits) return 0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
template <>
__device__ inline unsigned short f32_to_elem<kF16>(float f) {
  return __builtin_bit_cast(unsigned short, (_Float16)f);
}

// 16 bytes of input -> 4 (fp32) or 8 (16-bit) floats
template <int K, int EPL>
__device__ inline void unpack16(const v4u& w, float (&x)[EPL]) {
  if constexpr (K == kF32) {
    for (int d = 0; d < 4; ++d) x[d] = __uint_as_float(w[d]);
  } else {
    for (int d = 0; d < 4; ++d) {
      x[2 * d] = elem_to_f32<K>((unsigned short)(w[d] & 0xffffu));
      x[2 * d + 1] = elem_to_f32<K>((unsigned short)(w[d] >> 16));
    }
  }
}

template <int K, int EPL>
__device__ inline v4u pack16(const float (&x)[EPL]) {
  v4u w;
  if constexpr (K == kF32) {
    for (int d = 0; d < 4; ++d) w[d] = __float_as_uint(x[d]);
  } else {
    for (int d = 0; d < 4; ++d) {
      w[d] = (unsigned)f32_to_elem<K>(x[2 * d]) |
             ((unsigned)f32_to_elem<K>(x[2 * d + 1]) << 16);
    }
  }
  return w;
}

// ---- the codec rule -----------------------------------------------------

// amax_bits: max over the group of (bits & 0x7fffffff). Returns the scale
// byte; *E receives the shared exponent (unused when the byte is 255).
__device__ inline int mx8_scale_byte(unsigned amax_bits, int* E) {
  if (amax_bits >= kInfBits) {
    *E = 0;
    return 255;
  }
  const int e = (int)(amax_bits >> 23);
  const unsigned f = amax_bits & 0x7fffffu;
  int ex;
  if (amax_bits == 0) {
    ex = 0;
  } else if (e == 0) {
    ex = -127;  // fp32 subnormal amax: k <= -126, k-8 clamps
  } else {
    // amax = 1.f * 2^(e-127) = m * 2^(e-126), m = 1.f/2; m <= 0.875 <=>
    // f <= 0x600000
    ex = (e - 126) - (f <= 0x600000u ? 9 : 8);
    if (ex < -127) ex = -127;
  }
  *E = ex;
  return ex + 127;
}

__device__ inline float mx8_dequant(u8 b, int sb) {
  return sb == 255 ? __uint_as_float(kQNaNBits)
                   : ldexpf(e4m3_to_f32(b), sb - 127);
}

template <int N>
__device__ inline unsigned amax_bits_of(const float (&x)[N]) {
  unsigned a = 0;
  for (int k = 0; k < N; ++k) {
    const unsigned b = __float_as_uint(x[k]) & 0x7fffffffu;
    a = b > a ? b : a;
  }
  return a;
}

// ---- rounding policies ----------------------------------------------------
//
// The step y -> e4m3 byte of the codec, y = x * 2^-E with |y| <= 448. A policy
// is called as rnd(y, k), k the element's index within the lane (or within
// the group in the scalar routines). Rne is the codec's own rule and the
// default everywhere, in the way NoPre is the default Pre.
struct Rne {
  __device__ u8 operator()(float y, int) const { return f32_to_e4m3(y); }
};

// Stochastic rounding (the rule is normative in csrc/ops.cpp,
// mx8_quantize_groups_sr). The grid around y has ulp = 2^(e-3),
// e = max(floor(log2|y|), -6); with t = |y|/ulp = fl + frac the rule rounds
// up iff frac >= (65536 - r) * 2^-16 for the element's 16 random bits r. The
// threshold is a multiple of 2^-16, so only floor(frac * 2^16) takes part and
// the comparison is the carry out of the low half of t16 + r,
// t16 = floor(t * 2^16) < 2^20:  fl + up = (t16 + r) >> 16  in [0, 16].
// The e4m3 byte of (fl + up) * ulp is then plain integer arithmetic: with the
// biased exponent em = e + 127 >= 121 it is ((em - 121) << 3) + (fl + up):
// subnormal or the first normal binade for em == 121 (fl + up <= 8 counts
// ulps of 2^-9), and for em > 121, where fl >= 8, the exponent field
// em - 120 over mantissa fl + up - 8, the carry of fl + up == 16 going into
// the exponent. |y| <= 448 has fl + up <= 14 in the top binade, so 0x7e is
// the largest byte: the rule cannot saturate. Ten VALU operations per
// element and no use of the hardware conversion.
//
// The random bits are counter-based: element n of the logical stream takes
// half of the hash word of its aligned pair j = n >> 1,
//   w = h((h(lo32(j) ^ k0) + hi32(j)) ^ k1),  r = n & 1 ? w >> 16 : w & 0xffff,
// so a byte depends on (key, n) alone, never on the grid, the lane layout or
// the vector/twin path. A lane owns 2*W consecutive elements from a multiple
// of 2*W on (the stream's first index n0 is a multiple of 32), so its W words
// are j0 + slot*W + 0..W-1 without a carry out of the low word.
__device__ inline unsigned sr_hash(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

template <int W>
struct SrLane {
  unsigned w[W];
  __device__ u8 operator()(float y, int k) const {
    const unsigned u = __float_as_uint(y);
    const unsigned r = (k & 1) ? w[k >> 1] >> 16 : w[k >> 1] & 0xffffu;
    unsigned em = (u >> 23) & 0xffu;
    em = em > 121u ? em : 121u;  // y == 0 and tiny y sit on the 2^-9 grid
    const unsigned t16 = (unsigned)ldexpf(fabsf(y), 146 - (int)em);
    return (u8)(((u >> 24) & 0x80u) | (((em - 121u) << 3) + ((t16 + r) >> 16)));
  }
};

// By value in the kernel arguments: the key words and the pair index of the
// stream's first element.
struct SrKey {
  unsigned k0, k1;
  long long j0;
};

// The policy of lane slot `slot` (of 2*W elements). Without a key it is Rne:
// the round-to-nearest kernels pass none and stay the code they were. The
// high word of the pair index is taken once per slot.
template <int W>
__device__ inline Rne lane_rounding(long long) { return Rne{}; }
template <int W>
__device__ inline SrLane<W> lane_rounding(long long slot, const SrKey& key) {
  const long long jb = key.j0 + slot * W;
  const unsigned lo = (unsigned)jb, hi = (unsigned)(jb >> 32);
  SrLane<W> l;
  for (int d = 0; d < W; ++d) {
    l.w[d] = sr_hash((sr_hash((lo + d) ^ key.k0) + hi) ^ key.k1);
  }
  return l;
}

// four values -> one packed payload dword; k: index of `a` within the lane
template <typename Rnd = Rne>
__device__ inline unsigned quant4(float a, float b, float c, float d, int E,
                                  const Rnd& rnd = Rnd{}, int k = 0) {
  return (unsigned)rnd(ldexpf(a, -E), k) |
         ((unsigned)rnd(ldexpf(b, -E), k + 1) << 8) |
         ((unsigned)rnd(ldexpf(c, -E), k + 2) << 16) |
         ((unsigned)rnd(ldexpf(d, -E), k + 3) << 24);
}

// Gather the wave's scale bytes (group j's byte lives in lane j*LPG) so
// lane l stores groups 4l..4l+3 as one dword. Every lane of the wave must
// call this (the shuffles read across groups). gbase: first group of the
// wave; ngroups: bound of the scales array.
template <int LPG>
__device__ inline void store_scales(u8* __restrict__ sc, long long gbase,
                                    long long ngroups, int sb, int lane) {
  constexpr int GPW = 64 / LPG;
  unsigned packed = 0;
  for (int k = 0; k < 4; ++k) {
    const int src = ((lane * 4 + k) * LPG) & 63;
    packed |= ((unsigned)__shfl(sb, src) & 0xffu) << (8 * k);
  }
  if (lane < GPW / 4) {
    const long long g = gbase + 4 * lane;
    u8* p = sc + g;
    if (g + 4 <= ngroups && ((uintptr_t)p & 3) == 0) {
      __builtin_nontemporal_store(packed, reinterpret_cast<unsigned*>(p));
    } else {
      for (int k = 0; k < 4; ++k) {
        if (g + k < ngroups) p[k] = (u8)(packed >> (8 * k));
      }
    }
  }
}

// ---- scalar group routines (any alignment, partial groups) --------------

template <typename Rnd = Rne>
__device__ inline void encode_group_scalar(const float (&x)[32],
                                           u8* __restrict__ pay,
                                           u8* __restrict__ sc,
                                           const Rnd& rnd = Rnd{}) {
  int E;
  const int sb = mx8_scale_byte(amax_bits_of(x), &E);
  for (int k = 0; k < 32; ++k) {
    pay[k] = sb == 255 ? (u8)0 : rnd(ldexpf(x[k], -E), k);
  }
  *sc = (u8)sb;
}

template <int K, typename Rnd = Rne>
__device__ inline void quant_group_scalar(
    const typename Elem<K>::type* __restrict__ in, int cnt,
    u8* __restrict__ pay, u8* __restrict__ sc, const Rnd& rnd = Rnd{}) {
  float x[32];
  for (int k = 0; k < 32; ++k) {
    x[k] = k < cnt ? elem_to_f32<K>(in[k]) : 0.0f;
  }
  encode_group_scalar(x, pay, sc, rnd);
}

template <int K>
__device__ inline void dequant_group_scalar(
    const u8* __restrict__ pay, int sb, int cnt,
    typename Elem<K>::type* __restrict__ out) {
  for (int k = 0; k < 32; ++k) {
    if (k < cnt) out[k] = f32_to_elem<K>(mx8_dequant(pay[k], sb));
  }
}

// ---- vector lane routines -------------------------------------------------
//
// The quantize/dequantize family's lane layout: a lane owns one 16-byte
// chunk of the tensor side, EPL elements, and the EPL payload bytes that go
// with it; LPG lanes share a group.
template <int K> constexpr int kLPG = K == kF32 ? 8 : 4;  // lanes per group
template <int K> constexpr int kEPL = 32 / kLPG<K>;       // elements per lane

// Lane slot j's BPL payload bytes as dwords, one nontemporal load.
template <int BPL>
__device__ inline void load_payload(const u8* __restrict__ pin, long long j,
                                    unsigned (&w)[BPL / 4]) {
  if constexpr (BPL == 4) {
    w[0] =
        __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(pin) + j);
  } else if constexpr (BPL == 8) {
    const v2u t =
        __builtin_nontemporal_load(reinterpret_cast<const v2u*>(pin) + j);
    w[0] = t[0];
    w[1] = t[1];
  } else {
    const v4u t =
        __builtin_nontemporal_load(reinterpret_cast<const v4u*>(pin) + j);
    for (int d = 0; d < 4; ++d) w[d] = t[d];
  }
}

// 16-byte chunk `src` of the tensor as this lane's elements; zeros when the
// lane has nothing to read.
template <int K>
__device__ inline void load_chunk(const void* __restrict__ in, long long src,
                                  bool ok, float (&x)[kEPL<K>]) {
  if (ok) {
    const v4u w =
        __builtin_nontemporal_load(reinterpret_cast<const v4u*>(in) + src);
    unpack16<K, kEPL<K>>(w, x);
  } else {
    for (int k = 0; k < kEPL<K>; ++k) x[k] = 0.0f;
  }
}

// One lane of a group's quantization. The amax crosses the group's LPG lanes
// by xor-shuffles, so every lane of the wave must call this; a lane that
// stores writes its EPL payload bytes at lane slot i of `pay`. Returns the
// group's scale byte.
template <int K, typename Rnd = Rne>
__device__ inline int quant_lane(const float (&x)[kEPL<K>], bool store,
                                 u8* __restrict__ pay, long long i,
                                 const Rnd& rnd = Rnd{}) {
  constexpr int EPL = kEPL<K>;
  unsigned a = amax_bits_of(x);
  for (int m = 1; m < kLPG<K>; m <<= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)a, m);
    a = o > a ? o : a;
  }
  int E;
  const int sb = mx8_scale_byte(a, &E);
  if (store) {
    const unsigned lo =
        sb == 255 ? 0u : quant4(x[0], x[1], x[2], x[3], E, rnd, 0);
    if constexpr (K == kF32) {
      __builtin_nontemporal_store(lo, reinterpret_cast<unsigned*>(pay) + i);
    } else {
      v2u o;
      o[0] = lo;
      o[1] = sb == 255
                 ? 0u
                 : quant4(x[EPL - 4], x[EPL - 3], x[EPL - 2], x[EPL - 1], E,
                          rnd, EPL - 4);
      __builtin_nontemporal_store(o, reinterpret_cast<v2u*>(pay) + i);
    }
  }
  return sb;
}

// One lane of a group's dequantization: the EPL payload bytes at lane slot i
// of `pay` under scale byte sb, as the 16-byte chunk of the output dtype.
template <int K>
__device__ inline v4u dequant_lane(const u8* __restrict__ pay, long long i,
                                   int sb) {
  constexpr int EPL = kEPL<K>;
  unsigned w[EPL / 4];
  load_payload<EPL>(pay, i, w);
  float x[EPL];
  for (int d = 0; d < EPL / 4; ++d) {
    for (int k = 0; k < 4; ++k) {
      x[4 * d + k] = mx8_dequant((u8)(w[d] >> (8 * k)), sb);
    }
  }
  return pack16<K, EPL>(x);
}

// Lane slot j of group g summed over the P copies (copy r's lane slots start
// at r*cstride, its scales at r*G): copy 0 assigned, copies 1..P-1 added in
// rank order on dequantized values. Returns whether any copy's group is 255.
template <int BPL>
__device__ inline bool sum_copies(const u8* __restrict__ pin,
                                  const u8* __restrict__ sin, long long j,
                                  long long cstride, long long g, long long G,
                                  long long nranks, float (&acc)[BPL]) {
  bool bad = false;
  auto copy = [&](long long r, auto first) {
    unsigned w[BPL / 4];
    load_payload<BPL>(pin, r * cstride + j, w);
    const int sb = sin[r * G + g];
    bad = bad || sb == 255;
    for (int d = 0; d < BPL / 4; ++d) {
      for (int k = 0; k < 4; ++k) {
        const float v = ldexpf(e4m3_to_f32((u8)(w[d] >> (8 * k))), sb - 127);
        if constexpr (decltype(first)::value) {
          acc[4 * d + k] = v;
        } else {
          acc[4 * d + k] += v;
        }
      }
    }
  };
  copy(0, std::true_type{});
  for (long long r = 1; r < nranks; ++r) copy(r, std::false_type{});
  return bad;
}

// ---- quantize -----------------------------------------------------------

// Key is empty (round to nearest) or one SrKey (stochastic rounding, see
// lane_rounding); the same holds for the twin and the two reduce kernels.
template <int K, typename... Key>
__global__ __launch_bounds__(256) void mx8_quantize_kernel(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long nfull, long long N, Key... key) {
  using T = typename Elem<K>::type;
  constexpr int LPG = kLPG<K>;
  const long long total = nfull * LPG;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  // wave-uniform trip count: the shuffles in quant_lane and store_scales
  // need every lane present
  for (long long i0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
       i0 < total; i0 += stride) {
    const long long i = i0 + lane;
    const bool act = i < total;
    float x[kEPL<K>];
    load_chunk<K>(in, i, act, x);
    const int sb =
        quant_lane<K>(x, act, pay, i, lane_rounding<kEPL<K> / 2>(i, key...));
    store_scales<LPG>(sc, i0 / LPG, nfull, sb, lane);
  }
  // zero-padded partial last group
  const int tail = (int)(N - nfull * 32);
  if (tail > 0 && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    quant_group_scalar<K>(reinterpret_cast<const T*>(in) + nfull * 32, tail,
                          pay + nfull * 32, sc + nfull,
                          lane_rounding<16>(nfull, key...));
  }
}

template <int K, typename... Key>
__global__ __launch_bounds__(256) void mx8_quantize_kernel_scalar(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long G, long long N, Key... key) {
  using T = typename Elem<K>::type;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    const long long left = N - g * 32;
    quant_group_scalar<K>(reinterpret_cast<const T*>(in) + g * 32,
                          left < 32 ? (int)left : 32, pay + g * 32, sc + g,
                          lane_rounding<16>(g, key...));
  }
}

// ---- reduce -------------------------------------------------------------

template <typename... Key>
__global__ __launch_bounds__(256) void mx8_reduce_kernel(
    const u8* __restrict__ pin, const u8* __restrict__ sin,
    u8* __restrict__ pout, u8* __restrict__ sout, long long n,
    long long nranks, Key... key) {
  const long long total = n * 2;  // 16-byte vectors per copy
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  for (long long i0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
       i0 < total; i0 += stride) {
    const long long i = i0 + lane;
    const bool act = i < total;
    float acc[16];
    bool bad = false;
    if (act) {
      bad = sum_copies<16>(pin, sin, i, total, i >> 1, n, nranks, acc);
    } else {
      for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
    }
    unsigned a = bad ? kInfBits : amax_bits_of(acc);
    const unsigned o = (unsigned)__shfl_xor((int)a, 1);
    a = o > a ? o : a;
    int E;
    const int sb = mx8_scale_byte(a, &E);
    if (act) {
      const auto rnd = lane_rounding<8>(i, key...);
      v4u w;
      for (int d = 0; d < 4; ++d) {
        w[d] = sb == 255 ? 0u
                         : quant4(acc[4 * d], acc[4 * d + 1], acc[4 * d + 2],
                                  acc[4 * d + 3], E, rnd, 4 * d);
      }
      __builtin_nontemporal_store(w, reinterpret_cast<v4u*>(pout) + i);
    }
    store_scales<2>(sout, i0 >> 1, n, sb, lane);
  }
}

template <typename... Key>
__global__ __launch_bounds__(256) void mx8_reduce_kernel_scalar(
    const u8* __restrict__ pin, const u8* __restrict__ sin,
    u8* __restrict__ pout, u8* __restrict__ sout, long long n,
    long long nranks, Key... key) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n;
       g += stride) {
    float acc[32];
    bool bad;
    {
      const int sb = sin[g];
      bad = sb == 255;
      for (int k = 0; k < 32; ++k) {
        acc[k] = ldexpf(e4m3_to_f32(pin[g * 32 + k]), sb - 127);
      }
    }
    for (long long r = 1; r < nranks; ++r) {
      const int sb = sin[r * n + g];
      bad = bad || sb == 255;
      const u8* p = pin + (r * n + g) * 32;
      for (int k = 0; k < 32; ++k) {
        acc[k] += ldexpf(e4m3_to_f32(p[k]), sb - 127);
      }
    }
    if (bad) acc[0] = __uint_as_float(kQNaNBits);
    encode_group_scalar(acc, pout + g * 32, sout + g,
                        lane_rounding<16>(g, key...));
  }
}

// ---- dequantize ---------------------------------------------------------

template <int K>
__global__ __launch_bounds__(256) void mx8_dequantize_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long nfull, long long N) {
  using T = typename Elem<K>::type;
  constexpr int LPG = kLPG<K>;
  const long long total = nfull * LPG;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += stride) {
    __builtin_nontemporal_store(dequant_lane<K>(pay, i, sc[i / LPG]),
                                reinterpret_cast<v4u*>(out) + i);
  }
  // partial last group: exactly N - 32*nfull elements, nothing past N
  const int tail = (int)(N - nfull * 32);
  if (tail > 0 && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    dequant_group_scalar<K>(pay + nfull * 32, sc[nfull], tail,
                            reinterpret_cast<T*>(out) + nfull * 32);
  }
}

template <int K>
__global__ __launch_bounds__(256) void mx8_dequantize_kernel_scalar(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long G, long long N) {
  using T = typename Elem<K>::type;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    const long long left = N - g * 32;
    dequant_group_scalar<K>(pay + g * 32, sc[g], left < 32 ? (int)left : 32,
                            reinterpret_cast<T*>(out) + g * 32);
  }
}

// ---- reduce_to (the reduce-scatter tail) ---------------------------------
//
// P copies of G = ceil(N/32) groups -> N elements of the output dtype: fp32
// rank-order sum of dequantized values, one RNE cast, no requantization.
// Input layout as mx8_reduce_kernel: pin [nranks][G*32], sin [nranks][G].

// One group, any alignment, cnt <= 32 elements written.
template <int K>
__device__ inline void reduce_to_group_scalar(
    const u8* __restrict__ pin, const u8* __restrict__ sin, long long G,
    long long g, long long nranks, int cnt,
    typename Elem<K>::type* __restrict__ out) {
  bool bad = false;
  for (long long r = 0; r < nranks; ++r) bad = bad || sin[r * G + g] == 255;
  for (int k = 0; k < cnt; ++k) {
    float a = ldexpf(e4m3_to_f32(pin[g * 32 + k]), (int)sin[g] - 127);
    for (long long r = 1; r < nranks; ++r) {
      a += ldexpf(e4m3_to_f32(pin[(r * G + g) * 32 + k]),
                  (int)sin[r * G + g] - 127);
    }
    out[k] = f32_to_elem<K>(bad ? __uint_as_float(kQNaNBits) : a);
  }
}

// Vector body: every lane produces 32 output bytes, two consecutive 16-byte
// stores, so BPL payload bytes (= elements) per lane per copy are 8 for
// fp32 (dwordx2 loads, 4 lanes per group) and 16 for the 16-bit dtypes (the
// reduce kernel's dwordx4 loads, 2 lanes per group). Measured against the
// other widths in doc/kernels.md section 5: four stores per lane (fp32 at
// the reduce kernel's width) leave each 128-byte line to four store
// instructions and run at half the rate; one store per lane (the
// dequantize kernel's width) keeps too few load bytes in flight.
template <int K>
__global__ __launch_bounds__(256) void mx8_reduce_to_kernel(
    const u8* __restrict__ pin, const u8* __restrict__ sin,
    void* __restrict__ out, long long nfull, long long G, long long N,
    long long nranks) {
  using T = typename Elem<K>::type;
  constexpr int EPS = K == kF32 ? 4 : 8;          // elements per 16-B store
  constexpr int NS = 2;                           // 16-byte stores per lane
  constexpr int BPL = NS * EPS;                   // payload bytes per lane
  constexpr int LPG = 32 / BPL;                   // lanes per group
  const long long total = nfull * LPG;            // lane slots in the body
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += stride) {
    float acc[BPL];
    const bool bad =
        sum_copies<BPL>(pin, sin, i, G * LPG, i / LPG, G, nranks, acc);
    v4u* o = reinterpret_cast<v4u*>(out) + i * NS;
    for (int s = 0; s < NS; ++s) {
      float x[EPS];
      for (int k = 0; k < EPS; ++k) {
        x[k] = bad ? __uint_as_float(kQNaNBits) : acc[s * EPS + k];
      }
      __builtin_nontemporal_store(pack16<K, EPS>(x), o + s);
    }
  }
  // partial last group: exactly N - 32*nfull elements, nothing past N
  const int tail = (int)(N - nfull * 32);
  if (tail > 0 && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    reduce_to_group_scalar<K>(pin, sin, G, nfull, nranks, tail,
                              reinterpret_cast<T*>(out) + nfull * 32);
  }
}

template <int K>
__global__ __launch_bounds__(256) void mx8_reduce_to_kernel_scalar(
    const u8* __restrict__ pin, const u8* __restrict__ sin,
    void* __restrict__ out, long long G, long long N, long long nranks) {
  using T = typename Elem<K>::type;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    const long long left = N - g * 32;
    reduce_to_group_scalar<K>(pin, sin, G, g, nranks,
                              left < 32 ? (int)left : 32,
                              reinterpret_cast<T*>(out) + g * 32);
  }
}

// ---- mapped streams (the bodies of the _blocks and _segments kernels) -----
//
// One mxfp8 stream (payload base bp, scales base bs; grid.y picked it, so
// both are wave-uniform) whose 16-byte chunks lie scattered in the tensor:
// map(i) is the tensor's chunk index of stream chunk i, or, where
// Map::kCanMiss, -1 for a chunk that has no place there. I is the index
// type of the per-lane arithmetic, 32 bits whenever the stream has fewer
// than 2^31 lane slots. The grid-stride loop's two arguments, the thread's
// first index and the stride, are formed in the kernel: the compiler reads
// the launch dimensions as scalar kernel arguments only in the __global__
// function itself (read here they cost a vector load and 2 to 8 VGPRs).
#define MX8_GRID_STRIDE(I) \
  (I) blockIdx.x * blockDim.x + threadIdx.x, (I)gridDim.x * blockDim.x

// Chunk i of block r of a contiguous [rows][nblocks][cpr chunks] tensor: one
// division by the row length.
template <typename I>
struct BlockMap {
  static constexpr bool kCanMiss = false;
  long long r, nblocks;
  I cpr;
  __device__ long long operator()(I i) const {
    const I row = i / cpr;
    const I col = i - row * cpr;
    return ((long long)row * nblocks + r) * (long long)cpr + (long long)col;
  }
};

// The quantize kernel's lane layout over ALL `slots` = G*LPG lane slots of
// the stream (wave-uniform trip count: the shuffles and the scale gather
// need every lane). Slots from `chunks` on and missed chunks load nothing,
// count as zeros in the amax and store zero payload, so the partial last
// group needs no scalar tail. bs has any alignment: store_scales falls back
// to per-lane bytes. pre(i, x) may rework the elements of stream chunk
// i < chunks before they are quantized (the weighted head scales them).
// pre.elem(c, v) is the same hook for the general twins, which walk single
// elements: the value of an element of stream slice c.
struct NoPre {
  template <typename I, int N>
  __device__ void operator()(I, float (&)[N]) const {}
  __device__ float elem(long long, float v) const { return v; }
};

template <int K, typename I, typename Map, typename Pre = NoPre>
__device__ inline void quantize_stream(const void* __restrict__ in,
                                       u8* __restrict__ bp,
                                       u8* __restrict__ bs, long long G,
                                       I chunks, I slots, const Map& map,
                                       I first, I stride,
                                       const Pre& pre = Pre{}) {
  constexpr int LPG = kLPG<K>;
  const int lane = threadIdx.x & 63;
  // i0: the wave's first slot (workgroups are whole waves)
  for (I i0 = first & ~(I)63; i0 < slots; i0 += stride) {
    const I i = i0 + lane;
    long long src = -1;
    if (i < chunks) src = map(i);
    float x[kEPL<K>];
    load_chunk<K>(in, src, Map::kCanMiss ? src >= 0 : i < chunks, x);
    if (i < chunks) pre(i, x);
    const int sb = quant_lane<K>(x, i < slots, bp, (long long)i);
    store_scales<LPG>(bs, (long long)(i0 / LPG), G, sb, lane);
  }
}

// The dequantize kernel's lane layout over all `chunks` whole chunks of the
// stream, so nothing past its last element is written; the padded payload
// keeps the last group's loads inside the stream. A missed chunk is skipped.
template <int K, typename I, typename Map>
__device__ inline void dequantize_stream(const u8* __restrict__ bp,
                                         const u8* __restrict__ bs,
                                         void* __restrict__ out, I chunks,
                                         const Map& map, I first, I stride) {
  for (I i = first; i < chunks; i += stride) {
    const long long dst = map(i);
    if constexpr (Map::kCanMiss) {
      if (dst < 0) continue;
    }
    __builtin_nontemporal_store(
        dequant_lane<K>(bp, (long long)i, bs[i / kLPG<K>]),
        reinterpret_cast<v4u*>(out) + dst);
  }
}

// ---- dequantize_blocks (the allgather tail) ------------------------------
//
// nblocks mxfp8 streams of L = rows*row_elems elements each (groups start at
// the block's first element): pay [nblocks][Gb*32], sc [nblocks][Gb],
// Gb = ceil(L/32). Block r lands at out[:, r, :] of the contiguous
// [rows][nblocks][row_elems] output. grid.y is the block, so the block is
// wave-uniform and the only per-lane index arithmetic is chunk -> (row,
// column): one division by the row length in 16-byte chunks, in 32 bits
// whenever a block has fewer than 2^31 chunks (template parameter I).
//
// Vector body: the dequantize kernel's lane layout (4 or 8 payload bytes in,
// one 16-byte store out) over ALL L/EPL chunks of the block. It requires
// row_elems % EPL == 0, hence L % EPL == 0: every chunk lies inside one row
// and the partial last group is made of whole chunks, so it needs no
// separate tail and nothing past element L is written. Its payload bytes
// exist because the payload is padded to Gb*32. The scale is indexed by the
// block-flat group (chunk / LPG), never by the row, so a group may straddle
// a row boundary.
template <int K, typename I>
__global__ __launch_bounds__(256) void mx8_dequantize_blocks_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long Gb, I chunks, I cpr,
    long long nblocks) {
  const long long r = blockIdx.y;
  dequantize_stream<K, I>(pay + r * Gb * 32, sc + r * Gb, out, chunks,
                          BlockMap<I>{r, nblocks, cpr}, MX8_GRID_STRIDE(I));
}

// General twin: any row length, any alignment of the payload and output
// bases (an odd row_elems, a contiguous x[1:] view). A one-thread-per-group
// twin like the siblings' would leave every store to single elements, and
// the blocks of an odd-length allgather all start off 16 bytes. Instead
// every (block, row) segment of row_elems elements is split at the 16-byte
// boundaries of its DESTINATION: up to EPL-1 head elements, whole aligned
// chunks, up to EPL-1 tail elements. Lane slots are flattened over (row,
// slot) with row_elems/EPL + 2 slots per row: one per possible chunk, one
// for the head and one for the tail, so rows of any length keep the lanes
// busy; one division per lane maps the slot to its row. A chunk's EPL
// payload bytes start at any byte (the compiler is free to load them
// unaligned) and may belong to two groups, hence two scale bytes.
template <int K, typename I>
__global__ __launch_bounds__(256) void mx8_dequantize_blocks_kernel_shifted(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long Gb, long long row_elems, I slots,
    I total, long long nblocks) {
  using T = typename Elem<K>::type;
  constexpr int EPL = K == kF32 ? 4 : 8;
  const long long r = blockIdx.y;
  const u8* __restrict__ bp = pay + r * Gb * 32;
  const u8* __restrict__ bs = sc + r * Gb;
  const I stride = (I)gridDim.x * blockDim.x;
  for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const I b = i / slots;
    const long long k = (long long)(i - b * slots);
    T* d = reinterpret_cast<T*>(out) +
           ((long long)b * nblocks + r) * row_elems;  // the segment
    const long long s0 = (long long)b * row_elems;    // its block-flat start
    long long head =
        (long long)(((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15) /
                    sizeof(T));
    if (head > row_elems) head = row_elems;
    const long long nchunks = (row_elems - head) / EPL;
    if (k < nchunks) {
      const long long e = head + k * EPL;
      const long long src = s0 + e;
      u8 pb[EPL];
      __builtin_memcpy(pb, bp + src, EPL);
      const long long g0 = src >> 5;
      const int sb0 = bs[g0];
      const int sb1 = bs[(src + EPL - 1) >> 5];
      float x[EPL];
      for (int t = 0; t < EPL; ++t) {
        x[t] = mx8_dequant(pb[t], ((src + t) >> 5) == g0 ? sb0 : sb1);
      }
      __builtin_nontemporal_store(pack16<K, EPL>(x),
                                  reinterpret_cast<v4u*>(d + e));
    } else if (k >= (long long)slots - 2) {
      // head [0, head) or tail [head + nchunks*EPL, row_elems): fewer than
      // EPL elements each, stored one by one
      const bool is_head = k == (long long)slots - 2;
      const long long lo = is_head ? 0 : head + nchunks * EPL;
      const long long hi = is_head ? head : row_elems;
      for (long long e = lo; e < hi; ++e) {
        d[e] = f32_to_elem<K>(mx8_dequant(bp[s0 + e], bs[(s0 + e) >> 5]));
      }
    }
  }
}

// ---- quantize_blocks (the all-to-all head) -------------------------------
//
// The mirror of dequantize_blocks on the send side: the contiguous
// [rows][nblocks][row_elems] input is read in place and block r, the stream
// of L = rows*row_elems elements in[b][r][j] in (b, j) order, leaves as
// pay[r][Gb*32], sc[r][Gb], Gb = ceil(L/32), byte for byte what
// mx8_quantize gives on a contiguous copy of the block. grid.y is the block.
//
// Vector body: the quantize kernel's lane layout (one 16-byte load in, 4 or
// 8 payload bytes out, amax across LPG lanes) over ALL Gb*LPG lane slots of
// the block, so the wave-uniform loop also covers the partial last group. It
// requires row_elems % EPL == 0: every chunk lies inside one row and L is a
// whole number of chunks. Slots past L/EPL load nothing, count as zeros in
// the amax and store the zero padding of the payload, which exists because
// the payload is padded to Gb*32. Groups run over the block-flat slot index,
// never over the row, so a group may straddle a row boundary.
template <int K, typename I>
__global__ __launch_bounds__(256) void mx8_quantize_blocks_kernel(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long Gb, I chunks, I cpr, I slots, long long nblocks) {
  const long long r = blockIdx.y;
  quantize_stream<K, I>(in, pay + r * Gb * 32, sc + r * Gb, Gb, chunks, slots,
                        BlockMap<I>{r, nblocks, cpr}, MX8_GRID_STRIDE(I));
}

// General twin: any row length, any alignment of the input and payload
// bases (an odd row_elems, a contiguous x[1:] view). One thread per group,
// like the first four kernels' twins; the group's first element is mapped to
// (row, column) with one division and the 32 elements are walked from there.
template <int K>
__global__ __launch_bounds__(256) void mx8_quantize_blocks_kernel_scalar(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long Gb, long long L, long long row_elems, long long nblocks) {
  using T = typename Elem<K>::type;
  const long long r = blockIdx.y;
  const T* __restrict__ src = reinterpret_cast<const T*>(in);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < Gb;
       g += stride) {
    const long long e0 = g * 32;
    long long row = e0 / row_elems;
    long long col = e0 - row * row_elems;
    const T* p = src + (row * nblocks + r) * row_elems;
    float x[32];
    for (int k = 0; k < 32; ++k) {
      if (e0 + k < L) {
        x[k] = elem_to_f32<K>(p[col]);
        if (++col == row_elems) {
          col = 0;
          p += nblocks * row_elems;
        }
      } else {
        x[k] = 0.0f;
      }
    }
    encode_group_scalar(x, pay + (r * Gb + g) * 32, sc + r * Gb + g);
  }
}

// ---- segments (the pairwise all-to-all head and tail) --------------------
//
// The variable-count, optionally indexed siblings of the two kernels above.
// The tensor side is [rows][S][after] contiguous; segment p covers stream
// slices [displ_p, displ_p + count_p), its stream of L_p = rows*count_p*after
// elements in (b, c, a) order has G_p = ceil(L_p/32) groups, payload at byte
// 32*goff_p and scales at byte goff_p. Stream slice c of segment p is tensor
// slice idx[displ_p + c] with an index, displ_p + c without one. grid.y is
// the segment, so the descriptor (by value in the kernel arguments) is
// wave-uniform; grid.x is sized for the largest segment of the launch and a
// segment with count 0 returns at once.
//
// Vector bodies require after % EPL == 0 and aligned bases: every 16-byte
// chunk lies inside one slice. MODE picks the chunk -> tensor mapping:
//   0  no index: the rows of a segment are contiguous runs of count*after,
//      one division by the run length in chunks (as in the _blocks kernels);
//   1  index, rows == 1 (the MoE token case): one division by the slice
//      length in chunks, then the index load;
//   2  index, rows > 1: two divisions.
// The index load is a plain cached 8-byte load: all chunks of a slice share
// it. An index outside [0, S) gives -1: zeros on the quantize side, nothing
// stored on the dequantize side.

struct SegArgs {
  Mx8SegDesc s[kMaxMx8SegsPerLaunch];
};

// Segment blockIdx.y of the launch as a mapped stream: cps chunks per slice,
// cpr = count*cps per row.
template <typename I, int MODE>
struct SegMap {
  static constexpr bool kCanMiss = true;
  long long displ, goff;
  const long long* __restrict__ idx;
  long long S;
  I cps, cpr, chunks;
  __device__ SegMap(const Mx8SegDesc& d, const long long* idx, long long S,
                    I cps, long long rows)
      : displ(d.displ), goff(d.goff), idx(idx), S(S), cps(cps),
        cpr((I)d.count * cps), chunks((I)rows * cpr) {}
  __device__ long long operator()(I i) const {
    if constexpr (MODE == 0) {
      const I row = i / cpr;
      const I col = i - row * cpr;
      return ((long long)row * S + displ) * (long long)cps + (long long)col;
    } else if constexpr (MODE == 1) {
      const I c = i / cps;
      const I col = i - c * cps;
      const long long t = idx[displ + (long long)c];
      return (unsigned long long)t < (unsigned long long)S
                 ? t * (long long)cps + (long long)col
                 : -1;
    } else {
      const I row = i / cpr;
      const I rem = i - row * cpr;
      const I c = rem / cps;
      const I col = rem - c * cps;
      const long long t = idx[displ + (long long)c];
      return (unsigned long long)t < (unsigned long long)S
                 ? ((long long)row * S + t) * (long long)cps + (long long)col
                 : -1;
    }
  }
};

// quantize_stream over the segment's G_p*LPG lane slots.
template <int K, typename I, int MODE>
__global__ __launch_bounds__(256) void mx8_quantize_segments_kernel(
    const void* __restrict__ in, const long long* __restrict__ idx,
    u8* __restrict__ pay, u8* __restrict__ sc, SegArgs segs, long long S,
    I cps, long long rows) {
  if (segs.s[blockIdx.y].count == 0) return;
  const SegMap<I, MODE> map(segs.s[blockIdx.y], idx, S, cps, rows);
  const long long G = ((long long)map.chunks + kLPG<K> - 1) / kLPG<K>;
  quantize_stream<K, I>(in, pay + map.goff * 32, sc + map.goff, G, map.chunks,
                        (I)(G * kLPG<K>), map, MX8_GRID_STRIDE(I));
}

// dequantize_stream over the segment's L_p/EPL chunks.
template <int K, typename I, int MODE>
__global__ __launch_bounds__(256) void mx8_dequantize_segments_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ idx, void* __restrict__ out, SegArgs segs,
    long long S, I cps, long long rows) {
  if (segs.s[blockIdx.y].count == 0) return;
  const SegMap<I, MODE> map(segs.s[blockIdx.y], idx, S, cps, rows);
  dequantize_stream<K, I>(pay + map.goff * 32, sc + map.goff, out, map.chunks,
                          map, MX8_GRID_STRIDE(I));
}

// General twins: any slice length, any alignment of the bases (an odd
// `after`, a contiguous x[1:] view). One thread per group on both sides, like
// the first four kernels' twins: the group's first element is mapped to
// (b, c, a) with two divisions and the 32 elements are walked from there,
// the slice index reloaded whenever c changes. Token rows of an MoE layer
// (after % EPL == 0, allocator-aligned bases) never take them.

// Position (b, c, a) of a stream element of segment d and its tensor slice t.
template <bool IDX>
struct SegCursor {
  const Mx8SegDesc& d;
  const long long* __restrict__ idx;
  long long S, after, L;  // L: elements in the segment's stream
  long long e, b, c, a, t;

  __device__ SegCursor(const Mx8SegDesc& d, const long long* idx, long long S,
                       long long after, long long rows)
      : d(d), idx(idx), S(S), after(after), L(rows * d.count * after) {}
  __device__ long long slice() const {
    return IDX ? idx[d.displ + c] : d.displ + c;
  }
  // to stream element e0, which must exist
  __device__ void seek(long long e0) {
    const long long run = d.count * after;
    e = e0;
    b = e0 / run;
    const long long rem = e0 - b * run;
    c = rem / after;
    a = rem - c * after;
    t = slice();
  }
  __device__ bool in_stream() const { return e < L; }
  // the current element's tensor offset, or -1 when its slice index is
  // outside [0, S)
  __device__ long long offset() const {
    return (unsigned long long)t < (unsigned long long)S
               ? (b * S + t) * after + a
               : -1;
  }
  // one element on; the slice index is reloaded whenever c changes, but
  // never for an element past the stream
  __device__ void advance() {
    ++e;
    if (++a == after) {
      a = 0;
      if (++c == d.count) {
        c = 0;
        ++b;
      }
      if (e < L) t = slice();
    }
  }
};

// The quantizing twin's walk over segment d, one thread per group. An
// element past the stream is a zero; one whose slice index is outside
// [0, S) is pre.elem(c, 0): a weight still multiplies it. Inlined by force,
// like the combine bodies below: the kernel is then optimised as the one
// function it used to be (left to the inliner's own time, the 32-element
// loop is unrolled in the body first and the code grows 2.5 times).
template <int K, bool IDX, typename Pre = NoPre>
__device__ __forceinline__ void quantize_segment_scalar(
    const void* __restrict__ in, const long long* __restrict__ idx,
    u8* __restrict__ pay, u8* __restrict__ sc, const Mx8SegDesc& d,
    long long S, long long after, long long rows, long long first,
    long long stride, const Pre& pre = Pre{}) {
  using T = typename Elem<K>::type;
  if (d.count == 0) return;
  SegCursor<IDX> cur(d, idx, S, after, rows);
  const long long G = (cur.L + 31) / 32;
  const T* __restrict__ src = reinterpret_cast<const T*>(in);
  for (long long g = first; g < G; g += stride) {
    cur.seek(g * 32);
    float x[32];
    for (int k = 0; k < 32; ++k) {
      x[k] = 0.0f;
      if (cur.in_stream()) {
        const long long o = cur.offset();
        if (o >= 0) x[k] = elem_to_f32<K>(src[o]);
        x[k] = pre.elem(cur.c, x[k]);
        cur.advance();
      }
    }
    encode_group_scalar(x, pay + (d.goff + g) * 32, sc + d.goff + g);
  }
}

template <int K, bool IDX>
__global__ __launch_bounds__(256) void mx8_quantize_segments_kernel_scalar(
    const void* __restrict__ in, const long long* __restrict__ idx,
    u8* __restrict__ pay, u8* __restrict__ sc, SegArgs segs, long long S,
    long long after, long long rows) {
  quantize_segment_scalar<K, IDX>(in, idx, pay, sc, segs.s[blockIdx.y], S,
                                  after, rows, MX8_GRID_STRIDE(long long));
}

template <int K, bool IDX>
__global__ __launch_bounds__(256) void mx8_dequantize_segments_kernel_scalar(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ idx, void* __restrict__ out, SegArgs segs,
    long long S, long long after, long long rows) {
  using T = typename Elem<K>::type;
  const Mx8SegDesc& d = segs.s[blockIdx.y];
  if (d.count == 0) return;
  SegCursor<IDX> cur(d, idx, S, after, rows);
  const long long G = (cur.L + 31) / 32;
  T* __restrict__ dst = reinterpret_cast<T*>(out);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    cur.seek(g * 32);
    const int sb = sc[d.goff + g];
    const u8* __restrict__ p = pay + (d.goff + g) * 32;
    for (int k = 0; k < 32 && cur.in_stream(); ++k, cur.advance()) {
      const long long o = cur.offset();
      if (o >= 0) dst[o] = f32_to_elem<K>(mx8_dequant(p[k], sb));
    }
  }
}

// ---- quantize_segments_weighted (the head of the weighted combine's
// backward) ------------------------------------------------------------------
//
// quantize_segments for rows == 1 with one fp32 weight per stream slice:
// stream slice c of segment p is fl32(w[displ_p + c] * f32(slice)), and the
// group's amax is taken over the products. The product is a single fp32
// multiply and never passes through the tensor's dtype.

// One fp32 multiply / add, rounded on its own. The weighted kernels owe the
// composite exactly these, so they are spelled as the single VALU
// instruction: the compiler can neither contract a pair into an FMA nor fold
// neighbours into the packed two-lane forms. Compiled for another target,
// a plain a * b / a + b under contraction off is the fallback.
__device__ inline float mul_single(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ inline float add_single(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// pre() of quantize_stream: chunk i belongs to stream slice i / cps of the
// segment, whose weight is one cached 4-byte load shared by the slice's
// chunks (the division is the map's own). elem() is the general twins' form:
// they know the slice.
template <typename I>
struct SliceWeight {
  const float* __restrict__ w;  // the segment's first weight
  I cps;
  template <int N>
  __device__ void operator()(I i, float (&x)[N]) const {
    const float wi = w[i / cps];
    for (int k = 0; k < N; ++k) x[k] = mul_single(wi, x[k]);
  }
  __device__ float elem(long long c, float v) const {
    return mul_single(w[c], v);
  }
};

// MODE 0 (no index) or 1 of SegMap; with rows == 1 a segment's chunks are
// its slices' chunks one after the other under both.
template <int K, typename I, int MODE>
__global__ __launch_bounds__(256) void mx8_quantize_segments_weighted_kernel(
    const void* __restrict__ in, const long long* __restrict__ idx,
    const float* __restrict__ wt, u8* __restrict__ pay, u8* __restrict__ sc,
    SegArgs segs, long long S, I cps) {
  if (segs.s[blockIdx.y].count == 0) return;
  const SegMap<I, MODE> map(segs.s[blockIdx.y], idx, S, cps, 1);
  const long long G = ((long long)map.chunks + kLPG<K> - 1) / kLPG<K>;
  quantize_stream<K, I>(in, pay + map.goff * 32, sc + map.goff, G, map.chunks,
                        (I)(G * kLPG<K>), map, MX8_GRID_STRIDE(I),
                        SliceWeight<I>{wt + map.displ, cps});
}

// General twin: the segments twin's walk with the weight of the cursor's
// stream slice (cps counts elements here).
template <int K, bool IDX>
__global__ __launch_bounds__(256)
void mx8_quantize_segments_weighted_kernel_scalar(
    const void* __restrict__ in, const long long* __restrict__ idx,
    const float* __restrict__ wt, u8* __restrict__ pay, u8* __restrict__ sc,
    SegArgs segs, long long S, long long after) {
  const Mx8SegDesc& d = segs.s[blockIdx.y];
  quantize_segment_scalar<K, IDX>(
      in, idx, pay, sc, d, S, after, 1, MX8_GRID_STRIDE(long long),
      SliceWeight<long long>{wt + d.displ, after});
}

// ---- dequantize_combine (the top-k pairwise all-to-all tail) --------------
//
// The reduce side of the segments tail: several received slices name the
// same output slice and are summed there. The output is [out_slices][after];
// src is an int64 table [out_slices][fan] whose entries are the payload byte
// offset of a received slice's first element, or -1. Segments are streams of
// consecutive elements that start at payload byte 32*goff, so element a of a
// slice at offset o has payload byte o + a and scale byte (o + a) >> 5: the
// kernel needs no descriptor and no segment lookup. Rule, per output element:
//   acc = dq(src[s][0]), or +0.0 when that entry is -1;
//   acc = acc + dq(src[s][j]) for j = 1..fan-1 in that order, -1 skipped;
//   one RNE cast.
// All in fp32; a 255 scale or a NaN payload byte makes its own elements NaN
// through the sum and no others. Exactly out_slices*after elements are
// written, zeros where a slice has no source.
//
// Vector body (after % EPL == 0, out aligned to 16 bytes, payload to EPL): a
// flat grid-stride loop over the out_slices*after/EPL output chunks, one
// division by the chunks per slice. The table entries are plain cached
// 8-byte loads, shared by all chunks of a slice. A slice offset is a
// multiple of EPL (32*goff + c*after), so a chunk's EPL payload bytes are one
// aligned load inside one group. The sources are taken kCombineBatch at a
// time by a compile-time unroll: the table entries, then every payload and
// scale load of the batch, are issued before the first value is consumed, so
// a lane keeps up to four payload loads in flight for its one 16-byte store
// and the staging stays in registers.
//
// The weighted form (the gated top-k tail) has one fp32 weight per table
// entry: wsrc is a table [out_slices][fan] parallel to src, and the rule
// becomes, per output element, in fp32:
//   acc = fl(w0 * dq(src[s][0])), or +0.0 when that entry is -1;
//   acc = acc + fl(w_j * dq(src[s][j])) for j = 1..fan-1, -1 skipped;
//   one RNE cast.
// The product is rounded before the add: mul_single and add_single are never
// contracted, which is what lets the torch composite acc + w*v agree bit for
// bit. A weight of 0 on a NaN source stays NaN (IEEE through the product).
// The vector body loads a weight with its offset (both cached loads shared
// by a slice's chunks), before it knows the offset's sign, so every entry
// must be initialised; one whose offset is -1 is never used (the host
// writes 0).
constexpr int kCombineBatch = 4;

// The weight policy of the combine bodies: row(e) is the policy from table
// entry e on, load(j) what entry j contributes besides its offset,
// term(w, v) the summand of a dequantized value and add(acc, t) the
// accumulation. NoWeight loads nothing (Val is empty) and sums the values
// themselves with the plain acc + v.
struct NoWeight {
  struct Val {};
  __device__ NoWeight row(long long) const { return {}; }
  __device__ Val load(long long) const { return {}; }
  __device__ static float term(Val, float v) { return v; }
  __device__ static float add(float acc, float t) { return acc + t; }
};

struct TableWeight {
  using Val = float;
  const float* __restrict__ wsrc;
  __device__ TableWeight row(long long e) const { return {wsrc + e}; }
  __device__ float load(long long j) const { return wsrc[j]; }
  __device__ static float term(float w, float v) { return mul_single(w, v); }
  __device__ static float add(float acc, float t) {
    return add_single(acc, t);
  }
};

// The vector body over output chunks first, first + stride, ... < chunks of
// cps chunks per slice; the conditions above are the launcher's to check.
template <int K, typename I, typename W>
__device__ __forceinline__ void combine_stream(const u8* __restrict__ pay,
                                      const u8* __restrict__ sc,
                                      const long long* __restrict__ src,
                                      void* __restrict__ out, I chunks, I cps,
                                      int fan, I first, I stride,
                                      const W& wt) {
  constexpr int EPL = kEPL<K>;
  for (I i = first; i < chunks; i += stride) {
    const I s = i / cps;
    const long long col = (long long)(i - s * cps) * EPL;
    const long long* __restrict__ t = src + (long long)s * fan;
    const W tw = wt.row((long long)s * fan);
    float acc[EPL];
    for (int k = 0; k < EPL; ++k) acc[k] = 0.0f;
    for (int j0 = 0; j0 < fan; j0 += kCombineBatch) {
      long long o[kCombineBatch];
      typename W::Val wj[kCombineBatch];
      unsigned w[kCombineBatch][EPL / 4];
      int sb[kCombineBatch];
#pragma unroll
      for (int u = 0; u < kCombineBatch; ++u) {
        o[u] = j0 + u < fan ? t[j0 + u] : -1;
        wj[u] = j0 + u < fan ? tw.load(j0 + u) : typename W::Val{};
      }
#pragma unroll
      for (int u = 0; u < kCombineBatch; ++u) {
        if (o[u] >= 0) {
          const long long b = o[u] + col;
          load_payload<EPL>(pay, b / EPL, w[u]);
          sb[u] = sc[b >> 5];
        }
      }
#pragma unroll
      for (int u = 0; u < kCombineBatch; ++u) {
        if (o[u] >= 0) {
          // source 0 is assigned (it keeps a -0.0), the others are added
          const bool first = u == 0 && j0 == 0;
          for (int d = 0; d < EPL / 4; ++d) {
            for (int k = 0; k < 4; ++k) {
              const float v = W::term(
                  wj[u], mx8_dequant((u8)(w[u][d] >> (8 * k)), sb[u]));
              acc[4 * d + k] = first ? v : W::add(acc[4 * d + k], v);
            }
          }
        }
      }
    }
    __builtin_nontemporal_store(pack16<K, EPL>(acc),
                                reinterpret_cast<v4u*>(out) + i);
  }
}

// The general twins' body: any `after`, any alignment of the bases. One
// thread per output element with the same source loop; token rows never take
// it.
template <int K, typename W>
__device__ __forceinline__ void combine_scalar(const u8* __restrict__ pay,
                                      const u8* __restrict__ sc,
                                      const long long* __restrict__ src,
                                      void* __restrict__ out, long long total,
                                      long long after, int fan,
                                      long long first, long long stride,
                                      const W& wt) {
  using T = typename Elem<K>::type;
  for (long long e = first; e < total; e += stride) {
    const long long s = e / after;
    const long long a = e - s * after;
    float acc = 0.0f;
    for (int j = 0; j < fan; ++j) {
      const long long o = src[s * fan + j];
      if (o < 0) continue;
      const float v = W::term(wt.load(s * fan + j),
                              mx8_dequant(pay[o + a], sc[(o + a) >> 5]));
      acc = j == 0 ? v : W::add(acc, v);
    }
    reinterpret_cast<T*>(out)[e] = f32_to_elem<K>(acc);
  }
}

template <int K, typename I>
__global__ __launch_bounds__(256) void mx8_dequantize_combine_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ src, void* __restrict__ out, I chunks,
    I cps, int fan) {
  combine_stream<K, I>(pay, sc, src, out, chunks, cps, fan,
                       MX8_GRID_STRIDE(I), NoWeight{});
}

template <int K>
__global__ __launch_bounds__(256) void mx8_dequantize_combine_kernel_scalar(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ src, void* __restrict__ out,
    long long total, long long after, int fan) {
  combine_scalar<K>(pay, sc, src, out, total, after, fan,
                    MX8_GRID_STRIDE(long long), NoWeight{});
}

template <int K, typename I>
__global__ __launch_bounds__(256) void mx8_dequantize_combine_weighted_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ src, const float* __restrict__ wsrc,
    void* __restrict__ out, I chunks, I cps, int fan) {
  combine_stream<K, I>(pay, sc, src, out, chunks, cps, fan,
                       MX8_GRID_STRIDE(I), TableWeight{wsrc});
}

template <int K>
__global__ __launch_bounds__(256)
void mx8_dequantize_combine_weighted_kernel_scalar(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ src, const float* __restrict__ wsrc,
    void* __restrict__ out, long long total, long long after, int fan) {
  combine_scalar<K>(pay, sc, src, out, total, after, fan,
                    MX8_GRID_STRIDE(long long), TableWeight{wsrc});
}

// ---- dequantize_rowdot (the gate gradient of the weighted tail) -----------
//
// gw[i] = sum_a dq(received slice i)[a] * f32(g[index[i]][a]) for the R
// received slices of `after` elements; base[i] is slice i's payload byte
// offset (what the combine table is built from), g is [out_slices][after]
// of the tensor dtype, gw is fp32. A slice whose index lies outside
// [0, out_slices) gives exactly 0; a 255 scale or a NaN payload byte makes
// its own slice's result NaN. A reduction, so unlike the stream kernels it
// owns its order of association: fixed, hence the same bits on every run,
// but not the composite's. No atomics, no LDS.
//
// Vector body (after % EPL == 0, g aligned to 16 bytes, payload to EPL): a
// group of LPS lanes owns a slice, LPS in {8, 16, 32, 64} the smallest that
// is not below the cps chunks of a slice, so a 64-element bf16 row fills 8
// lanes and a wave does 8 slices at once, and a 4096-element one takes the
// whole wave for 8 trips. A lane's trip is one chunk: EPL payload bytes, the
// scale byte, the 16-byte chunk of g (a cached load: the k slices of a token
// read the same row), EPL fused multiply-adds into one fp32 accumulator. Two
// trips' loads are issued before the first is consumed. index[i] and base[i]
// are loaded by the group's first lane and broadcast. The lanes then add up
// by xor-shuffles below LPS and the first lane stores. Both loops have
// wave-uniform trip counts (the slice loop runs on the wave's first slice,
// the chunk loop on cps), so every lane is present at every shuffle; a lane
// without a chunk, or of a slice past R or out of range, carries zeros.
template <int K, int LPS, typename I>
__global__ __launch_bounds__(256) void mx8_dequantize_rowdot_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ base, const long long* __restrict__ idx,
    const void* __restrict__ g, float* __restrict__ gw, I R, I cps,
    long long out_slices) {
  constexpr int EPL = kEPL<K>;
  constexpr int SPW = 64 / LPS;  // slices per wave
  const int sub = threadIdx.x & (LPS - 1);
  const I stride = (I)gridDim.x * (256 / LPS);
  for (I s0 = ((I)blockIdx.x * 256 + (threadIdx.x & ~63)) / LPS; s0 < R;
       s0 += stride) {
    const I s = s0 + (I)((threadIdx.x & 63) / LPS);
    long long t = -1, o = 0;
    if (sub == 0 && s < R) {
      t = idx[s];
      o = base[s];
    }
    if constexpr (SPW == 1) {
      t = __shfl(t, 0);
      o = __shfl(o, 0);
    } else {
      t = __shfl(t, 0, LPS);
      o = __shfl(o, 0, LPS);
    }
    const bool ok = (unsigned long long)t < (unsigned long long)out_slices;
    const long long pslot = o / EPL;   // o is a multiple of EPL
    const long long gslot = t * (long long)cps;
    float acc = 0.0f;
    for (I c0 = 0; c0 < cps; c0 += 2 * LPS) {
      unsigned w[2][EPL / 4];
      int sb[2];
      v4u gv[2];
      bool act[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const I c = c0 + (I)(u * LPS + sub);
        act[u] = ok && c < cps;
        if (act[u]) {
          load_payload<EPL>(pay, pslot + (long long)c, w[u]);
          sb[u] = sc[(o + (long long)c * EPL) >> 5];
          gv[u] = reinterpret_cast<const v4u*>(g)[gslot + (long long)c];
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (act[u]) {
          float x[EPL];
          unpack16<K, EPL>(gv[u], x);
          for (int d = 0; d < EPL / 4; ++d) {
            for (int k = 0; k < 4; ++k) {
              acc = fmaf(mx8_dequant((u8)(w[u][d] >> (8 * k)), sb[u]),
                         x[4 * d + k], acc);
            }
          }
        }
      }
    }
    for (int m = LPS / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (sub == 0 && s < R) gw[s] = ok ? acc : 0.0f;
  }
}

// General twin: any `after`, any alignment. One thread per slice walks its
// elements in order.
template <int K>
__global__ __launch_bounds__(256) void mx8_dequantize_rowdot_kernel_scalar(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    const long long* __restrict__ base, const long long* __restrict__ idx,
    const void* __restrict__ g, float* __restrict__ gw, long long R,
    long long after, long long out_slices) {
  using T = typename Elem<K>::type;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < R;
       s += stride) {
    const long long t = idx[s];
    float acc = 0.0f;
    if ((unsigned long long)t < (unsigned long long)out_slices) {
      const long long o = base[s];
      const T* __restrict__ row = reinterpret_cast<const T*>(g) + t * after;
      for (long long a = 0; a < after; ++a) {
        acc = fmaf(mx8_dequant(pay[o + a], sc[(o + a) >> 5]),
                   elem_to_f32<K>(row[a]), acc);
      }
    }
    gw[s] = acc;
  }
}

inline unsigned grid_for(long long work) {
  long long blocks = (work + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// grid.y carries the block or segment; grid.x is capped so the launch stays
// near the 4096 workgroups of the flat kernels
inline dim3 grid2d(long long work, int ny) {
  const long long xcap = 4096 / ny > 0 ? 4096 / ny : 1;
  long long x = (work + 255) / 256;
  if (x > xcap) x = xcap;
  if (x < 1) x = 1;
  return dim3((unsigned)x, (unsigned)ny);
}

inline bool aligned(const void* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

template <int V> using Tag = std::integral_constant<int, V>;

// f(Tag<K>) for the dtype code of kernels.hpp
template <typename F>
void by_dtype(int dtype, F&& f) {
  switch (dtype) {
    case 0: f(Tag<kF32>{}); break;
    case 1: f(Tag<kBF16>{}); break;
    default: f(Tag<kF16>{}); break;
  }
}

// f(I) with a value of the per-lane index type: 32 bits whenever `work` lane
// slots fit
template <typename F>
void by_width(long long work, F&& f) {
  if (work < (1ll << 31)) {
    f(0u);
  } else {
    f(0ll);
  }
}

// f(I, Tag<MODE>) for a segments vector kernel (MODE as at SegMap)
template <typename F>
void by_width_mode(long long work, bool indexed, int64_t rows, F&& f) {
  by_width(work, [&](auto i) {
    if (!indexed) {
      f(i, Tag<0>{});
    } else if (rows == 1) {
      f(i, Tag<1>{});
    } else {
      f(i, Tag<2>{});
    }
  });
}

// key: nothing, or the SrKey of the stochastic kernels
template <int K, typename... Key>
void launch_quantize_t(const void* in, void* pay, void* sc, int64_t N,
                       hipStream_t stream, Key... key) {
  constexpr int LPG = kLPG<K>;
  const long long G = (N + 31) / 32;
  const long long nfull = N / 32;
  if (aligned(in, 16) && aligned(pay, 32 / LPG)) {
    hipLaunchKernelGGL((mx8_quantize_kernel<K, Key...>),
                       dim3(grid_for(nfull * LPG)), dim3(256), 0, stream, in,
                       static_cast<u8*>(pay), static_cast<u8*>(sc), nfull,
                       (long long)N, key...);
  } else {
    hipLaunchKernelGGL((mx8_quantize_kernel_scalar<K, Key...>),
                       dim3(grid_for(G)), dim3(256), 0, stream, in,
                       static_cast<u8*>(pay), static_cast<u8*>(sc), G,
                       (long long)N, key...);
  }
}

template <typename... Key>
void launch_reduce_t(const void* payload_in, const void* scales_in,
                     void* payload_out, void* scales_out, int64_t n_groups,
                     int nranks, hipStream_t stream, Key... key) {
  const u8* pin = static_cast<const u8*>(payload_in);
  const u8* sin = static_cast<const u8*>(scales_in);
  u8* pout = static_cast<u8*>(payload_out);
  u8* sout = static_cast<u8*>(scales_out);
  if (aligned(pin, 16) && aligned(pout, 16)) {
    hipLaunchKernelGGL((mx8_reduce_kernel<Key...>),
                       dim3(grid_for(n_groups * 2)), dim3(256), 0, stream, pin,
                       sin, pout, sout, (long long)n_groups,
                       (long long)nranks, key...);
  } else {
    hipLaunchKernelGGL((mx8_reduce_kernel_scalar<Key...>),
                       dim3(grid_for(n_groups)), dim3(256), 0, stream, pin,
                       sin, pout, sout, (long long)n_groups,
                       (long long)nranks, key...);
  }
}

// n0: stream index of the first element, a multiple of 32
inline SrKey sr_key(uint32_t k0, uint32_t k1, int64_t n0) {
  return SrKey{k0, k1, (long long)(n0 >> 1)};
}

template <int K>
void launch_dequantize_t(const void* pay, const void* sc, void* out, int64_t N,
                         hipStream_t stream) {
  constexpr int LPG = K == kF32 ? 8 : 4;
  const long long G = (N + 31) / 32;
  const long long nfull = N / 32;
  if (aligned(out, 16) && aligned(pay, 32 / LPG)) {
    hipLaunchKernelGGL((mx8_dequantize_kernel<K>),
                       dim3(grid_for(nfull * LPG)), dim3(256), 0, stream,
                       static_cast<const u8*>(pay),
                       static_cast<const u8*>(sc), out, nfull, (long long)N);
  } else {
    hipLaunchKernelGGL((mx8_dequantize_kernel_scalar<K>), dim3(grid_for(G)),
                       dim3(256), 0, stream, static_cast<const u8*>(pay),
                       static_cast<const u8*>(sc), out, G, (long long)N);
  }
}

template <int K>
void launch_reduce_to_t(const u8* pin, const u8* sin, void* out, int64_t N,
                        int nranks, hipStream_t stream) {
  const long long G = (N + 31) / 32;
  const long long nfull = N / 32;
  // The vector body indexes every copy from pin with stride G*32, a multiple
  // of 16, so an aligned base keeps every copy aligned.
  if (aligned(pin, 16) && aligned(out, 16)) {
    hipLaunchKernelGGL((mx8_reduce_to_kernel<K>),
                       dim3(grid_for(nfull * (K == kF32 ? 4 : 2))), dim3(256),
                       0, stream, pin, sin, out, nfull, G, (long long)N,
                       (long long)nranks);
  } else {
    hipLaunchKernelGGL((mx8_reduce_to_kernel_scalar<K>), dim3(grid_for(G)),
                       dim3(256), 0, stream, pin, sin, out, G, (long long)N,
                       (long long)nranks);
  }
}

template <int K>
void launch_dequantize_blocks_t(const u8* pay, const u8* sc, void* out,
                                int nblocks, int64_t rows, int64_t row_elems,
                                hipStream_t stream) {
  constexpr int LPG = kLPG<K>;
  constexpr int EPL = kEPL<K>;
  const long long L = rows * row_elems;
  const long long Gb = (L + 31) / 32;
  // Every block's payload base is pay + r*Gb*32, so an aligned pay keeps all
  // of them aligned; row_elems % EPL == 0 with an aligned out keeps every
  // chunk's destination aligned.
  const bool al = aligned(out, 16) && aligned(pay, 32 / LPG);
  if (al && rows == 1 && L % 32 == 0) {
    // the gathered buffer is one flat mxfp8 stream of nblocks*L elements
    launch_dequantize_t<K>(pay, sc, out, (int64_t)nblocks * L, stream);
    return;
  }
  if (al && row_elems % EPL == 0) {
    const long long chunks = L / EPL;
    const long long cpr = row_elems / EPL;
    by_width(chunks, [&](auto i) {
      using I = decltype(i);
      hipLaunchKernelGGL((mx8_dequantize_blocks_kernel<K, I>),
                         grid2d(chunks, nblocks), dim3(256), 0, stream, pay,
                         sc, out, Gb, (I)chunks, (I)cpr, (long long)nblocks);
    });
  } else {
    const long long slots = row_elems / EPL + 2;
    const long long total = rows * slots;
    by_width(total, [&](auto i) {
      using I = decltype(i);
      hipLaunchKernelGGL((mx8_dequantize_blocks_kernel_shifted<K, I>),
                         grid2d(total, nblocks), dim3(256), 0, stream, pay, sc,
                         out, Gb, (long long)row_elems, (I)slots, (I)total,
                         (long long)nblocks);
    });
  }
}

template <int K>
void launch_quantize_blocks_t(const void* in, u8* pay, u8* sc, int nblocks,
                              int64_t rows, int64_t row_elems,
                              hipStream_t stream) {
  constexpr int LPG = kLPG<K>;
  constexpr int EPL = kEPL<K>;
  const long long L = rows * row_elems;
  const long long Gb = (L + 31) / 32;
  // Every block's payload base is pay + r*Gb*32, so an aligned pay keeps all
  // of them aligned; row_elems % EPL == 0 with an aligned in keeps every
  // chunk's source aligned.
  const bool al = aligned(in, 16) && aligned(pay, 32 / LPG);
  if (al && rows == 1 && L % 32 == 0) {
    // the input is one flat stream of nblocks*L elements whose groups
    // coincide with the blocks' groups
    launch_quantize_t<K>(in, pay, sc, (int64_t)nblocks * L, stream);
    return;
  }
  if (al && row_elems % EPL == 0) {
    const long long chunks = L / EPL;
    const long long cpr = row_elems / EPL;
    const long long slots = Gb * LPG;
    by_width(slots, [&](auto i) {
      using I = decltype(i);
      hipLaunchKernelGGL((mx8_quantize_blocks_kernel<K, I>),
                         grid2d(slots, nblocks), dim3(256), 0, stream, in, pay,
                         sc, Gb, (I)chunks, (I)cpr, (I)slots,
                         (long long)nblocks);
    });
  } else {
    hipLaunchKernelGGL((mx8_quantize_blocks_kernel_scalar<K>),
                       grid2d(Gb, nblocks), dim3(256), 0, stream, in, pay, sc,
                       Gb, L, (long long)row_elems, (long long)nblocks);
  }
}

// One launch's worth of segments: the descriptors by value, the largest
// count (grid.x is sized for it) and the number of non-empty segments.
struct SegBatch {
  SegArgs args{};
  int n = 0;
  long long max_count = 0;
};

inline SegBatch seg_batch(const Mx8SegDesc* segs, int n) {
  SegBatch b;
  b.n = n;
  for (int k = 0; k < n; ++k) {
    b.args.s[k] = segs[k];
    if (segs[k].count > b.max_count) b.max_count = segs[k].count;
  }
  return b;
}

// f(batch) for every launch's worth of the segments that has a non-empty one.
template <typename F>
void for_seg_batches(const Mx8SegDesc* segs, int nsegs, F&& f) {
  for (int s0 = 0; s0 < nsegs; s0 += kMaxMx8SegsPerLaunch) {
    const int n = nsegs - s0 < kMaxMx8SegsPerLaunch ? nsegs - s0
                                                    : kMaxMx8SegsPerLaunch;
    const SegBatch b = seg_batch(segs + s0, n);
    if (b.max_count > 0) f(b);
  }
}

// f(std::bool_constant<indexed>) for a general twin or a rows == 1 MODE
template <typename F>
void by_indexed(const long long* idx, F&& f) {
  if (idx == nullptr) {
    f(std::false_type{});
  } else {
    f(std::true_type{});
  }
}

// With no index, rows == 1 and every L_p a multiple of 32, segments that
// follow each other on both sides form one flat mxfp8 stream. Returns its
// element count, or -1 when the segments are not of that shape; *first
// receives the first non-empty segment.
inline long long flat_stream_of(const Mx8SegDesc* segs, int nsegs,
                                int64_t after, int* first) {
  long long total = 0;
  *first = -1;
  for (int k = 0; k < nsegs; ++k) {
    if (segs[k].count == 0) continue;
    const long long L = segs[k].count * after;
    if (L % 32 != 0) return -1;
    if (*first < 0) {
      *first = k;
    } else {
      const Mx8SegDesc& f = segs[*first];
      if ((segs[k].displ - f.displ) * after != total ||
          (segs[k].goff - f.goff) * 32 != total) {
        return -1;
      }
    }
    total += L;
  }
  return total;
}

// Both segments launchers. Q is the direction: quantizing reads the tensor
// and writes the wire bytes, dequantizing the other way round.
template <int K, bool Q>
void launch_segments_t(std::conditional_t<Q, const void, void>* tensor,
                       const long long* idx,
                       std::conditional_t<Q, u8, const u8>* pay,
                       std::conditional_t<Q, u8, const u8>* sc,
                       const Mx8SegDesc* segs, int nsegs, int64_t rows,
                       int64_t S, int64_t after, hipStream_t stream) {
  using T = std::conditional_t<Q, const typename Elem<K>::type,
                               typename Elem<K>::type>;
  constexpr int LPG = kLPG<K>;
  constexpr int EPL = kEPL<K>;
  // Every segment's payload base is pay + 32*goff, so an aligned pay keeps
  // all of them aligned; after % EPL == 0 with an aligned tensor keeps every
  // chunk's place in it aligned.
  const bool al = aligned(tensor, 16) && aligned(pay, 32 / LPG);
  if (al && idx == nullptr && rows == 1) {
    int first;
    const long long total = flat_stream_of(segs, nsegs, after, &first);
    if (total == 0) return;
    if (total > 0) {
      T* base = reinterpret_cast<T*>(tensor) + segs[first].displ * after;
      if (aligned(base, 16)) {
        auto* p = pay + segs[first].goff * 32;
        auto* s = sc + segs[first].goff;
        if constexpr (Q) {
          launch_quantize_t<K>(base, p, s, total, stream);
        } else {
          launch_dequantize_t<K>(p, s, base, total, stream);
        }
        return;
      }
    }
  }
  for_seg_batches(segs, nsegs, [&](const SegBatch& b) {
    const int n = b.n;
    if (al && after % EPL == 0) {
      const long long cps = after / EPL;
      const long long chunks = rows * b.max_count * cps;
      // lane slots of the largest segment: whole groups when quantizing
      const long long work = Q ? (chunks + LPG - 1) / LPG * LPG : chunks;
      by_width_mode(work, idx != nullptr, rows, [&](auto i, auto mode) {
        using I = decltype(i);
        constexpr int MODE = decltype(mode)::value;
        if constexpr (Q) {
          hipLaunchKernelGGL((mx8_quantize_segments_kernel<K, I, MODE>),
                             grid2d(work, n), dim3(256), 0, stream, tensor,
                             idx, pay, sc, b.args, (long long)S, (I)cps,
                             (long long)rows);
        } else {
          hipLaunchKernelGGL((mx8_dequantize_segments_kernel<K, I, MODE>),
                             grid2d(work, n), dim3(256), 0, stream, pay, sc,
                             idx, tensor, b.args, (long long)S, (I)cps,
                             (long long)rows);
        }
      });
    } else {
      const long long G = (rows * b.max_count * after + 31) / 32;
      by_indexed(idx, [&](auto indexed) {
        constexpr bool IDX = decltype(indexed)::value;
        if constexpr (Q) {
          hipLaunchKernelGGL((mx8_quantize_segments_kernel_scalar<K, IDX>),
                             grid2d(G, n), dim3(256), 0, stream, tensor, idx,
                             pay, sc, b.args, (long long)S, (long long)after,
                             (long long)rows);
        } else {
          hipLaunchKernelGGL((mx8_dequantize_segments_kernel_scalar<K, IDX>),
                             grid2d(G, n), dim3(256), 0, stream, pay, sc, idx,
                             tensor, b.args, (long long)S, (long long)after,
                             (long long)rows);
        }
      });
    }
  });
}

// Both combine launchers: wsrc is the weight table, null for the unweighted
// kernels, which take no such argument.
template <int K>
void launch_dequantize_combine_t(const u8* pay, const u8* sc,
                                 const long long* src, const float* wsrc,
                                 void* out, int64_t out_slices, int fan,
                                 int64_t after, hipStream_t stream) {
  constexpr int EPL = kEPL<K>;
  // Every slice offset is 32*goff + c*after, a multiple of EPL when after
  // is, so a payload base aligned to EPL keeps every chunk's load aligned.
  if (after % EPL == 0 && aligned(out, 16) && aligned(pay, EPL)) {
    const long long cps = after / EPL;
    const long long chunks = out_slices * cps;
    by_width(chunks, [&](auto i) {
      using I = decltype(i);
      const dim3 grid(grid_for(chunks));
      if (wsrc == nullptr) {
        hipLaunchKernelGGL((mx8_dequantize_combine_kernel<K, I>), grid,
                           dim3(256), 0, stream, pay, sc, src, out, (I)chunks,
                           (I)cps, fan);
      } else {
        hipLaunchKernelGGL((mx8_dequantize_combine_weighted_kernel<K, I>),
                           grid, dim3(256), 0, stream, pay, sc, src, wsrc, out,
                           (I)chunks, (I)cps, fan);
      }
    });
  } else {
    const long long total = out_slices * after;
    const dim3 grid(grid_for(total));
    if (wsrc == nullptr) {
      hipLaunchKernelGGL((mx8_dequantize_combine_kernel_scalar<K>), grid,
                         dim3(256), 0, stream, pay, sc, src, out, total,
                         (long long)after, fan);
    } else {
      hipLaunchKernelGGL((mx8_dequantize_combine_weighted_kernel_scalar<K>),
                         grid, dim3(256), 0, stream, pay, sc, src, wsrc, out,
                         total, (long long)after, fan);
    }
  }
}

// launch_segments_t's quantizing side for rows == 1 with weights; no flat
// stream shortcut, the flat kernel takes no weights.
template <int K>
void launch_quantize_segments_weighted_t(const void* in, const long long* idx,
                                         const float* wt, u8* pay, u8* sc,
                                         const Mx8SegDesc* segs, int nsegs,
                                         int64_t S, int64_t after,
                                         hipStream_t stream) {
  constexpr int LPG = kLPG<K>;
  constexpr int EPL = kEPL<K>;
  const bool al = aligned(in, 16) && aligned(pay, 32 / LPG);
  for_seg_batches(segs, nsegs, [&](const SegBatch& b) {
    if (al && after % EPL == 0) {
      const long long cps = after / EPL;
      const long long work = (b.max_count * cps + LPG - 1) / LPG * LPG;
      by_width(work, [&](auto i) {
        using I = decltype(i);
        by_indexed(idx, [&](auto indexed) {
          constexpr int MODE = decltype(indexed)::value ? 1 : 0;
          hipLaunchKernelGGL(
              (mx8_quantize_segments_weighted_kernel<K, I, MODE>),
              grid2d(work, b.n), dim3(256), 0, stream, in, idx, wt, pay, sc,
              b.args, (long long)S, (I)cps);
        });
      });
    } else {
      const long long G = (b.max_count * after + 31) / 32;
      by_indexed(idx, [&](auto indexed) {
        constexpr bool IDX = decltype(indexed)::value;
        hipLaunchKernelGGL(
            (mx8_quantize_segments_weighted_kernel_scalar<K, IDX>),
            grid2d(G, b.n), dim3(256), 0, stream, in, idx, wt, pay, sc, b.args,
            (long long)S, (long long)after);
      });
    }
  });
}

template <int K>
void launch_dequantize_rowdot_t(const u8* pay, const u8* sc,
                                const long long* base, const long long* idx,
                                const void* g, float* gw, int64_t R,
                                int64_t out_slices, int64_t after,
                                hipStream_t stream) {
  constexpr int EPL = kEPL<K>;
  if (after % EPL == 0 && aligned(g, 16) && aligned(pay, EPL)) {
    const long long cps = after / EPL;
    // the widest per-lane index: a chunk of g, or a slice's padded sweep
    const long long most = (R > out_slices ? R : out_slices) * cps + 128;
    by_width(most, [&](auto i) {
      using I = decltype(i);
      auto go = [&](auto lps) {
        constexpr int LPS = decltype(lps)::value;
        hipLaunchKernelGGL((mx8_dequantize_rowdot_kernel<K, LPS, I>),
                           dim3(grid_for(R * LPS)), dim3(256), 0, stream, pay,
                           sc, base, idx, g, gw, (I)R, (I)cps,
                           (long long)out_slices);
      };
      if (cps <= 8) {
        go(Tag<8>{});
      } else if (cps <= 16) {
        go(Tag<16>{});
      } else if (cps <= 32) {
        go(Tag<32>{});
      } else {
        go(Tag<64>{});
      }
    });
  } else {
    hipLaunchKernelGGL((mx8_dequantize_rowdot_kernel_scalar<K>),
                       dim3(grid_for(R)), dim3(256), 0, stream, pay, sc, base,
                       idx, g, gw, (long long)R, (long long)after,
                       (long long)out_slices);
  }
}

} // namespace

void launch_mx8_dequantize_combine_weighted(
    const void* payload, const void* scales, const int64_t* src,
    const float* wsrc, void* out, int64_t out_slices, int fan, int64_t after,
    int dtype, hipStream_t stream) {
  if (out_slices <= 0 || after <= 0 || fan <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_dequantize_combine_t<k>(
        static_cast<const u8*>(payload), static_cast<const u8*>(scales),
        reinterpret_cast<const long long*>(src), wsrc, out, out_slices, fan,
        after, stream);
  });
}

void launch_mx8_quantize_segments_weighted(
    const void* in, const int64_t* idx, const float* weights, void* payload,
    void* scales, const Mx8SegDesc* segs, int nsegs, int64_t S, int64_t after,
    int dtype, hipStream_t stream) {
  if (nsegs <= 0 || S <= 0 || after <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_quantize_segments_weighted_t<k>(
        in, reinterpret_cast<const long long*>(idx), weights,
        static_cast<u8*>(payload), static_cast<u8*>(scales), segs, nsegs, S,
        after, stream);
  });
}

void launch_mx8_dequantize_rowdot(const void* payload, const void* scales,
                                  const int64_t* base, const int64_t* idx,
                                  const void* g, float* gw, int64_t R,
                                  int64_t out_slices, int64_t after, int dtype,
                                  hipStream_t stream) {
  if (R <= 0 || after <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_dequantize_rowdot_t<k>(
        static_cast<const u8*>(payload), static_cast<const u8*>(scales),
        reinterpret_cast<const long long*>(base),
        reinterpret_cast<const long long*>(idx), g, gw, R, out_slices, after,
        stream);
  });
}

void launch_mx8_dequantize_combine(const void* payload, const void* scales,
                                   const int64_t* src, void* out,
                                   int64_t out_slices, int fan, int64_t after,
                                   int dtype, hipStream_t stream) {
  launch_mx8_dequantize_combine_weighted(payload, scales, src, nullptr, out,
                                         out_slices, fan, after, dtype,
                                         stream);
}

void launch_mx8_quantize_segments(const void* in, const int64_t* idx,
                                  void* payload, void* scales,
                                  const Mx8SegDesc* segs, int nsegs,
                                  int64_t rows, int64_t S, int64_t after,
                                  int dtype, hipStream_t stream) {
  if (nsegs <= 0 || rows <= 0 || S <= 0 || after <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_segments_t<k, true>(in, reinterpret_cast<const long long*>(idx),
                               static_cast<u8*>(payload),
                               static_cast<u8*>(scales), segs, nsegs, rows, S,
                               after, stream);
  });
}

void launch_mx8_dequantize_segments(const void* payload, const void* scales,
                                    const int64_t* idx, void* out,
                                    const Mx8SegDesc* segs, int nsegs,
                                    int64_t rows, int64_t S, int64_t after,
                                    int dtype, hipStream_t stream) {
  if (nsegs <= 0 || rows <= 0 || S <= 0 || after <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_segments_t<k, false>(out, reinterpret_cast<const long long*>(idx),
                                static_cast<const u8*>(payload),
                                static_cast<const u8*>(scales), segs, nsegs,
                                rows, S, after, stream);
  });
}

void launch_mx8_quantize_blocks(const void* in, void* payload, void* scales,
                                int nblocks, int64_t rows, int64_t row_elems,
                                int dtype, hipStream_t stream) {
  if (nblocks <= 0 || rows <= 0 || row_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_quantize_blocks_t<k>(in, static_cast<u8*>(payload),
                                static_cast<u8*>(scales), nblocks, rows,
                                row_elems, stream);
  });
}

void launch_mx8_dequantize_blocks(const void* payload, const void* scales,
                                  void* out, int nblocks, int64_t rows,
                                  int64_t row_elems, int dtype,
                                  hipStream_t stream) {
  if (nblocks <= 0 || rows <= 0 || row_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_dequantize_blocks_t<k>(static_cast<const u8*>(payload),
                                  static_cast<const u8*>(scales), out, nblocks,
                                  rows, row_elems, stream);
  });
}

void launch_mx8_reduce_to(const void* payload_in, const void* scales_in,
                          void* out, int64_t n_elems, int nranks, int dtype,
                          hipStream_t stream) {
  if (n_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_reduce_to_t<k>(static_cast<const u8*>(payload_in),
                          static_cast<const u8*>(scales_in), out, n_elems,
                          nranks, stream);
  });
}

void launch_mx8_quantize(const void* in, void* payload, void* scales,
                         int64_t n_elems, int dtype, hipStream_t stream) {
  if (n_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_quantize_t<k>(in, payload, scales, n_elems, stream);
  });
}

void launch_mx8_quantize_sr(const void* in, void* payload, void* scales,
                            int64_t n_elems, int dtype, uint32_t k0,
                            uint32_t k1, int64_t n0, hipStream_t stream) {
  if (n_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_quantize_t<k>(in, payload, scales, n_elems, stream,
                         sr_key(k0, k1, n0));
  });
}

void launch_mx8_reduce(const void* payload_in, const void* scales_in,
                       void* payload_out, void* scales_out, int64_t n_groups,
                       int nranks, hipStream_t stream) {
  if (n_groups <= 0) return;
  launch_reduce_t(payload_in, scales_in, payload_out, scales_out, n_groups,
                  nranks, stream);
}

void launch_mx8_reduce_sr(const void* payload_in, const void* scales_in,
                          void* payload_out, void* scales_out,
                          int64_t n_groups, int nranks, uint32_t k0,
                          uint32_t k1, int64_t n0, hipStream_t stream) {
  if (n_groups <= 0) return;
  launch_reduce_t(payload_in, scales_in, payload_out, scales_out, n_groups,
                  nranks, stream, sr_key(k0, k1, n0));
}

void launch_mx8_dequantize(const void* payload, const void* scales, void* out,
                           int64_t n_elems, int dtype, hipStream_t stream) {
  if (n_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_dequantize_t<k>(payload, scales, out, n_elems, stream);
  });
}

// ===========================================================================
// mxfp4: the second wire of AllgatherCompressed
// ===========================================================================
//
// The family's rule with OCP e2m1 in place of e4m3 (normative in csrc/ops.cpp,
// mx4_quantize_groups / mx4_dequantize_groups): a group of 32 elements is 16
// payload bytes (element 2j in the low nibble of byte j, 2j+1 in the high
// one) plus the E8M0 scale byte, 17/32 byte per element. A nibble is
// sign<<3 | code, code 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6. With amax = m*2^k,
// m in [0.5,1): E = k-3 if m <= 0.75 else k-2, clamped to [-127,127], so
// amax*2^-E <= 6 and the conversion cannot saturate.
//
// The conversions are the gfx950 packed converts (v_cvt_scalef32_pk_fp4_f32,
// v_cvt_scalef32_pk_f32_fp4) at scale 1: the shared exponent is applied by
// ldexpf, exact and defined at E = -127, where the instruction's own scale
// operand would be an fp32 subnormal. Elements met one by one (heads, tails,
// nibble-shifted chunks of the general twin) are decoded in integer
// arithmetic, mx4_nibble_to_f32.
//
// Three kernels and the twins of the first and last, all 256 threads,
// grid-stride, no LDS:
//   quantize  : 8 elements per lane, 4 lanes per group, for every dtype (one
//               16-byte load for the 16-bit dtypes, two for fp32); the amax
//               crosses the group by two xor-shuffles; a lane stores one
//               packed payload dword, a wave 256 contiguous bytes; the
//               wave's 16 scale bytes leave through store_scales<4>. The
//               loop covers ALL G*4 lane slots: elements past N are zeros
//               and store the zero padding, so there is no scalar tail.
//   dequantize_blocks : the allgather tail, mx8_dequantize_blocks_kernel's
//               geometry (grid.y = block, BlockMap): one 16-byte store per
//               lane, fed by a payload dword (16-bit dtypes, 8 elements) or
//               two payload bytes (fp32, 4 elements).
//   its general twin : mx8_dequantize_blocks_kernel_shifted's split of every
//               (block, row) segment at the 16-byte boundaries of the
//               destination; a chunk may start at an odd element of the
//               block, i.e. in the middle of a payload byte (see there).

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ inline int mx4_scale_byte(unsigned amax_bits, int* E) {
  if (amax_bits >= kInfBits) {
    *E = 0;
    return 255;
  }
  const int e = (int)(amax_bits >> 23);
  const unsigned f = amax_bits & 0x7fffffu;
  int ex;
  if (amax_bits == 0) {
    ex = 0;
  } else if (e == 0) {
    ex = -127;  // fp32 subnormal amax: k <= -126, k-2 clamps
  } else {
    // amax = 1.f * 2^(e-127) = m * 2^(e-126); m <= 0.75 <=> f <= 0x400000
    ex = (e - 126) - (f <= 0x400000u ? 3 : 2);
    if (ex < -127) ex = -127;
  }
  *E = ex;
  return ex + 127;
}

// byte SEL of `old` <- the e2m1 nibbles of a (low) and b (high), RNE
template <int SEL>
__device__ inline unsigned mx4_cvt_pk(unsigned old, float a, float b) {
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, a, b, 1.0f, SEL);
}

// a lane's 8 elements under the shared exponent E -> its payload dword
__device__ inline unsigned mx4_quant8(const float (&x)[8], int E) {
  unsigned w = 0;
  w = mx4_cvt_pk<0>(w, ldexpf(x[0], -E), ldexpf(x[1], -E));
  w = mx4_cvt_pk<1>(w, ldexpf(x[2], -E), ldexpf(x[3], -E));
  w = mx4_cvt_pk<2>(w, ldexpf(x[4], -E), ldexpf(x[5], -E));
  w = mx4_cvt_pk<3>(w, ldexpf(x[6], -E), ldexpf(x[7], -E));
  return w;
}

// the low N (4 or 8) nibbles of w as their grid values (scale 1)
template <int N>
__device__ inline void mx4_decode(unsigned w, float (&v)[N]) {
  const v2f a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0);
  const v2f b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
  v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1];
  if constexpr (N == 8) {
    const v2f c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2);
    const v2f d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3);
    v[4] = c[0], v[5] = c[1], v[6] = d[0], v[7] = d[1];
  }
}

__device__ inline float mx4_scaled(float v, int sb) {
  return sb == 255 ? __uint_as_float(kQNaNBits) : ldexpf(v, sb - 127);
}

// One nibble in integer arithmetic: code 1 is 0.5, code c >= 2 is
// (1 + (c&1)/2) * 2^((c>>1) - 1); bit 3 is the sign, kept on zero.
__device__ inline float mx4_nibble_to_f32(unsigned nib) {
  const unsigned c = nib & 7u;
  const unsigned mag = c == 0   ? 0u
                       : c == 1 ? 0x3f000000u
                                : ((126u + (c >> 1)) << 23) | ((c & 1u) << 22);
  return __uint_as_float(mag | ((nib & 8u) << 28));
}

__device__ inline float mx4_dequant(unsigned nib, int sb) {
  return mx4_scaled(mx4_nibble_to_f32(nib), sb);
}

// ---- quantize -----------------------------------------------------------

// Lane slot i's elements [8i, 8i+8) of the N-element stream; zeros past N.
// Only the one slot that straddles N reads element by element.
template <int K>
__device__ inline void mx4_load8(const void* __restrict__ in, long long i,
                                 long long N, float (&x)[8]) {
  using T = typename Elem<K>::type;
  const long long e0 = i * 8;
  if (e0 + 8 <= N) {
    if constexpr (K == kF32) {
      const v4u a =
          __builtin_nontemporal_load(reinterpret_cast<const v4u*>(in) + 2 * i);
      const v4u b = __builtin_nontemporal_load(
          reinterpret_cast<const v4u*>(in) + 2 * i + 1);
      for (int d = 0; d < 4; ++d) {
        x[d] = __uint_as_float(a[d]);
        x[4 + d] = __uint_as_float(b[d]);
      }
    } else {
      unpack16<K, 8>(
          __builtin_nontemporal_load(reinterpret_cast<const v4u*>(in) + i), x);
    }
  } else {
    for (int k = 0; k < 8; ++k) {
      x[k] = e0 + k < N
                 ? elem_to_f32<K>(reinterpret_cast<const T*>(in)[e0 + k])
                 : 0.0f;
    }
  }
}

template <int K>
__global__ __launch_bounds__(256) void mx4_quantize_kernel(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long G, long long N) {
  const long long slots = G * 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  // wave-uniform trip count: the shuffles below and in store_scales need
  // every lane present; slots is a multiple of 4, so a group is never cut
  for (long long i0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
       i0 < slots; i0 += stride) {
    const long long i = i0 + lane;
    const bool act = i < slots;
    float x[8];
    if (act) {
      mx4_load8<K>(in, i, N, x);
    } else {
      for (int k = 0; k < 8; ++k) x[k] = 0.0f;
    }
    unsigned a = amax_bits_of(x);
    for (int m = 1; m < 4; m <<= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)a, m);
      a = o > a ? o : a;
    }
    int E;
    const int sb = mx4_scale_byte(a, &E);
    if (act) {
      __builtin_nontemporal_store(sb == 255 ? 0u : mx4_quant8(x, E),
                                  reinterpret_cast<unsigned*>(pay) + i);
    }
    store_scales<4>(sc, i0 / 4, G, sb, lane);
  }
}

// One thread per group, any alignment of the input and payload bases.
template <int K>
__global__ __launch_bounds__(256) void mx4_quantize_kernel_scalar(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long G, long long N) {
  using T = typename Elem<K>::type;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    const T* p = reinterpret_cast<const T*>(in) + g * 32;
    const long long left = N - g * 32;
    float x[32];
    for (int k = 0; k < 32; ++k) {
      x[k] = k < left ? elem_to_f32<K>(p[k]) : 0.0f;
    }
    int E;
    const int sb = mx4_scale_byte(amax_bits_of(x), &E);
    for (int j = 0; j < 16; ++j) {
      pay[g * 16 + j] =
          sb == 255 ? (u8)0
                    : (u8)mx4_cvt_pk<0>(0u, ldexpf(x[2 * j], -E),
                                        ldexpf(x[2 * j + 1], -E));
    }
    sc[g] = (u8)sb;
  }
}

// ---- dequantize_blocks (the allgather tail) ------------------------------
//
// pay [nblocks][Gb*16], sc [nblocks][Gb], Gb = ceil(L/32), L = rows*row_elems
// -> out [rows][nblocks][row_elems]. Vector body: one 16-byte store per lane,
// EPL = 8 elements (a payload dword) for the 16-bit dtypes and 4 (a 2-byte
// payload load) for fp32, where two stores per lane measured 19 % slower
// (doc/kernels.md section 5). It requires row_elems % EPL == 0, a 16-byte
// aligned output and an EPL/2-byte aligned payload. Chunk i of the block
// (scale byte i*EPL/32: the group runs over the block-flat index and may
// straddle rows) lies inside one row; BlockMap gives its place in 16-byte
// units. L % EPL == 0, so the partial last group is whole chunks and nothing
// past element L is written.
template <int K> constexpr int kMx4EPL = K == kF32 ? 4 : 8;

template <int K, typename I>
__global__ __launch_bounds__(256) void mx4_dequantize_blocks_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long Gb, I chunks, I cpr,
    long long nblocks) {
  using W = std::conditional_t<K == kF32, unsigned short, unsigned>;
  constexpr int EPL = kMx4EPL<K>;
  const long long r = blockIdx.y;
  const W* __restrict__ bp = reinterpret_cast<const W*>(pay + r * Gb * 16);
  const u8* __restrict__ bs = sc + r * Gb;
  const BlockMap<I> map{r, nblocks, cpr};
  const I stride = (I)gridDim.x * blockDim.x;
  for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < chunks;
       i += stride) {
    const int sb = bs[i / (32 / EPL)];
    float x[EPL];
    mx4_decode<EPL>(__builtin_nontemporal_load(bp + i), x);
    for (int k = 0; k < EPL; ++k) x[k] = mx4_scaled(x[k], sb);
    __builtin_nontemporal_store(pack16<K, EPL>(x),
                                reinterpret_cast<v4u*>(out) + map(i));
  }
}

// General twin: any row length, any alignment of the payload and output
// bases. The split and the lane slots are those of
// mx8_dequantize_blocks_kernel_shifted: per (block, row) segment up to EPL-1
// head elements, whole aligned 16-byte chunks of EPL elements, up to EPL-1
// tail elements; row_elems/EPL + 2 slots per row. New with nibbles: a chunk's
// first element src may be odd within the block, its EPL nibbles then start
// in the high half of payload byte src/2 and end in the low half of byte
// src/2 + EPL/2. The window is the EPL/2 bytes from src/2 on (one unaligned
// load) plus, for an odd src only, the byte after them, shifted right by the
// nibble phase. The chunk may belong to two groups, hence two scale bytes.
template <int K, typename I>
__global__ __launch_bounds__(256) void mx4_dequantize_blocks_kernel_shifted(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long Gb, long long row_elems, I slots,
    I total, long long nblocks) {
  using T = typename Elem<K>::type;
  using W = std::conditional_t<K == kF32, unsigned short, unsigned>;
  constexpr int EPL = kMx4EPL<K>;
  const long long r = blockIdx.y;
  const u8* __restrict__ bp = pay + r * Gb * 16;
  const u8* __restrict__ bs = sc + r * Gb;
  auto nibble = [&](long long e) {
    return (unsigned)(bp[e >> 1] >> (4 * (int)(e & 1))) & 15u;
  };
  const I stride = (I)gridDim.x * blockDim.x;
  for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const I b = i / slots;
    const long long k = (long long)(i - b * slots);
    T* d = reinterpret_cast<T*>(out) +
           ((long long)b * nblocks + r) * row_elems;  // the segment
    const long long s0 = (long long)b * row_elems;    // its block-flat start
    long long head =
        (long long)(((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15) /
                    sizeof(T));
    if (head > row_elems) head = row_elems;
    const long long nchunks = (row_elems - head) / EPL;
    if (k < nchunks) {
      const long long e = head + k * EPL;
      const long long src = s0 + e;
      const int ph = (int)(src & 1);
      const u8* p = bp + (src >> 1);
      W lo;
      __builtin_memcpy(&lo, p, EPL / 2);
      unsigned long long win = lo;
      if (ph) win |= (unsigned long long)p[EPL / 2] << (4 * EPL);
      win >>= 4 * ph;
      const long long g0 = src >> 5;
      const int sb0 = bs[g0];
      const int sb1 = bs[(src + EPL - 1) >> 5];
      float x[EPL];
      mx4_decode<EPL>((unsigned)win, x);
      for (int t = 0; t < EPL; ++t) {
        x[t] = mx4_scaled(x[t], ((src + t) >> 5) == g0 ? sb0 : sb1);
      }
      __builtin_nontemporal_store(pack16<K, EPL>(x),
                                  reinterpret_cast<v4u*>(d + e));
    } else if (k >= (long long)slots - 2) {
      // head [0, head) or tail [head + nchunks*EPL, row_elems): fewer than
      // EPL elements each, stored one by one
      const bool is_head = k == (long long)slots - 2;
      const long long lo = is_head ? 0 : head + nchunks * EPL;
      const long long hi = is_head ? head : row_elems;
      for (long long e = lo; e < hi; ++e) {
        d[e] = f32_to_elem<K>(mx4_dequant(nibble(s0 + e), bs[(s0 + e) >> 5]));
      }
    }
  }
}

template <int K>
void launch_mx4_quantize_t(const void* in, u8* pay, u8* sc, int64_t N,
                           hipStream_t stream) {
  const long long G = (N + 31) / 32;
  if (aligned(in, 16) && aligned(pay, 4)) {
    hipLaunchKernelGGL((mx4_quantize_kernel<K>), dim3(grid_for(G * 4)),
                       dim3(256), 0, stream, in, pay, sc, G, (long long)N);
  } else {
    hipLaunchKernelGGL((mx4_quantize_kernel_scalar<K>), dim3(grid_for(G)),
                       dim3(256), 0, stream, in, pay, sc, G, (long long)N);
  }
}

template <int K>
void launch_mx4_dequantize_blocks_t(const u8* pay, const u8* sc, void* out,
                                    int nblocks, int64_t rows,
                                    int64_t row_elems, hipStream_t stream) {
  const long long L = rows * row_elems;
  const long long Gb = (L + 31) / 32;
  // Every block's payload base is pay + r*Gb*16, so an aligned pay keeps all
  // of them aligned; row_elems % EPL == 0 with an aligned out keeps every
  // chunk's destination aligned.
  constexpr int EPL = kMx4EPL<K>;
  if (aligned(out, 16) && aligned(pay, EPL / 2) && row_elems % EPL == 0) {
    const long long chunks = L / EPL;
    const long long cpr = row_elems / EPL;
    by_width(chunks, [&](auto i) {
      using I = decltype(i);
      hipLaunchKernelGGL((mx4_dequantize_blocks_kernel<K, I>),
                         grid2d(chunks, nblocks), dim3(256), 0, stream, pay,
                         sc, out, Gb, (I)chunks, (I)cpr, (long long)nblocks);
    });
  } else {
    const long long slots = row_elems / EPL + 2;
    const long long total = rows * slots;
    by_width(total, [&](auto i) {
      using I = decltype(i);
      hipLaunchKernelGGL((mx4_dequantize_blocks_kernel_shifted<K, I>),
                         grid2d(total, nblocks), dim3(256), 0, stream, pay, sc,
                         out, Gb, (long long)row_elems, (I)slots, (I)total,
                         (long long)nblocks);
    });
  }
}

} // namespace

void launch_mx4_quantize(const void* in, void* payload, void* scales,
                         int64_t n_elems, int dtype, hipStream_t stream) {
  if (n_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_mx4_quantize_t<k>(in, static_cast<u8*>(payload),
                             static_cast<u8*>(scales), n_elems, stream);
  });
}

void launch_mx4_dequantize_blocks(const void* payload, const void* scales,
                                  void* out, int nblocks, int64_t rows,
                                  int64_t row_elems, int dtype,
                                  hipStream_t stream) {
  if (nblocks <= 0 || rows <= 0 || row_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_mx4_dequantize_blocks_t<k>(static_cast<const u8*>(payload),
                                      static_cast<const u8*>(scales), out,
                                      nblocks, rows, row_elems, stream);
  });
}

// ===========================================================================
// mxfp6 (e2m3): the third wire of AllgatherCompressed
// ===========================================================================
//
// The family's rule with OCP e2m3 in place of e4m3 (normative in csrc/ops.cpp,
// mx6_quantize_groups / mx6_dequantize_groups): a group of 32 elements is 24
// payload bytes plus the E8M0 scale byte, 25/32 byte per element. A code is
// sign<<5 | e<<3 | m with bias 1: m/8 for e = 0, (1 + m/8) * 2^(e-1) above,
// maximum 7.5. The 32 codes are a little-endian bit stream: code i sits in
// bits 6i..6i+5 of the group's 192. With amax = m*2^k, m in [0.5,1): E = k-3
// if m <= 0.9375 else k-2, clamped to [-127,127], so amax*2^-E <= 7.5 and the
// conversion cannot saturate.
//
// The gfx950 packed fp6 converts work on 32 values per lane and their
// element order, ties and signed zeros are not established, so they are not
// used. The conversions go through what the mxfp8 kernels already rely on:
//   encode : e2m3 is e4m3 with its exponent range cut to the lowest four
//            fields: both have three mantissa bits and subnormals below their
//            first normal binade, 2^0 here and 2^-6 there. So the e4m3 byte
//            of y * 2^-6 (the hardware RNE convert of quant4, under the
//            exponent E + 6) has the e2m3 magnitude in its low five bits and
//            the sign in bit 7; |y| <= 7.5 keeps its exponent field <= 3.
//            Four bytes become four codes in three mask operations, and 24
//            contiguous bits in seven more.
//   decode : the 5-bit magnitude shifted to fp32 bits 20..24 is the value
//            times 2^-126, fp32 subnormals included (e = 0 is a subnormal
//            there too); one ldexpf applies 2^126 and the shared exponent.
//
// Three kernels and the twins of the first and last, all 256 threads,
// grid-stride, no LDS:
//   quantize  : 16 elements per lane, 2 lanes per group, for every dtype (two
//               16-byte loads for the 16-bit dtypes, four for fp32); the amax
//               crosses the pair by one xor-shuffle; a lane's 16 codes are 96
//               bits, three dwords stored at once, a wave 768 contiguous
//               bytes; the wave's 32 scale bytes leave through
//               store_scales<2>. The loop covers ALL G*2 lane slots: elements
//               past N are zeros and store the zero padding.
//   dequantize_blocks : the allgather tail, mx4_dequantize_blocks_kernel's
//               geometry and its one 16-byte store per lane, fed by the 6
//               (16-bit dtypes, 8 elements) or 3 (fp32, 4 elements) payload
//               bytes of the chunk, read as the tail of one unaligned load.
//   its general twin : the destination-aligned split of the other two wires;
//               a chunk's codes start at any of four bit phases (see there).

namespace {

__device__ inline int mx6_scale_byte(unsigned amax_bits, int* E) {
  if (amax_bits >= kInfBits) {
    *E = 0;
    return 255;
  }
  const int e = (int)(amax_bits >> 23);
  const unsigned f = amax_bits & 0x7fffffu;
  int ex;
  if (amax_bits == 0) {
    ex = 0;
  } else if (e == 0) {
    ex = -127;  // fp32 subnormal amax: k <= -126, k-2 clamps
  } else {
    // amax = 1.f * 2^(e-127) = m * 2^(e-126); m <= 0.9375 <=> f <= 0x700000
    ex = (e - 126) - (f <= 0x700000u ? 3 : 2);
    if (ex < -127) ex = -127;
  }
  *E = ex;
  return ex + 127;
}

// four values under the shared exponent E -> their four codes, 24 bits
__device__ inline unsigned mx6_quant4(float a, float b, float c, float d,
                                      int E) {
  const unsigned b8 = quant4(a, b, c, d, E + 6);  // e4m3 bytes of y * 2^-6
  const unsigned c8 = (b8 & 0x1f1f1f1fu) | ((b8 >> 2) & 0x20202020u);
  return (c8 & 0x3fu) | ((c8 >> 2) & 0xfc0u) | ((c8 >> 4) & 0x3f000u) |
         ((c8 >> 6) & 0xfc0000u);
}

// a lane's 16 elements under the shared exponent E -> its 96 payload bits
__device__ inline void mx6_quant16(const float (&x)[16], int E,
                                   unsigned (&w)[3]) {
  unsigned t[4];
  for (int j = 0; j < 4; ++j) {
    t[j] = mx6_quant4(x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3], E);
  }
  w[0] = t[0] | t[1] << 24;
  w[1] = t[1] >> 8 | t[2] << 16;
  w[2] = t[2] >> 16 | t[3] << 8;
}

// one code under scale byte sb (the bits above the code are ignored)
__device__ inline float mx6_dequant(unsigned code, int sb) {
  const float t =
      __uint_as_float(((code & 31u) << 20) | ((code & 32u) << 26));
  return sb == 255 ? __uint_as_float(kQNaNBits) : ldexpf(t, sb - 1);
}

// ---- quantize -----------------------------------------------------------

template <int K>
__global__ __launch_bounds__(256) void mx6_quantize_kernel(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long G, long long N) {
  const long long slots = G * 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  // wave-uniform trip count: the shuffle below and those in store_scales need
  // every lane present; slots is even, so a group is never cut
  for (long long i0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
       i0 < slots; i0 += stride) {
    const long long i = i0 + lane;
    const bool act = i < slots;
    float x[16];
    if (act) {
      // slot i is the mx4 layout's slots 2i and 2i+1 (zeros past N)
      mx4_load8<K>(in, 2 * i, N, *reinterpret_cast<float(*)[8]>(&x[0]));
      mx4_load8<K>(in, 2 * i + 1, N, *reinterpret_cast<float(*)[8]>(&x[8]));
    } else {
      for (int k = 0; k < 16; ++k) x[k] = 0.0f;
    }
    unsigned a = amax_bits_of(x);
    const unsigned o = (unsigned)__shfl_xor((int)a, 1);
    a = o > a ? o : a;
    int E;
    const int sb = mx6_scale_byte(a, &E);
    if (act) {
      unsigned w[3];
      mx6_quant16(x, E, w);
      unsigned* p = reinterpret_cast<unsigned*>(pay) + 3 * i;
      for (int d = 0; d < 3; ++d) {
        __builtin_nontemporal_store(sb == 255 ? 0u : w[d], p + d);
      }
    }
    store_scales<2>(sc, i0 / 2, G, sb, lane);
  }
}

// One thread per group, any alignment of the input and payload bases.
template <int K>
__global__ __launch_bounds__(256) void mx6_quantize_kernel_scalar(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long G, long long N) {
  using T = typename Elem<K>::type;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    const T* p = reinterpret_cast<const T*>(in) + g * 32;
    const long long left = N - g * 32;
    float x[32];
    for (int k = 0; k < 32; ++k) {
      x[k] = k < left ? elem_to_f32<K>(p[k]) : 0.0f;
    }
    int E;
    const int sb = mx6_scale_byte(amax_bits_of(x), &E);
    for (int j = 0; j < 8; ++j) {  // four codes -> three bytes
      const unsigned t =
          sb == 255 ? 0u
                    : mx6_quant4(x[4 * j], x[4 * j + 1], x[4 * j + 2],
                                 x[4 * j + 3], E);
      for (int k = 0; k < 3; ++k) pay[g * 24 + 3 * j + k] = (u8)(t >> (8 * k));
    }
    sc[g] = (u8)sb;
  }
}

// ---- dequantize_blocks (the allgather tail) ------------------------------
//
// pay [nblocks][Gb*24], sc [nblocks][Gb], Gb = ceil(L/32), L = rows*row_elems
// -> out [rows][nblocks][row_elems]. Vector body: one 16-byte store per lane,
// EPL = 8 elements for the 16-bit dtypes and 4 for fp32, as on the other two
// wires: a lane slot of 16 elements (one 12-byte load, two or four stores at
// a stride of 32 or 64 bytes) measured 1.2 (bf16) and 3.5 to 4.1 (fp32) times
// the mxfp8 sibling's time (doc/kernels.md section 5). Chunk i of the block
// is payload bytes [WB*i, WB*i + WB), WB = 6 or 3, which is no power of two:
// the lane reads the 8 or 4 bytes that END with the chunk's last byte (one
// unaligned load, shifted right by the 2 or 1 bytes in front; chunk 0 starts
// at the block's first byte instead), so nothing past the payload is read.
// It requires row_elems % EPL == 0 and a 16-byte aligned output; scale byte
// i*EPL/32 (the group runs over the block-flat index and may straddle rows).
// L % EPL == 0, so the partial last group is whole chunks and nothing past
// element L is written.
template <int K, typename I>
__global__ __launch_bounds__(256) void mx6_dequantize_blocks_kernel(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long Gb, I chunks, I cpr,
    long long nblocks) {
  using W = std::conditional_t<K == kF32, unsigned, unsigned long long>;
  constexpr int EPL = kMx4EPL<K>;
  constexpr int WB = 6 * EPL / 8;            // payload bytes per chunk
  constexpr int BACK = (int)sizeof(W) - WB;  // bytes in front of them
  const long long r = blockIdx.y;
  const u8* __restrict__ bp = pay + r * Gb * 24;
  const u8* __restrict__ bs = sc + r * Gb;
  const BlockMap<I> map{r, nblocks, cpr};
  const I stride = (I)gridDim.x * blockDim.x;
  for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < chunks;
       i += stride) {
    const int sb = bs[i / (32 / EPL)];
    const int back = i ? BACK : 0;
    W win;
    __builtin_memcpy(&win, bp + (long long)i * WB - back, sizeof(W));
    win >>= 8 * back;
    float x[EPL];
    for (int k = 0; k < EPL; ++k) {
      x[k] = mx6_dequant((unsigned)(win >> (6 * k)), sb);
    }
    __builtin_nontemporal_store(pack16<K, EPL>(x),
                                reinterpret_cast<v4u*>(out) + map(i));
  }
}

// General twin: any row length, any alignment of the payload and output
// bases. The split and the lane slots are those of
// mx4_dequantize_blocks_kernel_shifted: per (block, row) segment up to EPL-1
// head elements, whole aligned 16-byte chunks of EPL elements (8 for the
// 16-bit dtypes, 4 for fp32), up to EPL-1 tail elements; row_elems/EPL + 2
// slots per row. A chunk's first element src may be any element of the block,
// so its codes start at bit 6*src: byte 6*src/8, bit phase 6*src mod 8, one
// of 0, 6, 4, 2. The window is the ceil((phase + 6*EPL)/8) bytes from there
// on (6 or 7 for EPL = 8, 3 or 4 for EPL = 4), read in unaligned pieces that
// end with the chunk's last code, never past the payload, and shifted right
// by the phase. The chunk may belong to two groups, hence two scale bytes.
template <int K, typename I>
__global__ __launch_bounds__(256) void mx6_dequantize_blocks_kernel_shifted(
    const u8* __restrict__ pay, const u8* __restrict__ sc,
    void* __restrict__ out, long long Gb, long long row_elems, I slots,
    I total, long long nblocks) {
  using T = typename Elem<K>::type;
  using W = std::conditional_t<K == kF32, unsigned short, unsigned>;
  constexpr int EPL = K == kF32 ? 4 : 8;
  constexpr int WB = (int)sizeof(W);  // 2 or 4: the window's first piece
  const long long r = blockIdx.y;
  const u8* __restrict__ bp = pay + r * Gb * 24;
  const u8* __restrict__ bs = sc + r * Gb;
  auto code_at = [&](long long e) {
    const long long bit = 6 * e;
    const int ph = (int)(bit & 7);
    unsigned v = bp[bit >> 3] >> ph;
    if (ph > 2) v |= (unsigned)bp[(bit >> 3) + 1] << (8 - ph);
    return v;
  };
  const I stride = (I)gridDim.x * blockDim.x;
  for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const I b = i / slots;
    const long long k = (long long)(i - b * slots);
    T* d = reinterpret_cast<T*>(out) +
           ((long long)b * nblocks + r) * row_elems;  // the segment
    const long long s0 = (long long)b * row_elems;    // its block-flat start
    long long head =
        (long long)(((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15) /
                    sizeof(T));
    if (head > row_elems) head = row_elems;
    const long long nchunks = (row_elems - head) / EPL;
    if (k < nchunks) {
      const long long e = head + k * EPL;
      const long long src = s0 + e;
      const int ph = (int)((6 * src) & 7);
      const u8* p = bp + ((6 * src) >> 3);
      // bytes [0, WB), [WB, WB + WB/2) and, off phase 0, one more
      W a;
      __builtin_memcpy(&a, p, WB);
      unsigned long long win = a;
      if constexpr (EPL == 8) {
        unsigned short m;
        __builtin_memcpy(&m, p + 4, 2);
        win |= (unsigned long long)m << 32;
      } else {
        win |= (unsigned long long)p[2] << 16;
      }
      if (ph) win |= (unsigned long long)p[WB + WB / 2] << (12 * WB);
      win >>= ph;
      const long long g0 = src >> 5;
      const int sb0 = bs[g0];
      const int sb1 = bs[(src + EPL - 1) >> 5];
      float x[EPL];
      for (int t = 0; t < EPL; ++t) {
        x[t] = mx6_dequant((unsigned)(win >> (6 * t)),
                           ((src + t) >> 5) == g0 ? sb0 : sb1);
      }
      __builtin_nontemporal_store(pack16<K, EPL>(x),
                                  reinterpret_cast<v4u*>(d + e));
    } else if (k >= (long long)slots - 2) {
      // head [0, head) or tail [head + nchunks*EPL, row_elems): fewer than
      // EPL elements each, stored one by one
      const bool is_head = k == (long long)slots - 2;
      const long long lo = is_head ? 0 : head + nchunks * EPL;
      const long long hi = is_head ? head : row_elems;
      for (long long e = lo; e < hi; ++e) {
        d[e] = f32_to_elem<K>(mx6_dequant(code_at(s0 + e), bs[(s0 + e) >> 5]));
      }
    }
  }
}

template <int K>
void launch_mx6_quantize_t(const void* in, u8* pay, u8* sc, int64_t N,
                           hipStream_t stream) {
  const long long G = (N + 31) / 32;
  if (aligned(in, 16) && aligned(pay, 4)) {
    hipLaunchKernelGGL((mx6_quantize_kernel<K>), dim3(grid_for(G * 2)),
                       dim3(256), 0, stream, in, pay, sc, G, (long long)N);
  } else {
    hipLaunchKernelGGL((mx6_quantize_kernel_scalar<K>), dim3(grid_for(G)),
                       dim3(256), 0, stream, in, pay, sc, G, (long long)N);
  }
}

template <int K>
void launch_mx6_dequantize_blocks_t(const u8* pay, const u8* sc, void* out,
                                    int nblocks, int64_t rows,
                                    int64_t row_elems, hipStream_t stream) {
  const long long L = rows * row_elems;
  const long long Gb = (L + 31) / 32;
  // row_elems % EPL == 0 with an aligned out keeps every chunk's destination
  // aligned; the payload is read by unaligned loads in either kernel.
  constexpr int EPL = kMx4EPL<K>;
  if (aligned(out, 16) && row_elems % EPL == 0) {
    const long long chunks = L / EPL;
    const long long cpr = row_elems / EPL;
    by_width(chunks, [&](auto i) {
      using I = decltype(i);
      hipLaunchKernelGGL((mx6_dequantize_blocks_kernel<K, I>),
                         grid2d(chunks, nblocks), dim3(256), 0, stream, pay,
                         sc, out, Gb, (I)chunks, (I)cpr, (long long)nblocks);
    });
  } else {
    const long long slots = row_elems / EPL + 2;
    const long long total = rows * slots;
    by_width(total, [&](auto i) {
      using I = decltype(i);
      hipLaunchKernelGGL((mx6_dequantize_blocks_kernel_shifted<K, I>),
                         grid2d(total, nblocks), dim3(256), 0, stream, pay, sc,
                         out, Gb, (long long)row_elems, (I)slots, (I)total,
                         (long long)nblocks);
    });
  }
}

} // namespace

void launch_mx6_quantize(const void* in, void* payload, void* scales,
                         int64_t n_elems, int dtype, hipStream_t stream) {
  if (n_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_mx6_quantize_t<k>(in, static_cast<u8*>(payload),
                             static_cast<u8*>(scales), n_elems, stream);
  });
}

void launch_mx6_dequantize_blocks(const void* payload, const void* scales,
                                  void* out, int nblocks, int64_t rows,
                                  int64_t row_elems, int dtype,
                                  hipStream_t stream) {
  if (nblocks <= 0 || rows <= 0 || row_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_mx6_dequantize_blocks_t<k>(static_cast<const u8*>(payload),
                                      static_cast<const u8*>(scales), out,
                                      nblocks, rows, row_elems, stream);
  });
}

} // namespace m4a
