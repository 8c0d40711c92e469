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
// Eight streaming kernels, all 256-thread workgroups, grid-stride, 16-byte
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

// four values -> one packed payload dword
__device__ inline unsigned quant4(float a, float b, float c, float d, int E) {
  return (unsigned)f32_to_e4m3(ldexpf(a, -E)) |
         ((unsigned)f32_to_e4m3(ldexpf(b, -E)) << 8) |
         ((unsigned)f32_to_e4m3(ldexpf(c, -E)) << 16) |
         ((unsigned)f32_to_e4m3(ldexpf(d, -E)) << 24);
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

__device__ inline void encode_group_scalar(const float (&x)[32],
                                           u8* __restrict__ pay,
                                           u8* __restrict__ sc) {
  int E;
  const int sb = mx8_scale_byte(amax_bits_of(x), &E);
  for (int k = 0; k < 32; ++k) {
    pay[k] = sb == 255 ? (u8)0 : f32_to_e4m3(ldexpf(x[k], -E));
  }
  *sc = (u8)sb;
}

template <int K>
__device__ inline void quant_group_scalar(
    const typename Elem<K>::type* __restrict__ in, int cnt,
    u8* __restrict__ pay, u8* __restrict__ sc) {
  float x[32];
  for (int k = 0; k < 32; ++k) {
    x[k] = k < cnt ? elem_to_f32<K>(in[k]) : 0.0f;
  }
  encode_group_scalar(x, pay, sc);
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
template <int K>
__device__ inline int quant_lane(const float (&x)[kEPL<K>], bool store,
                                 u8* __restrict__ pay, long long i) {
  constexpr int EPL = kEPL<K>;
  unsigned a = amax_bits_of(x);
  for (int m = 1; m < kLPG<K>; m <<= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)a, m);
    a = o > a ? o : a;
  }
  int E;
  const int sb = mx8_scale_byte(a, &E);
  if (store) {
    const unsigned lo = sb == 255 ? 0u : quant4(x[0], x[1], x[2], x[3], E);
    if constexpr (K == kF32) {
      __builtin_nontemporal_store(lo, reinterpret_cast<unsigned*>(pay) + i);
    } else {
      v2u o;
      o[0] = lo;
      o[1] = sb == 255
                 ? 0u
                 : quant4(x[EPL - 4], x[EPL - 3], x[EPL - 2], x[EPL - 1], E);
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

template <int K>
__global__ __launch_bounds__(256) void mx8_quantize_kernel(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long nfull, long long N) {
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
    const int sb = quant_lane<K>(x, act, pay, i);
    store_scales<LPG>(sc, i0 / LPG, nfull, sb, lane);
  }
  // zero-padded partial last group
  const int tail = (int)(N - nfull * 32);
  if (tail > 0 && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    quant_group_scalar<K>(reinterpret_cast<const T*>(in) + nfull * 32, tail,
                          pay + nfull * 32, sc + nfull);
  }
}

template <int K>
__global__ __launch_bounds__(256) void mx8_quantize_kernel_scalar(
    const void* __restrict__ in, u8* __restrict__ pay, u8* __restrict__ sc,
    long long G, long long N) {
  using T = typename Elem<K>::type;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    const long long left = N - g * 32;
    quant_group_scalar<K>(reinterpret_cast<const T*>(in) + g * 32,
                          left < 32 ? (int)left : 32, pay + g * 32, sc + g);
  }
}

// ---- reduce -------------------------------------------------------------

__global__ __launch_bounds__(256) void mx8_reduce_kernel(
    const u8* __restrict__ pin, const u8* __restrict__ sin,
    u8* __restrict__ pout, u8* __restrict__ sout, long long n,
    long long nranks) {
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
      v4u w;
      for (int d = 0; d < 4; ++d) {
        w[d] = sb == 255 ? 0u
                         : quant4(acc[4 * d], acc[4 * d + 1], acc[4 * d + 2],
                                  acc[4 * d + 3], E);
      }
      __builtin_nontemporal_store(w, reinterpret_cast<v4u*>(pout) + i);
    }
    store_scales<2>(sout, i0 >> 1, n, sb, lane);
  }
}

__global__ __launch_bounds__(256) void mx8_reduce_kernel_scalar(
    const u8* __restrict__ pin, const u8* __restrict__ sin,
    u8* __restrict__ pout, u8* __restrict__ sout, long long n,
    long long nranks) {
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
    encode_group_scalar(acc, pout + g * 32, sout + g);
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
// to per-lane bytes.
template <int K, typename I, typename Map>
__device__ inline void quantize_stream(const void* __restrict__ in,
                                       u8* __restrict__ bp,
                                       u8* __restrict__ bs, long long G,
                                       I chunks, I slots, const Map& map,
                                       I first, I stride) {
  constexpr int LPG = kLPG<K>;
  const int lane = threadIdx.x & 63;
  // i0: the wave's first slot (workgroups are whole waves)
  for (I i0 = first & ~(I)63; i0 < slots; i0 += stride) {
    const I i = i0 + lane;
    long long src = -1;
    if (i < chunks) src = map(i);
    float x[kEPL<K>];
    load_chunk<K>(in, src, Map::kCanMiss ? src >= 0 : i < chunks, x);
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

template <int K, bool IDX>
__global__ __launch_bounds__(256) void mx8_quantize_segments_kernel_scalar(
    const void* __restrict__ in, const long long* __restrict__ idx,
    u8* __restrict__ pay, u8* __restrict__ sc, SegArgs segs, long long S,
    long long after, long long rows) {
  using T = typename Elem<K>::type;
  const Mx8SegDesc& d = segs.s[blockIdx.y];
  if (d.count == 0) return;
  SegCursor<IDX> cur(d, idx, S, after, rows);
  const long long G = (cur.L + 31) / 32;
  const T* __restrict__ src = reinterpret_cast<const T*>(in);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += stride) {
    cur.seek(g * 32);
    float x[32];
    for (int k = 0; k < 32; ++k) {
      x[k] = 0.0f;
      if (cur.in_stream()) {
        const long long o = cur.offset();
        if (o >= 0) x[k] = elem_to_f32<K>(src[o]);
        cur.advance();
      }
    }
    encode_group_scalar(x, pay + (d.goff + g) * 32, sc + d.goff + g);
  }
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

template <int K>
void launch_quantize_t(const void* in, void* pay, void* sc, int64_t N,
                       hipStream_t stream) {
  constexpr int LPG = kLPG<K>;
  const long long G = (N + 31) / 32;
  const long long nfull = N / 32;
  if (aligned(in, 16) && aligned(pay, 32 / LPG)) {
    hipLaunchKernelGGL((mx8_quantize_kernel<K>), dim3(grid_for(nfull * LPG)),
                       dim3(256), 0, stream, in, static_cast<u8*>(pay),
                       static_cast<u8*>(sc), nfull, (long long)N);
  } else {
    hipLaunchKernelGGL((mx8_quantize_kernel_scalar<K>), dim3(grid_for(G)),
                       dim3(256), 0, stream, in, static_cast<u8*>(pay),
                       static_cast<u8*>(sc), G, (long long)N);
  }
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
  for (int s0 = 0; s0 < nsegs; s0 += kMaxMx8SegsPerLaunch) {
    const int n = nsegs - s0 < kMaxMx8SegsPerLaunch ? nsegs - s0
                                                    : kMaxMx8SegsPerLaunch;
    const SegBatch b = seg_batch(segs + s0, n);
    if (b.max_count == 0) continue;
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
      auto twin = [&](auto indexed) {
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
      };
      if (idx == nullptr) {
        twin(std::false_type{});
      } else {
        twin(std::true_type{});
      }
    }
  }
}

} // namespace

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

void launch_mx8_reduce(const void* payload_in, const void* scales_in,
                       void* payload_out, void* scales_out, int64_t n_groups,
                       int nranks, hipStream_t stream) {
  if (n_groups <= 0) return;
  const u8* pin = static_cast<const u8*>(payload_in);
  const u8* sin = static_cast<const u8*>(scales_in);
  u8* pout = static_cast<u8*>(payload_out);
  u8* sout = static_cast<u8*>(scales_out);
  if (aligned(pin, 16) && aligned(pout, 16)) {
    hipLaunchKernelGGL(mx8_reduce_kernel, dim3(grid_for(n_groups * 2)),
                       dim3(256), 0, stream, pin, sin, pout, sout,
                       (long long)n_groups, (long long)nranks);
  } else {
    hipLaunchKernelGGL(mx8_reduce_kernel_scalar, dim3(grid_for(n_groups)),
                       dim3(256), 0, stream, pin, sin, pout, sout,
                       (long long)n_groups, (long long)nranks);
  }
}

void launch_mx8_dequantize(const void* payload, const void* scales, void* out,
                           int64_t n_elems, int dtype, hipStream_t stream) {
  if (n_elems <= 0) return;
  by_dtype(dtype, [&](auto k) {
    launch_dequantize_t<k>(payload, scales, out, n_elems, stream);
  });
}

} // namespace m4a
