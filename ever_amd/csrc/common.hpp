// Shared helpers for the gfx950 kernels of libever_hip.so.  CDNA4 only: wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include <type_traits>
#include "../../include/ever_hip.h"

namespace evk {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return EVK_E_LAUNCH;
  }
  return EVK_OK;
}

#define EVK_REQUIRE(cond, code, ...)     \
  do {                                   \
    if (!(cond)) {                       \
      ::evk::set_error(__VA_ARGS__);     \
      return (code);                     \
    }                                    \
  } while (0)

// "Once per DEVICE" for hipFuncSetAttribute: a function attribute belongs to the device's copy of the code object, so a
// process that drives several devices has to set it on each (one flag per process left the second device's kernels at the
// 64 KB default: launch failure with a 98-160 KB ring).
struct PerDeviceOnce {
  std::atomic<uint64_t> mask{0};
  bool first() {
    int d = 0;
    (void)hipGetDevice(&d);
    const uint64_t b = 1ull << (d & 63);
    return !(mask.fetch_or(b) & b);
  }
};

constexpr int kWave = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

// what every 16-byte load and store of a launch asks of its pointers
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// uint8 or int64 label maps: the label of pixel pix, and those of first_pix .. first_pix+3 (first_pix a multiple of 4, the map
// on the 16-byte grid) as one 4-byte store or two 16-byte stores
__device__ __forceinline__ void store_label(void* __restrict__ out, bool is_i64, size_t pix, long long value) {
  if (is_i64) reinterpret_cast<long long*>(out)[pix] = value;
  else reinterpret_cast<uint8_t*>(out)[pix] = (uint8_t)value;
}
__device__ __forceinline__ void store_labels4(void* __restrict__ out, bool is_i64, size_t first_pix, const long long (&l)[4]) {
  if (is_i64) {
    i64x2* p = reinterpret_cast<i64x2*>(reinterpret_cast<long long*>(out) + first_pix);
    p[0] = i64x2{l[0], l[1]};
    p[1] = i64x2{l[2], l[3]};
  } else {
    *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(out) + first_pix) =
        ((uint32_t)l[0] & 255u) | (((uint32_t)l[1] & 255u) << 8) | (((uint32_t)l[2] & 255u) << 16) | (((uint32_t)l[3] & 255u) << 24);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Unsigned division by a runtime-invariant divisor (n < 2^31): q = (umulhi(n, mul) + n) >> shift.
struct FastDiv {
  uint32_t div, mul, shift;
};
inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.div = d;
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  f.shift = s;
  f.mul = (uint32_t)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
  return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  return (uint32_t)(((uint64_t)__umulhi(n, f.mul) + n) >> f.shift);
}

// XCD-aware tile order: consecutive tile ids (sharing A rows / weights) stay on one XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Run-time value -> template argument: f(std::integral_constant<int, V>{}) for the listed V that equals v, the LAST one when
// none does.
template <int V0, int... Vs, typename F>
inline int pick(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
  else return v == V0 ? f(std::integral_constant<int, V0>{}) : pick<Vs...>(v, f);
}
// the (bm, bn) tiles of the single-role kernels: f(BM, BN)
template <typename F>
inline int pick_tile(int bm, int bn, F&& f) {
  return pick<128, 64>(bm, [&](auto BM) { return pick<128, 64>(bn, [&](auto BN) { return f(BM, BN); }); });
}

// ---- ReLU bits of an fp32 tensor: one bit per element ("the activation's output was positive"), written by the
// BatchNorm + add + ReLU pass of a residual block and read wherever its backward needs the mask — 1/32 of the bytes of the
// output tensor it replaces there (csrc/bn.hip).  Layout: the tensor is cut into 16-byte elements j (4 floats), 64 of
// them make a chunk of 8 words: word (j >> 6) * 8 + ((j >> 5) & 1) * 4 + e holds, at bit (j & 31), the bit of float e of
// element j — so a writer that owns element j = wave-chunk * 64 + lane gets its four words from four wave ballots, and a
// reader with ANY thread-to-element mapping fetches one aligned 16-byte group and shifts.
__host__ __device__ inline size_t relu_bits_words(size_t n4) { return ((n4 + 63) / 64) * 8; }
__device__ __forceinline__ f32x4 relu_bits_mask(f32x4 g, const uint32_t* __restrict__ bits, size_t j) {
  const u32x4 w = *reinterpret_cast<const u32x4*>(bits + (j >> 6) * 8 + ((j >> 5) & 1) * 4);
  const uint32_t b = (uint32_t)(j & 31);
  f32x4 o;
  o.x = ((w.x >> b) & 1u) ? g.x : 0.f;
  o.y = ((w.y >> b) & 1u) ? g.y : 0.f;
  o.z = ((w.z >> b) & 1u) ? g.z : 0.f;
  o.w = ((w.w >> b) & 1u) ? g.w : 0.f;
  return o;
}
// writer: every lane of the wave calls this with ITS element j = chunk * 64 + lane (inactive elements pass pos = 0 bits)
__device__ __forceinline__ void relu_bits_store(uint32_t* __restrict__ bits, size_t chunk, bool p0, bool p1, bool p2, bool p3) {
  const uint64_t b0 = __ballot(p0), b1 = __ballot(p1), b2 = __ballot(p2), b3 = __ballot(p3);
  const int lane = threadIdx.x & 63;
  if (lane == 0)
    *reinterpret_cast<u32x4*>(bits + chunk * 8) = u32x4{(uint32_t)b0, (uint32_t)b1, (uint32_t)b2, (uint32_t)b3};
  if (lane == 32)
    *reinterpret_cast<u32x4*>(bits + chunk * 8 + 4) =
        u32x4{(uint32_t)(b0 >> 32), (uint32_t)(b1 >> 32), (uint32_t)(b2 >> 32), (uint32_t)(b3 >> 32)};
}


// max|v| of what a workgroup wrote into slot (workgroup & 63) of the output's operand-scale buffer (64 slots 32 words
// apart, zero on entry; include/ever_hip.h: evk_absmax) — one atomic per wave, as the BatchNorm and convolution epilogues
__device__ __forceinline__ uint32_t abs4_bits(uint32_t m, const f32x4 v) {
  // by value into floats first: __builtin_bit_cast on a vector-element lvalue (v.y) reads element 0 with this compiler
  const float x = v.x, y = v.y, z = v.z, w = v.w;
  m = max(m, __float_as_uint(x) & 0x7fffffffu); m = max(m, __float_as_uint(y) & 0x7fffffffu);
  m = max(m, __float_as_uint(z) & 0x7fffffffu); m = max(m, __float_as_uint(w) & 0x7fffffffu);
  return m;
}
__device__ __forceinline__ void commit_absmax(uint32_t* __restrict__ slots, uint32_t m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(&slots[(blockIdx.x & 63) * 32], m);
}

// Grid of the streaming kernels (stream_common.hpp: launch_elems; csrc/hr_fuse.hip): one element per thread (their grid-stride loops then run once): resident workgroups sweep one contiguous
// window of HBM in dispatch order, 6.1 TB/s for 1R+1W on 268 MB against 5.1 for 4096 grid-striding workgroups
// (tools/probes/copy_patterns.hip).
static inline int grid_for(size_t n, int per_block = 256, int cap = 1 << 24) {
  size_t b = (n + per_block - 1) / per_block;
  return (int)(b > (size_t)cap ? cap : (b < 1 ? 1 : b));
}

}  // namespace evk
