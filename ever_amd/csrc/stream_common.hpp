// What the streaming translation units share — pointwise.hip: element-wise and layout kernels; pool.hip: pools and
// selections; resample.hip: bilinear resampling; relation.hip: FS-Relation; hr_fuse.hip, wfuse.hip, ppm.hip: the
// multi-resolution maps; depthwise.hip — the 16-byte element, the NHWC element decode, the element a finer map reads in a
// coarser one, the 2 x 2 quad, the per-channel sum over the pixels and its adjoint, the argument checks of an NHWC map and of
// a term table, and the one-element-per-thread launch.  Header only.
// wfuse.hip and ppm.hip round every product on its own (`fp contract(off)`) while this header is compiled with contraction
// on, and a product inlined from here was fused with the addition behind it (csrc/ppm.hip: ppm_tap).  So the device code
// below is integer arithmetic, loads, stores and additions; the one product, the `* inv` of sum_hw_body and
// broadcast_hw_body, has no addition behind it.
#pragma once
#include "common.hpp"

namespace evk {

// the 16-byte element e of a float map; without e, the one at p itself
__device__ __forceinline__ f32x4 ld4(const float* p, size_t e = 0) { return *reinterpret_cast<const f32x4*>(p + e * 4); }
__device__ __forceinline__ void st4(float* p, size_t e, const f32x4 v) { *reinterpret_cast<f32x4*>(p + e * 4) = v; }
__device__ __forceinline__ void st4(float* p, const f32x4 v) { st4(p, 0, v); }

// Element i of a map [N][H][W][C / VEC] (cv = C / VEC elements per pixel): image, row, column, channel chunk.  H and W are
// the dims of the map that is being WALKED — the call site names it.
struct NhwcElem {
  int n, y, x, cb;
};
__device__ __forceinline__ NhwcElem nhwc_elem(size_t i, int H, int W, int cv) {
  NhwcElem e;
  e.cb = (int)(i % cv);
  size_t pix = i / cv;
  e.x = (int)(pix % W);
  pix /= W;
  e.y = (int)(pix % H);
  e.n = (int)(pix / H);
  return e;
}

// the same by multiply-shift (j < 2^31): fc4, fW, fH divide by C / 4, W and H of the map that is being walked
__device__ __forceinline__ NhwcElem nhwc_elem(uint32_t j, const FastDiv& fc4, const FastDiv& fW, const FastDiv& fH) {
  NhwcElem e;
  const uint32_t pix = fdiv(j, fc4), r = fdiv(pix, fW), n = fdiv(r, fH);
  e.cb = (int)(j - pix * fc4.div);
  e.x = (int)(pix - r * fW.div);
  e.y = (int)(r - n * fH.div);
  e.n = (int)n;
  return e;
}

// Nearest x 2^s: the element that e of an [N][H][W][c4] map reads in the [N][H >> s][W >> s][c4] map 2^s coarser
__device__ __forceinline__ size_t coarse_elem(const NhwcElem& e, uint32_t H, uint32_t W, size_t c4, int s) {
  return (((size_t)(uint32_t)e.n * (H >> s) + ((uint32_t)e.y >> s)) * (W >> s) + ((uint32_t)e.x >> s)) * c4 + (uint32_t)e.cb;
}

// The 2 x 2 block of pixels whose first is column x of row `row` of the [N * H][W] pixel grid, at channel chunk cb of c4: its
// four elements, and the order in which every block sum adds them
struct Quad {
  size_t e00, e01, e10, e11;
};
__device__ __forceinline__ Quad quad_elems(size_t row, uint32_t x, int W, uint32_t c4, uint32_t cb) {
  Quad q;
  q.e00 = (row * W + x) * c4 + cb;
  q.e01 = q.e00 + c4;
  q.e10 = q.e00 + (size_t)W * c4;
  q.e11 = q.e10 + c4;
  return q;
}
__device__ __forceinline__ f32x4 quad_sum(const f32x4 a, const f32x4 b, const f32x4 c, const f32x4 d) { return (a + b) + (c + d); }

// y[n][c] = inv * sum over p of x[n][p][c] for x [N][HW][C], in a fixed order: grid (ceil(c4 / tpc), N), a workgroup = tpc
// 16-byte channel columns x rl pixel slices; slice tr adds pixels tr, tr + rl, ... and the slices meet in LDS in slice order.
// Count: the entry point's type of a pixel count.
template <typename Count>
__device__ __forceinline__ void sum_hw_body(const float* __restrict__ x, float* __restrict__ y, Count HW, int C, int tpc,
                                            int rl, float inv) {
  __shared__ f32x4 red[256];
  const int c4 = C >> 2;
  const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
  const int cb = blockIdx.x * tpc + tc;
  const Count n = blockIdx.y;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (cb < c4 && tr < rl)
    for (Count p = tr; p < HW; p += rl) s += ld4(x, ((size_t)n * HW + p) * c4 + cb);
  red[threadIdx.x] = s;
  __syncthreads();
  if (tr == 0 && cb < c4) {
    for (int k = 1; k < rl; ++k) s += red[k * tpc + tc];
    st4(y, (size_t)n * c4 + cb, s * inv);
  }
}
// its adjoint, dx[n][p][c] = inv * dy[n][c]: a grid-stride walk of the total4 = N HW c4 elements of dx
template <typename Count>
__device__ __forceinline__ void broadcast_hw_body(const float* __restrict__ dy, float* __restrict__ dx, Count total4, Count HW,
                                                  int C, float inv) {
  const int c4 = C >> 2;
  for (Count i = (Count)blockIdx.x * 256 + threadIdx.x; i < total4; i += (Count)gridDim.x * 256) {
    const int cb = (int)(i % c4);
    const Count n = i / (HW * c4);
    st4(dx, i, ld4(dy, n * c4 + cb) * inv);
  }
}

// an NHWC map (H = HW, W = 1 for the kernels that take pixels as one axis) of 16-byte channel chunks
inline bool nhwc4_ok(int N, int H, int W, int C) { return N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0; }

// The terms of a multi-resolution sum (hr_fuse.hip, wfuse.hip), term k an [N][H >> shifts[k]][W >> shifts[k]][C] map: non-null
// (terms null: the call reads none), its shift within [0, max_shift], H and W multiples of 2^shift.  A family that shifts by
// one at most words the last two its own way.
inline int check_terms(const char* what, const float* const* terms, const int32_t* shifts, int nterms, int max_shift, int H, int W) {
  int smax = 0;
  for (int k = 0; k < nterms; ++k) {
    const int s = shifts[k];
    EVK_REQUIRE(!terms || terms[k], EVK_E_INVALID, "%s: term %d is a null pointer", what, k);
    if (max_shift == 1) {
      EVK_REQUIRE(s == 0 || s == 1, EVK_E_UNSUPPORTED, "%s: term %d has shift %d (0 and 1 are implemented)", what, k, s);
      EVK_REQUIRE(s == 0 || (H % 2 == 0 && W % 2 == 0), EVK_E_UNSUPPORTED, "%s: H = %d, W = %d must be even (term %d has shift 1)",
                  what, H, W, k);
    } else {
      EVK_REQUIRE(s >= 0 && s <= max_shift, EVK_E_UNSUPPORTED, "%s: term %d has shift %d (0 to %d are implemented)", what, k, s,
                  max_shift);
    }
    smax = s > smax ? s : smax;
  }
  EVK_REQUIRE(H % (1 << smax) == 0 && W % (1 << smax) == 0, EVK_E_UNSUPPORTED,
              "%s: H = %d, W = %d must be multiples of %d (the largest shift is %d)", what, H, W, 1 << smax, smax);
  return EVK_OK;
}

// kernel<<<grid_for(n), 256>>>(args...) for a kernel that takes one of its n elements per thread, and the launch check
// under the entry point's name
template <typename... KArgs, typename... Args>
inline int launch_elems(const char* what, void (*kernel)(KArgs...), size_t n, void* stream, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, static_cast<KArgs>(args)...);
  return check_launch(what);
}

}  // namespace evk
