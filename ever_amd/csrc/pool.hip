// Pools and selections of the EVer hot path on NHWC fp32 (gfx950): MaxPool 3x3 s2, the x2 sub-sampling of LastLevelMaxPool,
// nearest x2 + lateral add and its adjoint, global average pool, the broadcast of a 1x1 map and its adjoint.  16-byte
// accesses along the channel axis (C % 4 == 0).  Reference call sites are cited per entry point in include/ever_hip.h.
#include "stream_common.hpp"

namespace evk {

// ------------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1).  code[..] = winning tap ky*3+kx (first maximum in scan order, NaN propagates,
// matching aten's max_pool2d_with_indices).
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          uint8_t* __restrict__ code, int N, int H, int W, int C,
                                                          int Ho, int Wo) {
  const int c4 = C >> 2;
  const size_t total = (size_t)N * Ho * Wo * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const NhwcElem e = nhwc_elem(i, Ho, Wo, c4);     // of y
    const int n = e.n, oy = e.y, ox = e.x, cb = e.cb;
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bx = 0, by = 0, bz = 0, bw = 0;
    bool first = true;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * 2 - 1 + ky;
      if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 - 1 + kx;
        if ((unsigned)ix >= (unsigned)W) continue;
        const f32x4 v = ld4(x + (((size_t)n * H + iy) * W + ix) * C + cb * 4);
        const int t = ky * 3 + kx;
        if (first) {
          best = v; bx = by = bz = bw = t; first = false;
        } else {
          if (v.x > best.x || v.x != v.x) { best.x = v.x; bx = t; }
          if (v.y > best.y || v.y != v.y) { best.y = v.y; by = t; }
          if (v.z > best.z || v.z != v.z) { best.z = v.z; bz = t; }
          if (v.w > best.w || v.w != v.w) { best.w = v.w; bw = t; }
        }
      }
    }
    const size_t o = (((size_t)n * Ho + oy) * Wo + ox) * C + cb * 4;
    st4(y + o, best);
    *reinterpret_cast<uint32_t*>(code + o) = (uint32_t)bx | ((uint32_t)by << 8) | ((uint32_t)bz << 16) | ((uint32_t)bw << 24);
  }
}
// gather-form adjoint: input pixel (iy,ix) is tap (iy-2oy+1, ix-2ox+1) of at most 2x2 windows
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy,
                                                          const uint8_t* __restrict__ code, float* __restrict__ dx,
                                                          int N, int H, int W, int C, int Ho, int Wo) {
  const int c4 = C >> 2;
  const size_t total = (size_t)N * H * W * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const NhwcElem e = nhwc_elem(i, H, W, c4);       // of dx
    const int n = e.n, iy = e.y, ix = e.x, cb = e.cb;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    const int oy_lo = max(0, iy >> 1), oy_hi = min(Ho - 1, (iy + 1) >> 1);
    const int ox_lo = max(0, ix >> 1), ox_hi = min(Wo - 1, (ix + 1) >> 1);
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      const int ky = iy - 2 * oy + 1;
      if ((unsigned)ky > 2u) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        const int kx = ix - 2 * ox + 1;
        if ((unsigned)kx > 2u) continue;
        const uint32_t t = (uint32_t)(ky * 3 + kx);
        const size_t o = (((size_t)n * Ho + oy) * Wo + ox) * C + cb * 4;
        const uint32_t cd = *reinterpret_cast<const uint32_t*>(code + o);
        const f32x4 d = ld4(dy + o);
        if ((cd & 0xff) == t) g.x += d.x;
        if (((cd >> 8) & 0xff) == t) g.y += d.y;
        if (((cd >> 16) & 0xff) == t) g.z += d.z;
        if ((cd >> 24) == t) g.w += d.w;
      }
    }
    st4(dx, i, g);
  }
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nearest2x_add_kernel(const float* __restrict__ top,
                                                            const float* __restrict__ lateral,
                                                            float* __restrict__ out, int N, int H, int W, int C,
                                                            uint32_t* __restrict__ amax) {
  const int c4 = C >> 2;
  const size_t total = (size_t)N * H * W * c4;
  uint32_t m = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const NhwcElem e = nhwc_elem(i, H, W, c4);       // of out (the fine map)
    const f32x4 v = ld4(lateral, i) + ld4(top, coarse_elem(e, H, W, c4, 1));
    st4(out, i, v);
    m = abs4_bits(m, v);
  }
  if (amax) commit_absmax(amax, m);
}
__global__ __launch_bounds__(256) void nearest2x_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dtop,
                                                            int N, int H, int W, int C) {
  // H, W are the fine (dout) dims
  const int c4 = C >> 2;
  const int Ht = H >> 1, Wt = W >> 1;
  const size_t total = (size_t)N * Ht * Wt * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const NhwcElem e = nhwc_elem(i, Ht, Wt, c4);     // of dtop (the coarse map)
    const Quad q = quad_elems((size_t)e.n * H + 2 * e.y, 2 * e.x, W, c4, e.cb);
    st4(dtop, i, quad_sum(ld4(dout, q.e00), ld4(dout, q.e01), ld4(dout, q.e10), ld4(dout, q.e11)));
  }
}

// F.max_pool2d(x, 1, 2, 0) — a window of ONE pixel, stride 2: y[n, yo, xo, :] = x[n, 2 yo, 2 xo, :] (reference fpn.py:118-120,
// LastLevelMaxPool).  ADJ = the adjoint: dx is dy at the even pixels and zero elsewhere (one thread per 16 bytes of dx).
template <bool ADJ>
__global__ __launch_bounds__(256) void subsample2_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int H,
                                                         int W, int C, int Ho, int Wo) {
  const int c4 = C >> 2;
  const size_t total = ADJ ? (size_t)N * H * W * c4 : (size_t)N * Ho * Wo * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const NhwcElem e = nhwc_elem(i, ADJ ? H : Ho, ADJ ? W : Wo, c4);     // of dst
    const int n = e.n, y = e.y, x = e.x, cb = e.cb;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!ADJ)
      v = ld4(src + (((size_t)n * H + 2 * y) * W + 2 * x) * C + cb * 4);
    else if (!(x & 1) && !(y & 1))
      v = ld4(src + (((size_t)n * Ho + (y >> 1)) * Wo + (x >> 1)) * C + cb * 4);
    st4(dst, i, v);
  }
}

// ------------------------------------------------------------------------------------------------
// The per-channel sums over the pixels of x [N][HW][C] and their adjoints, each a call of the shared body
// (stream_common.hpp: sum_hw_body, broadcast_hw_body) under its own launch geometry, which fixes the summation order.
// Global average pool: y [N][C] = mean over p of x[n][p][c]
__global__ __launch_bounds__(256) void gap_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int HW, int C,
                                                      int tpc, int rl, float inv) {
  sum_hw_body(x, y, HW, C, tpc, rl, inv);
}
__global__ __launch_bounds__(256) void gap_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N,
                                                      int HW, int C, float inv) {
  broadcast_hw_body(dy, dx, (size_t)N * HW * (C >> 2), (size_t)HW, C, inv);
}
// dst[n][p][c] = src[n][c]: the bilinear resize of a 1x1 map (every output pixel reads the one source pixel, weight 1;
// reference ever/module/ops.py:89-100, PoolBlock's interpolate), and its adjoint dst[n][c] = sum over p of src[n][p][c].
// x * 1.0f is x for every x.
__global__ __launch_bounds__(256) void broadcast_hw_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           int64_t total4, int64_t HW, int C) {
  broadcast_hw_body(src, dst, total4, HW, C, 1.f);
}
__global__ __launch_bounds__(256) void sum_hw_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t HW,
                                                     int C, int tpc, int rl) {
  sum_hw_body(src, dst, HW, C, tpc, rl, 1.f);
}

}  // namespace evk

using namespace evk;

extern "C" int evk_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* code, int32_t N, int32_t H, int32_t W, int32_t C,
                                    void* stream) {
  EVK_REQUIRE(x && y && code && nhwc4_ok(N, H, W, C), EVK_E_INVALID, "maxpool_fwd: bad argument");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  return launch_elems("maxpool_fwd", maxpool_fwd_kernel, (size_t)N * Ho * Wo * (C / 4), stream, x, y, code, N, H, W, C, Ho, Wo);
}
extern "C" int evk_maxpool3x3s2_bwd(const float* dy, const uint8_t* code, float* dx, int32_t N, int32_t H, int32_t W,
                                    int32_t C, void* stream) {
  EVK_REQUIRE(dy && dx && code && nhwc4_ok(N, H, W, C), EVK_E_INVALID, "maxpool_bwd: bad argument");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  return launch_elems("maxpool_bwd", maxpool_bwd_kernel, (size_t)N * H * W * (C / 4), stream, dy, code, dx, N, H, W, C, Ho, Wo);
}

extern "C" int evk_upsample_nearest2x_add_fwd(const float* top, const float* lateral, float* out, int32_t N, int32_t H,
                                              int32_t W, int32_t C, uint32_t* out_absmax, void* stream) {
  EVK_REQUIRE(top && lateral && out && nhwc4_ok(N, H, W, C) && H % 2 == 0 && W % 2 == 0, EVK_E_INVALID,
              "nearest2x_add: bad argument (H,W must be even, C %% 4 == 0)");
  return launch_elems("nearest2x_add", nearest2x_add_kernel, (size_t)N * H * W * (C / 4), stream, top, lateral, out, N, H, W, C,
                      out_absmax);
}
extern "C" int evk_upsample_nearest2x_bwd(const float* dout, float* dtop, int32_t N, int32_t H, int32_t W, int32_t C,
                                          void* stream) {
  EVK_REQUIRE(dout && dtop && nhwc4_ok(N, H, W, C) && H % 2 == 0 && W % 2 == 0, EVK_E_INVALID, "nearest2x_bwd: bad argument");
  return launch_elems("nearest2x_bwd", nearest2x_bwd_kernel, (size_t)N * (H / 2) * (W / 2) * (C / 4), stream, dout, dtop, N, H, W,
                      C);
}

extern "C" int evk_subsample2_fwd(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
  EVK_REQUIRE(x && y && nhwc4_ok(N, H, W, C), EVK_E_INVALID, "subsample2_fwd: bad argument (C %% 4 == 0)");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  return launch_elems("subsample2_fwd", subsample2_kernel<false>, (size_t)N * Ho * Wo * (C / 4), stream, x, y, N, H, W, C, Ho, Wo);
}
extern "C" int evk_subsample2_bwd(const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
  EVK_REQUIRE(dy && dx && nhwc4_ok(N, H, W, C), EVK_E_INVALID, "subsample2_bwd: bad argument (C %% 4 == 0)");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  return launch_elems("subsample2_bwd", subsample2_kernel<true>, (size_t)N * H * W * (C / 4), stream, dy, dx, N, H, W, C, Ho, Wo);
}

extern "C" int evk_gap_fwd(const float* x, float* y, int32_t N, int32_t HW, int32_t C, void* stream) {
  EVK_REQUIRE(x && y && nhwc4_ok(N, HW, 1, C), EVK_E_INVALID, "gap_fwd: bad argument");
  const int c4 = C / 4;
  const int tpc = c4 < 64 ? c4 : 64;
  const int rl = 256 / tpc;
  hipLaunchKernelGGL(gap_fwd_kernel, dim3((c4 + tpc - 1) / tpc, N), dim3(256), 0, (hipStream_t)stream, x, y, HW, C,
                     tpc, rl, 1.f / (float)HW);
  return check_launch("gap_fwd");
}
extern "C" int evk_gap_bwd(const float* dy, float* dx, int32_t N, int32_t HW, int32_t C, void* stream) {
  EVK_REQUIRE(dy && dx && nhwc4_ok(N, HW, 1, C), EVK_E_INVALID, "gap_bwd: bad argument");
  return launch_elems("gap_bwd", gap_bwd_kernel, (size_t)N * HW * (C / 4), stream, dy, dx, N, HW, C, 1.f / (float)HW);
}

extern "C" int evk_broadcast_hw(const float* src, float* dst, int32_t N, int64_t HW, int32_t C, void* stream) {
  EVK_REQUIRE(src && dst && N > 0 && HW > 0 && C > 0 && C % 4 == 0, EVK_E_INVALID, "broadcast_hw: bad argument");
  const int64_t total4 = (int64_t)N * HW * (C / 4);
  const int64_t blocks = (total4 + 255) / 256;
  hipLaunchKernelGGL(broadcast_hw_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, total4, (int64_t)HW, C);
  return check_launch("broadcast_hw");
}

extern "C" int evk_sum_hw(const float* src, float* dst, int32_t N, int64_t HW, int32_t C, void* stream) {
  EVK_REQUIRE(src && dst && N > 0 && HW > 0 && C > 0 && C % 4 == 0, EVK_E_INVALID, "sum_hw: bad argument");
  const int c4 = C / 4;
  const int tpc = c4 < 8 ? c4 : 8;     // 8 channel groups x 32 pixel slices per workgroup (ASPP: 16 x 1024 x 256 in 128 groups)
  const int rl = 256 / tpc;
  hipLaunchKernelGGL(sum_hw_kernel, dim3((c4 + tpc - 1) / tpc, N), dim3(256), 0, (hipStream_t)stream, src, dst,
                     (int64_t)HW, C, tpc, rl);
  return check_launch("sum_hw");
}
