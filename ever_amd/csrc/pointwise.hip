// HBM-bound element-wise and layout kernels of the EVer hot path on NHWC fp32 (gfx950): ReLU / add / scale / GELU, the
// decoder's 4-way mean, channel padding and NCHW<->NHWC at the model boundary, grouped <-> dense convolution weights.
// (Pools: pool.hip; bilinear resampling: resample.hip; FS-Relation: relation.hip.)
// Reference call sites are cited per entry point in include/ever_hip.h.
// The element-wise kernels use 16-byte accesses with a scalar tail.
#include "stream_common.hpp"

namespace evk {

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// aten's relu is clamp_min(x, 0): -0.0 stays -0.0 (fmaxf gives +0.0 on this hardware).  A NaN becomes 0 here, as under fmaxf.
__device__ __forceinline__ float relu_f(float x) { return x >= 0.f ? x : 0.f; }

template <int OP>  // 0 relu, 1 relu_bwd, 2 add, 3 scale, 4 a*b*alpha, 5 gelu, 6 gelu_bwd (a = dy, b = x)
__global__ __launch_bounds__(256) void ew_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                 float* __restrict__ o, size_t n, float alpha) {
  const size_t n4 = n >> 2;
  const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
  const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
  f32x4* o4 = reinterpret_cast<f32x4*>(o);
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 v = a4[i];
    if (OP == 0) {
      v.x = relu_f(v.x); v.y = relu_f(v.y); v.z = relu_f(v.z); v.w = relu_f(v.w);
    } else if (OP == 1) {  // a = dy, b = y
      const f32x4 y = b4[i];
      v.x = y.x > 0.f ? v.x : 0.f; v.y = y.y > 0.f ? v.y : 0.f;
      v.z = y.z > 0.f ? v.z : 0.f; v.w = y.w > 0.f ? v.w : 0.f;
    } else if (OP == 2) {
      v += b4[i];
    } else if (OP == 3) {
      v *= alpha;
    } else if (OP == 4) {
      v = v * b4[i] * alpha;
    } else if (OP == 5) {
      v.x = gelu_f(v.x); v.y = gelu_f(v.y); v.z = gelu_f(v.z); v.w = gelu_f(v.w);
    } else {
      const f32x4 x = b4[i];
      v.x *= gelu_d(x.x); v.y *= gelu_d(x.y); v.z *= gelu_d(x.z); v.w *= gelu_d(x.w);
    }
    o4[i] = v;
  }
  // tail
  for (size_t i = (n4 << 2) + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float v = a[i];
    if (OP == 0) v = relu_f(v);
    else if (OP == 1) v = b[i] > 0.f ? v : 0.f;
    else if (OP == 2) v += b[i];
    else if (OP == 3) v *= alpha;
    else if (OP == 4) v = v * b[i] * alpha;
    else if (OP == 5) v = gelu_f(v);
    else v *= gelu_d(b[i]);
    o[i] = v;
  }
}

__global__ __launch_bounds__(256) void mean4_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                    const float* __restrict__ c, const float* __restrict__ d,
                                                    float* __restrict__ o, size_t n4, uint32_t* __restrict__ amax) {
  const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
  const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
  const f32x4* c4 = reinterpret_cast<const f32x4*>(c);
  const f32x4* d4 = reinterpret_cast<const f32x4*>(d);
  f32x4* o4 = reinterpret_cast<f32x4*>(o);
  uint32_t m = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = (((a4[i] + b4[i]) + c4[i]) + d4[i]) * 0.25f;  // same association as python sum(list)/4
    o4[i] = v;
    m = abs4_bits(m, v);
  }
  if (amax) commit_absmax(amax, m);
}

// ------------------------------------------------------------------------------------------------
__global__ void pad_channels_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t rows, int C,
                                    int Cp) {
  const size_t total = rows * (size_t)Cp;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / Cp;
    const int c = (int)(i - r * Cp);
    dst[i] = c < C ? src[r * C + c] : 0.f;
  }
}
__global__ void unpad_channels_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t rows, int Cp,
                                      int C) {
  const size_t total = rows * (size_t)C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / C;
    const int c = (int)(i - r * C);
    dst[i] = src[r * Cp + c];
  }
}
// one thread per pixel: plane reads are coalesced across lanes, the Cp-wide pixel is written whole
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, size_t HW,
                                    int Cp) {
  const size_t total = (size_t)N * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t n = i / HW, p = i - n * HW;
    const float* s = src + n * C * HW + p;
    float* d = dst + i * Cp;
    for (int c = 0; c < Cp; ++c) d[c] = c < C ? s[(size_t)c * HW] : 0.f;
  }
}
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, size_t HW,
                                    int Cp) {
  const size_t total = (size_t)N * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t n = i / HW, p = i - n * HW;
    const float* s = src + i * Cp;
    float* d = dst + n * C * HW + p;
    for (int c = 0; c < C; ++c) d[(size_t)c * HW] = s[c];
  }
}

// ------------------------------------------------------------------------------------------------
// Grouped convolution as a dense one (reference _resnets.py:21-24 `groups=groups`, the ResNeXt bodies :291-324): the
// weight [Cout][taps][Cin / groups] becomes the block-diagonal dense [Cout][taps][Cin], zeros outside an output channel's
// group — exact (the zeros contribute exact zeros in every arithmetic), and at 32 groups x 4..8 channels the dense form is
// what fills an MFMA tile anyway.  The adjoint gathers the diagonal blocks of the dense weight gradient.
__global__ __launch_bounds__(256) void group_weight_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cout,
                                                           int taps, int Cin, int groups, int gather) {
  const int cpg = Cin / groups, opg = Cout / groups;
  const size_t n = (size_t)Cout * taps * (gather ? cpg : Cin);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (gather) {   // dst = grouped [Cout][taps][cpg], src = dense
      const int c = (int)(i % cpg);
      const size_t r = i / cpg;           // co * taps + tap
      const int co = (int)(r / taps);
      dst[i] = src[r * Cin + (size_t)(co / opg) * cpg + c];
    } else {        // dst = dense [Cout][taps][Cin], src = grouped
      const int ci = (int)(i % Cin);
      const size_t r = i / Cin;
      const int co = (int)(r / taps), g = co / opg;
      const int c = ci - g * cpg;
      dst[i] = (c >= 0 && c < cpg) ? src[r * cpg + c] : 0.f;
    }
  }
}

}  // namespace evk

using namespace evk;

template <int OP>
static int ew_launch(const char* name, const float* a, const float* b, float* o, int64_t n, float alpha, void* stream) {
  EVK_REQUIRE(a && o && n >= 0, EVK_E_INVALID, "%s: bad argument", name);
  if (n == 0) return EVK_OK;
  return launch_elems(name, ew_kernel<OP>, ((size_t)n + 3) / 4, stream, a, b, o, n, alpha);
}

extern "C" int evk_relu_fwd(const float* x, float* y, int64_t n, void* stream) {
  return ew_launch<0>("relu_fwd", x, nullptr, y, n, 0.f, stream);
}
extern "C" int evk_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream) {
  EVK_REQUIRE(y, EVK_E_INVALID, "relu_bwd: null y");
  return ew_launch<1>("relu_bwd", dy, y, dx, n, 0.f, stream);
}
extern "C" int evk_add(const float* a, const float* b, float* out, int64_t n, void* stream) {
  EVK_REQUIRE(b, EVK_E_INVALID, "add: null b");
  return ew_launch<2>("add", a, b, out, n, 0.f, stream);
}
extern "C" int evk_scale(const float* a, float alpha, float* out, int64_t n, void* stream) {
  return ew_launch<3>("scale", a, nullptr, out, n, alpha, stream);
}
extern "C" int evk_mul_scale(const float* a, const float* b, float alpha, float* out, int64_t n, void* stream) {
  EVK_REQUIRE(b, EVK_E_INVALID, "mul_scale: null b");
  return ew_launch<4>("mul_scale", a, b, out, n, alpha, stream);
}
extern "C" int evk_gelu_fwd(const float* x, float* y, int64_t n, void* stream) {
  return ew_launch<5>("gelu_fwd", x, nullptr, y, n, 0.f, stream);
}
extern "C" int evk_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
  EVK_REQUIRE(x, EVK_E_INVALID, "gelu_bwd: null x");
  return ew_launch<6>("gelu_bwd", dy, x, dx, n, 0.f, stream);
}
extern "C" int evk_mean4_fwd(const float* a, const float* b, const float* c, const float* d, float* out, int64_t n,
                             uint32_t* out_absmax, void* stream) {
  EVK_REQUIRE(a && b && c && d && out && n > 0 && n % 4 == 0, EVK_E_INVALID, "mean4: bad argument");
  return launch_elems("mean4", mean4_kernel, (size_t)n / 4, stream, a, b, c, d, out, (size_t)n / 4, out_absmax);
}

static int group_weight(const float* src, float* dst, int Cout, int taps, int Cin, int groups, int gather, void* stream) {
  EVK_REQUIRE(src && dst, EVK_E_INVALID, "group_weight: null pointer");
  EVK_REQUIRE(Cout > 0 && taps > 0 && Cin > 0 && groups > 0 && Cin % groups == 0 && Cout % groups == 0, EVK_E_INVALID,
              "group_weight: Cout=%d Cin=%d groups=%d", Cout, Cin, groups);
  const size_t n = (size_t)Cout * taps * (gather ? Cin / groups : Cin);
  const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  hipLaunchKernelGGL(group_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, dst, Cout, taps, Cin, groups, gather);
  return check_launch("group_weight");
}
extern "C" int evk_group_weight_expand(const float* w, float* dense, int32_t Cout, int32_t taps, int32_t Cin, int32_t groups,
                                       void* stream) {
  return group_weight(w, dense, Cout, taps, Cin, groups, 0, stream);
}
extern "C" int evk_group_weight_gather(const float* ddense, float* dw, int32_t Cout, int32_t taps, int32_t Cin, int32_t groups,
                                       void* stream) {
  return group_weight(ddense, dw, Cout, taps, Cin, groups, 1, stream);
}

extern "C" int evk_pad_channels(const float* src, float* dst, int64_t rows, int32_t C, int32_t Cp, void* stream) {
  EVK_REQUIRE(src && dst && rows > 0 && C > 0 && Cp >= C, EVK_E_INVALID, "pad_channels: bad argument");
  return launch_elems("pad_channels", pad_channels_kernel, (size_t)rows * Cp, stream, src, dst, rows, C, Cp);
}
extern "C" int evk_unpad_channels(const float* src, float* dst, int64_t rows, int32_t Cp, int32_t C, void* stream) {
  EVK_REQUIRE(src && dst && rows > 0 && C > 0 && Cp >= C, EVK_E_INVALID, "unpad_channels: bad argument");
  return launch_elems("unpad_channels", unpad_channels_kernel, (size_t)rows * C, stream, src, dst, rows, Cp, C);
}
extern "C" int evk_nchw_to_nhwc(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Cp,
                                void* stream) {
  EVK_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && Cp >= C, EVK_E_INVALID, "nchw_to_nhwc: bad argument");
  return launch_elems("nchw_to_nhwc", nchw_to_nhwc_kernel, (size_t)N * H * W, stream, src, dst, N, C, (size_t)H * W, Cp);
}
extern "C" int evk_nhwc_to_nchw(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Cp,
                                void* stream) {
  EVK_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && Cp >= C, EVK_E_INVALID, "nhwc_to_nchw: bad argument");
  return launch_elems("nhwc_to_nchw", nhwc_to_nchw_kernel, (size_t)N * H * W, stream, src, dst, N, C, (size_t)H * W, Cp);
}
