// Host side and C ABI of the forward / data-gradient convolution family: descriptor checks, the residue-class plan of the
// strided data gradient, route-and-launch, every evk_conv2d_fwd* / evk_conv2d_dgrad* entry point and the fp32 data-gradient
// weight pack.  The kernels and their launchers: conv_igemm_f32.hip (fp32 MFMA, the gather's description), conv_igemm_x3.hip,
// conv_igemm_x3ws.hip, the 3x3 and one-tap files (conv_route.hpp names them all).
//
// Replaces aten::convolution / aten::convolution_backward(input) issued by nn.Conv2d at
// reference ever/module/_resnets.py:21-29,149 ; fpn.py:23-37,72-73,165,179 ; fs_relation.py:23-53.
#include "conv_route.hpp"

namespace evk {

static int check_desc(const evk_conv_desc* d) {
  EVK_REQUIRE(d, EVK_E_INVALID, "conv: null descriptor");
  EVK_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->kh > 0 && d->kw > 0,
              EVK_E_INVALID, "conv: non-positive dimension");
  EVK_REQUIRE(d->stride_h > 0 && d->stride_w > 0 && d->dil_h > 0 && d->dil_w > 0 && d->pad_h >= 0 &&
                  d->pad_w >= 0,
              EVK_E_INVALID, "conv: bad stride/dilation/padding");
  EVK_REQUIRE(d->Cin % 4 == 0, EVK_E_UNSUPPORTED,
              "conv: Cin=%d must be a multiple of 4 (use evk_pad_channels)", d->Cin);
  const int ho = (d->H + 2 * d->pad_h - d->dil_h * (d->kh - 1) - 1) / d->stride_h + 1;
  const int wo = (d->W + 2 * d->pad_w - d->dil_w * (d->kw - 1) - 1) / d->stride_w + 1;
  EVK_REQUIRE(ho == d->Ho && wo == d->Wo, EVK_E_INVALID, "conv: Ho/Wo (%d,%d) inconsistent, expect (%d,%d)",
              d->Ho, d->Wo, ho, wo);
  EVK_REQUIRE((long long)d->N * d->Ho * d->Wo < 0x7fffffffLL && (long long)d->N * d->H * d->W < 0x7fffffffLL,
              EVK_E_UNSUPPORTED, "conv: more than 2^31 pixels");
  return EVK_OK;
}

static int gcd_i(int a, int b) { return b == 0 ? a : gcd_i(b, a % b); }
AxisPlan plan_axis(int c, int pad, int dil, int stride, int ksize) {
  AxisPlan ap{0, 1, 0, 0, 0};
  const int g = gcd_i(dil, stride);
  if ((c + pad) % g != 0) return ap;  // no tap reaches this class
  ap.kstep = stride / g;
  int k0 = -1;
  for (int k = 0; k < ap.kstep && k < ksize; ++k)
    if ((c + pad - k * dil) % stride == 0) { k0 = k; break; }
  if (k0 < 0) return ap;
  ap.k0 = k0;
  ap.nt = (ksize - 1 - k0) / ap.kstep + 1;
  ap.o0 = (c + pad - k0 * dil) / stride;  // exact; may be negative
  ap.ostep = -(dil / g);
  return ap;
}

}  // namespace evk

using namespace evk;

// every forward / data-gradient launch: the planner names kernel and tile, the kernel's launcher does the rest
static int route_and_launch(IGemmArgs& a, hipStream_t stream) {
  const RouteKnobs knobs = route_knobs();
  ConvRoute r = route_conv(a, a.wgt3 != nullptr, knobs, kAnyDevice);
  if (r.kernel == ConvKernel::C1Ps2) {   // the one route that depends on the device: asked only then (a runtime call per launch)
    const int cus_per_xcd = device_cus_per_xcd();
    EVK_REQUIRE(cus_per_xcd > 0, EVK_E_LAUNCH, "conv: cannot query the device");
    r = route_conv(a, true, knobs, cus_per_xcd);
  }
  switch (r.kernel) {
    case ConvKernel::Igemm: return launch_igemm(a, r, stream);
    case ConvKernel::SmallM: return launch_conv1x1_smallm(a, r, stream);
    case ConvKernel::Wino: return launch_conv3x3_wino(a, r, stream);
    case ConvKernel::Halo: return launch_conv3x3_halo(a, r, stream);
    case ConvKernel::C1Ps2: return launch_conv1x1_ps2(a, r, stream);
    case ConvKernel::C1Dma: return launch_conv1x1_dma(a, r, stream);
    case ConvKernel::C1Sp: return launch_conv1x1_sp(a, r, stream);
    case ConvKernel::X3Ws: return launch_igemm_x3ws(a, r, stream);
    case ConvKernel::X3: return launch_igemm_x3(a, r, stream);
  }
  EVK_REQUIRE(false, EVK_E_INVALID, "conv: unknown route");
}

// w3 != nullptr selects the bf16-split kernel (conv_igemm_x3.hip) on pre-split weight planes
static int conv_fwd_any(const evk_conv_desc* d, const float* x, const float* w, const uint16_t* w3, const float* bias,
                        float* y, uint32_t flags, void* stream, const float* residual = nullptr,
                        float* bn_parts = nullptr, int32_t bn_cap = 0, int32_t* nparts = nullptr, int planes = 3,
                        const uint32_t* a_scale = nullptr, const uint32_t* w_scale = nullptr, uint32_t* out_amax = nullptr) {
  int rc = check_desc(d);
  if (rc) return rc;
  EVK_REQUIRE(x && (w || w3) && y, EVK_E_INVALID, "conv2d_fwd: null pointer");
  EVK_REQUIRE(residual != y, EVK_E_INVALID, "conv2d_fwd: residual must not alias y");
  IGemmArgs a = igemm_geometry_fwd(d);
  a.src = x; a.wgt = w; a.wgt3 = w3; a.bias = bias; a.accum = residual; a.dst = y;
  a.relu = (flags & EVK_CONV_RELU) ? 1 : 0;
  a.planes = planes;
  a.a_scale = a_scale; a.w_scale = w_scale;
  a.a_packed = (planes == 2 && (flags & EVK_CONV_X_PACKED)) ? 1 : 0;
  a.out_amax = out_amax;
  a.bn_want = (bn_parts && w3 && d->Cout % 4 == 0) ? 1 : 0;
  a.bn_buf = bn_parts;
  a.bn_cap = bn_cap;
  if (nparts) *nparts = 0;
  rc = route_and_launch(a, (hipStream_t)stream);
  if (nparts && rc == EVK_OK) *nparts = a.bn_parts;
  return rc;
}

extern "C" int evk_conv2d_fwd(const evk_conv_desc* d, const float* x, const float* w, const float* bias,
                              float* y, uint32_t flags, void* stream) {
  return conv_fwd_any(d, x, w, nullptr, bias, y, flags, stream);
}

extern "C" int evk_conv2d_fwd_x3(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                                 float* y, uint32_t flags, void* stream) {
  EVK_REQUIRE(wsplit, EVK_E_INVALID, "conv2d_fwd_x3: null weight planes");
  return conv_fwd_any(d, x, nullptr, reinterpret_cast<const uint16_t*>(wsplit), bias, y, flags, stream);
}

extern "C" int32_t evk_conv2d_stats_max_parts(const evk_conv_desc* d) {
  if (!d) return 0;
  // one record per tile of at least 64 rows
  return (int32_t)(((int64_t)d->N * d->Ho * d->Wo + 63) / 64 + 1);
}
extern "C" int evk_conv2d_fwd_x3_stats(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                                       float* y, uint32_t flags, float* bn_parts, int32_t bn_capacity, int32_t* nparts,
                                       void* stream) {
  EVK_REQUIRE(wsplit && bn_parts && nparts, EVK_E_INVALID, "conv2d_fwd_x3_stats: null pointer");
  return conv_fwd_any(d, x, nullptr, reinterpret_cast<const uint16_t*>(wsplit), bias, y, flags, stream, nullptr, bn_parts,
                      bn_capacity, nparts);
}

// Plain bf16 operands (ONE product per operand pair, fp32 accumulate): the counterpart of the reference's
// `--mixed_precision bf16`.  Same arguments and the same weight-plane buffers as the x3 forms (only plane 0 is read).
extern "C" int evk_conv2d_fwd_bf16(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias, float* y,
                                   uint32_t flags, float* bn_parts, int32_t bn_capacity, int32_t* nparts, void* stream) {
  EVK_REQUIRE(wsplit, EVK_E_INVALID, "conv2d_fwd_bf16: null weight planes");
  return conv_fwd_any(d, x, nullptr, reinterpret_cast<const uint16_t*>(wsplit), bias, y, flags, stream, nullptr, bn_parts,
                      bn_capacity, nparts, 1);
}

// 2-term fp16 split of operands scaled by a power of two (x3_common.hpp: NP = 2): three MFMA products per operand
// pair, 22-bit operands, fp32 accumulate — fp32-grade at half the matrix work of the x3 forms.  x_absmax / w_absmax:
// device words holding the bit image of max|x| (evk_absmax) and of max|w| (what the planes were produced with:
// evk_conv2d_split_weight_f16x2 / evk_conv2d_split_multi_f16x2).  residual, bn_parts, nparts may be null.
extern "C" int evk_conv2d_fwd_f16x2(const evk_conv_desc* d, const float* x, const uint32_t* x_absmax, const void* wsplit,
                                    const uint32_t* w_absmax, const float* bias, const float* residual, float* y,
                                    uint32_t flags, float* bn_parts, int32_t bn_capacity, int32_t* nparts,
                                    uint32_t* y_absmax, void* stream) {
  EVK_REQUIRE(wsplit && x_absmax && w_absmax, EVK_E_INVALID, "conv2d_fwd_f16x2: null weight planes / scales");
  return conv_fwd_any(d, x, nullptr, reinterpret_cast<const uint16_t*>(wsplit), bias, y, flags, stream, residual, bn_parts,
                      bn_capacity, nparts, 2, x_absmax, w_absmax, y_absmax);
}

// y = act(conv(x, w) + bias + residual): the inference form of a ResNet block's last convolution once its
// BatchNorm is folded into (w, bias) — reference _resnets.py:95-112 (`out += identity; relu`)
extern "C" int evk_conv2d_fwd_res(const evk_conv_desc* d, const float* x, const float* w, const float* bias,
                                  const float* residual, float* y, uint32_t flags, void* stream) {
  return conv_fwd_any(d, x, w, nullptr, bias, y, flags, stream, residual);
}
extern "C" int evk_conv2d_fwd_x3_res(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                                     const float* residual, float* y, uint32_t flags, void* stream) {
  EVK_REQUIRE(wsplit, EVK_E_INVALID, "conv2d_fwd_x3_res: null weight planes");
  return conv_fwd_any(d, x, nullptr, reinterpret_cast<const uint16_t*>(wsplit), bias, y, flags, stream, residual);
}

static int conv_dgrad_any(const evk_conv_desc* d, const float* dy, const float* wt, const uint16_t* wt3,
                          const float* accum, float* dx, void* stream, int planes = 3,
                          const uint32_t* a_scale = nullptr, const uint32_t* w_scale = nullptr, uint32_t* out_amax = nullptr,
                          int dy_packed = 0, const uint32_t* accum_bits = nullptr) {
  int rc = check_desc(d);
  if (rc) return rc;
  EVK_REQUIRE(dy && (wt || wt3) && dx, EVK_E_INVALID, "conv2d_dgrad: null pointer");
  EVK_REQUIRE(d->Cout % 4 == 0, EVK_E_UNSUPPORTED, "conv2d_dgrad: Cout=%d must be a multiple of 4", d->Cout);
  hipStream_t st = (hipStream_t)stream;
  const int sh = d->stride_h, sw = d->stride_w;
  // does every residue class receive at least one tap?  if not, those pixels of dx are plain zeros
  bool all_covered = true;
  for (int cy = 0; cy < sh; ++cy) all_covered = all_covered && plan_axis(cy, d->pad_h, d->dil_h, sh, d->kh).nt > 0;
  for (int cx = 0; cx < sw; ++cx) all_covered = all_covered && plan_axis(cx, d->pad_w, d->dil_w, sw, d->kw).nt > 0;
  // accum == dx (split kernels only): accumulate in place — every epilogue thread reads the accum quads of its row block
  // before it stores the same addresses (igemm_store_rows), and pixels no tap reaches already hold their value.  The
  // strided 1x1 shortcut of a residual block uses this: its data gradient touches one pixel in four of a tensor the
  // main branch's data gradient has just written, so the 268 MB fill / copy below disappears.
  EVK_REQUIRE(accum != dx || wt3, EVK_E_INVALID, "conv2d_dgrad: accum must not alias dx in the fp32 kernels");
  if (!all_covered && accum != dx) {  // pixels no tap reaches: dx = 0 (+ accum)
    const size_t bytes = (size_t)d->N * d->H * d->W * d->Cin * sizeof(float);
    hipError_t e = accum ? hipMemcpyAsync(dx, accum, bytes, hipMemcpyDeviceToDevice, st) : hipMemsetAsync(dx, 0, bytes, st);
    if (e != hipSuccess) { set_error("conv2d_dgrad fill: %s", hipGetErrorString(e)); return EVK_E_LAUNCH; }
  }
  size_t woff = 0;   // class weights are packed back to back by evk_conv2d_pack_dgrad_weight
  size_t woff3 = 0;  // ... and the class planes by evk_conv2d_split_weight(for_dgrad = 1)
  for (int cy = 0; cy < sh; ++cy)
    for (int cx = 0; cx < sw; ++cx) {
      IGemmArgs a = igemm_geometry_dgrad(d, cy, cx);
      if (a.kh > 0 && a.kw > 0 && a.Hm > 0 && a.Wm > 0) {
        a.planes = planes;
        a.a_scale = a_scale; a.w_scale = w_scale;
        a.a_packed = dy_packed;
        a.out_amax = out_amax;
        a.src = dy; a.wgt = wt ? wt + woff : nullptr; a.wgt3 = wt3 ? wt3 + woff3 : nullptr;
        a.accum = accum; a.dst = dx;
        a.accum_bits = accum_bits;
        rc = route_and_launch(a, st);
        if (rc) return rc;
      }
      woff += (size_t)d->Cin * a.Ktot;
      woff3 += (size_t)3 * d->Cin * a.Kpad;
    }
  return EVK_OK;
}

extern "C" int evk_conv2d_dgrad(const evk_conv_desc* d, const float* dy, const float* wt, const float* accum,
                                float* dx, void* stream) {
  return conv_dgrad_any(d, dy, wt, nullptr, accum, dx, stream);
}

extern "C" int evk_conv2d_dgrad_bf16(const evk_conv_desc* d, const float* dy, const void* wsplit_t, const float* accum,
                                     float* dx, void* stream) {
  EVK_REQUIRE(wsplit_t, EVK_E_INVALID, "conv2d_dgrad_bf16: null weight planes");
  return conv_dgrad_any(d, dy, nullptr, reinterpret_cast<const uint16_t*>(wsplit_t), accum, dx, stream, 1);
}

extern "C" int evk_conv2d_dgrad_f16x2(const evk_conv_desc* d, const float* dy, const uint32_t* dy_absmax,
                                      const void* wsplit_t, const uint32_t* w_absmax, const float* accum, float* dx,
                                      uint32_t* dx_absmax, void* stream) {
  EVK_REQUIRE(wsplit_t && dy_absmax && w_absmax, EVK_E_INVALID, "conv2d_dgrad_f16x2: null weight planes / scales");
  return conv_dgrad_any(d, dy, nullptr, reinterpret_cast<const uint16_t*>(wsplit_t), accum, dx, stream, 2, dy_absmax,
                        w_absmax, dx_absmax);
}

extern "C" int evk_conv2d_dgrad_f16x2_ex(const evk_conv_desc* d, const void* dy, const uint32_t* dy_absmax,
                                         const void* wsplit_t, const uint32_t* w_absmax, const float* accum, float* dx,
                                         uint32_t* dx_absmax, uint32_t flags, void* stream) {
  EVK_REQUIRE(wsplit_t && dy_absmax && w_absmax, EVK_E_INVALID, "conv2d_dgrad_f16x2_ex: null weight planes / scales");
  EVK_REQUIRE((flags & ~EVK_CONV_DY_PACKED) == 0, EVK_E_INVALID, "conv2d_dgrad_f16x2_ex: unknown flag 0x%x", flags);
  return conv_dgrad_any(d, reinterpret_cast<const float*>(dy), nullptr, reinterpret_cast<const uint16_t*>(wsplit_t), accum, dx,
                        stream, 2, dy_absmax, w_absmax, dx_absmax, (flags & EVK_CONV_DY_PACKED) ? 1 : 0);
}

// accum_bits: ReLU bits of `accum` (evk_bn_fwd_train_parts_bits): dx = dgrad + (accum where its bit is set).  Stride 1 only.
extern "C" int evk_conv2d_dgrad_f16x2_masked(const evk_conv_desc* d, const void* dy, const uint32_t* dy_absmax,
                                             const void* wsplit_t, const uint32_t* w_absmax, const float* accum,
                                             const uint32_t* accum_bits, float* dx, uint32_t* dx_absmax, uint32_t flags,
                                             void* stream) {
  EVK_REQUIRE(wsplit_t && dy_absmax && w_absmax && accum && accum_bits, EVK_E_INVALID, "conv2d_dgrad_f16x2_masked: null pointer");
  EVK_REQUIRE((flags & ~EVK_CONV_DY_PACKED) == 0, EVK_E_INVALID, "conv2d_dgrad_f16x2_masked: unknown flag 0x%x", flags);
  EVK_REQUIRE(d && d->stride_h == 1 && d->stride_w == 1 && d->Cin % 4 == 0 && accum != dx, EVK_E_UNSUPPORTED,
              "conv2d_dgrad_f16x2_masked: stride-1 convolutions with Cin %% 4 == 0, accum distinct from dx");
  return conv_dgrad_any(d, reinterpret_cast<const float*>(dy), nullptr, reinterpret_cast<const uint16_t*>(wsplit_t), accum, dx,
                        stream, 2, dy_absmax, w_absmax, dx_absmax, (flags & EVK_CONV_DY_PACKED) ? 1 : 0, accum_bits);
}

extern "C" int evk_conv2d_dgrad_x3(const evk_conv_desc* d, const float* dy, const void* wsplit_t, const float* accum,
                                   float* dx, void* stream) {
  EVK_REQUIRE(wsplit_t, EVK_E_INVALID, "conv2d_dgrad_x3: null weight planes");
  return conv_dgrad_any(d, dy, nullptr, reinterpret_cast<const uint16_t*>(wsplit_t), accum, dx, stream);
}

// Class-ordered data-gradient weights: for each residue class (cy, cx) in row-major order a block
// wt_c[ci][jy][jx][co] = w[co][ky0 + jy*kstep_y][kx0 + jx*kstep_x][ci].  Every tap belongs to exactly
// one class, so the total size is Cin*kh*kw*Cout; for stride 1 it is the plain [Cin][kh][kw][Cout].
__global__ void pack_dgrad_weight_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cout, int kh, int kw,
                                         int Cin, int ky0, int ksy, int nty, int kx0, int ksx, int ntx) {
  const size_t total = (size_t)Cin * nty * ntx * Cout;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout);
    size_t r = i / Cout;
    const int jx = (int)(r % ntx);
    r /= ntx;
    const int jy = (int)(r % nty);
    const int ci = (int)(r / nty);
    const int ky = ky0 + jy * ksy, kx = kx0 + jx * ksx;
    wt[i] = w[(((size_t)co * kh + ky) * kw + kx) * Cin + ci];
  }
}

extern "C" int evk_conv2d_pack_dgrad_weight(const evk_conv_desc* d, const float* w, float* wt, void* stream) {
  EVK_REQUIRE(d && w && wt, EVK_E_INVALID, "pack_dgrad_weight: null pointer");
  EVK_REQUIRE(d->stride_h > 0 && d->stride_w > 0 && d->dil_h > 0 && d->dil_w > 0, EVK_E_INVALID,
              "pack_dgrad_weight: bad stride/dilation");
  size_t woff = 0;
  for (int cy = 0; cy < d->stride_h; ++cy)
    for (int cx = 0; cx < d->stride_w; ++cx) {
      const AxisPlan py = plan_axis(cy, d->pad_h, d->dil_h, d->stride_h, d->kh);
      const AxisPlan px = plan_axis(cx, d->pad_w, d->dil_w, d->stride_w, d->kw);
      const size_t total = (size_t)d->Cin * py.nt * px.nt * d->Cout;
      if (total > 0) {
        const int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
        hipLaunchKernelGGL(pack_dgrad_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, wt + woff,
                           d->Cout, d->kh, d->kw, d->Cin, py.k0, py.kstep, py.nt, px.k0, px.kstep, px.nt);
        int rc = check_launch("pack_dgrad_weight");
        if (rc) return rc;
      }
      woff += total;
    }
  return EVK_OK;
}
