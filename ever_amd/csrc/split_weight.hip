// The weight planes of the split kernels from the OHWI parameter, one convolution at a time (the whole model in one launch:
// split_weight_multi.hip; the element-wise bodies: split_weight.hpp).  The planner's stage 1 (conv_route.hpp) names the
// layout: generic [3][rows][Kpad] for the implicit-GEMM and one-tap kernels (here), the halo and Winograd kernels' own orders
// (their files).
#include "conv_route.hpp"
#include "split_weight.hpp"

namespace evk {

// Weight planes for the split kernel.  Forward (`classes == nullptr` form): row co, k = (ky, kx, ci) as in
// the OHWI parameter.  out[pt][row][Kpad] bf16, zero padded along K.
__global__ void split_weight_fwd_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int rows, int K,
                                        int Kpad, const uint32_t* __restrict__ wscale) {
  split_fwd_body(w, out, rows, K, Kpad, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x,
                 wscale);
}

// Data-gradient planes of one residue class: row ci, k = (jy, jx, co) with ky = ky0 + jy*ksy, kx = kx0 + jx*ksx
// (the class-ordered layout of pack_dgrad_weight_kernel, produced straight from the OHWI parameter).
__global__ void split_weight_dgrad_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int Cout, int kh,
                                          int kw, int Cin, int ky0, int ksy, int nty, int kx0, int ksx, int ntx,
                                          int Kpad, const uint32_t* __restrict__ wscale) {
  split_dgrad_body(w, out, Cout, kh, kw, Cin, ky0, ksy, nty, kx0, ksx, ntx, Kpad,
                   (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, wscale);
}

}  // namespace evk

using namespace evk;

extern "C" size_t evk_conv2d_split_weight_bytes(const evk_conv_desc* d, int32_t for_dgrad) {
  if (!d) return 0;
  // (3x3: the LDS-halo kernel's layout pads the reduction channels to 16 per tap, the generic one the whole row to 32:
  // with channels % 16 != 0 the first can be the larger)
  auto k3 = [&](int K) { return d->kh == 3 && d->kw == 3 ? 9 * ((K + 15) / 16 * 16) : 0; };
  if (!for_dgrad) {
    const int kp = kpad32(d->kh * d->kw * d->Cin);
    return (size_t)3 * d->Cout * (kp > k3(d->Cin) ? kp : k3(d->Cin)) * sizeof(uint16_t);
  }
  if (d->stride_h == 1 && d->stride_w == 1 && d->kh == 3 && d->kw == 3) {
    const int kp = kpad32(9 * d->Cout);
    return (size_t)3 * d->Cin * (kp > k3(d->Cout) ? kp : k3(d->Cout)) * sizeof(uint16_t);
  }
  size_t total = 0;
  for (int cy = 0; cy < d->stride_h; ++cy)
    for (int cx = 0; cx < d->stride_w; ++cx) {
      const AxisPlan py = plan_axis(cy, d->pad_h, d->dil_h, d->stride_h, d->kh);
      const AxisPlan px = plan_axis(cx, d->pad_w, d->dil_w, d->stride_w, d->kw);
      total += (size_t)3 * d->Cin * kpad32(py.nt * px.nt * d->Cout) * sizeof(uint16_t);
    }
  return total;
}

// wscale == nullptr: the three bf16 planes; else the two fp16 planes of w / s(wscale) (planes 0 and 1 of the same layout)
static int split_weight_any(const evk_conv_desc* d, const float* w, int32_t for_dgrad, void* wsplit, const uint32_t* wscale,
                            void* stream) {
  EVK_REQUIRE(d && w && wsplit, EVK_E_INVALID, "split_weight: null pointer");
  EVK_REQUIRE(d->stride_h > 0 && d->stride_w > 0 && d->dil_h > 0 && d->dil_w > 0, EVK_E_INVALID,
              "split_weight: bad stride/dilation");
  hipStream_t st = (hipStream_t)stream;
  uint16_t* out = reinterpret_cast<uint16_t*>(wsplit);
  // the 3x3 kernels take their planes in their own order: the planner's stage 1 on the same geometry the consumer will build
  // (conv_route.hpp), so the two cannot disagree; never larger than the generic layout
  // (Winograd: 12 x 2 planes of taps, inside the 9 x 3 the buffer is sized for)
  const PlaneLayout layout = desc_layout(d, for_dgrad ? 1 : 0, wscale ? 2 : 3);
  if (layout == PlaneLayout::Wino) return launch_split_weight_wino(w, out, d->Cout, d->Cin, for_dgrad ? 1 : 0, st, wscale);
  if (layout == PlaneLayout::Halo) return launch_split_weight_halo(w, out, d->Cout, d->Cin, for_dgrad ? 1 : 0, st, wscale);
  if (!for_dgrad) {
    const int K = d->kh * d->kw * d->Cin, Kp = kpad32(K);
    const size_t total = (size_t)d->Cout * (Kp >> 1);
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(split_weight_fwd_kernel, dim3(blocks), dim3(256), 0, st, w, out, d->Cout, K, Kp, wscale);
    return check_launch("split_weight_fwd");
  }
  size_t off = 0;
  for (int cy = 0; cy < d->stride_h; ++cy)
    for (int cx = 0; cx < d->stride_w; ++cx) {
      const AxisPlan py = plan_axis(cy, d->pad_h, d->dil_h, d->stride_h, d->kh);
      const AxisPlan px = plan_axis(cx, d->pad_w, d->dil_w, d->stride_w, d->kw);
      const int K = py.nt * px.nt * d->Cout, Kp = kpad32(K);
      if (K > 0) {
        const size_t total = (size_t)d->Cin * (Kp >> 1);
        const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
        hipLaunchKernelGGL(split_weight_dgrad_kernel, dim3(blocks), dim3(256), 0, st, w, out + off, d->Cout, d->kh,
                           d->kw, d->Cin, py.k0, py.kstep, py.nt, px.k0, px.kstep, px.nt, Kp, wscale);
        int rc = check_launch("split_weight_dgrad");
        if (rc) return rc;
      }
      off += (size_t)3 * d->Cin * Kp;
    }
  return EVK_OK;
}

extern "C" int evk_conv2d_split_weight(const evk_conv_desc* d, const float* w, int32_t for_dgrad, void* wsplit,
                                       void* stream) {
  return split_weight_any(d, w, for_dgrad, wsplit, nullptr, stream);
}
extern "C" int evk_conv2d_split_weight_f16x2(const evk_conv_desc* d, const float* w, int32_t for_dgrad, void* wsplit,
                                             const uint32_t* w_absmax_bits, void* stream) {
  EVK_REQUIRE(w_absmax_bits, EVK_E_INVALID, "split_weight_f16x2: null scale");
  return split_weight_any(d, w, for_dgrad, wsplit, w_absmax_bits, stream);
}
