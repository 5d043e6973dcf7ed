// Host side of the weight-gradient family: arguments, plan, route and the launchers' prototypes (device pieces: wgrad_tile.hpp).
#pragma once
#include "common.hpp"

namespace evk {

struct WGradArgs {
  const float* x;
  const float* dy;
  float* out;  // dw (splitk==1) or workspace [splitk][Cout][Ktot]
  int N, H, W, Cin, Ho, Wo, Cout;
  int kh, kw, cpt;
  int sh, sw, ph, pw, dh, dw;
  int M, Ktot;
  int chunk;  // pixels per split (multiple of 32)
  int tiles_co, tiles_k, splitk;
  FastDiv fd_hw, fd_w;
  int planes;  // 3 (0 means 3): exact split, six products; 1: plain bf16 operands, one product (evk_conv2d_wgrad_bf16);
               // 2: 2-term fp16 split of scaled operands, three products (evk_conv2d_wgrad_f16x2)
  const uint32_t* x_scale;   // planes == 2: bit images of max|x| and max|dy| (evk_absmax)
  const uint32_t* dy_scale;
  int x_packed, dy_packed;   // planes == 2: the operand holds packed (h | l << 16) words of value / s (x3_common.hpp)
  int planar;                // planes == 2: BOTH operands are planar fp16 pairs (conv_wgrad_tr.hip)
  int reserved;  // (was: run-time ablation switches; they are compile-time now, EVK_WG_ABL)
};

constexpr int BKP = 32;  // pixels per step

struct WGradPlan {
  int bm, bn, tiles_co, tiles_k, splitk, chunk;
  int ws;  // 1: wave-specialised 128x256 kernel (conv_wgrad_x3ws.hip)
};
// x3 = 1: plan for the bf16-split kernel (different LDS footprint => different residency)
// tr = 1 / 2: the planar-operand kernel (conv_wgrad_tr.hip), one workgroup per CU: 128 x 256 tile / nine-tap form
// (128 output channels x 9 taps x 64 input channels per tile)
WGradPlan plan_wgrad(const evk_conv_desc* d, int x3, int planes = 3, int tr = 0, int shared = 0);

// Which instantiation a weight-gradient launch takes, decided ONCE (route_wgrad, conv_wgrad.hip): the launchers below switch
// on this value and evk_conv2d_wgrad_route prints it — there is no second copy of the decision.
enum class WGradKernel { Fp32, X3, X3Ws, Tr };
struct WGradRoute {
  WGradKernel kernel;
  int npx;            // operand form of the split kernels (NP / NPX): 1 bf16, 2 f16x2, 3 bf16x3, 4 f16x2 with a packed operand
  int w8, pkx, pkd;   // X3Ws: Wo % 8 == 0; x / dy arrive packed
  int nt;             // Tr: 1 (segments) or 9 (nine-tap halo form)
  WGradPlan plan;     // tile (bm x bn) and split
};
// planes: 0 the fp32 kernel, 1 bf16, 2 f16x2, 3 bf16x3; flags: EVK_CONV_{X,DY}_{PACKED,PLANAR}, EVK_CONV_WGRAD_SHARED.
// EVK_OK, or the error (with evk_last_error set) the launch entry points report for the same descriptor and flags.
int route_wgrad(const evk_conv_desc* d, int planes, uint32_t flags, WGradRoute* r);
void wgrad_kernel_name(const WGradRoute& r, char* buf, size_t n);
int launch_wgrad_f32(const WGradArgs& a, const WGradRoute& r, hipStream_t stream);
int launch_wgrad_x3(const WGradArgs& a, const WGradRoute& r, hipStream_t stream);
int launch_wgrad_x3ws(const WGradArgs& a, const WGradRoute& r, hipStream_t stream);
bool wgrad_tr_applicable(const evk_conv_desc* d, int planes);
bool wgrad_tr_nine_tap(const evk_conv_desc* d);
int launch_wgrad_tr(const WGradArgs& a, const WGradRoute& r, hipStream_t stream);

// every flag evk_conv2d_wgrad_f16x2_ex and evk_conv2d_wgrad_route know
constexpr uint32_t kWGradFlags = EVK_CONV_X_PACKED | EVK_CONV_DY_PACKED | EVK_CONV_X_PLANAR | EVK_CONV_DY_PLANAR | EVK_CONV_WGRAD_SHARED;

// column sums of a [rows][c] fp32 matrix (bias gradients; conv_wgrad.hip): also used by conv_transpose.hip
size_t colsum_workspace_bytes(int64_t rows, int c);
int launch_colsum(const float* src, float* out, int64_t rows, int c, float* workspace, hipStream_t st);

}  // namespace evk
