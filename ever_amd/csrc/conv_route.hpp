// Which kernel and tile a forward / data-gradient convolution launch takes: ONE planner for the launchers
// (conv_igemm.hip: conv_fwd_any / conv_dgrad_any) and for the weight-plane producers (evk_conv2d_split_weight*,
// evk_conv2d_split_jobs), which must lay the planes out for the kernel that will read them.  Host code only.
//
// Split of responsibilities: a kernel's HARD preconditions depend on constants that live beside the kernel — each kernel
// file keeps one `bool <kernel>_supports(const IGemmArgs&)` (no environment, no measured threshold).  Everything measured or
// switchable is here (conv_route.hip), with the measurements that justify each threshold.
//
// Two stages, because the producers know less than the launchers:
//   stage 1, route_layout: kernel family of the 3x3 layers = layout of the weight planes.  A function of what an
//     evk_conv_desc, the direction (forward, or residue class of the data gradient) and the arithmetic determine — the
//     geometry fields of IGemmArgs (igemm_geometry_fwd / _dgrad), its `planes`, the switches.  It does NOT look at accum,
//     a_packed, bn_want or the device: the planes are produced once per optimiser step, before any of those is known.  A
//     multi-tensor split job is even built before the arithmetic is known: its arg[3] carries "Winograd layout if f16x2",
//     which is why the Winograd kernel is only taken where the halo kernel would be (the layout under planes = 2 is
//     Generic exactly where the layout under planes = 3 is).
//   stage 2, route_conv: the tile inside the family, from the run-time fields as well (accum, a_packed, bn_want, the
//     device's CUs per XCD).
#pragma once
#include "igemm_common.hpp"

namespace evk {

enum class ConvKernel {
  Igemm,    // conv_igemm_f32.hip: fp32 implicit GEMM
  SmallM,   // conv_igemm_f32.hip: conv1x1_smallm (1x1 on a handful of rows)
  Wino,     // conv3x3_wino_x3.hip
  Halo,     // conv3x3_halo_x3.hip
  C1Ps2,    // conv1x1_ps2.hip
  C1Dma,    // conv1x1_dma.hip
  C1Sp,     // conv1x1_sp.hip
  X3Ws,     // conv_igemm_x3ws.hip
  X3,       // conv_igemm_x3.hip (single role)
};
enum class PlaneLayout { Generic, Halo, Wino };   // [3][rows][Kpad] | 9 taps, chunked | 12 transformed taps, chunked

struct ConvRoute {
  ConvKernel kernel;
  PlaneLayout layout;
  int bm, bn;    // tile: GEMM rows (Igemm, X3, X3Ws; 128 in the one-tap kernels) x output channels
  int ph;        // Halo, Wino: patch height (the patch is ph x 16 output pixels)
  int mw;        // Halo: matrix waves (8 exists in the f16x2 arithmetic only)
  int stages;    // ring stages: C1Dma 2 | 3, C1Sp 3 | 4
};

// The routing switches, read from the environment once per process (DESIGN.md §6b has the table).  Under EVK_TUNE
// (tools/autotune_convs.py) the two force strings are re-read on every call.
struct RouteKnobs {
  int wino;               // EVK_WINO: 0 never, 1 (default) where measured ahead, 2 wherever it applies (tests)
  int halo;               // EVK_X3_HALO: 0 = the implicit-GEMM kernels take every 3x3 layer
  long long halo_min_wg;  // EVK_X3_HALO_MIN_WG (256): grid below which the halo kernel leaves a launch to the implicit GEMM
  int c1_dma;             // EVK_C1_DMA: 0 never, 1 (default) where measured faster, 2 wherever the shape allows
  int c1_ps2;             // EVK_C1_PS2: 0 never, 1 (default) by the measured rule, 2 wherever it applies (tests)
  int c1_sp;              // EVK_C1_SP: 0 never, 1 (default) long reductions of the 16^2 maps
  int x3_ws;              // EVK_X3_WS: 0 never, 1 (default) where measured faster, 2 wherever the tile shapes allow
  const char* x3_force;   // EVK_TUNE only: EVK_X3_FORCE / EVK_X3_HALO_FORCE name a row of the forced-route table
  const char* halo_force;
};
RouteKnobs route_knobs();

PlaneLayout route_layout(const IGemmArgs& a, const RouteKnobs& k);
// split: the split arithmetics (weight planes) rather than the fp32 kernels.  cus_per_xcd: of the device that will run it
// (conv1x1_ps2 is persistent: its column tiles must fit one XCD's CUs; no other route depends on the device, so a launcher
// may route with kAnyDevice first and ask the device only when the answer is that kernel)
constexpr int kAnyDevice = 1 << 30;
ConvRoute route_conv(const IGemmArgs& a, bool split, const RouteKnobs& k, int cus_per_xcd);
int device_cus_per_xcd();   // of the current device (queried once per device); <= 0: the query failed
// "kernel<template arguments>" of the instantiation the launcher takes for this route, as a kernel trace spells it
void route_kernel_name(const IGemmArgs& a, const ConvRoute& r, char* buf, size_t n);

// The geometry part of IGemmArgs from a descriptor (everything but pointers, epilogue and arithmetic).  Data gradient: one
// launch per residue class (cy, cx) of the input pixel mod stride; kh * kw == 0 or Hm * Wm == 0: the class has no launch.
IGemmArgs igemm_geometry_fwd(const evk_conv_desc* d);
IGemmArgs igemm_geometry_dgrad(const evk_conv_desc* d, int cy, int cx);
// layout of the planes evk_conv2d_split_weight(d, for_dgrad) produces under `planes` (a strided data gradient is one
// generic block per residue class: every class declines the 3x3 kernels)
inline PlaneLayout desc_layout(const evk_conv_desc* d, int for_dgrad, int planes) {
  IGemmArgs a = for_dgrad ? igemm_geometry_dgrad(d, 0, 0) : igemm_geometry_fwd(d);
  a.planes = planes;
  return route_layout(a, route_knobs());
}

// Operand form of the split kernels' NP / NPX template parameter (x3_common.hpp: X3Mode): 1 bf16, 2 f16x2, 4 f16x2 with
// packed activations, 3 bf16x3.  ONE mapping for the launchers (pick_npx) and for route_kernel_name.
inline int x3_npx(const IGemmArgs& a) { return a.planes == 1 ? 1 : a.planes == 2 ? (a.a_packed ? 4 : 2) : 3; }
template <typename F>
inline int pick_npx(const IGemmArgs& a, F&& f) {   // f(std::integral_constant<int, NPX>)
  return pick<1, 2, 4, 3>(x3_npx(a), f);
}

// launchers: tiles_m/n, statistics setup, LDS size and grid of the instantiation the route names.  A route the kernel
// cannot take is an internal error.
int launch_igemm(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_conv1x1_smallm(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_conv3x3_wino(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_conv3x3_halo(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_conv1x1_ps2(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_conv1x1_dma(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_conv1x1_sp(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_igemm_x3ws(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);
int launch_igemm_x3(IGemmArgs& a, const ConvRoute& r, hipStream_t stream);

bool conv1x1_smallm_supports(const IGemmArgs& a);
bool conv3x3_wino_supports(const IGemmArgs& a);
bool conv3x3_halo_supports(const IGemmArgs& a);
bool conv1x1_ps2_supports(const IGemmArgs& a);
bool conv1x1_dma_supports(const IGemmArgs& a);
bool conv1x1_sp_supports(const IGemmArgs& a);
bool igemm_x3_supports(const IGemmArgs& a);   // X3 and X3Ws (and the precondition of the one-tap kernels' planes)

}  // namespace evk
