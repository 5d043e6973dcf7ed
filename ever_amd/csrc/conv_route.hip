// The planner of the forward / data-gradient convolutions (conv_route.hpp): switches, measured policy, forced routes.
#include "conv_route.hpp"
#include "x3_common.hpp"
#include <stdlib.h>
#include <string.h>

namespace evk {

static long long env_int(const char* name, long long dflt) {
  const char* v = getenv(name);
  return v ? atoll(v) : dflt;
}

RouteKnobs route_knobs() {
  static const RouteKnobs once = [] {
    RouteKnobs k{};
    k.wino = (int)env_int("EVK_WINO", 1);
    k.halo = (int)env_int("EVK_X3_HALO", 1);
    k.halo_min_wg = env_int("EVK_X3_HALO_MIN_WG", 256);
    k.c1_dma = (int)env_int("EVK_C1_DMA", 1);
    k.c1_ps2 = (int)env_int("EVK_C1_PS2", 1);
    k.c1_sp = (int)env_int("EVK_C1_SP", 1);
    k.x3_ws = (int)env_int("EVK_X3_WS", 1);
    return k;
  }();
  static const bool tune = getenv("EVK_TUNE") != nullptr;
  RouteKnobs k = once;
  if (tune) {   // tools/autotune_convs.py changes these between launches
    k.x3_force = getenv("EVK_X3_FORCE");
    k.halo_force = getenv("EVK_X3_HALO_FORCE");
  }
  return k;
}

int device_cus_per_xcd() {
  static int cus_of[64];   // per device id (one process may drive devices of different sizes)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev < 0 || dev >= 64) dev = 0;
  if (!cus_of[dev]) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    cus_of[dev] = prop.multiProcessorCount;
  }
  return cus_of[dev] / 8;
}

// ---- geometry ------------------------------------------------------------------------------------------------------
IGemmArgs igemm_geometry_fwd(const evk_conv_desc* d) {
  IGemmArgs a{};
  a.N = d->N; a.Hs = d->H; a.Ws = d->W; a.Cs = d->Cin;
  a.Hm = d->Ho; a.Wm = d->Wo; a.Cd = d->Cout;
  a.kh = d->kh; a.kw = d->kw; a.cpt = d->Cin / 4;
  a.ash = d->stride_h; a.asw = d->stride_w;
  a.oy0 = -d->pad_h; a.oys = d->dil_h; a.ox0 = -d->pad_w; a.oxs = d->dil_w;
  a.M = d->N * d->Ho * d->Wo;
  a.Ktot = d->kh * d->kw * d->Cin;
  a.Hd = d->Ho; a.Wd = d->Wo; a.dsh = 1; a.dsw = 1; a.dense_dst = 1;
  a.Kpad = kpad32(a.Ktot);
  return a;
}

IGemmArgs igemm_geometry_dgrad(const evk_conv_desc* d, int cy, int cx) {
  const int sh = d->stride_h, sw = d->stride_w;
  const AxisPlan py = plan_axis(cy, d->pad_h, d->dil_h, sh, d->kh);
  const AxisPlan px = plan_axis(cx, d->pad_w, d->dil_w, sw, d->kw);
  IGemmArgs a{};
  a.N = d->N; a.Hs = d->Ho; a.Ws = d->Wo; a.Cs = d->Cout;
  a.Hm = d->H > cy ? (d->H - cy + sh - 1) / sh : 0;
  a.Wm = d->W > cx ? (d->W - cx + sw - 1) / sw : 0;
  a.Cd = d->Cin;
  a.kh = py.nt; a.kw = px.nt; a.cpt = d->Cout / 4;
  a.ash = 1; a.asw = 1;
  a.oy0 = py.o0; a.oys = py.ostep; a.ox0 = px.o0; a.oxs = px.ostep;
  a.M = d->N * a.Hm * a.Wm;
  a.Ktot = py.nt * px.nt * d->Cout;
  a.Hd = d->H; a.Wd = d->W; a.dsh = sh; a.dsw = sw; a.doy = cy; a.dox = cx;
  a.dense_dst = (sh == 1 && sw == 1) ? 1 : 0;
  a.Kpad = kpad32(a.Ktot);
  return a;
}

// ---- stage 1: family of the 3x3 layers = layout of their weight planes -----------------------------------------------
constexpr int kPatchW = 16, kChunk = 16;   // both 3x3 kernels: patch width, reduction channels per chunk (asserted beside them)

static bool halo_wanted(const IGemmArgs& a, const RouteKnobs& k) {
  if (!k.halo || !conv3x3_halo_supports(a)) return false;
  // patches of 8 (or 16) x 16 output pixels; the last row / column of patches may hang over the edge of the map (the halo
  // loads zeros there, the epilogue drops those rows) as long as at least 3/4 of the patch grid is map
  // (round 4: H % 8 == 0 and W % 16 == 0 were required until then — a 616 x 344 scene, or the stride-4 map of a 416-wide
  // tile, fell back to the implicit-GEMM kernels)
  const long long cover = (long long)ceil_div(a.Hm, 8) * 8 * ceil_div(a.Wm, kPatchW) * kPatchW;
  if (a.Hm < 4 || a.Wm < 8 || 4LL * a.Hm * a.Wm < 3 * cover) return false;
  // (reduction channels: whole 16-channel chunks, or a partial last one as long as three quarters of the chunks' slots are
  // channels — Cin = 200 = 12.5 chunks)
  if (4 * a.Cs < 3 * ceil_div(a.Cs, kChunk) * kChunk || a.Cd < 64) return false;
  // enough workgroups for the 256 CUs, if necessary with the 64-wide N tile
  // (EVK_X3_HALO_MIN_WG=0 makes the choice independent of the batch size: tests/test_linearity_pinned_gpu.py pins the
  // accumulation order — chunk-major here, tap-major in the implicit-GEMM kernels — for a batch and its halves)
  const long long patches = (long long)a.N * ceil_div(a.Hm, 8) * ceil_div(a.Wm, kPatchW);
  return patches * ceil_div(a.Cd, 64) >= k.halo_min_wg;
}

static bool wino_wanted(const IGemmArgs& a, const RouteKnobs& k) {
  if (!k.wino || !conv3x3_wino_supports(a)) return false;
  if (a.Hm < 8 || a.Wm < 8 || a.Cd < 64) return false;
  if (4 * a.Cs < 3 * ceil_div(a.Cs, kChunk) * kChunk) return false;
  const long long cover = (long long)ceil_div(a.Hm, 16) * 16 * ceil_div(a.Wm, kPatchW) * kPatchW;
  if (4LL * a.Hm * a.Wm < 3 * cover) return false;
  if (k.wino >= 2) return true;
  // one 16 x 16 patch x 128 channels per workgroup: whole 128-wide column tiles and at least one workgroup per CU (measured,
  // tools/wino_probe.py, us direct -> this: 3x3x256 @128^2 926 -> 815 forward / 802 -> 707 data gradient, 256 -> 128 477 -> 430,
  // 256 @64^2 212 -> 190, 128 @64^2 57 -> 52; behind on 64 -> 64 @128^2 (half of the column tile is padding: 73 -> 103) and on
  // the 32^2 / 16^2 maps, which are not bound by the matrix pipe)
  return (a.Cd % 128) == 0 && (long long)a.N * ceil_div(a.Hm, 16) * ceil_div(a.Wm, kPatchW) * (a.Cd / 128) >= 256;
}

PlaneLayout route_layout(const IGemmArgs& a, const RouteKnobs& k) {
  if (!halo_wanted(a, k)) return PlaneLayout::Generic;
  // (the Winograd kernel only where the halo kernel applies as well: the producers of the other arithmetics lay those shapes
  // out for it, and a multi-tensor split job is built before the arithmetic is known)
  return wino_wanted(a, k) ? PlaneLayout::Wino : PlaneLayout::Halo;   // (f16x2 only: conv3x3_wino_supports)
}

// ---- forced routes (EVK_TUNE: tools/autotune_convs.py) ---------------------------------------------------------------
static const struct { const char* name; ConvRoute r; } kForced[] = {
    {"w256", {ConvKernel::X3Ws, PlaneLayout::Generic, 128, 256, 0, 0, 2}},
    {"w128", {ConvKernel::X3Ws, PlaneLayout::Generic, 128, 128, 0, 0, 2}},
    {"w64", {ConvKernel::X3Ws, PlaneLayout::Generic, 128, 64, 0, 0, 2}},
    {"d256", {ConvKernel::C1Dma, PlaneLayout::Generic, 128, 256, 0, 0, 3}},
    {"d128", {ConvKernel::C1Dma, PlaneLayout::Generic, 128, 128, 0, 0, 3}},
    {"d64", {ConvKernel::C1Dma, PlaneLayout::Generic, 128, 64, 0, 0, 3}},
    {"e128", {ConvKernel::C1Dma, PlaneLayout::Generic, 128, 128, 0, 0, 2}},
    {"e64", {ConvKernel::C1Dma, PlaneLayout::Generic, 128, 64, 0, 0, 2}},
    {"q128", {ConvKernel::C1Ps2, PlaneLayout::Generic, 128, 128, 0, 0, 3}},
    {"s128", {ConvKernel::C1Sp, PlaneLayout::Generic, 128, 128, 0, 0, 4}},
    {"s64", {ConvKernel::C1Sp, PlaneLayout::Generic, 128, 64, 0, 0, 4}},
    {"t128", {ConvKernel::C1Sp, PlaneLayout::Generic, 128, 128, 0, 0, 3}},
    {"t64", {ConvKernel::C1Sp, PlaneLayout::Generic, 128, 64, 0, 0, 3}},
    {"c128x128", {ConvKernel::X3, PlaneLayout::Generic, 128, 128, 0, 0, 1}},
    {"c64x128", {ConvKernel::X3, PlaneLayout::Generic, 64, 128, 0, 0, 1}},
    {"c128x64", {ConvKernel::X3, PlaneLayout::Generic, 128, 64, 0, 0, 1}},
    {"c64x64", {ConvKernel::X3, PlaneLayout::Generic, 64, 64, 0, 0, 1}},
    {"h64x8", {ConvKernel::Halo, PlaneLayout::Halo, 0, 64, 8, 4, 0}},
    {"m64x8", {ConvKernel::Halo, PlaneLayout::Halo, 0, 64, 8, 8, 0}},
    {"h64x16", {ConvKernel::Halo, PlaneLayout::Halo, 0, 64, 16, 4, 0}},
    {"m64x16", {ConvKernel::Halo, PlaneLayout::Halo, 0, 64, 16, 8, 0}},
    {"h128x8", {ConvKernel::Halo, PlaneLayout::Halo, 0, 128, 8, 4, 0}},
    {"h128x16", {ConvKernel::Halo, PlaneLayout::Halo, 0, 128, 16, 4, 0}},
    {"m128x8", {ConvKernel::Halo, PlaneLayout::Halo, 0, 128, 8, 8, 0}},
    {"m128x16", {ConvKernel::Halo, PlaneLayout::Halo, 0, 128, 16, 8, 0}},
};

static int ps2_tiles_n(const IGemmArgs& a) { return ceil_div(a.Cd, 128); }

// a forced route is taken when it names a kernel of this launch's plane layout that can run the shape; else the rules decide
static bool forced_route(const IGemmArgs& a, const char* name, PlaneLayout layout, int cus_per_xcd, ConvRoute& out) {
  if (!name || !*name) return false;
  for (const auto& f : kForced) {
    if (strcmp(f.name, name) != 0 || f.r.layout != layout) continue;
    ConvRoute r = f.r;
    switch (r.kernel) {
      case ConvKernel::C1Dma: if (!conv1x1_dma_supports(a)) return false; break;
      case ConvKernel::C1Sp: if (!conv1x1_sp_supports(a)) return false; break;
      case ConvKernel::C1Ps2: if (!conv1x1_ps2_supports(a) || ps2_tiles_n(a) > cus_per_xcd) return false; break;
      case ConvKernel::Halo:
        if (r.bn == 128 && a.Cd <= 64) return false;
        if (a.planes != 2) r.mw = 4;   // (the eight-matrix-wave form exists for the f16x2 arithmetic with DMA-fed weights)
        break;
      default: break;
    }
    out = r;
    return true;
  }
  return false;
}

// ---- stage 2: the tile inside the family ----------------------------------------------------------------------------
static ConvRoute route_fp32(const IGemmArgs& a) {
  if (conv1x1_smallm_supports(a)) return {ConvKernel::SmallM, PlaneLayout::Generic, 0, 0, 0, 0, 0};
  // Tile choice: N tile 64 for narrow outputs, else 128; M tile as large as keeps >= 2 workgroups per CU (256 CUs) in flight.
  const int bn = (a.Cd <= 64) ? 64 : 128;
  const long long tn = ceil_div(a.Cd, bn);
  auto tiles = [&](int bm) { return (long long)ceil_div(a.M, bm) * tn; };
  int bm = 64;
  if (bn == 64 && tiles(256) >= 512) bm = 256;
  else if (tiles(128) >= 512) bm = 128;
  return {ConvKernel::Igemm, PlaneLayout::Generic, bm, bn, 0, 0, 2};
}

static ConvRoute route_halo(const IGemmArgs& a) {
  // workgroup counts from which the 128-wide tile / the 16-row patch is taken (swept in the step in round 5, where the chip is
  // shared with the side stream: 128 / 384 / 768 all within 0.1 % of 256)
  constexpr long long min128 = 256, mintall = 256;
  if (a.Cd <= 64 || (long long)a.N * ceil_div(a.Hm, 8) * ceil_div(a.Wm, kPatchW) * ceil_div(a.Cd, 128) < min128)
    return {ConvKernel::Halo, PlaneLayout::Halo, 0, 64, 8, 4, 0};   // small maps (16^2 .. 32^2): 64-wide tiles keep every CU busy
  // 16 x 16 patches (256 GEMM rows) halve the weight bytes per MFMA, the larger share of the staging traffic now;
  // taken when they still fill the chip.  With the weights fed by DMA (f16x2) the staging waves no longer hold the matrix
  // waves back, and eight matrix waves (two per SIMD) are 1-7 % ahead of four on every 128-wide shape
  // (tools/autotune_convs.py: 777 -> 763 us on 3x3x256 @128^2, 61 -> 57 on 3x3x128 @64^2, 59-62 -> 58 on 3x3x256 @32^2).
  const int mw = a.planes == 2 ? 8 : 4;
  // (16-row patches unless they would add a mostly empty last patch row: H % 16 in 1..8 is served better by 8-row patches)
  const bool tall_fits = (a.Hm % 16) == 0 || (a.Hm % 16) > 8;
  const bool tall = tall_fits && (long long)a.N * ceil_div(a.Hm, 16) * ceil_div(a.Wm, kPatchW) * ceil_div(a.Cd, 128) >= mintall;
  return {ConvKernel::Halo, PlaneLayout::Halo, 0, 128, tall ? 16 : 8, mw, 0};
}

// the one-tap layers of the f16x2 arithmetic, both operands by LDS-DMA; false: the register-staged kernels take the launch
static bool route_one_tap(const IGemmArgs& a, const RouteKnobs& k, int cus_per_xcd, ConvRoute& out) {
  if (k.c1_dma == 0 || !conv1x1_dma_supports(a)) return false;
  auto dma = [](int bn, int stages) { return ConvRoute{ConvKernel::C1Dma, PlaneLayout::Generic, 128, bn, 0, 0, stages}; };
  // The three-role persistent form (conv1x1_ps2.hip: loader / compute / store waves, software-pipelined K step) takes the
  // 128^2-map layers and the short-reduction layers of the 64^2 maps (round 4's two-role persistent kernel, conv1x1_ps.hip,
  // which it superseded on every shape, was deleted in round 6) — measured (tools/ab_c1sp.py, us, best other
  // form -> this): 64 -> 256 @128^2 93 -> 78, 256 -> 256 173 -> 152, 256 -> 128 98 -> 83, 128 -> 512 @64^2 52 -> 46; level on
  // the longer reductions of the 64^2 / 32^2 maps, behind on 2048 -> 512 @16^2 (one tile per workgroup: nothing to overlap).
  if (k.c1_ps2 != 0 && conv1x1_ps2_supports(a) && a.Cd >= 128) {
    const int tm = ceil_div(a.M, 128), nk = a.Kpad / BK3;
    // (more column tiles than the device has CUs per XCD: the persistent grid cannot hold them — the non-persistent forms go on)
    if ((k.c1_ps2 == 2 || tm >= 1024 || (tm >= 512 && nk <= 4)) && ps2_tiles_n(a) <= cus_per_xcd) {
      out = {ConvKernel::C1Ps2, PlaneLayout::Generic, 128, 128, 0, 0, 3};
      return true;
    }
  }
  // two stages: two workgroups per CU (one's epilogue under the other's loop)
  if (k.c1_dma == 2) { out = dma(a.Cd >= 128 ? 128 : 64, 2); return true; }
  // Measured on the FarSeg-R50 one-tap shapes, fp32 and packed operands, with and without the statistics epilogue
  // (tools/ab_c1dma.py, us, register-staged default -> this kernel): the two-stage ring with TWO workgroups per CU (one's
  // store burst under the other's loop) is ahead of the three-stage ring at one workgroup per CU and of the default wherever
  // the output is at least 128 channels wide: 256->256 @128^2 225-244 -> 178-185, 256->128 115-136 -> 104-107, 128->512 @64^2
  // 62-69 -> 56-60, 512->128 41-50 -> 38-40, 512->256 75-86 -> 70-77, 1024->256 @32^2 36-42 -> 35-39, level on 64->256
  // (108-138 -> 108-113), 256->1024 and 512->2048; 64-wide outputs stay on the default (256->64: 66-76 vs 72-78).
  // 16^2 maps: 64-wide column tiles where 128-wide ones leave CUs without a workgroup (2048->512: 47-55 -> 41-50).
  // (four-wave forms, 2 x 2 waves of 64 x BN/2 — a third fewer LDS bytes per MFMA — measured behind the eight-wave ones on
  // every shape: 182-190 vs 178-180 us on 256->256 @128^2; conv1x1_dma.hip: launch_c1_pk<BN, NST, 2> to try them again)
  if (a.Cd < 128) return false;
  const long long tm = ceil_div(a.M, 128);
  // (below how many 128-wide tiles the 64-wide ones are taken: swept in the step in round 5, where the chip is shared with the
  // side stream — 128 / 320 / 640 / 1100 all behind or level with 224)
  constexpr long long fill_wg = 224;
  if (tm * ceil_div(a.Cd, 128) >= fill_wg) { out = dma(128, 2); return true; }
  if (tm * ceil_div(a.Cd, 64) < fill_wg) return false;   // cannot fill the chip
  // long reductions on the 16^2 maps (2048 -> 512: 64 steps, one 128 x 64 tile per CU): the software-pipelined form with
  // loader waves (conv1x1_sp.hip, ring of four) — 42.9 -> 32.8 us, 43.3 -> 33.6 with the statistics epilogue (tools/ab_c1sp.py)
  if (k.c1_sp && a.Kpad / BK3 >= 32 && conv1x1_sp_supports(a)) out = {ConvKernel::C1Sp, PlaneLayout::Generic, 128, 64, 0, 0, 4};
  else out = dma(64, 2);
  return true;
}

// the wave-specialised form for the large layers; false: the single-role kernel takes the launch
static bool route_ws(const IGemmArgs& a, const RouteKnobs& k, ConvRoute& out) {
  const int mode = k.x3_ws;
  if (mode == 0) return false;
  auto ws = [](int bn) { return ConvRoute{ConvKernel::X3Ws, PlaneLayout::Generic, 128, bn, 0, 0, 2}; };
  const int bn = (a.Cd <= 64) ? 64 : 128;
  const long long tm = ceil_div(a.M, 128);
  const long long t128 = tm * ceil_div(a.Cd, bn);
  if (t128 < 256) {
    // 16^2 maps with wide outputs and a long reduction (stage-4 layers: 512->512 3x3, 2048<->512 1x1; M = 4096 rows):
    // 128 x 64 tiles still give every CU a workgroup, and the two-role form beats 64-row single-role tiles there
    // (tools/autotune_convs.py, same process: 64-65 vs 71-83 us on the 1x1 layers, 138 vs 152 us on the strided 3x3)
    if (a.Kpad >= 1024 && a.Cd >= 128 && tm * ceil_div(a.Cd, 64) >= 256) { out = ws(64); return true; }
    return false;  // cannot fill the chip at one workgroup per CU
  }
  // One 8-wave workgroup per CU: nothing overlaps a tile's prologue / epilogue, so short reductions
  // (1x1 convolutions, K <= 512: 2..16 steps) run better as 2-3 single-role workgroups per CU, unless the
  // grid is below two per CU anyway.  Measured on the FarSeg-R50 layer set (tools/bench_conv_x3.py).
  // Persistent workgroups recover part of that (64->256 @128^2: 121 -> 111 us, 256->256: 267 -> 251, 512->256 @64^2:
  // 106 -> 99; tools/ab_conv1x1.py) except for 64-wide outputs (256->64 @128^2: 80 -> 95 us).
  // An accumulate / residual epilogue (one more load per store, in the matrix waves) turns the gain into a loss:
  // folded-BatchNorm inference 1370 -> 1325 tiles/s.
  if (mode == 1 && a.Kpad < 1024 && t128 >= 512 && (a.Cd < 128 || a.accum)) return false;
  // with the statistics epilogue the workgroups are not persistent: on the 128^2 maps (>= 2048 tiles, K <= 256) the
  // single-role kernel is ahead again (64->256: 129 -> 117 us, 256->128: 158 -> 140), on the smaller maps it is not
  if (mode == 1 && a.bn_want && a.Kpad < 1024 && tm * ceil_div(a.Cd, a.Cd >= 256 ? 256 : 128) >= 2048) return false;
  // 128x256 tiles where the output is wide enough: the activation split (VALU) and the L2 -> CU bytes per MFMA
  // drop by half / a fifth
  out = ws(a.Cd >= 256 && tm * ceil_div(a.Cd, 256) >= 256 ? 256 : bn);
  return true;
}

static ConvRoute route_single(const IGemmArgs& a) {
  const int bn = (a.Cd <= 64) ? 64 : 128;
  const long long tn = ceil_div(a.Cd, bn);
  auto tiles = [&](int bm) { return (long long)ceil_div(a.M, bm) * tn; };
  // single LDS stage (48 KB at 128x128 => 2-3 workgroups per CU, whose split / MFMA phases interleave)
  // measured faster than a double-buffered stage at 1 workgroup per CU: 180 vs 157 TFLOP/s on 3x3x256 @128^2
  if (tiles(128) >= 256) return {ConvKernel::X3, PlaneLayout::Generic, 128, bn, 0, 0, 1};
  if (bn == 128 && tiles(64) >= 256) return {ConvKernel::X3, PlaneLayout::Generic, 64, 128, 0, 0, 1};
  // 16^2 maps (M = 4096 rows at batch 16): 64 x 64 tiles are the only ones that give every CU a workgroup
  return {ConvKernel::X3, PlaneLayout::Generic, 64, 64, 0, 0, 1};
}

ConvRoute route_conv(const IGemmArgs& a, bool split, const RouteKnobs& k, int cus_per_xcd) {
  if (!split) return route_fp32(a);
  ConvRoute r{};
  const PlaneLayout layout = route_layout(a, k);
  if (layout == PlaneLayout::Wino) return {ConvKernel::Wino, PlaneLayout::Wino, 0, 128, 16, 8, 0};
  if (layout == PlaneLayout::Halo) return forced_route(a, k.halo_force, layout, cus_per_xcd, r) ? r : route_halo(a);
  if (!igemm_x3_supports(a)) return route_single(a);   // (the launcher reports what the kernels cannot take)
  if (forced_route(a, k.x3_force, layout, cus_per_xcd, r)) return r;
  if (route_one_tap(a, k, cus_per_xcd, r) || route_ws(a, k, r)) return r;
  return route_single(a);
}

// ---- the route as a kernel trace spells it --------------------------------------------------------------------------
void route_kernel_name(const IGemmArgs& a, const ConvRoute& r, char* buf, size_t n) {
  const char* pk = a.a_packed ? "true" : "false";
  const int np = x3_npx(a);   // what the launchers dispatch on (pick_npx)
  switch (r.kernel) {
    case ConvKernel::Igemm:
      snprintf(buf, n, "conv_igemm_kernel<%d, %d, %d, %d>", r.bm, r.bn, r.bm == 256 ? 4 : 2, r.bm == 256 ? 1 : 2);
      break;
    case ConvKernel::SmallM: snprintf(buf, n, "conv1x1_smallm_kernel"); break;
    case ConvKernel::Wino: snprintf(buf, n, "conv3x3_wino_x3_kernel<%d, %d, %s>", r.bn, r.ph, pk); break;
    case ConvKernel::Halo:
      snprintf(buf, n, "conv3x3_halo_x3_kernel<%d, %d, %d, %s, %d>", r.bn, r.ph, np, a.planes == 2 ? "true" : "false", r.mw);
      break;
    case ConvKernel::C1Ps2:   // <packed, statistics, non-temporal activation loads>
      snprintf(buf, n, "conv1x1_ps2_kernel<%s, %s, %s>", pk, a.bn_want ? "true" : "false", ps2_tiles_n(a) <= 2 ? "true" : "false");
      break;
    case ConvKernel::C1Dma: snprintf(buf, n, "conv1x1_dma_kernel<%d, %s, %d, 4>", r.bn, pk, r.stages); break;
    case ConvKernel::C1Sp: snprintf(buf, n, "conv1x1_sp_kernel<%d, %s, %d, 4>", r.bn, pk, r.stages); break;
    case ConvKernel::X3Ws: snprintf(buf, n, "conv_igemm_x3ws_kernel<%d, %d, 2, 2, %d, %d>", r.bm, r.bn, r.stages, np); break;
    case ConvKernel::X3: snprintf(buf, n, "conv_igemm_x3_kernel<%d, %d, 2, 2, %d, %d>", r.bm, r.bn, r.stages, np); break;
  }
}

}  // namespace evk

using namespace evk;

extern "C" int evk_conv2d_route(const evk_conv_desc* d, int32_t cls, int32_t planes, uint32_t flags, int32_t with_accum,
                                int32_t with_stats, int32_t cus_per_xcd, char* buf, size_t buf_bytes, int32_t* layout) {
  EVK_REQUIRE(d && buf && buf_bytes > 0, EVK_E_INVALID, "conv2d_route: null pointer");
  EVK_REQUIRE(d->stride_h > 0 && d->stride_w > 0 && d->dil_h > 0 && d->dil_w > 0 && d->Cin > 0 && d->Cout > 0, EVK_E_INVALID,
              "conv2d_route: bad descriptor");
  EVK_REQUIRE(planes >= 0 && planes <= 3 && cls < d->stride_h * d->stride_w, EVK_E_INVALID, "conv2d_route: bad planes / class");
  IGemmArgs a = cls < 0 ? igemm_geometry_fwd(d) : igemm_geometry_dgrad(d, cls / d->stride_w, cls % d->stride_w);
  buf[0] = 0;
  if (layout) *layout = 0;
  if (a.kh * a.kw == 0 || a.Hm * a.Wm == 0) return EVK_OK;   // a residue class without a launch
  a.planes = planes;
  a.a_packed = (planes == 2 && (flags & (cls < 0 ? EVK_CONV_X_PACKED : EVK_CONV_DY_PACKED))) ? 1 : 0;
  a.accum = with_accum ? reinterpret_cast<const float*>(d) : nullptr;   // (the planner asks whether there is one, no more)
  a.bn_want = (with_stats && cls < 0 && planes && d->Cout % 4 == 0) ? 1 : 0;
  const ConvRoute r = route_conv(a, planes != 0, route_knobs(), cus_per_xcd);
  route_kernel_name(a, r, buf, buf_bytes);
  if (layout) *layout = (int32_t)r.layout;
  return EVK_OK;
}
