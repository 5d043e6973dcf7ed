// What the weight-gradient family shares on the host, and the small kernels that finish its work:
//
//   dw[co][k] = sum_m dy[m][co] * im2col(x)[m][k]        m = (n, oy, ox),  k = (ky, kx, ci)
//
//   plan_wgrad / route_wgrad   tile, pixel split and THE decision which kernel a launch takes:
//                              conv_wgrad_f32.hip (fp32 MFMA), conv_wgrad_x3.hip / conv_wgrad_x3ws.hip (split operands, staged
//                              through registers), conv_wgrad_tr.hip (planar f16x2 operands by LDS DMA)
//   wgrad_kernel_name          the route as a kernel trace spells it (evk_conv2d_wgrad_route)
//   splitk_reduce              sums the splits' partial tiles in a fixed order
//   colsum_partial / _final    column sums of dy: the bias gradient (also conv_transpose.hip's)
//   conv_wgrad_any             arguments, launch, reduce, bias gradient; the extern "C" entry points
// The device pieces the kernels share are in wgrad_tile.hpp.
#include "wgrad_common.hpp"
#include <stdlib.h>

namespace evk {

#ifndef EVK_SK_NT
#define EVK_SK_NT 1   // (528.2 -> 528.6 tiles/s over three interleaved rounds: inside the noise, kept as the right hint)
#endif
#if EVK_SK_NT
#define SK_LD(p) __builtin_nontemporal_load(p)   // the partials' last reader
#else
#define SK_LD(p) (*(p))
#endif
// out[i] = sum_z ws[z][i]  (fixed order)
// `lanes` threads share one 16-byte element: lane l sums the splits z = l, l + lanes, ... (fixed order), the lanes are
// folded through LDS in index order => the result depends on (splitk, lanes) only, never on timing.  With one thread
// per element a small weight tensor with many splits (1x1 convolutions on 128^2 maps: 4096 floats x 1024 splits) ran on
// four workgroups and took 78 us — three times the weight-gradient kernel it follows.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, size_t n4,
                                                            int splitk, size_t stride4, int lanes) {
  __shared__ f32x4 red[256];
  const f32x4* w4 = reinterpret_cast<const f32x4*>(ws);
  f32x4* o4 = reinterpret_cast<f32x4*>(out);
  const int epb = 256 / lanes;                     // elements per workgroup
  const int e = threadIdx.x % epb, l = threadIdx.x / epb;
  for (size_t i0 = (size_t)blockIdx.x * epb; i0 < n4; i0 += (size_t)gridDim.x * epb) {
    const size_t i = i0 + e;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < n4) {
      int z = l;
      for (; z + 3 * lanes < splitk; z += 4 * lanes) {  // four independent 16-byte loads in flight
        const f32x4 a = SK_LD(w4 + (size_t)z * stride4 + i), b = SK_LD(w4 + (size_t)(z + lanes) * stride4 + i);
        const f32x4 c = SK_LD(w4 + (size_t)(z + 2 * lanes) * stride4 + i), d = SK_LD(w4 + (size_t)(z + 3 * lanes) * stride4 + i);
        s += (a + b) + (c + d);
      }
      for (; z < splitk; z += lanes) s += SK_LD(w4 + (size_t)z * stride4 + i);
    }
    if (lanes > 1) {
      red[threadIdx.x] = s;
      __syncthreads();
      if (l == 0 && i < n4) {
        for (int k = 1; k < lanes; ++k) s += red[k * epb + e];
        o4[i] = s;
      }
      __syncthreads();
    } else if (i < n4) {
      o4[i] = s;
    }
  }
}

// Column sums of a [rows][C] matrix: stage 1 -> partial[blk][C], stage 2 -> out[C].  C % 4 == 0.
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ src, float* __restrict__ partial,
                                                             int64_t rows, int C, int64_t rows_per_blk) {
  __shared__ f32x4 red[256];
  const int c4 = C >> 2;
  const int tpc = min(c4, 256);       // threads across channels
  const int rl = 256 / tpc;           // row lanes
  const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  const int64_t r1 = min(rows, r0 + rows_per_blk);
  for (int cb = tc; cb < c4; cb += tpc) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (tr < rl)
      for (int64_t r = r0 + tr; r < r1; r += rl) s += *reinterpret_cast<const f32x4*>(src + r * C + cb * 4);
    red[threadIdx.x] = s;
    __syncthreads();
    if (tr == 0) {
      for (int k = 1; k < rl; ++k) s += red[k * tpc + tc];
      *reinterpret_cast<f32x4*>(partial + (size_t)blockIdx.x * C + cb * 4) = s;
    }
    __syncthreads();
  }
}
// 32 channels x 8 partial-lanes per workgroup: coalesced 128-byte rows, fp64, LDS fold
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                           int nblk, int C) {
  // 8 channels x 32 partial-lanes per workgroup, four loads in flight per lane (as the BatchNorm finalisation)
  __shared__ double red[32][8];
  const int tc = threadIdx.x & 7, tl = threadIdx.x >> 3;
  const int c = xcd_remap((int)blockIdx.x, (int)gridDim.x) * 8 + tc;   // (neighbouring channel groups on ONE XCD: bn_common.hpp, bn_fin_group)
  double s = 0.0;
  if (c < C) {
    int b = tl;
    for (; b + 96 < nblk; b += 128) {
      const float a0 = partial[(size_t)b * C + c], a1 = partial[(size_t)(b + 32) * C + c];
      const float a2 = partial[(size_t)(b + 64) * C + c], a3 = partial[(size_t)(b + 96) * C + c];
      s += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
    }
    for (; b < nblk; b += 32) s += (double)partial[(size_t)b * C + c];
  }
  red[tl][tc] = s;
  __syncthreads();
  if (tl == 0 && c < C) {
    for (int k = 1; k < 32; ++k) s += red[k][tc];
    out[c] = (float)s;
  }
}

WGradPlan plan_wgrad(const evk_conv_desc* d, int x3, int planes, int tr, int shared) {
  WGradPlan pl;
  const int Ktot = d->kh * d->kw * d->Cin;
  const int M = d->N * d->Ho * d->Wo;
  pl.bm = d->Cout <= 64 ? 64 : 128;
  pl.bn = Ktot <= 64 ? 64 : 128;
  // wide wave-specialised tile (128 x 256, one 8-wave workgroup per CU) when both dimensions are there
  // (planner constants; ONLY under EVK_TUNE=1 — the survey tool tools/autotune_wgrad.py — are they read from the environment,
  // on every call, and clamped to values the plan below can divide by)
  static const bool tune = getenv("EVK_TUNE") != nullptr;
  auto knob = [&](const char* name, int dflt, int lo) {
    const char* v = tune ? getenv(name) : nullptr;
    const int k = (v && *v) ? atoi(v) : dflt;
    return k < lo ? lo : k;
  };
  const int ws_mode = knob("EVK_WG_WS", 1, 0);
  // (its gathers are raw buffer loads: 32-bit byte offsets, so both tensors must stay below 2 GiB)
  const bool fits32 = (long long)d->N * d->H * d->W * d->Cin * 4 < 0x7fffffffLL &&
                      (long long)d->N * d->Ho * d->Wo * d->Cout * 4 < 0x7fffffffLL;
  // (Cout below 128 leaves rows of the 128-row tile empty: 96 / 64 measured level on C5)
  const int ws_min = knob("EVK_WG_WS_MINCOUT", 128, 1);
  pl.ws = (x3 && ws_mode && d->Cout >= ws_min && Ktot >= 256 && fits32) ? 1 : 0;
  if (tr) { pl.ws = 1; pl.bm = 128; }
  if (pl.ws) pl.bn = 256;
  if (tr == 2) pl.bn = 9 * 64;   // nine taps x 64 input channels per tile (tiles_k = Cin / 64 below)
  pl.tiles_co = ceil_div(d->Cout, pl.bm);
  pl.tiles_k = tr == 2 ? d->Cin / 64 : ceil_div(Ktot, pl.bn);
  const int tiles = pl.tiles_co * pl.tiles_k;
  // Split the pixel reduction so that the grid fills WHOLE rounds of the machine: slots = 256 CUs x
  // resident workgroups per CU (LDS-limited: 64 KB tiles -> 2, 48 KB -> 3, 32 KB -> 4).  A grid of
  // 2.04 rounds costs 3 (measured: 1044 workgroups on 512 slots ran at 63 % MFMA utilisation).
  const int rounds = knob("EVK_WG_ROUNDS", 1, 1), min_chunk = knob("EVK_WG_MINCHUNK", 256, 32);
  const int lds_kb = 2 * BKP * (pl.bm + pl.bn) * 4 / 1024;
  // split kernel: single-buffered 3-plane bf16 stage (48 KB at 128x128), residency set by its VGPRs
  const int per_cu = pl.ws ? 1 : x3 ? (pl.bm + pl.bn >= 256 ? 3 : 4)
                        : (lds_kb >= 64 ? 2 : (lds_kb >= 48 ? 3 : 4));
  // A wide-tile kernel (one 8-wave workgroup per CU, up to 700 us long) that runs BESIDE the backward chain — the caller says
  // so with EVK_CONV_WGRAD_SHARED — is split for HALF of the CUs: sixteen workgroups per XCD, the other sixteen CUs of every XCD
  // stay with the main stream's kernels instead of queueing behind it.  Round 5, three interleaved rounds per box, tiles/s:
  // 100 % 545.9 / 541.8 / 560.0, 75 % 564.7, 62 % 545.6, 56 % 544.6, 50 % 557.4 / 552.2 / 565.9 (+1.1 .. +2.1 %), 44 % 545.8,
  // 37 % 531.2, 25 % 469.7; the nine-tap planar kernel alone at 50 %: +1.1 %, the x3ws kernels alone: +0.3 %; the 128 x 128
  // single-role tiles (3-4 workgroups per CU) do not care (percent; 100 = as if alone).
  const int fill = (shared && pl.ws) ? knob("EVK_WG_SHARED_FILL", 50, 1) : 100;
  const int slots = 256 * per_cu * (fill > 0 && fill <= 100 ? fill : 100) / 100;
  int maxsplit = ceil_div(M, min_chunk);  // at least min_chunk pixels per split
  int sk = (rounds * slots) / tiles;      // floor: never spill into an extra, nearly empty round
  if (sk > maxsplit) sk = maxsplit;
  if (sk < 1) sk = 1;
  int chunk = ceil_div(M, sk);
  chunk = ((chunk + BKP - 1) / BKP) * BKP;
  pl.chunk = chunk;
  pl.splitk = ceil_div(M, chunk);
  return pl;
}
static int colsum_blocks(int64_t rows) {
  int64_t b = (rows + 255) / 256;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

size_t colsum_workspace_bytes(int64_t rows, int c) { return (size_t)colsum_blocks(rows) * c * sizeof(float) + 256; }
int launch_colsum(const float* src, float* out, int64_t rows, int c, float* workspace, hipStream_t st) {
  const int nblk = colsum_blocks(rows);
  const int64_t rpb = (rows + nblk - 1) / nblk;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(256), 0, st, src, workspace, rows, c, rpb);
  int rc = check_launch("colsum_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(colsum_final_kernel, dim3((c + 7) / 8), dim3(256), 0, st, (const float*)workspace, out, nblk, c);
  return check_launch("colsum_final");
}

}  // namespace evk

using namespace evk;

static size_t wgrad_ws_bytes(const evk_conv_desc* d, int x3) {
  if (!d) return 0;
  const WGradPlan pl = plan_wgrad(d, x3), pl2 = plan_wgrad(d, x3, 2);   // the f16x2 plan may split differently
  const size_t Ktot = (size_t)d->kh * d->kw * d->Cin;
  int sk = pl.splitk > pl2.splitk ? pl.splitk : pl2.splitk;
  if (x3 && d->Cin % 64 == 0) {   // ... and the planar kernels'
    for (int tr = 1; tr <= 2; ++tr) { const int sk3 = plan_wgrad(d, x3, 2, tr).splitk; sk = sk > sk3 ? sk : sk3; }
  }
  size_t a = sk > 1 ? (size_t)sk * d->Cout * Ktot * sizeof(float) : 0;
  size_t b = (size_t)colsum_blocks((int64_t)d->N * d->Ho * d->Wo) * d->Cout * sizeof(float);
  return (a > b ? a : b) + 256;
}

extern "C" size_t evk_conv2d_wgrad_workspace_bytes(const evk_conv_desc* d) { return wgrad_ws_bytes(d, 0); }
extern "C" size_t evk_conv2d_wgrad_x3_workspace_bytes(const evk_conv_desc* d) { return wgrad_ws_bytes(d, 1); }

namespace evk {

// The one decision of the weight-gradient family: arithmetic + operand flags + descriptor -> kernel, tile, operand form, split.
int route_wgrad(const evk_conv_desc* d, int planes, uint32_t flags, WGradRoute* r) {
  EVK_REQUIRE(d && r, EVK_E_INVALID, "conv2d_wgrad: null pointer");
  EVK_REQUIRE(planes >= 0 && planes <= 3, EVK_E_INVALID, "conv2d_wgrad: arithmetic %d (0 fp32, 1 bf16, 2 f16x2, 3 bf16x3)", planes);
  EVK_REQUIRE(d->Cin % 4 == 0 && d->Cout % 4 == 0, EVK_E_UNSUPPORTED,
              "conv2d_wgrad: Cin=%d and Cout=%d must be multiples of 4", d->Cin, d->Cout);
  EVK_REQUIRE((long long)d->N * d->H * d->W * d->Cin < 0x7fffffffLL &&
                  (long long)d->N * d->Ho * d->Wo * d->Cout < 0x7fffffffLL,
              EVK_E_UNSUPPORTED, "conv2d_wgrad: tensors of 2^31 or more elements are not supported");
  EVK_REQUIRE(planes == 2 || flags == 0, EVK_E_INVALID, "conv2d_wgrad: flags 0x%x belong to the f16x2 arithmetic", flags);
  const int planar = (flags & (EVK_CONV_X_PLANAR | EVK_CONV_DY_PLANAR)) ? 1 : 0;
  EVK_REQUIRE(!planar || ((flags & EVK_CONV_X_PLANAR) && (flags & EVK_CONV_DY_PLANAR) && planes == 2),
              EVK_E_UNSUPPORTED, "conv2d_wgrad: planar operands come in pairs (x and dy), f16x2 only, no bias gradient");
  EVK_REQUIRE(!planar || wgrad_tr_applicable(d, planes), EVK_E_UNSUPPORTED,
              "conv2d_wgrad: planar operands need Cin %% 64 == 0, Cout %% 64 == 0 and Wo %% 8 == 0 "
              "(Cin=%d Cout=%d Wo=%d) and tensors below 2 GiB", d->Cin, d->Cout, d->Wo);
  const int x3 = planes != 0;
  const int nine = planar && wgrad_tr_nine_tap(d) ? 1 : 0;
  WGradRoute o{};
  o.plan = plan_wgrad(d, x3, x3 ? planes : 3, planar ? 1 + nine : 0, (flags & EVK_CONV_WGRAD_SHARED) ? 1 : 0);
  o.kernel = planar ? WGradKernel::Tr : !x3 ? WGradKernel::Fp32 : o.plan.ws ? WGradKernel::X3Ws : WGradKernel::X3;
  o.pkx = (flags & EVK_CONV_X_PACKED) ? 1 : 0;
  o.pkd = (flags & EVK_CONV_DY_PACKED) ? 1 : 0;
  o.w8 = d->Wo % 8 == 0;
  o.nt = nine ? 9 : 1;
  // (the wave-specialised kernel takes the packed operands as two booleans, the single-role tiles as a fourth operand form)
  o.npx = planes == 2 && (o.pkx || o.pkd) && o.kernel == WGradKernel::X3 ? 4 : planes;
  *r = o;
  return EVK_OK;
}

// ---- the route as a kernel trace spells it
void wgrad_kernel_name(const WGradRoute& r, char* buf, size_t n) {
  auto tf = [](int v) { return v ? "true" : "false"; };
  switch (r.kernel) {
    case WGradKernel::Fp32: snprintf(buf, n, "conv_wgrad_kernel<%d, %d, 2, 2>", r.plan.bm, r.plan.bn); break;
    case WGradKernel::X3: snprintf(buf, n, "conv_wgrad_x3_kernel<%d, %d, 2, 2, %d>", r.plan.bm, r.plan.bn, r.npx); break;
    case WGradKernel::X3Ws:
      snprintf(buf, n, "conv_wgrad_x3ws_kernel<%d, %d, %d, %s, %s, %s>", r.plan.bm, r.plan.bn, r.npx, tf(r.w8), tf(r.pkx), tf(r.pkd));
      break;
    case WGradKernel::Tr: snprintf(buf, n, "conv_wgrad_tr_kernel<%d>", r.nt); break;
  }
}

}  // namespace evk

static int conv_wgrad_any(const evk_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                          void* workspace, size_t workspace_bytes, void* stream, int x3, int planes = 3,
                          const uint32_t* x_scale = nullptr, const uint32_t* dy_scale = nullptr, uint32_t pk_flags = 0) {
  EVK_REQUIRE(d && x && dy && dw, EVK_E_INVALID, "conv2d_wgrad: null pointer");
  WGradRoute route;
  int rc = route_wgrad(d, x3 ? planes : 0, pk_flags, &route);
  if (rc) return rc;
  const WGradPlan& pl = route.plan;
  EVK_REQUIRE(workspace_bytes >= wgrad_ws_bytes(d, x3) && (workspace || workspace_bytes == 0), EVK_E_WORKSPACE,
              "conv2d_wgrad: workspace %zu < %zu", workspace_bytes, wgrad_ws_bytes(d, x3));   // (sized over every plan of the arithmetic)
  hipStream_t st = (hipStream_t)stream;
  const int planar = route.kernel == WGradKernel::Tr ? 1 : 0;
  EVK_REQUIRE(!(planar && dbias), EVK_E_UNSUPPORTED, "conv2d_wgrad: planar operands come in pairs (x and dy), f16x2 only, no bias gradient");
  WGradArgs a{};
  a.planes = planes;
  a.planar = planar;
  a.x_scale = x_scale; a.dy_scale = dy_scale;
  a.x_packed = route.pkx;
  a.dy_packed = route.pkd;
  EVK_REQUIRE(!(a.dy_packed && dbias), EVK_E_UNSUPPORTED, "conv2d_wgrad: the bias gradient needs dy as fp32");
  a.x = x; a.dy = dy;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
  a.kh = d->kh; a.kw = d->kw; a.cpt = d->Cin / 4;
  a.sh = d->stride_h; a.sw = d->stride_w; a.ph = d->pad_h; a.pw = d->pad_w; a.dh = d->dil_h; a.dw = d->dil_w;
  a.M = d->N * d->Ho * d->Wo;
  a.Ktot = d->kh * d->kw * d->Cin;
  a.chunk = pl.chunk; a.tiles_co = pl.tiles_co; a.tiles_k = pl.tiles_k; a.splitk = pl.splitk;
  a.fd_hw = make_fastdiv((uint32_t)(d->Ho * d->Wo));
  a.fd_w = make_fastdiv((uint32_t)d->Wo);
  a.out = pl.splitk > 1 ? (float*)workspace : dw;
  switch (route.kernel) {
    case WGradKernel::Tr: rc = launch_wgrad_tr(a, route, st); break;
    case WGradKernel::X3:
    case WGradKernel::X3Ws: rc = launch_wgrad_x3(a, route, st); break;
    default: rc = launch_wgrad_f32(a, route, st);
  }
  if (rc) return rc;
  if (pl.splitk > 1) {
    const size_t n = (size_t)d->Cout * a.Ktot;  // multiple of 4 since Cin % 4 == 0
    const size_t n4 = n / 4;
    // enough threads to fill the chip: lanes per element = smallest power of two with n4 * lanes >= 128 K (<= 64)
    int lanes = 1;
    while (lanes < 64 && lanes * 2 <= pl.splitk && n4 * (size_t)lanes < 131072) lanes *= 2;
    const size_t epb = 256 / lanes;
    const int blocks = (int)((n4 + epb - 1) / epb > 4096 ? 4096 : (n4 + epb - 1) / epb);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const float*)workspace, dw, n4,
                       pl.splitk, n4, lanes);
    rc = check_launch("splitk_reduce");
    if (rc) return rc;
  }
  if (dbias) rc = launch_colsum(dy, dbias, a.M, d->Cout, (float*)workspace, st);
  return rc;
}

extern "C" int evk_conv2d_wgrad(const evk_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return conv_wgrad_any(d, x, dy, dw, dbias, workspace, workspace_bytes, stream, 0);
}

extern "C" int evk_conv2d_wgrad_bf16(const evk_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(d && d->Cin % 4 == 0 && d->Cout % 4 == 0, EVK_E_UNSUPPORTED, "conv2d_wgrad_bf16: channels must be multiples of 4");
  return conv_wgrad_any(d, x, dy, dw, dbias, workspace, workspace_bytes, stream, 1, 1);
}

// f16x2 arithmetic (conv_igemm.hip: evk_conv2d_fwd_f16x2): both operands are scaled activations
extern "C" int evk_conv2d_wgrad_f16x2(const evk_conv_desc* d, const float* x, const uint32_t* x_absmax, const float* dy,
                                      const uint32_t* dy_absmax, float* dw, float* dbias, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(d && d->Cin % 4 == 0 && d->Cout % 4 == 0, EVK_E_UNSUPPORTED, "conv2d_wgrad_f16x2: channels must be multiples of 4");
  EVK_REQUIRE(x_absmax && dy_absmax, EVK_E_INVALID, "conv2d_wgrad_f16x2: null scales");
  return conv_wgrad_any(d, x, dy, dw, dbias, workspace, workspace_bytes, stream, 1, 2, x_absmax, dy_absmax);
}

// flags: EVK_CONV_X_PACKED / EVK_CONV_DY_PACKED — that operand holds packed words (evk_pack_f16x2) instead of fp32
extern "C" int evk_conv2d_wgrad_f16x2_ex(const evk_conv_desc* d, const void* x, const uint32_t* x_absmax, const void* dy,
                                         const uint32_t* dy_absmax, float* dw, float* dbias, void* workspace,
                                         size_t workspace_bytes, uint32_t flags, void* stream) {
  EVK_REQUIRE(d && d->Cin % 4 == 0 && d->Cout % 4 == 0, EVK_E_UNSUPPORTED, "conv2d_wgrad_f16x2_ex: channels must be multiples of 4");
  EVK_REQUIRE(x_absmax && dy_absmax, EVK_E_INVALID, "conv2d_wgrad_f16x2_ex: null scales");
  EVK_REQUIRE((flags & ~kWGradFlags) == 0, EVK_E_INVALID,
              "conv2d_wgrad_f16x2_ex: unknown flag 0x%x", flags);
  return conv_wgrad_any(d, reinterpret_cast<const float*>(x), reinterpret_cast<const float*>(dy), dw, dbias, workspace,
                        workspace_bytes, stream, 1, 2, x_absmax, dy_absmax, flags);
}

extern "C" int evk_conv2d_wgrad_x3(const evk_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(d && d->Cin % 4 == 0 && d->Cout % 4 == 0, EVK_E_UNSUPPORTED, "conv2d_wgrad_x3: channels must be multiples of 4");
  return conv_wgrad_any(d, x, dy, dw, dbias, workspace, workspace_bytes, stream, 1);
}

// Host only: the instantiation and split plan a weight-gradient launch of this descriptor takes (include/ever_hip.h)
extern "C" int evk_conv2d_wgrad_route(const evk_conv_desc* d, int32_t planes, uint32_t flags, char* buf, size_t buf_bytes,
                                      int32_t* plan) {
  EVK_REQUIRE(d && buf && buf_bytes > 0, EVK_E_INVALID, "conv2d_wgrad_route: null pointer");
  EVK_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0 && d->kh > 0 && d->kw > 0 && d->stride_h > 0 &&
                  d->stride_w > 0 && d->dil_h > 0 && d->dil_w > 0 && d->Cin > 0 && d->Cout > 0,
              EVK_E_INVALID, "conv2d_wgrad_route: bad descriptor");
  EVK_REQUIRE((flags & ~kWGradFlags) == 0,
              EVK_E_INVALID, "conv2d_wgrad_route: unknown flag 0x%x", flags);
  buf[0] = 0;
  WGradRoute r;
  const int rc = route_wgrad(d, planes, flags, &r);
  if (rc) return rc;
  wgrad_kernel_name(r, buf, buf_bytes);
  if (plan) {
    plan[0] = r.plan.bm; plan[1] = r.plan.bn; plan[2] = r.plan.tiles_co;
    plan[3] = r.plan.tiles_k; plan[4] = r.plan.splitk; plan[5] = r.plan.chunk;
  }
  return EVK_OK;
}
