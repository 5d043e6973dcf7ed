// Depthwise convolution (groups == Cin == Cout, channel multiplier 1) on the vector ALUs.  Reference call sites:
// ever/module/ops.py:25-42 (DepthwiseConv2d / SeparableConv2d).
//
// A 3x3 depthwise convolution does 9 MACs per 8 bytes it moves: HBM-bound, so the arithmetic is exact fp32 FMA in every
// conv-math mode, and the kernels below are built around the loads.
//   forward   one thread = 4 channels (16-byte loads / stores along C) x a strip of kTW output pixels of one row; the input
//             window of a kernel row (dilation 1 along W) sits in registers, so every input element is loaded once per
//             strip and row; the other kernel rows come from L2.  Padding is a bounds check.
//   backward  one thread = 4 channels x a strip of kTB pixels x kTH rows.  It writes dx (the correlation of dy with the
//             flipped weight; stride 2 tests each tap's residue) and accumulates dw / db over its pixels; a workgroup sums
//             its threads' accumulators in LDS in a fixed order and stores one record per tile: slab [tiles][taps + 1][C].
//             depthwise_reduce_kernel then sums the records of all tiles in a fixed order.  No float atomics: two runs give
//             the same bits.
// Every element offset is 64-bit.
#include "stream_common.hpp"

namespace evk {

namespace {

constexpr int kTW = 8;    // forward: output pixels per thread along W
constexpr int kTB = 4;    // backward: pixels per thread along W
constexpr int kTH = 4;    // backward: rows per tile
constexpr int kMaxK = 7;

struct DwArgs {
  const float* x;      // [N][H][W][C]
  const float* w;      // [C][kh][kw]
  const float* bias;   // [C] or null
  const float* dy;     // [N][Ho][Wo][C]
  const float* y;      // relu mask source (backward) or null
  float* out;          // forward: y; backward: dx (may be null)
  float* slab;         // backward: [tiles][taps + 1][C] (may be null: no dw / db)
  int N, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw;
  int strips;          // strips per row
  int relu;
  // backward tiling
  int cl, ps;          // channel lanes (of 4 channels) and strips per workgroup: cl * ps == 256
  int row_tiles, strip_groups;
};

__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
  return f32x4{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y), __builtin_fmaf(a.z, b.z, c.z),
               __builtin_fmaf(a.w, b.w, c.w)};
}
// the weights of 4 channels at one tap: w[c][tap] for c = c0 .. c0 + 3
__device__ __forceinline__ f32x4 wtap(const float* __restrict__ w, int c0, int taps, int tap) {
  const float* p = w + (int64_t)c0 * taps + tap;
  return f32x4{p[0], p[taps], p[2 * taps], p[3 * taps]};
}
// dy at one pixel, zero where the fused ReLU was off
__device__ __forceinline__ f32x4 grad_at(const DwArgs& a, int64_t off) {
  f32x4 g = ld4(a.dy + off);
  if (a.y) {
    const f32x4 v = ld4(a.y + off);
    g.x = v.x > 0.f ? g.x : 0.f;
    g.y = v.y > 0.f ? g.y : 0.f;
    g.z = v.z > 0.f ? g.z : 0.f;
    g.w = v.w > 0.f ? g.w : 0.f;
  }
  return g;
}

}  // namespace

// (the kernels live in evk:: itself, so that profiles name them evk::depthwise_*: tools/families.py)
// ---------------------------------------------------------------------------------------------------------- forward
// KW: kernel width; SW: stride along W; D1: dilation 1 along W (the input window of a strip is then a compile-time
// register array).  Kernel height, vertical stride / dilation and padding are runtime values.
template <int KW, int SW, bool D1>
__global__ __launch_bounds__(256) void depthwise_fwd_kernel(DwArgs a) {
  const int C4 = a.C >> 2;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.N * a.Ho * a.strips * C4) return;
  const int cb = (int)(t % C4);
  int64_t r = t / C4;
  const int k = (int)(r % a.strips);
  r /= a.strips;
  const int oh = (int)(r % a.Ho);
  const int n = (int)(r / a.Ho);
  const int c0 = cb * 4;
  const int ow0 = k * kTW;
  const int iw0 = ow0 * SW - a.pw;
  const int taps = a.kh * KW;
  f32x4 acc[kTW];
#pragma unroll
  for (int j = 0; j < kTW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kr = 0; kr < a.kh; ++kr) {
    const int ih = oh * a.sh - a.ph + kr * a.dh;
    if ((unsigned)ih >= (unsigned)a.H) continue;
    const float* xrow = a.x + ((int64_t)n * a.H + ih) * a.W * a.C + c0;
    f32x4 wv[KW];
#pragma unroll
    for (int s = 0; s < KW; ++s) wv[s] = wtap(a.w, c0, taps, kr * KW + s);
    if (D1) {
      constexpr int WIN = (kTW - 1) * SW + KW;
      f32x4 xv[WIN];
#pragma unroll
      for (int i = 0; i < WIN; ++i) {
        const int iw = iw0 + i;
        xv[i] = (unsigned)iw < (unsigned)a.W ? ld4(xrow + (int64_t)iw * a.C) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < kTW; ++j)
#pragma unroll
        for (int s = 0; s < KW; ++s) acc[j] = fma4(xv[j * SW + s], wv[s], acc[j]);
    } else {
#pragma unroll
      for (int j = 0; j < kTW; ++j)
#pragma unroll
        for (int s = 0; s < KW; ++s) {
          const int iw = iw0 + j * SW + s * a.dw;
          if ((unsigned)iw < (unsigned)a.W) acc[j] = fma4(ld4(xrow + (int64_t)iw * a.C), wv[s], acc[j]);
        }
    }
  }
  const f32x4 b = a.bias ? ld4(a.bias + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
  float* yrow = a.out + ((int64_t)n * a.Ho + oh) * a.Wo * a.C + c0;
#pragma unroll
  for (int j = 0; j < kTW; ++j) {
    if (ow0 + j >= a.Wo) break;
    f32x4 v = acc[j] + b;
    if (a.relu) {
      v.x = fmaxf(v.x, 0.f);
      v.y = fmaxf(v.y, 0.f);
      v.z = fmaxf(v.z, 0.f);
      v.w = fmaxf(v.w, 0.f);
    }
    st4(yrow + (int64_t)(ow0 + j) * a.C, v);
  }
}

// --------------------------------------------------------------------------------------------------------- backward
// Workgroup = cl channel lanes x ps strips of kTB pixels, over kTH rows: one tile.  blockIdx.y: channel block.
// S1D1: stride 1 and dilation 1 along W (register windows along W); otherwise every tap is bounds- and residue-tested.
template <int KW, bool S1D1>
__global__ __launch_bounds__(256) void depthwise_bwd_kernel(DwArgs a) {
  __shared__ f32x4 red[kMaxK + 1][256];
  const int C4 = a.C >> 2;
  const int cl = threadIdx.x % a.cl, sp = threadIdx.x / a.cl;
  const int cb = blockIdx.y * a.cl + cl;
  const bool cok = cb < C4;
  const int c0 = (cok ? cb : 0) * 4;
  const int tile = blockIdx.x;
  const int sg = tile % a.strip_groups;
  const int rt = (tile / a.strip_groups) % a.row_tiles;
  const int n = tile / (a.strip_groups * a.row_tiles);
  const int k = sg * a.ps + sp;
  const int p0 = k * kTB;          // first pixel column of the strip (dx: input column; dw: output column)
  const int q0 = rt * kTH;
  const int taps = a.kh * KW;
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- dx[n][q][p0 + j] = sum over taps of g[oh][ow] * w[kr][s], oh * sh = q + ph - kr * dh, ow * sw = iw + pw - s * dw
  if (a.out && cok && k < a.strips) {
    for (int q = q0; q < q0 + kTH && q < a.H; ++q) {
      f32x4 acc[kTB];
#pragma unroll
      for (int j = 0; j < kTB; ++j) acc[j] = z4;
      for (int kr = 0; kr < a.kh; ++kr) {
        const int th = q + a.ph - kr * a.dh;
        if (th < 0 || th % a.sh) continue;
        const int oh = th / a.sh;
        if (oh >= a.Ho) continue;
        const int64_t rowoff = ((int64_t)n * a.Ho + oh) * a.Wo * a.C + c0;
        f32x4 wv[KW];
#pragma unroll
        for (int s = 0; s < KW; ++s) wv[s] = wtap(a.w, c0, taps, kr * KW + s);
        if (S1D1) {
          // ow = p0 + j + pw - s: window over ow0 = p0 + pw - (KW - 1) .. + kTB + KW - 2
          constexpr int WIN = kTB + KW - 1;
          const int owb = p0 + a.pw - (KW - 1);
          f32x4 gv[WIN];
#pragma unroll
          for (int i = 0; i < WIN; ++i) {
            const int ow = owb + i;
            gv[i] = (unsigned)ow < (unsigned)a.Wo ? grad_at(a, rowoff + (int64_t)ow * a.C) : z4;
          }
#pragma unroll
          for (int j = 0; j < kTB; ++j)
#pragma unroll
            for (int s = 0; s < KW; ++s) acc[j] = fma4(gv[j + KW - 1 - s], wv[s], acc[j]);
        } else {
#pragma unroll
          for (int j = 0; j < kTB; ++j)
#pragma unroll
            for (int s = 0; s < KW; ++s) {
              const int tw = p0 + j + a.pw - s * a.dw;
              if (tw < 0 || tw % a.sw) continue;
              const int ow = tw / a.sw;
              if (ow < a.Wo) acc[j] = fma4(grad_at(a, rowoff + (int64_t)ow * a.C), wv[s], acc[j]);
            }
        }
      }
      float* dxrow = a.out + ((int64_t)n * a.H + q) * a.W * a.C + c0;
#pragma unroll
      for (int j = 0; j < kTB; ++j)
        if (p0 + j < a.W) st4(dxrow + (int64_t)(p0 + j) * a.C, acc[j]);
    }
  }

  // ---- dw[kr][s] += g[oh][ow] * x[oh * sh - ph + kr * dh][ow * sw - pw + s * dw], db += g, over this thread's pixels
  if (!a.slab) return;     // (uniform over the grid)
  const bool wok = cok && k < a.strips;
  float* rec = a.slab + (int64_t)tile * (taps + 1) * a.C;
  for (int kr = 0; kr < a.kh; ++kr) {
    f32x4 dacc[KW];
    f32x4 bacc = z4;
#pragma unroll
    for (int s = 0; s < KW; ++s) dacc[s] = z4;
    if (wok) {
      for (int q = q0; q < q0 + kTH && q < a.Ho; ++q) {
        const int64_t grow = ((int64_t)n * a.Ho + q) * a.Wo * a.C + c0;
        f32x4 g[kTB];
#pragma unroll
        for (int j = 0; j < kTB; ++j) g[j] = p0 + j < a.Wo ? grad_at(a, grow + (int64_t)(p0 + j) * a.C) : z4;
        if (kr == 0)
#pragma unroll
          for (int j = 0; j < kTB; ++j) bacc += g[j];
        const int ih = q * a.sh - a.ph + kr * a.dh;
        if ((unsigned)ih >= (unsigned)a.H) continue;
        const float* xrow = a.x + ((int64_t)n * a.H + ih) * a.W * a.C + c0;
        if (S1D1) {
          constexpr int WIN = kTB + KW - 1;
          const int iwb = p0 - a.pw;
          f32x4 xv[WIN];
#pragma unroll
          for (int i = 0; i < WIN; ++i) {
            const int iw = iwb + i;
            xv[i] = (unsigned)iw < (unsigned)a.W ? ld4(xrow + (int64_t)iw * a.C) : z4;
          }
#pragma unroll
          for (int j = 0; j < kTB; ++j)
#pragma unroll
            for (int s = 0; s < KW; ++s) dacc[s] = fma4(g[j], xv[j + s], dacc[s]);
        } else {
#pragma unroll
          for (int j = 0; j < kTB; ++j)
#pragma unroll
            for (int s = 0; s < KW; ++s) {
              const int iw = (p0 + j) * a.sw - a.pw + s * a.dw;
              if ((unsigned)iw < (unsigned)a.W) dacc[s] = fma4(g[j], ld4(xrow + (int64_t)iw * a.C), dacc[s]);
            }
        }
      }
    }
    // the workgroup's sum in a fixed order: strips 0 .. ps - 1 of each channel lane
#pragma unroll
    for (int s = 0; s < KW; ++s) red[s][threadIdx.x] = dacc[s];
    red[kMaxK][threadIdx.x] = bacc;
    __syncthreads();
    if (sp == 0 && cok) {
#pragma unroll
      for (int s = 0; s < KW; ++s) {
        f32x4 v = red[s][cl];
        for (int i = 1; i < a.ps; ++i) v += red[s][i * a.cl + cl];
        st4(rec + (int64_t)(kr * KW + s) * a.C + c0, v);
      }
      if (kr == 0) {
        f32x4 v = red[kMaxK][cl];
        for (int i = 1; i < a.ps; ++i) v += red[kMaxK][i * a.cl + cl];
        st4(rec + (int64_t)taps * a.C + c0, v);
      }
    }
    __syncthreads();
  }
}

// dw[c][tap] = sum over tiles of slab[tile][tap][c], db[c] = sum of slab[tile][taps][c]: 4 lanes of 4 channels x 64
// slices of the tiles per workgroup; slice i takes tiles i, i + 64, ...; the slices are summed in order.
__global__ __launch_bounds__(256) void depthwise_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                               float* __restrict__ db, int tiles, int taps, int C) {
  __shared__ f32x4 red[256];
  const int C4 = C >> 2;
  const int lane = threadIdx.x & 3, slice = threadIdx.x >> 2;
  const int e = blockIdx.x * 4 + lane;            // (tap, channel group) flat: tap * C4 + cb, tap == taps: bias
  const int rec = (taps + 1) * C;
  const bool ok = e < (taps + 1) * C4;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const float* p = slab + (int64_t)e * 4;
    for (int t = slice; t < tiles; t += 64) v += ld4(p + (int64_t)t * rec);
  }
  red[threadIdx.x] = v;
  __syncthreads();
  if (slice != 0 || !ok) return;
  for (int i = 1; i < 64; ++i) v += red[i * 4 + lane];
  const int tap = e / C4, c0 = (e % C4) * 4;
  if (tap < taps) {
    if (dw) {
      dw[(int64_t)c0 * taps + tap] = v.x;
      dw[(int64_t)(c0 + 1) * taps + tap] = v.y;
      dw[(int64_t)(c0 + 2) * taps + tap] = v.z;
      dw[(int64_t)(c0 + 3) * taps + tap] = v.w;
    }
  } else if (db) {
    st4(db + c0, v);
  }
}

// ------------------------------------------------------------------------------------------------------ host side
namespace {

typedef void (*Launch)(const DwArgs&, dim3, hipStream_t);

template <int KW, int SW, bool D1>
void launch_fwd(const DwArgs& a, dim3 g, hipStream_t st) {
  hipLaunchKernelGGL((depthwise_fwd_kernel<KW, SW, D1>), g, dim3(256), 0, st, a);
}
template <int KW, bool S1D1>
void launch_bwd(const DwArgs& a, dim3 g, hipStream_t st) {
  hipLaunchKernelGGL((depthwise_bwd_kernel<KW, S1D1>), g, dim3(256), 0, st, a);
}

#define EVK_DW_FWD_ROW(K) \
  { {launch_fwd<K, 1, false>, launch_fwd<K, 1, true>}, {launch_fwd<K, 2, false>, launch_fwd<K, 2, true>} }
const Launch kFwd[kMaxK][2][2] = {EVK_DW_FWD_ROW(1), EVK_DW_FWD_ROW(2), EVK_DW_FWD_ROW(3), EVK_DW_FWD_ROW(4),
                                  EVK_DW_FWD_ROW(5), EVK_DW_FWD_ROW(6), EVK_DW_FWD_ROW(7)};
#undef EVK_DW_FWD_ROW
#define EVK_DW_BWD_ROW(K) {launch_bwd<K, false>, launch_bwd<K, true>}
const Launch kBwd[kMaxK][2] = {EVK_DW_BWD_ROW(1), EVK_DW_BWD_ROW(2), EVK_DW_BWD_ROW(3), EVK_DW_BWD_ROW(4),
                               EVK_DW_BWD_ROW(5), EVK_DW_BWD_ROW(6), EVK_DW_BWD_ROW(7)};
#undef EVK_DW_BWD_ROW

// The scope of the kernels; the message names the first violation.
int check_desc(const evk_conv_desc* d, const char* what) {
  EVK_REQUIRE(d, EVK_E_INVALID, "%s: null descriptor", what);
  EVK_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Ho > 0 && d->Wo > 0, EVK_E_INVALID,
              "%s: non-positive dimension", what);
  EVK_REQUIRE(d->Cin == d->Cout, EVK_E_UNSUPPORTED, "%s: Cin (%d) must equal Cout (%d): channel multiplier 1 only", what,
              d->Cin, d->Cout);
  EVK_REQUIRE(d->Cin % 4 == 0, EVK_E_UNSUPPORTED, "%s: C (%d) must be a multiple of 4", what, d->Cin);
  EVK_REQUIRE(d->kh >= 1 && d->kh <= kMaxK && d->kw >= 1 && d->kw <= kMaxK, EVK_E_UNSUPPORTED,
              "%s: kernel %dx%d outside 1..7", what, d->kh, d->kw);
  EVK_REQUIRE((d->stride_h == 1 || d->stride_h == 2) && (d->stride_w == 1 || d->stride_w == 2), EVK_E_UNSUPPORTED,
              "%s: stride (%d, %d) must be 1 or 2", what, d->stride_h, d->stride_w);
  EVK_REQUIRE(d->dil_h >= 1 && d->dil_w >= 1 && d->pad_h >= 0 && d->pad_w >= 0, EVK_E_UNSUPPORTED,
              "%s: dilation must be positive and padding non-negative", what);
  EVK_REQUIRE(d->H + 2 * (int64_t)d->pad_h >= (int64_t)d->dil_h * (d->kh - 1) + 1, EVK_E_INVALID,
              "%s: kernel extent %lld along H exceeds the padded input (%lld): H + 2 * pad_h < dil_h * (kh - 1) + 1", what,
              (long long)d->dil_h * (d->kh - 1) + 1, (long long)d->H + 2 * (long long)d->pad_h);
  EVK_REQUIRE(d->W + 2 * (int64_t)d->pad_w >= (int64_t)d->dil_w * (d->kw - 1) + 1, EVK_E_INVALID,
              "%s: kernel extent %lld along W exceeds the padded input (%lld): W + 2 * pad_w < dil_w * (kw - 1) + 1", what,
              (long long)d->dil_w * (d->kw - 1) + 1, (long long)d->W + 2 * (long long)d->pad_w);
  EVK_REQUIRE(d->Ho == (d->H + 2 * d->pad_h - d->dil_h * (d->kh - 1) - 1) / d->stride_h + 1 &&
                  d->Wo == (d->W + 2 * d->pad_w - d->dil_w * (d->kw - 1) - 1) / d->stride_w + 1,
              EVK_E_INVALID, "%s: output size (%d, %d) does not follow from the geometry", what, d->Ho, d->Wo);
  return EVK_OK;
}

DwArgs make_args(const evk_conv_desc* d) {
  DwArgs a = {};
  a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo;
  a.kh = d->kh; a.kw = d->kw; a.sh = d->stride_h; a.sw = d->stride_w;
  a.ph = d->pad_h; a.pw = d->pad_w; a.dh = d->dil_h; a.dw = d->dil_w;
  return a;
}

// The forms and tilings of a descriptor in scope: the one place the launchers, the workspace size and evk_depthwise_plan
// take them from.
struct DwPlan {
  int fkw, fsw, fd1;          // forward instantiation <KW, SW, D1>
  int fstrips;                // forward: strips of kTW output pixels per row
  int64_t fblocks;            // forward: workgroups
  int bkw, bs1d1;             // backward instantiation <KW, S1D1>
  int cl, ps;                 // backward: channel lanes (a power of two <= 64) and strips per workgroup
  int bstrips, strip_groups, row_tiles, cblocks;
  int64_t tiles;
};

DwPlan dw_plan(const DwArgs& a) {
  DwPlan p;
  const int C4 = a.C / 4;
  p.fkw = a.kw; p.fsw = a.sw; p.fd1 = a.dw == 1 ? 1 : 0;
  p.fstrips = ceil_div(a.Wo, kTW);
  p.fblocks = ((int64_t)a.N * a.Ho * p.fstrips * C4 + 255) / 256;
  p.bkw = a.kw; p.bs1d1 = (a.sw == 1 && a.dw == 1) ? 1 : 0;
  int cl = 1;
  while (cl < C4 && cl < 16) cl *= 2;
  // the widest of 16 / 32 / 64 lanes that idles no more of them than a narrower one (C = 304: 16 lanes x 5 blocks)
  for (int w = 32; w <= 64 && C4 > 16; w *= 2)
    if ((int64_t)ceil_div(C4, w) * w <= (int64_t)ceil_div(C4, cl) * cl) cl = w;
  p.cl = cl;
  p.ps = 256 / cl;
  const int wmax = a.W > a.Wo ? a.W : a.Wo;
  const int hmax = a.H > a.Ho ? a.H : a.Ho;
  p.bstrips = ceil_div(wmax, kTB);
  p.strip_groups = ceil_div(p.bstrips, p.ps);
  p.row_tiles = ceil_div(hmax, kTH);
  p.cblocks = ceil_div(C4, cl);
  p.tiles = (int64_t)a.N * p.row_tiles * p.strip_groups;
  return p;
}

bool fwd_fits(const DwPlan& p) { return p.fblocks < 0x7fffffff; }
bool bwd_fits(const DwPlan& p) { return p.tiles < 0x7fffffff && p.cblocks <= 65535; }

void set_bwd_tiling(DwArgs& a, const DwPlan& p) {
  a.cl = p.cl; a.ps = p.ps;
  a.strips = p.bstrips; a.strip_groups = p.strip_groups; a.row_tiles = p.row_tiles;
}

size_t slab_bytes(const DwArgs& a, const DwPlan& p) {
  return (size_t)p.tiles * (size_t)(a.kh * a.kw + 1) * (size_t)a.C * sizeof(float);
}

}  // namespace

}  // namespace evk

using namespace evk;

extern "C" int evk_depthwise_fwd(const evk_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                                 uint32_t flags, void* stream) {
  int rc = check_desc(d, "depthwise_fwd");
  if (rc) return rc;
  EVK_REQUIRE(x && w && y, EVK_E_INVALID, "depthwise_fwd: null pointer");
  DwArgs a = make_args(d);
  a.x = x; a.w = w; a.bias = bias; a.out = y;
  a.relu = (flags & EVK_CONV_RELU) ? 1 : 0;
  const DwPlan p = dw_plan(a);
  EVK_REQUIRE(fwd_fits(p), EVK_E_UNSUPPORTED, "depthwise_fwd: grid too large");
  a.strips = p.fstrips;
  kFwd[p.fkw - 1][p.fsw - 1][p.fd1](a, dim3((unsigned)p.fblocks), (hipStream_t)stream);
  return check_launch("depthwise_fwd");
}

extern "C" size_t evk_depthwise_bwd_workspace_bytes(const evk_conv_desc* d) {
  if (check_desc(d, "depthwise_bwd_workspace_bytes")) return 0;
  const DwArgs a = make_args(d);
  return slab_bytes(a, dw_plan(a));
}

// Host only (no launch): out = {forward KW, SW, D1, forward strips per row, forward workgroups, backward KW, S1D1, channel
// lanes cl, strips per workgroup ps, backward strips per row, strip groups, row tiles, channel blocks, tiles}
extern "C" int evk_depthwise_plan(const evk_conv_desc* d, int32_t* out) {
  int rc = check_desc(d, "depthwise_plan");
  if (rc) return rc;
  EVK_REQUIRE(out, EVK_E_INVALID, "depthwise_plan: null pointer");
  const DwPlan p = dw_plan(make_args(d));
  EVK_REQUIRE(fwd_fits(p) && bwd_fits(p), EVK_E_UNSUPPORTED, "depthwise_plan: grid too large");
  const int32_t v[14] = {p.fkw, p.fsw, p.fd1, p.fstrips, (int32_t)p.fblocks, p.bkw, p.bs1d1, p.cl, p.ps, p.bstrips,
                         p.strip_groups, p.row_tiles, p.cblocks, (int32_t)p.tiles};
  for (int i = 0; i < 14; ++i) out[i] = v[i];
  return EVK_OK;
}

extern "C" int evk_depthwise_bwd(const evk_conv_desc* d, const float* dy, const float* x, const float* y, const float* w,
                                 float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_desc(d, "depthwise_bwd");
  if (rc) return rc;
  EVK_REQUIRE(dy && w, EVK_E_INVALID, "depthwise_bwd: null pointer");
  EVK_REQUIRE(!(dw || db) || x, EVK_E_INVALID, "depthwise_bwd: the weight / bias gradient needs x");
  if (!dx && !dw && !db) return EVK_OK;
  DwArgs a = make_args(d);
  const DwPlan p = dw_plan(a);
  set_bwd_tiling(a, p);
  const int64_t tiles = p.tiles;
  const bool params = dw || db;
  if (params)
    EVK_REQUIRE(workspace && workspace_bytes >= slab_bytes(a, p), EVK_E_WORKSPACE,
                "depthwise_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, slab_bytes(a, p));
  EVK_REQUIRE(bwd_fits(p), EVK_E_UNSUPPORTED, "depthwise_bwd: grid too large");
  a.dy = dy; a.x = x; a.y = y; a.w = w; a.out = dx;
  a.slab = params ? reinterpret_cast<float*>(workspace) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  kBwd[p.bkw - 1][p.bs1d1](a, dim3((unsigned)tiles, (unsigned)p.cblocks), st);
  if (params) {
    const int taps = a.kh * a.kw;
    hipLaunchKernelGGL(depthwise_reduce_kernel, dim3((unsigned)ceil_div((int64_t)(taps + 1) * (a.C / 4), 4)), dim3(256), 0,
                       st, (const float*)a.slab, dw, db, (int)tiles, taps, a.C);
  }
  return check_launch("depthwise_bwd");
}
