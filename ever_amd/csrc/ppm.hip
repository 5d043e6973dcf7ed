// Pyramid pooling (reference ppm.py:8-35, ops.py:89-100) as fused passes on NHWC fp32 (gfx950): the K adaptive average pools
// of one map from ONE read of it, the K bilinear (align_corners=False) up-samplings and the channel concat as ONE write of
// the concat map, and both backward halves in gather form.  Layer by layer the reference reads the input K times, writes K
// up-sampled maps and reads them again for torch.cat; its backward mirrors that and adds K + 1 gradients of the input.
//
// Pool forward.  Each axis is cut at the union of all bins' window edges (ys = floor(i L / b), ye = ceil((i + 1) L / b)):
// at most 2 sum(b) edges, so at most 63 elementary cells per axis, which partition the map.
//   stage 1 (ppm_cells_kernel): a workgroup owns one cell row of one image at 64 16-byte channel columns.  Its four waves
//     take the rows of the cell row round robin (wave g: rows y0 + g, y0 + g + 4, ...); a lane adds its rows in ascending y,
//     each row in ascending x, from +0; the four partials meet in LDS as ((g0 + g1) + g2) + g3.  One sum per cell, to the
//     workspace [N, ncy, ncx, C].
//   stage 2 (ppm_windows_kernel): a window's cells are added row-major from +0, then ONE division by float(count).
// Expand forward: a workgroup per output pixel; the K tap decodes and weights are computed once (threads 0..K-1, through
// LDS) and shared by all channels of the pixel.  Expand backward, separable and in gather form: stage 1 folds every row of
// dcat's pooled slices along x into [N, H, sum(b), Cp] (ascending x, one read of dcat for all K bins), stage 2 folds that
// along y (ascending y); every output element has one owner.  Pool backward: a workgroup per pixel adds, onto the skip
// gradient, dp / count of every window that holds the pixel: bins in order, windows row-major, one division per quotient.
// No float atomics, the same bits every run; 16-byte accesses along the channel axis (C % 4 == 0, Cp % 4 == 0) throughout.
#include "stream_common.hpp"

// every product and sum below is rounded on its own: the tests state the blend and the quotient sums bit for bit
#pragma clang fp contract(off)

namespace evk {

constexpr int kPpmMaxBins = 4, kPpmMaxBin = 8, kPpmThreads = 256;
constexpr int kPpmMaxEdges = 2 * kPpmMaxBins * kPpmMaxBin + 2;     // before duplicates are dropped; 64 remain at most

struct PpmGeom {
  int32_t K, ncy, ncx, sumb, sumb2;
  int32_t b[kPpmMaxBins];
  int32_t boff[kPpmMaxBins];                                     // sum of the bins in front of bin k
  int32_t ey[kPpmMaxEdges], ex[kPpmMaxEdges];                    // cell c of an axis is [e[c], e[c + 1])
  uint8_t wy0[kPpmMaxBins][kPpmMaxBin], wy1[kPpmMaxBins][kPpmMaxBin];   // window i of bin k = cells [w0, w1) of the axis
  uint8_t wx0[kPpmMaxBins][kPpmMaxBin], wx1[kPpmMaxBins][kPpmMaxBin];
};

struct PpmPtrs {
  float* p[kPpmMaxBins];
};

// window i of an axis of L pixels cut into b: [ws, we).  32-bit: (i + 1) L + b - 1 <= 8 (2^29 - 1) + 7 (L 4 < 2^31: C >= 4)
__host__ __device__ inline int ppm_ws(int i, int L, int b) { return (int)(((uint32_t)i * (uint32_t)L) / (uint32_t)b); }
__host__ __device__ inline int ppm_we(int i, int L, int b) {
  return (int)(((uint32_t)(i + 1) * (uint32_t)L + (uint32_t)(b - 1)) / (uint32_t)b);
}

// the table entries picked by constants: a run-time index into a by-value argument would put it in scratch
__device__ __forceinline__ int ppm_bin(const PpmGeom& g, int k) { return k == 0 ? g.b[0] : k == 1 ? g.b[1] : k == 2 ? g.b[2] : g.b[3]; }
__device__ __forceinline__ int ppm_boff(const PpmGeom& g, int k) {
  return k == 0 ? g.boff[0] : k == 1 ? g.boff[1] : k == 2 ? g.boff[2] : g.boff[3];
}
__device__ __forceinline__ float* ppm_ptr(const PpmPtrs& a, int k) { return k == 0 ? a.p[0] : k == 1 ? a.p[1] : k == 2 ? a.p[2] : a.p[3]; }

static int ppm_axis(int L, const int32_t* bins, int K, int32_t* e, uint8_t (*w0)[kPpmMaxBin], uint8_t (*w1)[kPpmMaxBin]) {
  int n = 0;
  e[n++] = 0;
  e[n++] = L;
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < bins[k]; ++i) {
      e[n++] = ppm_ws(i, L, bins[k]);
      e[n++] = ppm_we(i, L, bins[k]);
    }
  for (int a = 1; a < n; ++a) {      // insertion sort, then drop duplicates
    const int v = e[a];
    int c = a;
    for (; c > 0 && e[c - 1] > v; --c) e[c] = e[c - 1];
    e[c] = v;
  }
  int m = 1;
  for (int a = 1; a < n; ++a)
    if (e[a] != e[m - 1]) e[m++] = e[a];
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < bins[k]; ++i) {
      const int s = ppm_ws(i, L, bins[k]), t = ppm_we(i, L, bins[k]);
      int c0 = 0, c1 = 0;
      while (e[c0] != s) ++c0;
      while (e[c1] != t) ++c1;
      w0[k][i] = (uint8_t)c0;
      w1[k][i] = (uint8_t)c1;
    }
  return m - 1;      // cells
}

// pure host arithmetic, shared by the launchers, evk_ppm_plan and the workspace queries.  Cp == 0: the pools alone;
// C == 0: the up-sampled maps alone (the launchers ask for the side they need).
static int ppm_geom(const char* what, int N, int H, int W, int C, int Cp, const int32_t* bins, int K, PpmGeom* g) {
  EVK_REQUIRE(bins && N > 0 && H > 0 && W > 0 && C >= 0 && Cp >= 0 && (C > 0 || Cp > 0), EVK_E_INVALID,
              "%s: bad argument (null pointer or non-positive size)", what);
  EVK_REQUIRE(K >= 1 && K <= kPpmMaxBins, EVK_E_UNSUPPORTED, "%s: %d bins (1 to %d are implemented)", what, K, kPpmMaxBins);
  for (int k = 0; k < K; ++k)
    EVK_REQUIRE(bins[k] >= 1 && bins[k] <= kPpmMaxBin, EVK_E_UNSUPPORTED, "%s: bin %d is %d (1 to %d are implemented)", what, k,
                bins[k], kPpmMaxBin);
  EVK_REQUIRE(C % 4 == 0 && Cp % 4 == 0, EVK_E_UNSUPPORTED, "%s: C = %d and Cp = %d must be multiples of 4", what, C, Cp);
  const int64_t total = (int64_t)N * H * W * ((int64_t)C + (int64_t)K * Cp);
  EVK_REQUIRE(total < 0x80000000LL, EVK_E_UNSUPPORTED, "%s: N H W (C + K Cp) = %lld (fewer than 2^31 are implemented)", what,
              (long long)total);
  *g = PpmGeom{};
  g->K = K;
  for (int k = 0; k < K; ++k) {
    g->b[k] = bins[k];
    g->boff[k] = g->sumb;
    g->sumb += bins[k];
    g->sumb2 += bins[k] * bins[k];
  }
  for (int k = K; k < kPpmMaxBins; ++k) { g->b[k] = 1; g->boff[k] = g->sumb; }
  // (a batch of 2^23 one-pixel maps: the grids of the small stages are 32-bit too)
  EVK_REQUIRE((int64_t)N * g->sumb2 < 0x7fffffffLL && (int64_t)N * g->sumb * (Cp / 4) < 0x7fffffffLL, EVK_E_UNSUPPORTED,
              "%s: N = %d with %d pooled cells (fewer than 2^31 pooled elements are implemented)", what, N, g->sumb2);
  g->ncy = ppm_axis(H, bins, K, g->ey, g->wy0, g->wy1);
  g->ncx = ppm_axis(W, bins, K, g->ex, g->wx0, g->wx1);
  return EVK_OK;
}

static inline int64_t ppm_pool_ws_bytes(const PpmGeom& g, int N, int C) { return (int64_t)N * g.ncy * g.ncx * C * 4; }
static inline int64_t ppm_expand_ws_bytes(const PpmGeom& g, int N, int H, int Cp) { return (int64_t)N * H * g.sumb * Cp * 4; }

__device__ __forceinline__ f32x4 ppm_scale(float a, const f32x4 v) { return f32x4{a * v.x, a * v.y, a * v.z, a * v.w}; }
__device__ __forceinline__ f32x4 ppm_div(const f32x4 v, float d) {
  return f32x4{__fdiv_rn(v.x, d), __fdiv_rn(v.y, d), __fdiv_rn(v.z, d), __fdiv_rn(v.w, d)};
}

// ---- pool forward, stage 1: workgroup (n, cy, chunk), wave g the rows y0 + g, y0 + g + 4, ... of the cell row
__global__ __launch_bounds__(kPpmThreads) void ppm_cells_kernel(const PpmGeom g, const float* __restrict__ x,
                                                                float* __restrict__ cells, int H, int W, int C, int nchunk) {
  __shared__ f32x4 part[2][4][kWave];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const uint32_t row = blockIdx.x / (uint32_t)nchunk, chunk = blockIdx.x - row * (uint32_t)nchunk;   // row = n * ncy + cy
  const uint32_t n = row / (uint32_t)g.ncy, cy = row - n * (uint32_t)g.ncy;
  const int c = ((int)chunk * kWave + lane) * 4;
  const bool on = c < C;
  const int y0 = g.ey[cy], y1 = g.ey[cy + 1];
  for (int cx = 0; cx < g.ncx; ++cx) {
    const int x0 = g.ex[cx], x1 = g.ex[cx + 1];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (on)
      for (int y = y0 + grp; y < y1; y += 4) {
        const float* p = x + (((size_t)n * H + y) * W + x0) * C + c;
#pragma unroll 4
        for (int xx = x0; xx < x1; ++xx, p += C) acc = acc + ld4(p);
      }
    part[cx & 1][grp][lane] = acc;
    __syncthreads();      // one barrier per cell: the other half of `part` is written next
    if (grp == 0 && on) {
      const f32x4 s = ((part[cx & 1][0][lane] + part[cx & 1][1][lane]) + part[cx & 1][2][lane]) + part[cx & 1][3][lane];
      st4(cells + ((size_t)row * g.ncx + cx) * C + c, s);
    }
  }
}

// ---- pool forward, stage 2: workgroup (n, window); a thread per 16-byte channel column, striding
__global__ __launch_bounds__(kPpmThreads) void ppm_windows_kernel(const PpmGeom g, const float* __restrict__ cells,
                                                                  const PpmPtrs out, int H, int W, int C) {
  const uint32_t n = blockIdx.x / (uint32_t)g.sumb2;
  int rem = (int)(blockIdx.x - n * (uint32_t)g.sumb2), k = 0;
#pragma unroll
  for (int kk = 0; kk < kPpmMaxBins - 1; ++kk) {
    const int bb = g.b[kk] * g.b[kk];
    if (k == kk && kk < g.K - 1 && rem >= bb) { rem -= bb; k = kk + 1; }
  }
  const int b = ppm_bin(g, k), i = rem / b, j = rem - i * b;
  const int cy0 = g.wy0[k][i], cy1 = g.wy1[k][i], cx0 = g.wx0[k][j], cx1 = g.wx1[k][j];
  const float count = (float)((ppm_we(i, H, b) - ppm_ws(i, H, b)) * (ppm_we(j, W, b) - ppm_ws(j, W, b)));
  float* p = ppm_ptr(out, k);
  for (int c = threadIdx.x * 4; c < C; c += kPpmThreads * 4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int cy = cy0; cy < cy1; ++cy)
      for (int cx = cx0; cx < cx1; ++cx) acc = acc + ld4(cells + (((size_t)n * g.ncy + cy) * g.ncx + cx) * C + c);
    st4(p + (((size_t)n * b + i) * b + j) * C + c, ppm_div(acc, count));
  }
}

// the bilinear align_corners=False taps of output index y on an axis of b source cells and L outputs (include/ever_hip.h)
__device__ __forceinline__ void ppm_tap(int b, int L, int y, int& i0, int& i1, float& l0, float& l1) {
  // plain operators under this file's `fp contract(off)`: the __fmul_rn / __fsub_rn intrinsics are inlined from a header
  // compiled with contraction on, and s * (y + 0.5) - 0.5 became one fma (first GPU run: other bits than the statement)
  const float s = __fdiv_rn((float)b, (float)L);
  const float t = s * ((float)y + 0.5f);
  const float src = fmaxf(t - 0.5f, 0.f);
  i0 = min((int)src, b - 1);
  i1 = i0 + (i0 < b - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}
__device__ __forceinline__ f32x4 ppm_blend(float l0, const f32x4 a, float l1, const f32x4 b) {
  return ppm_scale(l0, a) + ppm_scale(l1, b);
}

// the pixel of a workgroup-per-pixel kernel: pix = (n * H + py) * W + px
__device__ __forceinline__ void ppm_pixel(uint32_t pix, int H, int W, uint32_t& n, uint32_t& py, uint32_t& px) {
  const uint32_t r = pix / (uint32_t)W;      // r = n * H + py
  px = pix - r * (uint32_t)W;
  n = r / (uint32_t)H;
  py = r - n * (uint32_t)H;
}

// ---- expand forward: workgroup per pixel
__global__ __launch_bounds__(kPpmThreads) void ppm_expand_fwd_kernel(const PpmGeom g, const float* __restrict__ x,
                                                                     const PpmPtrs z, float* __restrict__ cat, int H, int W,
                                                                     int C, int Cp) {
  __shared__ int si[kPpmMaxBins][4];
  __shared__ float sl[kPpmMaxBins][4];
  const uint32_t pix = blockIdx.x;
  uint32_t n, py, px;
  ppm_pixel(pix, H, W, n, py, px);
  if ((int)threadIdx.x < g.K) {
    const int k = threadIdx.x, b = ppm_bin(g, k);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    ppm_tap(b, H, (int)py, y0, y1, ly0, ly1);
    ppm_tap(b, W, (int)px, x0, x1, lx0, lx1);
    si[k][0] = y0; si[k][1] = y1; si[k][2] = x0; si[k][3] = x1;
    sl[k][0] = ly0; sl[k][1] = ly1; sl[k][2] = lx0; sl[k][3] = lx1;
  }
  __syncthreads();
  const int ctot = C + g.K * Cp;
  float* o = cat + (size_t)pix * ctot;
  const float* xi = x + (size_t)pix * C;
  for (int c = threadIdx.x * 4; c < ctot; c += kPpmThreads * 4) {
    if (c < C) {
      st4(o + c, ld4(xi + c));
      continue;
    }
    const int k = (c - C) / Cp, cc = (c - C) - k * Cp, b = ppm_bin(g, k);
    const int y0 = si[k][0], y1 = si[k][1], x0 = si[k][2], x1 = si[k][3];
    const float* zk = ppm_ptr(z, k) + (size_t)n * b * b * Cp + cc;
    f32x4 top = ld4(zk + (size_t)(y0 * b + x0) * Cp);
    if (x1 != x0) top = ppm_blend(sl[k][2], top, sl[k][3], ld4(zk + (size_t)(y0 * b + x1) * Cp));
    if (y1 != y0) {
      f32x4 bot = ld4(zk + (size_t)(y1 * b + x0) * Cp);
      if (x1 != x0) bot = ppm_blend(sl[k][2], bot, sl[k][3], ld4(zk + (size_t)(y1 * b + x1) * Cp));
      top = ppm_blend(sl[k][0], top, sl[k][1], bot);
    }
    st4(o + c, top);
  }
}

// One axis of the expand backward: `len` values come in ascending order, value t carries weight l0 for source cell i0 and
// l1 for i1 = i0 + 1 (weight 1 for i0 alone where the taps coincide).  i0 never decreases, so two running sums suffice:
// a0 for cell `cur`, a1 for cur + 1; a cell is written once, when the walk has passed it (zero if nothing reached it).
template <typename Load, typename Store>
__device__ __forceinline__ void ppm_fold_axis(int b, int len, Load&& load, Store&& store) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  int cur = 0;
  for (int t = 0; t < len; ++t) {
    int i0, i1;
    float l0, l1;
    ppm_tap(b, len, t, i0, i1, l0, l1);
    for (; cur < i0; ++cur) {
      store(cur, a0);
      a0 = a1;
      a1 = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const f32x4 v = load(t);
    if (i1 == i0) {
      a0 = a0 + v;
    } else {
      a0 = a0 + ppm_scale(l0, v);
      a1 = a1 + ppm_scale(l1, v);
    }
  }
  for (; cur < b; ++cur) {
    store(cur, a0);
    a0 = a1;
    a1 = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// ---- expand backward, stage 1: workgroup (row n * H + y, chunk of 256 16-byte columns of the K Cp pooled channels)
__global__ __launch_bounds__(kPpmThreads) void ppm_expand_bwd_rows_kernel(const PpmGeom g, const float* __restrict__ dcat,
                                                                          float* __restrict__ rows, int W, int C, int Cp,
                                                                          int nchunk) {
  const uint32_t r = blockIdx.x / (uint32_t)nchunk, chunk = blockIdx.x - r * (uint32_t)nchunk;
  const int q = ((int)chunk * kPpmThreads + (int)threadIdx.x) * 4;      // channel within the pooled slices
  if (q >= g.K * Cp) return;
  const int k = q / Cp, c = q - k * Cp, b = ppm_bin(g, k), ctot = C + g.K * Cp;
  const float* src = dcat + (size_t)r * W * ctot + C + q;
  float* dst = rows + ((size_t)r * g.sumb + ppm_boff(g, k)) * Cp + c;
  ppm_fold_axis(b, W, [&](int xx) { return ld4(src + (size_t)xx * ctot); },
                [&](int j, const f32x4 v) { st4(dst + (size_t)j * Cp, v); });
}

// ---- expand backward, stage 2: a thread per (n, column jj of sum(b), 16-byte channel column)
__global__ __launch_bounds__(kPpmThreads) void ppm_expand_bwd_cols_kernel(const PpmGeom g, const float* __restrict__ rows,
                                                                          const PpmPtrs dz, uint32_t total, int H, int Cp) {
  const uint32_t idx = blockIdx.x * (uint32_t)kPpmThreads + threadIdx.x;
  if (idx >= total) return;
  const uint32_t cp4 = (uint32_t)Cp >> 2;
  const uint32_t r = idx / cp4, c = (idx - r * cp4) * 4;
  const uint32_t n = r / (uint32_t)g.sumb;
  const int jj = (int)(r - n * (uint32_t)g.sumb);
  int k = 0;
#pragma unroll
  for (int kk = 1; kk < kPpmMaxBins; ++kk)
    if (kk < g.K && jj >= g.boff[kk]) k = kk;
  const int b = ppm_bin(g, k), j = jj - ppm_boff(g, k);
  const float* src = rows + ((size_t)n * H * g.sumb + jj) * Cp + c;
  float* dst = ppm_ptr(dz, k) + ((size_t)n * b * b + j) * Cp + c;
  const size_t ystride = (size_t)g.sumb * Cp;
  ppm_fold_axis(b, H, [&](int y) { return ld4(src + (size_t)y * ystride); },
                [&](int i, const f32x4 v) { st4(dst + (size_t)i * b * Cp, v); });
}

// ---- pool backward: workgroup per pixel; the windows of bin k that hold row y are i = floor(y b / H) .. ceil((y + 1) b / H) - 1.
// The pixel's window ranges and the window extents are decoded once (threads 0..63, through LDS) and shared by its channels.
__global__ __launch_bounds__(kPpmThreads) void ppm_pool_bwd_kernel(const PpmGeom g, const PpmPtrs dp,
                                                                   const float* __restrict__ dskip, int ld,
                                                                   float* __restrict__ dx, int H, int W, int C) {
  __shared__ int ext[kPpmMaxBins][2][kPpmMaxBin];      // rows (0) or columns (1) of window i of bin k
  __shared__ int rng[kPpmMaxBins][4];
  const uint32_t pix = blockIdx.x;
  uint32_t n, py, px;
  ppm_pixel(pix, H, W, n, py, px);
  if (threadIdx.x < kPpmMaxBins * 2 * kPpmMaxBin) {
    const int k = threadIdx.x >> 4, ax = (threadIdx.x >> 3) & 1, i = threadIdx.x & 7, b = ppm_bin(g, k);
    const int L = ax ? W : H;
    ext[k][ax][i] = i < b ? ppm_we(i, L, b) - ppm_ws(i, L, b) : 1;
    if (i == 0) {
      const uint32_t pos = ax ? px : py;
      rng[k][2 * ax] = (int)(pos * (uint32_t)b / (uint32_t)L);
      rng[k][2 * ax + 1] = (int)(((pos + 1) * (uint32_t)b + (uint32_t)(L - 1)) / (uint32_t)L) - 1;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x * 4; c < C; c += kPpmThreads * 4) {
    f32x4 acc = dskip ? ld4(dskip + (size_t)pix * ld + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kPpmMaxBins; ++k) {
      if (k >= g.K) break;
      const int b = g.b[k];
      const float* dk = dp.p[k] + (size_t)n * b * b * C + c;
      for (int i = rng[k][0]; i <= rng[k][1]; ++i)
        for (int j = rng[k][2]; j <= rng[k][3]; ++j)
          acc = acc + ppm_div(ld4(dk + (size_t)(i * b + j) * C), (float)(ext[k][0][i] * ext[k][1][j]));
    }
    st4(dx + (size_t)pix * C + c, acc);
  }
}

static int ppm_ptrs(const char* what, const float* const* p, int K, PpmPtrs* a) {
  EVK_REQUIRE(p, EVK_E_INVALID, "%s: bad argument (null pointer table)", what);
  *a = PpmPtrs{};
  for (int k = 0; k < K; ++k) {
    EVK_REQUIRE(p[k] && aligned16(p[k]), EVK_E_INVALID, "%s: map %d is a null pointer or off the 16-byte grid", what, k);
    a->p[k] = const_cast<float*>(p[k]);
  }
  return EVK_OK;
}

// What every launcher starts with: the geometry (Cp == 0: the pool side), the K maps as a table and, for a call with a
// workspace (ws_bytes >= 0), its size: the cells of the pool forward, the folded rows of the expand backward.
static int ppm_setup(const char* what, int N, int H, int W, int C, int Cp, const int32_t* bins, int K, const float* const* maps,
                     PpmGeom* g, PpmPtrs* a, int64_t ws_bytes = -1) {
  int rc = ppm_geom(what, N, H, W, C, Cp, bins, K, g);
  if (rc != EVK_OK) return rc;
  rc = ppm_ptrs(what, maps, K, a);
  if (rc != EVK_OK || ws_bytes < 0) return rc;
  const int64_t need = Cp ? ppm_expand_ws_bytes(*g, N, H, Cp) : ppm_pool_ws_bytes(*g, N, C);
  EVK_REQUIRE(ws_bytes >= need, EVK_E_WORKSPACE, "%s: workspace of %lld bytes, %lld are needed (%s)", what, (long long)ws_bytes,
              (long long)need, Cp ? "evk_ppm_expand_bwd_workspace_bytes" : "evk_ppm_pool_workspace_bytes");
  return EVK_OK;
}

}  // namespace evk

using namespace evk;

extern "C" int evk_ppm_plan(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cp, const int32_t* bins, int32_t K,
                            int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "ppm_plan: out is a null pointer");
  PpmGeom g;
  const int rc = ppm_geom("ppm_plan", N, H, W, C, Cp, bins, K, &g);
  if (rc != EVK_OK) return rc;
  const int64_t pws = ppm_pool_ws_bytes(g, N, C), ews = ppm_expand_ws_bytes(g, N, H, Cp);
  EVK_REQUIRE(pws < 0x7fffffffLL && ews < 0x7fffffffLL, EVK_E_UNSUPPORTED, "ppm_plan: workspaces of %lld and %lld bytes",
              (long long)pws, (long long)ews);
  const int nchunk = ceil_div(C, kWave * 4), rchunk = ceil_div((int64_t)K * Cp, kPpmThreads * 4);
  out[0] = 0;                 // kernel form: cells + windows, the only one
  out[1] = 16;                // bytes per load and store
  out[2] = g.ncy; out[3] = g.ncx;
  out[4] = N * g.ncy * nchunk;                                    // pool forward stage 1: workgroups
  out[5] = nchunk;                                                //   of which per cell row (256 channels each)
  out[6] = N * g.sumb2;                                           // pool forward stage 2
  out[7] = N * H * W;                                             // expand forward, pool backward: a workgroup per pixel
  out[8] = N * H * rchunk;                                        // expand backward stage 1
  out[9] = rchunk;                                                //   of which per row (1024 pooled channels each)
  out[10] = ceil_div((int64_t)N * g.sumb * (Cp / 4), kPpmThreads);   // expand backward stage 2
  out[11] = kPpmThreads;
  out[12] = (int32_t)pws; out[13] = (int32_t)ews;
  out[14] = g.sumb; out[15] = g.sumb2;
  return EVK_OK;
}

extern "C" size_t evk_ppm_pool_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, const int32_t* bins, int32_t K) {
  PpmGeom g;
  if (C <= 0 || ppm_geom("ppm_pool_workspace_bytes", N, H, W, C, 0, bins, K, &g) != EVK_OK) return 0;
  return (size_t)ppm_pool_ws_bytes(g, N, C);
}

extern "C" size_t evk_ppm_expand_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cp,
                                                     const int32_t* bins, int32_t K) {
  PpmGeom g;
  if (Cp <= 0 || ppm_geom("ppm_expand_bwd_workspace_bytes", N, H, W, C, Cp, bins, K, &g) != EVK_OK) return 0;
  return (size_t)ppm_expand_ws_bytes(g, N, H, Cp);
}

extern "C" int evk_ppm_pool_fwd(const float* x, float* const* p, const int32_t* bins, int32_t K, int32_t N, int32_t H,
                                int32_t W, int32_t C, void* workspace, size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(x && p && workspace && aligned16(x) && aligned16(workspace) && C > 0, EVK_E_INVALID,
              "ppm_pool_fwd: bad argument (null pointer or a pointer off the 16-byte grid)");
  PpmGeom g;
  PpmPtrs out;
  int rc = ppm_setup("ppm_pool_fwd", N, H, W, C, 0, bins, K, p, &g, &out, (int64_t)workspace_bytes);
  if (rc != EVK_OK) return rc;
  const int nchunk = ceil_div(C, kWave * 4);
  hipStream_t st = (hipStream_t)stream;
  float* cells = (float*)workspace;
  hipLaunchKernelGGL(ppm_cells_kernel, dim3((unsigned)((int64_t)N * g.ncy * nchunk)), dim3(kPpmThreads), 0, st, g, x, cells, H, W,
                     C, nchunk);
  rc = check_launch("ppm_pool_fwd (cells)");
  if (rc != EVK_OK) return rc;
  hipLaunchKernelGGL(ppm_windows_kernel, dim3((unsigned)(N * g.sumb2)), dim3(kPpmThreads), 0, st, g, cells, out, H, W, C);
  return check_launch("ppm_pool_fwd (windows)");
}

extern "C" int evk_ppm_pool_bwd(const float* const* dp, const int32_t* bins, int32_t K, const float* dskip, int32_t ld,
                                float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
  EVK_REQUIRE(dp && dx && aligned16(dx) && aligned16(dskip) && C > 0, EVK_E_INVALID,
              "ppm_pool_bwd: bad argument (null pointer or a pointer off the 16-byte grid)");
  PpmGeom g;
  PpmPtrs in;
  const int rc = ppm_setup("ppm_pool_bwd", N, H, W, C, 0, bins, K, dp, &g, &in);
  if (rc != EVK_OK) return rc;
  EVK_REQUIRE(!dskip || (ld >= C && ld % 4 == 0), EVK_E_INVALID,
              "ppm_pool_bwd: pixel stride %d of the skip gradient (at least C = %d and a multiple of 4)", ld, C);
  EVK_REQUIRE(!dskip || (int64_t)N * H * W * ld < 0x80000000LL, EVK_E_UNSUPPORTED,
              "ppm_pool_bwd: N H W ld = %lld (fewer than 2^31 are implemented)", (long long)((int64_t)N * H * W * ld));
  hipLaunchKernelGGL(ppm_pool_bwd_kernel, dim3((unsigned)((int64_t)N * H * W)), dim3(kPpmThreads), 0, (hipStream_t)stream, g, in,
                     dskip, ld, dx, H, W, C);
  return check_launch("ppm_pool_bwd");
}

extern "C" int evk_ppm_expand_fwd(const float* x, const float* const* z, const int32_t* bins, int32_t K, float* cat, int32_t N,
                                  int32_t H, int32_t W, int32_t C, int32_t Cp, void* stream) {
  EVK_REQUIRE((x || C == 0) && z && cat && aligned16(x) && aligned16(cat) && Cp > 0, EVK_E_INVALID,
              "ppm_expand_fwd: bad argument (null pointer, a pointer off the 16-byte grid or non-positive size)");
  PpmGeom g;
  PpmPtrs in;
  const int rc = ppm_setup("ppm_expand_fwd", N, H, W, C, Cp, bins, K, z, &g, &in);
  if (rc != EVK_OK) return rc;
  hipLaunchKernelGGL(ppm_expand_fwd_kernel, dim3((unsigned)((int64_t)N * H * W)), dim3(kPpmThreads), 0, (hipStream_t)stream, g, x,
                     in, cat, H, W, C, Cp);
  return check_launch("ppm_expand_fwd");
}

extern "C" int evk_ppm_expand_bwd(const float* dcat, float* const* dz, const int32_t* bins, int32_t K, int32_t N, int32_t H,
                                  int32_t W, int32_t C, int32_t Cp, void* workspace, size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(dcat && dz && workspace && aligned16(dcat) && aligned16(workspace) && Cp > 0, EVK_E_INVALID,
              "ppm_expand_bwd: bad argument (null pointer, a pointer off the 16-byte grid or non-positive size)");
  PpmGeom g;
  PpmPtrs out;
  int rc = ppm_setup("ppm_expand_bwd", N, H, W, C, Cp, bins, K, dz, &g, &out, (int64_t)workspace_bytes);
  if (rc != EVK_OK) return rc;
  const int rchunk = ceil_div((int64_t)K * Cp, kPpmThreads * 4);
  hipStream_t st = (hipStream_t)stream;
  float* rows = (float*)workspace;
  hipLaunchKernelGGL(ppm_expand_bwd_rows_kernel, dim3((unsigned)((int64_t)N * H * rchunk)), dim3(kPpmThreads), 0, st, g, dcat,
                     rows, W, C, Cp, rchunk);
  rc = check_launch("ppm_expand_bwd (rows)");
  if (rc != EVK_OK) return rc;
  const int64_t total = (int64_t)N * g.sumb * (Cp / 4);
  hipLaunchKernelGGL(ppm_expand_bwd_cols_kernel, dim3((unsigned)ceil_div(total, kPpmThreads)), dim3(kPpmThreads), 0, st, g, rows,
                     out, (uint32_t)total, H, Cp);
  return check_launch("ppm_expand_bwd (columns)");
}
