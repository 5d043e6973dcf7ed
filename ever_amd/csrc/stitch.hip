// Whole-scene tiled inference, the stitching half (gfx950): adding a batch of window score maps into a scene accumulator and a
// coverage plane, and turning the two into mean scores or a class map (magic/bigimage/scene.py; the gathering half is
// csrc/augment.hip).  It replaces, per window, `out[:, y0:y1, x0:x1] += s; count[y0:y1, x0:x1] += 1` and, per scene,
// `out / count` (+ argmax / threshold) of magic/bigimage/sliding_window.py.
//
// Both dense layouts are one geometry, as in csrc/d4.hip: a map is P planes of rows of RW floats with cpp floats per pixel,
//   NHWC memory      P = 1, cpp = C, RW = W*C      (acc [H,W,C], scores [M,h,w,C])
//   NCHW-contiguous  P = C, cpp = 1, RW = W        (acc [C,H,W], scores [M,C,h,w])
// and window m covers, in rows y0 .. y0+h-1 of every plane, the floats x0*cpp .. (x0+w)*cpp - 1.
//
// stitch_add: ONE OWNER per accumulator element and no atomics.  A wave owns 64 consecutive items (1 or 4 floats each) of one
// row of the bounding box of the launch's windows.  Lane k holds window k's origin and tests it against the wave's segment; the
// ballot is the set of windows that touch the segment, walked from its lowest bit, i.e. in table order, so an element's value
// is ((acc + s_a) + s_b) + ... with a < b < ...: the bits of the sequential `+=` loop (an add has no other rounding to choose).
// An element no window covers is neither read nor written.  The coverage of a pixel is added by the owner of its first float
// in plane 0, as acc + (float)n for n covering windows: equal to n times `+= 1` while the count stays below 2^24.
// The 16-byte form needs every window edge and every row start on the 4-float grid, so a 4-float item lies inside or outside
// a window as a whole: RW % 4 == 0, w*cpp % 4 == 0, x0*cpp % 4 == 0 for every window, pointers on the 16-byte grid.
// Up to 64 windows per launch (one per lane); the launcher chains a longer table in order.
//
// stitch_finalize: one pass.  scores: acc / count, one correctly rounded division per element (0/0 = NaN where nothing was
// added).  labels: per pixel the index of the first maximal QUOTIENT (two sums that differ can round to one quotient, so the
// sums are not compared), a NaN maximal as in torch.argmax; with one class `quotient > threshold`; fill_label where the
// coverage is 0.
// The uint8 / int64 label stores are csrc/common.hpp's, shared with csrc/augment.hip.
// Element offsets are 64-bit everywhere; what is 32-bit is an offset inside one row (RW < 2^31 is required).
#include "common.hpp"

namespace evk {

constexpr int kStitchMaxWindows = 64;    // per launch: one window per lane of the wave that ballots
constexpr int kStitchRecWords = 2;       // int64 words per window: y0, x0
constexpr int kStitchRows = 4;           // rows per workgroup: one per wave

struct StitchPlan {
  int vec;                 // stitch_add: 16-byte items
  int tiles_x, tiles_y;    // workgroups along a row of the bounding box, and down its rows
  int planes;              // grid.y
  int launches;            // ceil(M / 64)
  int by0, bx0, by1, bx1;  // bounding box of the FIRST launch's windows
  int fin_vec;             // stitch_finalize, scores: 16-byte items
  int lab_vec;             // stitch_finalize, labels: 4 pixels per thread (cpp == 1) or 16-byte channel loads (cpp % 4 == 0)
};

static int stitch_check_scene(int C, int H, int W, const char* what) {
  EVK_REQUIRE(C > 0 && H > 0 && W > 0, EVK_E_INVALID, "%s: non-positive size (C %d, H %d, W %d)", what, C, H, W);
  EVK_REQUIRE(C <= 65535, EVK_E_UNSUPPORTED, "%s: %d classes (up to 65535 are implemented)", what, C);
  EVK_REQUIRE((int64_t)W * C < 0x80000000LL, EVK_E_UNSUPPORTED, "%s: a row of %lld floats (fewer than 2^31 are implemented)", what,
              (long long)W * C);
  return EVK_OK;
}

// Every refusal of evk_stitch_add that concerns the table, and the form and grid of the launch that takes windows
// [first, first + n) of it.  Host arithmetic only; shared by evk_stitch_plan and evk_stitch_add.
static int stitch_plan(const int64_t* rec, int first, int n, int C, int H, int W, int h, int w, bool nchw, bool ptrs16,
                       StitchPlan* pl) {
  const int cpp = nchw ? 1 : C;
  bool vec = ptrs16 && ((int64_t)W * cpp) % 4 == 0 && ((int64_t)w * cpp) % 4 == 0;
  int by0 = H, bx0 = W, by1 = 0, bx1 = 0;
  for (int k = first; k < first + n; ++k) {
    const int64_t y0 = rec[(size_t)k * kStitchRecWords], x0 = rec[(size_t)k * kStitchRecWords + 1];
    EVK_REQUIRE(y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W, EVK_E_INVALID,
                "stitch: window %d at (%lld, %lld) of %d x %d is not inside the %d x %d scene", k, (long long)y0, (long long)x0,
                h, w, H, W);
    vec = vec && (x0 * cpp) % 4 == 0;
    by0 = y0 < by0 ? (int)y0 : by0; bx0 = x0 < bx0 ? (int)x0 : bx0;
    by1 = y0 + h > by1 ? (int)y0 + h : by1; bx1 = x0 + w > bx1 ? (int)x0 + w : bx1;
  }
  const int V = vec ? 4 : 1;
  const int64_t items = (int64_t)(bx1 - bx0) * cpp / V;
  pl->vec = vec;
  pl->tiles_x = (int)((items + kWave - 1) / kWave);
  pl->tiles_y = (by1 - by0 + kStitchRows - 1) / kStitchRows;
  pl->planes = nchw ? C : 1;
  pl->by0 = by0; pl->bx0 = bx0; pl->by1 = by1; pl->bx1 = bx1;
  EVK_REQUIRE((int64_t)pl->tiles_x * pl->tiles_y < 0x80000000LL, EVK_E_UNSUPPORTED, "stitch: a grid of %lld workgroups",
              (long long)pl->tiles_x * pl->tiles_y);
  return EVK_OK;
}

struct StitchGeom {
  int H, W, h, w, cpp, P;
  int by0, by1;              // rows of the bounding box
  uint32_t f0, f1;           // its floats inside a row: bx0*cpp .. bx1*cpp
  uint32_t RW, rw;           // floats per scene row and per window row
  FastDiv fTilesX, fCpp;
};

// V floats per item.  Every lane of a wave runs the window loop (the ballot and the lane reads are wave-wide); only the lanes
// whose item lies inside the bounding box touch memory.
template <int V>
__global__ __launch_bounds__(256) void stitch_add_kernel(const long long* __restrict__ table, int M,
                                                         const float* __restrict__ scores, float* __restrict__ acc,
                                                         float* __restrict__ count, const StitchGeom g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t ty = fdiv(blockIdx.x, g.fTilesX), tx = blockIdx.x - ty * g.fTilesX.div;
  const int y = g.by0 + (int)ty * kStitchRows + wave;
  if (y >= g.by1) return;                                   // the whole wave
  const int p = blockIdx.y;
  const uint32_t seg0 = g.f0 + tx * (uint32_t)(kWave * V);  // the wave's floats of row y: seg0 .. seg0 + 64 V - 1
  const uint32_t f = seg0 + (uint32_t)lane * V;
  const bool active = f < g.f1;
  int wy0 = 0, wx0 = 0;
  bool hit = false;
  if (lane < M) {
    wy0 = (int)table[(size_t)lane * kStitchRecWords];
    wx0 = (int)table[(size_t)lane * kStitchRecWords + 1];
    const uint32_t lo = (uint32_t)wx0 * g.cpp;
    hit = y >= wy0 && y < wy0 + g.h && lo < seg0 + (uint32_t)(kWave * V) && lo + g.rw > seg0;
  }
  uint64_t mask = __ballot(hit);
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  int n = 0;
  float* arow = acc + ((size_t)p * g.H + y) * g.RW + f;
  while (mask) {
    const int k = __builtin_ctzll(mask);
    mask &= mask - 1;
    const int ky0 = __builtin_amdgcn_readlane(wy0, k), kx0 = __builtin_amdgcn_readlane(wx0, k);
    const uint32_t lo = (uint32_t)kx0 * g.cpp;
    if (active && f >= lo && f < lo + g.rw) {
      const float* s = scores + (((size_t)k * g.P + p) * g.h + (y - ky0)) * g.rw + (f - lo);
      if (n == 0) {
        if (V == 4) a = *reinterpret_cast<const f32x4*>(arow);
        else a.x = *arow;
      }
      if (V == 4) a = a + *reinterpret_cast<const f32x4*>(s);
      else a.x = a.x + *s;
      ++n;
    }
  }
  if (n == 0) return;
  if (V == 4) *reinterpret_cast<f32x4*>(arow) = a;
  else *arow = a.x;
  if (p != 0) return;
  const float fn = (float)n;
  float* crow = count + (size_t)y * g.W;
  if (g.cpp == 1) {
    if (V == 4) {
      f32x4* c = reinterpret_cast<f32x4*>(crow + f);
      *c = *c + f32x4{fn, fn, fn, fn};
    } else {
      crow[f] = crow[f] + fn;
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const uint32_t pix = fdiv(f + j, g.fCpp);
      if (f + j == pix * (uint32_t)g.cpp) crow[pix] = crow[pix] + fn;
    }
  }
}

struct FinGeom {
  int C, H, W, cpp, P;
  uint32_t RW;
  int label_i64, fill;
  float threshold;
  FastDiv fTilesX, fCpp;
};

// scores: V floats of one row per thread, out = acc / count.  out may be acc: an element is read and written by its one owner.
template <int V>
__global__ __launch_bounds__(256) void stitch_scores_kernel(const float* acc, const float* __restrict__ count, float* out,
                                                            const FinGeom g) {
  const uint32_t y = fdiv(blockIdx.x, g.fTilesX), tx = blockIdx.x - y * g.fTilesX.div;
  const uint32_t f = (tx * 256u + threadIdx.x) * V;
  if (f >= g.RW) return;
  const size_t o = ((size_t)blockIdx.y * g.H + y) * g.RW + f;
  const float* crow = count + (size_t)y * g.W;
  if (V == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(acc + o);
    f32x4 c;
    if (g.cpp == 1) {
      c = *reinterpret_cast<const f32x4*>(crow + f);
    } else if (g.cpp % 4 == 0) {
      const float c0 = crow[fdiv(f, g.fCpp)];
      c = f32x4{c0, c0, c0, c0};
    } else {
      c = f32x4{crow[fdiv(f, g.fCpp)], crow[fdiv(f + 1, g.fCpp)], crow[fdiv(f + 2, g.fCpp)], crow[fdiv(f + 3, g.fCpp)]};
    }
    *reinterpret_cast<f32x4*>(out + o) =
        f32x4{__fdiv_rn(a.x, c.x), __fdiv_rn(a.y, c.y), __fdiv_rn(a.z, c.z), __fdiv_rn(a.w, c.w)};
  } else {
    out[o] = __fdiv_rn(acc[o], crow[g.cpp == 1 ? f : fdiv(f, g.fCpp)]);
  }
}

// first maximal quotient, a NaN maximal (torch.argmax): q replaces the best if it is greater, or a NaN while the best is not
__device__ __forceinline__ void stitch_best(float q, int k, float& best, int& idx) {
  if (q > best || (q != q && best == best)) { best = q; idx = k; }
}

// labels of planar maps (cpp == 1: NCHW-contiguous, or one class): PV consecutive pixels of a row per thread, class k of them
// H*W floats further on.
template <int PV>
__global__ __launch_bounds__(256) void stitch_labels_planar_kernel(const float* __restrict__ acc, const float* __restrict__ count,
                                                                   void* __restrict__ out, const FinGeom g) {
  const uint32_t y = fdiv(blockIdx.x, g.fTilesX), tx = blockIdx.x - y * g.fTilesX.div;
  const uint32_t x = (tx * 256u + threadIdx.x) * PV;
  if (x >= (uint32_t)g.W) return;
  const size_t pix = (size_t)y * g.W + x, plane = (size_t)g.H * g.W;
  float c[PV], best[PV];
  int idx[PV];
  if constexpr (PV == 4) {
    const f32x4 cv = *reinterpret_cast<const f32x4*>(count + pix);
    const f32x4 av = *reinterpret_cast<const f32x4*>(acc + pix);
    c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
    best[0] = av.x; best[1] = av.y; best[2] = av.z; best[3] = av.w;
  } else {
    c[0] = count[pix];
    best[0] = acc[pix];
  }
#pragma unroll
  for (int i = 0; i < PV; ++i) { best[i] = __fdiv_rn(best[i], c[i]); idx[i] = 0; }
  if (g.C == 1) {
#pragma unroll
    for (int i = 0; i < PV; ++i) idx[i] = best[i] > g.threshold ? 1 : 0;
  } else {
    for (int k = 1; k < g.C; ++k) {
      const float* a = acc + (size_t)k * plane + pix;
      if constexpr (PV == 4) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(a);
        const float q[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
        for (int i = 0; i < PV; ++i) stitch_best(__fdiv_rn(q[i], c[i]), k, best[i], idx[i]);
      } else {
        stitch_best(__fdiv_rn(*a, c[0]), k, best[0], idx[0]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PV; ++i)
    if (c[i] == 0.0f) idx[i] = g.fill;
  if constexpr (PV == 4) {
    const long long l[4] = {idx[0], idx[1], idx[2], idx[3]};
    store_labels4(out, g.label_i64, pix, l);
  } else {
    store_label(out, g.label_i64, pix, idx[0]);
  }
}

// labels of NHWC maps with two classes or more: a pixel per thread, its C floats read 1 or 4 at a time
template <int V>
__global__ __launch_bounds__(256) void stitch_labels_pixel_kernel(const float* __restrict__ acc, const float* __restrict__ count,
                                                                  void* __restrict__ out, const FinGeom g) {
  const uint32_t y = fdiv(blockIdx.x, g.fTilesX), tx = blockIdx.x - y * g.fTilesX.div;
  const uint32_t x = tx * 256u + threadIdx.x;
  if (x >= (uint32_t)g.W) return;
  const size_t pix = (size_t)y * g.W + x;
  const float c = count[pix];
  const float* a = acc + pix * g.C;
  float best = 0.0f;
  int idx = 0;
  if (V == 4) {
    for (int k = 0; k < g.C; k += 4) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + k);
      const float q0 = __fdiv_rn(av.x, c), q1 = __fdiv_rn(av.y, c), q2 = __fdiv_rn(av.z, c), q3 = __fdiv_rn(av.w, c);
      if (k == 0) best = q0;
      else stitch_best(q0, k, best, idx);
      stitch_best(q1, k + 1, best, idx);
      stitch_best(q2, k + 2, best, idx);
      stitch_best(q3, k + 3, best, idx);
    }
  } else {
    best = __fdiv_rn(a[0], c);
    for (int k = 1; k < g.C; ++k) stitch_best(__fdiv_rn(a[k], c), k, best, idx);
  }
  store_label(out, g.label_i64, pix, c == 0.0f ? g.fill : idx);
}

static inline bool stitch_fin_vec(int W, int cpp) { return ((int64_t)W * cpp) % 4 == 0; }
static inline bool stitch_lab_vec(int C, int W, bool nchw) { return (nchw || C == 1) ? W % 4 == 0 : C % 4 == 0; }

}  // namespace evk

using namespace evk;

extern "C" int evk_stitch_plan(const int64_t* records, int32_t M, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w,
                               int32_t nchw, int32_t* out) {
  EVK_REQUIRE(records && out, EVK_E_INVALID, "stitch_plan: null pointer");
  EVK_REQUIRE(M >= 1 && h > 0 && w > 0, EVK_E_INVALID, "stitch_plan: bad argument (M %d, window %d x %d)", M, h, w);
  int rc = stitch_check_scene(C, H, W, "stitch_plan");
  if (rc != EVK_OK) return rc;
  StitchPlan pl = {}, rest;
  for (int first = 0; first < M; first += kStitchMaxWindows) {      // every launch's refusals; the numbers of the first
    const int n = M - first < kStitchMaxWindows ? M - first : kStitchMaxWindows;
    rc = stitch_plan(records, first, n, C, H, W, h, w, nchw != 0, true, first ? &rest : &pl);
    if (rc != EVK_OK) return rc;
  }
  const int cpp = nchw ? 1 : C;
  out[0] = pl.vec; out[1] = pl.tiles_x; out[2] = pl.tiles_y; out[3] = pl.planes;
  out[4] = (M + kStitchMaxWindows - 1) / kStitchMaxWindows;
  out[5] = pl.by0; out[6] = pl.bx0; out[7] = pl.by1; out[8] = pl.bx1;
  out[9] = stitch_fin_vec(W, cpp); out[10] = stitch_lab_vec(C, W, nchw != 0); out[11] = 0;
  return EVK_OK;
}

extern "C" int evk_stitch_add(const int64_t* records, const int64_t* table, int32_t M, const float* scores, float* acc,
                              float* count, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, int32_t nchw, void* stream) {
  EVK_REQUIRE(records && table && scores && acc && count, EVK_E_INVALID, "stitch_add: null pointer");
  EVK_REQUIRE(M >= 1 && h > 0 && w > 0, EVK_E_INVALID, "stitch_add: bad argument (M %d, window %d x %d)", M, h, w);
  int rc = stitch_check_scene(C, H, W, "stitch_add");
  if (rc != EVK_OK) return rc;
  const bool ptrs16 = aligned16(scores) && aligned16(acc) && aligned16(count);
  StitchPlan pl;
  for (int first = 0; first < M; first += kStitchMaxWindows) {      // the whole table is checked before the first launch
    const int n = M - first < kStitchMaxWindows ? M - first : kStitchMaxWindows;
    rc = stitch_plan(records, first, n, C, H, W, h, w, nchw != 0, ptrs16, &pl);
    if (rc != EVK_OK) return rc;
  }
  const int cpp = nchw ? 1 : C, P = nchw ? C : 1;
  hipStream_t st = (hipStream_t)stream;
  for (int first = 0; first < M; first += kStitchMaxWindows) {
    const int n = M - first < kStitchMaxWindows ? M - first : kStitchMaxWindows;
    (void)stitch_plan(records, first, n, C, H, W, h, w, nchw != 0, ptrs16, &pl);
    StitchGeom g = {};
    g.H = H; g.W = W; g.h = h; g.w = w; g.cpp = cpp; g.P = P;
    g.by0 = pl.by0; g.by1 = pl.by1;
    g.f0 = (uint32_t)pl.bx0 * cpp; g.f1 = (uint32_t)pl.bx1 * cpp;
    g.RW = (uint32_t)W * cpp; g.rw = (uint32_t)w * cpp;
    g.fTilesX = make_fastdiv((uint32_t)pl.tiles_x); g.fCpp = make_fastdiv((uint32_t)cpp);
    const long long* tab = reinterpret_cast<const long long*>(table) + (size_t)first * kStitchRecWords;
    const float* s = scores + (size_t)first * C * h * w;
    const dim3 grid((unsigned)(pl.tiles_x * pl.tiles_y), (unsigned)P);
    if (pl.vec) hipLaunchKernelGGL(stitch_add_kernel<4>, grid, dim3(256), 0, st, tab, n, s, acc, count, g);
    else hipLaunchKernelGGL(stitch_add_kernel<1>, grid, dim3(256), 0, st, tab, n, s, acc, count, g);
    rc = check_launch("stitch_add");
    if (rc != EVK_OK) return rc;
  }
  return EVK_OK;
}

extern "C" int evk_stitch_finalize(float* acc, const float* count, int32_t C, int32_t H, int32_t W, int32_t nchw, int32_t mode,
                                   void* out, int32_t label_i64, float threshold, int32_t fill_label, void* stream) {
  EVK_REQUIRE(acc && count, EVK_E_INVALID, "stitch_finalize: null pointer");
  EVK_REQUIRE(mode == 0 || mode == 1, EVK_E_INVALID, "stitch_finalize: mode %d (0 scores, 1 labels)", mode);
  EVK_REQUIRE(mode == 0 || out, EVK_E_INVALID, "stitch_finalize: labels need an output");
  int rc = stitch_check_scene(C, H, W, "stitch_finalize");
  if (rc != EVK_OK) return rc;
  const bool i64 = label_i64 != 0;
  if (mode == 1) {
    EVK_REQUIRE(i64 || C <= 256, EVK_E_UNSUPPORTED, "stitch_finalize: %d classes do not fit uint8 labels", C);
    EVK_REQUIRE(i64 || (fill_label >= 0 && fill_label <= 255), EVK_E_INVALID, "stitch_finalize: fill label %d is no uint8", fill_label);
  }
  const bool planar = nchw != 0 || C == 1;
  const int cpp = planar ? 1 : C, P = planar ? C : 1;
  FinGeom g = {};
  g.C = C; g.H = H; g.W = W; g.cpp = cpp; g.P = P; g.RW = (uint32_t)W * cpp;
  g.label_i64 = i64; g.fill = fill_label; g.threshold = threshold;
  g.fCpp = make_fastdiv((uint32_t)cpp);
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0) {
    float* o = out ? reinterpret_cast<float*>(out) : acc;
    const bool vec = stitch_fin_vec(W, cpp) && aligned16(acc) && aligned16(o) && aligned16(count);
    const int64_t tx = ((int64_t)g.RW / (vec ? 4 : 1) + 255) / 256;
    EVK_REQUIRE(tx * H < 0x80000000LL, EVK_E_UNSUPPORTED, "stitch_finalize: a grid of %lld workgroups", (long long)tx * H);
    g.fTilesX = make_fastdiv((uint32_t)tx);
    const dim3 grid((unsigned)(tx * H), (unsigned)P);
    if (vec) hipLaunchKernelGGL(stitch_scores_kernel<4>, grid, dim3(256), 0, st, acc, count, o, g);
    else hipLaunchKernelGGL(stitch_scores_kernel<1>, grid, dim3(256), 0, st, acc, count, o, g);
  } else {
    const bool vec = stitch_lab_vec(C, W, planar) && aligned16(acc) && aligned16(count) && (!planar || aligned16(out));
    const int64_t tx = ((int64_t)W / (planar && vec ? 4 : 1) + 255) / 256;
    EVK_REQUIRE(tx * H < 0x80000000LL, EVK_E_UNSUPPORTED, "stitch_finalize: a grid of %lld workgroups", (long long)tx * H);
    g.fTilesX = make_fastdiv((uint32_t)tx);
    const dim3 grid((unsigned)(tx * H));
    if (planar && vec) hipLaunchKernelGGL(stitch_labels_planar_kernel<4>, grid, dim3(256), 0, st, acc, count, out, g);
    else if (planar) hipLaunchKernelGGL(stitch_labels_planar_kernel<1>, grid, dim3(256), 0, st, acc, count, out, g);
    else if (vec) hipLaunchKernelGGL(stitch_labels_pixel_kernel<4>, grid, dim3(256), 0, st, acc, count, out, g);
    else hipLaunchKernelGGL(stitch_labels_pixel_kernel<1>, grid, dim3(256), 0, st, acc, count, out, g);
  }
  return check_launch("stitch_finalize");
}
