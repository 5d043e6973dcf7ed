// Device-side augmentation and input preparation for a whole batch in one launch (gfx950): the reference's per-image chain
// THRandomRotate90k -> THRandomHorizontalFlip -> THRandomVerticalFlip -> THRandomCrop -> THChannelFirst2 ->
// THMeanStdNormalize2 -> THDivisiblePad (preprocess/thsegm.py, thcomm.py) and torch.stack, with the random draws made on the
// host and handed over as one dihedral op (the 3 bits of csrc/d4.hip: swap | flip_rows << 1 | flip_cols << 2, transpose first,
// then flip) and one crop origin per sample.
//   sample i: S [Hs, Ws, C] uint8 or fp32 at any byte address, an optional label map [Hs, Ws] uint8 or int64, op, (y0, x0)
//   T = d4(S, op), (Ht, Wt) = swap ? (Ws, Hs) : (Hs, Ws);   output pixel (r, c) of the [Ho, Wo] map:
//     r < ch and c < cw (the window): (a, b) = (y0 + r, x0 + c); raw = a < Ht and b < Wt ? T[a, b, :] : 0, label likewise
//                                     (the zero pad of THRandomCrop); value = (float(raw) - mean[k]) / std[k], one rounded
//                                     subtraction and one correctly rounded division, or float(raw) without mean / std
//     else                          : value +0.0f, label mask_pad_value (THDivisiblePad)
// Per-sample records (kAugRecWords int64 each: image address, mask address, Hs, Ws, op, y0, x0, 0) live in a device table; a
// workgroup reads its sample's record by the uniform index blockIdx.y, so nothing is indexed inside a by-value argument.
// Three kernels, every output element and every label written by exactly one thread (no atomics: two runs give the same bits):
//   direct   four consecutive output elements per thread and one 16-byte store (Ho*Wo % 4 == 0, outputs on the 16-byte grid),
//            else an output element per thread.  A non-swap op maps output rows to input rows (reversed at most): both sides
//            run along rows.  A swap op gathers one pixel per input row.
//   tile     a workgroup owns T x T output pixels and stores 16 bytes per thread as well (Wo % 4 == 0), else 4.  A sample with a swap op stages the T x T source pixels they come from
//            through LDS, read along INPUT rows and written along OUTPUT rows, by d4_apply_tile_kernel's own code (the plan,
//            the staging loop and the tile index arithmetic of csrc/d4_tile.hpp); a sample
//            without one reads directly (its rows already run along the output's).  The launch takes this kernel when the plan
//            of any sample names it (evk_augment_plan), as evk_d4_merge does for its terms.
// The tile holds the raw values as fp32 words with row stride S = T*C + pad.  NHWC output: S == C (mod 32), the lanes of a
// 32-lane half run over (cl, k) and read words (al + bl)*C + k (mod 32), consecutive banks (the derivation of d4.hip, with
// the same limits: T*C a multiple of 32).  NCHW output: the lanes run over cl alone and read words al*S + const, so S == 1
// (mod 32) puts them on consecutive banks for every C.  Both are derived, not measured.  The label tile is T x (T + 1) int64.
// Sources are read a byte (uint8) or a word (fp32) at a time: there is no wide-load path, so no alignment is assumed.
// Indices are 32-bit: the entry point refuses a sample or an output of 2^31 elements or more.
// The scaled pass (evk_augment_scale_batch, THRandomScale in front of the chain) is a kernel of its own further down.
#include <string.h>
#include <atomic>
#include "d4_tile.hpp"

namespace evk {

constexpr int kAugRecWords = 8;
constexpr int kAugMaskTile = 32 * 33;  // the label tile, T x (T + 1) int64 with T <= 32

enum AugKernel { kAugDirect = 0, kAugTile = 1 };
enum AugMask { kAugNoMask = 0, kAugMaskU8 = 1, kAugMaskU8ToI64 = 2, kAugMaskI64 = 3 };

struct AugPlan {
  int kernel;
  D4TilePlan tile;   // the image tile; all 0 for the direct kernels
  int vec;       // 16-byte stores (direct: Ho*Wo % 4 == 0, tile: Wo % 4 == 0; the launcher also wants the outputs on the 16-byte grid)
};

// Which swap ops take the tile, measured with tools/bench_augment.py on 16 sources of 1024 x 1024 x C -> 16 x C x 512 x 512 with
// uint8 labels, an MI355X (table in DESIGN 2.16; us per batch, tile against direct):
//   NHWC output: C = 1: 23 / 30, 3: 45 / 68, 4: 55 / 82, 6: 94 / 97, 8: 110 / 106, 16: 271 / 230 (fp32 sources: 3: 47 / 117,
//                4: 57 / 86, 16: 308 / 233)
//   NCHW output: C = 1: 23 / 30, 3: 45 / 55, 4: 55 / 67, 6: 91 / 92, 8: 106 / 116, 16: 274 / 243 (fp32: 3: 46 / 72, 4: 57 / 80,
//                16: 324 / 305)
// So the tile up to the widest pixel at which it was measured ahead, 6 (NHWC) and 8 (NCHW), whatever the source type; the
// widths between the measured ones (5, 7, 9 .. 15) and those above 16 follow their neighbours: derived, not measured.
constexpr int kAugTileNhwcC = 6, kAugTileNchwC = 8;
static inline bool aug_rule_tile(int C, bool nchw) { return C <= (nchw ? kAugTileNchwC : kAugTileNhwcC); }

static std::atomic<int> g_aug_force{-1};      // evk_augment_force_kernel: 0 direct, 1 tile, 2 direct with 4-byte stores only

// One sample's geometry against the launch's: every refusal of evk_augment_batch that concerns a sample, and the kernel its
// (C, dtype, op, layout) takes.  Host arithmetic only; shared by evk_augment_plan and evk_augment_batch.
static int aug_plan(int Hs, int Ws, int C, int op, int y0, int x0, int ch, int cw, int Ho, int Wo, bool src_f32, bool nchw,
                    AugPlan* pl) {
  EVK_REQUIRE(Hs > 0 && Ws > 0 && C > 0 && ch > 0 && cw > 0 && Ho > 0 && Wo > 0 && op >= 0 && op <= 7, EVK_E_INVALID,
              "augment: bad argument (non-positive size or op outside 0..7)");
  EVK_REQUIRE(C <= kTileMaxC, EVK_E_UNSUPPORTED, "augment: %d channels (up to %d are implemented)", C, kTileMaxC);
  EVK_REQUIRE(ch <= Ho && cw <= Wo, EVK_E_INVALID, "augment: crop %d x %d is larger than the output %d x %d", ch, cw, Ho, Wo);
  const int64_t nsrc = (int64_t)Hs * Ws * C;
  EVK_REQUIRE(nsrc < 0x80000000LL, EVK_E_UNSUPPORTED, "augment: a source of %lld elements (fewer than 2^31 are implemented)",
              (long long)nsrc);
  const bool swap = op & 1;
  const int Ht = swap ? Ws : Hs, Wt = swap ? Hs : Ws;
  const int ymax = (Ht > ch ? Ht : ch) - ch, xmax = (Wt > cw ? Wt : cw) - cw;
  EVK_REQUIRE(y0 >= 0 && y0 <= ymax && x0 >= 0 && x0 <= xmax, EVK_E_INVALID,
              "augment: crop origin (%d, %d) outside [0, %d] x [0, %d]", y0, x0, ymax, xmax);
  (void)src_f32;      // measured: the source type does not move the crossover
  int k = swap && aug_rule_tile(C, nchw) ? kAugTile : kAugDirect;
  const int want = g_aug_force.load(std::memory_order_relaxed);
  if (want == kAugDirect || want == 2) k = kAugDirect;
  if (want == kAugTile && swap) k = kAugTile;
  *pl = AugPlan{};
  pl->kernel = k;
  pl->vec = want != 2 && (k == kAugDirect ? ((int64_t)Ho * Wo) % 4 == 0 : Wo % 4 == 0);
  if (k == kAugTile) pl->tile = d4_tile_plan(C, nchw ? 1 : C);
  return EVK_OK;
}

struct AugGeom {
  int ch, cw, Ho, Wo, C;
  int nchw, src_f32, mask_mode, mask_pad;
  int T, S, vec;                 // tile kernel only; vec: 16-byte stores (Wo % 4 == 0, outputs on the 16-byte grid)
  FastDiv fC, fWo, fHW;          // C, Wo, Ho*Wo
  FastDiv fT, fTC, fTT, fTilesC; // T, T*C, T*T, tiles per output row
};

struct AugRec {
  const uint8_t* img;
  const uint8_t* mask;
  int Hs, Ws, op, y0, x0;
};
__device__ __forceinline__ AugRec aug_rec(const long long* __restrict__ table, int n) {
  const long long* t = table + (size_t)n * kAugRecWords;
  AugRec r;
  r.img = reinterpret_cast<const uint8_t*>(t[0]);
  r.mask = reinterpret_cast<const uint8_t*>(t[1]);
  r.Hs = (int)t[2]; r.Ws = (int)t[3]; r.op = (int)t[4]; r.y0 = (int)t[5]; r.x0 = (int)t[6];
  return r;
}

__device__ __forceinline__ float aug_load_raw(const AugRec& rec, const AugGeom& g, uint32_t off) {
  return g.src_f32 ? reinterpret_cast<const float*>(rec.img)[off] : (float)rec.img[off];
}
__device__ __forceinline__ long long aug_load_label(const AugRec& rec, const AugGeom& g, uint32_t pix) {
  return g.mask_mode == kAugMaskI64 ? reinterpret_cast<const long long*>(rec.mask)[pix] : (long long)rec.mask[pix];
}
// one rounded subtraction, one correctly rounded division: the intrinsics keep the compiler from contracting or inverting
__device__ __forceinline__ float aug_normalize(float raw, const float* __restrict__ mean, const float* __restrict__ stdv, int k) {
  return mean ? __fdiv_rn(__fsub_rn(raw, mean[k]), stdv[k]) : raw;
}
__device__ __forceinline__ uint32_t aug_out_offset(const AugGeom& g, int n, int r, int c, int k) {
  return g.nchw ? (((uint32_t)n * g.C + k) * g.Ho + r) * g.Wo + c : (((uint32_t)n * g.Ho + r) * g.Wo + c) * g.C + k;
}
__device__ __forceinline__ bool aug_labels_i64(const AugGeom& g) { return g.mask_mode != kAugMaskU8; }

// Source pixel of window pixel (r, c), or false where the window lies past the source (raw value and label 0 there).
__device__ __forceinline__ bool aug_src_pixel(const AugRec& rec, int r, int c, uint32_t& spix) {
  const int op = rec.op;
  const int Ht = (op & 1) ? rec.Ws : rec.Hs, Wt = (op & 1) ? rec.Hs : rec.Ws;
  const int a = rec.y0 + r, b = rec.x0 + c;
  if (a >= Ht || b >= Wt) return false;
  int sa, sb;
  d4_source(op, a, b, Ht, Wt, sa, sb);
  spix = (uint32_t)sa * rec.Ws + sb;
  return true;
}
// Value of output element (r, c, k) and, on request, the label of its pixel, read from the source directly.
__device__ __forceinline__ float aug_value(const AugRec& rec, const AugGeom& g, const float* __restrict__ mean,
                                           const float* __restrict__ stdv, int r, int c, int k) {
  if (r >= g.ch || c >= g.cw) return 0.0f;
  uint32_t spix;
  const float raw = aug_src_pixel(rec, r, c, spix) ? aug_load_raw(rec, g, spix * g.C + k) : 0.0f;
  return aug_normalize(raw, mean, stdv, k);
}
__device__ __forceinline__ long long aug_label(const AugRec& rec, const AugGeom& g, int r, int c) {
  if (r >= g.ch || c >= g.cw) return g.mask_pad;
  uint32_t spix;
  return aug_src_pixel(rec, r, c, spix) ? aug_load_label(rec, g, spix) : 0;
}

// An output element per thread (4-byte stores): any output size, any output address.
__global__ __launch_bounds__(256) void augment_direct_kernel(const long long* __restrict__ table, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, float* __restrict__ out,
                                                             void* __restrict__ out_mask, const AugGeom g) {
  const int n = blockIdx.y;
  const uint32_t HW = g.fHW.div, j = blockIdx.x * 256u + threadIdx.x;
  if (j >= HW * g.C) return;
  const AugRec rec = aug_rec(table, n);
  uint32_t pix, k;
  if (g.nchw) { k = fdiv(j, g.fHW); pix = j - k * HW; }
  else { pix = fdiv(j, g.fC); k = j - pix * g.C; }
  const uint32_t r = fdiv(pix, g.fWo), c = pix - r * g.Wo;
  out[(uint32_t)n * HW * g.C + j] = aug_value(rec, g, mean, stdv, r, c, k);
  if (g.mask_mode != kAugNoMask && k == 0)
    store_label(out_mask, aug_labels_i64(g), (uint32_t)n * HW + pix, aug_label(rec, g, r, c));
}

// Four consecutive output elements per thread, one 16-byte store (Ho*Wo a multiple of 4, outputs on the 16-byte grid): with a
// 4-byte store per thread the pass is bound by the number of store instructions, not by bytes (table in DESIGN 2.16).  The
// labels are work items of their own after the image's, four consecutive pixels each: one 4-byte store of uint8 labels or two
// 16-byte stores of int64 ones (store_labels4).  Sources are still read element by element, at any address.
__global__ __launch_bounds__(256) void augment_direct_vec_kernel(const long long* __restrict__ table, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, float* __restrict__ out,
                                                                 void* __restrict__ out_mask, const AugGeom g) {
  const int n = blockIdx.y;
  const uint32_t HW = g.fHW.div, nimg = HW * g.C / 4, nlab = g.mask_mode != kAugNoMask ? HW / 4 : 0;
  const uint32_t item = blockIdx.x * 256u + threadIdx.x;
  if (item >= nimg + nlab) return;
  const AugRec rec = aug_rec(table, n);
  if (item < nimg) {
    const uint32_t j = item * 4;
    uint32_t pix, k;
    if (g.nchw) { k = fdiv(j, g.fHW); pix = j - k * HW; }
    else { pix = fdiv(j, g.fC); k = j - pix * g.C; }
    uint32_t r = fdiv(pix, g.fWo), c = pix - r * g.Wo;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = aug_value(rec, g, mean, stdv, r, c, k);
      // the next element in memory order
      if (g.nchw) {
        if (++c == (uint32_t)g.Wo) { c = 0; if (++r == (uint32_t)g.Ho) { r = 0; ++k; } }
      } else {
        if (++k == (uint32_t)g.C) { k = 0; if (++c == (uint32_t)g.Wo) { c = 0; ++r; } }
      }
    }
    *reinterpret_cast<f32x4*>(out + (size_t)n * HW * g.C + j) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    const uint32_t pix = (item - nimg) * 4;
    uint32_t r = fdiv(pix, g.fWo), c = pix - r * g.Wo;
    long long l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      l[i] = aug_label(rec, g, r, c);
      if (++c == (uint32_t)g.Wo) { c = 0; ++r; }
    }
    store_labels4(out_mask, aug_labels_i64(g), (size_t)n * HW + pix, l);
  }
}

// ---- the tile kernel.  Element e of a workgroup's T x T output tile is (rl, cl, k) in the output's own memory order.
__device__ __forceinline__ D4TileElem aug_tile_decode(int e, const AugGeom& g) {
  return g.nchw ? d4_tile_decode_planar(e, g.T, g.fTT, g.fT) : d4_tile_decode(e, g.T, g.C, g.fTC, g.fC);
}
// Value and label of tile pixel (rl, cl) of the tile at (r0, c0): from the staged tiles inside the window, else read directly.
__device__ __forceinline__ float aug_tile_value(const uint32_t* tile, bool staged, const AugRec& rec, const AugGeom& g,
                                                const float* __restrict__ mean, const float* __restrict__ stdv, int r0, int c0,
                                                int rl, int cl, int k) {
  const int r = r0 + rl, c = c0 + cl;
  if (staged && r < g.ch && c < g.cw)
    return aug_normalize(__uint_as_float(tile[d4_tile_word(rec.op, g.T, g.S, g.C, rl, cl, k)]), mean, stdv, k);
  return aug_value(rec, g, mean, stdv, r, c, k);
}
__device__ __forceinline__ long long aug_tile_label(const long long* mtile, bool staged, const AugRec& rec, const AugGeom& g,
                                                    int r0, int c0, int rl, int cl) {
  const int r = r0 + rl, c = c0 + cl;
  if (staged && r < g.ch && c < g.cw) return mtile[d4_tile_word(rec.op, g.T, g.T + 1, 1, rl, cl, 0)];
  return aug_label(rec, g, r, c);
}

__global__ __launch_bounds__(256) void augment_tile_kernel(const long long* __restrict__ table, const float* __restrict__ mean,
                                                           const float* __restrict__ stdv, float* __restrict__ out,
                                                           void* __restrict__ out_mask, const AugGeom g) {
  __shared__ uint32_t tile[kTileFloats];      // the raw values as fp32 words
  __shared__ long long mtile[kAugMaskTile];
  const int n = blockIdx.y;
  const AugRec rec = aug_rec(table, n);
  const int T = g.T, nel = T * T * g.C, op = rec.op;
  const uint32_t tr = fdiv(blockIdx.x, g.fTilesC);
  const int r0 = (int)tr * T, c0 = (int)(blockIdx.x - tr * g.fTilesC.div) * T;
  const bool masks = g.mask_mode != kAugNoMask;
  // uniform over the workgroup (one sample, one tile): so is the barrier
  const bool staged = (op & 1) && r0 < g.ch && c0 < g.cw;
  if (staged) {
    // The tile's origin in d4(S, op) is the crop origin further on; what lies outside the source is stored as 0, which is the
    // raw value the window has there.
    d4_tile_stage<kTilePerThread>(tile, op, T, g.C, g.S, g.fTC, rec.y0 + r0, rec.x0 + c0, rec.Hs, rec.Ws,
                                  [&](uint32_t o) { return __float_as_uint(aug_load_raw(rec, g, o)); });
    if (masks)      // the label tile: one-word pixels, T * T <= 4 * 256 of them
      d4_tile_stage<4>(mtile, op, T, 1, T + 1, g.fT, rec.y0 + r0, rec.x0 + c0, rec.Hs, rec.Ws,
                       [&](uint32_t o) { return aug_load_label(rec, g, o); });
  }
  __syncthreads();
  if (g.vec) {
    // Four consecutive elements of one tile row per thread (T and T*C are multiples of 4, and so is Wo: a quad lies inside the
    // map or outside it as a whole), one 16-byte store.  The four LDS reads of a lane are 4 words apart from its neighbour's:
    // a 4-way bank conflict, derived and accepted — the tile's LDS traffic is a few percent of the kernel's time.
#pragma unroll
    for (int i = 0; i < kTilePerThread / 4; ++i) {
      const int e = (threadIdx.x + 256 * i) * 4;
      if (e < nel) {
        const D4TileElem t = aug_tile_decode(e, g);
        int rl = t.rl, cl = t.cl, k = t.ch;
        const int r = r0 + rl;
        if (r < g.Ho && c0 + cl < g.Wo) {
          const uint32_t off = aug_out_offset(g, n, r, c0 + cl, k);
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            v[q] = aug_tile_value(tile, staged, rec, g, mean, stdv, r0, c0, rl, cl, k);
            if (g.nchw) ++cl;
            else if (++k == g.C) { k = 0; ++cl; }
          }
          *reinterpret_cast<f32x4*>(out + off) = f32x4{v[0], v[1], v[2], v[3]};
        }
      }
    }
    const int e = threadIdx.x * 4;      // the labels: four consecutive pixels of one tile row
    if (masks && e < T * T) {
      const int rl = (int)fdiv((uint32_t)e, g.fT), r = r0 + rl;
      int cl = e - rl * T;
      if (r < g.Ho && c0 + cl < g.Wo) {
        const size_t o = ((size_t)n * g.Ho + r) * g.Wo + c0 + cl;
        long long l[4];
#pragma unroll
        for (int q = 0; q < 4; ++q, ++cl) l[q] = aug_tile_label(mtile, staged, rec, g, r0, c0, rl, cl);
        store_labels4(out_mask, aug_labels_i64(g), o, l);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < kTilePerThread; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < nel) {
      const D4TileElem t = aug_tile_decode(e, g);
      const int rl = t.rl, cl = t.cl, k = t.ch, r = r0 + rl, c = c0 + cl;
      if (r < g.Ho && c < g.Wo) {
        out[aug_out_offset(g, n, r, c, k)] = aug_tile_value(tile, staged, rec, g, mean, stdv, r0, c0, rl, cl, k);
        if (masks && k == 0)
          store_label(out_mask, aug_labels_i64(g), ((uint32_t)n * g.Ho + r) * g.Wo + c,
                      aug_tile_label(mtile, staged, rec, g, r0, c0, rl, cl));
      }
    }
  }
}

// ---- the scaled pass (evk_augment_scale_batch): THRandomScale in front of the chain.  T = d4(Z, op) with Z [Hz, Wz, C] the
// bilinear (align_corners) image of S and the nearest image of its label map, neither of which is ever stored: an output pixel
// decodes its Z pixel (d4_source), from it four clamped source pixels and four weights, and its label's source pixel, ONCE,
// and its C channels share them.  So a thread owns whole pixels: four consecutive ones with 16-byte stores (NCHW: one store
// per channel; NHWC: their 4 C consecutive floats as C stores), else one.  Taps are byte or dword loads at any address; the
// four taps of neighbouring lanes share cache lines and there is no LDS form.  The transposing ops pay for that: measured on
// an MI355X at 191-197 us against 42-50 us for the others (16 x 1024^2 x 3 -> 16 x 3 x 512^2, f = 1.25; table in DESIGN 2.16).
// Records are kAugScaleRecWords int64: the eight above, then Hz, Wz, the bit image of s = float(1 / f), 0.
constexpr int kAugScaleRecWords = 12;

struct AugScaleRec {
  AugRec r;
  int Hz, Wz;
  float s, ry, rx;
  bool scaled;      // false: Hz == Hs, Wz == Ws, s == 1: Z is S itself, one tap
};
__host__ __device__ __forceinline__ float aug_scale_ratio(int src, int dst) {
  if (dst <= 1) return 0.0f;      // one correctly rounded division on either side
#ifdef __HIP_DEVICE_COMPILE__
  return __fdiv_rn((float)(src - 1), (float)(dst - 1));
#else
  return (float)(src - 1) / (float)(dst - 1);
#endif
}
__device__ __forceinline__ AugScaleRec aug_scale_rec(const long long* __restrict__ table, int n) {
  const long long* t = table + (size_t)n * kAugScaleRecWords;
  AugScaleRec q;
  q.r.img = reinterpret_cast<const uint8_t*>(t[0]);
  q.r.mask = reinterpret_cast<const uint8_t*>(t[1]);
  q.r.Hs = (int)t[2]; q.r.Ws = (int)t[3]; q.r.op = (int)t[4]; q.r.y0 = (int)t[5]; q.r.x0 = (int)t[6];
  q.Hz = (int)t[8]; q.Wz = (int)t[9];
  q.s = __uint_as_float((uint32_t)t[10]);
  q.ry = aug_scale_ratio(q.r.Hs, q.Hz);
  q.rx = aug_scale_ratio(q.r.Ws, q.Wz);
  q.scaled = !(q.Hz == q.r.Hs && q.Wz == q.r.Ws && q.s == 1.0f);
  return q;
}

// What the C channels of one output pixel share.  kind 0: outside the window (+0.0f, the pad label); 1: inside the window, past
// T (raw 0, label 0); 2: one tap at o00 (an unscaled sample); 3: four taps.  Offsets are in source pixels.
struct AugScalePix {
  int kind;
  uint32_t o00, o01, o10, o11, lab;
  float hy, ly, hx, lx;
};
// Every operation of the contract is rounded on its own.  The compiler contracts a * b + c into one fma by default, and the
// __fmul_rn / __fadd_rn intrinsics do not stop it (they are plain operators that inherit the default), so the sums below are
// written under `fp contract(off)`: an addition compiled there carries no permission to fuse.
// one axis: the first tap, whether a second one follows it, and the weights
__device__ __forceinline__ void aug_scale_axis(float ratio, int z, int n, int& i0, int& step, float& lo, float& hi) {
#pragma clang fp contract(off)
  const float pos = ratio * (float)z;
  i0 = min((int)pos, n - 1);
  step = i0 < n - 1;
  lo = pos - (float)i0;
  hi = 1.0f - lo;
}
__device__ __forceinline__ AugScalePix aug_scale_pixel(const AugScaleRec& q, const AugGeom& g, int r, int c) {
  AugScalePix p = {};
  if (r >= g.ch || c >= g.cw) return p;
  const int op = q.r.op;
  const int Ht = (op & 1) ? q.Wz : q.Hz, Wt = (op & 1) ? q.Hz : q.Wz;
  const int a = q.r.y0 + r, b = q.r.x0 + c;
  p.kind = 1;
  if (a >= Ht || b >= Wt) return p;
  int za, zb;
  d4_source(op, a, b, Ht, Wt, za, zb);
  const int Hs = q.r.Hs, Ws = q.r.Ws;
  if (!q.scaled) {
    p.kind = 2;
    p.o00 = p.lab = (uint32_t)za * Ws + zb;
    return p;
  }
  p.kind = 3;
  int y0, ys, x0, xs;
  aug_scale_axis(q.ry, za, Hs, y0, ys, p.ly, p.hy);
  aug_scale_axis(q.rx, zb, Ws, x0, xs, p.lx, p.hx);
  p.o00 = (uint32_t)y0 * Ws + x0;
  p.o01 = p.o00 + xs;
  p.o10 = p.o00 + (ys ? Ws : 0);
  p.o11 = p.o10 + xs;
  // a >= 0 and s > 0: the truncation is floorf; a product past the int range saturates and the clamp takes it
  const int my = min((int)((float)za * q.s), Hs - 1), mx = min((int)((float)zb * q.s), Ws - 1);
  p.lab = (uint32_t)my * Ws + mx;
  return p;
}
__device__ __forceinline__ float aug_scale_value(const AugScaleRec& q, const AugGeom& g, const float* __restrict__ mean,
                                                 const float* __restrict__ stdv, const AugScalePix& p, int k) {
#pragma clang fp contract(off)
  if (p.kind == 0) return 0.0f;
  float raw = 0.0f;
  if (p.kind == 2) raw = aug_load_raw(q.r, g, p.o00 * g.C + k);
  if (p.kind == 3) {
    const float p00 = aug_load_raw(q.r, g, p.o00 * g.C + k), p01 = aug_load_raw(q.r, g, p.o01 * g.C + k);
    const float p10 = aug_load_raw(q.r, g, p.o10 * g.C + k), p11 = aug_load_raw(q.r, g, p.o11 * g.C + k);
    const float top = p.hx * p00 + p.lx * p01;
    const float bot = p.hx * p10 + p.lx * p11;
    raw = p.hy * top + p.ly * bot;
  }
  return aug_normalize(raw, mean, stdv, k);
}
__device__ __forceinline__ long long aug_scale_label(const AugScaleRec& q, const AugGeom& g, const AugScalePix& p) {
  return p.kind == 0 ? g.mask_pad : p.kind == 1 ? 0 : aug_load_label(q.r, g, p.lab);
}
// PIX = 4: four consecutive output pixels per thread and 16-byte stores (Ho*Wo a multiple of 4, outputs on the 16-byte grid);
// PIX = 1: a pixel per thread, 4-byte stores, any size and address.
template <int PIX>
__global__ __launch_bounds__(256) void augment_scale_kernel(const long long* __restrict__ table, const float* __restrict__ mean,
                                                            const float* __restrict__ stdv, float* __restrict__ out,
                                                            void* __restrict__ out_mask, const AugGeom g) {
  const int n = blockIdx.y;
  const uint32_t HW = g.fHW.div, pix = (blockIdx.x * 256u + threadIdx.x) * PIX;
  if (pix >= HW) return;
  const AugScaleRec q = aug_scale_rec(table, n);
  uint32_t r = fdiv(pix, g.fWo), c = pix - r * g.Wo;
  AugScalePix p[PIX];
#pragma unroll
  for (int i = 0; i < PIX; ++i) {
    p[i] = aug_scale_pixel(q, g, (int)r, (int)c);
    if (++c == (uint32_t)g.Wo) { c = 0; ++r; }
  }
  const uint32_t C = g.C;
  if constexpr (PIX == 1) {
    for (uint32_t k = 0; k < C; ++k)
      out[g.nchw ? ((uint32_t)n * C + k) * HW + pix : ((uint32_t)n * HW + pix) * C + k] = aug_scale_value(q, g, mean, stdv, p[0], k);
    if (g.mask_mode != kAugNoMask) store_label(out_mask, aug_labels_i64(g), (uint32_t)n * HW + pix, aug_scale_label(q, g, p[0]));
  } else {
    if (g.nchw) {
      for (uint32_t k = 0; k < C; ++k) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = aug_scale_value(q, g, mean, stdv, p[i], k);
        *reinterpret_cast<f32x4*>(out + ((size_t)n * C + k) * HW + pix) = f32x4{v[0], v[1], v[2], v[3]};
      }
    } else {
      float* o = out + ((size_t)n * HW + pix) * C;      // 4 C floats from a multiple of 4 C: on the 16-byte grid
      // pixel-major, so each pixel's registers are named at compile time; element m goes to slot m % 4 of the pending store by
      // selects (an indexed array would go to scratch), and m is the same in every lane: the store is uniform
      float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        for (uint32_t k = 0; k < C; ++k, ++m) {
          const float val = aug_scale_value(q, g, mean, stdv, p[i], k);
          const uint32_t slot = m & 3u;
          if (slot == 3u) reinterpret_cast<f32x4*>(o)[m >> 2] = f32x4{v0, v1, v2, val};
          v0 = slot == 0u ? val : v0;
          v1 = slot == 1u ? val : v1;
          v2 = slot == 2u ? val : v2;
        }
      }
    }
    if (g.mask_mode != kAugNoMask) {
      long long l[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) l[i] = aug_scale_label(q, g, p[i]);
      store_labels4(out_mask, aug_labels_i64(g), (size_t)n * HW + pix, l);
    }
  }
}

// One sample of the scaled pass against the launch: every refusal that concerns a sample.  Host arithmetic only.
static int aug_scale_plan(int Hs, int Ws, int C, int op, int y0, int x0, int ch, int cw, int Ho, int Wo, int Hz, int Wz,
                          uint32_t s_bits, AugPlan* pl) {
  EVK_REQUIRE(Hs > 0 && Ws > 0 && C > 0 && ch > 0 && cw > 0 && Ho > 0 && Wo > 0 && op >= 0 && op <= 7, EVK_E_INVALID,
              "augment_scale: bad argument (non-positive size or op outside 0..7)");
  EVK_REQUIRE(C <= kTileMaxC, EVK_E_UNSUPPORTED, "augment_scale: %d channels (up to %d are implemented)", C, kTileMaxC);
  EVK_REQUIRE(ch <= Ho && cw <= Wo, EVK_E_INVALID, "augment_scale: crop %d x %d is larger than the output %d x %d", ch, cw, Ho, Wo);
  const int64_t nsrc = (int64_t)Hs * Ws * C;
  EVK_REQUIRE(nsrc < 0x80000000LL, EVK_E_UNSUPPORTED, "augment_scale: a source of %lld elements (fewer than 2^31 are implemented)",
              (long long)nsrc);
  EVK_REQUIRE(Hz >= 1 && Wz >= 1, EVK_E_INVALID, "augment_scale: scaled size %d x %d", Hz, Wz);
  const int64_t nz = (int64_t)Hz * Wz * C;
  EVK_REQUIRE(nz < 0x80000000LL, EVK_E_UNSUPPORTED, "augment_scale: a scaled image of %lld elements (fewer than 2^31 are implemented)",
              (long long)nz);
  // finite and positive: sign 0, exponent not all ones, not zero
  EVK_REQUIRE(s_bits != 0 && s_bits < 0x7f800000u, EVK_E_INVALID, "augment_scale: 1 / factor (bits 0x%08x) is not finite and positive",
              s_bits);
  const bool swap = op & 1;
  const int Ht = swap ? Wz : Hz, Wt = swap ? Hz : Wz;
  const int ymax = (Ht > ch ? Ht : ch) - ch, xmax = (Wt > cw ? Wt : cw) - cw;
  EVK_REQUIRE(y0 >= 0 && y0 <= ymax && x0 >= 0 && x0 <= xmax, EVK_E_INVALID,
              "augment_scale: crop origin (%d, %d) outside [0, %d] x [0, %d]", y0, x0, ymax, xmax);
  *pl = AugPlan{};
  pl->kernel = kAugDirect;
  pl->vec = g_aug_force.load(std::memory_order_relaxed) != 2 && ((int64_t)Ho * Wo) % 4 == 0;
  return EVK_OK;
}

}  // namespace evk

using namespace evk;

extern "C" int evk_augment_plan(int32_t Hs, int32_t Ws, int32_t C, int32_t op, int32_t y0, int32_t x0, int32_t crop_h,
                                int32_t crop_w, int32_t Ho, int32_t Wo, int32_t src_f32, int32_t nchw, int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "augment_plan: out is a null pointer");
  AugPlan pl;
  const int rc = aug_plan(Hs, Ws, C, op, y0, x0, crop_h, crop_w, Ho, Wo, src_f32 != 0, nchw != 0, &pl);
  if (rc != EVK_OK) return rc;
  const D4TilePlan& t = pl.tile;      // the LDS of the tile kernel: the image tile and the label tile
  out[0] = pl.kernel; out[1] = t.T; out[2] = t.S; out[4] = t.per_thread; out[5] = pl.vec;
  out[3] = pl.kernel == kAugTile ? t.lds_floats * (int)sizeof(float) + kAugMaskTile * (int)sizeof(long long) : 0;
  return EVK_OK;
}

extern "C" int evk_augment_force_kernel(int32_t kernel) {
  return g_aug_force.exchange(kernel >= 0 && kernel <= 2 ? kernel : -1, std::memory_order_relaxed);
}

extern "C" int evk_augment_batch(const int64_t* records, const int64_t* table, int32_t N, int32_t C, int32_t crop_h,
                                 int32_t crop_w, int32_t Ho, int32_t Wo, const float* mean, const float* stdv,
                                 int32_t mask_pad_value, int32_t nchw, int32_t src_f32, int32_t mask_mode, float* out,
                                 void* out_mask, void* stream) {
  EVK_REQUIRE(records && table, EVK_E_INVALID, "augment_batch: null record table");
  EVK_REQUIRE(out && N > 0, EVK_E_INVALID, "augment_batch: bad argument (null output or non-positive batch)");
  EVK_REQUIRE((mean == nullptr) == (stdv == nullptr), EVK_E_INVALID, "augment_batch: mean and std come together or not at all");
  EVK_REQUIRE(mask_mode >= kAugNoMask && mask_mode <= kAugMaskI64, EVK_E_INVALID, "augment_batch: mask mode %d outside 0..3",
              mask_mode);
  EVK_REQUIRE(mask_mode == kAugNoMask || out_mask, EVK_E_INVALID, "augment_batch: a mask mode without a mask output");
  AugPlan pl, tile_pl = {};
  bool any_tile = false;
  for (int i = 0; i < N; ++i) {
    const int64_t* r = records + (size_t)i * kAugRecWords;
    EVK_REQUIRE(r[0] != 0, EVK_E_INVALID, "augment_batch: image %d is a null pointer", i);
    EVK_REQUIRE(mask_mode == kAugNoMask || r[1] != 0, EVK_E_INVALID, "augment_batch: mask %d is a null pointer", i);
    for (int k = 2; k < 7; ++k)
      EVK_REQUIRE(r[k] >= 0 && r[k] < 0x80000000LL, EVK_E_INVALID, "augment_batch: record %d, word %d out of range", i, k);
    const int rc = aug_plan((int)r[2], (int)r[3], C, (int)r[4], (int)r[5], (int)r[6], crop_h, crop_w, Ho, Wo, src_f32 != 0,
                            nchw != 0, &pl);
    if (rc != EVK_OK) return rc;
    if (pl.kernel == kAugTile) { any_tile = true; tile_pl = pl; }
  }
  const int64_t total = (int64_t)N * Ho * Wo * C;
  EVK_REQUIRE(total < 0x80000000LL, EVK_E_UNSUPPORTED, "augment_batch: an output of %lld elements (fewer than 2^31 are implemented)",
              (long long)total);
  EVK_REQUIRE(N <= 65535, EVK_E_UNSUPPORTED, "augment_batch: %d samples (up to 65535 per launch)", N);
  AugGeom g = {};
  g.ch = crop_h; g.cw = crop_w; g.Ho = Ho; g.Wo = Wo; g.C = C;
  g.nchw = nchw != 0; g.src_f32 = src_f32 != 0; g.mask_mode = mask_mode; g.mask_pad = mask_pad_value;
  g.fC = make_fastdiv((uint32_t)C); g.fWo = make_fastdiv((uint32_t)Wo); g.fHW = make_fastdiv((uint32_t)(Ho * Wo));
  g.fT = g.fTC = g.fTT = g.fTilesC = make_fastdiv(1);
  hipStream_t st = (hipStream_t)stream;
  const long long* tab = reinterpret_cast<const long long*>(table);
  const bool wide_ok = g_aug_force.load(std::memory_order_relaxed) != 2 && aligned16(out) &&
                       (mask_mode == kAugNoMask || aligned16(out_mask));
  if (any_tile) {
    const int T = tile_pl.tile.T, tr = (Ho + T - 1) / T, tc = (Wo + T - 1) / T;
    g.T = T; g.S = tile_pl.tile.S; g.vec = wide_ok && Wo % 4 == 0;
    g.fT = make_fastdiv((uint32_t)T); g.fTC = make_fastdiv((uint32_t)(T * C)); g.fTT = make_fastdiv((uint32_t)(T * T));
    g.fTilesC = make_fastdiv((uint32_t)tc);
    hipLaunchKernelGGL(augment_tile_kernel, dim3((unsigned)(tr * tc), (unsigned)N), dim3(256), 0, st, tab, mean, stdv, out,
                       out_mask, g);
  } else {
    const int64_t hw = (int64_t)Ho * Wo;
    if (wide_ok && hw % 4 == 0) {
      const int64_t items = hw * C / 4 + (mask_mode != kAugNoMask ? hw / 4 : 0);
      hipLaunchKernelGGL(augment_direct_vec_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)N), dim3(256), 0, st, tab, mean,
                         stdv, out, out_mask, g);
    } else {
      hipLaunchKernelGGL(augment_direct_kernel, dim3((unsigned)((hw * C + 255) / 256), (unsigned)N), dim3(256), 0, st, tab, mean,
                         stdv, out, out_mask, g);
    }
  }
  return check_launch("augment_batch");
}

extern "C" int evk_augment_scale_plan(int32_t Hs, int32_t Ws, int32_t C, int32_t op, int32_t y0, int32_t x0, int32_t crop_h,
                                      int32_t crop_w, int32_t Ho, int32_t Wo, int32_t src_f32, int32_t nchw, int32_t Hz, int32_t Wz,
                                      int32_t s_bits, int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "augment_scale_plan: out is a null pointer");
  (void)src_f32; (void)nchw;      // one kernel form for every source type and layout
  AugPlan pl;
  const int rc = aug_scale_plan(Hs, Ws, C, op, y0, x0, crop_h, crop_w, Ho, Wo, Hz, Wz, (uint32_t)s_bits, &pl);
  if (rc != EVK_OK) return rc;
  const float ry = aug_scale_ratio(Hs, Hz), rx = aug_scale_ratio(Ws, Wz);
  out[0] = pl.kernel; out[1] = (pl.vec ? 4 : 1) * C; out[2] = pl.vec;
  memcpy(&out[3], &ry, sizeof(float));
  memcpy(&out[4], &rx, sizeof(float));
  return EVK_OK;
}

extern "C" int evk_augment_scale_batch(const int64_t* records, const int64_t* table, int32_t N, int32_t C, int32_t crop_h,
                                       int32_t crop_w, int32_t Ho, int32_t Wo, const float* mean, const float* stdv,
                                       int32_t mask_pad_value, int32_t nchw, int32_t src_f32, int32_t mask_mode, float* out,
                                       void* out_mask, void* stream) {
  EVK_REQUIRE(records && table, EVK_E_INVALID, "augment_scale_batch: null record table");
  EVK_REQUIRE(out && N > 0, EVK_E_INVALID, "augment_scale_batch: bad argument (null output or non-positive batch)");
  EVK_REQUIRE((mean == nullptr) == (stdv == nullptr), EVK_E_INVALID, "augment_scale_batch: mean and std come together or not at all");
  EVK_REQUIRE(mask_mode >= kAugNoMask && mask_mode <= kAugMaskI64, EVK_E_INVALID, "augment_scale_batch: mask mode %d outside 0..3",
              mask_mode);
  EVK_REQUIRE(mask_mode == kAugNoMask || out_mask, EVK_E_INVALID, "augment_scale_batch: a mask mode without a mask output");
  AugPlan pl;
  for (int i = 0; i < N; ++i) {
    const int64_t* r = records + (size_t)i * kAugScaleRecWords;
    EVK_REQUIRE(r[0] != 0, EVK_E_INVALID, "augment_scale_batch: image %d is a null pointer", i);
    EVK_REQUIRE(mask_mode == kAugNoMask || r[1] != 0, EVK_E_INVALID, "augment_scale_batch: mask %d is a null pointer", i);
    for (int k = 2; k < 10; ++k)
      EVK_REQUIRE(k == 7 || (r[k] >= 0 && r[k] < 0x80000000LL), EVK_E_INVALID, "augment_scale_batch: record %d, word %d out of range",
                  i, k);
    EVK_REQUIRE(r[10] >= 0 && r[10] <= 0xffffffffLL, EVK_E_INVALID, "augment_scale_batch: record %d, word 10 out of range", i);
    const int rc = aug_scale_plan((int)r[2], (int)r[3], C, (int)r[4], (int)r[5], (int)r[6], crop_h, crop_w, Ho, Wo, (int)r[8],
                                  (int)r[9], (uint32_t)r[10], &pl);
    if (rc != EVK_OK) return rc;
  }
  const int64_t total = (int64_t)N * Ho * Wo * C;
  EVK_REQUIRE(total < 0x80000000LL, EVK_E_UNSUPPORTED,
              "augment_scale_batch: an output of %lld elements (fewer than 2^31 are implemented)", (long long)total);
  EVK_REQUIRE(N <= 65535, EVK_E_UNSUPPORTED, "augment_scale_batch: %d samples (up to 65535 per launch)", N);
  AugGeom g = {};
  g.ch = crop_h; g.cw = crop_w; g.Ho = Ho; g.Wo = Wo; g.C = C;
  g.nchw = nchw != 0; g.src_f32 = src_f32 != 0; g.mask_mode = mask_mode; g.mask_pad = mask_pad_value;
  g.fC = make_fastdiv((uint32_t)C); g.fWo = make_fastdiv((uint32_t)Wo); g.fHW = make_fastdiv((uint32_t)(Ho * Wo));
  g.fT = g.fTC = g.fTT = g.fTilesC = make_fastdiv(1);
  hipStream_t st = (hipStream_t)stream;
  const long long* tab = reinterpret_cast<const long long*>(table);
  const int64_t hw = (int64_t)Ho * Wo;
  if (pl.vec && aligned16(out) && (mask_mode == kAugNoMask || aligned16(out_mask)))
    hipLaunchKernelGGL(augment_scale_kernel<4>, dim3((unsigned)((hw / 4 + 255) / 256), (unsigned)N), dim3(256), 0, st, tab, mean,
                       stdv, out, out_mask, g);
  else
    hipLaunchKernelGGL(augment_scale_kernel<1>, dim3((unsigned)((hw + 255) / 256), (unsigned)N), dim3(256), 0, st, tab, mean, stdv,
                       out, out_mask, g);
  return check_launch("augment_scale_batch");
}
