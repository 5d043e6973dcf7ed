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
