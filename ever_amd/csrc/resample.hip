// Bilinear resampling, align_corners=True, and its adjoint on NHWC fp32 (gfx950): element-per-thread kernels, the tile
// forward and the wave-per-pixel backward of the wide-channel maps, the host-side plan that picks among them, dense and
// channel-slice entry points.  Reference call sites are cited per entry point in include/ever_hip.h.
// 16-byte accesses along the channel axis (C % 4 == 0) with a scalar fallback where the path has C == 1 (classifier logits).
#include "stream_common.hpp"

namespace evk {

// ------------------------------------------------------------------------------------------------
// Bilinear, align_corners=True (nn.UpsamplingBilinear2d).  Cy is the pixel stride of the OUTPUT-sized map (y in the forward,
// dy in the backward): C for a dense map, Ctot when it is a channel slice of a [N,Ho,Wo,Ctot] concat buffer
// (evk_upsample_bilinear_slice_*: the pointer is then advanced to the slice's first channel).  Index math follows aten's
// upsample_bilinear2d: scale = (in-1)/(out-1) in float, src = scale*dst, i0 = (int)src,
// i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1.
__device__ __forceinline__ void bl_coord(int o, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  const float s = scale * (float)o;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

template <int VEC>
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int N,
                                                           int Hi, int Wi, int Ho, int Wo, int C, int Cy, float sy, float sx) {
  const int cv = C / VEC;
  const size_t total = (size_t)N * Ho * Wo * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const NhwcElem e = nhwc_elem(i, Ho, Wo, cv);     // of y
    const int n = e.n, oy = e.y, ox = e.x, cb = e.cb;
    float* o = y + (i / cv) * Cy + cb * VEC;
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    bl_coord(oy, sy, Hi, y0, y1, hy0, hy1);
    bl_coord(ox, sx, Wi, x0, x1, wx0, wx1);
    const float* b = x + (size_t)n * Hi * Wi * C + cb * VEC;
    const size_t o00 = ((size_t)y0 * Wi + x0) * C, o01 = ((size_t)y0 * Wi + x1) * C;
    const size_t o10 = ((size_t)y1 * Wi + x0) * C, o11 = ((size_t)y1 * Wi + x1) * C;
    if (VEC == 4) {
      const f32x4 v00 = *reinterpret_cast<const f32x4*>(b + o00), v01 = *reinterpret_cast<const f32x4*>(b + o01);
      const f32x4 v10 = *reinterpret_cast<const f32x4*>(b + o10), v11 = *reinterpret_cast<const f32x4*>(b + o11);
      *reinterpret_cast<f32x4*>(o) = hy0 * (wx0 * v00 + wx1 * v01) + hy1 * (wx0 * v10 + wx1 * v11);
    } else {
      *o = hy0 * (wx0 * b[o00] + wx1 * b[o01]) + hy1 * (wx0 * b[o10] + wx1 * b[o11]);
    }
  }
}

// The adjoint in gather form: every input pixel sums the (few) output pixels whose 2x2 footprint contains it, with exactly
// the forward's weights.  Candidate range [lo, hi] of input coordinate i on one axis (is = 1 / scale, o_max = out - 1):
// src in (i-1, i+1)  <=>  o in ((i-1)/scale, (i+1)/scale), widened by one for float rounding.
__device__ __forceinline__ void bl_candidates(int i, float is, int o_max, int& lo, int& hi) {
  lo = max((int)floorf((float)(i - 1) * is) - 1, 0);
  hi = min((int)ceilf((float)(i + 1) * is) + 1, o_max);
}
// weight with which output coordinate o (one axis) reads input coordinate i; 0 when it does not, or o is out of range
__device__ __forceinline__ float bl_adjoint_weight(int o, int o_hi, float scale, int in, int i) {
  int i0, i1;
  float l0, l1;
  bl_coord(o, scale, in, i0, i1, l0, l1);
  float w = 0.f;
  if (i0 == i) w += l0;
  if (i1 == i) w += l1;
  return o <= o_hi ? w : 0.f;
}

template <int VEC>
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N,
                                                           int Hi, int Wi, int Ho, int Wo, int C, int Cy, float sy, float sx,
                                                           float isy, float isx) {
  const int cv = C / VEC;
  const size_t total = (size_t)N * Hi * Wi * cv;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const NhwcElem e = nhwc_elem(i, Hi, Wi, cv);     // of dx
    const int n = e.n, iy = e.y, ix = e.x, cb = e.cb;
    int oy_lo, oy_hi, ox_lo, ox_hi;
    bl_candidates(iy, isy, Ho - 1, oy_lo, oy_hi);
    bl_candidates(ix, isx, Wo - 1, ox_lo, ox_hi);
    f32x4 acc4 = {0.f, 0.f, 0.f, 0.f};
    float acc1 = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      const float wy = bl_adjoint_weight(oy, oy_hi, sy, Hi, iy);
      if (wy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        const float wx = bl_adjoint_weight(ox, ox_hi, sx, Wi, ix);
        if (wx == 0.f) continue;
        const size_t o = (((size_t)n * Ho + oy) * Wo + ox) * Cy + cb * VEC;
        if (VEC == 4) acc4 += (wy * wx) * *reinterpret_cast<const f32x4*>(dy + o);
        else acc1 += (wy * wx) * dy[o];
      }
    }
    if (VEC == 4) *reinterpret_cast<f32x4*>(dx + i * 4) = acc4;
    else dx[i] = acc1;
  }
}

// Wide-channel forms (C >= 128): ONE WAVE PER PIXEL, lanes across the 16-byte channel chunks, so that the pixel's
// index arithmetic is wave-uniform.  The element-per-thread kernels above spend ~100 (forward) to ~1000 (backward)
// VALU instructions per 16 bytes on it and are VALU-bound on the 256-channel decoder maps (2.9 TB/s).  Uniform
// arithmetic lands on the scalar unit, ONE per CU: three integer divisions per pixel there were just as slow
// (124 us for 335 MB), hence the multiply-shift divisions and, in the backward, the candidate weights computed
// across lanes (one VALU pass for all 12 candidates of an axis) and fetched by v_readlane.
// Forward: a workgroup owns kTileR x kTileC output pixels, stages the input patch they read in LDS (one global load
// per input pixel and workgroup) and interpolates out of LDS.  Four global loads per output pixel — even wave-uniform
// and L2-resident — made the kernel L2->L1 bound: 90 us for the 64^2 -> 128^2 x 256 maps against 38 us for its
// 268 MB of stores alone (tools/probes/upsample_probe.hip).
constexpr int kTileR = 4, kTileC = 16;
// LPP lanes per pixel: 64 (C > 128), or 32 — the decoder's 128-channel maps fill only half a wave per pixel, so a wave
// takes two pixels side by side there (the per-pixel arithmetic is then per half-wave, on the vector unit)
template <int LPP>
__global__ __launch_bounds__(256) void bilinear_fwd_tile_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                int Hi, int Wi, int Ho, int Wo, int C, int Cy,
                                                                float sy, float sx, int patch_cols) {
  extern __shared__ __attribute__((aligned(16))) float patch[];  // [rows][patch_cols][C]
  constexpr int PPW = 64 / LPP;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int sub = lane / LPP, cl = (lane % LPP) * 4;
  const int n = blockIdx.z, oy0 = blockIdx.y * kTileR, ox0 = blockIdx.x * kTileC;
  const int oy_last = min(oy0 + kTileR, Ho) - 1, ox_last = min(ox0 + kTileC, Wo) - 1;
  int ylo, yhi, xlo, xhi, t0;
  float f0, f1;
  bl_coord(oy0, sy, Hi, ylo, t0, f0, f1);
  bl_coord(oy_last, sy, Hi, t0, yhi, f0, f1);
  bl_coord(ox0, sx, Wi, xlo, t0, f0, f1);
  bl_coord(ox_last, sx, Wi, t0, xhi, f0, f1);
  const int pr = yhi - ylo + 1, pc = xhi - xlo + 1;  // pc <= patch_cols by the host's bound
  const float* b = x + (size_t)n * Hi * Wi * C;
  for (int q = wave * PPW + sub; q < pr * pc; q += 4 * PPW) {
    const int r = q / pc, c = q - r * pc;
    const float* src = b + ((size_t)(ylo + r) * Wi + (xlo + c)) * C;
    float* dst = patch + (size_t)(r * patch_cols + c) * C;
    for (int k = cl; k < C; k += LPP * 4) *reinterpret_cast<f32x4*>(dst + k) = *reinterpret_cast<const f32x4*>(src + k);
  }
  __syncthreads();
  // wave w: output row oy0 + w (kTileR == 4 waves), all kTileC columns
  const int oy = oy0 + wave;
  if (oy > oy_last) return;
  int y0, y1;
  float hy0, hy1;
  bl_coord(oy, sy, Hi, y0, y1, hy0, hy1);
  const float* r0 = patch + (size_t)(y0 - ylo) * patch_cols * C;
  const float* r1 = patch + (size_t)(y1 - ylo) * patch_cols * C;
  float* o = y + (((size_t)n * Ho + oy) * Wo + ox0) * Cy;
  for (int j = sub; j <= ox_last - ox0; j += PPW) {
    int x0, x1;
    float wx0, wx1;
    bl_coord(ox0 + j, sx, Wi, x0, x1, wx0, wx1);
    const int c0 = (x0 - xlo) * C, c1 = (x1 - xlo) * C;
    for (int k = cl; k < C; k += LPP * 4) {
      const f32x4 v00 = *reinterpret_cast<const f32x4*>(r0 + c0 + k), v01 = *reinterpret_cast<const f32x4*>(r0 + c1 + k);
      const f32x4 v10 = *reinterpret_cast<const f32x4*>(r1 + c0 + k), v11 = *reinterpret_cast<const f32x4*>(r1 + c1 + k);
      *reinterpret_cast<f32x4*>(o + (size_t)j * Cy + k) = hy0 * (wx0 * v00 + wx1 * v01) + hy1 * (wx0 * v10 + wx1 * v11);
    }
  }
}

__global__ __launch_bounds__(256) void bilinear_bwd_wave_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                int npix, FastDiv fdWi, FastDiv fdHi, int Ho, int Wo,
                                                                int C, int Cy, float sy, float sx, float isy, float isx) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int pix = xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;   // see bilinear_fwd_wave_kernel
  if (pix >= npix) return;
  const int Hi = (int)fdHi.div, Wi = (int)fdWi.div;
  const uint32_t t = fdiv((uint32_t)pix, fdWi), ix = (uint32_t)pix - t * fdWi.div;
  const uint32_t n = fdiv(t, fdHi), iy = t - n * fdHi.div;
  int oy_lo, oy_hi, ox_lo, ox_hi;
  bl_candidates((int)iy, isy, Ho - 1, oy_lo, oy_hi);
  bl_candidates((int)ix, isx, Wo - 1, ox_lo, ox_hi);
  // lane j (mod 16) holds the weight of candidate lo + j on each axis; the candidate range of this kernel's callers
  // (scale >= 2 up-sampling) is at most 12 wide, wider ranges take the element-per-thread kernel
  const int j = lane & 15;
  const float wyv = bl_adjoint_weight(oy_lo + j, oy_hi, sy, Hi, (int)iy);
  const float wxv = bl_adjoint_weight(ox_lo + j, ox_hi, sx, Wi, (int)ix);
  uint32_t my = (uint32_t)(__ballot(wyv != 0.f) & 0xffffull);
  const uint32_t mx = (uint32_t)(__ballot(wxv != 0.f) & 0xffffull);
  const float* b = dy + (size_t)n * Ho * Wo * Cy;
  float* o = dx + (size_t)pix * C;
  f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  // same candidate order (oy ascending, then ox ascending) and weight arithmetic as bilinear_bwd_kernel
  while (my) {
    const int jy = __builtin_ctz(my);
    my &= my - 1;
    const float wy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wyv), jy));
    const float* row = b + (size_t)(oy_lo + jy) * Wo * Cy;
    uint32_t m = mx;
    while (m) {
      const int jx = __builtin_ctz(m);
      m &= m - 1;
      const float wx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wxv), jx));
      const float w = wy * wx;
      const float* src = row + (size_t)(ox_lo + jx) * Cy + lane * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (lane * 4 + 256 * k < C) acc[k] += w * *reinterpret_cast<const f32x4*>(src + 256 * k);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane * 4 + 256 * k < C) *reinterpret_cast<f32x4*>(o + lane * 4 + 256 * k) = acc[k];
}

}  // namespace evk

using namespace evk;

static inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// Which kernel a resampling call takes, and the numbers that kernel is launched with.  Pure host arithmetic, shared by the two
// launchers and evk_upsample_bilinear_plan.  `vec`: 16-byte accesses are legal (C, and for a slice c0 and Ctot, multiples of 4).
enum BilinearKernel { kBlScalar = 0, kBlVec = 1, kBlTile32 = 2, kBlTile64 = 3, kBlWave = 4 };
struct BilinearPlan {
  int kernel;
  int prow, pcol;        // forward: bound of the input patch one kTileR x kTileC output tile reads (the tile kernels' LDS)
  size_t patch_bytes;
  float sy, sx;          // (in - 1) / (out - 1), 0 for a one-pixel output
  float isy, isx;        // backward: inverse scales of the candidate range (in == 1 => every output maps to input 0)
};
static BilinearPlan bilinear_plan(int N, int Hi, int Wi, int Ho, int Wo, int C, bool vec, bool backward) {
  BilinearPlan pl = {};
  pl.sy = ac_scale(Hi, Ho);
  pl.sx = ac_scale(Wi, Wo);
  pl.kernel = vec ? kBlVec : kBlScalar;
  if (!backward) {
    // patch of one kTileR x kTileC output tile: rows/cols <= floor((tile - 1) * scale) + 3 (first i0 .. last i1)
    pl.prow = (int)((kTileR - 1) * pl.sy) + 3;
    pl.pcol = (int)((kTileC - 1) * pl.sx) + 3;
    pl.patch_bytes = (size_t)pl.prow * pl.pcol * C * sizeof(float);
    if (vec && C >= 128 && pl.patch_bytes <= 64 * 1024 && N <= 65535 && (Ho + kTileR - 1) / kTileR <= 65535)
      pl.kernel = C <= 128 ? kBlTile32 : kBlTile64;
  } else {
    pl.isy = pl.sy > 0.f ? 1.f / pl.sy : (float)Ho;
    pl.isx = pl.sx > 0.f ? 1.f / pl.sx : (float)Wo;
    const long long npix_i = (long long)N * Hi * Wi;
    // candidate range per axis: ceil((i+1)/s)+1 - (floor((i-1)/s)-1) + 1 <= 2/s + 5; the wave kernel holds 16 per axis
    const bool narrow = 2.f * pl.isy + 5.f <= 16.f && 2.f * pl.isx + 5.f <= 16.f && Hi > 1 && Wi > 1;
    if (vec && C >= 128 && C <= 1024 && narrow && npix_i < 0x7fffffffLL) pl.kernel = kBlWave;
  }
  return pl;
}

// y / dy: the output-sized map's first channel of this call, Cy its pixel stride (C when dense)
static int bilinear_fwd_launch(const float* x, float* y, int N, int Hi, int Wi, int Ho, int Wo, int C, int Cy, bool vec,
                               void* stream) {
  const BilinearPlan pl = bilinear_plan(N, Hi, Wi, Ho, Wo, C, vec, false);
  if (pl.kernel == kBlVec)
    return launch_elems("bilinear_fwd", bilinear_fwd_kernel<4>, (size_t)N * Ho * Wo * (C / 4), stream, x, y, N, Hi, Wi, Ho, Wo, C,
                        Cy, pl.sy, pl.sx);
  if (pl.kernel == kBlScalar)
    return launch_elems("bilinear_fwd", bilinear_fwd_kernel<1>, (size_t)N * Ho * Wo * C, stream, x, y, N, Hi, Wi, Ho, Wo, C, Cy,
                        pl.sy, pl.sx);
  static PerDeviceOnce attr_once;
  if (attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&bilinear_fwd_tile_kernel<64>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&bilinear_fwd_tile_kernel<32>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  }
  const dim3 grid((Wo + kTileC - 1) / kTileC, (Ho + kTileR - 1) / kTileR, N);
  pick<32, 64>(pl.kernel == kBlTile32 ? 32 : 64, [&](auto LPP) {
    hipLaunchKernelGGL(bilinear_fwd_tile_kernel<LPP()>, grid, dim3(256), pl.patch_bytes, (hipStream_t)stream, x, y, Hi, Wi, Ho,
                       Wo, C, Cy, pl.sy, pl.sx, pl.pcol);
    return 0;
  });
  return check_launch("bilinear_fwd");
}
static int bilinear_bwd_launch(const float* dy, float* dx, int N, int Hi, int Wi, int Ho, int Wo, int C, int Cy, bool vec,
                               void* stream) {
  const BilinearPlan pl = bilinear_plan(N, Hi, Wi, Ho, Wo, C, vec, true);
  if (pl.kernel == kBlVec)
    return launch_elems("bilinear_bwd", bilinear_bwd_kernel<4>, (size_t)N * Hi * Wi * (C / 4), stream, dy, dx, N, Hi, Wi, Ho, Wo, C,
                        Cy, pl.sy, pl.sx, pl.isy, pl.isx);
  if (pl.kernel == kBlScalar)
    return launch_elems("bilinear_bwd", bilinear_bwd_kernel<1>, (size_t)N * Hi * Wi * C, stream, dy, dx, N, Hi, Wi, Ho, Wo, C, Cy,
                        pl.sy, pl.sx, pl.isy, pl.isx);
  const long long npix_i = (long long)N * Hi * Wi;
  hipLaunchKernelGGL(bilinear_bwd_wave_kernel, dim3((unsigned)((npix_i + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dy, dx,
                     (int)npix_i, make_fastdiv((uint32_t)Wi), make_fastdiv((uint32_t)Hi), Ho, Wo, C, Cy, pl.sy, pl.sx, pl.isy,
                     pl.isx);
  return check_launch("bilinear_bwd");
}

// Host only (no launch): the plan of a resampling call.  out[8] = {kernel (0 scalar element, 1 16-byte element, 2 tile with 32
// lanes per pixel, 3 tile with 64, 4 wave per pixel), patch rows, patch columns, patch bytes (forward; 0 in the backward;
// saturated at INT32_MAX), bit images of sy, sx, isy, isx as the kernels receive them (isy, isx: 0 in the forward)}
extern "C" int evk_upsample_bilinear_plan(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t C, int32_t vec,
                                          int32_t backward, int32_t* out) {
  EVK_REQUIRE(out && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && (!vec || C % 4 == 0), EVK_E_INVALID,
              "bilinear_plan: bad argument");
  const BilinearPlan pl = bilinear_plan(N, Hi, Wi, Ho, Wo, C, vec != 0, backward != 0);
  out[0] = pl.kernel;
  out[1] = pl.prow;
  out[2] = pl.pcol;
  out[3] = pl.patch_bytes > 0x7fffffffull ? 0x7fffffff : (int32_t)pl.patch_bytes;
  out[4] = __builtin_bit_cast(int32_t, pl.sy);
  out[5] = __builtin_bit_cast(int32_t, pl.sx);
  out[6] = __builtin_bit_cast(int32_t, pl.isy);
  out[7] = __builtin_bit_cast(int32_t, pl.isx);
  return EVK_OK;
}

// The four entry points: src -> dst is x -> y, or dy -> dx; the OUTPUT-sized map (y, or dy) is channels [c0, c0 + C) of pixels
// Ctot wide, and a dense call is the slice c0 = 0, Ctot = C.  16-byte accesses need the slice and the stride aligned.
// `what` names the entry point that was called, `hint` ends its error text.
static int bilinear_slice(const char* what, const char* hint, bool backward, const float* src, float* dst, int N, int Hi, int Wi,
                          int Ho, int Wo, int C, int c0, int Ctot, void* stream) {
  EVK_REQUIRE(src && dst && N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && c0 >= 0 && (int64_t)c0 + C <= Ctot,
              EVK_E_INVALID, "%s: bad argument%s", what, hint);
  const bool vec = C % 4 == 0 && c0 % 4 == 0 && Ctot % 4 == 0;
  return backward ? bilinear_bwd_launch(src + c0, dst, N, Hi, Wi, Ho, Wo, C, Ctot, vec, stream)
                  : bilinear_fwd_launch(src, dst + c0, N, Hi, Wi, Ho, Wo, C, Ctot, vec, stream);
}
static const char kSliceHint[] = " (need 0 <= c0, c0 + C <= Ctot)";

extern "C" int evk_upsample_bilinear_fwd(const float* x, float* y, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                         int32_t Wo, int32_t C, void* stream) {
  return bilinear_slice("bilinear_fwd", "", false, x, y, N, Hi, Wi, Ho, Wo, C, 0, C, stream);
}
extern "C" int evk_upsample_bilinear_bwd(const float* dy, float* dx, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                         int32_t Wo, int32_t C, void* stream) {
  return bilinear_slice("bilinear_bwd", "", true, dy, dx, N, Hi, Wi, Ho, Wo, C, 0, C, stream);
}
extern "C" int evk_upsample_bilinear_slice_fwd(const float* x, float* y, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                               int32_t Wo, int32_t C, int32_t c0, int32_t Ctot, void* stream) {
  return bilinear_slice("bilinear_slice_fwd", kSliceHint, false, x, y, N, Hi, Wi, Ho, Wo, C, c0, Ctot, stream);
}
extern "C" int evk_upsample_bilinear_slice_bwd(const float* dy, float* dx, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                               int32_t Wo, int32_t C, int32_t c0, int32_t Ctot, void* stream) {
  return bilinear_slice("bilinear_slice_bwd", kSliceHint, true, dy, dx, N, Hi, Wi, Ho, Wo, C, c0, Ctot, stream);
}
