// The multi-resolution exchange that ends an HRNet module (reference _hrnet.py:377-397) as ONE pass each way on NHWC fp32
// (gfx950):  y_i = ReLU(sum_j T_ij(x_j)),  T_ii = identity,  T_ij (j > i) = nearest x 2^(j-i) of BN(conv1x1(x_j)),
// T_ij (j < i) = BN(conv3x3s2 chain(x_j)).  The forward reads every term at its own resolution (a coarse pixel is re-read by the
// 4^shift fine pixels that share it: out of L2), applies the BatchNorm as scale / shift on the fly and writes y with its ReLU
// bits; the backward reads dy and the bits once and writes the masked gradient and its 2^s x 2^s block sums.  The composed
// form (BatchNorm apply, upsample and add per term, ReLU) moves about six times the bytes on a W48 stage-4 module.
// 16-byte accesses along the channel axis (C % 4 == 0) throughout.
#include "common.hpp"

namespace evk {

constexpr int kHrMaxTerms = 4, kHrMaxShift = 3;

struct HrFuseTerms {
  const float* t[kHrMaxTerms];    // [N, H >> shift, W >> shift, C]
  const float* ss[kHrMaxTerms];   // scale_shift [2][C] or null (the term enters as it is)
  int32_t shift[kHrMaxTerms];
};

// One thread per 16-byte element j of y, a wave per 64 consecutive elements (= one chunk of the ReLU bits, common.hpp).
// NT is a template parameter so that the term tables are indexed by constants (a runtime index would put them in scratch).
template <int NT>
__global__ __launch_bounds__(256) void hr_fuse_fwd_kernel(const HrFuseTerms a, float* __restrict__ y,
                                                          uint32_t* __restrict__ bits, uint32_t* __restrict__ amax,
                                                          uint32_t n4, FastDiv fc4, FastDiv fW, FastDiv fH, int C) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nchunk = (n4 + 63) >> 6;
  const uint32_t H = fH.div, W = fW.div;
  uint32_t m = 0;
  for (uint32_t chunk = blockIdx.x * 4 + (threadIdx.x >> 6); chunk < nchunk; chunk += gridDim.x * 4) {
    const uint32_t j = chunk * 64 + lane;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (j < n4) {
      const uint32_t pix = fdiv(j, fc4), cb = j - pix * fc4.div;
      const uint32_t r = fdiv(pix, fW), px = pix - r * W;
      const uint32_t n = fdiv(r, fH), py = r - n * H;
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        const int s = a.shift[k];
        const size_t off = s == 0 ? (size_t)j * 4
                                  : (((size_t)n * (H >> s) + (py >> s)) * (W >> s) + (px >> s)) * C + cb * 4;
        f32x4 t = *reinterpret_cast<const f32x4*>(a.t[k] + off);
        if (a.ss[k]) {
          const f32x4 sc = *reinterpret_cast<const f32x4*>(a.ss[k] + cb * 4);
          const f32x4 sh = *reinterpret_cast<const f32x4*>(a.ss[k] + C + cb * 4);
          t.x = fmaf(t.x, sc.x, sh.x); t.y = fmaf(t.y, sc.y, sh.y); t.z = fmaf(t.z, sc.z, sh.z); t.w = fmaf(t.w, sc.w, sh.w);
        }
        v = k == 0 ? t : v + t;      // ((t0 + t1) + t2) + t3: the reference's order, j ascending
      }
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      *reinterpret_cast<f32x4*>(y + (size_t)j * 4) = v;
      m = abs4_bits(m, v);
    }
    relu_bits_store(bits, chunk, v.x > 0.f, v.y > 0.f, v.z > 0.f, v.w > 0.f);   // (elements past the end: clear bits)
  }
  if (amax) commit_absmax(amax, m);
}

// Backward without pools: dmasked = dy where the bit is set
__global__ __launch_bounds__(256) void hr_fuse_bwd_mask_kernel(const float* __restrict__ dy, const uint32_t* __restrict__ bits,
                                                               float* __restrict__ dmasked, size_t n4) {
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n4; j += (size_t)gridDim.x * 256)
    *reinterpret_cast<f32x4*>(dmasked + j * 4) = relu_bits_mask(*reinterpret_cast<const f32x4*>(dy + j * 4), bits, j);
}

// Backward with pools up to shift S.  A thread owns one 2 x 2 quad of fine pixels at one 16-byte channel chunk: it reads its
// four dy and their bits, writes the four masked values and the quad's sum (the shift-1 pool).  A workgroup owns whole
// 2^S x 2^S blocks (QB = 4^(S-1) quads each) at CW channel chunks, threads ordered chunk-fastest, then quads of a block row by
// row: the quad sums go through LDS and the quad at a block's even position sums its 2 x 2 neighbours (shift 2), then one
// thread per block the four shift-2 sums (shift 3).  Every output element has one owner and a fixed summation order:
// no atomics, the same bits every run.
template <int S>
__global__ __launch_bounds__(256) void hr_fuse_bwd_pool_kernel(const float* __restrict__ dy, const uint32_t* __restrict__ bits,
                                                               float* __restrict__ dmasked, float* __restrict__ dp1,
                                                               float* __restrict__ dp2, float* __restrict__ dp3,
                                                               uint32_t nblocks, FastDiv fBW, FastDiv fBH, int H, int W, int C,
                                                               int CW, int BPW) {
  constexpr int B = 1 << S, QE = B / 2, QB = QE * QE;     // block edge in pixels, in quads; quads per block
  __shared__ f32x4 s1[S >= 2 ? 256 : 1];
  __shared__ f32x4 s2[S >= 3 ? 256 : 1];
  const int tid = threadIdx.x;
  const int cw = tid % CW, q = tid / CW;
  const int blk = q / QB, qi = q % QB, qy = qi / QE, qx = qi % QE;
  const uint32_t b = blockIdx.x * (uint32_t)BPW + blk;
  const bool on = blk < BPW && b < nblocks;
  const int c4 = C >> 2, cb = blockIdx.y * CW + cw;
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  uint32_t n = 0, by = 0, bx = 0;
  if (on) {
    const uint32_t r = fdiv(b, fBW);
    bx = b - r * fBW.div;
    n = fdiv(r, fBH);
    by = r - n * fBH.div;
    const int y0 = by * B + 2 * qy, x0 = bx * B + 2 * qx;
    const size_t p00 = ((size_t)n * H + y0) * W + x0, p10 = p00 + W;
    const size_t e00 = p00 * c4 + cb, e01 = e00 + c4, e10 = p10 * c4 + cb, e11 = e10 + c4;
    const f32x4 g00 = relu_bits_mask(*reinterpret_cast<const f32x4*>(dy + e00 * 4), bits, e00);
    const f32x4 g01 = relu_bits_mask(*reinterpret_cast<const f32x4*>(dy + e01 * 4), bits, e01);
    const f32x4 g10 = relu_bits_mask(*reinterpret_cast<const f32x4*>(dy + e10 * 4), bits, e10);
    const f32x4 g11 = relu_bits_mask(*reinterpret_cast<const f32x4*>(dy + e11 * 4), bits, e11);
    if (dmasked) {
      *reinterpret_cast<f32x4*>(dmasked + e00 * 4) = g00;
      *reinterpret_cast<f32x4*>(dmasked + e01 * 4) = g01;
      *reinterpret_cast<f32x4*>(dmasked + e10 * 4) = g10;
      *reinterpret_cast<f32x4*>(dmasked + e11 * 4) = g11;
    }
    sum = (g00 + g01) + (g10 + g11);
    if (dp1)
      *reinterpret_cast<f32x4*>(dp1 + ((((size_t)n * (H >> 1) + (y0 >> 1)) * (W >> 1) + (x0 >> 1)) * c4 + cb) * 4) = sum;
  }
  if (S >= 2) {
    s1[tid] = sum;
    __syncthreads();
    const bool lead2 = on && !(qy & 1) && !(qx & 1);
    if (lead2) {      // neighbours: quad qi + 1 is CW threads on, the quad row below QE * CW
      sum = (s1[tid] + s1[tid + CW]) + (s1[tid + QE * CW] + s1[tid + (QE + 1) * CW]);
      if (dp2) {
        const int y2 = by * (B / 4) + (qy >> 1), x2 = bx * (B / 4) + (qx >> 1);
        *reinterpret_cast<f32x4*>(dp2 + ((((size_t)n * (H >> 2) + y2) * (W >> 2) + x2) * c4 + cb) * 4) = sum;
      }
    }
    if (S >= 3) {
      s2[tid] = sum;
      __syncthreads();
      if (lead2 && qi == 0 && dp3) {
        sum = (s2[tid] + s2[tid + 2 * CW]) + (s2[tid + 2 * QE * CW] + s2[tid + (2 * QE + 2) * CW]);
        *reinterpret_cast<f32x4*>(dp3 + ((((size_t)n * (H >> 3) + by) * (W >> 3) + bx) * c4 + cb) * 4) = sum;
      }
    }
  }
}

}  // namespace evk

using namespace evk;

extern "C" int evk_hr_fuse_fwd(const float* const* terms, const int32_t* shifts, const float* const* scale_shifts,
                               int32_t nterms, float* y, uint32_t* relu_bits, uint32_t* y_absmax, int32_t N, int32_t H,
                               int32_t W, int32_t C, void* stream) {
  EVK_REQUIRE(terms && shifts && scale_shifts && y && relu_bits && N > 0 && H > 0 && W > 0 && C > 0, EVK_E_INVALID,
              "hr_fuse_fwd: bad argument (null pointer or non-positive size)");
  EVK_REQUIRE(nterms >= 1 && nterms <= kHrMaxTerms, EVK_E_UNSUPPORTED, "hr_fuse_fwd: %d terms (1 to %d are implemented)",
              nterms, kHrMaxTerms);
  EVK_REQUIRE(C % 4 == 0, EVK_E_UNSUPPORTED, "hr_fuse_fwd: C = %d must be a multiple of 4", C);
  HrFuseTerms a = {};
  int smax = 0;
  for (int k = 0; k < nterms; ++k) {
    EVK_REQUIRE(terms[k], EVK_E_INVALID, "hr_fuse_fwd: term %d is a null pointer", k);
    EVK_REQUIRE(shifts[k] >= 0 && shifts[k] <= kHrMaxShift, EVK_E_UNSUPPORTED,
                "hr_fuse_fwd: term %d has shift %d (0 to %d are implemented)", k, shifts[k], kHrMaxShift);
    a.t[k] = terms[k]; a.ss[k] = scale_shifts[k]; a.shift[k] = shifts[k];
    smax = shifts[k] > smax ? shifts[k] : smax;
  }
  EVK_REQUIRE(H % (1 << smax) == 0 && W % (1 << smax) == 0, EVK_E_UNSUPPORTED,
              "hr_fuse_fwd: H = %d, W = %d must be multiples of %d (the largest shift is %d)", H, W, 1 << smax, smax);
  const int64_t n4 = (int64_t)N * H * W * (C / 4);
  EVK_REQUIRE(n4 < 0x7fffffffLL - 64, EVK_E_UNSUPPORTED, "hr_fuse_fwd: %lld 16-byte elements (fewer than 2^31 are implemented)",
              (long long)n4);
  const dim3 grid(grid_for((size_t)n4)), block(256);
  const FastDiv fc4 = make_fastdiv((uint32_t)(C / 4)), fW = make_fastdiv((uint32_t)W), fH = make_fastdiv((uint32_t)H);
  hipStream_t st = (hipStream_t)stream;
  switch (nterms) {
    case 1: hipLaunchKernelGGL(hr_fuse_fwd_kernel<1>, grid, block, 0, st, a, y, relu_bits, y_absmax, (uint32_t)n4, fc4, fW, fH, C); break;
    case 2: hipLaunchKernelGGL(hr_fuse_fwd_kernel<2>, grid, block, 0, st, a, y, relu_bits, y_absmax, (uint32_t)n4, fc4, fW, fH, C); break;
    case 3: hipLaunchKernelGGL(hr_fuse_fwd_kernel<3>, grid, block, 0, st, a, y, relu_bits, y_absmax, (uint32_t)n4, fc4, fW, fH, C); break;
    default: hipLaunchKernelGGL(hr_fuse_fwd_kernel<4>, grid, block, 0, st, a, y, relu_bits, y_absmax, (uint32_t)n4, fc4, fW, fH, C); break;
  }
  return check_launch("hr_fuse_fwd");
}

extern "C" int evk_hr_fuse_bwd(const float* dy, const uint32_t* relu_bits, float* dmasked, float* dpooled1, float* dpooled2,
                               float* dpooled3, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
  EVK_REQUIRE(dy && relu_bits && (dmasked || dpooled1 || dpooled2 || dpooled3) && N > 0 && H > 0 && W > 0 && C > 0,
              EVK_E_INVALID, "hr_fuse_bwd: bad argument (null pointer, no output or non-positive size)");
  EVK_REQUIRE(C % 4 == 0, EVK_E_UNSUPPORTED, "hr_fuse_bwd: C = %d must be a multiple of 4", C);
  const int S = dpooled3 ? 3 : dpooled2 ? 2 : dpooled1 ? 1 : 0;
  EVK_REQUIRE(H % (1 << S) == 0 && W % (1 << S) == 0, EVK_E_UNSUPPORTED,
              "hr_fuse_bwd: H = %d, W = %d must be multiples of %d (the largest shift is %d)", H, W, 1 << S, S);
  const int c4 = C / 4;
  const int64_t n4 = (int64_t)N * H * W * c4;
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {
    hipLaunchKernelGGL(hr_fuse_bwd_mask_kernel, dim3(grid_for((size_t)n4)), dim3(256), 0, st, dy, relu_bits, dmasked, (size_t)n4);
    return check_launch("hr_fuse_bwd");
  }
  const int B = 1 << S, QB = (B / 2) * (B / 2);
  const int64_t nblocks = (int64_t)N * (H / B) * (W / B);
  int CW = c4 < 16 ? c4 : 16;       // channel chunks per workgroup: the largest divisor of C / 4 up to 16
  while (c4 % CW) --CW;
  const int BPW = 256 / (CW * QB);  // whole blocks per workgroup (>= 1: CW, QB <= 16)
  const int64_t gx = (nblocks + BPW - 1) / BPW;
  EVK_REQUIRE(nblocks < 0x7fffffffLL && gx <= 0x7fffffffLL && c4 / CW <= 65535, EVK_E_UNSUPPORTED,
              "hr_fuse_bwd: map too large (%lld blocks, %d channel groups)", (long long)nblocks, c4 / CW);
  const dim3 grid((unsigned)gx, (unsigned)(c4 / CW)), block(256);
  const FastDiv fBW = make_fastdiv((uint32_t)(W / B)), fBH = make_fastdiv((uint32_t)(H / B));
  if (S == 1)
    hipLaunchKernelGGL(hr_fuse_bwd_pool_kernel<1>, grid, block, 0, st, dy, relu_bits, dmasked, dpooled1, dpooled2, dpooled3,
                       (uint32_t)nblocks, fBW, fBH, H, W, C, CW, BPW);
  else if (S == 2)
    hipLaunchKernelGGL(hr_fuse_bwd_pool_kernel<2>, grid, block, 0, st, dy, relu_bits, dmasked, dpooled1, dpooled2, dpooled3,
                       (uint32_t)nblocks, fBW, fBH, H, W, C, CW, BPW);
  else
    hipLaunchKernelGGL(hr_fuse_bwd_pool_kernel<3>, grid, block, 0, st, dy, relu_bits, dmasked, dpooled1, dpooled2, dpooled3,
                       (uint32_t)nblocks, fBW, fBH, H, W, C, CW, BPW);
  return check_launch("hr_fuse_bwd");
}
