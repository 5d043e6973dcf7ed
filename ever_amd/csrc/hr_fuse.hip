// The multi-resolution exchange that ends an HRNet module (reference _hrnet.py:377-397) as ONE pass each way on NHWC fp32
// (gfx950):  y_i = ReLU(sum_j T_ij(x_j)),  T_ii = identity,  T_ij (j > i) = nearest x 2^(j-i) of BN(conv1x1(x_j)),
// T_ij (j < i) = BN(conv3x3s2 chain(x_j)).  The forward reads every term at its own resolution (a coarse pixel is re-read by the
// 4^shift fine pixels that share it: out of L2), applies the BatchNorm as scale / shift on the fly and writes y with its ReLU
// bits; the backward reads dy and the bits once and writes the masked gradient and its 2^s x 2^s block sums.  The composed
// form (BatchNorm apply, upsample and add per term, ReLU) moves about six times the bytes on a W48 stage-4 module.
// 16-byte accesses along the channel axis (C % 4 == 0) throughout.
#include "stream_common.hpp"

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
  const uint32_t H = fH.div, W = fW.div, c4 = fc4.div;
  uint32_t m = 0;
  for (uint32_t chunk = blockIdx.x * 4 + (threadIdx.x >> 6); chunk < nchunk; chunk += gridDim.x * 4) {
    const uint32_t j = chunk * 64 + lane;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (j < n4) {
      const NhwcElem e = nhwc_elem(j, fc4, fW, fH);
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        const int s = a.shift[k];
        f32x4 t = ld4(a.t[k], s == 0 ? (size_t)j : coarse_elem(e, H, W, c4, s));
        if (a.ss[k]) {
          const f32x4 sc = ld4(a.ss[k], e.cb), sh = ld4(a.ss[k] + C, e.cb);
          t.x = fmaf(t.x, sc.x, sh.x); t.y = fmaf(t.y, sc.y, sh.y); t.z = fmaf(t.z, sc.z, sh.z); t.w = fmaf(t.w, sc.w, sh.w);
        }
        v = k == 0 ? t : v + t;      // ((t0 + t1) + t2) + t3: the reference's order, j ascending
      }
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      st4(y, j, v);
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
    st4(dmasked, j, relu_bits_mask(ld4(dy, j), bits, j));
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
    const Quad e = quad_elems((size_t)n * H + y0, x0, W, c4, cb);
    const f32x4 g00 = relu_bits_mask(ld4(dy, e.e00), bits, e.e00), g01 = relu_bits_mask(ld4(dy, e.e01), bits, e.e01);
    const f32x4 g10 = relu_bits_mask(ld4(dy, e.e10), bits, e.e10), g11 = relu_bits_mask(ld4(dy, e.e11), bits, e.e11);
    if (dmasked) {
      st4(dmasked, e.e00, g00); st4(dmasked, e.e01, g01);
      st4(dmasked, e.e10, g10); st4(dmasked, e.e11, g11);
    }
    sum = quad_sum(g00, g01, g10, g11);
    if (dp1) st4(dp1, (((size_t)n * (H >> 1) + (y0 >> 1)) * (W >> 1) + (x0 >> 1)) * c4 + cb, sum);
  }
  if (S >= 2) {
    s1[tid] = sum;
    __syncthreads();
    const bool lead2 = on && !(qy & 1) && !(qx & 1);
    if (lead2) {      // neighbours: quad qi + 1 is CW threads on, the quad row below QE * CW
      sum = quad_sum(s1[tid], s1[tid + CW], s1[tid + QE * CW], s1[tid + (QE + 1) * CW]);
      if (dp2) {
        const int y2 = by * (B / 4) + (qy >> 1), x2 = bx * (B / 4) + (qx >> 1);
        st4(dp2, (((size_t)n * (H >> 2) + y2) * (W >> 2) + x2) * c4 + cb, sum);
      }
    }
    if (S >= 3) {
      s2[tid] = sum;
      __syncthreads();
      if (lead2 && qi == 0 && dp3) {
        sum = quad_sum(s2[tid], s2[tid + 2 * CW], s2[tid + 2 * QE * CW], s2[tid + (2 * QE + 2) * CW]);
        st4(dp3, (((size_t)n * (H >> 3) + by) * (W >> 3) + bx) * c4 + cb, sum);
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
  const int rc = check_terms("hr_fuse_fwd", terms, shifts, nterms, kHrMaxShift, H, W);
  if (rc != EVK_OK) return rc;
  HrFuseTerms a = {};
  for (int k = 0; k < nterms; ++k) { a.t[k] = terms[k]; a.ss[k] = scale_shifts[k]; a.shift[k] = shifts[k]; }
  const int64_t n4 = (int64_t)N * H * W * (C / 4);
  EVK_REQUIRE(n4 < 0x7fffffffLL - 64, EVK_E_UNSUPPORTED, "hr_fuse_fwd: %lld 16-byte elements (fewer than 2^31 are implemented)",
              (long long)n4);
  const dim3 grid(grid_for((size_t)n4)), block(256);
  const FastDiv fc4 = make_fastdiv((uint32_t)(C / 4)), fW = make_fastdiv((uint32_t)W), fH = make_fastdiv((uint32_t)H);
  return pick<1, 2, 3, 4>(nterms, [&](auto NT) {
    hipLaunchKernelGGL(hr_fuse_fwd_kernel<NT()>, grid, block, 0, (hipStream_t)stream, a, y, relu_bits, y_absmax, (uint32_t)n4, fc4,
                       fW, fH, C);
    return check_launch("hr_fuse_fwd");
  });
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
  if (S == 0) return launch_elems("hr_fuse_bwd", hr_fuse_bwd_mask_kernel, (size_t)n4, stream, dy, relu_bits, dmasked, (size_t)n4);
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
  return pick<1, 2, 3>(S, [&](auto SS) {
    hipLaunchKernelGGL(hr_fuse_bwd_pool_kernel<SS()>, grid, block, 0, (hipStream_t)stream, dy, relu_bits, dmasked, dpooled1,
                       dpooled2, dpooled3, (uint32_t)nblocks, fBW, fBH, H, W, C, CW, BPW);
    return check_launch("hr_fuse_bwd");
  });
}
