// BatchNorm2d (+ residual add, + ReLU) forward / backward on NHWC fp32 for gfx950.
// Replaces aten::batch_norm / native_batch_norm_backward, aten::add_, aten::relu_ at reference
// ever/module/_resnets.py:95-112 (bn1..bn3, `out += identity`, relu), fs_relation.py:39-53,
// fpn.py:163-167.  HBM-bound: every kernel streams [rows][C] with 16-byte accesses, a workgroup's
// row range is one contiguous span.  Statistics are reduced in two stages (fp32 partials per
// workgroup, fp64 finalisation) so results do not depend on the launch grid.
#include "bn_common.hpp"

namespace evk {

// partial[blk][0][C] = sum (x - pivot), partial[blk][1][C] = sum (x - pivot)^2 with pivot[c] = x[0][c].
// Shifting by a sample of the same channel keeps var = E[d^2] - E[d]^2 free of the catastrophic
// cancellation the raw moments suffer when |mean| >> std (8-sample statistics at 2x2 maps).
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ x, float* __restrict__ partial,
                                                               int64_t rows, int C, int64_t rows_per_blk, int tpc,
                                                               int rl) {
  __shared__ f32x4 red[2][256];
  const int c4 = C >> 2;
  const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  const int64_t r1 = min(rows, r0 + rows_per_blk);
  for (int cb = tc; cb < c4; cb += tpc) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    const f32x4 pv = *reinterpret_cast<const f32x4*>(x + cb * 4);
    if (tr < rl) {
      // 4 independent 16-byte loads in flight per lane: the reduction is latency bound otherwise
      // (measured 2.7 TB/s with one load per lane per trip)
      int64_t r = r0 + tr;
      const int64_t st = rl;
      for (; r + 3 * st < r1; r += 4 * st) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + r * C + cb * 4) - pv;
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(x + (r + st) * C + cb * 4) - pv;
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(x + (r + 2 * st) * C + cb * 4) - pv;
        const f32x4 v3 = *reinterpret_cast<const f32x4*>(x + (r + 3 * st) * C + cb * 4) - pv;
        s += (v0 + v1) + (v2 + v3);
        q += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
      }
      for (; r < r1; r += st) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * C + cb * 4) - pv;
        s += v;
        q += v * v;
      }
    }
    fold_store_record(red, s, q, partial, blockIdx.x, C, cb, tc, tr, tpc, rl);
  }
}

// mean / biased var -> save_mean, save_invstd, scale/shift for the apply pass; running stats update
// follows torch: running = (1-m)*running + m*stat, with the UNBIASED variance (n/(n-1)).
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ partial, int nblk, int C,
                                                             double inv_rows, double unbias,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, float momentum,
                                                             float eps, float* __restrict__ save_mean,
                                                             float* __restrict__ save_invstd,
                                                             float* __restrict__ scale_shift,
                                                             uint32_t* __restrict__ amax) {
  zero_amax(amax);   // the apply pass accumulates max|y| into its slots
  int c;
  double s, q;
  if (!reduce_partials(partial, nblk, C, c, s, q)) return;
  const double dm = s * inv_rows;  // mean of (x - pivot)
  const double mean = (double)x[c] + dm;
  double var = q * inv_rows - dm * dm;
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float meanf = (float)mean;
  save_mean[c] = meanf;
  save_invstd[c] = invstd;
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * unbias);
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float sc = g * invstd;
  scale_shift[c] = sc;
  scale_shift[C + c] = b - meanf * sc;
}

__global__ void bn_eval_coef_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                    const float* __restrict__ rm, const float* __restrict__ rv, float eps, int C,
                                    float* __restrict__ scale_shift, float* __restrict__ save_mean,
                                    float* __restrict__ save_invstd, uint32_t* __restrict__ amax) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  zero_amax(amax);
  if (c >= C) return;
  const float invstd = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
  if (save_mean) save_mean[c] = rm[c];
  if (save_invstd) save_invstd[c] = invstd;
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float sc = g * invstd;
  scale_shift[c] = sc;
  scale_shift[C + c] = b - rm[c] * sc;
}

// Channel chunk of flat 16-byte element i: (i mod c4) without a per-lane 64-bit division — the workgroup's base
// goes through the scalar unit, the lane offset (< 256 + c4 <= 768) through an exact float reciprocal.
__device__ __forceinline__ int chunk_of(size_t blk_base, int c4) {
  const uint32_t v = (uint32_t)(blk_base % (size_t)c4) + threadIdx.x;
  const uint32_t q = (uint32_t)((float)v * (1.0f / (float)c4));
  int r = (int)(v - q * (uint32_t)c4);
  r = r < 0 ? r + c4 : r;
  return r >= c4 ? r - c4 : r;
}

// y = act(x*scale + shift [+ residual]).
// ONE 16-byte element per thread and a grid of n4/256 workgroups: on the 268 MB maps a 1-read + 1-write stream
// runs at 6.1 TB/s this way against 4.3 TB/s for 2048 grid-striding workgroups with four loads in flight each
// (tools/probes/copy_patterns.hip) — the resident workgroups then sweep one contiguous window of HBM in dispatch
// order instead of 2048 x 4 scattered pages.  scale/shift (2C floats) come from L1/L2, not LDS: staging them
// per workgroup would cost more than the 4 KB a workgroup streams.
// PK: y is written as packed words of y / s (x3_common.hpp: pack_hl), s from the bound the finalisation left in slot 0
// of `amax` — the tensor is the next convolution's operand and nothing else.
template <bool PK = false>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ residual,
                                                       const float* __restrict__ scale_shift, float* __restrict__ y,
                                                       size_t n4, int C, int relu, uint32_t* __restrict__ amax,
                                                       uint32_t* __restrict__ relu_bits = nullptr) {
  const size_t base = (size_t)bn_blk() * 256;
  const size_t i = base + threadIdx.x;
  const bool valid = i < n4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  float pk_inv = 1.f;
  if constexpr (PK) pk_inv = op_scale(amax[0]).inv;
  if (valid) {
    const int c4 = C >> 2;
    const int cb = chunk_of(base, c4);
    const f32x4 sc = reinterpret_cast<const f32x4*>(scale_shift)[cb];
    const f32x4 sh = reinterpret_cast<const f32x4*>(scale_shift + C)[cb];
    v = bn_ld(x, i) * sc + sh;
    if (residual) v += bn_ld(residual, i);
  }
  // the backward's mask, one bit per element (common.hpp: relu_bits_*): every lane of the wave takes part (v = 0 where
  // the element does not exist), i >> 6 is this wave's chunk
  if (relu_bits) relu_bits_store(relu_bits, i >> 6, v.x > 0.f, v.y > 0.f, v.z > 0.f, v.w > 0.f);
  if (valid) {
    if (relu) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    if constexpr (PK) {
      reinterpret_cast<u32x4*>(y)[i] = pack_hl4(v, pk_inv);
    } else {
      reinterpret_cast<f32x4*>(y)[i] = v;
    }
  }
  if constexpr (!PK)
    if (amax) block_absmax(v, valid, amax);   // all lanes of the workgroup arrive here together
}

// Backward stage 1: g = dy * (y > 0) ; partial[blk][0][C] = sum g, [1][C] = sum g * xhat.
// Optionally writes g to d_residual.
// PK (dx will be written packed, EVK_BN_PACK_DX): also pmax[blk][0][C] = max |g|, [1][C] = max |xhat| — what the
// finalisation needs to bound |dx| per channel BEFORE the apply pass writes it under that scale.
// (plain loads: the apply pass re-reads what this pass streams.  The non-temporal hint here, gated by map size, measured
// level from 128 MB up and -0.3 % below — removed)
__device__ __forceinline__ f32x4 bp_ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <bool PK>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ y,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             float* __restrict__ d_residual,
                                                             float* __restrict__ partial, int64_t rows, int C,
                                                             int64_t rows_per_blk, int tpc, int rl, int relu,
                                                             float* __restrict__ pmax,
                                                             const uint32_t* __restrict__ bits = nullptr) {
  // relu: 0 none, 1 mask from the saved output y, 2 mask recomputed from x (no residual: the
  // forward's pre-activation is x*sc+sh with the same sc/sh arithmetic as bn_stats_final_kernel), 3 mask from `bits`
  // (common.hpp: relu_bits_*: the forward's own bits, or the mask of a gradient that arrives unmasked — EVK_BN_LAZY_RES)
  __shared__ f32x4 red[2][256];
  const int c4 = C >> 2;
  const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
  const int64_t r0 = (int64_t)bn_blk() * rows_per_blk;
  const int64_t r1 = min(rows, r0 + rows_per_blk);
  for (int cb = tc; cb < c4; cb += tpc) {
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + cb * 4);
    const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + cb * 4);
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (relu == 2) {
      const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
      const f32x4 g4 = gamma ? *reinterpret_cast<const f32x4*>(gamma + cb * 4) : one;
      const f32x4 b4 = beta ? *reinterpret_cast<const f32x4*>(beta + cb * 4) : zero;
      sc = g4 * is;
      sh = b4 - mu * sc;
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    f32x4 gm = {0.f, 0.f, 0.f, 0.f}, xm = {0.f, 0.f, 0.f, 0.f};
    if (tr < rl) {
      auto one = [&](const f32x4 gin, const f32x4 xv, const f32x4 yin, size_t off) {
        f32x4 g = gin;
        if (relu == 3) {
          g = relu_bits_mask(g, bits, off >> 2);
        } else if (relu) {
          const f32x4 yy = (relu == 1) ? yin : xv * sc + sh;
          g = relu_mask(g, yy);
        }
        if (d_residual) *reinterpret_cast<f32x4*>(d_residual + off) = g;
        s += g;
        const f32x4 xh = (xv - mu) * is;
        q += g * xh;
        if constexpr (PK) {
          gm.x = fmaxf(gm.x, fabsf(g.x)); gm.y = fmaxf(gm.y, fabsf(g.y));
          gm.z = fmaxf(gm.z, fabsf(g.z)); gm.w = fmaxf(gm.w, fabsf(g.w));
          xm.x = fmaxf(xm.x, fabsf(xh.x)); xm.y = fmaxf(xm.y, fabsf(xh.y));
          xm.z = fmaxf(xm.z, fabsf(xh.z)); xm.w = fmaxf(xm.w, fabsf(xh.w));
        }
      };
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      int64_t r = r0 + tr;
      const int64_t st = rl;
      // four rows per trip: 8-12 independent 16-byte loads in flight per lane
      for (; r + 3 * st < r1; r += 4 * st) {
        const size_t o0 = (size_t)r * C + cb * 4, o1 = (size_t)(r + st) * C + cb * 4;
        const size_t o2 = (size_t)(r + 2 * st) * C + cb * 4, o3 = (size_t)(r + 3 * st) * C + cb * 4;
        const f32x4 g0 = bp_ld(dy + o0), g1 = bp_ld(dy + o1);
        const f32x4 g2 = bp_ld(dy + o2), g3 = bp_ld(dy + o3);
        const f32x4 x0 = bp_ld(x + o0), x1 = bp_ld(x + o1);
        const f32x4 x2 = bp_ld(x + o2), x3 = bp_ld(x + o3);
        f32x4 y0 = zero4, y1 = zero4, y2 = zero4, y3 = zero4;
        if (relu == 1) {
          y0 = bp_ld(y + o0);
          y1 = bp_ld(y + o1);
          y2 = bp_ld(y + o2);
          y3 = bp_ld(y + o3);
        }
        one(g0, x0, y0, o0);
        one(g1, x1, y1, o1);
        one(g2, x2, y2, o2);
        one(g3, x3, y3, o3);
      }
      for (; r < r1; r += st) {
        const size_t o0 = (size_t)r * C + cb * 4;
        const f32x4 g0 = bp_ld(dy + o0);
        const f32x4 x0 = bp_ld(x + o0);
        const f32x4 y0 = (relu == 1) ? bp_ld(y + o0) : zero4;
        one(g0, x0, y0, o0);
      }
    }
    fold_store_record(red, s, q, partial, bn_blk(), C, cb, tc, tr, tpc, rl);
    if constexpr (PK) {
      red[0][threadIdx.x] = gm;
      red[1][threadIdx.x] = xm;
      __syncthreads();
      if (tr == 0) {
        for (int k = 1; k < rl; ++k) {
          const f32x4 a = red[0][k * tpc + tc], b = red[1][k * tpc + tc];
          gm.x = fmaxf(gm.x, a.x); gm.y = fmaxf(gm.y, a.y); gm.z = fmaxf(gm.z, a.z); gm.w = fmaxf(gm.w, a.w);
          xm.x = fmaxf(xm.x, b.x); xm.y = fmaxf(xm.y, b.y); xm.z = fmaxf(xm.z, b.z); xm.w = fmaxf(xm.w, b.w);
        }
        float* o = pmax + (size_t)bn_blk() * 2 * C;
        *reinterpret_cast<f32x4*>(o + cb * 4) = gm;
        *reinterpret_cast<f32x4*>(o + C + cb * 4) = xm;
      }
      __syncthreads();
    }
  }
}

// coef[0][C] = gamma*invstd ; coef[1][C] = mean(g) ; coef[2][C] = mean(g*xhat)  (0 when !train)
// FC channels x 256 / FC lanes per workgroup: 8 x 32 by default; 2 x 128 (four times the workgroups) when the partials are many
// (the body is a function of its own so that bn_bwd_final_dual_kernel below can finish two BatchNorms in one launch)
template <int FC>
__device__ __forceinline__ void bn_bwd_final_body(const float* __restrict__ partial, int nblk, int C,
                                                  double inv_rows, const float* __restrict__ gamma,
                                                  const float* __restrict__ invstd,
                                                  float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                  float* __restrict__ coef, int train,
                                                  uint32_t* __restrict__ amax,
                                                  const float* __restrict__ pmax) {
  // pmax == nullptr: stage 3 accumulates max|dx| into the slots (zeroed here).  pmax != nullptr (packed dx): the slots
  // arrive ZERO and every workgroup raises one of them to a bound of its channels' |dx| before stage 3 starts:
  //   |dx_c| = |k0 (g - k1 - xhat k2)| <= |k0| (max|g_c| + |k1| + max|xhat_c| |k2|)
  // (tight to a factor of ~2; an upper bound is all a scale needs, x3_common.hpp).
  if (!pmax) zero_amax(amax);
  float gmax = 0.f, xmax = 0.f;
  if (pmax) {
    __shared__ float mred[4][FC];
    const int tc = threadIdx.x % FC, tl = threadIdx.x / FC;
    const int cc = bn_fin_group() * FC + tc;
    if (cc < C) {
      const float* pm = pmax + cc;
      const size_t st = (size_t)2 * C;
      int b = tl;
      for (; b + 3 * (256 / FC) < nblk; b += 4 * (256 / FC)) {   // eight independent loads in flight per lane
        const float g0 = pm[b * st], g1 = pm[(b + (256 / FC)) * st], g2 = pm[(b + 2 * (256 / FC)) * st],
                    g3 = pm[(b + 3 * (256 / FC)) * st];
        const float x0 = pm[b * st + C], x1 = pm[(b + (256 / FC)) * st + C], x2 = pm[(b + 2 * (256 / FC)) * st + C],
                    x3 = pm[(b + 3 * (256 / FC)) * st + C];
        gmax = fmaxf(gmax, fmaxf(fmaxf(g0, g1), fmaxf(g2, g3)));
        xmax = fmaxf(xmax, fmaxf(fmaxf(x0, x1), fmaxf(x2, x3)));
      }
      for (; b < nblk; b += (256 / FC)) {
        gmax = fmaxf(gmax, pm[b * st]);
        xmax = fmaxf(xmax, pm[b * st + C]);
      }
    }
    auto mx = [](float a, float b) { return fmaxf(a, b); };
    gmax = fold_channel_lanes<FC>(gmax, mred, mx);
    xmax = fold_channel_lanes<FC>(xmax, mred, mx);
  }
  int c;
  double s, q;
  if (!reduce_partials<FC>(partial, nblk, C, c, s, q)) return;
  if (dbeta) dbeta[c] = (float)s;
  if (dgamma) dgamma[c] = (float)q;
  const float g = gamma ? gamma[c] : 1.f;
  const float k0 = g * invstd[c], k1 = train ? (float)(s * inv_rows) : 0.f, k2 = train ? (float)(q * inv_rows) : 0.f;
  coef[c] = k0;
  coef[C + c] = k1;
  coef[2 * C + c] = k2;
  if (pmax) {
    const float bound = fabsf(k0) * (gmax + fabsf(k1) + xmax * fabsf(k2));
    uint32_t bits = __builtin_bit_cast(uint32_t, bound);
    if (bound != bound) bits = 0x7fc00000u;
    // slot 0 only (C / 8 workgroups in this launch: nothing to spread), so that the apply pass — one 16-byte element
    // per thread — reads ONE word instead of folding 64 cache lines per wave (measured: the fold cost the pass 5 %)
    if (bits) atomicMax(&amax[0], bits);
  }
}
template <int FC = kFinCh>
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float* __restrict__ partial, int nblk, int C,
                                                           double inv_rows, const float* __restrict__ gamma,
                                                           const float* __restrict__ invstd,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           float* __restrict__ coef, int train,
                                                           uint32_t* __restrict__ amax,
                                                           const float* __restrict__ pmax) {
  bn_bwd_final_body<FC>(partial, nblk, C, inv_rows, gamma, invstd, dgamma, dbeta, coef, train, amax, pmax);
}

// dx = coef0 * (g - coef1 - xhat*coef2); one 16-byte element per thread (see bn_apply_kernel), the per-channel
// vectors read through L1.  PK: dx is written as packed words of dx / s (x3_common.hpp: pack_hl), s from the bound the
// finalisation left in `amax` — the tensor is the producing convolution's dy operand and nothing else.
template <bool PK>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ coef,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ dx,
                                                           size_t n4, int C, int relu, uint32_t* __restrict__ amax,
                                                           const uint32_t* __restrict__ bits = nullptr) {
  const size_t base = (size_t)bn_blk() * 256;
  const size_t i = base + threadIdx.x;
  const bool valid = i < n4;
  f32x4 out = {0.f, 0.f, 0.f, 0.f};
  float pk_inv = 1.f;
  if constexpr (PK) pk_inv = op_scale(amax[0]).inv;   // the finalisation's bound lives in slot 0 alone
  if (valid) {
    const int c4 = C >> 2;
    const int c = chunk_of(base, c4);
    const f32x4 one4 = {1.f, 1.f, 1.f, 1.f}, z4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 k0 = reinterpret_cast<const f32x4*>(coef)[c];
    const f32x4 k1 = reinterpret_cast<const f32x4*>(coef + C)[c];
    const f32x4 k2 = reinterpret_cast<const f32x4*>(coef + 2 * C)[c];
    const f32x4 mu = reinterpret_cast<const f32x4*>(mean)[c];
    const f32x4 is = reinterpret_cast<const f32x4*>(invstd)[c];
    f32x4 g = bn_ld(dy, i);
    const f32x4 xv = bn_ld(x, i);
    if (relu == 3) {
      g = relu_bits_mask(g, bits, i);
    } else if (relu) {
      f32x4 yy;
      if (relu == 1) {
        yy = reinterpret_cast<const f32x4*>(y)[i];
      } else {  // the forward's pre-activation, same sc/sh arithmetic as bn_stats_final_kernel
        const f32x4 sc = (gamma ? reinterpret_cast<const f32x4*>(gamma)[c] : one4) * is;
        const f32x4 sh = (beta ? reinterpret_cast<const f32x4*>(beta)[c] : z4) - mu * sc;
        yy = xv * sc + sh;
      }
      g = relu_mask(g, yy);
    }
    const f32x4 xh = (xv - mu) * is;
    out = k0 * (g - k1 - xh * k2);
    if constexpr (PK) {
      reinterpret_cast<u32x4*>(dx)[i] = pack_hl4(out, pk_inv);
    } else {
      reinterpret_cast<f32x4*>(dx)[i] = out;
    }
  }
  if constexpr (!PK)
    if (amax) block_absmax(out, valid, amax);   // all lanes of the workgroup arrive here together
}

// Statistics that arrive as per-row-part records (count, mean, M2) from the producing convolution's epilogue
// (igemm_common.hpp: igemm_store_rows_stats): Chan's pairwise merge in fp64, 32 lanes per channel over a fixed strided
// subset each, then the 32 lanes folded in index order — the same outputs as bn_stats_final_kernel, no pass over x.
// FC channels x FL record lanes per workgroup (FC * FL = 256): 8 x 32 for the small maps; 2 x 128 where a channel has
// hundreds of records (the 128^2 maps: 2048 per channel — at 32 lanes each lane walked 64 strided records: 9-47 us a launch)
// (the body is a function of its own so that bn_parts_final_dual_kernel below can merge two BatchNorms' records in one launch)
template <int FC, int FL>
__device__ __forceinline__ void bn_parts_final_body(const float* __restrict__ parts, int nparts, int C,
                                                    double rows, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta,
                                                    float* __restrict__ running_mean,
                                                    float* __restrict__ running_var, float momentum, float eps,
                                                    float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                    float* __restrict__ scale_shift,
                                                    uint32_t* __restrict__ amax, int pack) {
  // pack == 0: the apply pass accumulates max|y| into the slots (zeroed here).  pack != 0 (y will be written packed,
  // EVK_BN_PACK_Y): the slots arrive ZERO and slot 0 is raised HERE to a bound of |y|, from the records alone: a row of
  // record i deviates from the record's mean by at most sqrt(M2_i) (one term of the sum), so
  //   |x - mean_c| <= E_c + |pivot - mean_c|,  E_c = max_i (sqrt(M2_i) + |mean_i - pivot|),  |y_c| <= |sc| (..) + |beta|
  // — about 2-3x the true maximum at 64..256 rows per record; an upper bound is all a scale needs (x3_common.hpp).
  if (!pack) zero_amax(amax);
  float E = 0.f;
  // With a common pivot p (the first record's mean) the merge of all records is three plain sums,
  //   N = sum n_i,  A = sum n_i (mean_i - p),  B = sum [M2_i + n_i (mean_i - p)^2]:  mean = p + A/N,  M2 = B - A^2/N
  // (Chan's pairwise formula telescoped; no division inside the loop, no order dependence beyond the fixed one below).
  __shared__ double red[4][FC];
  const int tc = threadIdx.x % FC, tl = threadIdx.x / FC;
  const int c = bn_fin_group() * FC + tc;
  double N = 0.0, A = 0.0, B = 0.0, piv = 0.0;
  if (c < C) {
    const size_t st = (size_t)3 * C;
    piv = (double)parts[C + c];
    const float* r = parts + c;
    int b = tl;
    for (; b + 3 * FL < nparts; b += 4 * FL) {   // four independent records in flight per lane
      const float* r0 = r + (size_t)b * st;
      const float* r1 = r0 + (size_t)FL * st;
      const float* r2 = r1 + (size_t)FL * st;
      const float* r3 = r2 + (size_t)FL * st;
      const float n0 = r0[0], m0 = r0[C], q0 = r0[2 * C], n1 = r1[0], m1 = r1[C], q1 = r1[2 * C];
      const float n2 = r2[0], m2 = r2[C], q2 = r2[2 * C], n3 = r3[0], m3 = r3[C], q3 = r3[2 * C];
      const double d0 = (double)m0 - piv, d1 = (double)m1 - piv, d2 = (double)m2 - piv, d3 = (double)m3 - piv;
      N += ((double)n0 + (double)n1) + ((double)n2 + (double)n3);
      A += ((double)n0 * d0 + (double)n1 * d1) + ((double)n2 * d2 + (double)n3 * d3);
      B += (((double)q0 + (double)n0 * d0 * d0) + ((double)q1 + (double)n1 * d1 * d1)) +
           (((double)q2 + (double)n2 * d2 * d2) + ((double)q3 + (double)n3 * d3 * d3));
      if (pack) {
        const float e0 = n0 > 0.f ? sqrtf(q0) + fabsf((float)d0) : 0.f, e1 = n1 > 0.f ? sqrtf(q1) + fabsf((float)d1) : 0.f;
        const float e2 = n2 > 0.f ? sqrtf(q2) + fabsf((float)d2) : 0.f, e3 = n3 > 0.f ? sqrtf(q3) + fabsf((float)d3) : 0.f;
        E = fmaxf(E, fmaxf(fmaxf(e0, e1), fmaxf(e2, e3)));
      }
    }
    for (; b < nparts; b += FL) {
      const float* r0 = r + (size_t)b * st;
      const double n0 = (double)r0[0], d0 = (double)r0[C] - piv;
      N += n0;
      A += n0 * d0;
      B += (double)r0[2 * C] + n0 * d0 * d0;
      if (pack && n0 > 0.0) E = fmaxf(E, sqrtf(r0[2 * C]) + fabsf((float)d0));
    }
  }
  __shared__ float ered[4][FC];
  auto add = [](double a, double b) { return a + b; };
  N = fold_channel_lanes<FC>(N, red, add);
  A = fold_channel_lanes<FC>(A, red, add);
  B = fold_channel_lanes<FC>(B, red, add);
  if (pack) E = fold_channel_lanes<FC>(E, ered, [](float a, float b) { return fmaxf(a, b); });
  if (tl != 0 || c >= C) return;
  const double mean = N > 0.0 ? piv + A / N : 0.0;
  double var = N > 0.0 ? (B - A * A / N) / N : 0.0;
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float meanf = (float)mean;
  save_mean[c] = meanf;
  save_invstd[c] = invstd;
  const double unbias = rows > 1.0 ? rows / (rows - 1.0) : 1.0;
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * unbias);
  const float g = gamma ? gamma[c] : 1.f, bb = beta ? beta[c] : 0.f;
  const float sc = g * invstd;
  scale_shift[c] = sc;
  scale_shift[C + c] = bb - meanf * sc;
  if (pack) {
    const float bound = fabsf(sc) * (E * 1.001f + fabsf((float)(piv - mean))) + fabsf(bb);
    uint32_t bits = __builtin_bit_cast(uint32_t, bound);
    if (bound != bound) bits = 0x7fc00000u;
    if (bits) atomicMax(&amax[0], bits);   // slot 0 alone: the apply pass reads one word (see bn_bwd_final_kernel)
  }
}
template <int FC, int FL>
__global__ __launch_bounds__(256) void bn_parts_final_kernel(const float* __restrict__ parts, int nparts, int C,
                                                             double rows, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, float momentum, float eps,
                                                             float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                             float* __restrict__ scale_shift,
                                                             uint32_t* __restrict__ amax, int pack) {
  bn_parts_final_body<FC, FL>(parts, nparts, C, rows, gamma, beta, running_mean, running_var, momentum, eps, save_mean,
                              save_invstd, scale_shift, amax, pack);
}

// The two finalisations of a block end with a shortcut convolution in ONE launch each: blockIdx.y selects the BatchNorm, the
// workgroups of a row do what the single kernels' workgroups do (bn_fin_group and zero_amax look at blockIdx.x alone).
struct BnPartsFinalSet {
  const float* parts;
  int nparts;
  const float *gamma, *beta;
  float *running_mean, *running_var;
  float momentum, eps;
  float *save_mean, *save_invstd, *scale_shift;
  uint32_t* amax;
};
template <int FC, int FL>
__global__ __launch_bounds__(256) void bn_parts_final_dual_kernel(BnPartsFinalSet a, BnPartsFinalSet b, int C, double rows) {
  const BnPartsFinalSet s = blockIdx.y ? b : a;
  bn_parts_final_body<FC, FL>(s.parts, s.nparts, C, rows, s.gamma, s.beta, s.running_mean, s.running_var, s.momentum, s.eps,
                              s.save_mean, s.save_invstd, s.scale_shift, s.amax, 0);
}
struct BnBwdFinalSet {
  const float *partial, *gamma, *invstd;
  float *dgamma, *dbeta, *coef;
  uint32_t* amax;
  const float* pmax;
};
__global__ __launch_bounds__(256) void bn_bwd_final_dual_kernel(BnBwdFinalSet a, BnBwdFinalSet b, int nblk, int C,
                                                                double inv_rows) {
  const BnBwdFinalSet s = blockIdx.y ? b : a;
  bn_bwd_final_body<kFinCh>(s.partial, nblk, C, inv_rows, s.gamma, s.invstd, s.dgamma, s.dbeta, s.coef, 1, s.amax, s.pmax);
}

// (A one-launch backward for small maps — every thread's rows in registers across two grid-wide barriers, 3 tensor transfers
// instead of 5 — lived here in rounds 2 and 3.  Its grid had to be resident as a whole, so it was off beside the weight-
// gradient side stream, under RCCL and on any stream but one; at the end it ran on ~1 call in 30 of the default path.
// Removed in round 4: EVK_BN_FUSED=1 vs 0 measured 547.7 / 547.4 tiles/s on the default path, 524.4 / 519.4 single-stream,
// 521.6 / 521.2 captured, same box — and with it went the spin barrier, its device words and the stream ownership.)

// record lanes per channel of the merge: bn_parts_final_kernel<256 / lanes, lanes>
static int parts_final_lanes(int nparts) { return nparts >= 1024 ? 256 : (nparts >= 512 ? 128 : 32); }

void launch_parts_final(hipStream_t st, const float* parts, int nparts, int C, double rows, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                        float* save_mean, float* save_invstd, float* scale_shift, uint32_t* amax, int pack) {
  // one channel per workgroup above 1024 records — eight records per lane, all in flight at once (level with the two-channel
  // form on the step, ahead in the family: 407 vs 460 us per step)
  const int fl = parts_final_lanes(nparts);
#define EVK_PARTS_FINAL(FC, FL)                                                                                            \
  hipLaunchKernelGGL((bn_parts_final_kernel<FC, FL>), dim3((C + FC - 1) / FC), dim3(256), 0, st, parts, nparts, C, rows, gamma, \
                     beta, running_mean, running_var, momentum, eps, save_mean, save_invstd, scale_shift, amax, pack)
  if (fl == 256) EVK_PARTS_FINAL(1, 256);
  else if (fl == 128) EVK_PARTS_FINAL(2, 128);
  else EVK_PARTS_FINAL(8, 32);
#undef EVK_PARTS_FINAL
}

void launch_bn_bwd_final(hipStream_t st, const float* partial, int nblk, int C, int64_t rows, const float* gamma,
                         const float* invstd, float* dgamma, float* dbeta, float* coef, int train, uint32_t* amax,
                         const float* pmax) {
  // (two channels x 128 lanes per workgroup, four times the workgroups, measured -0.2 % chosen from 128 partials up and -2.5 %
  // everywhere: the 8-byte pieces of a partial row it reads cost more than the shorter chains save — removed)
  hipLaunchKernelGGL(bn_bwd_final_kernel<kFinCh>, dim3((C + kFinCh - 1) / kFinCh), dim3(256), 0, st, partial, nblk, C,
                     1.0 / (double)rows, gamma, invstd, dgamma, dbeta, coef, train ? 1 : 0, amax, pmax);
}

// the forward apply pass over a [rows][C] map (pack: y as packed words, EVK_BN_PACK_Y)
static void launch_bn_apply(hipStream_t st, bool pack, const float* x, const float* residual, const float* scale_shift,
                            float* y, int64_t rows, int C, uint32_t flags, uint32_t* amax, uint32_t* relu_bits = nullptr) {
  const size_t n4 = (size_t)rows * C / 4;
  EVK_BN_LAUNCH_PK(bn_apply_kernel, pack, dim3(oneshot_grid(n4)), 0, st, x, residual, scale_shift, y, n4, C,
                   (flags & EVK_BN_RELU) ? 1 : 0, amax, relu_bits);
}

// ---- The end of a residual block whose shortcut is a convolution (`layerN.0`): out = relu(bn_a(za) + bn_b(zb)), za the
// main branch's last convolution output, zb the shortcut convolution's.  The passes below take BOTH maps, so the shortcut's
// normalised copy yb = bn_b(zb) is never stored: forward 3 transfers of the map instead of 5, backward reduce 3 instead of 4,
// backward apply 5 instead of 6.  New kernels only: the single-map kernels above keep their code.

// y = relu((za*sca + sha) + (zb*scb + shb)), ReLU bits, max|y|: bn_apply_kernel's residual form with the residual computed in
// registers.  The shortcut term is an expression of its own, so it is rounded as the stored yb was (one fused multiply-add)
// before the add.
__global__ __launch_bounds__(256) void bn_apply_dual_kernel(const float* __restrict__ za, const float* __restrict__ zb,
                                                            const float* __restrict__ scale_shift_a,
                                                            const float* __restrict__ scale_shift_b, float* __restrict__ y,
                                                            size_t n4, int C, uint32_t* __restrict__ amax,
                                                            uint32_t* __restrict__ relu_bits) {
  const size_t base = (size_t)bn_blk() * 256;
  const size_t i = base + threadIdx.x;
  const bool valid = i < n4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (valid) {
    const int c4 = C >> 2;
    const int cb = chunk_of(base, c4);
    const f32x4 sca = reinterpret_cast<const f32x4*>(scale_shift_a)[cb];
    const f32x4 sha = reinterpret_cast<const f32x4*>(scale_shift_a + C)[cb];
    const f32x4 scb = reinterpret_cast<const f32x4*>(scale_shift_b)[cb];
    const f32x4 shb = reinterpret_cast<const f32x4*>(scale_shift_b + C)[cb];
    const f32x4 yb = bn_ld(zb, i) * scb + shb;
    v = bn_ld(za, i) * sca + sha;
    v += yb;
  }
  // every lane of a wave takes part (v = 0 where the element does not exist); a wave wholly past the end has no chunk
  if (((i >> 6) << 6) < n4) relu_bits_store(relu_bits, i >> 6, v.x > 0.f, v.y > 0.f, v.z > 0.f, v.w > 0.f);
  if (valid) {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    reinterpret_cast<f32x4*>(y)[i] = v;
  }
  if (amax) block_absmax(v, valid, amax);   // all lanes of the workgroup arrive here together
}

// Backward stage 1 for both maps: g = dy where the block's ReLU bit is set, masked ONCE;
// partial_a[blk] = (sum g, sum g * xhat_a), partial_b[blk] = (sum g, sum g * xhat_b) — bn_bwd_partial_kernel's plan, row
// order and fold, so each record has the bits the single-map pass gives.  PK: pmax_a / pmax_b as bn_bwd_partial_kernel<true>.
template <bool PK>
__global__ __launch_bounds__(256) void bn_bwd_partial_dual_kernel(
    const float* __restrict__ dy, const float* __restrict__ xa, const float* __restrict__ xb,
    const float* __restrict__ mean_a, const float* __restrict__ invstd_a, const float* __restrict__ mean_b,
    const float* __restrict__ invstd_b, float* __restrict__ partial_a, float* __restrict__ partial_b, int64_t rows, int C,
    int64_t rows_per_blk, int tpc, int rl, float* __restrict__ pmax_a, float* __restrict__ pmax_b,
    const uint32_t* __restrict__ bits) {
  __shared__ f32x4 red[2][256];
  const int c4 = C >> 2;
  const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
  const int64_t r0 = (int64_t)bn_blk() * rows_per_blk;
  const int64_t r1 = min(rows, r0 + rows_per_blk);
  for (int cb = tc; cb < c4; cb += tpc) {
    const f32x4 mua = *reinterpret_cast<const f32x4*>(mean_a + cb * 4);
    const f32x4 isa = *reinterpret_cast<const f32x4*>(invstd_a + cb * 4);
    const f32x4 mub = *reinterpret_cast<const f32x4*>(mean_b + cb * 4);
    const f32x4 isb = *reinterpret_cast<const f32x4*>(invstd_b + cb * 4);
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, qa = {0.f, 0.f, 0.f, 0.f}, qb = {0.f, 0.f, 0.f, 0.f};
    f32x4 gm = {0.f, 0.f, 0.f, 0.f}, xma = {0.f, 0.f, 0.f, 0.f}, xmb = {0.f, 0.f, 0.f, 0.f};
    if (tr < rl) {
      auto one = [&](const f32x4 gin, const f32x4 xva, const f32x4 xvb, size_t off) {
        const f32x4 g = relu_bits_mask(gin, bits, off >> 2);
        s += g;
        const f32x4 xha = (xva - mua) * isa;
        qa += g * xha;
        const f32x4 xhb = (xvb - mub) * isb;
        qb += g * xhb;
        if constexpr (PK) {
          gm.x = fmaxf(gm.x, fabsf(g.x)); gm.y = fmaxf(gm.y, fabsf(g.y));
          gm.z = fmaxf(gm.z, fabsf(g.z)); gm.w = fmaxf(gm.w, fabsf(g.w));
          xma.x = fmaxf(xma.x, fabsf(xha.x)); xma.y = fmaxf(xma.y, fabsf(xha.y));
          xma.z = fmaxf(xma.z, fabsf(xha.z)); xma.w = fmaxf(xma.w, fabsf(xha.w));
          xmb.x = fmaxf(xmb.x, fabsf(xhb.x)); xmb.y = fmaxf(xmb.y, fabsf(xhb.y));
          xmb.z = fmaxf(xmb.z, fabsf(xhb.z)); xmb.w = fmaxf(xmb.w, fabsf(xhb.w));
        }
      };
      int64_t r = r0 + tr;
      const int64_t st = rl;
      // four rows per trip: 12 independent 16-byte loads in flight per lane
      for (; r + 3 * st < r1; r += 4 * st) {
        const size_t o0 = (size_t)r * C + cb * 4, o1 = (size_t)(r + st) * C + cb * 4;
        const size_t o2 = (size_t)(r + 2 * st) * C + cb * 4, o3 = (size_t)(r + 3 * st) * C + cb * 4;
        const f32x4 g0 = bp_ld(dy + o0), g1 = bp_ld(dy + o1);
        const f32x4 g2 = bp_ld(dy + o2), g3 = bp_ld(dy + o3);
        const f32x4 a0 = bp_ld(xa + o0), a1 = bp_ld(xa + o1);
        const f32x4 a2 = bp_ld(xa + o2), a3 = bp_ld(xa + o3);
        const f32x4 b0 = bp_ld(xb + o0), b1 = bp_ld(xb + o1);
        const f32x4 b2 = bp_ld(xb + o2), b3 = bp_ld(xb + o3);
        one(g0, a0, b0, o0);
        one(g1, a1, b1, o1);
        one(g2, a2, b2, o2);
        one(g3, a3, b3, o3);
      }
      for (; r < r1; r += st) {
        const size_t o0 = (size_t)r * C + cb * 4;
        one(bp_ld(dy + o0), bp_ld(xa + o0), bp_ld(xb + o0), o0);
      }
    }
    fold_store_record(red, s, qa, partial_a, bn_blk(), C, cb, tc, tr, tpc, rl);
    fold_store_record(red, s, qb, partial_b, bn_blk(), C, cb, tc, tr, tpc, rl);
    if constexpr (PK) {
      red[0][threadIdx.x] = gm;
      red[1][threadIdx.x] = xma;
      __syncthreads();
      if (tr == 0) {
        for (int k = 1; k < rl; ++k) {
          const f32x4 a = red[0][k * tpc + tc], b = red[1][k * tpc + tc];
          gm.x = fmaxf(gm.x, a.x); gm.y = fmaxf(gm.y, a.y); gm.z = fmaxf(gm.z, a.z); gm.w = fmaxf(gm.w, a.w);
          xma.x = fmaxf(xma.x, b.x); xma.y = fmaxf(xma.y, b.y); xma.z = fmaxf(xma.z, b.z); xma.w = fmaxf(xma.w, b.w);
        }
      }
      __syncthreads();
      red[0][threadIdx.x] = xmb;
      __syncthreads();
      if (tr == 0) {
        for (int k = 1; k < rl; ++k) {
          const f32x4 b = red[0][k * tpc + tc];
          xmb.x = fmaxf(xmb.x, b.x); xmb.y = fmaxf(xmb.y, b.y); xmb.z = fmaxf(xmb.z, b.z); xmb.w = fmaxf(xmb.w, b.w);
        }
        float* oa = pmax_a + (size_t)bn_blk() * 2 * C;
        float* ob = pmax_b + (size_t)bn_blk() * 2 * C;
        *reinterpret_cast<f32x4*>(oa + cb * 4) = gm;
        *reinterpret_cast<f32x4*>(oa + C + cb * 4) = xma;
        *reinterpret_cast<f32x4*>(ob + cb * 4) = gm;
        *reinterpret_cast<f32x4*>(ob + C + cb * 4) = xmb;
      }
      __syncthreads();
    }
  }
}

// Backward stage 3 for both maps: dxa = ka0 * (g - ka1 - xhat_a*ka2), dxb likewise from the second coefficient set; g is
// read and masked once.  PKA / PKB: that output packed under the bound its finalisation left in slot 0 of its `amax`.
template <bool PKA, bool PKB>
__global__ __launch_bounds__(256) void bn_bwd_apply_dual_kernel(
    const float* __restrict__ dy, const float* __restrict__ xa, const float* __restrict__ xb,
    const float* __restrict__ mean_a, const float* __restrict__ invstd_a, const float* __restrict__ coef_a,
    const float* __restrict__ mean_b, const float* __restrict__ invstd_b, const float* __restrict__ coef_b,
    float* __restrict__ dxa, float* __restrict__ dxb, size_t n4, int C, uint32_t* __restrict__ amax_a,
    uint32_t* __restrict__ amax_b, const uint32_t* __restrict__ bits) {
  const size_t base = (size_t)bn_blk() * 256;
  const size_t i = base + threadIdx.x;
  const bool valid = i < n4;
  f32x4 outa = {0.f, 0.f, 0.f, 0.f}, outb = {0.f, 0.f, 0.f, 0.f};
  float pk_inv_a = 1.f, pk_inv_b = 1.f;
  if constexpr (PKA) pk_inv_a = op_scale(amax_a[0]).inv;
  if constexpr (PKB) pk_inv_b = op_scale(amax_b[0]).inv;
  if (valid) {
    const int c4 = C >> 2;
    const int c = chunk_of(base, c4);
    const f32x4 g = relu_bits_mask(bn_ld(dy, i), bits, i);
    {
      const f32x4 k0 = reinterpret_cast<const f32x4*>(coef_a)[c];
      const f32x4 k1 = reinterpret_cast<const f32x4*>(coef_a + C)[c];
      const f32x4 k2 = reinterpret_cast<const f32x4*>(coef_a + 2 * C)[c];
      const f32x4 mu = reinterpret_cast<const f32x4*>(mean_a)[c];
      const f32x4 is = reinterpret_cast<const f32x4*>(invstd_a)[c];
      const f32x4 xh = (bn_ld(xa, i) - mu) * is;
      outa = k0 * (g - k1 - xh * k2);
      if constexpr (PKA) {
        reinterpret_cast<u32x4*>(dxa)[i] = pack_hl4(outa, pk_inv_a);
      } else {
        reinterpret_cast<f32x4*>(dxa)[i] = outa;
      }
    }
    {
      const f32x4 k0 = reinterpret_cast<const f32x4*>(coef_b)[c];
      const f32x4 k1 = reinterpret_cast<const f32x4*>(coef_b + C)[c];
      const f32x4 k2 = reinterpret_cast<const f32x4*>(coef_b + 2 * C)[c];
      const f32x4 mu = reinterpret_cast<const f32x4*>(mean_b)[c];
      const f32x4 is = reinterpret_cast<const f32x4*>(invstd_b)[c];
      const f32x4 xh = (bn_ld(xb, i) - mu) * is;
      outb = k0 * (g - k1 - xh * k2);
      if constexpr (PKB) {
        reinterpret_cast<u32x4*>(dxb)[i] = pack_hl4(outb, pk_inv_b);
      } else {
        reinterpret_cast<f32x4*>(dxb)[i] = outb;
      }
    }
  }
  // all lanes of the workgroup arrive here together; block_absmax's LDS words are free again after the barrier between
  if constexpr (!PKA)
    if (amax_a) block_absmax(outa, valid, amax_a);
  if constexpr (!PKA && !PKB) __syncthreads();
  if constexpr (!PKB)
    if (amax_b) block_absmax(outb, valid, amax_b);
}

// The (packed dz of the main branch, packed dz of the shortcut) forms of bn_bwd_apply_dual_kernel that exist: what the
// ResNet-50 / ResNet-18 blocks produce — both packed (the f16x2 default), both plain (another arithmetic, observers), plain
// main + packed shortcut (a BasicBlock whose 3x3 takes the planar weight gradient).  The fourth takes the two-call path.
static bool bn_dual_fused(bool pack_a, bool pack_b) { return !(pack_a && !pack_b); }

}  // namespace evk

using namespace evk;

extern "C" size_t evk_bn_workspace_bytes(int64_t rows, int32_t C) {
  return rows > 0 && C > 0 ? BnWorkspace::bytes(C) : 0;
}

// Host only (no launch): the plan the reduce passes take for a [rows][C] map.  kind 0: evk_bn_fwd_train / evk_bn_bwd / the
// staged entry points; kind 1: evk_bn_relu_pool_bwd.  out = {nblk, rows_per_blk, tpc, rl, quad nblk, quads per workgroup}
// (the last two: the split of an even map into 2 x 2 quads, kind 1 with rows % 4 == 0, else 0).  kind 2: the merge of `rows`
// statistics records (launch_parts_final): out = {workgroups, 0, channels per workgroup, record lanes per channel, 0, 0}.
extern "C" int evk_bn_plan(int64_t rows, int32_t C, int32_t kind, int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "bn_plan: null pointer");
  int rc = bn_check("bn_plan", rows, C, nullptr, 0, 0);
  if (rc) return rc;
  EVK_REQUIRE(kind >= 0 && kind <= 2 && (kind == 0 || rows < 0x7fffffffLL), EVK_E_UNSUPPORTED,
              "bn_plan: rows=%lld C=%d kind=%d", (long long)rows, C, kind);
  if (kind == 2) {
    const int fl = parts_final_lanes((int)rows), fc = 256 / fl;
    out[0] = (C + fc - 1) / fc;
    out[2] = fc;
    out[3] = fl;
    out[1] = out[4] = out[5] = 0;
    return EVK_OK;
  }
  const BnPlan pl = kind ? bn_plan(rows, C, 65536, kMaxStatBlocks) : bn_plan(rows, C);
  EVK_REQUIRE(pl.rows_per_blk <= 0x7fffffffLL, EVK_E_UNSUPPORTED, "bn_plan: rows=%lld do not fit the answer", (long long)rows);
  out[0] = pl.nblk;
  out[1] = (int32_t)pl.rows_per_blk;
  out[2] = pl.tpc;
  out[3] = pl.rl;
  out[4] = out[5] = 0;
  if (kind == 1 && rows % 4 == 0) {
    int nblk, qpb;
    bn_quad_split(rows, pl, nblk, qpb);
    out[4] = nblk;
    out[5] = qpb;
  }
  return EVK_OK;
}

extern "C" int evk_bn_fwd_train(const float* x, const float* residual, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, float momentum, float eps, float* y,
                                float* save_mean, float* save_invstd, int64_t rows, int32_t C, uint32_t flags,
                                void* workspace, size_t workspace_bytes, uint32_t* y_absmax, void* stream) {
  EVK_REQUIRE(x && y && save_mean && save_invstd, EVK_E_INVALID, "bn_fwd_train: null pointer");
  int rc = bn_check("bn_fwd_train", rows, C, workspace, workspace_bytes, BnWorkspace::bytes(C));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const BnPlan pl = bn_plan(rows, C);
  const BnWorkspace ws(workspace, C);
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(pl.nblk), dim3(256), 0, st, x, ws.partial, rows, C, pl.rows_per_blk,
                     pl.tpc, pl.rl);
  rc = check_launch("bn_stats_partial");
  if (rc) return rc;
  const double unbias = rows > 1 ? (double)rows / (double)(rows - 1) : 1.0;
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(256), 0, st, x, ws.partial, pl.nblk, C,
                     1.0 / (double)rows, unbias, gamma, beta, running_mean, running_var, momentum, eps, save_mean,
                     save_invstd, ws.coef, y_absmax);
  rc = check_launch("bn_stats_final");
  if (rc) return rc;
  launch_bn_apply(st, false, x, residual, ws.coef, y, rows, C, flags, y_absmax);
  return check_launch("bn_apply");
}

extern "C" int evk_bn_fwd_train_parts_bits(const float* x, const float* residual, const float* gamma, const float* beta,
                                           float* running_mean, float* running_var, float momentum, float eps, float* y,
                                           float* save_mean, float* save_invstd, int64_t rows, int32_t C, uint32_t flags,
                                           const float* parts, int32_t nparts, void* workspace, size_t workspace_bytes,
                                           uint32_t* y_absmax, uint32_t* relu_bits, void* stream) {
  EVK_REQUIRE(x && y && save_mean && save_invstd && parts && nparts > 0, EVK_E_INVALID, "bn_fwd_train_parts: bad argument");
  int rc = bn_check("bn_fwd_train_parts", rows, C, workspace, workspace_bytes, BnWorkspace::bytes(C));
  if (rc) return rc;
  const bool pack = (flags & EVK_BN_PACK_Y) != 0;
  EVK_REQUIRE(!pack || (y_absmax && !residual), EVK_E_INVALID,
              "bn_fwd_train_parts: EVK_BN_PACK_Y needs y_absmax (slots zero on entry) and no residual");
  hipStream_t st = (hipStream_t)stream;
  float* scale_shift = BnWorkspace(workspace, C).coef;
  launch_parts_final(st, parts, nparts, C, (double)rows, gamma, beta, running_mean, running_var, momentum, eps, save_mean,
                     save_invstd, scale_shift, y_absmax, pack ? 1 : 0);
  rc = check_launch("bn_parts_final");
  if (rc) return rc;
  launch_bn_apply(st, pack, x, residual, scale_shift, y, rows, C, flags, y_absmax, relu_bits);
  return check_launch("bn_apply");
}
extern "C" int evk_bn_fwd_train_parts(const float* x, const float* residual, const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, float momentum, float eps, float* y,
                                      float* save_mean, float* save_invstd, int64_t rows, int32_t C, uint32_t flags,
                                      const float* parts, int32_t nparts, void* workspace, size_t workspace_bytes,
                                      uint32_t* y_absmax, void* stream) {
  return evk_bn_fwd_train_parts_bits(x, residual, gamma, beta, running_mean, running_var, momentum, eps, y, save_mean,
                                     save_invstd, rows, C, flags, parts, nparts, workspace, workspace_bytes, y_absmax, nullptr,
                                     stream);
}

extern "C" int evk_bn_fwd_eval(const float* x, const float* residual, const float* gamma, const float* beta,
                               const float* running_mean, const float* running_var, float eps, float* y,
                               float* save_mean, float* save_invstd, int64_t rows, int32_t C, uint32_t flags,
                               void* workspace, size_t workspace_bytes, uint32_t* y_absmax, void* stream) {
  EVK_REQUIRE(x && y && running_mean && running_var, EVK_E_INVALID, "bn_fwd_eval: null pointer");
  int rc = bn_check("bn_fwd_eval", rows, C, workspace, workspace_bytes, 2 * (size_t)C * sizeof(float));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* scale_shift = (float*)workspace;
  hipLaunchKernelGGL(bn_eval_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, st, gamma, beta, running_mean,
                     running_var, eps, C, scale_shift, save_mean, save_invstd, y_absmax);
  rc = check_launch("bn_eval_coef");
  if (rc) return rc;
  launch_bn_apply(st, false, x, residual, scale_shift, y, rows, C, flags, y_absmax);
  return check_launch("bn_apply");
}

extern "C" int evk_bn_bwd_bits(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, float* dx, float* d_residual,
                               float* dgamma, float* dbeta, int64_t rows, int32_t C, uint32_t flags, int32_t train,
                               void* workspace, size_t workspace_bytes, uint32_t* dx_absmax, const uint32_t* relu_bits,
                               void* stream) {
  EVK_REQUIRE(dy && x && save_mean && save_invstd && dx, EVK_E_INVALID, "bn_bwd: null pointer");
  // mask of the incoming gradient: the given bits (the forward's ReLU bits, EVK_BN_RELU set — or, without EVK_BN_RELU, the
  // mask of a gradient that arrives unmasked from a residual block's lazy backward); else from the saved output y when
  // given (needed with a residual), else recomputed from x
  const int relu = relu_bits ? 3 : ((flags & EVK_BN_RELU) ? (y ? 1 : 2) : 0);
  EVK_REQUIRE(relu != 2 || !d_residual, EVK_E_INVALID,
              "bn_bwd: a residual branch needs the forward output y (or its ReLU bits) for the mask");
  int rc = bn_check("bn_bwd", rows, C, workspace, workspace_bytes, BnWorkspace::bytes(C));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const BnPlan pl = bn_plan(rows, C);
  const BnWorkspace ws(workspace, C);
  const bool pack = (flags & EVK_BN_PACK_DX) != 0;
  EVK_REQUIRE(!pack || dx_absmax, EVK_E_INVALID, "bn_bwd: EVK_BN_PACK_DX needs dx_absmax (slots zero on entry)");
  float* pmax = pack ? ws.pmax : nullptr;
  EVK_BN_LAUNCH_PK(bn_bwd_partial_kernel, pack, dim3(pl.nblk), 0, st, dy, x, y, save_mean, save_invstd, gamma, beta, d_residual,
                   ws.partial, rows, C, pl.rows_per_blk, pl.tpc, pl.rl, relu, pmax, relu_bits);
  rc = check_launch("bn_bwd_partial");
  if (rc) return rc;
  launch_bn_bwd_final(st, ws.partial, pl.nblk, C, rows, gamma, save_invstd, dgamma, dbeta, ws.coef, train, dx_absmax, pmax);
  rc = check_launch("bn_bwd_final");
  if (rc) return rc;
  const size_t n4 = (size_t)rows * C / 4;
  // when d_residual holds g already, stage 3 can read it instead of re-masking dy
  const float* gsrc = d_residual ? d_residual : dy;
  const int relu3 = d_residual ? 0 : relu;
  EVK_BN_LAUNCH_PK(bn_bwd_apply_kernel, pack, dim3(oneshot_grid(n4)), 0, st, gsrc, x, y, save_mean, save_invstd, ws.coef, gamma,
                   beta, dx, n4, C, relu3, dx_absmax, relu_bits);
  return check_launch("bn_bwd_apply");
}

extern "C" int evk_bn_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                          const float* save_mean, const float* save_invstd, float* dx, float* d_residual,
                          float* dgamma, float* dbeta, int64_t rows, int32_t C, uint32_t flags, int32_t train,
                          void* workspace, size_t workspace_bytes, uint32_t* dx_absmax, void* stream) {
  return evk_bn_bwd_bits(dy, x, y, gamma, beta, save_mean, save_invstd, dx, d_residual, dgamma, dbeta, rows, C, flags, train,
                         workspace, workspace_bytes, dx_absmax, nullptr, stream);
}

// ---- Both BatchNorms at the end of a residual block with a shortcut convolution (bn_apply_dual_kernel and its neighbours).
// Training mode, both statistics from epilogue records.  workspace: TWO single-map workspaces back to back
// (2 * evk_bn_workspace_bytes): the main branch's records and coefficients in the first, the shortcut's in the second.
extern "C" int evk_bn_fwd_train_parts_dual(const float* za, const float* zb, const float* gamma_a, const float* beta_a,
                                           float* running_mean_a, float* running_var_a, float momentum_a, float eps_a,
                                           const float* gamma_b, const float* beta_b, float* running_mean_b,
                                           float* running_var_b, float momentum_b, float eps_b, float* y, float* save_mean_a,
                                           float* save_invstd_a, float* save_mean_b, float* save_invstd_b, int64_t rows,
                                           int32_t C, const float* parts_a, int32_t nparts_a, const float* parts_b,
                                           int32_t nparts_b, void* workspace, size_t workspace_bytes, uint32_t* y_absmax,
                                           uint32_t* relu_bits, void* stream) {
  EVK_REQUIRE(za && zb && y && save_mean_a && save_invstd_a && save_mean_b && save_invstd_b && parts_a && parts_b &&
                  nparts_a > 0 && nparts_b > 0 && relu_bits,
              EVK_E_INVALID, "bn_fwd_train_parts_dual: bad argument");
  int rc = bn_check("bn_fwd_train_parts_dual", rows, C, workspace, workspace_bytes, 2 * BnWorkspace::bytes(C));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* ss_a = BnWorkspace(workspace, C).coef;
  float* ss_b = BnWorkspace((char*)workspace + BnWorkspace::bytes(C), C).coef;
  // only the main branch's finalisation owns the slots of y_absmax
  const int fl = parts_final_lanes(nparts_a);
  if (fl == parts_final_lanes(nparts_b)) {   // the same form of the merge for both: one launch, a row of workgroups each
    const BnPartsFinalSet sa = {parts_a, nparts_a, gamma_a, beta_a, running_mean_a, running_var_a, momentum_a, eps_a,
                                save_mean_a, save_invstd_a, ss_a, y_absmax};
    const BnPartsFinalSet sb = {parts_b, nparts_b, gamma_b, beta_b, running_mean_b, running_var_b, momentum_b, eps_b,
                                save_mean_b, save_invstd_b, ss_b, nullptr};
#define EVK_PARTS_FINAL_DUAL(FC, FL)                                                                                       \
  hipLaunchKernelGGL((bn_parts_final_dual_kernel<FC, FL>), dim3((C + FC - 1) / FC, 2), dim3(256), 0, st, sa, sb, C, (double)rows)
    if (fl == 256) EVK_PARTS_FINAL_DUAL(1, 256);
    else if (fl == 128) EVK_PARTS_FINAL_DUAL(2, 128);
    else EVK_PARTS_FINAL_DUAL(8, 32);
#undef EVK_PARTS_FINAL_DUAL
    rc = check_launch("bn_parts_final_dual");
    if (rc) return rc;
  } else {
    launch_parts_final(st, parts_b, nparts_b, C, (double)rows, gamma_b, beta_b, running_mean_b, running_var_b, momentum_b,
                       eps_b, save_mean_b, save_invstd_b, ss_b, nullptr, 0);
    rc = check_launch("bn_parts_final");
    if (rc) return rc;
    launch_parts_final(st, parts_a, nparts_a, C, (double)rows, gamma_a, beta_a, running_mean_a, running_var_a, momentum_a,
                       eps_a, save_mean_a, save_invstd_a, ss_a, y_absmax, 0);
    rc = check_launch("bn_parts_final");
    if (rc) return rc;
  }
  const size_t n4 = (size_t)rows * C / 4;
  hipLaunchKernelGGL(bn_apply_dual_kernel, dim3(oneshot_grid(n4)), dim3(256), 0, st, za, zb, (const float*)ss_a,
                     (const float*)ss_b, y, n4, C, y_absmax, relu_bits);
  return check_launch("bn_apply_dual");
}

// 1 when evk_bn_bwd_dual runs the two-map passes for this pair of flags, 0 when it takes the two-call path (host only)
extern "C" int evk_bn_bwd_dual_fused(uint32_t flags_a, uint32_t flags_b) {
  return bn_dual_fused((flags_a & EVK_BN_PACK_DX) != 0, (flags_b & EVK_BN_PACK_DX) != 0) ? 1 : 0;
}

// dza, dzb, both dgamma / dbeta from dy (masked already if it arrived lazily) and the block's ReLU bits.
// flags_a / flags_b: EVK_BN_PACK_DX per output (its absmax buffer then arrives zero).
extern "C" int evk_bn_bwd_dual(const float* dy, const float* za, const float* zb, const float* gamma_a,
                               const float* save_mean_a, const float* save_invstd_a, const float* gamma_b,
                               const float* save_mean_b, const float* save_invstd_b, float* dza, float* dzb, float* dgamma_a,
                               float* dbeta_a, float* dgamma_b, float* dbeta_b, int64_t rows, int32_t C, uint32_t flags_a,
                               uint32_t flags_b, void* workspace, size_t workspace_bytes, uint32_t* dza_absmax,
                               uint32_t* dzb_absmax, const uint32_t* relu_bits, void* stream) {
  EVK_REQUIRE(dy && za && zb && save_mean_a && save_invstd_a && save_mean_b && save_invstd_b && dza && dzb && relu_bits,
              EVK_E_INVALID, "bn_bwd_dual: null pointer");
  int rc = bn_check("bn_bwd_dual", rows, C, workspace, workspace_bytes, 2 * BnWorkspace::bytes(C));
  if (rc) return rc;
  const bool pack_a = (flags_a & EVK_BN_PACK_DX) != 0, pack_b = (flags_b & EVK_BN_PACK_DX) != 0;
  EVK_REQUIRE((!pack_a || dza_absmax) && (!pack_b || dzb_absmax), EVK_E_INVALID,
              "bn_bwd_dual: EVK_BN_PACK_DX needs the output's absmax buffer (slots zero on entry)");
  if (!bn_dual_fused(pack_a, pack_b)) {
    // a form that was not built: the block-end BatchNorm, then the shortcut's, as their own callers run them
    rc = evk_bn_bwd_bits(dy, za, nullptr, gamma_a, nullptr, save_mean_a, save_invstd_a, dza, nullptr, dgamma_a, dbeta_a, rows, C,
                         EVK_BN_RELU | (flags_a & EVK_BN_PACK_DX), 1, workspace, workspace_bytes, dza_absmax, relu_bits, stream);
    if (rc) return rc;
    return evk_bn_bwd_bits(dy, zb, nullptr, gamma_b, nullptr, save_mean_b, save_invstd_b, dzb, nullptr, dgamma_b, dbeta_b, rows,
                           C, flags_b & EVK_BN_PACK_DX, 1, workspace, workspace_bytes, dzb_absmax, relu_bits, stream);
  }
  hipStream_t st = (hipStream_t)stream;
  const BnPlan pl = bn_plan(rows, C);
  const BnWorkspace wa(workspace, C), wb((char*)workspace + BnWorkspace::bytes(C), C);
  const bool pack = pack_a || pack_b;
  EVK_BN_LAUNCH_PK(bn_bwd_partial_dual_kernel, pack, dim3(pl.nblk), 0, st, dy, za, zb, save_mean_a, save_invstd_a, save_mean_b,
                   save_invstd_b, wa.partial, wb.partial, rows, C, pl.rows_per_blk, pl.tpc, pl.rl, pack ? wa.pmax : nullptr,
                   pack ? wb.pmax : nullptr, relu_bits);
  rc = check_launch("bn_bwd_partial_dual");
  if (rc) return rc;
  const BnBwdFinalSet fa = {wa.partial, gamma_a, save_invstd_a, dgamma_a, dbeta_a, wa.coef, dza_absmax, pack_a ? wa.pmax : nullptr};
  const BnBwdFinalSet fb = {wb.partial, gamma_b, save_invstd_b, dgamma_b, dbeta_b, wb.coef, dzb_absmax, pack_b ? wb.pmax : nullptr};
  hipLaunchKernelGGL(bn_bwd_final_dual_kernel, dim3((C + kFinCh - 1) / kFinCh, 2), dim3(256), 0, st, fa, fb, pl.nblk, C,
                     1.0 / (double)rows);
  rc = check_launch("bn_bwd_final_dual");
  if (rc) return rc;
  const size_t n4 = (size_t)rows * C / 4;
#define EVK_BN_APPLY_DUAL(PA, PB)                                                                                            \
  hipLaunchKernelGGL((bn_bwd_apply_dual_kernel<PA, PB>), dim3(oneshot_grid(n4)), dim3(256), 0, st, dy, za, zb, save_mean_a,    \
                     save_invstd_a, (const float*)wa.coef, save_mean_b, save_invstd_b, (const float*)wb.coef, dza, dzb, n4, C, \
                     dza_absmax, dzb_absmax, relu_bits)
  if (pack_a) EVK_BN_APPLY_DUAL(true, true);
  else if (pack_b) EVK_BN_APPLY_DUAL(false, true);
  else EVK_BN_APPLY_DUAL(false, false);
#undef EVK_BN_APPLY_DUAL
  return check_launch("bn_bwd_apply_dual");
}

// ---- BatchNorm around a fused consumer (FS-Relation, pointwise.hip: relation_bn_*): the statistics records of the
// producing convolution are merged into (mean, invstd, scale, shift) WITHOUT an apply pass — the consumer applies scale /
// shift / ReLU while it reads z — and the backward takes per-workgroup partial sums that the consumer's backward formed
// while it had g and z in registers, instead of a reduce pass of its own.
extern "C" int evk_bn_finalize_parts(const float* parts, int32_t nparts, int32_t C, int64_t rows, const float* gamma,
                                     const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                     float* save_mean, float* save_invstd, float* scale_shift, void* stream) {
  EVK_REQUIRE(parts && nparts > 0 && save_mean && save_invstd && scale_shift, EVK_E_INVALID, "bn_finalize_parts: null pointer");
  int rc = bn_check("bn_finalize_parts", rows, C, nullptr, 0, 0);
  if (rc) return rc;
  launch_parts_final((hipStream_t)stream, parts, nparts, C, (double)rows, gamma, beta, running_mean, running_var, momentum, eps,
                     save_mean, save_invstd, scale_shift, nullptr, 0);
  return check_launch("bn_parts_final");
}
// dx from g (already masked), x and `nparts` partial records: partial [nparts][2][C] = (sum g, sum g * xhat) and, with
// EVK_BN_PACK_DX, maxima [nparts][2][C] = (max|g|, max|xhat|).  workspace: 16 C floats.
extern "C" int evk_bn_bwd_from_partials(const float* g, const float* x, const float* gamma, const float* save_mean,
                                        const float* save_invstd, const float* partial, const float* maxima, int32_t nparts,
                                        float* dx, float* dgamma, float* dbeta, int64_t rows, int32_t C, uint32_t flags,
                                        int32_t train, void* workspace, size_t workspace_bytes, uint32_t* dx_absmax,
                                        void* stream) {
  EVK_REQUIRE(g && x && save_mean && save_invstd && partial && dx && nparts > 0, EVK_E_INVALID, "bn_bwd_from_partials: null pointer");
  int rc = bn_check("bn_bwd_from_partials", rows, C, workspace, workspace_bytes, (size_t)16 * C * sizeof(float));
  if (rc) return rc;
  const bool pack = (flags & EVK_BN_PACK_DX) != 0;
  EVK_REQUIRE(!pack || (dx_absmax && maxima), EVK_E_INVALID,
              "bn_bwd_from_partials: EVK_BN_PACK_DX needs dx_absmax (slots zero on entry) and the maxima");
  hipStream_t st = (hipStream_t)stream;
  float* coef = (float*)workspace;
  launch_bn_bwd_final(st, partial, nparts, C, rows, gamma, save_invstd, dgamma, dbeta, coef, train, dx_absmax,
                      pack ? maxima : nullptr);
  rc = check_launch("bn_bwd_final");
  if (rc) return rc;
  const size_t n4 = (size_t)rows * C / 4;
  EVK_BN_LAUNCH_PK(bn_bwd_apply_kernel, pack, dim3(oneshot_grid(n4)), 0, st, g, x, (const float*)nullptr, save_mean, save_invstd,
                   coef, gamma, (const float*)nullptr, dx, n4, C, 0, dx_absmax, (const uint32_t*)nullptr);
  return check_launch("bn_bwd_apply");
}

// ---- ReLU bits (common.hpp: relu_bits_*)
namespace evk {
__global__ __launch_bounds__(256) void relu_bits_apply_kernel(const float* __restrict__ g, const uint32_t* __restrict__ bits,
                                                              float* __restrict__ out, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) reinterpret_cast<f32x4*>(out)[i] = relu_bits_mask(reinterpret_cast<const f32x4*>(g)[i], bits, i);
}
}  // namespace evk
extern "C" size_t evk_relu_bits_bytes(int64_t n) { return n > 0 ? relu_bits_words(((size_t)n + 3) / 4) * sizeof(uint32_t) : 0; }
// out = g where the bit is set, 0 elsewhere (materialises a lazily masked gradient for a reader that cannot take the bits)
extern "C" int evk_relu_bits_apply(const float* g, const uint32_t* bits, float* out, int64_t n, void* stream) {
  EVK_REQUIRE(g && bits && out && n > 0 && n % 4 == 0, EVK_E_INVALID, "relu_bits_apply: null pointer or n %% 4 != 0");
  const size_t n4 = (size_t)n / 4;
  hipLaunchKernelGGL(relu_bits_apply_kernel, dim3(oneshot_grid(n4)), dim3(256), 0, (hipStream_t)stream, g, bits, out, n4);
  return check_launch("relu_bits_apply");
}

// ------------------------------------------------------------------------------------------------
// Staged entry points for synchronized BatchNorm (torch.nn.SyncBatchNorm under
// `sync_bn=True`, reference ever/trainer/th_ddp_trainer.py): the same kernels as above with the
// cross-rank exchange left to the caller between the stages (one small all-gather forward, one small
// all-reduce backward, on torch.distributed / RCCL).
namespace evk {

// stats[c] = local mean, stats[C + c] = local sum of squared deviations from it (fp64)
__global__ __launch_bounds__(256) void bn_local_final_kernel(const float* __restrict__ x, const float* __restrict__ partial,
                                                             int nblk, int C, double rows, double* __restrict__ stats) {
  int c;
  double s, q;
  if (!reduce_partials(partial, nblk, C, c, s, q)) return;
  const double dm = s / rows;  // mean of (x - pivot)
  stats[c] = (double)x[c] + dm;
  double m2 = q - s * dm;
  stats[C + c] = m2 > 0.0 ? m2 : 0.0;
}
__global__ void bn_coef_from_stats_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                          const float* __restrict__ mean, const float* __restrict__ invstd, int C,
                                          float* __restrict__ scale_shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = (gamma ? gamma[c] : 1.f) * invstd[c];
  scale_shift[c] = sc;
  scale_shift[C + c] = (beta ? beta[c] : 0.f) - mean[c] * sc;
}
__global__ __launch_bounds__(256) void bn_bwd_sums_final_kernel(const float* __restrict__ partial, int nblk, int C,
                                                                double* __restrict__ sums) {
  int c;
  double s, q;
  if (!reduce_partials(partial, nblk, C, c, s, q)) return;
  sums[c] = s;
  sums[C + c] = q;
}
__global__ void bn_bwd_coef_kernel(const float* __restrict__ gamma, const float* __restrict__ invstd,
                                   const float* __restrict__ mean_g, const float* __restrict__ mean_gx, int C,
                                   float* __restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  coef[c] = (gamma ? gamma[c] : 1.f) * invstd[c];
  coef[C + c] = mean_g[c];
  coef[2 * C + c] = mean_gx[c];
}

}  // namespace evk

extern "C" int evk_bn_local_stats(const float* x, double* stats, int64_t rows, int32_t C, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(x && stats, EVK_E_INVALID, "bn_local_stats: null pointer");
  int rc = bn_check("bn_local_stats", rows, C, workspace, workspace_bytes, BnWorkspace::bytes(C));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const BnPlan pl = bn_plan(rows, C);
  float* partial = (float*)workspace;
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(pl.nblk), dim3(256), 0, st, x, partial, rows, C, pl.rows_per_blk,
                     pl.tpc, pl.rl);
  rc = check_launch("bn_stats_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_local_final_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(256), 0, st, x, (const float*)partial,
                     pl.nblk, C, (double)rows, stats);
  return check_launch("bn_local_stats");
}

extern "C" int evk_bn_apply_stats(const float* x, const float* residual, const float* gamma, const float* beta,
                                  const float* mean, const float* invstd, float* y, int64_t rows, int32_t C,
                                  uint32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(x && y && mean && invstd, EVK_E_INVALID, "bn_apply_stats: null pointer");
  int rc = bn_check("bn_apply_stats", rows, C, workspace, workspace_bytes, BnWorkspace::bytes(C));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* scale_shift = (float*)workspace;
  hipLaunchKernelGGL(bn_coef_from_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, st, gamma, beta, mean, invstd, C,
                     scale_shift);
  rc = check_launch("bn_coef_from_stats");
  if (rc) return rc;
  launch_bn_apply(st, false, x, residual, scale_shift, y, rows, C, flags, nullptr);
  return check_launch("bn_apply_stats");
}

extern "C" int evk_bn_bwd_local_sums(const float* dy, const float* x, const float* y, const float* gamma,
                                     const float* beta, const float* mean, const float* invstd, float* d_residual,
                                     double* sums, int64_t rows, int32_t C, uint32_t flags, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(dy && x && mean && invstd && sums, EVK_E_INVALID, "bn_bwd_local_sums: null pointer");
  const int relu = (flags & EVK_BN_RELU) ? (y ? 1 : 2) : 0;
  EVK_REQUIRE(relu != 2 || !d_residual, EVK_E_INVALID, "bn_bwd_local_sums: a residual branch needs y for the ReLU mask");
  int rc = bn_check("bn_bwd_local_sums", rows, C, workspace, workspace_bytes, BnWorkspace::bytes(C));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const BnPlan pl = bn_plan(rows, C);
  float* partial = (float*)workspace;
  hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, dim3(pl.nblk), dim3(256), 0, st, dy, x, y, mean, invstd, gamma, beta,
                     d_residual, partial, rows, C, pl.rows_per_blk, pl.tpc, pl.rl, relu, (float*)nullptr);
  rc = check_launch("bn_bwd_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_bwd_sums_final_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(256), 0, st, (const float*)partial,
                     pl.nblk, C, sums);
  return check_launch("bn_bwd_local_sums");
}

extern "C" int evk_bn_bwd_apply_sums(const float* dy, const float* x, const float* y, const float* gamma,
                                     const float* beta, const float* mean, const float* invstd, const float* mean_g,
                                     const float* mean_gx, float* dx, int64_t rows, int32_t C, uint32_t flags,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(dy && x && mean && invstd && mean_g && mean_gx && dx, EVK_E_INVALID, "bn_bwd_apply_sums: null pointer");
  const int relu = (flags & EVK_BN_RELU) ? (y ? 1 : 2) : 0;
  int rc = bn_check("bn_bwd_apply_sums", rows, C, workspace, workspace_bytes, BnWorkspace::bytes(C));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* coef = (float*)workspace;
  hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, st, gamma, invstd, mean_g, mean_gx, C, coef);
  rc = check_launch("bn_bwd_coef");
  if (rc) return rc;
  const size_t n4 = (size_t)rows * C / 4;
  hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(oneshot_grid(n4)), dim3(256), 0, st, dy, x, y, mean,
                     invstd, (const float*)coef, gamma, beta, dx, n4, C, relu, (uint32_t*)nullptr);
  return check_launch("bn_bwd_apply_sums");
}
