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
// DUAL (the end of a residual block whose shortcut is a convolution, see evk_bn_fwd_train_parts_dual below): `residual` is
// the shortcut convolution's output zb and the added term is bn_b(zb) = zb*scb + shb, computed in registers from
// `scale_shift_b` — an expression of its own, so it is rounded as the stored copy was (one fused multiply-add) before the
// add; always with ReLU and bits.
template <bool PK, bool DUAL>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ residual,
                                                       const float* __restrict__ scale_shift,
                                                       const float* __restrict__ scale_shift_b, float* __restrict__ y,
                                                       size_t n4, int C, int relu, uint32_t* __restrict__ amax,
                                                       uint32_t* __restrict__ relu_bits) {
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
    f32x4 yb = {0.f, 0.f, 0.f, 0.f};
    if constexpr (DUAL) {
      const f32x4 scb = reinterpret_cast<const f32x4*>(scale_shift_b)[cb];
      const f32x4 shb = reinterpret_cast<const f32x4*>(scale_shift_b + C)[cb];
      yb = bn_ld(residual, i) * scb + shb;
    }
    v = bn_ld(x, i) * sc + sh;
    if constexpr (DUAL) v += yb;
    else if (residual) v += bn_ld(residual, i);
  }
  // the backward's mask, one bit per element (common.hpp: relu_bits_*): every lane of the wave takes part (v = 0 where
  // the element does not exist), i >> 6 is this wave's chunk; a wave wholly past the end has no chunk in the buffer
  if ((DUAL || relu_bits) && ((i >> 6) << 6) < n4)
    relu_bits_store(relu_bits, i >> 6, v.x > 0.f, v.y > 0.f, v.z > 0.f, v.w > 0.f);
  if (valid) {
    if (DUAL || relu) {
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
// NM = 2 (the two BatchNorms at the end of a residual block whose shortcut is a convolution, evk_bn_bwd_dual): g is read and
// masked ONCE — mask mode 3, no d_residual — and summed against both maps, xhat of `x` into `partial`, xhat of `xb` (under
// mean_b / invstd_b) into `partial_b`: one plan, row order and fold, so each record has the bits the NM = 1 pass gives.
// PK (dx will be written packed, EVK_BN_PACK_DX): also pmax[blk][0][C] = max |g|, [1][C] = max |xhat| (and pmax_b) — what
// the finalisation needs to bound |dx| per channel BEFORE the apply pass writes it under that scale.
// (plain loads: the apply pass re-reads what this pass streams.  The non-temporal hint here, gated by map size, measured
// level from 128 MB up and -0.3 % below — removed)
__device__ __forceinline__ f32x4 bp_ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <int NM, bool PK>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ xb, const float* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ mean_b,
    const float* __restrict__ invstd_b, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ d_residual, float* __restrict__ partial, float* __restrict__ partial_b, int64_t rows, int C,
    int64_t rows_per_blk, int tpc, int rl, int relu, float* __restrict__ pmax, float* __restrict__ pmax_b,
    const uint32_t* __restrict__ bits) {
  // relu: 0 none, 1 mask from the saved output y, 2 mask recomputed from x (no residual: the
  // forward's pre-activation is x*sc+sh with the same sc/sh arithmetic as bn_stats_final_kernel), 3 mask from `bits`
  // (common.hpp: relu_bits_*: the forward's own bits, or the mask of a gradient that arrives unmasked — EVK_BN_LAZY_RES)
  if constexpr (NM == 2) {
    relu = 3;
    d_residual = nullptr;
  }
  __shared__ f32x4 red[2][256];
  const float* const xs[2] = {x, xb};
  const float* const means[2] = {mean, mean_b};
  const float* const invstds[2] = {invstd, invstd_b};
  float* const partials[2] = {partial, partial_b};
  float* const pmaxs[2] = {pmax, pmax_b};
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int c4 = C >> 2;
  const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
  const int64_t r0 = (int64_t)bn_blk() * rows_per_blk;
  const int64_t r1 = min(rows, r0 + rows_per_blk);
  for (int cb = tc; cb < c4; cb += tpc) {
    f32x4 mu[NM], is[NM], q[NM], xm[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      mu[m] = *reinterpret_cast<const f32x4*>(means[m] + cb * 4);
      is[m] = *reinterpret_cast<const f32x4*>(invstds[m] + cb * 4);
      q[m] = xm[m] = zero4;
    }
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = zero4;
    if (relu == 2) {
      const f32x4 one = {1.f, 1.f, 1.f, 1.f};
      const f32x4 g4 = gamma ? *reinterpret_cast<const f32x4*>(gamma + cb * 4) : one;
      const f32x4 b4 = beta ? *reinterpret_cast<const f32x4*>(beta + cb * 4) : zero4;
      sc = g4 * is[0];
      sh = b4 - mu[0] * sc;
    }
    f32x4 s = zero4, gm = zero4;
    if (tr < rl) {
      auto one = [&](const f32x4 gin, const f32x4* xv, const f32x4 yin, size_t off) {
        f32x4 g = gin;
        if (relu == 3) {
          g = relu_bits_mask(g, bits, off >> 2);
        } else if (relu) {
          const f32x4 yy = (relu == 1) ? yin : xv[0] * sc + sh;
          g = relu_mask(g, yy);
        }
        if (d_residual) *reinterpret_cast<f32x4*>(d_residual + off) = g;
        s += g;
        f32x4 xh[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          xh[m] = (xv[m] - mu[m]) * is[m];
          q[m] += g * xh[m];
        }
        if constexpr (PK) {
          absmax4(gm, g);
#pragma unroll
          for (int m = 0; m < NM; ++m) absmax4(xm[m], xh[m]);
        }
      };
      int64_t r = r0 + tr;
      const int64_t st = rl;
      // four rows per trip: 8-12 independent 16-byte loads in flight per lane
      for (; r + 3 * st < r1; r += 4 * st) {
        size_t o[4];
        f32x4 g[4], xv[4][NM], yv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (size_t)(r + k * st) * C + cb * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = bp_ld(dy + o[k]);
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
          for (int k = 0; k < 4; ++k) xv[k][m] = bp_ld(xs[m] + o[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) yv[k] = zero4;
        if (relu == 1) {
#pragma unroll
          for (int k = 0; k < 4; ++k) yv[k] = bp_ld(y + o[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) one(g[k], xv[k], yv[k], o[k]);
      }
      for (; r < r1; r += st) {
        const size_t o0 = (size_t)r * C + cb * 4;
        f32x4 xv[NM];
        const f32x4 g0 = bp_ld(dy + o0);
#pragma unroll
        for (int m = 0; m < NM; ++m) xv[m] = bp_ld(xs[m] + o0);
        one(g0, xv, (relu == 1) ? bp_ld(y + o0) : zero4, o0);
      }
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) fold_store_record(red, s, q[m], partials[m], bn_blk(), C, cb, tc, tr, tpc, rl);
    if constexpr (PK) {
#pragma unroll
      for (int m = 0; m < NM; ++m) fold_store_maxima(red, gm, xm[m], pmaxs[m], bn_blk(), C, cb, tc, tr, tpc, rl);
    }
  }
}

// coef[0][C] = gamma*invstd ; coef[1][C] = mean(g) ; coef[2][C] = mean(g*xhat)  (0 when !train)
// FC channels x 256 / FC lanes per workgroup: 8 x 32 by default; 2 x 128 (four times the workgroups) when the partials are many
// (the body: bn_bwd_final_kernel below hands it the arguments of the BatchNorm its row of workgroups finishes)
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
// One BatchNorm's arguments; the kernel takes NR sets, one per row of workgroups (gridDim.y = NR: 1, or 2 for the pair at the
// end of a residual block whose shortcut is a convolution): blockIdx.y selects the set, the workgroups of a row look at
// blockIdx.x alone (bn_fin_group, zero_amax).  (NR is a template argument because with two sets in every launch the one-row
// launches paid for the second: 0.1-0.4 us on launches of 6-17 us, above the parent's range in every run.)
struct BnBwdFinalSet {
  const float *partial, *gamma, *invstd;
  float *dgamma, *dbeta, *coef;
  int train;
  uint32_t* amax;
  const float* pmax;
};
template <typename Set, int NR>
struct BnFinalSets {
  Set row[NR];
};
// the set of this workgroup's row (both sets loaded, then selected — the two-row kernels' form since they exist; loading the
// one at index blockIdx.y measured the same)
template <typename Set, int NR>
__device__ __forceinline__ Set bn_final_row(const BnFinalSets<Set, NR>& sets) {
  if constexpr (NR == 1) return sets.row[0];
  else return blockIdx.y ? sets.row[1] : sets.row[0];
}
template <int NR>
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(BnFinalSets<BnBwdFinalSet, NR> sets, int nblk, int C, double inv_rows) {
  const BnBwdFinalSet s = bn_final_row(sets);
  bn_bwd_final_body<kFinCh>(s.partial, nblk, C, inv_rows, s.gamma, s.invstd, s.dgamma, s.dbeta, s.coef, s.train, s.amax, s.pmax);
}

// dx = coef0 * (g - coef1 - xhat*coef2); one 16-byte element per thread (see bn_apply_kernel), the per-channel
// vectors read through L1.  PK: dx is written as packed words of dx / s (x3_common.hpp: pack_hl), s from the bound the
// finalisation left in `amax` — the tensor is the producing convolution's dy operand and nothing else.
// One map's share of an element, in two steps so that a kernel can issue the loads of the channel chunk's coefficients ahead
// of its streaming loads (in one step the apply kernels came out 2.2-2.5 % slower): bn_dx_coef loads them, bn_dx_store forms
// dx, stores it packed or plain and returns it for block_absmax.
struct BnDxCoef {
  f32x4 k0, k1, k2, mu, is;
};
__device__ __forceinline__ BnDxCoef bn_dx_coef(const float* __restrict__ coef, const float* __restrict__ mean,
                                               const float* __restrict__ invstd, int C, int c) {
  return {reinterpret_cast<const f32x4*>(coef)[c], reinterpret_cast<const f32x4*>(coef + C)[c],
          reinterpret_cast<const f32x4*>(coef + 2 * C)[c], reinterpret_cast<const f32x4*>(mean)[c],
          reinterpret_cast<const f32x4*>(invstd)[c]};
}
template <bool PK>
__device__ __forceinline__ f32x4 bn_dx_store(const BnDxCoef& k, const f32x4 g, const f32x4 xv, float* __restrict__ dx, size_t i,
                                             float pk_inv) {
  const f32x4 xh = (xv - k.mu) * k.is;
  const f32x4 out = k.k0 * (g - k.k1 - xh * k.k2);
  if constexpr (PK) {
    reinterpret_cast<u32x4*>(dx)[i] = pack_hl4(out, pk_inv);
  } else {
    reinterpret_cast<f32x4*>(dx)[i] = out;
  }
  return out;
}
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
    const BnDxCoef k = bn_dx_coef(coef, mean, invstd, C, c);
    f32x4 g = bn_ld(dy, i);
    const f32x4 xv = bn_ld(x, i);
    if (relu == 3) {
      g = relu_bits_mask(g, bits, i);
    } else if (relu) {
      f32x4 yy;
      if (relu == 1) {
        yy = reinterpret_cast<const f32x4*>(y)[i];
      } else {  // the forward's pre-activation, same sc/sh arithmetic as bn_stats_final_kernel
        const f32x4 sc = (gamma ? reinterpret_cast<const f32x4*>(gamma)[c] : one4) * k.is;
        const f32x4 sh = (beta ? reinterpret_cast<const f32x4*>(beta)[c] : z4) - k.mu * sc;
        yy = xv * sc + sh;
      }
      g = relu_mask(g, yy);
    }
    out = bn_dx_store<PK>(k, g, xv, dx, i, pk_inv);
  }
  if constexpr (!PK)
    if (amax) block_absmax(out, valid, amax);   // all lanes of the workgroup arrive here together
}

// Statistics that arrive as per-row-part records (count, mean, M2) from the producing convolution's epilogue
// (igemm_common.hpp: igemm_store_rows_stats): Chan's pairwise merge in fp64, 32 lanes per channel over a fixed strided
// subset each, then the 32 lanes folded in index order — the same outputs as bn_stats_final_kernel, no pass over x.
// FC channels x FL record lanes per workgroup (FC * FL = 256): 8 x 32 for the small maps; 2 x 128 where a channel has
// hundreds of records (the 128^2 maps: 2048 per channel — at 32 lanes each lane walked 64 strided records: 9-47 us a launch)
// (the body: bn_parts_final_kernel below hands it the arguments of the BatchNorm whose records its row of workgroups merges)
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
// One BatchNorm's arguments, NR sets, one per row of workgroups as for bn_bwd_final_kernel (two rows: the two merges of a
// block end with a shortcut convolution in ONE launch, when both take the same form FC x FL).
struct BnPartsFinalSet {
  const float* parts;
  int nparts;
  const float *gamma, *beta;
  float *running_mean, *running_var;
  float momentum, eps;
  float *save_mean, *save_invstd, *scale_shift;
  uint32_t* amax;
  int pack;
};
template <int FC, int FL, int NR>
__global__ __launch_bounds__(256) void bn_parts_final_kernel(BnFinalSets<BnPartsFinalSet, NR> sets, int C, double rows) {
  const BnPartsFinalSet s = bn_final_row(sets);
  // (a pair never packs — the output of a block end has several readers — so its kernels carry no code or LDS for the bound)
  bn_parts_final_body<FC, FL>(s.parts, s.nparts, C, rows, s.gamma, s.beta, s.running_mean, s.running_var, s.momentum, s.eps,
                              s.save_mean, s.save_invstd, s.scale_shift, s.amax, NR == 1 ? s.pack : 0);
}

// (A one-launch backward for small maps — every thread's rows in registers across two grid-wide barriers, 3 tensor transfers
// instead of 5 — lived here in rounds 2 and 3.  Its grid had to be resident as a whole, so it was off beside the weight-
// gradient side stream, under RCCL and on any stream but one; at the end it ran on ~1 call in 30 of the default path.
// Removed in round 4: EVK_BN_FUSED=1 vs 0 measured 547.7 / 547.4 tiles/s on the default path, 524.4 / 519.4 single-stream,
// 521.6 / 521.2 captured, same box — and with it went the spin barrier, its device words and the stream ownership.)

// record lanes per channel of the merge: bn_parts_final_kernel<256 / lanes, lanes>
static int parts_final_lanes(int nparts) { return nparts >= 1024 ? 256 : (nparts >= 512 ? 128 : 32); }

// the merge of one BatchNorm's records (b null), or of two that take the same form: a row of workgroups each
static void launch_parts_final_sets(hipStream_t st, const BnPartsFinalSet& a, const BnPartsFinalSet* b, int C, double rows) {
  // one channel per workgroup above 1024 records — eight records per lane, all in flight at once (level with the two-channel
  // form on the step, ahead in the family: 407 vs 460 us per step)
  pick<256, 128, 32>(parts_final_lanes(a.nparts), [&](auto FL) {
    constexpr int fl = decltype(FL)::value, fc = 256 / fl;
    const dim3 grid((C + fc - 1) / fc, b ? 2 : 1);
    if (b) hipLaunchKernelGGL((bn_parts_final_kernel<fc, fl, 2>), grid, dim3(256), 0, st, BnFinalSets<BnPartsFinalSet, 2>{{a, *b}}, C, rows);
    else hipLaunchKernelGGL((bn_parts_final_kernel<fc, fl, 1>), grid, dim3(256), 0, st, BnFinalSets<BnPartsFinalSet, 1>{{a}}, C, rows);
    return 0;
  });
}
void launch_parts_final(hipStream_t st, const float* parts, int nparts, int C, double rows, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                        float* save_mean, float* save_invstd, float* scale_shift, uint32_t* amax, int pack) {
  const BnPartsFinalSet s = {parts, nparts, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd,
                             scale_shift, amax, pack};
  launch_parts_final_sets(st, s, nullptr, C, rows);
}

// the backward finalisation of one BatchNorm (b null) or two
static void launch_bn_bwd_final_sets(hipStream_t st, const BnBwdFinalSet& a, const BnBwdFinalSet* b, int nblk, int C,
                                     int64_t rows) {
  // (two channels x 128 lanes per workgroup, four times the workgroups, measured -0.2 % chosen from 128 partials up and -2.5 %
  // everywhere: the 8-byte pieces of a partial row it reads cost more than the shorter chains save — removed)
  const dim3 grid((C + kFinCh - 1) / kFinCh, b ? 2 : 1);
  const double inv_rows = 1.0 / (double)rows;
  if (b) hipLaunchKernelGGL(bn_bwd_final_kernel<2>, grid, dim3(256), 0, st, BnFinalSets<BnBwdFinalSet, 2>{{a, *b}}, nblk, C, inv_rows);
  else hipLaunchKernelGGL(bn_bwd_final_kernel<1>, grid, dim3(256), 0, st, BnFinalSets<BnBwdFinalSet, 1>{{a}}, nblk, C, inv_rows);
}
void launch_bn_bwd_final(hipStream_t st, const float* partial, int nblk, int C, int64_t rows, const float* gamma,
                         const float* invstd, float* dgamma, float* dbeta, float* coef, int train, uint32_t* amax,
                         const float* pmax) {
  const BnBwdFinalSet s = {partial, gamma, invstd, dgamma, dbeta, coef, train ? 1 : 0, amax, pmax};
  launch_bn_bwd_final_sets(st, s, nullptr, nblk, C, rows);
}

// the forward apply pass over a [rows][C] map (pack: y as packed words, EVK_BN_PACK_Y); scale_shift_b given: the two-map form,
// `residual` the shortcut convolution's output (always ReLU and bits, never packed)
static void launch_bn_apply(hipStream_t st, bool pack, const float* x, const float* residual, const float* scale_shift,
                            float* y, int64_t rows, int C, uint32_t flags, uint32_t* amax, uint32_t* relu_bits = nullptr,
                            const float* scale_shift_b = nullptr) {
  const size_t n4 = (size_t)rows * C / 4;
  const int relu = (flags & EVK_BN_RELU) ? 1 : 0;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(oneshot_grid(n4)), dim3(256), 0, st, x, residual, scale_shift, scale_shift_b, y, n4, C, relu,
                       amax, relu_bits);
  };
  if (scale_shift_b) launch(bn_apply_kernel<false, true>);
  else if (pack) launch(bn_apply_kernel<true, false>);
  else launch(bn_apply_kernel<false, false>);
}

// the backward reduce pass over a [rows][C] map (pmax given: the maxima as well); xb given: over both maps of a block end,
// the second one's statistics and records in the *_b arguments (mask from `bits`, no d_residual)
static void launch_bn_bwd_partial(hipStream_t st, const BnPlan& pl, const float* dy, const float* x, const float* y,
                                  const float* mean, const float* invstd, const float* gamma, const float* beta,
                                  float* d_residual, float* partial, int64_t rows, int C, int relu, float* pmax,
                                  const uint32_t* bits, const float* xb = nullptr, const float* mean_b = nullptr,
                                  const float* invstd_b = nullptr, float* partial_b = nullptr, float* pmax_b = nullptr) {
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(pl.nblk), dim3(256), 0, st, dy, x, xb, y, mean, invstd, mean_b, invstd_b, gamma, beta,
                       d_residual, partial, partial_b, rows, C, pl.rows_per_blk, pl.tpc, pl.rl, relu, pmax, pmax_b, bits);
  };
  if (xb) pmax ? launch(bn_bwd_partial_kernel<2, true>) : launch(bn_bwd_partial_kernel<2, false>);
  else pmax ? launch(bn_bwd_partial_kernel<1, true>) : launch(bn_bwd_partial_kernel<1, false>);
}

// ---- The end of a residual block whose shortcut is a convolution (`layerN.0`): out = relu(bn_a(za) + bn_b(zb)), za the
// main branch's last convolution output, zb the shortcut convolution's.  The passes below take BOTH maps, so the shortcut's
// normalised copy yb = bn_b(zb) is never stored: forward 3 transfers of the map instead of 5, backward reduce 3 instead of 4,
// backward apply 5 instead of 6.  Each pass is a form of the single-map pass above, not a copy of it: the forward apply is
// bn_apply_kernel<false, true> (the added term computed from zb in registers), the backward reduce bn_bwd_partial_kernel<2, PK>,
// both finalisations their kernels with a second row of workgroups; the backward apply below is a kernel of its own (two
// outputs, each packed or not) built from bn_bwd_apply_kernel's per-map step, bn_dx_store.

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
    const BnDxCoef ka = bn_dx_coef(coef_a, mean_a, invstd_a, C, c);
    outa = bn_dx_store<PKA>(ka, g, bn_ld(xa, i), dxa, i, pk_inv_a);
    const BnDxCoef kb = bn_dx_coef(coef_b, mean_b, invstd_b, C, c);
    outb = bn_dx_store<PKB>(kb, g, bn_ld(xb, i), dxb, i, pk_inv_b);
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
  launch_bn_bwd_partial(st, pl, dy, x, y, save_mean, save_invstd, gamma, beta, d_residual, ws.partial, rows, C, relu, pmax,
                        relu_bits);
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

// ---- Both BatchNorms at the end of a residual block with a shortcut convolution (the two-map forms of the passes above).
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
  const BnPartsFinalSet sa = {parts_a, nparts_a, gamma_a, beta_a, running_mean_a, running_var_a, momentum_a, eps_a,
                              save_mean_a, save_invstd_a, ss_a, y_absmax, 0};
  const BnPartsFinalSet sb = {parts_b, nparts_b, gamma_b, beta_b, running_mean_b, running_var_b, momentum_b, eps_b,
                              save_mean_b, save_invstd_b, ss_b, nullptr, 0};
  if (parts_final_lanes(nparts_a) == parts_final_lanes(nparts_b)) {   // the same form of the merge for both: one launch
    launch_parts_final_sets(st, sa, &sb, C, (double)rows);
    rc = check_launch("bn_parts_final_dual");
    if (rc) return rc;
  } else {
    launch_parts_final_sets(st, sb, nullptr, C, (double)rows);
    rc = check_launch("bn_parts_final");
    if (rc) return rc;
    launch_parts_final_sets(st, sa, nullptr, C, (double)rows);
    rc = check_launch("bn_parts_final");
    if (rc) return rc;
  }
  launch_bn_apply(st, false, za, zb, ss_a, y, rows, C, EVK_BN_RELU, y_absmax, relu_bits, ss_b);
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
  launch_bn_bwd_partial(st, pl, dy, za, nullptr, save_mean_a, save_invstd_a, nullptr, nullptr, nullptr, wa.partial, rows, C, 3,
                        pack ? wa.pmax : nullptr, relu_bits, zb, save_mean_b, save_invstd_b, wb.partial, pack ? wb.pmax : nullptr);
  rc = check_launch("bn_bwd_partial_dual");
  if (rc) return rc;
  const BnBwdFinalSet fa = {wa.partial, gamma_a, save_invstd_a, dgamma_a, dbeta_a, wa.coef, 1, dza_absmax, pack_a ? wa.pmax : nullptr};
  const BnBwdFinalSet fb = {wb.partial, gamma_b, save_invstd_b, dgamma_b, dbeta_b, wb.coef, 1, dzb_absmax, pack_b ? wb.pmax : nullptr};
  launch_bn_bwd_final_sets(st, fa, &fb, pl.nblk, C, rows);
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

// ---- BatchNorm around a fused consumer (FS-Relation, relation.hip: relation_*<BN>): the statistics records of the
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
  launch_bn_bwd_partial(st, pl, dy, x, y, mean, invstd, gamma, beta, d_residual, partial, rows, C, relu, nullptr, nullptr);
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
