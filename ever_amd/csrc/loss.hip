// The scalar losses on NHWC logits (gfx950), forward statistics and gradients:
//   * BCE, dice, CE and soft CE with ignore_index on int64 labels.  Replaces the masked_select compaction + reductions
//     of reference ever/module/loss.py:10-17 (_masked_ignore), :26-37 (select), :40-75 (dice), :207-219 (LS-CE),
//     :229-235 (BCE) and F.cross_entropy(ignore_index=...) in user model code;
//   * class-probability statistics (tp, sum p, sum y per class) and their adjoint: the sufficient statistics of
//     tversky_loss_with_logits (loss.py:78-143) and of any dice-like ratio loss;
//   * focal losses on float targets (loss.py:158-201).
// HBM-bound masked reductions: fp64 accumulation, per-workgroup partials, then a finalisation in a fixed order
// (reproducible).  stats layout: [K finals][nblk x K partials].  The shared pieces are in loss_common.hpp; the
// per-pixel losses are in loss_pixel.hip, the confusion matrix in metric.hip.
#include "loss_common.hpp"

namespace evk {

constexpr int kMaxClasses = 64;
constexpr int kDiceLdsBytes = 64 * 1024;
constexpr int kDiceMaxClasses = kDiceLdsBytes / (256 * 2 * (int)sizeof(double));  // 16: [256][2C] doubles of the softmax path

// the two folds of loss_common.hpp as kernels: tree = one workgroup of 256 per k, in order = one thread per k
__global__ __launch_bounds__(256) void finalize_partials_kernel(double* stats, int K, int nblk) {
  fold_partials_tree(stats, K, nblk);
}
__global__ void finalize_partials_in_order_kernel(double* stats, int K, int nblk) {
  fold_partials_in_order(stats, K, nblk);
}
// the loss word of a sum (scale 1: exact) or of a mean over a count the host knows
__global__ void loss_scale_store_kernel(const double* stats, double scale, float* loss) {
  if (threadIdx.x == 0) *loss = (float)(stats[0] * scale);  // reduction='sum': 0 for an empty selection, as aten
}
// ... and over the counted valid pixels: a quotient, which a product with the reciprocal would round differently
__global__ void mean_loss_kernel(const double* stats, float* loss) {
  if (threadIdx.x == 0) *loss = (float)(stats[0] / stats[1]);  // 0/0 -> NaN, as mean of an empty tensor
}

// ---------------------------------------------------------------- BCE with logits -----------------
__device__ __forceinline__ float bce_term(float x, float y, float pw) {
  // aten binary_cross_entropy_with_logits: (1-y)*x + (1 + (pos_weight-1)*y) * (log1p(exp(-|x|)) + max(-x,0))
  return (1.f - y) * x + (1.f + (pw - 1.f) * y) * (softplus_neg_abs(x) + fmaxf(-x, 0.f));
}
__global__ __launch_bounds__(256) void bce_partial_kernel(const float* __restrict__ logits,
                                                          const int64_t* __restrict__ labels, int64_t npix,
                                                          int64_t ignore, float eps, float pw,
                                                          double* __restrict__ stats) {
  double v[2] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t t = labels[i];
    if (t != ignore) {
      const float y = (t == 0) ? eps : (float)t - eps;  // label smoothing (eps = 0: plain BCE)
      v[0] += (double)bce_term(logits[i], y, pw);
      v[1] += 1.0;
    }
  }
  block_sum_store<2>(v, stats + 2 + (size_t)blockIdx.x * 2);
}
__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ logits,
                                                      const int64_t* __restrict__ labels, int64_t npix, int64_t ignore,
                                                      float eps, float pw, int sum_reduction,
                                                      const double* __restrict__ stats,
                                                      const float* __restrict__ grad_scale, float* __restrict__ dlogits,
                                                      int accumulate) {
  const float k = upstream_scale(grad_scale) / (sum_reduction ? 1.f : (float)stats[1]);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t t = labels[i];
    float g = 0.f;
    if (t != ignore) {
      const float p = sigmoidf_(logits[i]);
      const float y = (t == 0) ? eps : (float)t - eps;
      g = ((1.f - y) - (1.f + (pw - 1.f) * y) * (1.f - p)) * k;   // pw = 1: p - y
    }
    store_grad(dlogits, i, g, accumulate);
  }
}

// ---------------------------------------------------------------- dice -----------------------------
// stats finals: inter[c] (k = c), z[c] (k = C + c)
template <int CT>  // CT == 1: sigmoid path;  CT == 0: softmax path with runtime C
__global__ __launch_bounds__(256) void dice_partial_kernel(const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels, int64_t npix, int C,
                                                           int64_t ignore, double* __restrict__ stats) {
  extern __shared__ double dacc[];  // [256][2C] only for the softmax path
  if (CT == 1) {
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
      const int64_t t = labels[i];
      if (t != ignore) {
        const float p = sigmoidf_(logits[i]);
        const float y = (float)t;
        v[0] += (double)(p * y);
        v[1] += (double)p + (double)y;
      }
    }
    block_sum_store<2>(v, stats + 2 + (size_t)blockIdx.x * 2);
  } else {
    const int K = 2 * C;
    double* mine = dacc + (size_t)threadIdx.x * K;
    for (int k = 0; k < K; ++k) mine[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
      const int64_t t = labels[i];
      if (t == ignore) continue;
      const float* x = logits + i * C;
      const PixelSoftmax sm = pixel_softmax(x, C);
      for (int c = 0; c < C; ++c) {
        const float p = sm.p(x[c]);
        const float y = (t == c) ? 1.f : 0.f;
        mine[c] += (double)(p * y);
        mine[C + c] += (double)p + (double)y;
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
      double s = 0.0;
      for (int t = 0; t < 256; ++t) s += dacc[(size_t)t * K + k];
      stats[K + (size_t)blockIdx.x * K + k] = s;
    }
  }
}
__global__ void dice_finish_kernel(const double* stats, int C, float smooth, int ignore_channel, float* loss) {
  if (threadIdx.x != 0) return;
  double acc = 0.0;
  int nc = 0;
  for (int c = 0; c < C; ++c) {
    if (C > 1 && c == ignore_channel) continue;
    acc += (2.0 * stats[c] + (double)smooth) / (stats[C + c] + (double)smooth);
    ++nc;
  }
  *loss = (float)(1.0 - acc / (double)nc);
}
// d loss / d p_c = a_c * y_c + b_c,  a_c = -2/(nc (z_c+s)),  b_c = (2 I_c + s)/(nc (z_c+s)^2)
template <int CT>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ labels, int64_t npix, int C,
                                                       int64_t ignore, const double* __restrict__ stats, float smooth,
                                                       int ignore_channel, const float* __restrict__ grad_scale,
                                                       float* __restrict__ dlogits, int accumulate) {
  __shared__ float sa[kMaxClasses], sb[kMaxClasses];
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    int nc = 0;
    for (int k = 0; k < C; ++k) nc += (C > 1 && k == ignore_channel) ? 0 : 1;
    const double zs = stats[C + c] + (double)smooth;
    const double gs = (double)upstream_scale(grad_scale);
    const bool off = (C > 1 && c == ignore_channel);
    sa[c] = off ? 0.f : (float)(-2.0 / ((double)nc * zs) * gs);
    sb[c] = off ? 0.f : (float)((2.0 * stats[c] + (double)smooth) / ((double)nc * zs * zs) * gs);
  }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t t = labels[i];
    if (CT == 1) {
      float g = 0.f;
      if (t != ignore) {
        const float p = sigmoidf_(logits[i]);
        g = (sa[0] * (float)t + sb[0]) * p * (1.f - p);
      }
      store_grad(dlogits, i, g, accumulate);
    } else {
      const float* x = logits + i * C;
      float* d = dlogits + i * C;
      if (t == ignore) {
        zero_grad(d, C, accumulate);
        continue;
      }
      const PixelSoftmax sm = pixel_softmax(x, C);
      float dotgp = 0.f;
      for (int c = 0; c < C; ++c) {
        const float p = sm.p(x[c]);
        const float g = sa[c] * ((t == c) ? 1.f : 0.f) + sb[c];
        dotgp += g * p;
      }
      for (int c = 0; c < C; ++c) {
        const float p = sm.p(x[c]);
        const float g = sa[c] * ((t == c) ? 1.f : 0.f) + sb[c];
        store_grad(d, c, p * (g - dotgp), accumulate);
      }
    }
  }
}

// ---------------------------------------------------------------- cross entropy -------------------
// stats finals: [0] sum nll, [1] count, [2] sum_p (-sum_c logp_c)
__global__ __launch_bounds__(256) void ce_partial_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ labels, int64_t npix, int C,
                                                         int64_t ignore, double* __restrict__ stats) {
  double v[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t t = labels[i];
    if (t == ignore) continue;
    const float* x = logits + i * C;
    float sx = 0.f;
    const PixelSoftmax sm = pixel_softmax(x, C, [&](int, float xm) { sx += xm; });
    const float nll = (t >= 0 && t < C) ? sm.ls - (x[t] - sm.m) : sm.m + sm.ls;
    v[0] += (double)nll;
    v[1] += 1.0;
    v[2] += (double)((float)C * sm.ls - sx);
  }
  block_sum_store<3>(v, stats + 3 + (size_t)blockIdx.x * 3);
}
__global__ void ce_finish_kernel(const double* stats, int C, float eps, float* loss) {
  if (threadIdx.x != 0) return;
  const double nll = stats[0] / stats[1];
  const double sm = stats[2] / stats[1];
  *loss = (float)((1.0 - (double)eps) * nll + (eps != 0.f ? (double)eps / (double)C * sm : 0.0));
}
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits,
                                                     const int64_t* __restrict__ labels, int64_t npix, int C,
                                                     int64_t ignore, float eps, const double* __restrict__ stats,
                                                     const float* __restrict__ grad_scale, float* __restrict__ dlogits,
                                                     int accumulate) {
  const float k = upstream_scale(grad_scale) / (float)stats[1];
  const float k1 = (1.f - eps) * k, k2 = eps / (float)C * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t t = labels[i];
    const float* x = logits + i * C;
    float* d = dlogits + i * C;
    if (t == ignore) {
      zero_grad(d, C, accumulate);
      continue;
    }
    const PixelSoftmax sm = pixel_softmax(x, C);
    for (int c = 0; c < C; ++c) {
      const float p = sm.p(x[c]);
      store_grad(d, c, k1 * (p - ((t == c) ? 1.f : 0.f)) + k2 * ((float)C * p - 1.f), accumulate);
    }
  }
}

// ---------------------------------------------------------------- soft cross entropy --------------
// reference loss.py:238-242: -(target * log_softmax(input, 1)).mean(dim=(0,2,3)).sum()
//   = -sum_{pixels, c} t_c * logp_c / npix.   stats final: [0] = sum_{p,c} t_c * (lse - x_c)
__global__ __launch_bounds__(256) void soft_ce_partial_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ target, int64_t npix, int C,
                                                              double* __restrict__ stats) {
  double v[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const float* x = logits + i * C;
    const float* t = target + i * C;
    const PixelSoftmax sm = pixel_softmax(x, C);
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc += t[c] * (sm.ls - (x[c] - sm.m));
    v[0] += (double)acc;
  }
  block_sum_store<1>(v, stats + 1 + (size_t)blockIdx.x);
}
__global__ __launch_bounds__(256) void soft_ce_bwd_kernel(const float* __restrict__ logits,
                                                          const float* __restrict__ target, int64_t npix, int C,
                                                          float inv_npix, const float* __restrict__ grad_scale,
                                                          float* __restrict__ dlogits) {
  const float k = upstream_scale(grad_scale) * inv_npix;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const float* x = logits + i * C;
    const float* t = target + i * C;
    float* d = dlogits + i * C;
    float ts = 0.f;
    const PixelSoftmax sm = pixel_softmax(x, C, [&](int c, float) { ts += t[c]; });
    for (int c = 0; c < C; ++c) d[c] = k * (sm.p(x[c]) * ts - t[c]);
  }
}

// ---------------------------------------------------------------- class-probability statistics ----
constexpr int kProbStatsMaxC = 64;
// stats layout: [3C finals: tp[C], sp[C], sy[C]] [nblk x 3C partials]
__global__ __launch_bounds__(256) void prob_stats_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ labels, int64_t npix, int C,
                                                         int64_t ignore, double* __restrict__ stats) {
  double tp[kProbStatsMaxC], sp[kProbStatsMaxC], sy[kProbStatsMaxC];
  for (int c = 0; c < C; ++c) tp[c] = sp[c] = sy[c] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t t = labels[i];
    if (t == ignore) continue;
    const float* z = logits + i * C;
    if (C == 1) {
      const float p = logsigmoid_prob(z[0]);
      const double y = (double)t;
      tp[0] += (double)p * y;
      sp[0] += (double)p;
      sy[0] += y;
    } else {
      const PixelSoftmax sm = pixel_softmax(z, C);
      for (int c = 0; c < C; ++c) {
        const float p = sm.p(z[c]);
        sp[c] += (double)p;
        if (t == c) {
          tp[c] += (double)p;
          sy[c] += 1.0;
        }
      }
    }
  }
  double* out = stats + 3 * C + (size_t)blockIdx.x * 3 * C;
  for (int c = 0; c < C; ++c) {
    const double a = block_sum(tp[c]), b = block_sum(sp[c]), d = block_sum(sy[c]);
    if (threadIdx.x == 0) {
      out[c] = a;
      out[C + c] = b;
      out[2 * C + c] = d;
    }
  }
}
// dlogits for L(tp, sp): per pixel G_c = gtp[c]*y_c + gsp[c];  sigmoid: dz = G p (1-p);
// softmax: dz_j = p_j (G_j - sum_k G_k p_k).  (sy does not depend on the logits.)
__global__ __launch_bounds__(256) void prob_stats_bwd_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ labels, int64_t npix, int C,
                                                             int64_t ignore, const float* __restrict__ gtp,
                                                             const float* __restrict__ gsp, float* __restrict__ dlogits,
                                                             int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t t = labels[i];
    const float* z = logits + i * C;
    float* d = dlogits + i * C;
    if (t == ignore) {
      zero_grad(d, C, accumulate);
      continue;
    }
    if (C == 1) {
      const float p = logsigmoid_prob(z[0]);
      store_grad(d, 0, (gtp[0] * (float)t + gsp[0]) * p * (1.f - p), accumulate);
    } else {
      const PixelSoftmax sm = pixel_softmax(z, C);
      float dot = 0.f;
      for (int c = 0; c < C; ++c) dot += (gsp[c] + (t == c ? gtp[c] : 0.f)) * sm.p(z[c]);
      for (int c = 0; c < C; ++c)
        store_grad(d, c, sm.p(z[c]) * ((gsp[c] + (t == c ? gtp[c] : 0.f)) - dot), accumulate);
    }
  }
}

// ---------------------------------------------------------------- focal losses on float targets ---
// mode 0: focal_loss(normalize=False): mean_i w_i * bce_i, w = pt^gamma detached (loss.py:158-176)
// mode 1: sigmoid_focal_loss: sum_i alpha_t * bce_i * (1-p_t)^gamma, gradient through the factor (:179-201)
// mode 2: focal_loss(normalize=True): value sum_i bce_i (the normalisation cancels identically)
__device__ __forceinline__ void focal_term(float x, float y, float gamma, float alpha, int mode, float& val,
                                           float& grad) {
  const float bce = (1.f - y) * x + (softplus_neg_abs(x) + fmaxf(-x, 0.f));
  const float p = sigmoidf_(x);
  const float dbce = p - y;
  if (mode == 2) {
    val = bce;
    grad = dbce;
  } else if (mode == 0) {
    const float pt = (1.f - p) * y + p * (1.f - y);
    const float w = powf(pt, gamma);
    val = w * bce;
    grad = w * dbce;
  } else {
    const float p_t = p * y + (1.f - p) * (1.f - y);
    const float q = 1.f - p_t;                 // modulating base
    const float dq = -(2.f * y - 1.f) * p * (1.f - p);  // d(1 - p_t)/dx
    const float qg = powf(q, gamma);
    const float dqg = (q > 0.f) ? gamma * powf(q, gamma - 1.f) * dq : 0.f;
    const float a = alpha >= 0.f ? alpha * y + (1.f - alpha) * (1.f - y) : 1.f;
    val = a * bce * qg;
    grad = a * (dbce * qg + bce * dqg);
  }
}
__global__ __launch_bounds__(256) void focal_partial_kernel(const float* __restrict__ logits,
                                                            const float* __restrict__ target, int64_t n, float gamma,
                                                            float alpha, int mode, double* __restrict__ stats) {
  double v[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float val, g;
    focal_term(logits[i], target[i], gamma, alpha, mode, val, g);
    v[0] += (double)val;
  }
  block_sum_store<1>(v, stats + 1 + blockIdx.x);
}
__global__ __launch_bounds__(256) void focal_bwd_kernel(const float* __restrict__ logits,
                                                        const float* __restrict__ target, int64_t n, float gamma,
                                                        float alpha, int mode, float scale,
                                                        const float* __restrict__ grad_scale,
                                                        float* __restrict__ dlogits) {
  const float k = upstream_scale(grad_scale) * scale;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float val, g;
    focal_term(logits[i], target[i], gamma, alpha, mode, val, g);
    dlogits[i] = k * g;
  }
}

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_loss_stats_doubles(int32_t K) { return (int64_t)K * (1 + kLossBlocks); }
extern "C" int64_t evk_prob_stats_doubles(int32_t C) { return (int64_t)3 * C * (1 + kStreamBlocks); }

extern "C" int evk_soft_ce_fwd(const float* logits, const float* target, int64_t npix, int32_t C, float* loss,
                               double* stats, void* stream) {
  EVK_REQUIRE(logits && target && loss && stats && npix > 0 && C >= 1, EVK_E_INVALID, "soft_ce_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int nb = fwd_grid(npix, kLossPix, kLossBlocks);
  hipLaunchKernelGGL(soft_ce_partial_kernel, dim3(nb), dim3(256), 0, st, logits, target, npix, C, stats);
  hipLaunchKernelGGL(finalize_partials_kernel, dim3(1), dim3(256), 0, st, stats, 1, nb);
  hipLaunchKernelGGL(loss_scale_store_kernel, dim3(1), dim3(64), 0, st, (const double*)stats, 1.0 / (double)npix, loss);
  return check_launch("soft_ce_fwd");
}
extern "C" int evk_soft_ce_bwd(const float* logits, const float* target, int64_t npix, int32_t C,
                               const float* grad_scale, float* dlogits, void* stream) {
  EVK_REQUIRE(logits && target && dlogits && npix > 0 && C >= 1, EVK_E_INVALID, "soft_ce_bwd: bad argument");
  hipLaunchKernelGGL(soft_ce_bwd_kernel, dim3(bwd_grid(npix)), dim3(256), 0, (hipStream_t)stream, logits, target, npix,
                     C, (float)(1.0 / (double)npix), grad_scale, dlogits);
  return check_launch("soft_ce_bwd");
}

extern "C" int evk_bce_fwd_ex(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                              float label_smoothing, float pos_weight, int32_t reduction, float* loss, double* stats,
                              void* stream) {
  EVK_REQUIRE(logits && labels && loss && stats && npix > 0, EVK_E_INVALID, "bce_fwd: bad argument");
  EVK_REQUIRE(reduction == 0 || reduction == 1, EVK_E_UNSUPPORTED, "bce_fwd: reduction must be 0 (mean) or 1 (sum)");
  hipStream_t st = (hipStream_t)stream;
  const int nb = fwd_grid(npix, kLossPix, kLossBlocks);
  hipLaunchKernelGGL(bce_partial_kernel, dim3(nb), dim3(256), 0, st, logits, labels, npix, ignore_index,
                     label_smoothing, pos_weight, stats);
  hipLaunchKernelGGL(finalize_partials_kernel, dim3(2), dim3(256), 0, st, stats, 2, nb);
  if (reduction == 0) {
    hipLaunchKernelGGL(mean_loss_kernel, dim3(1), dim3(64), 0, st, (const double*)stats, loss);
  } else {
    hipLaunchKernelGGL(loss_scale_store_kernel, dim3(1), dim3(64), 0, st, (const double*)stats, 1.0, loss);
  }
  return check_launch("bce_fwd");
}
extern "C" int evk_bce_fwd(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                           float label_smoothing, float* loss, double* stats, void* stream) {
  return evk_bce_fwd_ex(logits, labels, npix, ignore_index, label_smoothing, 1.f, 0, loss, stats, stream);
}
extern "C" int evk_bce_bwd_ex(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                              float label_smoothing, float pos_weight, int32_t reduction, const double* stats,
                              const float* grad_scale, float* dlogits, int32_t accumulate, void* stream) {
  EVK_REQUIRE(logits && labels && stats && dlogits && npix > 0, EVK_E_INVALID, "bce_bwd: bad argument");
  hipLaunchKernelGGL(bce_bwd_kernel, dim3(bwd_grid(npix)), dim3(256), 0, (hipStream_t)stream, logits, labels, npix,
                     ignore_index, label_smoothing, pos_weight, reduction == 1 ? 1 : 0, stats, grad_scale, dlogits,
                     accumulate);
  return check_launch("bce_bwd");
}
extern "C" int evk_bce_bwd(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                           float label_smoothing, const double* stats, const float* grad_scale, float* dlogits,
                           int32_t accumulate, void* stream) {
  return evk_bce_bwd_ex(logits, labels, npix, ignore_index, label_smoothing, 1.f, 0, stats, grad_scale, dlogits,
                        accumulate, stream);
}

extern "C" int evk_dice_stats(const float* logits, const int64_t* labels, int64_t npix, int32_t C, int64_t ignore_index,
                              double* stats, void* stream) {
  EVK_REQUIRE(logits && labels && stats && npix > 0, EVK_E_INVALID, "dice_stats: bad argument");
  EVK_REQUIRE(C >= 1 && C <= kDiceMaxClasses, EVK_E_UNSUPPORTED,
              "dice_stats: C=%d outside [1,%d] (the softmax path keeps 256 x 2C doubles in 64 KiB of LDS)", C,
              kDiceMaxClasses);
  hipStream_t st = (hipStream_t)stream;
  const int nb = fwd_grid(npix, kLossPix, kLossBlocks);
  if (C == 1) {
    hipLaunchKernelGGL(dice_partial_kernel<1>, dim3(nb), dim3(256), 0, st, logits, labels, npix, C, ignore_index, stats);
  } else {
    const size_t lds = (size_t)256 * 2 * C * sizeof(double);
    hipLaunchKernelGGL(dice_partial_kernel<0>, dim3(nb), dim3(256), lds, st, logits, labels, npix, C, ignore_index,
                       stats);
  }
  hipLaunchKernelGGL(finalize_partials_kernel, dim3(2 * C), dim3(256), 0, st, stats, 2 * C, nb);
  return check_launch("dice_stats");
}
extern "C" int evk_dice_finish(const double* stats, int32_t C, float smooth, int32_t ignore_channel, float* loss,
                               void* stream) {
  EVK_REQUIRE(stats && loss && C >= 1, EVK_E_INVALID, "dice_finish: bad argument");
  hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, C, smooth, ignore_channel,
                     loss);
  return check_launch("dice_finish");
}
extern "C" int evk_dice_bwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C, int64_t ignore_index,
                            const double* stats, float smooth, int32_t ignore_channel, const float* grad_scale,
                            float* dlogits, int32_t accumulate, void* stream) {
  EVK_REQUIRE(logits && labels && stats && dlogits && npix > 0 && C >= 1 && C <= kMaxClasses, EVK_E_INVALID,
              "dice_bwd: bad argument");
  const int nb = bwd_grid(npix);
  if (C == 1)
    hipLaunchKernelGGL(dice_bwd_kernel<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, logits, labels, npix, C,
                       ignore_index, stats, smooth, ignore_channel, grad_scale, dlogits, accumulate);
  else
    hipLaunchKernelGGL(dice_bwd_kernel<0>, dim3(nb), dim3(256), 0, (hipStream_t)stream, logits, labels, npix, C,
                       ignore_index, stats, smooth, ignore_channel, grad_scale, dlogits, accumulate);
  return check_launch("dice_bwd");
}

extern "C" int evk_ce_fwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C, int64_t ignore_index,
                          float label_smoothing, float* loss, double* stats, void* stream) {
  EVK_REQUIRE(logits && labels && loss && stats && npix > 0 && C >= 1, EVK_E_INVALID, "ce_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int nb = fwd_grid(npix, kLossPix, kLossBlocks);
  hipLaunchKernelGGL(ce_partial_kernel, dim3(nb), dim3(256), 0, st, logits, labels, npix, C, ignore_index, stats);
  hipLaunchKernelGGL(finalize_partials_kernel, dim3(3), dim3(256), 0, st, stats, 3, nb);
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)stats, C, label_smoothing, loss);
  return check_launch("ce_fwd");
}
extern "C" int evk_ce_bwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C, int64_t ignore_index,
                          float label_smoothing, const double* stats, const float* grad_scale, float* dlogits,
                          int32_t accumulate, void* stream) {
  EVK_REQUIRE(logits && labels && stats && dlogits && npix > 0 && C >= 1, EVK_E_INVALID, "ce_bwd: bad argument");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(bwd_grid(npix)), dim3(256), 0, (hipStream_t)stream, logits, labels, npix, C,
                     ignore_index, label_smoothing, stats, grad_scale, dlogits, accumulate);
  return check_launch("ce_bwd");
}

extern "C" int evk_prob_stats(const float* logits, const int64_t* labels, int64_t npix, int32_t C, int64_t ignore_index,
                              double* stats, void* stream) {
  EVK_REQUIRE(logits && labels && stats, EVK_E_INVALID, "prob_stats: null pointer");
  EVK_REQUIRE(C >= 1 && C <= kProbStatsMaxC, EVK_E_UNSUPPORTED, "prob_stats: C=%d outside [1,%d]", C, kProbStatsMaxC);
  hipStream_t st = (hipStream_t)stream;
  const int nblk = fwd_grid(npix, kStreamPix, kStreamBlocks);
  hipLaunchKernelGGL(prob_stats_kernel, dim3(nblk), dim3(256), 0, st, logits, labels, npix, C, ignore_index, stats);
  hipLaunchKernelGGL(finalize_partials_in_order_kernel, dim3(1), dim3(256), 0, st, stats, 3 * C, nblk);
  return check_launch("prob_stats");
}
extern "C" int evk_prob_stats_bwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
                                  int64_t ignore_index, const float* g_tp, const float* g_sp, float* dlogits,
                                  int32_t accumulate, void* stream) {
  EVK_REQUIRE(logits && labels && g_tp && g_sp && dlogits, EVK_E_INVALID, "prob_stats_bwd: null pointer");
  EVK_REQUIRE(C >= 1 && C <= kProbStatsMaxC, EVK_E_UNSUPPORTED, "prob_stats_bwd: C=%d outside [1,%d]", C,
              kProbStatsMaxC);
  hipLaunchKernelGGL(prob_stats_bwd_kernel, dim3(bwd_grid(npix)), dim3(256), 0, (hipStream_t)stream, logits, labels,
                     npix, C, ignore_index, g_tp, g_sp, dlogits, accumulate);
  return check_launch("prob_stats_bwd");
}

extern "C" int evk_focal_fwd(const float* logits, const float* target, int64_t n, float gamma, float alpha,
                             int32_t mode, int32_t mean, float* loss, double* stats, void* stream) {
  EVK_REQUIRE(logits && target && loss && stats, EVK_E_INVALID, "focal_fwd: null pointer");
  EVK_REQUIRE(mode >= 0 && mode <= 2, EVK_E_INVALID, "focal_fwd: mode %d", mode);
  hipStream_t st = (hipStream_t)stream;
  const int nblk = fwd_grid(n, kStreamPix, kStreamBlocks);
  hipLaunchKernelGGL(focal_partial_kernel, dim3(nblk), dim3(256), 0, st, logits, target, n, gamma, alpha, mode, stats);
  hipLaunchKernelGGL(finalize_partials_in_order_kernel, dim3(1), dim3(64), 0, st, stats, 1, nblk);
  hipLaunchKernelGGL(loss_scale_store_kernel, dim3(1), dim3(64), 0, st, (const double*)stats,
                     mean ? 1.0 / (double)n : 1.0, loss);
  return check_launch("focal_fwd");
}
extern "C" int evk_focal_bwd(const float* logits, const float* target, int64_t n, float gamma, float alpha,
                             int32_t mode, int32_t mean, const float* grad_scale, float* dlogits, void* stream) {
  EVK_REQUIRE(logits && target && dlogits, EVK_E_INVALID, "focal_bwd: null pointer");
  hipLaunchKernelGGL(focal_bwd_kernel, dim3(bwd_grid(n)), dim3(256), 0, (hipStream_t)stream, logits, target, n, gamma,
                     alpha, mode, mean ? 1.f / (float)n : 1.f, grad_scale, dlogits);
  return check_launch("focal_bwd");
}
