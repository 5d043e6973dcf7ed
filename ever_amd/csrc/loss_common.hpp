// What the loss and metric kernels share (loss.hip, loss_pixel.hip, metric.hip): the per-pixel softmax, the sigmoid /
// softplus forms, the gradient-store idioms, the launch grids, the workgroup sum of doubles and the two folds of the
// per-workgroup partials.  Every piece is written once here; a kernel of the family that needs one calls it.
#pragma once
#include "common.hpp"

namespace evk {

// ---------------------------------------------------------------- grids (256 threads per workgroup)
// Forward: one workgroup per `pix_per_block` elements, at most `max_blocks`; the scalar losses of loss.hip keep
// kLossBlocks x K partials, the streaming kernels (class-probability statistics, focal, OHEM, confusion) kStreamBlocks.
constexpr int kLossPix = 2048, kLossBlocks = 2048;   // >= 8 pixels per thread; 256 workgroups left the 4-million-pixel
                                                     // losses on a quarter of the chip (62 us for 50 MB)
constexpr int kStreamPix = 1024, kStreamBlocks = 256;
static inline int fwd_grid(int64_t n, int pix_per_block, int max_blocks) {
  const int64_t b = (n + pix_per_block - 1) / pix_per_block;
  return (int)(b > max_blocks ? max_blocks : (b < 1 ? 1 : b));
}
// Backward and per-pixel kernels: one thread per element up to 4096 workgroups, grid-stride beyond.
static inline int bwd_grid(int64_t n) { return fwd_grid(n, 256, 4096); }

// ---------------------------------------------------------------- element functions
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float softplus_neg_abs(float x) { return log1pf(expf(-fabsf(x))); }  // log(1 + e^-|x|)
// sigmoid as exp(logsigmoid(z)), the way the reference's statistics compute it (ever/module/loss.py:121)
__device__ __forceinline__ float logsigmoid_prob(float z) { return expf(fminf(z, 0.f) - softplus_neg_abs(z)); }

// ---------------------------------------------------------------- the pixel softmax
// m = max_c x_c and ls = log sum_c exp(x_c - m) of one pixel's C logits; p(x_c) is the softmax probability.
// log p_c = (x_c - m) - ls and not x_c - (m + ls): the subtraction x_c - m is exact near the maximum, so nothing is
// rounded at the size of m (m + ls would lose a small loss under a large logit).  This is log_softmax(dim=1).exp().
struct PixelSoftmax {
  float m, ls;
  __device__ __forceinline__ float p(float xc) const { return expf((xc - m) - ls); }
};
// also(c, x_c - m) runs inside the exponential pass, after that channel's term is added: a kernel that accumulates a
// second quantity there (CE's sum of x_c - m, soft CE's target mass) keeps its own order of additions.
template <class Also>
__device__ __forceinline__ PixelSoftmax pixel_softmax(const float* x, int C, Also&& also) {
  float m = x[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float se = 0.f;
  for (int c = 0; c < C; ++c) {
    se += expf(x[c] - m);
    also(c, x[c] - m);
  }
  return {m, logf(se)};
}
__device__ __forceinline__ PixelSoftmax pixel_softmax(const float* x, int C) {
  return pixel_softmax(x, C, [](int, float) {});
}

// ---------------------------------------------------------------- gradient stores
__device__ __forceinline__ float upstream_scale(const float* grad_scale) { return grad_scale ? *grad_scale : 1.f; }
// d[i] as base and index, not a pointer to the word: with the one pointer for load and store the compiler turns the
// channel loops of ce_bwd / dice_bwd into two-wide vector loops with twice the registers
__device__ __forceinline__ void store_grad(float* d, int64_t i, float v, int accumulate) {
  d[i] = accumulate ? d[i] + v : v;
}
// an ignored pixel has no gradient: zero its C words, or leave what is there when accumulating
__device__ __forceinline__ void zero_grad(float* d, int C, int accumulate) {
  if (!accumulate)
    for (int c = 0; c < C; ++c) d[c] = 0.f;
}

// ---------------------------------------------------------------- workgroup sum of K doubles (256 threads)
// v[k] becomes the sum over the workgroup in every thread: a wave sum, then the four waves folded as
// (w0 + w1) + (w2 + w3).  The leading barrier lets a kernel call it again before every wave has read the last result.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K]) {
  __shared__ double red[K][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = wave_sum_d(v[k]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][wave] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}
__device__ __forceinline__ double block_sum(double v) {
  double a[1] = {v};
  block_sum<1>(a);
  return a[0];
}
template <int K>  // ... and thread 0 writes the K sums: a workgroup's row of partials
__device__ __forceinline__ void block_sum_store(double (&v)[K], double* out) {
  block_sum<K>(v);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = v[k];
  }
}

// ---------------------------------------------------------------- folds of the per-workgroup partials
// stats layout: [K finals][nblk x K partials].  The finals go out as fp64 (prob_stats returns them) and into the fp32
// loss, so the order of additions is part of the value: the two folds stay two.
//
// In index order, one thread per k.  Class-probability statistics and focal (at most 256 partials per k) use it; a
// tree over them would change the fp64 statistics that tversky-like losses read.
__device__ __forceinline__ void fold_partials_in_order(double* stats, int K, int nblk) {
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += stats[K + (size_t)b * K + k];
    stats[k] = s;
  }
}
// One workgroup of 256 per k: 256 strided sub-sums, then a halving tree through LDS.  BCE, dice, CE and soft CE (up
// to 2048 partials per k) use it; it replaced one thread per k walking all of them, and its order has been their value since.
__device__ __forceinline__ void fold_partials_tree(double* stats, int K, int nblk) {
  __shared__ double red[256];
  const int k = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += stats[K + (size_t)b * K + k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[k] = red[0];
}

}  // namespace evk
