// One output column of a 1x1 convolution on a handful of rows: the body of conv1x1_smallm_kernel (conv_igemm_f32.hip) and of
// the FS-Relation scene MLP's forward launches (relation_scene.hip), which must give the same bits.  One workgroup of 256
// threads owns column n and all M <= kSmallM rows: it streams the weight row once with 16-byte loads, every thread sums its
// chunks kc = tid, tid + 256, ... in that order, the waves fold through wave_sum and the four wave sums as
// (r0 + r1) + (r2 + r3); then bias, then ReLU.
#pragma once
#include "common.hpp"

namespace evk {

constexpr int kSmallM = 32;

__device__ __forceinline__ void smallm_column(const float* __restrict__ src, const float* __restrict__ wgt,
                                              const float* __restrict__ bias, float* __restrict__ dst, int M, int K, int Cd,
                                              int relu, int n) {
  __shared__ float red[4][kSmallM];
  const int k4 = K >> 2;
  float acc[kSmallM];
#pragma unroll
  for (int m = 0; m < kSmallM; ++m) acc[m] = 0.f;
  for (int kc = threadIdx.x; kc < k4; kc += 256) {
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wgt + (size_t)n * K + kc * 4);
#pragma unroll
    for (int m = 0; m < kSmallM; ++m)
      if (m < M) {
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(src + (size_t)m * K + kc * 4);
        acc[m] += w4.x * x4.x + w4.y * x4.y + w4.z * x4.z + w4.w * x4.w;
      }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < kSmallM; ++m) {
    const float s = wave_sum(acc[m]);
    if (lane == 0) red[wave][m] = s;
  }
  __syncthreads();
  if (threadIdx.x < M) {
    const int m = threadIdx.x;
    float v = (red[0][m] + red[1][m]) + (red[2][m] + red[3][m]);
    if (bias) v += bias[n];
    if (relu) v = fmaxf(v, 0.f);
    dst[(size_t)m * Cd + n] = v;
  }
}

}  // namespace evk
