// The confusion matrix of the evaluation loop (reference ever/metric/confusion_matrix.py:11-24, which goes through the
// host and scipy.sparse) accumulated on the device, from predictions or straight from logits (threshold 0 / argmax
// fused).  Integer: an LDS-privatised histogram + integer atomics, exact in any order.
#include "loss_common.hpp"

namespace evk {

constexpr int kCmLdsBins = 4096;
template <int FROM_LOGITS>
__global__ __launch_bounds__(256) void confusion_kernel(const void* __restrict__ pred_or_logits,
                                                        const int64_t* __restrict__ y_true, int64_t n, int Cl, int C,
                                                        unsigned long long* __restrict__ cm) {
  __shared__ unsigned int h[kCmLdsBins];
  const int bins = C * C;
  const bool lds = bins <= kCmLdsBins;
  if (lds) {
    for (int i = threadIdx.x; i < bins; i += 256) h[i] = 0u;
    __syncthreads();
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t t = y_true[i];
    int64_t pr;
    if (FROM_LOGITS) {
      const float* z = reinterpret_cast<const float*>(pred_or_logits) + i * Cl;
      if (Cl == 1) {
        pr = z[0] > 0.f ? 1 : 0;  // sigmoid(z) > 0.5
      } else {
        int best = 0;
        float bv = z[0];
        for (int c = 1; c < Cl; ++c)
          if (z[c] > bv) { bv = z[c]; best = c; }  // first maximum, as torch.argmax
        pr = best;
      }
    } else {
      pr = reinterpret_cast<const int64_t*>(pred_or_logits)[i];
    }
    if (t < 0 || t >= C || pr < 0 || pr >= C) continue;  // ignore labels (255, -1) fall outside [0, C)
    const int bin = (int)t * C + (int)pr;
    if (lds) atomicAdd(&h[bin], 1u);
    else atomicAdd(&cm[bin], 1ull);
  }
  if (lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
      if (h[i]) atomicAdd(&cm[i], (unsigned long long)h[i]);
  }
}

}  // namespace evk

using namespace evk;

extern "C" int evk_confusion_matrix(const int64_t* y_true, const int64_t* y_pred, int64_t n, int32_t num_classes,
                                    int64_t* cm, void* stream) {
  EVK_REQUIRE(y_true && y_pred && cm, EVK_E_INVALID, "confusion_matrix: null pointer");
  EVK_REQUIRE(num_classes >= 1 && num_classes <= 4096, EVK_E_UNSUPPORTED, "confusion_matrix: %d classes", num_classes);
  hipLaunchKernelGGL(confusion_kernel<0>, dim3(fwd_grid(n, kStreamPix, kStreamBlocks)), dim3(256), 0, (hipStream_t)stream,
                     (const void*)y_pred, y_true, n, 0, num_classes, reinterpret_cast<unsigned long long*>(cm));
  return check_launch("confusion_matrix");
}

extern "C" int evk_confusion_from_logits(const float* logits, const int64_t* y_true, int64_t npix, int32_t C_logits,
                                         int32_t num_classes, int64_t* cm, void* stream) {
  EVK_REQUIRE(logits && y_true && cm, EVK_E_INVALID, "confusion_from_logits: null pointer");
  EVK_REQUIRE(C_logits >= 1 && num_classes >= (C_logits == 1 ? 2 : C_logits) && num_classes <= 4096, EVK_E_INVALID,
              "confusion_from_logits: %d logit channels vs %d classes", C_logits, num_classes);
  hipLaunchKernelGGL(confusion_kernel<1>, dim3(fwd_grid(npix, kStreamPix, kStreamBlocks)), dim3(256), 0, (hipStream_t)stream,
                     (const void*)logits, y_true, npix, C_logits, num_classes, reinterpret_cast<unsigned long long*>(cm));
  return check_launch("confusion_from_logits");
}
