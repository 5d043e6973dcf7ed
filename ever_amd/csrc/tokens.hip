// The token prefix of a ViT: out[b] = cat(prefix [P][C], patch[b] [HW][C]) — the reference's prepare_tokens_with_masks without
// masks, cat([cls.expand(B), storage.expand(B), patches], dim=1) (ever/module/dinov3/models/vision_transformer.py:201-231).
// Forward and the patch gradient are 16-byte copies over a capped grid; the prefix gradient dprefix[t][c] = sum_b dout[b][t][c]
// is summed by one lane per 16-byte column in batch order: no atomics, same bits every run.  64-bit element offsets.
#include "common.hpp"

namespace evk {

constexpr int kTokGridCap = 1024;   // workgroups of 256 lanes; a larger tensor takes more than one trip

__global__ __launch_bounds__(256) void tokens_prepend_fwd_kernel(const f32x4* __restrict__ patch, const f32x4* __restrict__ prefix,
                                                                 f32x4* __restrict__ out, int64_t total, int64_t hw4, int64_t p4) {
  const int64_t per = p4 + hw4;   // 16-byte words of one sample of out
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / per, r = i - b * per;
    out[i] = r < p4 ? prefix[r] : patch[b * hw4 + (r - p4)];
  }
}

__global__ __launch_bounds__(256) void tokens_prepend_bwd_kernel(const f32x4* __restrict__ dout, f32x4* __restrict__ dpatch,
                                                                 int64_t total, int64_t hw4, int64_t p4) {
  const int64_t per = p4 + hw4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / hw4, r = i - b * hw4;
    dpatch[i] = dout[b * per + p4 + r];
  }
}

__global__ __launch_bounds__(256) void tokens_prefix_grad_kernel(const f32x4* __restrict__ dout, f32x4* __restrict__ dprefix,
                                                                 int B, int64_t hw4, int64_t p4) {
  const int64_t per = p4 + hw4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p4; i += (int64_t)gridDim.x * 256) {
    f32x4 s = dout[i];
    for (int b = 1; b < B; ++b) s += dout[(int64_t)b * per + i];
    dprefix[i] = s;
  }
}

static int tokens_check(const char* what, int32_t B, int64_t HW, int32_t P, int32_t C) {
  EVK_REQUIRE(B >= 1 && HW >= 1, EVK_E_INVALID, "%s: B = %d, HW = %lld: at least one sample and one patch", what, B, (long long)HW);
  EVK_REQUIRE(P >= 1, EVK_E_INVALID, "%s: P = %d: at least one prefix token", what, P);
  EVK_REQUIRE(C >= 4 && C % 4 == 0, EVK_E_INVALID, "%s: C = %d is not a positive multiple of 4", what, C);
  return EVK_OK;
}

static inline unsigned tok_grid(int64_t n) { return (unsigned)(n < (int64_t)kTokGridCap * 256 ? ceil_div(n, 256) : kTokGridCap); }

}  // namespace evk

using namespace evk;

extern "C" int evk_tokens_prepend_fwd(const float* patch, const float* prefix, float* out, int32_t B, int64_t HW, int32_t P,
                                      int32_t C, void* stream) {
  int rc = tokens_check("tokens_prepend_fwd", B, HW, P, C);
  if (rc) return rc;
  EVK_REQUIRE(patch && prefix && out, EVK_E_INVALID, "tokens_prepend_fwd: null pointer");
  EVK_REQUIRE(aligned16(patch) && aligned16(prefix) && aligned16(out), EVK_E_INVALID,
              "tokens_prepend_fwd: patch, prefix and out must be 16-byte aligned");
  const int64_t c4 = C / 4, hw4 = HW * c4, p4 = (int64_t)P * c4, total = B * (hw4 + p4);
  hipLaunchKernelGGL(tokens_prepend_fwd_kernel, dim3(tok_grid(total)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(patch), reinterpret_cast<const f32x4*>(prefix), reinterpret_cast<f32x4*>(out),
                     total, hw4, p4);
  return check_launch("tokens_prepend_fwd");
}

extern "C" int evk_tokens_prepend_bwd(const float* dout, float* dpatch, float* dprefix, int32_t B, int64_t HW, int32_t P, int32_t C,
                                      void* stream) {
  int rc = tokens_check("tokens_prepend_bwd", B, HW, P, C);
  if (rc) return rc;
  if (!dpatch && !dprefix) return EVK_OK;
  EVK_REQUIRE(dout, EVK_E_INVALID, "tokens_prepend_bwd: null pointer");
  EVK_REQUIRE(aligned16(dout) && aligned16(dpatch) && aligned16(dprefix), EVK_E_INVALID,
              "tokens_prepend_bwd: dout, dpatch and dprefix must be 16-byte aligned");
  const int64_t c4 = C / 4, hw4 = HW * c4, p4 = (int64_t)P * c4;
  hipStream_t st = (hipStream_t)stream;
  if (dpatch)
    hipLaunchKernelGGL(tokens_prepend_bwd_kernel, dim3(tok_grid(B * hw4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(dout),
                       reinterpret_cast<f32x4*>(dpatch), B * hw4, hw4, p4);
  if (dprefix)
    hipLaunchKernelGGL(tokens_prefix_grad_kernel, dim3(tok_grid(p4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(dout),
                       reinterpret_cast<f32x4*>(dprefix), B, hw4, p4);
  return check_launch("tokens_prepend_bwd");
}
