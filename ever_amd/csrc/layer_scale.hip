// The tail of a ConvNeXt block, `input + drop_path(gamma * x)` (reference ever/module/dinov3/models/convnext.py:20-28,78-82),
// in one pass each way on NHWC fp32 for gfx950:
//   forward   y = a + (s[n] gamma[c]) z         s[n] = floor(keep + u[n]) / keep, the drop-path factor of sample n (or null)
//   backward  dz = (s[n] gamma[c]) dy,  dgamma[c] = sum over (n, p) of s[n] (dy z);  the gradient of a is dy itself
// Each product and the sum are rounded separately, in the order written (no contraction), so y and dz are the bits of the
// fp32 expression.  3 tensor transfers forward (5 in aten: gamma * x, x / keep, * mask, + input), 3 backward (4 and a
// reduction launch in aten).
// The thread mapping is the row groups of csrc/row_groups.hpp over the R = N HW pixel rows: gamma stays in registers, dgamma
// accumulates per lane, folds to one record [C] per workgroup and is summed in order by ln_records_finalize_kernel.  No float
// atomics: two runs give the same bits.  Every element offset is 64-bit.
#include "row_groups.hpp"

namespace evk {

// sample of pixel row r (the 32-bit division where the row count allows it)
__device__ __forceinline__ float lscale_sample(const float* __restrict__ s, int64_t r, int64_t HW, bool small) {
  const int64_t n = small ? (int64_t)((uint32_t)r / (uint32_t)HW) : r / HW;
  return s[n];
}

// a + (s g) z and (s g) d with every operation rounded on its own: __fmul_rn / __fadd_rn are plain operators to this
// compiler and would be contracted into fused multiply-adds (502 ulp off the fp32 expression where a and the product cancel)
__device__ __forceinline__ float lscale_axpy(float a, float s, float g, float z) {
#pragma clang fp contract(off)
  const float f = s * g;
  const float t = f * z;
  return a + t;
}
__device__ __forceinline__ float lscale_mul(float s, float g, float d) {
#pragma clang fp contract(off)
  const float f = s * g;
  return f * d;
}

template <int COLS>
__global__ __launch_bounds__(256) void lscale_fwd_kernel(const float* __restrict__ a, const float* __restrict__ z,
                                                         const float* __restrict__ gamma, const float* __restrict__ s,
                                                         float* __restrict__ y, int64_t R, int64_t HW, int C, int L, int rows) {
  const int c4 = C >> 2;
  const int j = threadIdx.x & (L - 1), g = threadIdx.x / L;
  const bool small = R < (1ll << 31);
  f32x4 gm[COLS];
  bool on[COLS];
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    const int cb = k * L + j;
    on[k] = cb < c4;
    gm[k] = (on[k] && gamma) ? rg_ld(gamma + cb * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
  }
  for (int64_t base = (int64_t)blockIdx.x * rows; base < R; base += (int64_t)gridDim.x * rows) {
    const int64_t r = base + g;
    if (r >= R) continue;
    const float sn = s ? lscale_sample(s, r, HW, small) : 1.f;
    const int64_t o = r * C + j * 4;
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      if (!on[k]) continue;
      const int64_t ok = o + (int64_t)k * L * 4;
      const f32x4 av = rg_ld(a + ok), zv = rg_ld(z + ok);
      f32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = lscale_axpy(av[e], sn, gm[k][e], zv[e]);
      rg_st(y + ok, out);
    }
  }
}

template <int COLS>
__global__ __launch_bounds__(256) void lscale_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                         const float* __restrict__ gamma, const float* __restrict__ s,
                                                         float* __restrict__ dz, float* __restrict__ records, int64_t R,
                                                         int64_t HW, int C, int L, int rows) {
  __shared__ f32x4 red[COLS * 64];
  const int c4 = C >> 2;
  const int j = threadIdx.x & (L - 1), g = threadIdx.x / L;
  const bool small = R < (1ll << 31);
  f32x4 gm[COLS], dg[COLS];
  bool on[COLS];
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    const int cb = k * L + j;
    on[k] = cb < c4;
    gm[k] = (on[k] && gamma) ? rg_ld(gamma + cb * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
    dg[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t base = (int64_t)blockIdx.x * rows; base < R; base += (int64_t)gridDim.x * rows) {
    const int64_t r = base + g;
    if (r >= R) continue;
    const float sn = s ? lscale_sample(s, r, HW, small) : 1.f;
    const int64_t o = r * C + j * 4;
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      if (!on[k]) continue;
      const int64_t ok = o + (int64_t)k * L * 4;
      const f32x4 gv = rg_ld(dy + ok);
      if (records) dg[k] += (gv * rg_ld(z + ok)) * sn;
      if (dz) {
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = lscale_mul(sn, gm[k][e], gv[e]);
        rg_st(dz + ok, out);
      }
    }
  }
  if (records) rg_fold_record<COLS>(dg, L, c4, red, records + (int64_t)blockIdx.x * C);
}

}  // namespace evk

using namespace evk;

static int lscale_check(const char* what, int32_t N, int64_t HW, int32_t C) {
  EVK_REQUIRE(N >= 1 && HW >= 1, EVK_E_INVALID, "%s: non-positive dimension (N=%d, HW=%lld)", what, N, (long long)HW);
  return row_shape_check(what, (int64_t)N * HW, C);
}

extern "C" int evk_scale_residual_fwd(const float* a, const float* z, const float* gamma, const float* sample_scale, float* y,
                                      int32_t N, int64_t HW, int32_t C, void* stream) {
  int rc = lscale_check("scale_residual_fwd", N, HW, C);
  if (rc) return rc;
  EVK_REQUIRE(a && z && y, EVK_E_INVALID, "scale_residual_fwd: null pointer");
  EVK_REQUIRE(aligned16(a) && aligned16(z) && aligned16(y) && aligned16(gamma), EVK_E_INVALID,
              "scale_residual_fwd: a, z, y and gamma must be 16-byte aligned");
  const int64_t R = (int64_t)N * HW;
  const RowPlan p = row_plan(R, C);
  pick<1, 2, 3, 4, 5, 6, 7, 8>(p.cols, [&](auto COLS) {
    hipLaunchKernelGGL(lscale_fwd_kernel<decltype(COLS)::value>, dim3(p.workgroups), dim3(kRgThreads), 0, (hipStream_t)stream,
                       a, z, gamma, sample_scale, y, R, HW, C, p.lanes, p.rows);
    return 0;
  });
  return check_launch("scale_residual_fwd");
}

// Host only: bytes of the per-workgroup dgamma records, [workgroups of evk_ln_plan(N HW, C)][C] (0 for a shape out of scope)
extern "C" size_t evk_scale_residual_bwd_workspace_bytes(int32_t N, int64_t HW, int32_t C) {
  if (N < 1 || HW < 1 || C <= 0 || C % 4 != 0 || C > kRgMaxC) return 0;
  return (size_t)row_plan((int64_t)N * HW, C).workgroups * C * sizeof(float);
}

extern "C" int evk_scale_residual_bwd(const float* dy, const float* z, const float* gamma, const float* sample_scale,
                                      float* dz, float* dgamma, int32_t N, int64_t HW, int32_t C, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  int rc = lscale_check("scale_residual_bwd", N, HW, C);
  if (rc) return rc;
  EVK_REQUIRE(dy && (dz || dgamma) && (z || !dgamma), EVK_E_INVALID, "scale_residual_bwd: null pointer");
  EVK_REQUIRE(aligned16(dy) && aligned16(z) && aligned16(gamma) && aligned16(dz) && aligned16(dgamma) &&
                  aligned16(workspace),
              EVK_E_INVALID, "scale_residual_bwd: dy, z, gamma, dz, dgamma and the workspace must be 16-byte aligned");
  const size_t need = evk_scale_residual_bwd_workspace_bytes(N, HW, C);
  EVK_REQUIRE(!dgamma || (workspace && workspace_bytes >= need), EVK_E_WORKSPACE,
              "scale_residual_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int64_t R = (int64_t)N * HW;
  const RowPlan p = row_plan(R, C);
  hipStream_t st = (hipStream_t)stream;
  float* records = dgamma ? reinterpret_cast<float*>(workspace) : nullptr;
  pick<1, 2, 3, 4, 5, 6, 7, 8>(p.cols, [&](auto COLS) {
    hipLaunchKernelGGL(lscale_bwd_kernel<decltype(COLS)::value>, dim3(p.workgroups), dim3(kRgThreads), 0, st, dy, z, gamma,
                       sample_scale, dz, records, R, HW, C, p.lanes, p.rows);
    return 0;
  });
  if (dgamma) ln_launch_records_finalize(records, p.workgroups, 1, C, dgamma, nullptr, st);
  return check_launch("scale_residual_bwd");
}
