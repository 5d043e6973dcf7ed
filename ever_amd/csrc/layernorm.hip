// LayerNorm over the channels of a pixel (or the last axis of a token matrix) on [R][C] fp32 for gfx950 — ConvNeXt's
// LayerNorm in both of its data formats (reference ever/module/dinov3/models/convnext.py:86-113: a logical-NCHW map is
// NHWC memory here, so "channels_first" and "channels_last" are the same contiguous row of C floats) and nn.LayerNorm(C)
// on [N, HW + 1, C] tokens (convnext.py:177,224).
//
// Forward:  a row is read ONCE with 16-byte loads into the registers of its row group (csrc/row_groups.hpp: L lanes x COLS
//           columns), reduced by shuffles inside the group — no LDS — and written once: 2|x| of HBM traffic.  The mean comes
//           first, then the sum of (x - mean)^2 from the registers (never E[x^2] - mean^2: eps is 1e-6 and rows with a large
//           common offset occur).  The fp32 mean of such a row is off by up to half an ulp OF THE OFFSET; the mean of the
//           residuals x - mean, which are small and (nearly) exact, gives that rounding error back, and it is taken off
//           before the variance: one more shuffle reduction, no memory traffic.
// Backward: one pass over dy and x.  g = dy gamma, dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)); dgamma[c] = sum_r dy xhat
//           and dbeta[c] = sum_r dy accumulate in per-lane registers over the trips of the capped grid and fold, in a fixed
//           order, to one record [2][C] per workgroup; ln_records_finalize_kernel sums the records in order.  No float
//           atomics: two runs give the same bits.  3|x| + the records.
// Every element offset is 64-bit (16 x 128^2 x 1536 elements are past 2^31 bytes).
#include "row_groups.hpp"

namespace evk {

template <int COLS>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                     float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                     int64_t R, int C, int L, int rows) {
  const int c4 = C >> 2;
  const int j = threadIdx.x & (L - 1), g = threadIdx.x / L;
  const float fc = (float)C;
  f32x4 gm[COLS], bt[COLS];
  bool on[COLS];
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    const int cb = k * L + j;
    on[k] = cb < c4;
    gm[k] = (on[k] && gamma) ? rg_ld(gamma + cb * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
    bt[k] = (on[k] && beta) ? rg_ld(beta + cb * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t base = (int64_t)blockIdx.x * rows; base < R; base += (int64_t)gridDim.x * rows) {
    const int64_t r = base + g;
    const bool live = r < R;
    const float* xr = x + r * C + j * 4;
    f32x4 v[COLS];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      v[k] = (live && on[k]) ? rg_ld(xr + (int64_t)k * L * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      s += rg_hsum(v[k]);
    }
    const float mu0 = rg_group_sum(s, L) / fc;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      v[k] = on[k] ? v[k] - mu0 : v[k];      // (masked columns stay zero)
      t += rg_hsum(v[k]);
    }
    const float fix = rg_group_sum(t, L) / fc;   // the rounding error of mu0
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      v[k] = on[k] ? v[k] - fix : v[k];
      q += rg_hsum(v[k] * v[k]);
    }
    const float var = rg_group_sum(q, L) / fc;
    // (in fp64 and rounded once: 1.f / sqrtf() is two roundings, 1.02 ulp off at var = 0, eps = 1e-6; once per row)
    const float rstd = (float)(1.0 / sqrt((double)var + (double)eps));
    if (live) {
      float* yr = y + r * C + j * 4;
#pragma unroll
      for (int k = 0; k < COLS; ++k)
        if (on[k]) rg_st(yr + (int64_t)k * L * 4, v[k] * rstd * gm[k] + bt[k]);
      if (j == 0) {
        if (save_mean) save_mean[r] = mu0 + fix;
        if (save_rstd) save_rstd[r] = rstd;
      }
    }
  }
}

template <int COLS>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                                     const float* __restrict__ gamma, float* __restrict__ dx,
                                                     float* __restrict__ records, int64_t R, int C, int L, int rows) {
  __shared__ f32x4 red[COLS * 64];
  const int c4 = C >> 2;
  const int j = threadIdx.x & (L - 1), g = threadIdx.x / L;
  const float fc = (float)C;
  f32x4 gm[COLS], dg[COLS], db[COLS];
  bool on[COLS];
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    const int cb = k * L + j;
    on[k] = cb < c4;
    gm[k] = (on[k] && gamma) ? rg_ld(gamma + cb * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
    dg[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    db[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t base = (int64_t)blockIdx.x * rows; base < R; base += (int64_t)gridDim.x * rows) {
    const int64_t r = base + g;
    const bool live = r < R;
    const int64_t o = r * C + j * 4;
    const float mu = live ? save_mean[r] : 0.f, rstd = live ? save_rstd[r] : 0.f;
    f32x4 gy[COLS], xh[COLS];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      const bool ld = live && on[k];
      gy[k] = ld ? rg_ld(dy + o + (int64_t)k * L * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      xh[k] = ld ? (rg_ld(x + o + (int64_t)k * L * 4) - mu) * rstd : f32x4{0.f, 0.f, 0.f, 0.f};
      db[k] += gy[k];
      dg[k] += gy[k] * xh[k];
      gy[k] *= gm[k];
      s1 += rg_hsum(gy[k]);
      s2 += rg_hsum(gy[k] * xh[k]);
    }
    if (dx) {       // (uniform over the grid)
      const float m1 = rg_group_sum(s1, L) / fc, m2 = rg_group_sum(s2, L) / fc;
      if (live) {
#pragma unroll
        for (int k = 0; k < COLS; ++k)
          if (on[k]) rg_st(dx + o + (int64_t)k * L * 4, (gy[k] - m1 - xh[k] * m2) * rstd);
      }
    }
  }
  if (records) {
    float* rec = records + (int64_t)blockIdx.x * 2 * C;
    rg_fold_record<COLS>(dg, L, c4, red, rec);
    rg_fold_record<COLS>(db, L, c4, red, rec + C);
  }
}

// out_q[c] = sum_t rec[t][q][c]: four 16-byte columns per workgroup, 64 slices of the records each, folded in order
// (as depthwise_reduce_kernel and the BatchNorm finalisers)
__global__ __launch_bounds__(256) void ln_records_finalize_kernel(const float* __restrict__ rec, int nrec, int nq, int C,
                                                                  float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ f32x4 red[256];
  const int c4 = C >> 2;
  const int lane = threadIdx.x & 3, slice = threadIdx.x >> 2;
  const int e = blockIdx.x * 4 + lane;          // (q, column) flat: q * c4 + cb
  const bool ok = e < nq * c4;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const float* p = rec + (int64_t)e * 4;
    for (int t = slice; t < nrec; t += 64) v += rg_ld(p + (int64_t)t * nq * C);
  }
  red[threadIdx.x] = v;
  __syncthreads();
  if (slice != 0 || !ok) return;
  for (int i = 1; i < 64; ++i) v += red[i * 4 + lane];
  float* out = e < c4 ? out0 : out1;
  if (out) rg_st(out + (e % c4) * 4, v);
}

int ln_launch_records_finalize(const float* rec, int nrec, int nq, int C, float* out0, float* out1, hipStream_t st) {
  hipLaunchKernelGGL(ln_records_finalize_kernel, dim3((unsigned)ceil_div((int64_t)nq * (C / 4), 4)), dim3(256), 0, st, rec,
                     nrec, nq, C, out0, out1);
  return EVK_OK;
}

}  // namespace evk

using namespace evk;

// Host only (no launch): out = {lanes per row, 16-byte columns per lane, rows per workgroup per trip, workgroups}
extern "C" int evk_ln_plan(int64_t R, int32_t C, int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "ln_plan: null pointer");
  int rc = row_shape_check("ln_plan", R, C);
  if (rc) return rc;
  const RowPlan p = row_plan(R, C);
  out[0] = p.lanes;
  out[1] = p.cols;
  out[2] = p.rows;
  out[3] = p.workgroups;
  return EVK_OK;
}

extern "C" size_t evk_ln_bwd_workspace_bytes(int64_t R, int32_t C) {
  if (R < 1 || C <= 0 || C % 4 != 0 || C > kRgMaxC) return 0;
  return (size_t)row_plan(R, C).workgroups * 2 * C * sizeof(float);
}

extern "C" int evk_ln_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, float* save_mean,
                          float* save_rstd, int64_t R, int32_t C, void* stream) {
  int rc = row_shape_check("ln_fwd", R, C);
  if (rc) return rc;
  EVK_REQUIRE(x && y, EVK_E_INVALID, "ln_fwd: null pointer");
  EVK_REQUIRE(aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta), EVK_E_INVALID,
              "ln_fwd: x, y, gamma and beta must be 16-byte aligned");
  EVK_REQUIRE(eps >= 0.f, EVK_E_INVALID, "ln_fwd: negative eps");
  const RowPlan p = row_plan(R, C);
  hipStream_t st = (hipStream_t)stream;
  pick<1, 2, 3, 4, 5, 6, 7, 8>(p.cols, [&](auto COLS) {
    hipLaunchKernelGGL(ln_fwd_kernel<decltype(COLS)::value>, dim3(p.workgroups), dim3(kRgThreads), 0, st, x, gamma, beta, eps, y,
                       save_mean, save_rstd, R, C, p.lanes, p.rows);
    return 0;
  });
  return check_launch("ln_fwd");
}

extern "C" int evk_ln_bwd(const float* dy, const float* x, const float* save_mean, const float* save_rstd,
                          const float* gamma, float* dx, float* dgamma, float* dbeta, int64_t R, int32_t C,
                          void* workspace, size_t workspace_bytes, void* stream) {
  int rc = row_shape_check("ln_bwd", R, C);
  if (rc) return rc;
  EVK_REQUIRE(dy && x && save_mean && save_rstd, EVK_E_INVALID, "ln_bwd: null pointer");
  EVK_REQUIRE(dx || dgamma || dbeta, EVK_E_INVALID, "ln_bwd: no output requested");
  EVK_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(gamma) && aligned16(dx) && aligned16(dgamma) &&
                  aligned16(dbeta) && aligned16(workspace),
              EVK_E_INVALID, "ln_bwd: dy, x, gamma, dx, dgamma, dbeta and the workspace must be 16-byte aligned");
  const bool params = dgamma || dbeta;
  EVK_REQUIRE(!params || (workspace && workspace_bytes >= evk_ln_bwd_workspace_bytes(R, C)), EVK_E_WORKSPACE,
              "ln_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, evk_ln_bwd_workspace_bytes(R, C));
  const RowPlan p = row_plan(R, C);
  hipStream_t st = (hipStream_t)stream;
  float* records = params ? reinterpret_cast<float*>(workspace) : nullptr;
  pick<1, 2, 3, 4, 5, 6, 7, 8>(p.cols, [&](auto COLS) {
    hipLaunchKernelGGL(ln_bwd_kernel<decltype(COLS)::value>, dim3(p.workgroups), dim3(kRgThreads), 0, st, dy, x, save_mean, save_rstd,
                       gamma, dx, records, R, C, p.lanes, p.rows);
    return 0;
  });
  if (params) ln_launch_records_finalize(records, p.workgroups, 2, C, dgamma, dbeta, st);
  return check_launch("ln_bwd");
}
