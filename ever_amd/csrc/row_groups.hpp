// Row groups: the thread mapping the row LayerNorm (csrc/layernorm.hip) and the layer-scale residual (csrc/layer_scale.hip)
// share for an [R][C] fp32 matrix whose per-channel sums over the rows they need in a fixed order.
//
// A row belongs to L consecutive lanes (L a power of two, 1..64); lane j of the group holds the 16-byte columns
// j, j + L, ... j + (COLS - 1) L of its row in registers (columns past C/4 are masked).  A workgroup of 256 threads takes
// 256 / L rows per trip and walks the matrix with the stride of the (capped) grid, so that a per-channel sum over the rows
// is first a per-lane register over the trips, then ONE record per workgroup (rg_fold_record: the groups of a wave by
// shuffles, the four waves one after the other through LDS), and last the ordered sum of at most kRgMaxWorkgroups records
// (ln_records_finalize_kernel).  No float atomics: two runs give the same bits.
#pragma once
#include "common.hpp"

namespace evk {

constexpr int kRgThreads = 256;
constexpr int kRgMaxCols = 8;             // 16-byte columns a lane holds: C <= 4 * 64 * 8 = 2048
constexpr int kRgFewCols = 4;
constexpr int kRgMaxC = 4 * kWave * kRgMaxCols;
constexpr int kRgMaxWorkgroups = 1024;    // four workgroups per CU; bounds the records whatever R is

struct RowPlan {
  int lanes;        // L
  int cols;         // ceil(C / 4 / L)
  int rows;         // rows of a workgroup per trip: 256 / L
  int workgroups;
};

// The L with the fewest masked columns among those that keep cols <= kRgMaxCols; of equals the narrowest that holds at most
// kRgFewCols columns (several 16-byte loads in flight per lane and fewer shuffle steps per row: with one column per lane the
// row's reductions, not its bytes, fill the SIMD), else the widest.  C = 96: L = 8 x 3 columns, every lane busy; C = 100:
// L = 4 x 7, 3 of 28 masked; C = 256: L = 16 x 4; C = 1536: L = 64 x 6.
inline RowPlan row_plan(int64_t R, int C) {
  const int c4 = C / 4;
  RowPlan p{1, c4, kRgThreads, 1};
  int best = 1 << 30;
  for (int L = 1; L <= kWave; L <<= 1) {
    const int cols = (c4 + L - 1) / L;
    if (cols > kRgMaxCols) continue;
    const int waste = L * cols - c4;
    if (waste < best || (waste == best && p.cols > kRgFewCols)) {
      best = waste;
      p.lanes = L;
      p.cols = cols;
    }
  }
  p.rows = kRgThreads / p.lanes;
  const int64_t wg = (R + p.rows - 1) / p.rows;
  p.workgroups = (int)(wg < 1 ? 1 : (wg > kRgMaxWorkgroups ? kRgMaxWorkgroups : wg));
  return p;
}

// what both families refuse before a launch
inline int row_shape_check(const char* what, int64_t R, int32_t C) {
  EVK_REQUIRE(R >= 1 && C > 0, EVK_E_INVALID, "%s: non-positive dimension (R=%lld, C=%d)", what, (long long)R, C);
  EVK_REQUIRE(C % 4 == 0 && C <= kRgMaxC, EVK_E_UNSUPPORTED, "%s: C=%d must be a multiple of 4 in 4..%d", what, C, kRgMaxC);
  return EVK_OK;
}

#if defined(__HIPCC__)
__device__ __forceinline__ f32x4 rg_ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void rg_st(float* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float rg_hsum(const f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// sum over the L lanes of a row group (L a power of two, groups aligned to L): every lane gets the sum
__device__ __forceinline__ float rg_group_sum(float v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Per-lane accumulators of a workgroup -> its record rec[C] (16-byte column k L + j from lane j's acc[k]).  Fixed order:
// the groups of a wave by xor shuffles (L, 2L, .. 32), then wave 0, 1, 2, 3 through red[COLS * 64].  Every thread of the
// workgroup calls it; red may be reused right after.
template <int COLS>
__device__ __forceinline__ void rg_fold_record(f32x4 (&acc)[COLS], int L, int c4, f32x4* red, float* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = L; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      f32x4 t;
      t.x = __shfl_xor(acc[k].x, o, 64);
      t.y = __shfl_xor(acc[k].y, o, 64);
      t.z = __shfl_xor(acc[k].z, o, 64);
      t.w = __shfl_xor(acc[k].w, o, 64);
      acc[k] += t;
    }
  }
  for (int w = 0; w < kRgThreads / 64; ++w) {
    if (wave == w && lane < L) {
#pragma unroll
      for (int k = 0; k < COLS; ++k) red[k * 64 + lane] = w ? red[k * 64 + lane] + acc[k] : acc[k];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < L) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
      const int cb = k * L + (int)threadIdx.x;
      if (cb < c4) rg_st(rec + cb * 4, red[k * 64 + threadIdx.x]);
    }
  }
  __syncthreads();
}
#endif

// out_q[c] = sum over t < nrec of rec[t][q][c], q < nq <= 2, in a fixed order (csrc/layernorm.hip); a null out_q is skipped
int ln_launch_records_finalize(const float* rec, int nrec, int nq, int C, float* out0, float* out1, hipStream_t st);

}  // namespace evk
