// The scene branch of FS-Relation (reference fs_relation.py:23-29,56-60): L <= 8 MLPs  Conv2d(K, C, 1) -> ReLU -> Conv2d(C, C, 1)
// on one pooled vector per image, s [N][K] with N <= kSmallM rows.  Layer by layer that is ~16 launches per level and pass
// of kernels that are almost pure launch latency; here it is two launches forward and three backward, for all levels:
//   F1  h[l][n][j] = relu(b1[l][j] + sum_k W1[l][j][k] s[n][k])          F2  o[l][n][i] = b2[l][i] + sum_j W2[l][i][j] h[l][n][j]
//   B1  dW2[l][i][j] = sum_n g[l][n][i] h[l][n][j]    db2[l][i] = sum_n g[l][n][i]
//       dh[l][n][j]  = h[l][n][j] > 0 ? sum_i W2[l][i][j] g[l][n][i] : 0
//   B2  dW1[l][j][k] = sum_n dh[l][n][j] s[n][k]      db1[l][j] = sum_n dh[l][n][j]
//       part[q][n][k] = sum over the rows (l, j) of slice q of W1[l][j][k] dh[l][n][j]
//   B3  ds[n][k] = sum_q part[q][n][k]
// All fp32, no atomics.  Every sum has ONE order, fixed by the shapes alone: n, i and the rows of a slice ascending inside a
// thread, the four waves of B1's dh as (w0 + w1) + (w2 + w3), the slices ascending in B3.  The forward is the body of
// conv1x1_smallm_kernel (smallm_body.hpp) with blockIdx.y = level: the same bits as the layer path.
// The per-level pointers (the modules' own parameters and gradients, the relation backward's dscene tensors) travel by value
// in the kernel arguments: no device-side table, no copy, nothing a stream capture could not record.
#include "smallm_body.hpp"

namespace evk {

constexpr int kSceneLevels = 8;
struct SceneIn { const float* p[kSceneLevels]; };
struct SceneOut { float* p[kSceneLevels]; };

// src + level * src_level (F1: 0, every level reads s; F2: N * C, level l reads h[l]) -> dst[level][M][Cd]
__global__ __launch_bounds__(256) void relation_scene_fwd_kernel(const float* __restrict__ src, size_t src_level, const SceneIn wgt,
                                                                 const SceneIn bias, float* __restrict__ dst, int M, int K, int Cd,
                                                                 int relu) {
  const int l = blockIdx.y;
  smallm_column(src + l * src_level, wgt.p[l], bias.p[l], dst + (size_t)l * M * Cd, M, K, Cd, relu, blockIdx.x);
}

// ---- B1.  blockIdx.y = level.  blockIdx.x < na: dW2 / db2, one thread per (i, four columns j): the sum over n in a register,
// 16-byte stores along j.  The others: dh for kDhCols columns j (one per lane: the reads of W2's rows run along j) and kDhRows
// rows n; wave w sums the rows i of its quarter of W2, 64 at a time: their g values wait in the LDS (gt), so that the loop holds
// nothing but the loads of W2's rows — independent of each other, many in flight — and broadcast LDS reads.  (With the g values
// fetched inside the loop every step waited for its own scalar loads: 64 us for what is now a few.)
constexpr int kDhCols = 64, kDhRows = 8;
__global__ __launch_bounds__(256) void relation_scene_bwd_w2_kernel(const SceneIn g, const float* __restrict__ h, const SceneIn w2,
                                                                    const SceneOut dw2, const SceneOut db2, float* __restrict__ dh,
                                                                    int N, int C, int na, int col_tiles) {
  __shared__ float red[4][kDhRows][kDhCols];
  __shared__ __attribute__((aligned(16))) float gt[4][kDhRows][64];
  const int l = blockIdx.y, c4 = C >> 2;
  const float* __restrict__ gl = g.p[l];      // (null: this level's output had no gradient = zeros)
  const float* __restrict__ hl = h + (size_t)l * N * C;
  if ((int)blockIdx.x < na) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * c4) return;
    const int i = idx / c4, jc = idx - i * c4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float gsum = 0.f;
    for (int nb = 0; nb < N; nb += 8) {       // eight rows' loads in flight (from a valid row, zeroed past N), then n ascending
      float gv[8];
      f32x4 h4[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int n = min(nb + u, N - 1);
        gv[u] = gl ? gl[(size_t)n * C + i] : 0.f;
        h4[u] = *reinterpret_cast<const f32x4*>(hl + (size_t)n * C + jc * 4);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (nb + u < N) {
          acc.x += gv[u] * h4[u].x; acc.y += gv[u] * h4[u].y; acc.z += gv[u] * h4[u].z; acc.w += gv[u] * h4[u].w;
          gsum += gv[u];
        }
    }
    *reinterpret_cast<f32x4*>(dw2.p[l] + (size_t)i * C + jc * 4) = acc;
    if (jc == 0) db2.p[l][i] = gsum;
    return;
  }
  const int b = blockIdx.x - na;
  const int j = (b % col_tiles) * kDhCols + (threadIdx.x & 63), n0 = (b / col_tiles) * kDhRows;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int per = C >> 2, jv = min(j, C - 1);      // (C % 4 == 0: every wave has `per` rows; lanes past C read a valid column)
  const float* __restrict__ wl = w2.p[l];
  float acc[kDhRows];
#pragma unroll
  for (int r = 0; r < kDhRows; ++r) acc[r] = 0.f;
  for (int ib = 0; ib < per; ib += 64) {           // the same trip count in all four waves: the barriers are uniform
    const int cnt = min(64, per - ib), i0 = wave * per + ib;
    float wv[64];        // all 64 rows' loads leave before anything waits (W2 comes from HBM: a round trip per row otherwise)
#pragma unroll
    for (int ii = 0; ii < 64; ++ii) wv[ii] = wl[(size_t)(i0 + min(ii, cnt - 1)) * C + jv];
#pragma unroll
    for (int r = 0; r < kDhRows; ++r)
      gt[wave][r][lane] = (gl && lane < cnt && n0 + r < N) ? gl[(size_t)(n0 + r) * C + i0 + lane] : 0.f;
    __syncthreads();
#pragma unroll
    for (int ii = 0; ii < 64; ++ii)
      if (ii < cnt) {
#pragma unroll
        for (int r = 0; r < kDhRows; ++r) acc[r] += wv[ii] * gt[wave][r][ii];
      }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < kDhRows; ++r) red[wave][r][lane] = acc[r];
  __syncthreads();
  // 256 threads finish kDhRows x kDhCols = 512 elements: two each
  for (int e = threadIdx.x; e < kDhRows * kDhCols; e += 256) {
    const int r = e >> 6, c = e & 63, jj = (b % col_tiles) * kDhCols + c;
    if (n0 + r < N && jj < C) {
      const size_t at = (size_t)(n0 + r) * C + jj;
      const float v = (red[0][r][c] + red[1][r][c]) + (red[2][r][c] + red[3][r][c]);
      dh[(size_t)l * N * C + at] = hl[at] > 0.f ? v : 0.f;
    }
  }
}

// ---- B2.  blockIdx.x < na: dW1 / db1 of kW1Rows rows j of one level and 256 16-byte chunks along k: s[n][chunk] is held in
// registers (16 rows n at a time) while the rows j go by, n ascending for every output.  The others: one slice of the rows
// (l, j) of all levels for 256 columns k, one column per lane; the dh values of 64 rows at a time wait in the LDS (dt, NT = N
// rounded up to 8 / 16 / 32, zeros past N), the loop holds the loads of W1's rows and 16-byte broadcast reads.
constexpr int kW1Rows = 8;
template <int NT>
__global__ __launch_bounds__(256) void relation_scene_bwd_w1_kernel(const float* __restrict__ dh, const float* __restrict__ s,
                                                                    const SceneIn w1, const SceneOut dw1, const SceneOut db1,
                                                                    float* __restrict__ part, int N, int K, int C, int L, int na,
                                                                    int kblocks4, int row_tiles, int kblocks, int slice_rows) {
  if ((int)blockIdx.x < na) {
    int id = blockIdx.x;
    const int kb = id % kblocks4; id /= kblocks4;
    const int jt = id % row_tiles, l = id / row_tiles;
    const int j0 = jt * kW1Rows, kc = kb * 256 + threadIdx.x;
    const float* __restrict__ dl = dh + (size_t)l * N * C;
    if (kb == 0 && threadIdx.x < kW1Rows && j0 + (int)threadIdx.x < C) {
      float bsum = 0.f;
#pragma unroll
      for (int n = 0; n < NT; ++n)
        if (n < N) bsum += dl[(size_t)n * C + j0 + threadIdx.x];
      db1.p[l][j0 + threadIdx.x] = bsum;
    }
    if (kc >= (K >> 2)) return;
    f32x4 acc[kW1Rows];
#pragma unroll
    for (int r = 0; r < kW1Rows; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int nb = 0; nb < N; nb += 16) {
      f32x4 sv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        sv[u] = nb + u < N ? *reinterpret_cast<const f32x4*>(s + (size_t)(nb + u) * K + kc * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < kW1Rows; ++r)
        if (j0 + r < C) {
#pragma unroll
          for (int u = 0; u < 16; ++u)
            if (nb + u < N) {
              const float d = dl[(size_t)(nb + u) * C + j0 + r];
              acc[r].x += d * sv[u].x; acc[r].y += d * sv[u].y; acc[r].z += d * sv[u].z; acc[r].w += d * sv[u].w;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kW1Rows; ++r)
      if (j0 + r < C) *reinterpret_cast<f32x4*>(dw1.p[l] + (size_t)(j0 + r) * K + kc * 4) = acc[r];
    return;
  }
  const int b = blockIdx.x - na;
  __shared__ __attribute__((aligned(16))) float dt[64][NT];
  const int q = b / kblocks, k = (b - q * kblocks) * 256 + threadIdx.x, kv = min(k, K - 1);   // (lanes past K read a valid column)
  const int r0 = q * slice_rows, r1 = min(L * C, r0 + slice_rows);
  float acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = 0.f;
  for (int l = r0 / C; l <= (r1 - 1) / C; ++l) {        // the slice's rows, level by level, ascending
    const int ja = max(r0, l * C) - l * C, jb = min(r1, (l + 1) * C) - l * C;
    const float* __restrict__ wl = w1.p[l];
    const float* __restrict__ dl = dh + (size_t)l * N * C;
    for (int jc = ja; jc < jb; jc += 64) {
      const int cnt = min(64, jb - jc);
      for (int e = threadIdx.x; e < 64 * NT; e += 256) {
        const int rr = e & 63, n = e >> 6;
        dt[rr][n] = (rr < cnt && n < N) ? dl[(size_t)n * C + jc + rr] : 0.f;
      }
      __syncthreads();
      for (int rb = 0; rb < cnt; rb += 16) {     // sixteen rows' loads in flight (from a valid row past cnt), rows ascending
        float wv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) wv[u] = wl[(size_t)(jc + min(rb + u, cnt - 1)) * K + kv];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (rb + u < cnt) {
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] += wv[u] * dt[rb + u][n];
          }
      }
      __syncthreads();
    }
  }
  if (k < K) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
      if (n < N) part[((size_t)q * N + n) * K + k] = acc[n];
  }
}

// ---- B3.  ds = the slices' partials, summed in index order; one 16-byte chunk per thread
__global__ __launch_bounds__(256) void relation_scene_bwd_ds_kernel(const float* __restrict__ part, float* __restrict__ ds, int slices,
                                                                    size_t chunks) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  f32x4 acc = *reinterpret_cast<const f32x4*>(part + c * 4);
#pragma unroll 8
  for (int q = 1; q < slices; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + ((size_t)q * chunks + c) * 4);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *reinterpret_cast<f32x4*>(ds + c * 4) = acc;
}

// The reduction of ds runs over L * C weight rows of 4 K bytes each (1024 rows of 8 KB for FarSeg-R50).  It is cut into slices
// so that slices x ceil(K / 256) workgroups cover the 256 CUs, at most 64 of them (the partials are written and read once
// more: 64 x N x K floats at most); a function of the shapes alone, so the sums keep their order on every device.
struct ScenePlan {
  int slice_rows, slices, kblocks;
};
static ScenePlan scene_plan(int L, int K, int C) {
  ScenePlan p;
  p.kblocks = ceil_div(K, 256);
  const int rows = L * C;
  int want = ceil_div(256, p.kblocks);
  want = want > 64 ? 64 : want;
  want = want > rows ? rows : want;
  p.slice_rows = ceil_div(rows, want);
  p.slices = ceil_div(rows, p.slice_rows);
  return p;
}

static int scene_shape_ok(const char* what, int L, int N, int K, int C) {
  EVK_REQUIRE(L >= 1 && N >= 1 && K >= 1 && C >= 1, EVK_E_INVALID, "%s: L=%d N=%d K=%d C=%d", what, L, N, K, C);
  EVK_REQUIRE(L <= kSceneLevels, EVK_E_UNSUPPORTED, "%s: %d levels, at most %d are supported", what, L, kSceneLevels);
  EVK_REQUIRE(N <= kSmallM, EVK_E_UNSUPPORTED, "%s: %d rows, at most %d are supported", what, N, kSmallM);
  EVK_REQUIRE(K % 4 == 0 && C % 4 == 0, EVK_E_UNSUPPORTED, "%s: K=%d and C=%d must be multiples of 4", what, K, C);
  EVK_REQUIRE((long long)L * C * (K > C ? K : C) < 0x7fffffffLL, EVK_E_UNSUPPORTED, "%s: L=%d K=%d C=%d too large", what, L, K, C);
  return EVK_OK;
}

// every level's pointer present and on the 16-byte grid -> out; `optional`: a null entry is allowed (and kept)
template <typename S, typename T>
static bool scene_take(S& out, T* const* in, int L, bool optional = false) {
  if (!in) return false;
  for (int l = 0; l < kSceneLevels; ++l) {
    out.p[l] = l < L ? in[l] : nullptr;
    if (l < L && !(in[l] ? aligned16(in[l]) : optional)) return false;
  }
  return true;
}

}  // namespace evk

using namespace evk;

extern "C" int evk_relation_scene_fwd(const float* s, const float* const* w1, const float* const* b1, const float* const* w2,
                                      const float* const* b2, float* h, float* o, int32_t L, int32_t N, int32_t K, int32_t C,
                                      void* stream) {
  if (int rc = scene_shape_ok("relation_scene_fwd", L, N, K, C)) return rc;
  EVK_REQUIRE(b1 && b2, EVK_E_UNSUPPORTED, "relation_scene_fwd: convolutions without bias are not supported");
  for (int l = 0; l < L; ++l)
    EVK_REQUIRE(b1[l] && b2[l], EVK_E_UNSUPPORTED, "relation_scene_fwd: level %d has a convolution without bias", l);
  SceneIn W1, B1, W2, B2;
  EVK_REQUIRE(s && h && o && aligned16(s) && aligned16(h) && aligned16(o) && scene_take(W1, w1, L) && scene_take(B1, b1, L) &&
                  scene_take(W2, w2, L) && scene_take(B2, b2, L),
              EVK_E_INVALID, "relation_scene_fwd: null or misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(relation_scene_fwd_kernel, dim3(C, L), dim3(256), 0, st, s, (size_t)0, W1, B1, h, N, K, C, 1);
  if (int rc = check_launch("relation_scene_fwd (hidden)")) return rc;
  hipLaunchKernelGGL(relation_scene_fwd_kernel, dim3(C, L), dim3(256), 0, st, (const float*)h, (size_t)N * C, W2, B2, o, N, C, C, 0);
  return check_launch("relation_scene_fwd (output)");
}

extern "C" size_t evk_relation_scene_bwd_workspace_bytes(int32_t L, int32_t N, int32_t K, int32_t C) {
  if (L < 1 || N < 1 || K < 1 || C < 1) return 0;
  return (size_t)scene_plan(L, K, C).slices * N * K * sizeof(float);
}

extern "C" int evk_relation_scene_bwd(const float* s, const float* h, const float* const* g, const float* const* w1,
                                      const float* const* w2, float* dh, float* ds, float* const* dw1, float* const* db1,
                                      float* const* dw2, float* const* db2, int32_t L, int32_t N, int32_t K, int32_t C,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = scene_shape_ok("relation_scene_bwd", L, N, K, C)) return rc;
  SceneIn G, W1, W2;
  SceneOut DW1, DB1, DW2, DB2;
  EVK_REQUIRE(s && h && dh && ds && aligned16(s) && aligned16(h) && aligned16(dh) && aligned16(ds) && scene_take(G, g, L, true) &&
                  scene_take(W1, w1, L) && scene_take(W2, w2, L) && scene_take(DW1, dw1, L) && scene_take(DB1, db1, L) &&
                  scene_take(DW2, dw2, L) && scene_take(DB2, db2, L),
              EVK_E_INVALID, "relation_scene_bwd: null or misaligned pointer");
  const ScenePlan p = scene_plan(L, K, C);
  EVK_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= evk_relation_scene_bwd_workspace_bytes(L, N, K, C),
              EVK_E_WORKSPACE, "relation_scene_bwd: workspace of %zu bytes, %zu needed", workspace_bytes,
              evk_relation_scene_bwd_workspace_bytes(L, N, K, C));
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  {
    const int na = ceil_div((int64_t)C * (C / 4), 256), col_tiles = ceil_div(C, kDhCols), row_tiles = ceil_div(N, kDhRows);
    hipLaunchKernelGGL(relation_scene_bwd_w2_kernel, dim3(na + col_tiles * row_tiles, L), dim3(256), 0, st, G, h, W2, DW2, DB2, dh, N, C,
                       na, col_tiles);
    if (int rc = check_launch("relation_scene_bwd (w2)")) return rc;
  }
  {
    const int kblocks4 = ceil_div(K / 4, 256), row_tiles = ceil_div(C, kW1Rows);
    const int na = L * row_tiles * kblocks4;
    pick<8, 16, 32>(N <= 8 ? 8 : N <= 16 ? 16 : 32, [&](auto NT) {
      hipLaunchKernelGGL(relation_scene_bwd_w1_kernel<NT.value>, dim3(na + p.slices * p.kblocks), dim3(256), 0, st, (const float*)dh, s,
                         W1, DW1, DB1, part, N, K, C, L, na, kblocks4, row_tiles, p.kblocks, p.slice_rows);
      return 0;
    });
    if (int rc = check_launch("relation_scene_bwd (w1)")) return rc;
  }
  const size_t chunks = (size_t)N * K / 4;
  hipLaunchKernelGGL(relation_scene_bwd_ds_kernel, dim3(ceil_div((int64_t)chunks, 256)), dim3(256), 0, st, (const float*)part, ds, p.slices,
                     chunks);
  return check_launch("relation_scene_bwd (ds)");
}
