// Multi-head self-attention with axial RoPE on Q and K, forward and backward, on the exact fp32 MFMA of gfx950 — the one
// hot path of a DINOv3 ViT block (reference ever/module/dinov3/layers/attention.py:16-27 rope_apply, :66-85 apply_rope,
// :106-118 compute_attention).
//
// Operands as they lie in memory: qkv [B][N][3][H][D] is the QKV Linear's output, o [B][N][H*D] what the projection Linear
// takes; the reference's reshape / unbind / transpose / transpose back / reshape are index arithmetic here.  RoPE is applied
// while a Q or K element is loaded: the first `prefix` tokens are left alone, token n >= prefix takes row n - prefix of the
// [N - prefix][D] sin / cos tables, y = x cos + rotate_half(x) sin with rotate_half([x1, x2]) = [-x2, x1].  V is not rotated.
//
// One shape of work in all three kernels (Tq = Tk = 64, four waves, a wave owns 16 rows of its workgroup's tile):
//   * the OWNED rows (queries in attn_fwd / attn_bwd_dq, keys in attn_bwd_dkv) sit in registers as the B operand of
//     v_mfma_f32_16x16x4_f32: lane (c = lane & 15, g = lane >> 4) holds element d = 4 kk + g of row c for kk < D / 4;
//   * the WALKED rows come through LDS in 64-row tiles with a row stride of D + 4 floats, which makes both read patterns
//     (16 rows x 4 consecutive floats, and 4 x 4 rows x 16 consecutive floats) conflict-free;
//   * the first product is taken TRANSPOSED with respect to the owned rows (walked row on the C/D row index, owned row on
//     the lane), so its C/D registers — walked row 16 t + 4 g + r in s[t][r] — ARE the B operand of the second product,
//     which sums over the walked rows: k-step (t, r) of that product covers walked rows 16 t + 4 g' + r for g' = 0..3 and its
//     A operand is read from LDS in the same permuted order.  No LDS round trip for P and no lane movement; the softmax
//     statistics of an owned row reduce over 16 registers and two shuffles (xor 16, 32) with all 64 lanes busy.
// Forward: online softmax over the key tiles.  The running maximum starts at -inf; every key tile holds at least one real
//   key, so the new maximum is finite and exp(-inf - m) = 0 handles the first tile, a lone key in the last tile and the padded
//   key columns, whose logits are set to -inf and whose K / V rows are zero-filled in LDS, never read from memory.  The
//   accumulator is rescaled on every trip (no threshold, no branch).  lse = m + log(l) is written when asked for.
// Backward: two owners, no float atomics, same bits every run.  attn_delta_kernel writes delta[b][n][h] = sum_d do o into the
//   caller's workspace; attn_bwd_dkv_kernel owns a key tile and walks the query tiles for dK and dV, attn_bwd_dq_kernel owns
//   a query tile and walks the key tiles for dQ; both recompute P = exp(scale S - lse).  The gradient leaves through the
//   adjoint of the rotation, dx = dy cos + rotate_half^T(dy sin) with rotate_half^T([g1, g2]) = [g2, -g1], valid for any
//   sin / cos tables; the partner element d ^ (D / 2) lives in the same lane (accumulator tile dt ^ (D / 32)).
// Plain fp32 under every conv-math mode; every element offset is 64-bit.
#include "common.hpp"
#include <math.h>

namespace evk {

constexpr int kAttnTile = 64;       // queries per workgroup == keys per trip
constexpr int kAttnThreads = 256;

__device__ __forceinline__ f32x4 attn_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void attn_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

struct AttnDims {
  int N, H, prefix;
  const float* sin;   // [N - prefix][D] or null: no RoPE
  const float* cos;
};

// Rows n0 .. n0 + 63 of one (batch, head) slab to LDS [64][D + 4]: `src` points at row 0 of the slab, rows are `stride`
// floats apart.  Rows at or past N are zero-filled without a read.  rot: apply RoPE (Q and K).
template <int D>
__device__ __forceinline__ void attn_stage(float* __restrict__ dst, const float* __restrict__ src, int64_t stride, int n0,
                                           const AttnDims& a, bool rot) {
  constexpr int LS = D + 4, C4 = D / 4;
  for (int i = threadIdx.x; i < kAttnTile * C4; i += kAttnThreads) {
    const int row = i / C4, d = (i % C4) * 4;
    const int n = n0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (n < a.N) {
      const float* p = src + (int64_t)n * stride;
      v = attn_ld4(p + d);
      if (rot && n >= a.prefix) {
        const f32x4 w = attn_ld4(p + (d ^ (D / 2)));
        const int64_t t = (int64_t)(n - a.prefix) * D + d;
        const f32x4 sn = attn_ld4(a.sin + t), cs = attn_ld4(a.cos + t);
        v = v * cs + (d < D / 2 ? -w : w) * sn;
      }
    }
    attn_st4(dst + row * LS + d, v);
  }
}

// Row n of a slab into the B-operand registers of lane (c, g): element 4 kk + g in reg[kk]; zero past N.
template <int D>
__device__ __forceinline__ void attn_own_row(float (&reg)[D / 4], const float* __restrict__ src, int64_t stride, int n, int g,
                                             const AttnDims& a, bool rot) {
#pragma unroll
  for (int kk = 0; kk < D / 4; ++kk) reg[kk] = 0.f;
  if (n >= a.N) return;
  const float* p = src + (int64_t)n * stride;
  const bool r = rot && n >= a.prefix;
  const int64_t t = r ? (int64_t)(n - a.prefix) * D : 0;
#pragma unroll
  for (int kk = 0; kk < D / 4; ++kk) {
    const int d = 4 * kk + g;
    float x = p[d];
    if (r) {
      const float w = p[d ^ (D / 2)];
      x = x * a.cos[t + d] + (d < D / 2 ? -w : w) * a.sin[t + d];
    }
    reg[kk] = x;
  }
}

// acc[t] (t = 0..3) += LDS rows 16 t + c (A operand, element 4 kk + g) times own[kk] (B operand): the transposed product,
// walked row 16 t + 4 g + r of owned row c in acc[t][r].
template <int D>
__device__ __forceinline__ void attn_mma_walk(f32x4 (&acc)[4], const float* __restrict__ tile, const float (&own)[D / 4], int c,
                                              int g) {
  constexpr int LS = D + 4;
#pragma unroll
  for (int kk = 0; kk < D / 4; ++kk)
#pragma unroll
    for (int t = 0; t < 4; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[(16 * t + c) * LS + 4 * kk + g], own[kk], acc[t], 0, 0, 0);
}

// out[dt] (dt < D / 16) += sum over the 64 walked rows of tile[row][16 dt + c] * w[t][r] — w in the C/D layout of
// attn_mma_walk, rows taken in its permuted order.  Element d = 16 dt + 4 g + r of owned row c lands in out[dt][r].
template <int D>
__device__ __forceinline__ void attn_mma_fold(f32x4 (&out)[D / 16], const float* __restrict__ tile, const f32x4 (&w)[4], int c,
                                              int g) {
  constexpr int LS = D + 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
        out[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[(16 * t + 4 * g + r) * LS + 16 * dt + c], w[t][r], out[dt], 0, 0, 0);
}

__device__ __forceinline__ float attn_max4(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float attn_sum4(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// The gradient of a rotated row back through the rotation and out: gr[dt][r] is element 16 dt + 4 g + r of token n.
template <int D>
__device__ __forceinline__ void attn_store_grad(float* __restrict__ dst, f32x4 (&gr)[D / 16], int n, int g, const AttnDims& a,
                                                bool rot) {
  constexpr int DT = D / 16;
  if (rot && n >= a.prefix) {
    const int64_t t = (int64_t)(n - a.prefix) * D;
    f32x4 gs[DT], out[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) gs[dt] = gr[dt] * attn_ld4(a.sin + t + 16 * dt + 4 * g);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const f32x4 cs = attn_ld4(a.cos + t + 16 * dt + 4 * g);
      const f32x4 w = gs[dt ^ (DT / 2)];
      out[dt] = gr[dt] * cs + (dt < DT / 2 ? w : -w);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) attn_st4(dst + 16 * dt + 4 * g, out[dt]);
  } else {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) attn_st4(dst + 16 * dt + 4 * g, gr[dt]);
  }
}

template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                                float* __restrict__ lse, AttnDims a, int tiles, float scale) {
  constexpr int LS = D + 4, DT = D / 16;
  __shared__ __attribute__((aligned(16))) float Ks[kAttnTile * LS];
  __shared__ __attribute__((aligned(16))) float Vs[kAttnTile * LS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int qt = blockIdx.x % tiles, bh = blockIdx.x / tiles, h = bh % a.H, b = bh / a.H;
  const int64_t hd = (int64_t)a.H * D, stride = 3 * hd;
  const float* slab = qkv + (int64_t)b * a.N * stride + (int64_t)h * D;   // q of token 0; k at + hd, v at + 2 hd
  const bool rot = a.sin != nullptr;
  const int q = qt * kAttnTile + wave * 16 + c;
  float qr[D / 4];
  attn_own_row<D>(qr, slab, stride, q, g, a, rot);
  float m = -INFINITY, l = 0.f;
  f32x4 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < tiles; ++kt) {
    __syncthreads();
    attn_stage<D>(Ks, slab + hd, stride, kt * kAttnTile, a, rot);
    attn_stage<D>(Vs, slab + 2 * hd, stride, kt * kAttnTile, a, false);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    attn_mma_walk<D>(s, Ks, qr, c, g);
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * kAttnTile + 16 * t + 4 * g + r;
        s[t][r] = key < a.N ? s[t][r] * scale : -INFINITY;
        mx = fmaxf(mx, s[t][r]);
      }
    const float mn = fmaxf(m, attn_max4(mx));    // finite: every tile has a real key
    const float alpha = expf(m - mn);            // 0 on the first trip
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = expf(s[t][r] - mn);
        ps += s[t][r];
      }
    l = l * alpha + attn_sum4(ps);
    m = mn;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] *= alpha;
    attn_mma_fold<D>(acc, Vs, s, c, g);
  }
  if (q >= a.N) return;
  float* orow = o + ((int64_t)b * a.N + q) * hd + (int64_t)h * D;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) attn_st4(orow + 16 * dt + 4 * g, acc[dt] / l);
  if (lse && g == 0) lse[((int64_t)b * a.H + h) * a.N + q] = m + logf(l);
}

// delta[i] = sum_d do[i][d] o[i][d] over the rows i = (b N + n) H + h of the [B N H][D] view of o
template <int D>
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ o, const float* __restrict__ go,
                                                         float* __restrict__ delta, int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int d = 0; d < D; d += 4) s += attn_ld4(o + i * D + d) * attn_ld4(go + i * D + d);
  delta[i] = (s[0] + s[1]) + (s[2] + s[3]);
}

template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ go,
                                                                    const float* __restrict__ lse, const float* __restrict__ delta,
                                                                    float* __restrict__ dqkv, AttnDims a, int tiles, float scale) {
  constexpr int LS = D + 4, DT = D / 16;
  __shared__ __attribute__((aligned(16))) float Qs[kAttnTile * LS];
  __shared__ __attribute__((aligned(16))) float Gs[kAttnTile * LS];
  __shared__ __attribute__((aligned(16))) float Ls[kAttnTile];
  __shared__ __attribute__((aligned(16))) float Es[kAttnTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int kt = blockIdx.x % tiles, bh = blockIdx.x / tiles, h = bh % a.H, b = bh / a.H;
  const int64_t hd = (int64_t)a.H * D, stride = 3 * hd;
  const float* slab = qkv + (int64_t)b * a.N * stride + (int64_t)h * D;
  const float* gslab = go + (int64_t)b * a.N * hd + (int64_t)h * D;
  const bool rot = a.sin != nullptr;
  const int key = kt * kAttnTile + wave * 16 + c;
  float kr[D / 4], vr[D / 4];
  attn_own_row<D>(kr, slab + hd, stride, key, g, a, rot);
  attn_own_row<D>(vr, slab + 2 * hd, stride, key, g, a, false);
  f32x4 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int qt = 0; qt < tiles; ++qt) {
    __syncthreads();
    attn_stage<D>(Qs, slab, stride, qt * kAttnTile, a, rot);
    attn_stage<D>(Gs, gslab, hd, qt * kAttnTile, a, false);
    if (threadIdx.x < kAttnTile) {
      const int q = qt * kAttnTile + threadIdx.x;
      // a padded query: P = exp(0 - inf) = 0 and dS = 0 (delta - 0)
      Ls[threadIdx.x] = q < a.N ? lse[((int64_t)b * a.H + h) * a.N + q] : INFINITY;
      Es[threadIdx.x] = q < a.N ? delta[((int64_t)b * a.N + q) * a.H + h] : 0.f;
    }
    __syncthreads();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    attn_mma_walk<D>(s, Qs, kr, c, g);
    attn_mma_walk<D>(dp, Gs, vr, c, g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 lq = attn_ld4(Ls + 16 * t + 4 * g), eq = attn_ld4(Es + 16 * t + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = expf(s[t][r] * scale - lq[r]);
        dp[t][r] = s[t][r] * (dp[t][r] - eq[r]);
      }
    }
    attn_mma_fold<D>(dv, Gs, s, c, g);
    attn_mma_fold<D>(dk, Qs, dp, c, g);
  }
  if (key >= a.N) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] *= scale;
  float* drow = dqkv + ((int64_t)b * a.N + key) * stride + (int64_t)h * D;
  attn_store_grad<D>(drow + hd, dk, key, g, a, rot);
  attn_store_grad<D>(drow + 2 * hd, dv, key, g, a, false);
}

template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ go,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   float* __restrict__ dqkv, AttnDims a, int tiles, float scale) {
  constexpr int LS = D + 4, DT = D / 16;
  __shared__ __attribute__((aligned(16))) float Ks[kAttnTile * LS];
  __shared__ __attribute__((aligned(16))) float Vs[kAttnTile * LS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int qt = blockIdx.x % tiles, bh = blockIdx.x / tiles, h = bh % a.H, b = bh / a.H;
  const int64_t hd = (int64_t)a.H * D, stride = 3 * hd;
  const float* slab = qkv + (int64_t)b * a.N * stride + (int64_t)h * D;
  const float* gslab = go + (int64_t)b * a.N * hd + (int64_t)h * D;
  const bool rot = a.sin != nullptr;
  const int q = qt * kAttnTile + wave * 16 + c;
  float qr[D / 4], gr[D / 4];
  attn_own_row<D>(qr, slab, stride, q, g, a, rot);
  attn_own_row<D>(gr, gslab, hd, q, g, a, false);
  const float lq = q < a.N ? lse[((int64_t)b * a.H + h) * a.N + q] : INFINITY;
  const float eq = q < a.N ? delta[((int64_t)b * a.N + q) * a.H + h] : 0.f;
  f32x4 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < tiles; ++kt) {
    __syncthreads();
    attn_stage<D>(Ks, slab + hd, stride, kt * kAttnTile, a, rot);
    attn_stage<D>(Vs, slab + 2 * hd, stride, kt * kAttnTile, a, false);
    __syncthreads();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    attn_mma_walk<D>(s, Ks, qr, c, g);
    attn_mma_walk<D>(dp, Vs, gr, c, g);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * kAttnTile + 16 * t + 4 * g + r;
        const float p = key < a.N ? expf(s[t][r] * scale - lq) : 0.f;
        dp[t][r] = p * (dp[t][r] - eq);
      }
    attn_mma_fold<D>(dq, Ks, dp, c, g);
  }
  if (q >= a.N) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] *= scale;
  attn_store_grad<D>(dqkv + ((int64_t)b * a.N + q) * stride + (int64_t)h * D, dq, q, g, a, rot);
}


// what every entry point refuses, before a launch
static int attn_shape_check(const char* what, int32_t B, int32_t N, int32_t H, int32_t D, int32_t prefix) {
  EVK_REQUIRE(B >= 1 && H >= 1, EVK_E_INVALID, "%s: B = %d, H = %d: at least one sample and one head", what, B, H);
  EVK_REQUIRE(N >= 1, EVK_E_INVALID, "%s: N = %d: at least one token", what, N);
  EVK_REQUIRE(prefix >= 0 && prefix <= N, EVK_E_INVALID, "%s: prefix = %d outside 0..N = %d", what, prefix, N);
  EVK_REQUIRE(D >= 1 && ((int64_t)H * D) % 4 == 0, EVK_E_INVALID, "%s: H * D = %lld is not a multiple of 4", what,
              (long long)H * D);
  EVK_REQUIRE(D == 32 || D == 64, EVK_E_UNSUPPORTED, "%s: head dimension %d: only 32 and 64 have kernels", what, D);
  const int64_t grid = (int64_t)B * H * ceil_div(N, kAttnTile);
  EVK_REQUIRE(grid <= 0x7fffffff, EVK_E_UNSUPPORTED, "%s: %lld workgroups", what, (long long)grid);
  return EVK_OK;
}

static int attn_rope_check(const char* what, const float* sin, const float* cos) {
  EVK_REQUIRE((sin == nullptr) == (cos == nullptr), EVK_E_INVALID, "%s: sin and cos come together or not at all", what);
  EVK_REQUIRE(aligned16(sin) && aligned16(cos), EVK_E_INVALID, "%s: sin and cos must be 16-byte aligned", what);
  return EVK_OK;
}

}  // namespace evk

using namespace evk;

extern "C" int evk_attn_plan(int32_t B, int32_t N, int32_t H, int32_t D, int32_t prefix, int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "attn_plan: null pointer");
  int rc = attn_shape_check("attn_plan", B, N, H, D, prefix);
  if (rc) return rc;
  const int tiles = ceil_div(N, kAttnTile);
  out[0] = kAttnTile;                                   // query tile
  out[1] = kAttnTile;                                   // key tile
  out[2] = tiles;                                       // key trips of a query tile (query trips of a key tile)
  out[3] = B * H * tiles;                               // workgroups of each of the three tiled kernels
  out[4] = 2 * kAttnTile * (D + 4) * (int)sizeof(float);  // LDS bytes, forward and dQ
  out[5] = out[4] + 2 * kAttnTile * (int)sizeof(float);   // LDS bytes, dK / dV
  return EVK_OK;
}

extern "C" int evk_attn_fwd(const float* qkv, const float* sin, const float* cos, float* o, float* lse, int32_t B, int32_t N,
                            int32_t H, int32_t D, int32_t prefix, void* stream) {
  int rc = attn_shape_check("attn_fwd", B, N, H, D, prefix);
  if (rc) return rc;
  EVK_REQUIRE(qkv && o, EVK_E_INVALID, "attn_fwd: null pointer");
  if ((rc = attn_rope_check("attn_fwd", sin, cos))) return rc;
  EVK_REQUIRE(aligned16(qkv) && aligned16(o), EVK_E_INVALID, "attn_fwd: qkv and o must be 16-byte aligned");
  const int tiles = ceil_div(N, kAttnTile);
  const AttnDims a{N, H, prefix, prefix < N ? sin : nullptr, prefix < N ? cos : nullptr};
  const float scale = (float)(1.0 / sqrt((double)D));
  hipStream_t st = (hipStream_t)stream;
  pick<32, 64>(D, [&](auto DD) {
    hipLaunchKernelGGL(attn_fwd_kernel<decltype(DD)::value>, dim3((unsigned)(B * H * tiles)), dim3(kAttnThreads), 0, st, qkv, o,
                       lse, a, tiles, scale);
    return 0;
  });
  return check_launch("attn_fwd");
}

extern "C" size_t evk_attn_bwd_workspace_bytes(int32_t B, int32_t N, int32_t H, int32_t D) {
  if (B < 1 || N < 1 || H < 1 || (D != 32 && D != 64)) return 0;
  return (size_t)B * N * H * sizeof(float);
}

extern "C" int evk_attn_bwd(const float* qkv, const float* sin, const float* cos, const float* o, const float* d_o,
                            const float* lse, float* dqkv, int32_t B, int32_t N, int32_t H, int32_t D, int32_t prefix,
                            void* workspace, size_t workspace_bytes, void* stream) {
  int rc = attn_shape_check("attn_bwd", B, N, H, D, prefix);
  if (rc) return rc;
  if (!dqkv) return EVK_OK;   // nothing asked for
  EVK_REQUIRE(qkv && o && d_o && lse, EVK_E_INVALID, "attn_bwd: null pointer");
  if ((rc = attn_rope_check("attn_bwd", sin, cos))) return rc;
  EVK_REQUIRE(aligned16(qkv) && aligned16(o) && aligned16(d_o) && aligned16(dqkv) && aligned16(workspace),
              EVK_E_INVALID, "attn_bwd: qkv, o, do, dqkv and the workspace must be 16-byte aligned");
  const size_t need = evk_attn_bwd_workspace_bytes(B, N, H, D);
  EVK_REQUIRE(workspace && workspace_bytes >= need, EVK_E_WORKSPACE, "attn_bwd: workspace of %zu bytes, %zu needed",
              workspace_bytes, need);
  const int tiles = ceil_div(N, kAttnTile);
  const AttnDims a{N, H, prefix, prefix < N ? sin : nullptr, prefix < N ? cos : nullptr};
  const float scale = (float)(1.0 / sqrt((double)D));
  float* delta = reinterpret_cast<float*>(workspace);
  const int64_t rows = (int64_t)B * N * H;
  hipStream_t st = (hipStream_t)stream;
  pick<32, 64>(D, [&](auto DD) {
    constexpr int DV = decltype(DD)::value;
    hipLaunchKernelGGL(attn_delta_kernel<DV>, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, o, d_o, delta, rows);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<DV>, dim3((unsigned)(B * H * tiles)), dim3(kAttnThreads), 0, st, qkv, d_o, lse, delta,
                       dqkv, a, tiles, scale);
    hipLaunchKernelGGL(attn_bwd_dq_kernel<DV>, dim3((unsigned)(B * H * tiles)), dim3(kAttnThreads), 0, st, qkv, d_o, lse, delta,
                       dqkv, a, tiles, scale);
    return 0;
  });
  return check_launch("attn_bwd");
}
