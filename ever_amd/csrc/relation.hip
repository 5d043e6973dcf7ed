// FS-Relation on NHWC fp32 (gfx950): out = sigmoid(<scene, content>) * feat, plain and with the two BatchNorm + ReLU passes
// that produce content and feat inside the kernels.  Reference call sites are cited per entry point in include/ever_hip.h.
// 16-byte accesses along the channel axis (C % 4 == 0).
#include "stream_common.hpp"

namespace evk {

// ---- With BN, the two BatchNorm + ReLU passes run inside (reference fs_relation.py:39-53,61-71: content / re-encoding =
// ReLU(BN(conv1x1(p))), out = sigmoid(<scene, content>) * re-encoded).  The separate passes wrote the two normalised
// 256-channel maps only for this kernel to read them back, and their backward re-read both pairs (g, z) just to form the
// per-channel sums: here the forward reads the convolution outputs z and applies scale / shift / ReLU on the fly, the
// backward rebuilds both activations from z, writes the MASKED gradients g and leaves the BatchNorm partial sums
// (sum g, sum g * xhat, max|g|, max|xhat| per workgroup and channel) for evk_bn_bwd_from_partials.
__device__ __forceinline__ f32x4 bn_relu4(const f32x4 z, const f32x4 sc, const f32x4 sh) {
  f32x4 y = z * sc + sh;
  y.x = fmaxf(y.x, 0.f); y.y = fmaxf(y.y, 0.f); y.z = fmaxf(y.z, 0.f); y.w = fmaxf(y.w, 0.f);
  return y;
}
// channel chunk cb of a pixel's activation: the map itself, or with BN ReLU(z * scale + shift) of ss = [scale | shift][C]
template <bool BN>
__device__ __forceinline__ f32x4 relation_act(const float* __restrict__ z, const float* __restrict__ ss, int C, int cb) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(z + cb * 4);
  if (!BN) return v;
  return bn_relu4(v, *reinterpret_cast<const f32x4*>(ss + cb * 4), *reinterpret_cast<const f32x4*>(ss + C + cb * 4));
}
// One wave per pixel; lanes stride the channel axis in 16-byte chunks.  The plain form takes content and feat as zc and zf
// (ssc, ssf, amax unused) and commits no max|out|.
template <bool BN>
__global__ __launch_bounds__(256) void relation_fwd_kernel(const float* __restrict__ scene, const float* __restrict__ zc,
                                                           const float* __restrict__ ssc, const float* __restrict__ zf,
                                                           const float* __restrict__ ssf, float* __restrict__ out,
                                                           float* __restrict__ r, int N, int HW, int C,
                                                           uint32_t* __restrict__ amax) {
  const int c4 = C >> 2;
  const int lane = threadIdx.x & 63;
  const size_t npix = (size_t)N * HW;
  const size_t wstride = (size_t)gridDim.x * 4;
  uint32_t m = 0;
  for (size_t pix = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); pix < npix; pix += wstride) {
    const size_t n = pix / HW;
    const float* sc = scene + n * C;
    const float* ct = zc + pix * C;
    float dot = 0.f;
    for (int cb = lane; cb < c4; cb += 64) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(sc + cb * 4);
      const f32x4 b = relation_act<BN>(ct, ssc, C, cb);
      dot += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    dot = wave_sum(dot);
    const float rv = 1.f / (1.f + expf(-dot));
    if (lane == 0) r[pix] = rv;
    const float* ft = zf + pix * C;
    float* o = out + pix * C;
    for (int cb = lane; cb < c4; cb += 64) {
      const f32x4 v = relation_act<BN>(ft, ssf, C, cb) * rv;
      *reinterpret_cast<f32x4*>(o + cb * 4) = v;
      if (BN) m = abs4_bits(m, v);
    }
  }
  if (BN && amax) commit_absmax(amax, m);
}

// backward: dfeat = r*dout ; dz = (sum_c dout*feat) * r*(1-r) ; dcontent = dz*scene ;
// partial dscene[blk][n?]: each workgroup owns a pixel range inside ONE image n and accumulates
// sum_p dz*content into partial[n][blk][C].
__global__ __launch_bounds__(256) void relation_bwd_kernel(const float* __restrict__ dout,
                                                           const float* __restrict__ scene,
                                                           const float* __restrict__ content,
                                                           const float* __restrict__ feat, const float* __restrict__ r,
                                                           float* __restrict__ dcontent, float* __restrict__ dfeat,
                                                           float* __restrict__ partial, int HW, int C, int pix_per_blk,
                                                           int nblk) {
  extern __shared__ __attribute__((aligned(16))) float sacc[];  // [4 waves][C]
  const int c4 = C >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y;
  const int p0 = blockIdx.x * pix_per_blk, p1 = min(HW, p0 + pix_per_blk);
  const float* sc = scene + (size_t)n * C;
  float* myacc = sacc + wave * C;
  for (int c = lane; c < C; c += 64) myacc[c] = 0.f;
  for (int p = p0 + wave; p < p1; p += 4) {
    const size_t pix = (size_t)n * HW + p;
    const float rv = r[pix];
    const float* d_o = dout + pix * C;
    const float* ft = feat + pix * C;
    const float* ct = content + pix * C;
    float dot = 0.f;
    for (int cb = lane; cb < c4; cb += 64) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(d_o + cb * 4);
      const f32x4 b = *reinterpret_cast<const f32x4*>(ft + cb * 4);
      dot += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
      *reinterpret_cast<f32x4*>(dfeat + pix * C + cb * 4) = a * rv;
    }
    dot = wave_sum(dot);
    const float dz = dot * rv * (1.f - rv);
    for (int cb = lane; cb < c4; cb += 64) {
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(sc + cb * 4);
      const f32x4 c4v = *reinterpret_cast<const f32x4*>(ct + cb * 4);
      *reinterpret_cast<f32x4*>(dcontent + pix * C + cb * 4) = s4 * dz;
      f32x4* a = reinterpret_cast<f32x4*>(myacc + cb * 4);
      *a = *a + c4v * dz;
    }
  }
  __syncthreads();
  float* o = partial + ((size_t)n * nblk + blockIdx.x) * C;
  for (int c = threadIdx.x; c < C; c += 256) o[c] = (sacc[c] + sacc[C + c]) + (sacc[2 * C + c] + sacc[3 * C + c]);
}
// 8 channels x 32 partial-lanes per workgroup (fixed fold order), as the other finalisations: a serial walk over up to
// 256 partials per thread was 32 us of latency per call
__global__ __launch_bounds__(256) void relation_dscene_final_kernel(const float* __restrict__ partial,
                                                                    float* __restrict__ dscene, int nblk, int C) {
  __shared__ double red[32][8];
  const int tc = threadIdx.x & 7, tl = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + tc;
  const int n = blockIdx.y;
  double s = 0.0;
  if (c < C)
    for (int b = tl; b < nblk; b += 32) s += (double)partial[((size_t)n * nblk + b) * C + c];
  red[tl][tc] = s;
  __syncthreads();
  if (tl == 0 && c < C) {
    for (int k = 1; k < 32; ++k) s += red[k][tc];
    dscene[(size_t)n * C + c] = (float)s;
  }
}

// Per-lane REGISTER accumulators over a workgroup's pixels (a lane owns NCH 16-byte channel chunks): the scene gradient,
// then per BatchNorm (content, re-encoding) sum g, sum g*xhat, max|g|, max|xhat|; the four waves are folded through LDS once,
// at the end ([4 waves][9][C] floats).  (Accumulating in LDS per pixel — nine dependent read-modify-writes — made this
// kernel slower than the plain relation backward it replaces.)
template <int NCH>
__global__ __launch_bounds__(256) void relation_bn_bwd_kernel(
    const float* __restrict__ dout, const float* __restrict__ scene, const float* __restrict__ zc,
    const float* __restrict__ ssc, const float* __restrict__ mic, const float* __restrict__ zf, const float* __restrict__ ssf,
    const float* __restrict__ mif, const float* __restrict__ r, float* __restrict__ gc, float* __restrict__ gf,
    float* __restrict__ partial, float* __restrict__ bnp_c, float* __restrict__ bnm_c, float* __restrict__ bnp_f,
    float* __restrict__ bnm_f, int HW, int C, int pix_per_blk, int nblk) {
  extern __shared__ __attribute__((aligned(16))) float sacc[];
  const int c4 = C >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y;
  const int p0 = blockIdx.x * pix_per_blk, p1 = min(HW, p0 + pix_per_blk);
  const float* sc = scene + (size_t)n * C;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[NCH][9];
  f32x4 s4[NCH], scc[NCH], shc[NCH], muc[NCH], isc[NCH], scf[NCH], shf[NCH], muf[NCH], isf[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int cb = lane + 64 * j;
    const bool ok = cb < c4;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[j][k] = zero4;
    s4[j] = ok ? *reinterpret_cast<const f32x4*>(sc + cb * 4) : zero4;
    scc[j] = ok ? *reinterpret_cast<const f32x4*>(ssc + cb * 4) : zero4;
    shc[j] = ok ? *reinterpret_cast<const f32x4*>(ssc + C + cb * 4) : zero4;
    muc[j] = ok ? *reinterpret_cast<const f32x4*>(mic + cb * 4) : zero4;
    isc[j] = ok ? *reinterpret_cast<const f32x4*>(mic + C + cb * 4) : zero4;
    scf[j] = ok ? *reinterpret_cast<const f32x4*>(ssf + cb * 4) : zero4;
    shf[j] = ok ? *reinterpret_cast<const f32x4*>(ssf + C + cb * 4) : zero4;
    muf[j] = ok ? *reinterpret_cast<const f32x4*>(mif + cb * 4) : zero4;
    isf[j] = ok ? *reinterpret_cast<const f32x4*>(mif + C + cb * 4) : zero4;
  }
  auto amax4 = [](f32x4& m, const f32x4 v) {
    m.x = fmaxf(m.x, fabsf(v.x)); m.y = fmaxf(m.y, fabsf(v.y)); m.z = fmaxf(m.z, fabsf(v.z)); m.w = fmaxf(m.w, fabsf(v.w));
  };
  for (int p = p0 + wave; p < p1; p += 4) {
    const size_t pix = (size_t)n * HW + p;
    const float rv = r[pix];
    f32x4 a[NCH], zfv[NCH], zcv[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {     // all three rows of the pixel in flight before the first use
      const int cb = lane + 64 * j;
      const bool ok = cb < c4;
      a[j] = ok ? *reinterpret_cast<const f32x4*>(dout + pix * C + cb * 4) : zero4;
      zfv[j] = ok ? *reinterpret_cast<const f32x4*>(zf + pix * C + cb * 4) : zero4;
      zcv[j] = ok ? *reinterpret_cast<const f32x4*>(zc + pix * C + cb * 4) : zero4;
    }
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {     // re-encoding branch: g_f = dout * r where the activation is positive
      const int cb = lane + 64 * j;
      const f32x4 y = bn_relu4(zfv[j], scf[j], shf[j]);
      dot += a[j].x * y.x + a[j].y * y.y + a[j].z * y.z + a[j].w * y.w;
      f32x4 g = a[j] * rv;
      g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f; g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
      if (cb < c4) *reinterpret_cast<f32x4*>(gf + pix * C + cb * 4) = g;
      const f32x4 xh = (zfv[j] - muf[j]) * isf[j];
      acc[j][5] += g;
      acc[j][6] += g * xh;
      amax4(acc[j][7], g);
      amax4(acc[j][8], xh);
    }
    dot = wave_sum(dot);
    const float dz = dot * rv * (1.f - rv);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {     // content branch: g_c = dz * scene where the activation is positive
      const int cb = lane + 64 * j;
      const f32x4 y = bn_relu4(zcv[j], scc[j], shc[j]);
      f32x4 g = s4[j] * dz;
      g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f; g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
      if (cb < c4) *reinterpret_cast<f32x4*>(gc + pix * C + cb * 4) = g;
      acc[j][0] += y * dz;
      const f32x4 xh = (zcv[j] - muc[j]) * isc[j];
      acc[j][1] += g;
      acc[j][2] += g * xh;
      amax4(acc[j][3], g);
      amax4(acc[j][4], xh);
    }
  }
  float* my = sacc + (size_t)wave * 9 * C;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int cb = lane + 64 * j;
    if (cb < c4)
#pragma unroll
      for (int k = 0; k < 9; ++k) *reinterpret_cast<f32x4*>(my + (size_t)k * C + cb * 4) = acc[j][k];
  }
  __syncthreads();
  const size_t blk = (size_t)n * nblk + blockIdx.x;
  const size_t W9 = (size_t)9 * C;
  for (int c = threadIdx.x; c < C; c += 256) {
    auto fold = [&](int k) { return (sacc[k * C + c] + sacc[W9 + k * C + c]) + (sacc[2 * W9 + k * C + c] + sacc[3 * W9 + k * C + c]); };
    auto fmx = [&](int k) {
      return fmaxf(fmaxf(sacc[k * C + c], sacc[W9 + k * C + c]), fmaxf(sacc[2 * W9 + k * C + c], sacc[3 * W9 + k * C + c]));
    };
    partial[blk * C + c] = fold(0);
    bnp_c[blk * 2 * C + c] = fold(1);
    bnp_c[blk * 2 * C + C + c] = fold(2);
    bnm_c[blk * 2 * C + c] = fmx(3);
    bnm_c[blk * 2 * C + C + c] = fmx(4);
    bnp_f[blk * 2 * C + c] = fold(5);
    bnp_f[blk * 2 * C + C + c] = fold(6);
    bnm_f[blk * 2 * C + c] = fmx(7);
    bnm_f[blk * 2 * C + C + c] = fmx(8);
  }
}

static int relation_blocks(int HW) {
  // pixels per workgroup and the cap on workgroups per image (swept in the step in round 5: level)
  constexpr int ppb = 64, cap = 256;
  int b = (HW + ppb - 1) / ppb;
  return b > cap ? cap : (b < 1 ? 1 : b);
}

// what the two backward entry points share: the split of an image's pixels over nblk workgroups of ppb pixels each — launch(nblk,
// ppb) is the caller's own kernel, which leaves its scene-gradient partials [N * nblk][C] in `partial` — and their fold
template <typename F>
static int relation_bwd_launch(const char* what, const float* partial, float* dscene, int N, int HW, int C, hipStream_t st,
                               F&& launch) {
  const int nblk = relation_blocks(HW);
  const int ppb = (HW + nblk - 1) / nblk;
  launch(nblk, ppb);
  int rc = check_launch(what);
  if (rc) return rc;
  hipLaunchKernelGGL(relation_dscene_final_kernel, dim3((C + 7) / 8, N), dim3(256), 0, st, partial, dscene, nblk, C);
  return check_launch("relation_dscene_final");
}
// partial records of a backward call (0 for an empty map); C floats of scene gradient each, with BN + 2 x (sums [2][C] +
// maxima [2][C])
static size_t relation_records(int N, int HW) { return N > 0 && HW > 0 ? (size_t)N * relation_blocks(HW) : 0; }

}  // namespace evk

using namespace evk;

extern "C" int evk_relation_fwd(const float* scene, const float* content, const float* feat, float* out, float* r,
                                int32_t N, int32_t HW, int32_t C, void* stream) {
  EVK_REQUIRE(scene && content && feat && out && r && nhwc4_ok(N, HW, 1, C), EVK_E_INVALID, "relation_fwd: bad argument");
  hipLaunchKernelGGL(relation_fwd_kernel<false>, dim3(grid_for((size_t)N * HW, 4, 8192)), dim3(256), 0, (hipStream_t)stream,
                     scene, content, (const float*)nullptr, feat, (const float*)nullptr, out, r, N, HW, C, (uint32_t*)nullptr);
  return check_launch("relation_fwd");
}
extern "C" int evk_relation_bn_fwd(const float* scene, const float* zc, const float* scale_shift_c, const float* zf,
                                   const float* scale_shift_f, float* out, float* r, int32_t N, int32_t HW, int32_t C,
                                   uint32_t* out_absmax, void* stream) {
  EVK_REQUIRE(scene && zc && scale_shift_c && zf && scale_shift_f && out && r && nhwc4_ok(N, HW, 1, C), EVK_E_INVALID,
              "relation_bn_fwd: bad argument");
  hipLaunchKernelGGL(relation_fwd_kernel<true>, dim3(grid_for((size_t)N * HW, 4, 8192)), dim3(256), 0, (hipStream_t)stream,
                     scene, zc, scale_shift_c, zf, scale_shift_f, out, r, N, HW, C, out_absmax);
  return check_launch("relation_bn_fwd");
}
// partial records per BatchNorm: evk_relation_bn_parts(N, HW); workspace: evk_relation_bn_workspace_bytes
extern "C" int32_t evk_relation_bn_parts(int32_t N, int32_t HW) { return (int32_t)relation_records(N, HW); }
extern "C" size_t evk_relation_bn_workspace_bytes(int32_t N, int32_t HW, int32_t C) {
  return C > 0 ? relation_records(N, HW) * C * 9 * sizeof(float) : 0;
}
extern "C" int evk_relation_bn_bwd(const float* dout, const float* scene, const float* zc, const float* scale_shift_c,
                                   const float* mean_invstd_c, const float* zf, const float* scale_shift_f,
                                   const float* mean_invstd_f, const float* r, float* dscene, float* gc, float* gf,
                                   int32_t N, int32_t HW, int32_t C, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  EVK_REQUIRE(dout && scene && zc && scale_shift_c && mean_invstd_c && zf && scale_shift_f && mean_invstd_f && r && dscene &&
                  gc && gf,
              EVK_E_INVALID, "relation_bn_bwd: null pointer");
  EVK_REQUIRE(nhwc4_ok(N, HW, 1, C) && C <= 448, EVK_E_UNSUPPORTED, "relation_bn_bwd: C=%d", C);
  EVK_REQUIRE(workspace && workspace_bytes >= evk_relation_bn_workspace_bytes(N, HW, C), EVK_E_WORKSPACE,
              "relation_bn_bwd: workspace too small");
  const size_t nb = relation_records(N, HW);
  // workspace, in floats (nb = evk_relation_bn_parts records): [nb C] scene-gradient partials | content BatchNorm sums
  // [nb][2][C] | its maxima [nb][2][C] | re-encoding BatchNorm sums | its maxima  (evk_bn_bwd_from_partials takes the pairs)
  float* w = (float*)workspace;
  float* partial = w;
  float* bnp_c = w + nb * C;
  float* bnm_c = w + nb * 3 * C;
  float* bnp_f = w + nb * 5 * C;
  float* bnm_f = w + nb * 7 * C;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)4 * 9 * C * sizeof(float);
  EVK_REQUIRE(lds <= 64 * 1024, EVK_E_UNSUPPORTED, "relation_bn_bwd: C=%d does not fit the LDS", C);
  return relation_bwd_launch("relation_bn_bwd", partial, dscene, N, HW, C, st, [&](int nblk, int ppb) {
    pick<1, 2, 4>((C / 4 + 63) / 64, [&](auto NCH) {
      hipLaunchKernelGGL(relation_bn_bwd_kernel<NCH()>, dim3(nblk, N), dim3(256), lds, st, dout, scene, zc, scale_shift_c,
                         mean_invstd_c, zf, scale_shift_f, mean_invstd_f, r, gc, gf, partial, bnp_c, bnm_c, bnp_f, bnm_f, HW, C,
                         ppb, nblk);
      return 0;
    });
  });
}
extern "C" size_t evk_relation_workspace_bytes(int32_t N, int32_t HW, int32_t C) {
  return C > 0 ? relation_records(N, HW) * C * sizeof(float) : 0;
}
extern "C" int evk_relation_bwd(const float* dout, const float* scene, const float* content, const float* feat,
                                const float* r, float* dscene, float* dcontent, float* dfeat, int32_t N, int32_t HW,
                                int32_t C, void* workspace, size_t workspace_bytes, void* stream) {
  EVK_REQUIRE(dout && scene && content && feat && r && dscene && dcontent && dfeat, EVK_E_INVALID,
              "relation_bwd: null pointer");
  EVK_REQUIRE(nhwc4_ok(N, HW, 1, C) && C <= 4096, EVK_E_UNSUPPORTED, "relation_bwd: C=%d", C);
  EVK_REQUIRE(workspace && workspace_bytes >= evk_relation_workspace_bytes(N, HW, C), EVK_E_WORKSPACE,
              "relation_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  return relation_bwd_launch("relation_bwd", (const float*)workspace, dscene, N, HW, C, st, [&](int nblk, int ppb) {
    hipLaunchKernelGGL(relation_bwd_kernel, dim3(nblk, N), dim3(256), 4 * C * sizeof(float), st, dout, scene, content, feat, r,
                       dcontent, dfeat, (float*)workspace, HW, C, ppb, nblk);
  });
}
