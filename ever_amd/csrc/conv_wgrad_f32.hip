// Convolution weight gradient for gfx950 on v_mfma_f32_32x32x2_f32: the fp32 kernel of the family (conv_wgrad.hip).
//
//   dw[co][k] = sum_m dy[m][co] * im2col(x)[m][k]        m = (n, oy, ox),  k = (ky, kx, ci)
//
// Replaces aten::convolution_backward(weight, bias) of the nn.Conv2d sites listed in
// conv_igemm_f32.hip (reference ever/module/_resnets.py:21-29,149 ; fpn.py ; fs_relation.py).
//
// GEMM view: rows = Cout, cols = kh*kw*Cin, reduction = pixels.  Both operands are stored
// pixel-major in HBM ([pixel][channel]), which is exactly the k-major LDS image the f32 MFMA
// fragments want (lane l reads row k=l>>5, column i=l&31: 32 consecutive words, conflict free),
// so tiles are staged [32 pixels][BM or BN channels] without any transpose.  The pixel range is
// split across workgroups (grid.z); partial tiles go to the caller's workspace and are summed in a
// fixed order by a second kernel (splitk_reduce, conv_wgrad.hip) => bitwise reproducible, no atomics.
#include "wgrad_tile.hpp"

namespace evk {

template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WGradArgs p) {
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MB = WM / 32, NB = WN / 32;
  constexpr int ACH = BM / 4, BCH = BN / 4;          // 16-byte chunks per staged row
  constexpr int APASS = BKP * ACH / 256, BPASS = BKP * BCH / 256;
  constexpr int AROWS = 256 / ACH, BROWS = 256 / BCH;  // rows covered per pass
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  static_assert(MB <= 2 && NB <= 2, "fragment vectors are float or float2");
  struct alignas(4 * MB) FragA { float v[MB]; };
  struct alignas(4 * NB) FragB { float v[NB]; };

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                   // [2][32][BM]
  float* Bs = smem + 2 * BKP * BM;    // [2][32][BN]

  const WGradTile tl(p, BM, BN);
  const int z = tl.z, co0 = tl.co0, k0 = tl.k0, pbeg = tl.pbeg;
  WGRAD_PIXEL_RANGE(p, pbeg);

  const int tid = threadIdx.x;
  // A staging: dy rows
  const int a_c = tid % ACH, a_r = tid / ACH;
  const bool a_cvalid = (co0 + a_c * 4) < p.Cout;
  // B staging: im2col rows; this thread's K chunk is fixed for the whole reduction
  const int b_c = tid % BCH, b_r = tid / BCH;
  const WGradTap tap(p, (k0 >> 2) + b_c);

  f32x4 ra[APASS], rb[BPASS];
  uint32_t okmask = 0;  // bit j: A pass j valid; bit 16+j: B pass j valid

  // Branch-free gathers: every load is issued from a clamped (valid) 32-bit element offset; the
  // zero-fill select is applied when the chunk is written to LDS (after the MFMA block), so the
  // prefetch stays in flight under the MFMAs.
  auto load_tiles = [&](int pix0) {
    okmask = 0;
#pragma unroll
    for (int j = 0; j < APASS; ++j) {
      const int m = pix0 + a_r + j * AROWS;
      const bool ok = a_cvalid && m < pend;
      okmask |= ok ? (1u << j) : 0u;
      ra[j] = *reinterpret_cast<const f32x4*>(p.dy + (ok ? m * p.Cout + co0 + a_c * 4 : 0));
    }
#pragma unroll
    for (int j = 0; j < BPASS; ++j) {
      const int m = pix0 + b_r + j * BROWS;
      const WGradPix px(p, m);
      const int sy = px.oy * p.sh + tap.offy;
      const int sx = px.ox * p.sw + tap.offx;
      const bool ok = tap.valid && m < pend && (unsigned)sy < (unsigned)p.H && (unsigned)sx < (unsigned)p.W;
      okmask |= ok ? (1u << (16 + j)) : 0u;
      rb[j] = *reinterpret_cast<const f32x4*>(p.x + (ok ? ((px.n * p.H + sy) * p.W + sx) * p.Cin + tap.coff : 0));
    }
  };
  auto store_tiles = [&](int buf) {
    float* Ab = As + buf * BKP * BM;
    float* Bb = Bs + buf * BKP * BN;
#pragma unroll
    for (int j = 0; j < APASS; ++j) {
      const bool ok = (okmask >> j) & 1u;
      f32x4 v = ra[j];
      v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
      *reinterpret_cast<f32x4*>(Ab + (a_r + j * AROWS) * BM + a_c * 4) = v;
    }
#pragma unroll
    for (int j = 0; j < BPASS; ++j) {
      const bool ok = (okmask >> (16 + j)) & 1u;
      f32x4 v = rb[j];
      v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
      *reinterpret_cast<f32x4*>(Bb + (b_r + j * BROWS) * BN + b_c * 4) = v;
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;

  f32x16 acc[MB][NB];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  if (nk > 0) {
    load_tiles(pbeg);
    store_tiles(0);
  }
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_tiles(pbeg + (kt + 1) * BKP);
    // Fragment reads: the wave's 64 (or 32) tile rows are dealt to (MFMA block a, lane row i) as
    // row = MB*i + a, so ONE ds_read_b64 per operand feeds both blocks of a k-step, and the reads of
    // step s+1 are issued before the MFMAs of step s (register double buffer) to hide LDS latency.
    const float* Ab = As + buf * BKP * BM + wm * WM + MB * li;
    const float* Bb = Bs + buf * BKP * BN + wn * WN + NB * li;
    FragA fa_cur = *reinterpret_cast<const FragA*>(Ab + lh * BM);
    FragB fb_cur = *reinterpret_cast<const FragB*>(Bb + lh * BN);
#pragma unroll
    for (int s = 0; s < BKP / 2; ++s) {
      FragA fa_nxt = fa_cur;
      FragB fb_nxt = fb_cur;
      if (s + 1 < BKP / 2) {
        fa_nxt = *reinterpret_cast<const FragA*>(Ab + (2 * s + 2 + lh) * BM);
        fb_nxt = *reinterpret_cast<const FragB*>(Bb + (2 * s + 2 + lh) * BN);
      }
#pragma unroll
      for (int a = 0; a < MB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa_cur.v[a], fb_cur.v[b], acc[a][b], 0, 0, 0);
      fa_cur = fa_nxt;
      fb_cur = fb_nxt;
      // pin the issue order: this step's (prefetch) LDS reads first, then its MFMAs -> the reads'
      // latency is covered by MB*NB MFMAs (>= 256 cycles) instead of being waited for at once
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, MB * NB, 0);
    }
    if (kt + 1 < nk) store_tiles(buf ^ 1);
    __syncthreads();
  }

  float* out = p.out + (size_t)z * p.Cout * p.Ktot;
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = co0 + wm * WM + MB * ((r & 3) + 8 * (r >> 2) + 4 * lh) + a;
      if (row >= p.Cout) continue;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int col = k0 + wn * WN + NB * li + b;
        if (col < p.Ktot) out[(size_t)row * p.Ktot + col] = acc[a][b][r];
      }
    }
}

int launch_wgrad_f32(const WGradArgs& a, const WGradRoute& r, hipStream_t stream) {
  return pick_tile(r.plan.bm, r.plan.bn, [&](auto BM, auto BN) {
    constexpr int bm = decltype(BM)::value, bn = decltype(BN)::value;
    hipLaunchKernelGGL((conv_wgrad_kernel<bm, bn, 2, 2>), dim3(a.tiles_co * a.tiles_k * a.splitk), dim3(256),
                       (size_t)2 * BKP * (bm + bn) * sizeof(float), stream, a);
    return check_launch("conv_wgrad");
  });
}

}  // namespace evk
