// Convolution weight gradient on the bf16 matrix pipe at fp32-grade accuracy (3-way bf16 operand split,
// six partial products per product; arithmetic argument in conv_igemm_x3.hip).
//
//   dw[co][k] = sum_m dy[m][co] * im2col(x)[m][k]        m = (n, oy, ox),  k = (ky, kx, ci)
//
// Same reference call sites as conv_wgrad.hip (aten::convolution_backward(weight) of every nn.Conv2d on
// the path).  GEMM view: rows = Cout, cols = kh*kw*Cin, reduction = pixels, 32 pixels per step.
//
// v_mfma_f32_32x32x16_bf16 wants, per lane, EIGHT reduction-consecutive bf16 values of one row, but both
// operands are pixel-major in HBM ([pixel][channel]).  The transpose happens in registers: a staging
// thread owns a micro-block of 8 consecutive pixels x 4 consecutive channels (eight 16-byte global loads,
// coalesced across the lanes along the channel axis), splits its 32 values, and writes, per channel and
// plane, one 16-byte run of 8 pixels into the LDS image [plane][channel row][32 pixels] bf16.  Channel
// 4*cq + e of the tile is stored at LDS row e*(B/4) + cq: the lanes of one ds_write_b128 (fixed e) then hit
// consecutive rows = distinct bank slots; the epilogue undoes the permutation.  Threads 0..BM-1 stage dy,
// threads BM..BM+BN-1 stage im2col(x): both are the same gather with different (wave-uniform) parameters.
// Split over pixel ranges (grid.y) into the caller's workspace + splitk_reduce, as the fp32 kernel.
#include "wgrad_tile.hpp"
#include <stdlib.h>

namespace evk {

template <int BM, int BN, int WAVES_M, int WAVES_N, int NPX>
__global__ __launch_bounds__(256) void conv_wgrad_x3_kernel(const WGradArgs p) {
  constexpr int NP = X3Mode<NPX>::NP;
  constexpr bool PK = X3Mode<NPX>::PK;   // one or both operands arrive packed (p.x_packed / p.dy_packed; x3_common.hpp)
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MB = WM / 32, NB = WN / 32;
  constexpr int QA = BM / 4, QB = BN / 4;  // channel quads per operand
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  static_assert(BM % 64 == 0 && BN % 64 == 0 && BM + BN <= 256, "one micro-block per thread, wave-uniform roles");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
  unsigned char* const Ap = smem3;                      // [3][BM][64 B]
  unsigned char* const Bp = smem3 + 3 * BM * kRowBytes;  // [3][BN][64 B]

  const WGradTile tl(p, BM, BN);
  const int z = tl.z, co0 = tl.co0, k0 = tl.k0, pbeg = tl.pbeg;
  WGRAD_PIXEL_RANGE(p, pbeg);

  const int tid = threadIdx.x;
  // ---- staging role (wave-uniform): which tensor this thread gathers, and how
  const bool roleA = tid < BM;
  const bool staged = tid < BM + BN;
  const int idx = roleA ? tid : tid - BM;
  const int Q = roleA ? QA : QB;
  const int cq = idx % Q;  // channel quad
  const int pg = idx / Q;  // pixel group (8 pixels) 0..3
  const PtrLoad ld(roleA ? p.dy : p.x);
  WGather g{roleA ? p.Ho : p.H, roleA ? p.Wo : p.W, roleA ? p.Cout : p.Cin, roleA ? 1 : p.sh, roleA ? 1 : p.sw, 0, 0, 0, false};
  if (roleA) {
    g.coff = co0 + cq * 4;
    g.cvalid = g.coff < p.Cout;
  } else if (staged) {
    const WGradTap tap(p, (k0 >> 2) + cq);
    g.offy = tap.offy; g.offx = tap.offx; g.coff = tap.coff;
    g.cvalid = tap.valid;
  }
  unsigned char* const st_base = (roleA ? Ap : Bp);
  const int st_plane = (roleA ? BM : BN) * kRowBytes;

  f32x4 rv[8];
  uint32_t okmask = 0;
  float st_inv = 1.f, out_scale = 1.f;   // f16x2: 1 / scale of the operand this thread stages; product of both scales
  if constexpr (NP == 2) {
    const OpScale sx = op_scale(act_absmax(p.x_scale)), sd = op_scale(act_absmax(p.dy_scale));
    st_inv = roleA ? sd.inv : sx.inv;
    out_scale = sx.s * sd.s;
  }
  const bool st_packed = PK && (roleA ? p.dy_packed : p.x_packed) != 0;   // wave-uniform

  auto load_tiles = [&](int pix0) {
    // (Wo % 8 == 0: the 8 pixels share an output row, one (n, oy, ox) decomposition per micro-block)
    if ((p.Wo & 7) == 0) gather8<true>(p, g, ld, pix0 + pg * 8, pend, rv, okmask);
    else gather8<false>(p, g, ld, pix0 + pg * 8, pend, rv, okmask);
  };
  auto store_tiles = [&]() {
    zero_masked(rv, okmask);
    if constexpr (PK) {
      if (st_packed) return split_store<NP, 4, true>(rv, st_base, st_plane, Q, cq, pg, st_inv);
    }
    split_store<NP, 4, false>(rv, st_base, st_plane, Q, cq, pg, st_inv);
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

  int fa_off[MB][2], fb_off[NB][2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
    for (int a = 0; a < MB; ++a) fa_off[a][kk] = wg_off(wm * WM + a * 32 + li, 2 * kk + lh);
#pragma unroll
    for (int b = 0; b < NB; ++b) fb_off[b][kk] = wg_off(wn * WN + b * 32 + li, 2 * kk + lh);
  }

  if (nk > 0 && staged) {
    load_tiles(pbeg);
    store_tiles();
  }
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more && staged) load_tiles(pbeg + (kt + 1) * BKP);
    half_step<MB, NB, NP>(acc, Ap, Bp, BM * kRowBytes, BN * kRowBytes, fa_off, fb_off, 0);
    half_step<MB, NB, NP>(acc, Ap, Bp, BM * kRowBytes, BN * kRowBytes, fa_off, fb_off, 1);
    __syncthreads();
    if (more) {
      if (staged) store_tiles();
      __syncthreads();
    }
  }

  // D rows = A rows (dy channels), D cols = B rows (im2col columns), both under the staging permutation
  float* out = p.out + (size_t)z * p.Cout * p.Ktot;
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ra = wm * WM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int row = co0 + 4 * (ra % QA) + ra / QA;
      if (row >= p.Cout) continue;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int rb = wn * WN + b * 32 + li;
        const int col = k0 + 4 * (rb % QB) + rb / QB;
        if (col < p.Ktot) out[(size_t)row * p.Ktot + col] = acc[a][b][r] * out_scale;
      }
    }
}

int launch_wgrad_x3(const WGradArgs& a, const WGradRoute& r, hipStream_t stream) {
  if (r.kernel == WGradKernel::X3Ws) return launch_wgrad_x3ws(a, r, stream);
  return pick_tile(r.plan.bm, r.plan.bn, [&](auto BM, auto BN) {
    return pick<1, 4, 2, 3>(r.npx, [&](auto NPX) {
      constexpr int bm = decltype(BM)::value, bn = decltype(BN)::value;
      hipLaunchKernelGGL((conv_wgrad_x3_kernel<bm, bn, 2, 2, decltype(NPX)::value>), dim3(a.tiles_co * a.tiles_k * a.splitk),
                         dim3(256), (size_t)3 * (bm + bn) * kRowBytes, stream, a);
      return check_launch("conv_wgrad_x3");
    });
  });
}

}  // namespace evk
