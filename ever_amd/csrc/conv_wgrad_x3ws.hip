// Wave-specialised, wide-tile form of the split-MFMA weight gradient (arithmetic and LDS image: see
// conv_wgrad_x3.hip / conv_igemm_x3.hip).  One 8-wave workgroup per CU computes a 128 (Cout) x 256 (k) tile
// of dw over its pixel chunk:
//   waves 0-3  matrix waves, 64 x 128 each (2 x 4 MFMA blocks): fragment reads + v_mfma_f32_32x32x16_bf16;
//   waves 4-7  staging waves: every thread gathers an 8-pixel x 4-channel micro-block of im2col(x) (256 per
//              step), threads of waves 4-5 one of dy in addition (128 per step); exact 3-way bf16 split and
//              the register transpose into the pixel-contiguous planes; two register sets deep, two LDS stages.
// Against the 128x128 single-role kernel: 25 % fewer operand elements (loads and splits) per MFMA, and the
// split no longer shares a wave with the MFMA stream.
#include "wgrad_tile.hpp"
#include <stdlib.h>

namespace evk {

// PKX / PKD: x / dy arrive packed (f16x2 only; x3_common.hpp)
template <int BM, int BN, int NP, bool W8, bool PKX = false, bool PKD = false>
__global__ __launch_bounds__(512) void conv_wgrad_x3ws_kernel(const WGradArgs p) {
  static_assert(NP == 2 || (!PKX && !PKD), "packed operands exist for the f16x2 arithmetic only");
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int MB = WM / 32, NB = WN / 32;
  constexpr int QA = BM / 4, QB = BN / 4;
  constexpr int kStage = 3 * (BM + BN) * kRowBytes;
  static_assert(QB * 4 == 256 && QA * 4 <= 256, "staging waves: one im2col micro-block per thread, dy on the first ones");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];

  const WGradTile tl(p, BM, BN);
  const int z = tl.z, co0 = tl.co0, k0 = tl.k0, pbeg = tl.pbeg;
  WGRAD_PIXEL_RANGE(p, pbeg);
  const int tid = threadIdx.x;

  if (tid >= 256) {
    // ------------------------------------------------------------------ staging waves
    const int ptid = tid - 256;
    // every staging thread: one im2col micro-block (8 px x 4 ch) + one HALF dy micro-block (8 px x 2 ch) — the
    // dy tile dealt over all four waves (with whole dy micro-blocks on two waves those two set the pace:
    // measured 51 % matrix-pipe occupancy, the matrix waves waiting at the barrier)
    constexpr int QA2 = BM / 2;
    static_assert(QA2 * 4 == 256, "one half dy micro-block per staging thread");
    const int bcq = ptid % QB, bpg = ptid / QB;
    const int acq = ptid % QA2, apg = ptid / QA2;
    const int a_coff = co0 + acq * 2;
    const bool a_cvalid = a_coff < p.Cout;
    const WGradTap tap(p, (k0 >> 2) + bcq);
    const WGather gb{p.H, p.W, p.Cin, p.sh, p.sw, tap.offy, tap.offx, tap.coff, tap.valid};
    f32x2v ra[2][8];
    f32x4 rb[2][8];
    uint32_t oka[2] = {0, 0}, okb[2] = {0, 0};
    // f16x2: buffer loads with out-of-range zero fill (the other arithmetics measure slower with them: wgrad_tile.hpp)
    using Ld = std::conditional_t<NP == 2, BufLoad, PtrLoad>;
    const Ld ld_x(p.x, p.N * p.H * p.W * p.Cin * 4), ld_dy(p.dy, p.M * p.Cout * 4);
    float x_inv = 1.f, dy_inv = 1.f;   // f16x2: 1 / operand scales
    if constexpr (NP == 2) {
      x_inv = op_scale(act_absmax(p.x_scale)).inv;
      dy_inv = op_scale(act_absmax(p.dy_scale)).inv;
    }

    auto load = [&](auto SET, int kt) {
      constexpr int s = decltype(SET)::value;
      const int pix0 = pbeg + kt * BKP;
      if (kWgAbl & 1) return;   // ablation: no global loads
      gather8<W8>(p, gb, ld_x, pix0 + bpg * 8, pend, rb[s], okb[s]);
      gather8h(ld_dy, p.Cout, a_coff, a_cvalid, pix0 + apg * 8, pend, ra[s], oka[s]);
    };
    auto store = [&](auto SET, int stage) {
      constexpr int s = decltype(SET)::value;
      unsigned char* Ab = smem3 + stage * kStage;
      unsigned char* Bb = Ab + 3 * BM * kRowBytes;
      if (kWgAbl & 2) return;   // ablation: no split, no LDS writes
      if constexpr (!Ld::kZeroFill) {
        zero_masked(rb[s], okb[s]);
        zero_masked(ra[s], oka[s]);
      }
      split_store<NP, 4, PKX>(rb[s], Bb, BN * kRowBytes, QB, bcq, bpg, x_inv);
      split_store<NP, 2, PKD>(ra[s], Ab, BM * kRowBytes, QA2, acq, apg, dy_inv);
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    if (nk > 0) {
      load(S0{}, 0);
      if (1 < nk) load(S1{}, 1);
      store(S0{}, 0);
      if (2 < nk) load(S0{}, 2);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
      if (kt + 1 < nk) {
        store(S1{}, 1);
        if (kt + 3 < nk) load(S1{}, kt + 3);
      }
      __syncthreads();
      if (kt + 1 < nk) {
        if (kt + 2 < nk) {
          store(S0{}, 0);
          if (kt + 4 < nk) load(S0{}, kt + 4);
        }
        __syncthreads();
      }
    }
    return;
  }

  // -------------------------------------------------------------------- matrix waves
  __builtin_amdgcn_s_setprio(3);
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  f32x16 acc[MB][NB];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // im2col LDS row e * QB + q holds channel 4q + e of the k range (staging permutation).  Matrix wave wn takes q in
  // [32 wn, 32 wn + 32) of ALL four e-blocks as its NB = 4 column blocks: lane li then owns the four CONSECUTIVE
  // k columns 4 (32 wn + li) + {0..3} across its blocks, i.e. one 16-byte store per accumulator row.
  int fa_off[MB][2], fb_off[NB][2];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) fa_off[a][kk] = wg_off(wm * WM + a * 32 + li, 2 * kk + lh);
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) fb_off[b][kk] = 3 * BM * kRowBytes + wg_off(b * QB + wn * 32 + li, 2 * kk + lh);

  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const unsigned char* S = smem3 + (kt & 1) * kStage;
    if (!(kWgAbl & 4)) {      // ablation: no fragment reads / MFMAs
      half_step<MB, NB, NP>(acc, S, S, BM * kRowBytes, BN * kRowBytes, fa_off, fb_off, 0);
      half_step<MB, NB, NP>(acc, S, S, BM * kRowBytes, BN * kRowBytes, fa_off, fb_off, 1);
    }
    __syncthreads();
  }
  if (kWgAbl & 8) {           // ablation: no stores
    if (acc[0][0][0] == 12345.f) p.out[0] = 0.f;
    return;
  }

  if constexpr (NP == 2) {   // f16x2: back to the operands' units
    const float sc = op_scale(act_absmax(p.x_scale)).s * op_scale(act_absmax(p.dy_scale)).s;
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] *= sc;
  }
  float* out = p.out + (size_t)z * p.Cout * p.Ktot;
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ra_ = wm * WM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int row = co0 + 2 * (ra_ % (BM / 2)) + ra_ / (BM / 2);   // inverse of the dy staging permutation
      if (row >= p.Cout) continue;
      static_assert(NB == 4 && QB == 64, "column blocks = the four channels of a staging micro-block");
      const int col = k0 + 4 * (wn * 32 + li);
      if (col + 3 < p.Ktot) {   // Ktot = taps * Cin with Cin % 4 == 0: rows are 16-byte aligned
        const f32x4 v = {acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]};
        *reinterpret_cast<f32x4*>(out + (size_t)row * p.Ktot + col) = v;
      } else {
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (col + b < p.Ktot) out[(size_t)row * p.Ktot + col + b] = acc[a][b][r];
      }
    }
}

template <int NP, bool W8, bool PKX = false, bool PKD = false>
static int launch_wgrad_x3ws_t(const WGradArgs& a, hipStream_t stream) {
  constexpr int BM = 128, BN = 256;
  const size_t lds = (size_t)2 * 3 * (BM + BN) * kRowBytes;
  static PerDeviceOnce attr_once;
  if (attr_once.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wgrad_x3ws_kernel<BM, BN, NP, W8, PKX, PKD>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  hipLaunchKernelGGL((conv_wgrad_x3ws_kernel<BM, BN, NP, W8, PKX, PKD>), dim3(a.tiles_co * a.tiles_k * a.splitk), dim3(512), lds, stream, a);
  return check_launch("conv_wgrad_x3ws");
}

int launch_wgrad_x3ws(const WGradArgs& a, const WGradRoute& r, hipStream_t stream) {
  return pick<1, 2, 3>(r.npx, [&](auto NP) {
    return pick<1, 0>(r.w8, [&](auto W8) {
      constexpr int np = decltype(NP)::value;
      constexpr bool w8 = decltype(W8)::value != 0;
      if constexpr (np != 2) return launch_wgrad_x3ws_t<np, w8>(a, stream);   // (packed operands: f16x2 only)
      else return pick<1, 0>(r.pkx, [&](auto PKX) {
        return pick<1, 0>(r.pkd, [&](auto PKD) {
          return launch_wgrad_x3ws_t<np, w8, decltype(PKX)::value != 0, decltype(PKD)::value != 0>(a, stream);
        });
      });
    });
  });
}

}  // namespace evk
