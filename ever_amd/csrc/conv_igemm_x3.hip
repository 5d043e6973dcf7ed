// Implicit-GEMM convolution (forward and data gradient) on the bf16 matrix pipe with fp32-grade
// arithmetic: every fp32 operand is split EXACTLY into three bf16 terms  x = h + m + l  (round-to-
// nearest-even at each level: |m| <= 2^-9 |x|, |l| <= 2^-18 |x|) and the product is assembled from the six
// partial products that are not below fp32 resolution,
//     x*w  ~=  l*wh + h*wl + m*wm + m*wh + h*wm + h*wh        (dropped: m*wl, l*wm, l*wl  <=  2^-26 |x*w|)
// each an exact bf16 x bf16 product accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  Six bf16 MFMAs
// (6 x 32 cycles for 32x32x16) replace eight v_mfma_f32_32x32x2_f32 (8 x 64 cycles): 2.67x the
// matrix-pipe rate of the exact-fp32 kernel in conv_igemm_f32.hip, with an error per product below one
// fp32 rounding (measured at the logits against fp64: same as the fp32 CPU reference).
//
// Same gather / destination algebra as conv_igemm_f32.hip (IGemmArgs), from the same code (igemm_tile.hpp); requires Cs % 8 == 0.
//   A (im2col rows, fp32 in HBM): global -> VGPR (two 16-byte loads = 8 floats per row slot) -> split in
//     registers (v_cvt_pk_bf16_f32 + exact residuals) -> three bf16 planes in LDS.
//   B (weights): split ONCE per step (split_weight.hip, split_weight_multi.hip) into three bf16 planes [3][Cd][Kpad] in HBM
//     (they are reused by every tile), streamed global -> VGPR -> LDS with no VALU work.
// LDS stage: 3 x [BM][32] + 3 x [BN][32] bf16, rows of 64 bytes, 16-byte chunk index ^= (row>>2)&3 so
// that the ds_read_b128 fragment reads of a 16-lane group cover 16 distinct 16-byte slots.
// Fragment: lane l holds row l&31, k = 16*kk + 8*(l>>5) .. +7 (one ds_read_b128) for A and B alike.
#include "conv_route.hpp"
#include "igemm_tile.hpp"

namespace evk {

// One LDS stage (NBUF = 1; 48 KB at 128 x 128 => 2-3 workgroups per CU, whose split and MFMA phases interleave): the next
// step's global loads fly under this step's MFMAs, the split and the LDS writes follow between two barriers.
template <int BM, int BN, int WAVES_M, int WAVES_N, int NBUF, int NPX>
__global__ __launch_bounds__(256) void conv_igemm_x3_kernel(const IGemmArgs p) {
  constexpr int NP = X3Mode<NPX>::NP;
  constexpr bool PK = X3Mode<NPX>::PK;   // the activation operand arrives packed (x3_common.hpp)
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MB = WM / 32, NB = WN / 32;
  constexpr int AR = BM / 64, BR = BN / 64;  // row slots per thread (64 rows x 4 sixteen-byte chunks per pass)
  constexpr int kAPlane = BM * kRowBytes, kBPlane = BN * kRowBytes;
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");
  static_assert(NBUF == 1, "the K loop below is written for one LDS stage");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];

  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_n = bid % p.tiles_n;
  const int tile_m = bid / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const int tid = threadIdx.x;
  const int c4 = tid & 3;   // 8-float group inside the K step
  const int rb = tid >> 2;  // base row 0..63

  IGemmRows<AR> rows;
#pragma unroll
  for (int j = 0; j < AR; ++j) rows.decode(p, j, m0 + rb + 64 * j);
  int b_off[BR];
  weight_rows_decode(p, n0 + rb, c4, b_off);

  const int plane = p.Cd * p.Kpad;  // bf16 elements per weight plane

  const int cp8 = p.Cs >> 3;  // 8-float groups per tap
  IGemmCursor<4> cur;
  cur.seek(c4, cp8, p.kw);

  f32x4 ra[AR][2];
  u32x4 rbv[BR][3];
  uint32_t okmask = 0;
  float a_inv = 1.f, out_scale = 1.f;   // f16x2: 1 / activation scale; activation scale x weight scale
  if constexpr (NP == 2) {
    const OpScale sa = op_scale(act_absmax(p.a_scale)), sw = op_scale(*p.w_scale);
    a_inv = sa.inv;
    out_scale = sa.s * sw.s;
  }

  auto load_tiles = [&](int kt) {
    okmask = igemm_gather<8>(p, rows, cur, ra);
    weight_rows_load<NP>(p, b_off, plane, kt, rbv);
    cur.advance(kt, c4, cp8, p.kw);
  };
  auto store_tiles = [&]() {
    unsigned char* Ab = smem3;                 // [3][BM][64 B]
    unsigned char* Bb = smem3 + 3 * kAPlane;   // [3][BN][64 B]
    split_store_rows<NP, PK>(ra, okmask, Ab, kAPlane, rb, c4, a_inv);
    weight_rows_store<NP>(rbv, Bb, kBPlane, rb, c4);
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

  const int nk = p.Kpad / BK3;

  load_tiles(0);
  store_tiles();
  __syncthreads();

  // fragment byte offsets inside a plane (igemm_tile.hpp: the tables are filled here)
  int fa_off[MB][2], fb_off[NB][2];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) fa_off[a][kk] = plane_off(wm * WM + a * 32 + li, 2 * kk + lh);
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) fb_off[b][kk] = plane_off(wn * WN + b * 32 + li, 2 * kk + lh);
  auto half_step = [&](const unsigned char* Ab, const unsigned char* Bb, int kk) {
    bf16x8 fa[MB][3], fb[NB][3];
    frag_read<NP, kAPlane, kBPlane>(fa, fb, Ab, Bb, fa_off, fb_off, kk);
    frag_mma<NP>(acc, fa, fb);
  };

  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    const unsigned char* Ab = smem3;
    const unsigned char* Bb = Ab + 3 * kAPlane;
    if (more) load_tiles(kt + 1);
    half_step(Ab, Bb, 0);
    half_step(Ab, Bb, 1);
    __syncthreads();
    if (more) {
      store_tiles();
      __syncthreads();
    }
  }

  if constexpr (NP == 2) igemm_scale_acc<MB, NB>(acc, out_scale);
  if (p.bn_part) {
    // every wave is done with the last stage (the loop ends on a barrier): the ring becomes epilogue scratch
    igemm_epilogue_stats<MB, NB, WM, WN, WAVES_M, WAVES_N>(p, acc, m0, n0, wm, wn, li, lh, reinterpret_cast<float*>(smem3));
    return;
  }
  AmaxAcc amax_l{0u, p.out_amax != nullptr};
  igemm_epilogue<MB, NB, WM, WN>(p, acc, m0, n0, wm, wn, li, lh, amax_l);
  if (p.out_amax) amax_commit(p.out_amax, amax_l.m);
}

// the register-staged split kernels (this one and conv_igemm_x3ws.hip): 32-bit element offsets, 16-byte loads of 8 channels
bool igemm_x3_supports(const IGemmArgs& a) {
  const long long src_elems = (long long)a.N * a.Hs * a.Ws * a.Cs;
  const long long wgt_elems = (long long)a.Cd * a.Kpad * 3;
  return src_elems < 0x7fffffffLL && wgt_elems < 0x7fffffffLL && (a.Cs & 7) == 0;
}

int launch_igemm_x3(IGemmArgs& a, const ConvRoute& r, hipStream_t stream) {
  EVK_REQUIRE((a.Cs & 7) == 0, EVK_E_UNSUPPORTED, "conv_igemm_x3: source channels (%d) must be a multiple of 8", a.Cs);
  EVK_REQUIRE(igemm_x3_supports(a), EVK_E_UNSUPPORTED, "conv_igemm_x3: tensors of 2^31 or more elements are not supported");
  EVK_REQUIRE((r.bm == 128 || r.bm == 64) && (r.bn == 128 || r.bn == 64), EVK_E_INVALID, "conv_igemm_x3: no %d x %d tile", r.bm, r.bn);
  return pick_tile(r.bm, r.bn, [&](auto BM, auto BN) {
    return pick_npx(a, [&](auto NPX) {
      constexpr int bm = decltype(BM)::value, bn = decltype(BN)::value;
      // statistics epilogue: per-wave scratch + the row waves' exchange area
      return launch_igemm_tile<&conv_igemm_x3_kernel<bm, bn, 2, 2, 1, decltype(NPX)::value>>(
          a, stream, "conv_igemm_x3", bm, bn, 2, 256, (size_t)3 * (bm + bn) * kRowBytes,
          ((size_t)4 * 32 * (bn / 2 + 4) + (size_t)3 * bn) * sizeof(float));
    });
  });
}

}  // namespace evk
