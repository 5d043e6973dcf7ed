// Wave-specialised form of the bf16-split implicit-GEMM convolution (arithmetic: conv_igemm_x3.hip).
//
// One workgroup = 8 waves on one CU = 2 waves per SIMD with different jobs:
//   waves 0-3  "matrix" waves: ds_read_b128 fragments + v_mfma_f32_32x32x16_bf16, nothing else.  One per
//              SIMD, so each owns its SIMD's matrix pipe and issues MFMAs back to back.
//   waves 4-7  "staging" waves: im2col gather (global -> VGPR), exact 3-way bf16 split (~6 VALU per
//              element), ds_write_b128 of the three planes, and the pre-split weight planes
//              global -> VGPR -> LDS.  Their VALU / VMEM / LDS-write instructions issue from a different
//              wave than the MFMAs, so they fill the matrix pipe's shadow instead of serialising with
//              it (in the single-role kernel the split is a ~900-cycle MFMA-free phase per step:
//              measured 56 % matrix-pipe occupancy at 2 workgroups per CU).
// LDS is a ring of NSTAGE stages; stage s of step kt is written while the matrix waves read step kt's
// stage, one s_barrier per step for all 8 waves.
#include "conv_route.hpp"
#include "igemm_tile.hpp"

namespace evk {

template <int BM, int BN, int WAVES_M, int WAVES_N, int NSTAGE, int NPX>
__global__ __launch_bounds__(512) void conv_igemm_x3ws_kernel(const IGemmArgs p) {
  constexpr int NP = X3Mode<NPX>::NP;
  constexpr bool PK = X3Mode<NPX>::PK;   // the activation operand arrives packed (x3_common.hpp)
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MB = WM / 32, NB = WN / 32;
  constexpr int AR = BM / 64, BR = BN / 64;
  constexpr int kAPlane = BM * kRowBytes, kBPlane = BN * kRowBytes;
  constexpr int kStage = 3 * (kAPlane + kBPlane);
  static_assert(WAVES_M * WAVES_N == 4, "4 matrix waves");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];

  // PERSISTENT: workgroup b walks tiles b, b + gridDim.x, ... and treats their K loops as ONE sequence of steps
  // g = 0 .. G-1 (G = my tiles x nk).  The LDS ring, the register sets and the one-barrier-per-step protocol run on
  // across tile boundaries, so while the matrix waves store tile t's accumulators the staging waves are already two
  // steps into tile t+1 — and the two roles' memory instructions are counted by different waves' vmcnt, so the
  // stores' drain never sits in front of a wait for new loads (which is what made persistent tiles useless in the
  // single-role kernel).  With gridDim.x == tiles it is the one-tile-per-workgroup kernel it used to be.
  const int ntiles = p.tiles_m * p.tiles_n;
  const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int nk = p.Kpad / BK3;
  const int G = my_tiles * nk;
  const int tid = threadIdx.x;

  if (tid >= 256) {
    // ------------------------------------------------------------------ staging waves
    const int ptid = tid - 256;
    const int c4 = ptid & 3;   // 8-float group inside the K step
    const int rb = ptid >> 2;  // base row 0..63

    IGemmRows<AR> rows;
    int b_off[BR];
    const int plane = p.Cd * p.Kpad;  // bf16 elements per weight plane
    const int cp8 = p.Cs >> 3;
    IGemmCursor<4> cur;
    int lt_tile = 0, lt_kt = 0;  // load cursor: (index among my tiles, K step) of the next load_tiles call

    auto begin_tile = [&](int i) {
      const int bid = xcd_remap((int)blockIdx.x + i * (int)gridDim.x, ntiles);
      const int tile_n = bid % p.tiles_n;
      const int tile_m = bid / p.tiles_n;
#pragma unroll
      for (int j = 0; j < AR; ++j) rows.decode(p, j, tile_m * BM + rb + 64 * j);
      weight_rows_decode(p, tile_n * BN + rb, c4, b_off);
      cur.seek(c4, cp8, p.kw);
    };

    // two register sets: the loads of step t+2 are issued before step t+1's registers are consumed, so a
    // global / L2 round trip has two full steps (~1.5 us) to land (with one set the staging waves sat
    // in s_waitcnt vmcnt for most of every step and the matrix waves waited for them at the barrier:
    // measured 209 -> 273 TFLOP/s on 3x3x256 @128^2 when the loads were removed)
    f32x4 ra[2][AR][2];
    u32x4 rbv[2][BR][3];
    uint32_t okmask[2] = {0, 0};
    float a_inv = 1.f;   // f16x2: 1 / activation scale
    if constexpr (NP == 2) a_inv = op_scale(act_absmax(p.a_scale)).inv;

    auto load_tiles = [&](auto SET) {
      constexpr int s = decltype(SET)::value;
      if (lt_kt == 0) begin_tile(lt_tile);
      okmask[s] = igemm_gather<8>(p, rows, cur, ra[s]);
      weight_rows_load<NP>(p, b_off, plane, lt_kt, rbv[s]);
      cur.advance(lt_kt, c4, cp8, p.kw);
      if (++lt_kt == nk) {
        lt_kt = 0;
        ++lt_tile;
      }
    };
    auto store_tiles = [&](auto SET, int stage) {
      constexpr int s = decltype(SET)::value;
      unsigned char* Ab = smem3 + stage * kStage;
      split_store_rows<NP, PK>(ra[s], okmask[s], Ab, kAPlane, rb, c4, a_inv);
      weight_rows_store<NP>(rbv[s], Ab + 3 * kAPlane, kBPlane, rb, c4);
    };

    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    static_assert(NSTAGE == 2, "staging schedule below is written for a two-stage ring");
    // step g lives in register set g & 1 and LDS stage g & 1.  Prologue: step 0 -> stage 0, steps 1 and 2 in flight.
    load_tiles(S0{});
    if (1 < G) load_tiles(S1{});
    store_tiles(S0{}, 0);
    if (2 < G) load_tiles(S0{});
    __syncthreads();
    // iteration g: the matrix waves read stage g & 1; step g+1 goes to the other stage and its
    // register set is refilled with step g+3
    for (int g = 0; g < G; g += 2) {
      if (g + 1 < G) {
        store_tiles(S1{}, 1);
        if (g + 3 < G) load_tiles(S1{});
      }
      __syncthreads();
      if (g + 1 < G) {
        if (g + 2 < G) {
          store_tiles(S0{}, 0);
          if (g + 4 < G) load_tiles(S0{});
        }
        __syncthreads();
      }
    }
    return;
  }

  // -------------------------------------------------------------------- matrix waves
  // issue arbitration on a SIMD is by priority, then age: the MFMA stream must never queue behind the
  // staging wave's VALU work
  __builtin_amdgcn_s_setprio(3);
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;

  f32x16 acc[MB][NB];

  int fa_off[MB][2], fb_off[NB][2];   // from the stage's base: the weight planes follow the three activation planes
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) fa_off[a][kk] = plane_off(wm * WM + a * 32 + li, 2 * kk + lh);
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) fb_off[b][kk] = 3 * kAPlane + plane_off(wn * WN + b * 32 + li, 2 * kk + lh);

  float out_scale = 1.f;   // f16x2: activation scale x weight scale
  if constexpr (NP == 2) out_scale = op_scale(act_absmax(p.a_scale)).s * op_scale(*p.w_scale).s;
  bf16x8 fa[2][MB][3], fb[2][NB][3];   // fragment registers, double buffered across the two k-halves
  auto read_frags = [&](const unsigned char* S, int kk, int slot) {
    frag_read<NP, kAPlane, kBPlane>(fa[slot], fb[slot], S, S, fa_off, fb_off, kk);
  };
  auto mfmas = [&](int slot) { frag_mma<NP>(acc, fa[slot], fb[slot]); };

  __syncthreads();
  int g = 0;
  AmaxAcc amax_l{0u, p.out_amax != nullptr};
  for (int i = 0; i < my_tiles; ++i) {
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    for (int kt = 0; kt < nk; ++kt, ++g) {
      const unsigned char* S = smem3 + (g & 1) * kStage;
      read_frags(S, 0, 0);
      read_frags(S, 1, 1);
      mfmas(0);
      mfmas(1);
      __syncthreads();
    }
    const int bid = xcd_remap((int)blockIdx.x + i * (int)gridDim.x, ntiles);
    if constexpr (NP == 2) igemm_scale_acc<MB, NB>(acc, out_scale);
    if (p.bn_part) {
      // statistics mode is launched one tile per workgroup: the staging waves are done (the epilogue's one barrier
      // must not meet a staging wave's step barrier, which it would in a persistent workgroup), every matrix wave
      // has passed the loop's last barrier, and the ring is free to serve as the epilogue's scratch
      igemm_epilogue_stats<MB, NB, WM, WN, WAVES_M, WAVES_N>(p, acc, (bid / p.tiles_n) * BM, (bid % p.tiles_n) * BN, wm, wn,
                                                             li, lh, reinterpret_cast<float*>(smem3 + p.bn_scratch_off));
      continue;
    }
    igemm_epilogue<MB, NB, WM, WN>(p, acc, (bid / p.tiles_n) * BM, (bid % p.tiles_n) * BN, wm, wn, li, lh,
                                   amax_l);
  }
  if (p.out_amax) amax_commit(p.out_amax, amax_l.m);   // once per wave, over all the tiles of this workgroup
}

// Persistent workgroups, and the wave-specialised form also for short reductions (one tile per workgroup with the short
// reductions on the single-role kernel: 3-9 % behind on the K <= 512 layers with Cd >= 128).
int launch_igemm_x3ws(IGemmArgs& a, const ConvRoute& r, hipStream_t stream) {
  EVK_REQUIRE(igemm_x3_supports(a) && r.bm == 128 && r.stages == 2, EVK_E_INVALID, "conv_igemm_x3ws: routed a launch it cannot take");
  EVK_REQUIRE(r.bn == 256 || r.bn == 128 || r.bn == 64, EVK_E_INVALID, "conv_igemm_x3ws: no 128 x %d tile", r.bn);
  a.bn_scratch_off = 0;   // the ring (>= the statistics epilogue's scratch) serves as the scratch
  // one workgroup per CU (LDS), each walking ceil(tiles / 256) tiles; 256 is a multiple of 8, so a workgroup's
  // tiles stay on its XCD under the remap
  // statistics mode: one tile per workgroup (the epilogue parks the tile in the LDS ring, which a persistent
  // workgroup's staging waves would already be refilling)
  auto grid = [&](long long tiles) { return (tiles > 256 && !a.bn_part) ? 256 : tiles; };
  return pick<256, 128, 64>(r.bn, [&](auto BN) {
    return pick_npx(a, [&](auto NPX) {
      constexpr int bn = decltype(BN)::value;
      return launch_igemm_tile<&conv_igemm_x3ws_kernel<128, bn, 2, 2, 2, decltype(NPX)::value>>(
          a, stream, "conv_igemm_x3ws", 128, bn, 2, 512, (size_t)2 * 3 * (128 + bn) * kRowBytes, 0, grid);
    });
  });
}

}  // namespace evk
