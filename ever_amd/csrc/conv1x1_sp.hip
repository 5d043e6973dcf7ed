// One-tap (1x1, any stride) convolutions of the f16x2 arithmetic, forward and data gradient, SOFTWARE-PIPELINED with LOADER
// WAVES:   dst[m][co] = sum_k src[row(m)][k] * w[co][k]      (arithmetic: conv_igemm_x3.hip / x3_common.hpp)
//
// Round 5.  conv1x1_dma.hip moves both operands global -> LDS by DMA, but its K step is
//     wait(DMA) | barrier | issue DMA | read 6 fragments | WAIT | 6 MFMA | read 6 fragments | WAIT | 6 MFMA
// (seen in its ISA: four exposed `s_waitcnt lgkmcnt(0)` per step): the LDS latency, the DMA issue (~60-100 cycles per
// instruction in the issuing wave's in-order stream) and the barrier all ADD to the 12 MFMAs.  Measured on 1024 -> 256 @32^2
// (tools/ab_c1_small.py, us): everything 35.9, the K loop with no DMA and no stores 26.0 — against 10.3 for its MFMAs at
// the matrix pipe's nominal rate; the DMA alone 19.1.  Two more facts from tools/probes/dma_issue.hip + dma_patterns.hip:
// a CU takes ~32-40 outstanding 1 KB vector-memory instructions, the wave that issues the next one BLOCKS until one
// returns; and the streaming rate of LDS-DMA scales with the number of ISSUING waves (2 waves: 3.0 TB/s chip-wide at any
// depth, 4: 5.8, 8: 7.1), not with the access pattern (128-byte row segments 4 KB apart = whole rows).  Hence:
//  * the eight compute waves (4 x 2, 32 x BN/2 each) issue NO vector-memory instruction inside the K loop; four LOADER waves
//    issue the whole ring (the LDS image, its source offsets and fragment reads: c1_tile.hpp, shared with conv1x1_dma.hip)
//    and absorb the queue's back-pressure;
//  * the fragment registers are double-buffered ACROSS the barrier (c1_tile.hpp: c1_step); this needs stage kt+1 complete
//    one half step early: ring of NST = 4 stages, NST - 1 in flight;
//  * no run-time ablation switch inside the loop (compile-time EVK_SP_ABL: 1 no loader DMA, 4 no compute, 8 no stores).
// Epilogues: the shared ones of igemm_common.hpp; the loader waves end before them (an ended wave is not waited for).
#include "conv_route.hpp"
#include "c1_tile.hpp"
#include <stdlib.h>
#include <string.h>

#ifndef EVK_SP_ABL
#define EVK_SP_ABL 0
#endif

namespace evk {

namespace {

constexpr int kSpCW = 8;   // compute waves

// (ablations 16: no barrier; 32: the fragments are read once, in front of the loop; 64: no operand split / byte permutes)
__device__ __forceinline__ void sp_barrier() { if (!(EVK_SP_ABL & 16)) ring_barrier(); }

}  // namespace

// LW loader waves (4); NST ring stages
template <int BN, bool PK, int NST, int LW>
__global__ __launch_bounds__(64 * (kSpCW + LW)) void conv1x1_sp_kernel(const IGemmArgs p, uint32_t src_bytes, uint32_t wgt_bytes) {
  constexpr int BM = kC1BM, WAVES_M = 4, WAVES_N = 2, WM = 32, WN = BN / 2, NB = WN / 32;
  using St = C1Stage<BN>;
  constexpr int kStage = St::bytes;
  constexpr int AI = St::a_instr(LW), BI = St::b_instr(LW), PER = AI + BI;   // DMA instructions per loader wave and stage
  static_assert(LW == 4 && AI >= 1 && BI >= 1 && NB >= 1 && NST >= 3, "tile shape");
  static_assert((NST - 2) * PER <= 62, "vmcnt range");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_sp[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int ntiles = p.tiles_m * p.tiles_n;
  const int bid = xcd_remap((int)blockIdx.x, ntiles);
  const int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nk = p.Kpad / BK3;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_sp;

  if (wave >= kSpCW) {
    // ================================================================== loader waves
    const int lw = wave - kSpCW;
    const i32x4 rs_a = make_rsrc(p.src, src_bytes), rs_b = make_rsrc(p.wgt3, wgt_bytes);
    uint32_t a_voff[AI], b_voff[BI];
    c1_a_voff<AI>(p, m0, lw, lane, a_voff);
    c1_b_voff<BN, BI>(p, n0, lw, lane, b_voff);
    auto issue = [&](int kt, uint32_t S) {
      if (EVK_SP_ABL & 1) return;
      const uint32_t ka = c1_a_soff(kt), kb = c1_b_soff(kt);
#pragma unroll
      for (int t = 0; t < AI; ++t) dma16s_loader(rs_a, S + (AI * lw + t) * 1024, a_voff[t], ka);
#pragma unroll
      for (int t = 0; t < BI; ++t) dma16s_loader(rs_b, S + St::a_bytes + (BI * lw + t) * 1024, b_voff[t], kb);
    };
    // prologue: stages 0 .. NST-2 in flight
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
      if (s < nk) issue(s, lds0 + s * kStage);
    // stage 0 landed: at most the later prologue stages outstanding (fewer than NST - 2 of them exist when nk is short: the
    // count is then an over-estimate of what may stay in flight only if nk - 1 < NST - 2, handled by the full wait)
    if (nk - 1 >= NST - 2) wait_vmcnt<(NST - 2) * PER>(); else wait_vmcnt<0>();
    sp_barrier();                                   // P0
    uint32_t S_i = lds0 + (NST - 1) * kStage;         // slot of stage kt + NST - 1 (= the slot stage kt - 1 has left)
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + NST - 1 < nk) issue(kt + NST - 1, S_i);
      S_i = S_i == lds0 + (NST - 1) * kStage ? lds0 : S_i + kStage;
      // stage kt + 1 landed: the younger stages may stay in flight — NST - 2 of them, fewer in the tail
      const int younger = nk - 2 - kt;                // stages kt + 2 .. nk - 1 exist
      if (younger >= NST - 2) wait_vmcnt<(NST - 2) * PER>();
      else if (NST > 3 && younger == 1) wait_vmcnt<PER>();
      else wait_vmcnt<0>();
      sp_barrier();                                 // B(kt)
    }
    return;
  }

  // ==================================================================== compute waves
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;
  const C1FragOff fo = c1_frag_off<BN>(wm * WM + li, wn * WN + li, lh);
  const C1Scale sc = c1_scale(act_absmax(p.a_scale), *p.w_scale);
  f32x16 acc[1][NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][b][r] = 0.f;

  using Frag = C1Frag<NB>;
  auto read_frag_now = [&](uint32_t S, int kk, Frag& f) { f.template read<BN>(S, fo.a[kk], fo.b[kk]); };
  auto read_frag = [&](uint32_t S, int kk, Frag& f) {
    if (!(EVK_SP_ABL & 32)) read_frag_now(S, kk, f);
  };
  auto mma = [&](const Frag& f) { f.template mma<PK, !(EVK_SP_ABL & 64)>(acc, sc.a_inv); };

  Frag fx, fy;
  sp_barrier();                                     // P0: stage 0 has landed
  uint32_t S_c = lds0;
  if (!(EVK_SP_ABL & 4)) read_frag_now(opaque(S_c), 0, fx);
  if (EVK_SP_ABL & 32) read_frag_now(opaque(S_c), 1, fy);
  for (int kt = 0; kt + 1 < nk; ++kt) {
    const uint32_t S = opaque(S_c);
    S_c = S_c == lds0 + (NST - 1) * kStage ? lds0 : S_c + kStage;
    const uint32_t Sn = opaque(S_c);
    if (EVK_SP_ABL & 4) {
      sp_barrier();
      continue;
    }
    c1_step(S, Sn, fx, fy, read_frag, mma, sp_barrier);   // its barrier is B(kt)
  }
  if (EVK_SP_ABL & 4) {
    sp_barrier();
  } else {
    c1_last_step(opaque(S_c), fx, fy, read_frag, mma, sp_barrier);   // B(nk - 1)
  }
  if (EVK_SP_ABL & 8) {   // (every accumulator register stays live: nothing of the loop may be optimised away)
    float sum = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) sum += acc[0][b][r];
    if (sum == 12345.f) p.dst[0] = 0.f;
    return;
  }
  igemm_scale_acc<1, NB>(acc, sc.out);
  if (p.bn_part) {
    __syncthreads();   // the ring becomes the statistics epilogue's scratch: every compute wave is done reading the last stage
    igemm_epilogue_stats<1, NB, WM, WN, WAVES_M, WAVES_N>(p, acc, m0, n0, wm, wn, li, lh, reinterpret_cast<float*>(smem_sp));
    return;
  }
  AmaxAcc amax_l{0u, p.out_amax != nullptr};
  igemm_epilogue<1, NB, WM, WN>(p, acc, m0, n0, wm, wn, li, lh, amax_l);
  if (p.out_amax) amax_commit(p.out_amax, amax_l.m);
}

template <int BN, bool PK, int NST>
static int launch_sp(IGemmArgs& a, hipStream_t stream) {
  constexpr int LW = 4;
  return launch_c1_ring<&conv1x1_sp_kernel<BN, PK, NST, LW>, BN, NST>(a, stream, 64 * (kSpCW + LW), 4, "conv1x1_sp");
}

bool conv1x1_sp_supports(const IGemmArgs& a) { return conv1x1_dma_supports(a) && a.Kpad / BK3 >= 2; }

// column tile 128 / 64 with a ring of four or three stages
int launch_conv1x1_sp(IGemmArgs& a, const ConvRoute& r, hipStream_t stream) {
  EVK_REQUIRE(conv1x1_sp_supports(a), EVK_E_UNSUPPORTED,
              "conv1x1_sp: shape not supported (1x1, Cs %% 32 == 0, Cs >= 64, f16x2 arithmetic)");
  switch (r.bn * 10 + r.stages) {
    case 1284: return a.a_packed ? launch_sp<128, true, 4>(a, stream) : launch_sp<128, false, 4>(a, stream);
    case 644: return a.a_packed ? launch_sp<64, true, 4>(a, stream) : launch_sp<64, false, 4>(a, stream);
    case 1283: return a.a_packed ? launch_sp<128, true, 3>(a, stream) : launch_sp<128, false, 3>(a, stream);
    case 643: return a.a_packed ? launch_sp<64, true, 3>(a, stream) : launch_sp<64, false, 3>(a, stream);
  }
  EVK_REQUIRE(false, EVK_E_INVALID, "conv1x1_sp: no %d-wide tile with %d stages", r.bn, r.stages);
}

}  // namespace evk
