// One-tap (1x1, any stride) convolutions of the f16x2 arithmetic, forward and data gradient, with BOTH operands moved
// global -> LDS by DMA:   dst[m][co] = sum_k src[row(m)][k] * w[co][k]      (arithmetic: conv_igemm_x3.hip / x3_common.hpp)
//
// These layers are HBM-bound (64..2048 reduction channels, 0.2-0.3 of their byte bound in the register-staged
// kernels, whose one step of look-ahead leaves 16-32 KB per CU in flight against the ~64 KB that 8 TB/s x ~2 us of latency
// asks of each of 256 CUs).  Here
//  * the LDS image of a K step, the source offsets that make it and the fragment reads are c1_tile.hpp's, shared with
//    conv1x1_sp.hip and conv1x1_ps2.hip;
//  * ring of three stages (48 KB each at 128 x 256), two steps = up to 96 KB per CU in flight, counted vmcnt, raw
//    s_barrier; the DMA is inline asm (lds_dma.hpp: the builtin makes hipcc drain it before every LDS read);
//  * the split of an fp32 activation happens on the fragment a lane has just read (8 floats -> h, l fp16x8: 4 packed
//    converts + 4 subtract pairs + 4 packed converts), once per 32 rows x BN/2 columns, in the shadow of the other wave of
//    the SIMD's MFMAs; a packed operand needs 8 byte permutes;
//  * eight symmetric waves, 4 (rows) x 2 (column halves), two per SIMD: each issues its eighth of the step's DMA, reads
//    its own fragments and owns 32 rows x BN/2 columns of the tile.
// Epilogue: the shared ones of igemm_common.hpp (bias / accumulate (+ ReLU bits) / ReLU / operand-scale slots, or the
// BatchNorm statistics form through LDS, which reuses the ring).
#include "conv_route.hpp"
#include "c1_tile.hpp"
#include <stdlib.h>
#include <string.h>

#ifndef EVK_C1_DMA_ABL
#define EVK_C1_DMA_ABL 0   // timing ablations (tools/build_variant.sh -DEVK_C1_DMA_ABL=n; wrong results): 1 no activation DMA, 2 no weight
#endif                     // DMA, 4 no compute, 8 no stores, 16 every tile twice with half of the K loop each
namespace evk {

template <int BN, bool PK, int NST, int WAVES_M>
__global__ __launch_bounds__(128 * WAVES_M) void conv1x1_dma_kernel(const IGemmArgs p, uint32_t src_bytes, uint32_t wgt_bytes) {
  constexpr int dbg = EVK_C1_DMA_ABL;
  constexpr int BM = kC1BM, WAVES_N = 2, NW = WAVES_M * WAVES_N, WM = BM / WAVES_M, MB = WM / 32, WN = BN / 2, NB = WN / 32;
  static_assert(NST == 2 || NST == 3, "ring depth");
  static_assert(WAVES_M == 4 || WAVES_M == 2, "row waves");
  using St = C1Stage<BN>;
  constexpr int AI = St::a_instr(NW), BI = St::b_instr(NW), PER = AI + BI;   // DMA instructions per wave and stage
  static_assert(AI >= 2 && BI >= 1 && NB >= 1 && MB >= 1, "tile shape");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_c1[];

  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;
  const int ntiles = p.tiles_m * p.tiles_n;
  // (timing probe, dbg & 16: the grid is doubled and each copy of a tile runs one half of the K loop — what a split of the
  // reduction over two co-resident workgroups would cost per half; results are garbage)
  const int khalf = (dbg & 16) ? (int)blockIdx.x >= ntiles : 0;
  const int bid = xcd_remap((int)blockIdx.x - khalf * ntiles, ntiles);
  const int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nk_all = p.Kpad / BK3;
  const int kbeg = (dbg & 16) ? khalf * (nk_all / 2) : 0;
  const int nk = (dbg & 16) ? kbeg + nk_all / 2 : nk_all;

  const i32x4 rs_a = make_rsrc(p.src, src_bytes), rs_b = make_rsrc(p.wgt3, wgt_bytes);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_c1;

  // ---- per-lane DMA source offsets (constant over the K loop; the K step advances the scalar offset)
  uint32_t a_voff[AI], b_voff[BI];
  c1_a_voff<AI>(p, m0, wave, lane, a_voff);
  c1_b_voff<BN, BI>(p, n0, wave, lane, b_voff);

  auto issue = [&](int kt, int slot) {
    const uint32_t S = lds0 + slot * St::bytes;
    const uint32_t ka = c1_a_soff(kt), kb = c1_b_soff(kt);
    if (!(dbg & 1)) {
#pragma unroll
      for (int t = 0; t < AI; ++t) dma16s(rs_a, S + (AI * wave + t) * 1024, a_voff[t], ka);
    }
    if (!(dbg & 2)) {
#pragma unroll
      for (int t = 0; t < BI; ++t) dma16s(rs_b, S + St::a_bytes + (BI * wave + t) * 1024, b_voff[t], kb);
    }
  };

  const C1FragOff fo = c1_frag_off<BN>(wm * WM + li, wn * WN + li, lh);
  const C1Scale sc = c1_scale(act_absmax(p.a_scale), *p.w_scale);

  f32x16 acc[MB][NB];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // ---- prologue: NST - 1 steps in flight
  issue(kbeg, 0);
  if (NST == 3 && nk > kbeg + 1) issue(kbeg + 1, 1);

  int slot = 0;
  for (int kt = kbeg; kt < nk; ++kt) {
    // my DMA of step kt has landed when at most the next step's instructions are outstanding; after the barrier
    // everybody's has, and everybody is done reading the stage that step kt + 2 overwrites (read in step kt - 1)
    if (NST == 3 && kt + 1 < nk) {
      wait_vmcnt<PER>();
    } else {
      wait_vmcnt<0>();
    }
    ring_barrier();
    if (kt + NST - 1 < nk) issue(kt + NST - 1, slot == 0 ? NST - 1 : slot - 1);
    const uint32_t S = opaque(lds0 + slot * St::bytes);
    slot = slot == NST - 1 ? 0 : slot + 1;
    if (dbg & 4) continue;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      C1Frag<NB, MB> f;
      f.template read<BN>(S, fo.a[kk], fo.b[kk]);
      f.template mma<PK>(acc, sc.a_inv);
    }
  }
  if (dbg & 8) {
    if (acc[0][0][0] == 12345.f) p.dst[0] = 0.f;
    return;
  }
  igemm_scale_acc<MB, NB>(acc, sc.out);
  if (p.bn_part) {
    __syncthreads();   // the ring becomes the statistics epilogue's scratch: every wave is done reading the last stage
    igemm_epilogue_stats<MB, NB, WM, WN, WAVES_M, WAVES_N>(p, acc, m0, n0, wm, wn, li, lh, reinterpret_cast<float*>(smem_c1));
    return;
  }
  AmaxAcc amax_l{0u, p.out_amax != nullptr};
  igemm_epilogue<MB, NB, WM, WN>(p, acc, m0, n0, wm, wn, li, lh, amax_l);
  if (p.out_amax) amax_commit(p.out_amax, amax_l.m);
}

template <int BN, bool PK, int NST, int WAVES_M>
static int launch_c1(IGemmArgs& a, hipStream_t stream) {
  return launch_c1_ring<&conv1x1_dma_kernel<BN, PK, NST, WAVES_M>, BN, NST>(a, stream, 128 * WAVES_M, WAVES_M, "conv1x1_dma",
                                                                           (EVK_C1_DMA_ABL & 16) ? 2 : 1);
}

template <int BN, int NST, int WAVES_M = 4>
static int launch_c1_pk(IGemmArgs& a, hipStream_t stream) {
  return a.a_packed ? launch_c1<BN, true, NST, WAVES_M>(a, stream) : launch_c1<BN, false, NST, WAVES_M>(a, stream);
}

bool conv1x1_dma_supports(const IGemmArgs& a) {
  if (a.planes != 2 || a.kh != 1 || a.kw != 1 || (a.Cs & 31) != 0 || a.Kpad != a.Cs) return false;
  return c1_src_bytes(a) < 0x80000000ull && c1_wgt_bytes(a) < 0x80000000ull;  // 32-bit buffer offsets, kDmaOOB above every valid one
}

// column tile 256 / 128 / 64 with a ring of three stages (one workgroup per CU), or 128 / 64 with two (two per CU)
int launch_conv1x1_dma(IGemmArgs& a, const ConvRoute& r, hipStream_t stream) {
  EVK_REQUIRE(conv1x1_dma_supports(a), EVK_E_UNSUPPORTED, "conv1x1_dma: shape not supported (1x1, Cs %% 32 == 0, f16x2 arithmetic)");
  switch (r.bn * 10 + r.stages) {
    case 2563: return launch_c1_pk<256, 3>(a, stream);
    case 1283: return launch_c1_pk<128, 3>(a, stream);
    case 643: return launch_c1_pk<64, 3>(a, stream);
    case 1282: return launch_c1_pk<128, 2>(a, stream);
    case 642: return launch_c1_pk<64, 2>(a, stream);
  }
  EVK_REQUIRE(false, EVK_E_INVALID, "conv1x1_dma: no %d-wide tile with %d stages", r.bn, r.stages);
}

}  // namespace evk
