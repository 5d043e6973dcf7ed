// Device pieces the implicit-GEMM forward / data-gradient kernels share (conv_igemm_f32 / _x3 / _x3ws.hip): the decode of a
// thread's GEMM rows, its K-chunk cursor, the branch-free gather, the split of gathered rows into LDS planes, the weight
// planes' way through registers, and the fragment read and products of the split arithmetics (DESIGN.md 2.1 lists them
// and what stayed in the kernels).  Everything is
// __forceinline__.  What stays in the kernels is what differs between them: how loads, stores and MFMAs are scheduled
// against each other (the fp32 kernel threads the staging through its four MFMA groups, the single-role split kernel has
// one LDS stage and two barriers per step, the wave-specialised one two register sets and a two-stage ring) and the
// persistent tile walk.  The yardstick for a change here is the same as in wgrad_tile.hpp: registers, LDS, scratch and
// instruction counts of every instantiation (tools/vgpr_report.sh and a diff of `hipcc -S --cuda-device-only`).
#pragma once
#include "igemm_common.hpp"
#include "x3_common.hpp"

namespace evk {

constexpr int kInvalidRow = -(1 << 28);  // y0 of a row past M: every tap fails the bounds test

// Source pixel of tap (0, 0) for the AR GEMM rows a thread stages: row m = (n, gy, gx) of the Hm x Wm row grid reads source
// pixel (gy * ash + oy0, gx * asw + ox0); base = its element offset (valid or not: the gather tests).
// decode() takes ONE row and the loop over the thread's rows stays in the kernel: a function is simplified on its own before
// it is inlined, and the loop inside it came out of the compiler with the divisions arranged differently (fp32 <64, 64>:
// 56 -> 58 VGPRs, the split kernels +-6).
template <int AR>
struct IGemmRows {
  int y0[AR], x0[AR], base[AR];
  __device__ __forceinline__ void decode(const IGemmArgs& p, int j, int m) {
    if (m < p.M) {
      const int hw = p.Hm * p.Wm;
      const int n = m / hw;
      const int rem = m - n * hw;
      const int gy = rem / p.Wm;
      const int gx = rem - gy * p.Wm;
      y0[j] = gy * p.ash + p.oy0;
      x0[j] = gx * p.asw + p.ox0;
      base[j] = ((n * p.Hs + y0[j]) * p.Ws + x0[j]) * p.Cs;
    } else {
      y0[j] = kInvalidRow;
      x0[j] = 0;
      base[j] = 0;
    }
  }
};

// K-chunk cursor of a thread: chunk q of the reduction -> tap (ky, kx) and chunk cc inside the tap; a K step is CPS chunks
// (8 four-float chunks in the fp32 kernel, 4 eight-float chunks in the split kernels)
template <int CPS>
struct IGemmCursor {
  int cc, kx, ky;
  __device__ __forceinline__ void seek(int q, int chunks_per_tap, int kw) {
    const int tap = q / chunks_per_tap;
    cc = q - tap * chunks_per_tap;
    ky = tap / kw;
    kx = tap - ky * kw;
  }
  // from step kt to step kt + 1 of the thread whose chunk inside a step is c (wave-uniform branch on the channel count)
  __device__ __forceinline__ void advance(int kt, int c, int chunks_per_tap, int kw) {
    if (chunks_per_tap >= CPS) {
      cc += CPS;
      const bool wrap = cc >= chunks_per_tap;
      cc = wrap ? cc - chunks_per_tap : cc;
      kx += wrap ? 1 : 0;
      const bool wrapx = kx == kw;
      kx = wrapx ? 0 : kx;
      ky += wrapx ? 1 : 0;
    } else {  // narrow inputs: a step spans several taps
      seek((kt + 1) * CPS + c, chunks_per_tap, kw);
    }
  }
};

// The gather of one K step: chunk (cursor) of every row, CF floats per chunk.  Branch free: every 16-byte load is issued
// from a clamped (valid) 32-bit element offset and the zero fill is applied when the chunk goes to LDS, so the prefetch
// stays in flight under the MFMAs.  Returns the mask of rows whose tap lies inside the source (bit j = row j).
template <int CF, int AR, int CPS>
__device__ __forceinline__ uint32_t igemm_gather(const IGemmArgs& p, const IGemmRows<AR>& r, const IGemmCursor<CPS>& k,
                                                 f32x4 (&ra)[AR][CF / 4]) {
  uint32_t okmask = 0;
  const bool kvalid = k.ky < p.kh;
  const int oy = k.ky * p.oys, ox = k.kx * p.oxs;
  const int tapoff = (oy * p.Ws + ox) * p.Cs + k.cc * CF;
#pragma unroll
  for (int j = 0; j < AR; ++j) {
    const int sy = r.y0[j] + oy, sx = r.x0[j] + ox;
    const bool ok = kvalid && (unsigned)sy < (unsigned)p.Hs && (unsigned)sx < (unsigned)p.Ws;
    okmask |= ok ? (1u << j) : 0u;
    const float* src = p.src + (ok ? r.base[j] + tapoff : 0);
#pragma unroll
    for (int h = 0; h < CF / 4; ++h) ra[j][h] = *reinterpret_cast<const f32x4*>(src + 4 * h);
  }
  return okmask;
}

// ---- the split kernels' staging: a thread owns 16-byte chunk c4 of LDS rows rb + 64 j
// gathered rows -> zero fill, split into the NP planes (plane_bytes apart), one 16-byte store per plane
template <int NP, bool PK, int AR>
__device__ __forceinline__ void split_store_rows(const f32x4 (&ra)[AR][2], uint32_t okmask, unsigned char* Ab, int plane_bytes,
                                                 int rb, int c4, float a_inv) {
#pragma unroll
  for (int j = 0; j < AR; ++j) {
    const int off = plane_off(rb + 64 * j, c4);
    const bool ok = (okmask >> j) & 1u;
    u32x4 H, M, L;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x4 v = ra[j][e >> 1];
      const float x0 = ok ? v[2 * (e & 1)] : 0.f, x1 = ok ? v[2 * (e & 1) + 1] : 0.f;
      uint32_t h, m = 0, l = 0;
      split_op<NP, PK>(x0, x1, a_inv, h, m, l);
      H[e] = h; M[e] = m; L[e] = l;
    }
    *reinterpret_cast<u32x4*>(Ab + off) = H;
    if (NP >= 2) *reinterpret_cast<u32x4*>(Ab + plane_bytes + off) = M;
    if (NP == 3) *reinterpret_cast<u32x4*>(Ab + 2 * plane_bytes + off) = L;
  }
}
// The pre-split weight planes [3][Cd][Kpad] go global -> VGPR -> LDS with no VALU work.  Rows past Cd re-read the last row
// (their columns are never stored); K is zero padded in HBM.
template <int BR>
__device__ __forceinline__ void weight_rows_decode(const IGemmArgs& p, int first_row, int c4, int (&b_off)[BR]) {
#pragma unroll
  for (int j = 0; j < BR; ++j) {
    int co = first_row + 64 * j;
    co = co < p.Cd ? co : p.Cd - 1;
    b_off[j] = co * p.Kpad + c4 * 8;
  }
}
template <int NP, int BR>
__device__ __forceinline__ void weight_rows_load(const IGemmArgs& p, const int (&b_off)[BR], int plane, int kt, u32x4 (&rbv)[BR][3]) {
#pragma unroll
  for (int j = 0; j < BR; ++j)
#pragma unroll
    for (int pt = 0; pt < NP; ++pt)
      rbv[j][pt] = *reinterpret_cast<const u32x4*>(p.wgt3 + (size_t)pt * plane + b_off[j] + kt * BK3);
}
template <int NP, int BR>
__device__ __forceinline__ void weight_rows_store(const u32x4 (&rbv)[BR][3], unsigned char* Bb, int plane_bytes, int rb, int c4) {
#pragma unroll
  for (int j = 0; j < BR; ++j) {
    const int off = plane_off(rb + 64 * j, c4);
#pragma unroll
    for (int pt = 0; pt < NP; ++pt) *reinterpret_cast<u32x4*>(Bb + pt * plane_bytes + off) = rbv[j][pt];
  }
}

// ---- the split kernels' matrix side.  Fragment: lane l holds row l & 31, k = 16 kk + 8 (l >> 5) .. + 7 (one ds_read_b128)
// for A and B alike.  fa_off[f][kk] / fb_off[f][kk]: byte offset (plane_off) of that chunk for the lane's row in 32-row
// fragment f and k-half kk.  The kernels fill the two tables themselves, four lines each: behind a helper the same formula
// cost the single-role kernel registers (<64, 64, .., 3>: 68 -> 74 VGPRs, <128, 128, .., 1>: 152 -> 154) — what
// wgrad_tile.hpp found for its tables.
// The fragments of one k-half (16 reduction elements) and their products.  The MFMAs are issued as W_tile x X_tile^T
// (igemm_common.hpp: a lane then holds four consecutive output channels of one pixel), smallest magnitude first.  Two
// functions on the kernel's own arrays: the wave-specialised kernel double-buffers the fragments across the k-halves and
// calls them through two one-line lambdas (called directly, or as members of a fragment struct, they cost its <128, 64>
// forms 108 -> 136 VGPRs).  The weight-gradient kernels' half_step
// (wgrad_tile.hpp) is the same shape with the operands the other way round and stays its own: its kernels' assembly is
// the yardstick there.
template <int NP, int A_PLANE, int B_PLANE, int MB, int NB>   // (bytes between planes)
__device__ __forceinline__ void frag_read(bf16x8 (&fa)[MB][3], bf16x8 (&fb)[NB][3], const unsigned char* A, const unsigned char* B,
                                          const int (&fa_off)[MB][2], const int (&fb_off)[NB][2], int kk) {
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int pt = 0; pt < NP; ++pt) fa[a][pt] = *reinterpret_cast<const bf16x8*>(A + pt * A_PLANE + fa_off[a][kk]);
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int pt = 0; pt < NP; ++pt) fb[b][pt] = *reinterpret_cast<const bf16x8*>(B + pt * B_PLANE + fb_off[b][kk]);
}
template <int NP, int MB, int NB>
__device__ __forceinline__ void frag_mma(f32x16 (&acc)[MB][NB], const bf16x8 (&fa)[MB][3], const bf16x8 (&fb)[NB][3]) {
#pragma unroll
  for (int t = 0; t < X3Prod<NP>::N; ++t)
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = mfma_np<NP>(fb[b][x3_pb(NP, t)], fa[a][x3_pa(NP, t)], acc[a][b]);
}

}  // namespace evk
