// What the three forms of the f16x2 one-tap (1x1, any stride) convolution share — conv1x1_dma.hip (symmetric eight-wave
// ring), conv1x1_sp.hip (software-pipelined, loader waves), conv1x1_ps2.hip (persistent, three wave roles):
//     dst[m][co] = sum_k src[row(m)][k] * w[co][k]      (arithmetic: conv_igemm_x3.hip / x3_common.hpp)
// The files differ in WHO issues the DMA and how a K step is scheduled; the LDS image of a K step, the source offsets that
// produce it, the fragment reads that consume it and the split-and-MFMA of a fragment are ONE contract, kept here.
//
// A stage = one K step (BK3 = 32 reduction channels) of a 128-row x BN-column tile:
//   [0, a_bytes)            activations, 128 rows of 128 bytes: the step's 32 RAW 4-byte words of a pixel — fp32 values, or
//                           the producer's packed (h | l << 16) words — i.e. whole cache lines of the source;
//   [a_bytes, + 2 b_plane)  weights, their two pre-split fp16 planes (h, l), BN rows of 64 bytes each.
// One DMA instruction (lds_dma.hpp) moves 64 lanes x 16 bytes = 1 KB = 8 activation rows or 16 rows of a weight plane, and
// its LDS side is lane-linear.  The conflict-free image is therefore made on the SOURCE side: lane i fetches the chunk that
// belongs at LDS chunk i (c1_a_voff / c1_b_voff apply the XOR of c1_arow_off / plane_off to the source chunk), and the
// fragment reads XOR the same way (c1_frag_off).  Rows past M, columns past Cd and pixels outside the image get the
// out-of-range offset kDmaOOB: the DMA writes zeros.  The K step advances the instruction's SCALAR offset only.
#pragma once
#include "igemm_common.hpp"
#include "x3_common.hpp"
#include "lds_dma.hpp"

namespace evk {

constexpr int kC1BM = 128;       // rows of a tile
constexpr int kC1Row = BK3 * 4;  // bytes of one activation row of a K step (32 four-byte words)

template <int BN>
struct C1Stage {
  static constexpr int a_bytes = kC1BM * kC1Row, b_plane = BN * kRowBytes, bytes = a_bytes + 2 * b_plane;
  // DMA instructions per issuing wave and stage, `waves` waves sharing the issue: activations (8 rows each), weight planes
  static constexpr int a_instr(int waves) { return a_bytes / 1024 / waves; }
  static constexpr int b_instr(int waves) { return 2 * b_plane / 1024 / waves; }
};

__device__ __forceinline__ u32x4 lds_read16(uint32_t lds_byte) {
  return *(const __attribute__((address_space(3))) u32x4*)(uintptr_t)lds_byte;
}
__device__ __forceinline__ void lds_write16(uint32_t lds_byte, f32x4 v) {
  *(__attribute__((address_space(3))) f32x4*)(uintptr_t)lds_byte = v;
}
// byte offset of 16-byte chunk c (0..7) of activation row `row`: rows are 128 B, two per 256-byte bank row; the XOR puts
// the same logical chunk of the 16 rows a ds_read_b128 service group touches on 16 distinct 16-byte slots.  (The weight
// planes' 64-byte rows use plane_off of x3_common.hpp, the same argument with four rows per bank row.)
__device__ __forceinline__ int c1_arow_off(int row, int c) { return row * kC1Row + ((c ^ ((row >> 1) & 7)) << 4); }

// ---- per-lane DMA source offsets of issuing wave `iw` (constant over the K loop).  The argument block is taken BY VALUE:
// through a reference hipcc leaves the loads of Hm, Wm and Cs and their products inside every row's bounds branch (seen
// in the ISA as four multiplies per DMA instruction more); the copy costs nothing in a function that is always inlined.
//
// activations of the row tile at m0: instruction t of the wave moves rows 8 (AI iw + t) .. + 7
template <int AI>
__device__ __forceinline__ void c1_a_voff(const IGemmArgs p, int m0, int iw, int lane, uint32_t (&a_voff)[AI]) {
#pragma unroll
  for (int t = 0; t < AI; ++t) {
    const int row = 8 * (AI * iw + t) + (lane >> 3);  // row of the tile this lane's 16 bytes belong to
    const int c = (lane & 7) ^ ((row >> 1) & 7);      // source chunk that lands on LDS chunk (lane & 7)
    const int m = m0 + row;
    uint32_t off = kDmaOOB;
    if (m < p.M) {
      const int hw = p.Hm * p.Wm;
      const int n = m / hw;
      const int rem = m - n * hw;
      const int gy = rem / p.Wm;
      const int gx = rem - gy * p.Wm;
      const int sy = gy * p.ash + p.oy0, sx = gx * p.asw + p.ox0;
      if ((unsigned)sy < (unsigned)p.Hs && (unsigned)sx < (unsigned)p.Ws)
        off = (uint32_t)(((n * p.Hs + sy) * p.Ws + sx) * p.Cs) * 4u + (uint32_t)c * 16u;
    }
    a_voff[t] = off;
  }
}
// weights of the column tile at n0: instruction t of the wave moves 16-byte slots 64 (BI iw + t) .. + 63
template <int BN, int BI>
__device__ __forceinline__ void c1_b_voff(const IGemmArgs p, int n0, int iw, int lane, uint32_t (&b_voff)[BI]) {
  const uint32_t plane_bytes = (uint32_t)p.Cd * (uint32_t)p.Kpad * 2u;
#pragma unroll
  for (int t = 0; t < BI; ++t) {
    const int s = 64 * (BI * iw + t) + lane;  // 16-byte slot among the stage's 2 * BN * 4 weight slots
    const int pt = s / (BN * 4);
    const int row = (s - pt * BN * 4) >> 2;
    const int c = (s & 3) ^ ((row >> 2) & 3);
    const int co = n0 + row;
    b_voff[t] = co < p.Cd ? (uint32_t)pt * plane_bytes + (uint32_t)co * (uint32_t)p.Kpad * 2u + (uint32_t)c * 16u : kDmaOOB;
  }
}
// scalar offsets of K step kt; the lds_byte of instruction t of wave iw is stage + (AI iw + t) * 1024 for activations,
// stage + a_bytes + (BI iw + t) * 1024 for weights
__device__ __forceinline__ uint32_t c1_a_soff(int kt) { return (uint32_t)kt * kC1Row; }
__device__ __forceinline__ uint32_t c1_b_soff(int kt) { return (uint32_t)kt * kRowBytes; }

// ---- fragment read offsets inside a stage (lane constants) of the lane whose MFMA row is activation row `arow` and
// weight row `brow` of the tile; lh = lane >> 5.  a[k half][16-byte half of the lane's 8 words], b[k half] (plane h; l is
// b_plane further, the wave's next 32 rows 32 rows further: same XOR pattern)
struct C1FragOff {
  uint32_t a[2][2], b[2];
};
template <int BN>
__device__ __forceinline__ C1FragOff c1_frag_off(int arow, int brow, int lh) {
  C1FragOff o;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int h = 0; h < 2; ++h) o.a[kk][h] = (uint32_t)c1_arow_off(arow, 4 * kk + 2 * lh + h);
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) o.b[kk] = (uint32_t)(C1Stage<BN>::a_bytes + plane_off(brow, 2 * kk + lh));
  return o;
}

// ---- operand scales of the launch from the bit images of max|src| and max|weight|, c1_scale(act_absmax(p.a_scale),
// *p.w_scale): 1 / s_a for the split, s_a * s_w for the accumulators at the end
struct C1Scale {
  float a_inv, out;
};
__device__ __forceinline__ C1Scale c1_scale(uint32_t a_absmax, uint32_t w_absmax) {
  const OpScale sa = op_scale(a_absmax), sw = op_scale(w_absmax);
  return C1Scale{sa.inv, sa.s * sw.s};
}

// ---- the fragments of one k half (16 reduction channels) of a wave's MB x 32 rows and NB x 32 columns
template <int NB, int MB = 1>
struct C1Frag {
  u32x4 a[MB][2];          // raw activation words: 8 consecutive k of this lane's row
  bf16x8 b[NB][2];         // weight planes h, l

  // from the stage at LDS byte S, with c1_frag_off's a[kk], b[kk].  S comes through opaque() (lds_dma.hpp), and the offsets
  // stay REFERENCES into the kernel's C1FragOff: how hipcc associates S + offset + immediate — one base register and
  // ds_read offset fields, or a VGPR add per read — follows from where it can see the offset's value, and these two forms
  // give each of the three kernels the K loop it had with the reads written out in place
  template <int BN>
  __device__ __forceinline__ void read(uint32_t S, const uint32_t (&a_off)[2], const uint32_t& b_off) {
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
        b[n][pt] = __builtin_bit_cast(bf16x8, lds_read16(S + b_off + pt * C1Stage<BN>::b_plane + n * 32 * kRowBytes));
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      a[m][0] = lds_read16(S + a_off[0] + m * 32 * kC1Row);
      a[m][1] = lds_read16(S + a_off[1] + m * 32 * kC1Row);
    }
  }
  // split the activation words into their h and l fp16 operands (PK: byte permutes of packed words) and issue the three
  // products, smallest magnitude first.  SPLIT = false is the kernels' timing ablation: the raw words go to the matrix pipe
  template <bool PK, bool SPLIT = true>
  __device__ __forceinline__ void mma(f32x16 (&acc)[MB][NB], float a_inv) const {
    bf16x8 fa[MB][2];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      // (read as floats: a bit_cast of an ext-vector ELEMENT is miscompiled by this hipcc — seen in the ISA as one element
      // used twice; packed words only travel through split_op's scalar bit_cast)
      const f32x4 w0 = __builtin_bit_cast(f32x4, a[m][0]), w1 = __builtin_bit_cast(f32x4, a[m][1]);
      u32x4 H, L;
      uint32_t h, l, unused = 0;
      if constexpr (SPLIT) {
        split_op<2, PK>(w0.x, w0.y, a_inv, h, l, unused); H[0] = h; L[0] = l;
        split_op<2, PK>(w0.z, w0.w, a_inv, h, l, unused); H[1] = h; L[1] = l;
        split_op<2, PK>(w1.x, w1.y, a_inv, h, l, unused); H[2] = h; L[2] = l;
        split_op<2, PK>(w1.z, w1.w, a_inv, h, l, unused); H[3] = h; L[3] = l;
      } else {
        H = a[m][0]; L = a[m][1];
      }
      fa[m][0] = __builtin_bit_cast(bf16x8, H);
      fa[m][1] = __builtin_bit_cast(bf16x8, L);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = mfma_np<2>(b[n][kHB[t]], fa[m][kHA[t]], acc[m][n]);
  }
};

// ---- the double-buffered K step of the loader-wave kernels: the fragment registers live ACROSS the barrier,
//     read k-half 1 | MFMAs of k-half 0 | barrier (the next stage has landed) | read k-half 0 of the next stage | MFMAs of k-half 1
// so every fragment read has a whole MFMA group (192 cycles) to return and the only wait left is the barrier itself.
// read(S, kk, f), mma(f) and barrier() are the kernel's own (they carry its ablation switches); fx holds k-half 0 of stage
// S on entry and of stage Sn on exit.  The LAST step of a kernel has no next stage and is peeled (c1_last_step): a
// conditional read of the next stage would merge two LDS-counter states behind the barrier and make hipcc wait for the
// reads just issued — seen in the ISA as lgkmcnt(1) in front of the second MFMA group.
template <class F, class Read, class Mma, class Barrier>
__device__ __forceinline__ void c1_step(uint32_t S, uint32_t Sn, F& fx, F& fy, Read&& read, Mma&& mma, Barrier&& barrier) {
  read(S, 1, fy);
  __builtin_amdgcn_sched_barrier(0);
  mma(fx);
  __builtin_amdgcn_sched_barrier(0);
  barrier();                                        // stage Sn has landed; fy has returned long ago
  read(Sn, 0, fx);
  __builtin_amdgcn_sched_barrier(0);
  mma(fy);
  __builtin_amdgcn_sched_barrier(0);
}
template <class F, class Read, class Mma, class Barrier>
__device__ __forceinline__ void c1_last_step(uint32_t S, F& fx, F& fy, Read&& read, Mma&& mma, Barrier&& barrier) {
  read(S, 1, fy);
  __builtin_amdgcn_sched_barrier(0);
  mma(fx);
  __builtin_amdgcn_sched_barrier(0);
  barrier();                                        // the loader waves' last barrier
  mma(fy);
}

// ---- host side
// bytes of the two buffer resources.  conv1x1_dma_supports admits a launch only if both fit 31 bits: 32-bit buffer
// offsets, and kDmaOOB above every valid one — which is why the check and every launcher share these two functions
inline unsigned long long c1_src_bytes(const IGemmArgs& a) { return (unsigned long long)a.N * a.Hs * a.Ws * a.Cs * 4ull; }
inline unsigned long long c1_wgt_bytes(const IGemmArgs& a) { return 2ull * a.Cd * a.Kpad * 2ull; }

// launch of a ring kernel (`row_waves` x 2 compute waves, NST stages) through the family's tile launcher, with the two
// buffer sizes as the kernel's extra arguments.  copies: workgroups per tile (2 under conv1x1_dma.hip's K-split timing probe)
template <auto Kern, int BN, int NST>
int launch_c1_ring(IGemmArgs& a, hipStream_t stream, int block, int row_waves, const char* name, int copies = 1) {
  return launch_igemm_tile<Kern>(a, stream, name, kC1BM, BN, row_waves, block, (size_t)NST * C1Stage<BN>::bytes,
                                 igemm_stats_scratch_bytes(row_waves, 2, BN / 2), [&](long long tiles) { return copies * tiles; },
                                 (uint32_t)c1_src_bytes(a), (uint32_t)c1_wgt_bytes(a));
}

}  // namespace evk
