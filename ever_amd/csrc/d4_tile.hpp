// What the dihedral kernels of csrc/d4.hip (test-time augmentation) and csrc/augment.hip (input preparation) share: the op, the
// plan of the T x T pixel LDS tile a swap op is staged through, the staging loop, and the index arithmetic of a tile element.
// The LDS arrays are declared in the kernels; why the row stride S keeps the transposed read off bank conflicts is derived there.
#pragma once
#include "common.hpp"

namespace evk {

// ---- the op: 3 bits, swap | flip_rows << 1 | flip_cols << 2, transpose first, then flip.  Output pixel (r, c) of the Ho x Wo
// map is source pixel (a, b): row a, column b of a map that is Wo x Ho under a swap op and Ho x Wo otherwise.
template <typename I>
__host__ __device__ __forceinline__ void d4_source(int op, I r, I c, I Ho, I Wo, I& a, I& b) {
  const I rr = (op & 2) ? Ho - 1 - r : r, cc = (op & 4) ? Wo - 1 - c : c;
  a = (op & 1) ? cc : rr;
  b = (op & 1) ? rr : cc;
}

// ---- the tile plan
constexpr int kTileMaxC = 64;        // widest pixel the tile kernels hold
constexpr int kTileFloats = 5120;    // the kernels' LDS tile: T * S floats fit (checked below)
constexpr int kTilePerThread = 16;   // the tile kernels' elements (accumulators) per thread of 256: T*T*C / 256 fits

struct D4TilePlan {
  int T, S, lds_floats, per_thread;    // T x T pixels of C floats, S floats per tile row; T * S; ceil(T*T*C / 256)
};
constexpr int d4_tile_edge(int C) { return C <= 4 ? 32 : C <= 16 ? 16 : 8; }
// S is the least stride >= T*C with S == residue (mod 32): residue C where the lanes run over (column, channel), NHWC; 1 where
// they run over columns alone, NCHW.
constexpr D4TilePlan d4_tile_plan(int C, int residue) {
  const int T = d4_tile_edge(C), TC = T * C, S = TC + (((residue - TC) % 32) + 32) % 32;
  return D4TilePlan{T, S, T * S, (T * TC + 255) / 256};
}
constexpr bool d4_tile_plans_fit() {
  for (int C = 1; C <= kTileMaxC; ++C)
    for (int residue = 0; residue < 32; ++residue) {      // every stride the rule can give; C and 1 (mod 32) are among them
      const D4TilePlan p = d4_tile_plan(C, residue);
      if (p.lds_floats > kTileFloats || p.per_thread > kTilePerThread) return false;
    }
  return true;
}
static_assert(d4_tile_plans_fit(), "a tile of d4_tile_plan is larger than kTileFloats, or gives a thread more than kTilePerThread");

// ---- a tile element, returned by value: reference outputs put augment_tile_kernel's in scratch (profiles/d4_shared_resources.txt)
struct D4TileElem {
  int rl, cl, ch;    // tile row, tile column, channel
};
// element e = (rl * T + cl) * C + ch of a pixel-major tile
__device__ __forceinline__ D4TileElem d4_tile_decode(int e, int T, int C, const FastDiv& fTC, const FastDiv& fC) {
  const int rl = (int)fdiv((uint32_t)e, fTC), kk = e - rl * T * C;
  const int cl = (int)fdiv((uint32_t)kk, fC);
  return D4TileElem{rl, cl, kk - cl * C};
}
// element e = (ch * T + rl) * T + cl of a plane-major tile
__device__ __forceinline__ D4TileElem d4_tile_decode_planar(int e, int T, const FastDiv& fTT, const FastDiv& fT) {
  const int ch = (int)fdiv((uint32_t)e, fTT), p = e - ch * T * T, rl = (int)fdiv((uint32_t)p, fT);
  return D4TileElem{rl, p - rl * T, ch};
}
// the staged word of output tile element (rl, cl, ch): input row al, input pixel bl of the tile.  A label tile is C = 1, ch = 0.
__device__ __forceinline__ int d4_tile_word(int op, int T, int S, int C, int rl, int cl, int ch) {
  const int al = (op & 4) ? T - 1 - cl : cl, bl = (op & 2) ? T - 1 - rl : rl;
  return al * S + bl * C + ch;
}

// Stage the source pixels of a SWAP term that the T x T output tile at rows r0.., columns c0.. of the transformed map reads:
// source rows alo .. alo+T-1 (the source's rows are the transformed map's columns), pixels blo .. blo+T-1, read as T runs of
// T*C consecutive words.  The source is Hi x Wi pixels of C words and load(o) is word o of it; what lies outside it (a ragged
// tile, a crop window past the source) is stored as 0.  256 threads, PER_THREAD >= T*T*C / 256 words each; a barrier follows in
// the caller.
template <int PER_THREAD, typename Word, typename Load>
__device__ __forceinline__ void d4_tile_stage(Word* __restrict__ tile, int op, int T, int C, int S, const FastDiv& fTC, int r0,
                                              int c0, int Hi, int Wi, Load load) {
  const int TC = T * C, nel = T * TC;
  const int alo = (op & 4) ? Hi - c0 - T : c0;
  const int blo = (op & 2) ? Wi - r0 - T : r0;
#pragma unroll
  for (int i = 0; i < PER_THREAD; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < nel) {
      const int ra = (int)fdiv((uint32_t)e, fTC), kk = e - ra * TC;
      const int arow = alo + ra, f = blo * C + kk;
      Word v = 0;
      if (arow >= 0 && arow < Hi && f >= 0 && f < Wi * C) v = load((uint32_t)arow * Wi * C + f);
      tile[ra * S + kk] = v;
    }
  }
}

}  // namespace evk
