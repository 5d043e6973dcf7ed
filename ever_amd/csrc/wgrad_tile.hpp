// Device pieces the weight-gradient kernels share (conv_wgrad_f32 / _x3 / _x3ws / _tr.hip): the workgroup's tile and split,
// the tap of a k-quad, the pixel decomposition, the 8-pixel micro-block gather with its two load forms, the split into LDS
// planes and the MFMA half step of the register-staged kernels.  Everything is __forceinline__ and takes its tables by
// reference.  The yardstick for a change here is the assembly of the kernels that did not ask for it (tools/vgpr_report.sh
// and a diff of `hipcc -S --cuda-device-only`): conv_wgrad_tr_kernel<1> / <9>, the fp32 tiles and the W8 f16x2 forms of the
// wave-specialised kernel compile to the instructions AND registers they had with this code written out in each of them;
// where a helper did not manage that (WGRAD_PIXEL_RANGE, the fragment offset tables) the note beside it says what it cost.
#pragma once
#include "wgrad_common.hpp"
#include "x3_common.hpp"

#ifndef EVK_WG_ABL
#define EVK_WG_ABL 0   // timing ablations (tools/build_variant.sh -DEVK_WG_ABL=n; wrong results): 1 no loads, 2 no split / LDS writes,
#endif                 // 4 no fragment reads / MFMAs, 8 no stores
namespace evk {
constexpr int kWgAbl = EVK_WG_ABL;

// Workgroup -> split z, tile origin (output channel co0, k column k0) and first pixel pbeg of the split.
// XCD-aware order: all (co, k) tiles of one pixel chunk z run on the same XCD, so the chunk's dy / x rows are fetched
// into ONE L2 instead of eight (PMC: 3.4x the algorithmic bytes with the default order).
// The end of the pixel range and the step count, WGRAD_PIXEL_RANGE, are spelled in the kernel: a function is simplified
// on its own before it is inlined, and `min(M, pbeg + chunk) - pbeg` then takes another form than inside the kernel —
// same values, other loop guards, and the wave-specialised and planar kernels' blocks are laid out differently (measured
// over six alternated rounds: x3ws f16x2 +1.1 %, tr<1> +1.8 %, tr<9> -1.3 %).
struct WGradTile {
  int z, co0, k0, pbeg;
  __device__ __forceinline__ WGradTile(const WGradArgs& p, int bm, int bn) {   // bm x bn: rows / k columns per tile index
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int ntile = p.tiles_co * p.tiles_k;
    z = bid / ntile;
    const int tile = bid - z * ntile;
    const int tile_k = tile % p.tiles_k;
    const int tile_co = tile / p.tiles_k;
    co0 = tile_co * bm;
    k0 = tile_k * bn;
    pbeg = z * p.chunk;
  }
};
// pixels [pbeg, pend) in nk steps of BKP
#define WGRAD_PIXEL_RANGE(p, pbeg)                    \
  const int pend = min((p).M, (pbeg) + (p).chunk);    \
  const int nk = (pend - (pbeg) + BKP - 1) / BKP

// k-quad q (four consecutive k columns) -> its tap's offset into the image and its first input channel
struct WGradTap {
  int offy, offx, coff;
  bool valid;   // q lies inside Ktot
  __device__ __forceinline__ WGradTap(const WGradArgs& p, int q) : offy(0), offx(0), coff(0), valid(q * 4 < p.Ktot) {
    if (valid) {
      const int tap = q / p.cpt;
      coff = (q - tap * p.cpt) * 4;
      const int ky = tap / p.kw, kx = tap - ky * p.kw;
      offy = ky * p.dh - p.ph;
      offx = kx * p.dw - p.pw;
    }
  }
};

// output pixel m (clamped to the last one) -> (n, oy, ox) by two fast divisions
struct WGradPix {
  int n, oy, ox;
  __device__ __forceinline__ WGradPix(const WGradArgs& p, int m) {
    const uint32_t mm = (uint32_t)min(m, p.M - 1);
    const uint32_t un = fdiv(mm, p.fd_hw);
    const uint32_t rem = mm - un * p.fd_hw.div;
    const uint32_t uoy = fdiv(rem, p.fd_w);
    n = (int)un;
    oy = (int)uoy;
    ox = (int)(rem - uoy * p.fd_w.div);
  }
};

// ---- the micro-block gather: 8 consecutive output pixels x one 16-byte (or 8-byte) run of channels
// What a staging thread gathers from: im2col(x) of one tap, or dy (the same gather with unit strides and no offset).
struct WGather {
  int Hs, Ws, Cs, ssh, ssw, offy, offx, coff;
  bool cvalid;
};

// The two load forms.  Offsets are counted in the form's own unit (off()), so a running offset costs one add either way.
typedef float f32x2v __attribute__((ext_vector_type(2)));
struct PtrLoad {   // plain loads from a clamped (valid) address: the caller zeroes what okmask leaves out (zero_masked)
  static constexpr bool kZeroFill = false;
  const float* src;
  __device__ __forceinline__ PtrLoad(const float* t, int /*bytes*/ = 0) : src(t) {}
  static __device__ __forceinline__ int off(int elem) { return elem; }
  template <typename V>
  __device__ __forceinline__ V load(bool ok, int o) const { return *reinterpret_cast<const V*>(src + (ok ? o : 0)); }
};
// Buffer loads (the f16x2 instantiation of the wave-specialised kernel, where they measure faster: staging alone 874 -> 771
// us, whole kernel 1326 -> 1301 / 320 -> 277 / 90 -> 80 us on 3x3x256 @128^2 / 64^2 / 32^2; under bf16x3 they are slower,
// 1567 -> 1726): 32-bit byte offsets on a buffer resource, out-of-image pixels get an out-of-range offset and the hardware
// returns zeros — no 64-bit address arithmetic, no selects on the loaded data.
constexpr uint32_t kOOBOff = 0x80000000u;
struct BufLoad {
  static constexpr bool kZeroFill = true;
  __amdgpu_buffer_rsrc_t rs;
  __device__ __forceinline__ BufLoad(const float* t, int bytes) : rs(__builtin_amdgcn_make_buffer_rsrc((void*)t, 0, bytes, 0x00020000)) {}
  static __device__ __forceinline__ uint32_t off(int elem) { return (uint32_t)elem << 2; }
  template <typename V>
  __device__ __forceinline__ V load(bool ok, uint32_t o) const {
    if constexpr (sizeof(V) == 16) return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(ok ? o : kOOBOff), 0, 0));
    else return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(ok ? o : kOOBOff), 0, 0));
  }
};

// W8: Wo % 8 == 0 (every map of this network): the 8 pixels of a micro-block lie in one image row, one decomposition
// (two fast divisions) per micro-block, running sums for the column and the address.  A W8 instantiation carries no
// code of the per-pixel path — the staging waves are VALU-issue bound (PMC: 83 % VALU-busy with the matrix waves idle).
// Every load is issued whatever the bounds say (branch free), so a prefetch stays in flight under the MFMAs.
template <bool W8, typename Ld>
__device__ __forceinline__ void gather8(const WGradArgs& p, const WGather& g, const Ld& ld, int m0, int pend, f32x4 (&rv)[8],
                                        uint32_t& okmask) {
  okmask = 0;
  if (W8) {
    const WGradPix px(p, m0);
    const int sy = px.oy * g.ssh + g.offy;
    const bool rowok = g.cvalid && m0 < pend && (unsigned)sy < (unsigned)g.Hs;
    int sx = px.ox * g.ssw + g.offx;
    auto off = Ld::off(((px.n * g.Hs + sy) * g.Ws + sx) * g.Cs + g.coff);
    const auto step = Ld::off(g.ssw * g.Cs);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = rowok && (unsigned)sx < (unsigned)g.Ws;
      okmask |= ok ? (1u << j) : 0u;
      rv[j] = ld.template load<f32x4>(ok, off);
      sx += g.ssw;
      off += step;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = m0 + j;
      const WGradPix px(p, m);
      const int sy = px.oy * g.ssh + g.offy, sx = px.ox * g.ssw + g.offx;
      const bool ok = g.cvalid && m < pend && (unsigned)sy < (unsigned)g.Hs && (unsigned)sx < (unsigned)g.Ws;
      okmask |= ok ? (1u << j) : 0u;
      rv[j] = ld.template load<f32x4>(ok, Ld::off(((px.n * g.Hs + sy) * g.Ws + sx) * g.Cs + g.coff));
    }
  }
}
// Half micro-block of dy: 8 pixels x 2 channels (8-byte loads, 512 B contiguous per pixel across a wave).  dy is the
// plain [M][Cout] matrix: no tap, no spatial bound, only the pixel range.
template <typename Ld>
__device__ __forceinline__ void gather8h(const Ld& ld, int Cout, int coff, bool cvalid, int m0, int pend, f32x2v (&rv)[8],
                                         uint32_t& okmask) {
  okmask = 0;
  auto off = Ld::off(m0 * Cout + coff);      // (both tensors are below 2^31 bytes: plan_wgrad's fits32)
  const auto step = Ld::off(Cout);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool ok = cvalid && m0 + j < pend;
    okmask |= ok ? (1u << j) : 0u;
    rv[j] = ld.template load<f32x2v>(ok, off);
    off += step;
  }
}

// zero the pixels of a micro-block that okmask leaves out (PtrLoad; BufLoad's are zero already)
template <typename V>
__device__ __forceinline__ void zero_masked(V (&rv)[8], uint32_t okmask) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool ok = (okmask >> j) & 1u;
#pragma unroll
    for (int e = 0; e < (int)(sizeof(V) / sizeof(float)); ++e) rv[j][e] = ok ? rv[j][e] : 0.f;
  }
}
// split a micro-block of NCH channels and write channel NCH*cq+e to LDS row e*Q + cq, 16-byte chunk pg, of the NP planes
template <int NP, int NCH, bool PK, typename V>
__device__ __forceinline__ void split_store(V (&rv)[8], unsigned char* base, int plane_bytes, int Q, int cq, int pg, float inv) {
#pragma unroll
  for (int e = 0; e < NCH; ++e) {
    const int off = wg_off(e * Q + cq, pg);
    u32x4 H, M, L;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint32_t h, m = 0, l = 0;
      split_op<NP, PK>(rv[2 * t][e], rv[2 * t + 1][e], inv, h, m, l);
      H[t] = h; M[t] = m; L[t] = l;
    }
    *reinterpret_cast<u32x4*>(base + off) = H;
    if (NP >= 2) *reinterpret_cast<u32x4*>(base + plane_bytes + off) = M;
    if (NP == 3) *reinterpret_cast<u32x4*>(base + 2 * plane_bytes + off) = L;
  }
}

// ---- the matrix side.  fa_off[a][kk] / fb_off[b][kk]: byte offset (from A / B) of the 16-byte chunk this lane reads of its
// row in 32-row fragment a / b and k-half kk.  The two kernels fill the tables themselves, four lines each: the row
// formulas differ, and the same formula behind a helper comes out of the compiler with the registers of the f16x2
// wave-specialised kernels renumbered (168 -> 166) and those kernels 0.9 % slower over six alternated rounds.
// one k-half (16 pixels) of a step: fragment reads of the NP planes, then the products of the arithmetic
template <int MB, int NB, int NP>
__device__ __forceinline__ void half_step(f32x16 (&acc)[MB][NB], const unsigned char* A, const unsigned char* B, int a_plane,
                                          int b_plane, const int (&fa_off)[MB][2], const int (&fb_off)[NB][2], int kk) {
  bf16x8 fa[MB][3], fb[NB][3];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int pt = 0; pt < NP; ++pt) fa[a][pt] = *reinterpret_cast<const bf16x8*>(A + pt * a_plane + fa_off[a][kk]);
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int pt = 0; pt < NP; ++pt) fb[b][pt] = *reinterpret_cast<const bf16x8*>(B + pt * b_plane + fb_off[b][kk]);
#pragma unroll
  for (int t = 0; t < X3Prod<NP>::N; ++t)
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = mfma_np<NP>(fa[a][x3_pa(NP, t)], fb[b][x3_pb(NP, t)], acc[a][b]);
}

}  // namespace evk
