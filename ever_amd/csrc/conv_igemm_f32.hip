// Implicit-GEMM convolution (forward and data-gradient) for gfx950 on v_mfma_f32_32x32x2_f32.
//
//   dst[m][co] = sum_k  gather(src)[m][k] * wgt[co][k]      m = (n, gy, gx),  k = (jy, jx, ci)
//
// Replaces aten::convolution / aten::convolution_backward(input) issued by nn.Conv2d at
// reference ever/module/_resnets.py:21-29,149 ; fpn.py:23-37,72-73,165,179 ; fs_relation.py:23-53.
//
// Layout: src NHWC fp32, wgt [Cd][Ktot] (K contiguous, = OHWI), dst NHWC fp32.
// One workgroup = 256 threads = 4 waves computes a BM x BN tile; K advances in steps of 32 floats.
// A (im2col rows) and B (weight rows) are staged global -> VGPR -> LDS as 16-byte chunks, double
// buffered, with the next step's global loads in flight under the current step's MFMAs.  The LDS
// image is [row][8 chunks] with chunk ^= (row>>1)&7 so the ds_read_b128 fragment reads of a
// 16-lane group hit 16 distinct 16-byte slots of the 256-byte bank row.
// Fragment mapping (guide §3): A operand lane l = A[i=l&31][k=l>>5], B lane l = B[k=l>>5][j=l&31];
// one ds_read_b128 per lane supplies k = 8g+4h .. 8g+4h+3, i.e. four consecutive MFMAs.
// C/D: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5); the MFMA is issued as W_tile x X_tile^T so
// that rows = output channels (4 consecutive per lane and register quad => 16-byte stores).
//
// ONE gather form serves every use: source pixel of GEMM row (n, gy, gx) and tap (jy, jx) is
//     sy = gy*ash + oy0 + jy*oys ,   sx = gx*asw + ox0 + jx*oxs            (affine in the tap index)
//   forward            ash = stride, oy0 = -pad,  oys = dilation
//   dgrad, stride 1    ash = 1,      oy0 = +pad,  oys = -dilation          (taps are not flipped: the
//                                                                           sign of oys does it)
//   dgrad, stride s    one launch per residue class (cy, cx) of the input pixel mod s: only the taps
//                      with (cy + pad - ky*dil) % s == 0 reach that class, they are ky = ky0 + j*kstep
//                      and their source row is gy + (cy+pad-ky0*dil)/s - j*dil/g : again affine.  No
//                      MFMA is spent on the (s*s-1)/(s*s) structurally-zero products.
// The gather is branch-free: every 16-byte load is issued from a clamped (valid) 32-bit element
// offset and the zero fill is applied when the chunk is written to LDS, after the MFMA block, so the
// prefetch stays in flight under the MFMAs.
// Row decode, K cursor and gather are igemm_tile.hpp's, shared with the split kernels; host side and C ABI: conv_igemm.hip.
#include "conv_route.hpp"
#include "igemm_tile.hpp"
#include "smallm_body.hpp"

namespace evk {

constexpr int BK = 32;

template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const IGemmArgs p) {
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MB = WM / 32, NB = WN / 32;
  constexpr int AR = BM / 32, BR = BN / 32;  // rows per thread for the A / B staging passes
  static_assert(WAVES_M * WAVES_N == 4, "4 waves");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                  // [2][BM][32]
  float* Bs = smem + 2 * BM * BK;    // [2][BN][32]

  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_n = bid % p.tiles_n;
  const int tile_m = bid / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const int tid = threadIdx.x;
  const int c8 = tid & 7;   // chunk column inside the K step
  const int rb = tid >> 3;  // base row 0..31

  // ---- per-thread gather state for its A rows
  IGemmRows<AR> rows;
#pragma unroll
  for (int j = 0; j < AR; ++j) rows.decode(p, j, m0 + rb + 32 * j);
  // B rows: element offset of this thread's chunk in step 0, or -1 past Cd
  int b_off[BR];
#pragma unroll
  for (int j = 0; j < BR; ++j) {
    const int co = n0 + rb + 32 * j;
    b_off[j] = (co < p.Cd) ? co * p.Ktot + c8 * 4 : -1;
  }

  // K-chunk cursor of this thread: chunk q = kt*8 + c8  ->  (ky, kx, cc)
  IGemmCursor<8> cur;
  cur.seek(c8, p.cpt, p.kw);

  f32x4 ra[AR][1], rbv[BR];
  uint32_t okmask = 0;  // bit j: A row j valid; bit 16+j: B row j valid (for the chunk held in ra / rbv)

  auto load_tiles = [&](int kt) {
    const bool kvalid = cur.ky < p.kh;
    okmask = igemm_gather<4>(p, rows, cur, ra);
#pragma unroll
    for (int j = 0; j < BR; ++j) {
      const bool ok = kvalid && b_off[j] >= 0;
      okmask |= ok ? (1u << (16 + j)) : 0u;
      rbv[j] = *reinterpret_cast<const f32x4*>(p.wgt + (ok ? b_off[j] + kt * BK : 0));
    }
    cur.advance(kt, c8, p.cpt, p.kw);
  };

  auto store_tiles = [&](int buf) {
    float* Ab = As + buf * BM * BK;
    float* Bb = Bs + buf * BN * BK;
#pragma unroll
    for (int j = 0; j < AR; ++j) {
      const int row = rb + 32 * j;
      const int pc = c8 ^ ((row >> 1) & 7);
      const bool ok = (okmask >> j) & 1u;
      f32x4 v = ra[j][0];
      v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
      *reinterpret_cast<f32x4*>(Ab + row * BK + pc * 4) = v;
    }
#pragma unroll
    for (int j = 0; j < BR; ++j) {
      const int row = rb + 32 * j;
      const int pc = c8 ^ ((row >> 1) & 7);
      const bool ok = (okmask >> (16 + j)) & 1u;
      f32x4 v = rbv[j];
      v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
      *reinterpret_cast<f32x4*>(Bb + row * BK + pc * 4) = v;
    }
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

  const int nk = (p.Ktot + BK - 1) / BK;

  load_tiles(0);
  store_tiles(0);
  __syncthreads();

  // One K step.  The staging work of the NEXT tile is threaded through this tile's MFMA groups so
  // that it issues in the shadow of the matrix pipe (an in-order wave can issue VALU / VMEM / LDS
  // right behind an MFMA while that MFMA occupies the pipe for 64 cycles):
  //   g0 | address math + 8 global loads (tile kt+1) | g1 | g2 | vmcnt + zero-fill + 8 ds_write | g3 | barrier
  // Writing buffer buf^1 during the step is safe: its last readers passed the previous barrier.
  auto mfma_group = [&](const float* Ab, const float* Bb, int g) {
    f32x4 fa[MB], fb[NB];
#pragma unroll
    for (int a = 0; a < MB; ++a) {
      const int row = wm * WM + a * 32 + li;
      const int pc = (2 * g + lh) ^ ((row >> 1) & 7);
      fa[a] = *reinterpret_cast<const f32x4*>(Ab + a * 32 * BK + pc * 4);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int row = wn * WN + b * 32 + li;
      const int pc = (2 * g + lh) ^ ((row >> 1) & 7);
      fb[b] = *reinterpret_cast<const f32x4*>(Bb + b * 32 * BK + pc * 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int a = 0; a < MB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[b][j], fa[a][j], acc[a][b], 0, 0, 0);
  };

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    const float* Ab = As + buf * BM * BK + (wm * WM + li) * BK;
    const float* Bb = Bs + buf * BN * BK + (wn * WN + li) * BK;
    mfma_group(Ab, Bb, 0);
    if (more) load_tiles(kt + 1);
    mfma_group(Ab, Bb, 1);
    mfma_group(Ab, Bb, 2);
    if (more) store_tiles(buf ^ 1);
    mfma_group(Ab, Bb, 3);
    __syncthreads();
  }

  igemm_epilogue<MB, NB, WM, WN>(p, acc, m0, n0, wm, wn, li, lh);
}

template <int BM, int BN, int WAVES_M, int WAVES_N>
static int launch_cfg(IGemmArgs& a, hipStream_t stream) {   // (no statistics epilogue: the LDS is the two-stage ring)
  return launch_igemm_tile<&conv_igemm_kernel<BM, BN, WAVES_M, WAVES_N>>(a, stream, "conv_igemm", BM, BN, 0, 256,
                                                                         (size_t)2 * (BM + BN) * BK * sizeof(float), 0);
}

// 1x1 convolution on a handful of rows (the FS-Relation scene MLP on 1x1 maps: M = batch, K up to
// 2048; reference fs_relation.py:23-29).  An MFMA tile would be >90 % padding and latency bound on a
// 64-step K loop in 2-4 workgroups; here one workgroup owns one output column and all rows, streams
// its weight row once with 16-byte loads and reduces across the block.
__global__ __launch_bounds__(256) void conv1x1_smallm_kernel(const float* __restrict__ src,
                                                             const float* __restrict__ wgt,
                                                             const float* __restrict__ bias, float* __restrict__ dst,
                                                             int M, int K, int Cd, int relu) {
  smallm_column(src, wgt, bias, dst, M, K, Cd, relu, blockIdx.x);   // (smallm_body.hpp: shared with relation_scene.hip)
}

static int check_fp32_sizes(const IGemmArgs& a) {
  const long long src_elems = (long long)a.N * a.Hs * a.Ws * a.Cs;
  const long long wgt_elems = (long long)a.Cd * a.Ktot;
  EVK_REQUIRE(src_elems < 0x7fffffffLL && wgt_elems < 0x7fffffffLL, EVK_E_UNSUPPORTED,
              "conv_igemm: tensors of 2^31 or more elements are not supported (%lld / %lld)", src_elems, wgt_elems);
  return EVK_OK;
}

bool conv1x1_smallm_supports(const IGemmArgs& a) {
  return a.kh == 1 && a.kw == 1 && a.M <= kSmallM && a.dense_dst && !a.accum && a.ash == 1 && a.asw == 1 && a.oy0 == 0 &&
         a.ox0 == 0 && a.Hm == a.Hs && a.Wm == a.Ws;
}

int launch_conv1x1_smallm(IGemmArgs& a, const ConvRoute&, hipStream_t stream) {
  if (int rc = check_fp32_sizes(a)) return rc;
  EVK_REQUIRE(conv1x1_smallm_supports(a), EVK_E_INVALID, "conv1x1_smallm: routed a launch it cannot take");
  hipLaunchKernelGGL(conv1x1_smallm_kernel, dim3(a.Cd), dim3(256), 0, stream, a.src, a.wgt, a.bias, a.dst, a.M, a.Ktot, a.Cd,
                     a.relu);
  return check_launch("conv1x1_smallm");
}

int launch_igemm(IGemmArgs& a, const ConvRoute& r, hipStream_t stream) {
  if (int rc = check_fp32_sizes(a)) return rc;
  switch (r.bm * 1000 + r.bn) {
    case 256064: return launch_cfg<256, 64, 4, 1>(a, stream);
    case 128064: return launch_cfg<128, 64, 2, 2>(a, stream);
    case 64064: return launch_cfg<64, 64, 2, 2>(a, stream);
    case 128128: return launch_cfg<128, 128, 2, 2>(a, stream);
    case 64128: return launch_cfg<64, 128, 2, 2>(a, stream);
  }
  EVK_REQUIRE(false, EVK_E_INVALID, "conv_igemm: no %d x %d tile", r.bm, r.bn);
}

}  // namespace evk
