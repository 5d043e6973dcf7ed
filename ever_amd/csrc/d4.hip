// The eight symmetries of the square on NHWC fp32 maps (gfx950), and their fused mean: the device side of test-time
// augmentation (reference magic/transform/segm.py, tta.py).  An op is 3 bits, op = swap | flip_rows << 1 | flip_cols << 2,
// x: [N, Hi, Wi, C] -> y: [N, Ho, Wo, C] with (Ho, Wo) = swap ? (Wi, Hi) : (Hi, Wi) and
//   y[n, r, c, :] = x[n, a, b, :],  r' = flip_rows ? Ho-1-r : r,  c' = flip_cols ? Wo-1-c : c,  (a, b) = swap ? (c', r') : (r', c')
// (transpose first, then flip).  Three kernels each for the copy (d4_apply_*) and the mean (d4_merge_*):
//   element per thread, scalar          any C; a non-swap op maps rows to rows (reversed at most): coalesced both sides
//   element per thread, 16 bytes        C % 4 == 0
//   LDS tile                            swap ops on narrow pixels: a workgroup reads a T x T pixel tile along INPUT rows and
//                                       writes it along OUTPUT rows, full cache lines on both sides, where a direct gather
//                                       reads one 4..32-byte pixel per cache line.
// The tile's row stride S = T*C + pad with S == C (mod 32): the transposed read of output element (rl, cl, ch) is word
// al*S + bl*C + ch with al = cl (or T-1-cl), so the lanes of a 32-lane half, which run over (cl, ch), hit words
// (al + bl)*C + ch (mod 32): consecutive banks (b32 bank = (a/4) mod 32, conflicts within each half only).  This is derived,
// not measured, and it holds while a half stays inside one row of the output tile, i.e. for T*C a multiple of 32 (every
// C <= 4, even C <= 16, C % 4 == 0 above).  For the other widths (5, 21, ...) some halves straddle two rows, where bl changes
// and the words are no longer consecutive; and with a column flip and C not a divisor of 32 a half that starts inside a
// pixel can meet a 2-way conflict.
// The op, the tile plan (T, S, the LDS capacity and its compile-time check), the staging loop and a tile element's index
// arithmetic are in csrc/d4_tile.hpp, shared with csrc/augment.hip.
// Indices are 32-bit: the entry points refuse N*H*W*C >= 2^31.
#include <atomic>
#include "d4_tile.hpp"

namespace evk {

constexpr int kD4MaxTerms = 16;
// Which swap terms take the tile kernel, measured with tools/bench_tta.py on [N, 512, 512, C], an MI355X (table in DESIGN
// 2.14): the tile kernel copies at 3.4-3.7 TB/s whatever C is; the 16-byte element kernel at 3.2 (C = 4), 4.8 (8), 6.0 (16),
// 5.4 (32), 4.9 (64) TB/s; the scalar element kernel at 1.7 (C = 1), 2.3 (3), 2.6 (6) and, forced, 3.0-3.5 (4, 8 ... 64) TB/s.
// So the rule of d4_plan: a swap term whose pixel the 16-byte kernel can take (C % 4 == 0) goes to the tile up to
// kD4TileVecC = 4 floats and to the 16-byte kernel above; a swap term only the scalar kernel could take (C % 4 != 0) goes to
// the tile as far as the tile holds it (C <= kTileMaxC).  Of the widths off the 4-grid only 1, 3 and 6 were timed; that the
// tile stays ahead of the scalar kernel up to 64 rests on the forced rows of C = 8 ... 64 (3.4-3.6 against 3.0-3.5 TB/s).
constexpr int kD4TileVecC = 4;

enum D4Kernel { kD4Scalar = 0, kD4Vec = 1, kD4Tile = 2 };
struct D4Plan {
  int kernel;
  D4TilePlan tile;   // all 0 for the element kernels
};

// Which kernel a term of shape [N, Hi, Wi, C] under `op` takes: pure host arithmetic, shared by evk_d4_apply, evk_d4_merge
// and evk_d4_plan.  evk_d4_force_kernel (tools/bench_tta.py and the tests; nothing in the package calls it) overrides the
// rule wherever the forced kernel is legal.
static std::atomic<int> g_d4_force{-1};
static int d4_plan(int N, int Hi, int Wi, int C, int op, bool ptrs16, D4Plan* pl) {
  EVK_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && C > 0 && op >= 0 && op <= 7, EVK_E_INVALID,
              "d4: bad argument (non-positive size or op outside 0..7)");
  const int64_t total = (int64_t)N * Hi * Wi * C;
  EVK_REQUIRE(total < 0x80000000LL, EVK_E_UNSUPPORTED, "d4: %lld elements (fewer than 2^31 are implemented)", (long long)total);
  const bool swap = op & 1, vec_ok = C % 4 == 0 && ptrs16, tile_ok = swap && C <= kTileMaxC;
  int k = tile_ok && (C % 4 != 0 || C <= kD4TileVecC) ? kD4Tile : vec_ok ? kD4Vec : kD4Scalar;
  const int want = g_d4_force.load(std::memory_order_relaxed);
  if (want == kD4Scalar || (want == kD4Vec && vec_ok) || (want == kD4Tile && tile_ok)) k = want;
  *pl = D4Plan{};
  pl->kernel = k;
  if (k == kD4Tile) pl->tile = d4_tile_plan(C, C);
  return EVK_OK;
}

struct D4Terms {
  const float* t[kD4MaxTerms];
  uint8_t op[kD4MaxTerms];
  uint8_t tile[kD4MaxTerms];     // the term is staged through LDS (tile kernel only)
};

// source offset, in units of V floats, of output element j (V floats of one pixel): one fastdiv chain
struct D4Geom {
  FastDiv fcv, fWo, fHo;    // C / V, Wo, Ho
};
__device__ __forceinline__ uint32_t d4_src(uint32_t j, const D4Geom& g, int op) {
  const uint32_t cv = g.fcv.div, Wo = g.fWo.div, Ho = g.fHo.div;
  const uint32_t pix = fdiv(j, g.fcv), cb = j - pix * cv;
  const uint32_t t = fdiv(pix, g.fWo), c = pix - t * Wo;
  const uint32_t n = fdiv(t, g.fHo), r = t - n * Ho;
  uint32_t a, b;
  d4_source(op, r, c, Ho, Wo, a, b);
  // swap: x is [N, Wo, Ho, C];  else x is [N, Ho, Wo, C]
  const uint32_t spix = (op & 1) ? (n * Wo + a) * Ho + b : (n * Ho + a) * Wo + b;
  return spix * cv + cb;
}

// The copy, an element (V = 1: one word, V = 4: 16 bytes) per thread.  Words, not floats: every bit pattern survives.
template <int V>
__global__ __launch_bounds__(256) void d4_apply_kernel(const uint32_t* __restrict__ x, uint32_t* __restrict__ y, uint32_t nel,
                                                       D4Geom g, int op) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= nel) return;
  const uint32_t s = d4_src(j, g, op);
  if (V == 4)
    *reinterpret_cast<u32x4*>(y + (size_t)j * 4) = *reinterpret_cast<const u32x4*>(x + (size_t)s * 4);
  else
    y[j] = x[s];
}

// The mean, an element per thread: s = (acc or 0.0f) + T_0, s += T_k in index order, y = s / count (a true division) or s.
// y may be acc: element j is read and written by its one owner.  The term tables are indexed by constants (a runtime index
// would put them in scratch), so the loop is unrolled under a uniform guard.
template <int V>
__global__ __launch_bounds__(256) void d4_merge_kernel(const D4Terms a, int nterms, const float* acc, float* y, uint32_t nel,
                                                       D4Geom g, int count) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= nel) return;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (acc) {
    if (V == 4) s = *reinterpret_cast<const f32x4*>(acc + (size_t)j * 4);
    else s.x = acc[j];
  }
#pragma unroll
  for (int k = 0; k < kD4MaxTerms; ++k) {
    if (k < nterms) {
      const uint32_t o = d4_src(j, g, a.op[k]);
      if (V == 4) s = s + *reinterpret_cast<const f32x4*>(a.t[k] + (size_t)o * 4);
      else s.x = s.x + a.t[k][o];
    }
  }
  if (count > 0) {
    const float d = (float)count;
    s.x = __fdiv_rn(s.x, d);
    if (V == 4) { s.y = __fdiv_rn(s.y, d); s.z = __fdiv_rn(s.z, d); s.w = __fdiv_rn(s.w, d); }
  }
  if (V == 4) *reinterpret_cast<f32x4*>(y + (size_t)j * 4) = s;
  else y[j] = s.x;
}

// ---- the tile kernels.  A workgroup owns the T x T output pixels at rows r0.., columns c0.. of image n, i.e. nel = T*T*C
// elements e = rl * T*C + cl * C + ch, element e = tid + 256 * i of thread tid.
struct D4Tile {
  int Ho, Wo, C, T, S;
  FastDiv fC, fTC, fTilesC, fTilesR;    // C, T*C, tiles per output row, tile rows per image
};

// Stage a SWAP term of image n: x's rows are y's columns, so x is [N, Wo, Ho, C].
__device__ __forceinline__ void d4_stage(uint32_t* __restrict__ tile, const uint32_t* __restrict__ x, const D4Tile& g, int op,
                                         int n, int r0, int c0) {
  const uint32_t* xn = x + (size_t)n * g.Wo * g.Ho * g.C;
  d4_tile_stage<kTilePerThread>(tile, op, g.T, g.C, g.S, g.fTC, r0, c0, g.Wo, g.Ho, [xn](uint32_t o) { return xn[o]; });
}
// element e of the output tile: its offset in y (or -1 outside the map) and the word of a staged swap term that holds it
__device__ __forceinline__ bool d4_tile_elem(int e, const D4Tile& g, int n, int r0, int c0, D4TileElem& t, uint32_t& off) {
  t = d4_tile_decode(e, g.T, g.C, g.fTC, g.fC);
  const int r = r0 + t.rl, c = c0 + t.cl;
  off = (((uint32_t)n * g.Ho + r) * g.Wo + c) * g.C + t.ch;      // < 2^31 inside the map, unused outside
  return r < g.Ho && c < g.Wo;
}
__device__ __forceinline__ void d4_tile_origin(const D4Tile& g, int& n, int& r0, int& c0) {
  const uint32_t b = blockIdx.x;
  const uint32_t t = fdiv(b, g.fTilesC), tc = b - t * g.fTilesC.div;
  const uint32_t nn = fdiv(t, g.fTilesR), tr = t - nn * g.fTilesR.div;
  n = (int)nn; r0 = (int)tr * g.T; c0 = (int)tc * g.T;
}

__global__ __launch_bounds__(256) void d4_apply_tile_kernel(const uint32_t* __restrict__ x, uint32_t* __restrict__ y,
                                                            const D4Tile g, int op) {
  __shared__ uint32_t tile[kTileFloats];
  int n, r0, c0;
  d4_tile_origin(g, n, r0, c0);
  d4_stage(tile, x, g, op, n, r0, c0);
  __syncthreads();
  const int nel = g.T * g.T * g.C;
#pragma unroll
  for (int i = 0; i < kTilePerThread; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < nel) {
      D4TileElem t;
      uint32_t off;
      const bool in = d4_tile_elem(e, g, n, r0, c0, t, off);
      const uint32_t v = tile[d4_tile_word(op, g.T, g.S, g.C, t.rl, t.cl, t.ch)];     // the address is computed for every lane, the store masked
      if (in) y[off] = v;
    }
  }
}

// The mean on output tiles: every term takes its own path inside the one launch, a direct read (the non-swap terms, which run
// along the output row: coalesced) or the LDS tile between two barriers (the swap terms: they share C, so they share a plan, and
// this kernel runs only if that plan is the tile); the accumulators (up to 16 per thread) stay in registers.
// The term loop is rolled; its tables are copied to LDS by constant indices first (see d4_merge_kernel).
__global__ __launch_bounds__(256) void d4_merge_tile_kernel(const D4Terms a, int nterms, const float* acc, float* y,
                                                            const D4Tile g, int count) {
  __shared__ uint32_t tile[kTileFloats];
  __shared__ const float* sp[kD4MaxTerms];
  __shared__ uint32_t sop[kD4MaxTerms];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kD4MaxTerms; ++k) {
      sp[k] = a.t[k];
      sop[k] = (uint32_t)a.op[k] | ((uint32_t)a.tile[k] << 8);
    }
  }
  int n, r0, c0;
  d4_tile_origin(g, n, r0, c0);
  const int nel = g.T * g.T * g.C;
  float s[kTilePerThread];
#pragma unroll
  for (int i = 0; i < kTilePerThread; ++i) {
    s[i] = 0.0f;
    const int e = threadIdx.x + 256 * i;
    if (acc && e < nel) {
      D4TileElem t;
      uint32_t off;
      if (d4_tile_elem(e, g, n, r0, c0, t, off)) s[i] = acc[off];
    }
  }
  __syncthreads();
  for (int k = 0; k < nterms; ++k) {
    const float* p = sp[k];
    const int op = (int)(sop[k] & 7u);
    const bool staged = (sop[k] >> 8) != 0;       // uniform over the workgroup: the barriers below are too
    if (staged) {
      __syncthreads();                            // the previous term's readers are done with the tile
      d4_stage(tile, reinterpret_cast<const uint32_t*>(p), g, op, n, r0, c0);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < kTilePerThread; ++i) {
      const int e = threadIdx.x + 256 * i;
      if (e < nel) {
        D4TileElem t;
        uint32_t off;
        const bool in = d4_tile_elem(e, g, n, r0, c0, t, off);
        float v = 0.0f;
        if (staged) {
          v = __uint_as_float(tile[d4_tile_word(op, g.T, g.S, g.C, t.rl, t.cl, t.ch)]);
        } else if (in) {
          int rr, cc;       // a term that is not staged has no swap
          d4_source(op & 6, r0 + t.rl, c0 + t.cl, g.Ho, g.Wo, rr, cc);
          v = p[(((size_t)n * g.Ho + rr) * g.Wo + cc) * g.C + t.ch];
        }
        s[i] = s[i] + v;
      }
    }
  }
  const float d = (float)count;
#pragma unroll
  for (int i = 0; i < kTilePerThread; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < nel) {
      D4TileElem t;
      uint32_t off;
      if (d4_tile_elem(e, g, n, r0, c0, t, off)) y[off] = count > 0 ? __fdiv_rn(s[i], d) : s[i];
    }
  }
}

static D4Geom d4_geom(int Ho, int Wo, int cv) {
  return D4Geom{make_fastdiv((uint32_t)cv), make_fastdiv((uint32_t)Wo), make_fastdiv((uint32_t)Ho)};
}
static D4Tile d4_tile_geom(int N, int Ho, int Wo, int C, const D4Plan& pl, unsigned* grid) {
  const int T = pl.tile.T, tr = (Ho + T - 1) / T, tc = (Wo + T - 1) / T;
  *grid = (unsigned)((int64_t)N * tr * tc);     // <= N*Ho*Wo < 2^31
  return D4Tile{Ho, Wo, C, T, pl.tile.S, make_fastdiv((uint32_t)C), make_fastdiv((uint32_t)(T * C)),
                make_fastdiv((uint32_t)tc), make_fastdiv((uint32_t)tr)};
}

}  // namespace evk

using namespace evk;

extern "C" int evk_d4_plan(int32_t N, int32_t Hi, int32_t Wi, int32_t C, int32_t op, int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "d4_plan: out is a null pointer");
  D4Plan pl;
  const int rc = d4_plan(N, Hi, Wi, C, op, true, &pl);
  if (rc != EVK_OK) return rc;
  const D4TilePlan& t = pl.tile;
  out[0] = pl.kernel; out[1] = t.T; out[2] = t.T; out[3] = t.S; out[4] = t.lds_floats * (int)sizeof(float); out[5] = t.per_thread;
  return EVK_OK;
}

extern "C" int evk_d4_force_kernel(int32_t kernel) {
  return g_d4_force.exchange(kernel >= kD4Scalar && kernel <= kD4Tile ? kernel : -1, std::memory_order_relaxed);
}

extern "C" int evk_d4_apply(const float* x, float* y, int32_t N, int32_t Hi, int32_t Wi, int32_t C, int32_t op, void* stream) {
  EVK_REQUIRE(x && y, EVK_E_INVALID, "d4_apply: null pointer");
  D4Plan pl;
  const int rc = d4_plan(N, Hi, Wi, C, op, aligned16(x) && aligned16(y), &pl);
  if (rc != EVK_OK) return rc;
  const int Ho = (op & 1) ? Wi : Hi, Wo = (op & 1) ? Hi : Wi;
  const uint32_t* xw = reinterpret_cast<const uint32_t*>(x);
  uint32_t* yw = reinterpret_cast<uint32_t*>(y);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t total = (uint32_t)((int64_t)N * Hi * Wi * C);
  if (pl.kernel == kD4Tile) {
    unsigned grid;
    const D4Tile g = d4_tile_geom(N, Ho, Wo, C, pl, &grid);
    hipLaunchKernelGGL(d4_apply_tile_kernel, dim3(grid), dim3(256), 0, st, xw, yw, g, op);
  } else if (pl.kernel == kD4Vec) {
    hipLaunchKernelGGL(d4_apply_kernel<4>, dim3((total / 4 + 255) / 256), dim3(256), 0, st, xw, yw, total / 4,
                       d4_geom(Ho, Wo, C / 4), op);
  } else {
    hipLaunchKernelGGL(d4_apply_kernel<1>, dim3((total + 255) / 256), dim3(256), 0, st, xw, yw, total, d4_geom(Ho, Wo, C), op);
  }
  return check_launch("d4_apply");
}

extern "C" int evk_d4_merge(const float* const* terms, const int32_t* ops, int32_t nterms, const float* acc, float* y, int32_t N,
                            int32_t Ho, int32_t Wo, int32_t C, int32_t count, void* stream) {
  EVK_REQUIRE(terms && ops && y && count >= 0, EVK_E_INVALID, "d4_merge: bad argument (null pointer or negative count)");
  EVK_REQUIRE(nterms >= 1 && nterms <= kD4MaxTerms, EVK_E_UNSUPPORTED, "d4_merge: %d terms (1 to %d per launch)", nterms,
              kD4MaxTerms);
  D4Terms a = {};
  D4Plan pl, tile_pl = {};
  bool al = aligned16(y) && aligned16(acc), any_tile = false, all_vec = true;
  for (int k = 0; k < nterms; ++k) {
    EVK_REQUIRE(terms[k], EVK_E_INVALID, "d4_merge: term %d is a null pointer", k);
    EVK_REQUIRE(terms[k] != y, EVK_E_INVALID, "d4_merge: y may not alias term %d", k);
    al = al && aligned16(terms[k]);
  }
  for (int k = 0; k < nterms; ++k) {
    const int op = ops[k];
    const bool swap = op >= 0 && (op & 1);
    const int rc = d4_plan(N, swap ? Wo : Ho, swap ? Ho : Wo, C, op, al, &pl);    // the term's own dims
    if (rc != EVK_OK) return rc;
    a.t[k] = terms[k];
    a.op[k] = (uint8_t)op;
    a.tile[k] = pl.kernel == kD4Tile;
    if (a.tile[k]) { any_tile = true; tile_pl = pl; }
    all_vec = all_vec && pl.kernel == kD4Vec;
  }
  hipStream_t st = (hipStream_t)stream;
  const uint32_t total = (uint32_t)((int64_t)N * Ho * Wo * C);
  if (any_tile) {
    unsigned grid;
    const D4Tile g = d4_tile_geom(N, Ho, Wo, C, tile_pl, &grid);
    hipLaunchKernelGGL(d4_merge_tile_kernel, dim3(grid), dim3(256), 0, st, a, nterms, acc, y, g, count);
  } else if (all_vec) {
    hipLaunchKernelGGL(d4_merge_kernel<4>, dim3((total / 4 + 255) / 256), dim3(256), 0, st, a, nterms, acc, y, total / 4,
                       d4_geom(Ho, Wo, C / 4), count);
  } else {
    hipLaunchKernelGGL(d4_merge_kernel<1>, dim3((total + 255) / 256), dim3(256), 0, st, a, nterms, acc, y, total,
                       d4_geom(Ho, Wo, C), count);
  }
  return check_launch("d4_merge");
}
