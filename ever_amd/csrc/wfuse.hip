// The learned weighted fusion node of a BiFPN (reference fpn.py:196-224, 281-309) as ONE pass each way on NHWC fp32 (gfx950):
//   y = ((w^0 t0 + w^1 t1) + w^2 t2) + w^3 t3,   w^ = fast_normalize(w) = relu(w) / (sum relu(w) + eps)  or  softmax(w)
// with w the RAW [K] parameter on the device (normalised inside the kernels: no read-back, no launch for three floats) and
// term k read at its own resolution: a shift-1 term enters output pixel (y, x) as its pixel (y >> 1, x >> 1), the
// UpsamplingNearest2d in front of the node as an index shift.  The reference's form (materialised up-sampling, stack,
// broadcast multiply, sum) writes and reads K + 1 more maps than this one.
// Backward, one launch over dy: a thread owns one 2 x 2 quad of output pixels at one 16-byte channel chunk (one element on a
// map with an odd side, where no term can be shifted), writes w^ dy for the same-resolution terms and the quad's sum of w^ dy
// for the shifted ones — one owner per output element, a fixed order — and, when the weight gradient is wanted, reads every
// term once and keeps d_k = sum dy up(t_k) as one fp32 partial per term over its run of kWfRun quads.  A wave butterfly and
// an LDS tree make one record per workgroup, a second, one-workgroup launch adds the records in double, in index order,
// and applies the Jacobian of the normalisation: no float atomics, the same bits every run.
// 16-byte accesses along the channel axis (C % 4 == 0) throughout.
#include "stream_common.hpp"

// a * b + c stays two roundings here: the shifted term's gradient (w^ g00 + w^ g01) + (w^ g10 + w^ g11) is then bit for
// bit what the same-resolution form followed by the unit-weight block sum gives.  The dots ask for their fmaf by name.
#pragma clang fp contract(off)

namespace evk {

constexpr int kWfMaxTerms = 4, kWfThreads = 256;
constexpr int kWfRunQuad = 4, kWfRunElem = 16;     // items a backward thread walks: 16 elements = 64 floats per partial either way
constexpr int kWfDepth = 64;                       // D: products one thread adds serially into one partial

struct WfTerms {
  const float* t[kWfMaxTerms];    // [N, H >> shift, W >> shift, C]
  float* d[kWfMaxTerms];          // its gradient, or null (backward only)
  int32_t shift[kWfMaxTerms];
};

struct WfPlan {
  int quad;              // the backward's item is a 2 x 2 quad (H and W even) or one element
  int run;               // items per backward thread
  int64_t items;         // quads or elements, each at one 16-byte channel chunk
  int64_t grid;          // workgroups of the backward = records of the dots
  int64_t ws_bytes;      // records [grid][4] fp32, then the four dots as fp32
};

// pure host arithmetic, shared by the launchers, evk_wfuse_plan and evk_wfuse_workspace_bytes
static int wfuse_plan(const char* what, int N, int H, int W, int C, int nterms, WfPlan* pl) {
  EVK_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, EVK_E_INVALID, "%s: bad argument (null pointer or non-positive size)", what);
  EVK_REQUIRE(nterms >= 1 && nterms <= kWfMaxTerms, EVK_E_UNSUPPORTED, "%s: %d terms (1 to %d are implemented)", what, nterms,
              kWfMaxTerms);
  EVK_REQUIRE(C % 4 == 0, EVK_E_UNSUPPORTED, "%s: C = %d must be a multiple of 4", what, C);
  const int64_t n4 = (int64_t)N * H * W * (C / 4);
  EVK_REQUIRE(n4 < 0x7fffffffLL - 64, EVK_E_UNSUPPORTED, "%s: %lld 16-byte elements (fewer than 2^31 are implemented)", what,
              (long long)n4);
  pl->quad = H % 2 == 0 && W % 2 == 0;
  pl->run = pl->quad ? kWfRunQuad : kWfRunElem;
  pl->items = pl->quad ? n4 / 4 : n4;
  const int64_t share = (int64_t)kWfThreads * pl->run;
  pl->grid = (pl->items + share - 1) / share;
  pl->ws_bytes = (pl->grid * kWfMaxTerms + kWfMaxTerms) * (int64_t)sizeof(float);
  return EVK_OK;
}

// w^ from the raw parameter, by every thread for itself (K scalar loads, K expf at most)
template <int NT>
__device__ __forceinline__ void wfuse_normalise(const float* __restrict__ w, int norm, float eps, float (&wh)[NT]) {
  if (!w) {
#pragma unroll
    for (int k = 0; k < NT; ++k) wh[k] = 1.f;
    return;
  }
  float r[NT], s = 0.f;
  if (norm == 0) {
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const float v = w[k];
      r[k] = v > 0.f ? v : (v == v ? 0.f : v);      // relu; a NaN stays one
      s = k == 0 ? r[k] : s + r[k];
    }
    s = s + eps;
  } else {
    float m = w[0];
#pragma unroll
    for (int k = 1; k < NT; ++k) m = fmaxf(m, w[k]);
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      r[k] = expf(w[k] - m);
      s = k == 0 ? r[k] : s + r[k];
    }
  }
#pragma unroll
  for (int k = 0; k < NT; ++k) wh[k] = r[k] / s;
}

__device__ __forceinline__ f32x4 wf_scale(float a, const f32x4 v) { return f32x4{a * v.x, a * v.y, a * v.z, a * v.w}; }
__device__ __forceinline__ float wf_dot(float p, const f32x4 g, const f32x4 t) {
  return fmaf(g.w, t.w, fmaf(g.z, t.z, fmaf(g.y, t.y, fmaf(g.x, t.x, p))));
}

// One thread per 16-byte element j of y.  NT is a template parameter so that the term tables are indexed by constants
// (a runtime index would put them in scratch).
template <int NT>
__global__ __launch_bounds__(kWfThreads) void wfuse_fwd_kernel(const WfTerms a, const float* __restrict__ weights, int norm,
                                                               float eps, float* __restrict__ y, uint32_t n4, FastDiv fc4,
                                                               FastDiv fW, FastDiv fH, int C) {
  const uint32_t j = blockIdx.x * (uint32_t)kWfThreads + threadIdx.x;
  if (j >= n4) return;
  float wh[NT];
  wfuse_normalise<NT>(weights, norm, eps, wh);
  const NhwcElem e = nhwc_elem(j, fc4, fW, fH);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const size_t ek = a.shift[k] == 0 ? (size_t)j : coarse_elem(e, fH.div, fW.div, (size_t)(C >> 2), 1);
    const f32x4 p = wf_scale(wh[k], ld4(a.t[k], ek));     // a zero weight still multiplies: an infinity gives its NaN
    v = k == 0 ? p : v + p;
  }
  st4(y, j, v);
}

// The backward.  Item i is, with QUAD, the quad (n, qy, qx) at channel chunk cb — its index among the quads is also the
// element index of a shifted term — and otherwise element i.  Workgroup b walks items [b * 256 * RUN, (b + 1) * 256 * RUN),
// 256 consecutive ones at a time.  DW: the dots are wanted.
template <int NT, bool QUAD, bool DW>
__global__ __launch_bounds__(kWfThreads) void wfuse_bwd_kernel(const WfTerms a, const float* __restrict__ dy,
                                                               const float* __restrict__ weights, int norm, float eps,
                                                               float* __restrict__ records, uint32_t nitems, FastDiv fc4,
                                                               FastDiv fWq, int W) {
  constexpr int RUN = QUAD ? kWfRunQuad : kWfRunElem;
  float wh[NT], p[NT];
  wfuse_normalise<NT>(weights, norm, eps, wh);
#pragma unroll
  for (int k = 0; k < NT; ++k) p[k] = 0.f;
  const uint32_t c4 = fc4.div;
  for (int it = 0; it < RUN; ++it) {
    const uint32_t i = (blockIdx.x * (uint32_t)RUN + it) * kWfThreads + threadIdx.x;
    if (i >= nitems) break;
    if (QUAD) {
      const uint32_t q = fdiv(i, fc4), cb = i - q * c4;
      const uint32_t r = fdiv(q, fWq), qx = q - r * fWq.div;     // r = n * (H / 2) + qy: row 2 r of the [N * H, W] pixel grid
      const Quad e = quad_elems((size_t)r * 2, 2 * qx, W, c4, cb);
      const f32x4 g00 = ld4(dy, e.e00), g01 = ld4(dy, e.e01), g10 = ld4(dy, e.e10), g11 = ld4(dy, e.e11);
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        if (a.shift[k] == 0) {
          if (a.d[k]) {
            st4(a.d[k], e.e00, wf_scale(wh[k], g00)); st4(a.d[k], e.e01, wf_scale(wh[k], g01));
            st4(a.d[k], e.e10, wf_scale(wh[k], g10)); st4(a.d[k], e.e11, wf_scale(wh[k], g11));
          }
          if (DW) p[k] = wf_dot(wf_dot(wf_dot(wf_dot(p[k], g00, ld4(a.t[k], e.e00)), g01, ld4(a.t[k], e.e01)),
                                       g10, ld4(a.t[k], e.e10)), g11, ld4(a.t[k], e.e11));
        } else {
          if (a.d[k])
            st4(a.d[k], i, quad_sum(wf_scale(wh[k], g00), wf_scale(wh[k], g01), wf_scale(wh[k], g10), wf_scale(wh[k], g11)));
          if (DW) {
            const f32x4 t = ld4(a.t[k], i);
            p[k] = wf_dot(wf_dot(wf_dot(wf_dot(p[k], g00, t), g01, t), g10, t), g11, t);
          }
        }
      }
    } else {
      const f32x4 g = ld4(dy, i);
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        if (a.d[k]) st4(a.d[k], i, wf_scale(wh[k], g));
        if (DW) p[k] = wf_dot(p[k], g, ld4(a.t[k], i));
      }
    }
  }
  if (DW) {
    __shared__ float sw[kWfThreads / kWave][kWfMaxTerms];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const float s = wave_sum(p[k]);          // a butterfly: every lane ends with the same bits
      if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kWfMaxTerms) {
      const int k = threadIdx.x;
      records[(size_t)blockIdx.x * kWfMaxTerms + k] = k < NT ? (sw[0][k] + sw[1][k]) + (sw[2][k] + sw[3][k]) : 0.f;
    }
  }
}

// One workgroup: thread t adds its contiguous slice of the records in index order, in double; an LDS tree over the 256
// slices in a fixed order; thread 0 leaves the dots (fp32, behind the records) and the gradient of the RAW weights.
__global__ __launch_bounds__(kWfThreads) void wfuse_dw_finalize_kernel(const float* __restrict__ records, uint32_t nrec,
                                                                       int nterms, const float* __restrict__ weights, int norm,
                                                                       float eps, float* __restrict__ dots,
                                                                       float* __restrict__ dweights) {
  __shared__ double sd[kWfThreads][kWfMaxTerms];
  const uint32_t per = (nrec + kWfThreads - 1) / kWfThreads, tid = threadIdx.x;
  const uint32_t lo = tid * per, hi = lo + per < nrec ? lo + per : nrec;
  double s[kWfMaxTerms] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t b = lo; b < hi; ++b) {
    const f32x4 rec = ld4(records, b);
    s[0] += (double)rec.x; s[1] += (double)rec.y; s[2] += (double)rec.z; s[3] += (double)rec.w;
  }
#pragma unroll
  for (int k = 0; k < kWfMaxTerms; ++k) sd[tid][k] = s[k];
  __syncthreads();
  for (int o = kWfThreads / 2; o > 0; o >>= 1) {
    if ((int)tid < o) {
#pragma unroll
      for (int k = 0; k < kWfMaxTerms; ++k) sd[tid][k] += sd[tid + o][k];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  double d[kWfMaxTerms], w[kWfMaxTerms], wh[kWfMaxTerms], S = 0.0, m = 0.0;
  for (int k = 0; k < kWfMaxTerms; ++k) {
    d[k] = k < nterms ? sd[0][k] : 0.0;
    w[k] = k < nterms ? (double)weights[k] : 0.0;
    dots[k] = (float)d[k];
  }
  if (norm == 0) {
    for (int k = 0; k < nterms; ++k) { wh[k] = w[k] > 0.0 ? w[k] : (w[k] == w[k] ? 0.0 : w[k]); S += wh[k]; }
    S += (double)eps;
  } else {
    double mx = w[0];
    for (int k = 1; k < nterms; ++k) mx = fmax(mx, w[k]);
    for (int k = 0; k < nterms; ++k) { wh[k] = exp(w[k] - mx); S += wh[k]; }
  }
  for (int k = 0; k < nterms; ++k) { wh[k] = wh[k] / S; m += wh[k] * d[k]; }
  for (int k = 0; k < nterms; ++k) {
    // fast_normalize: [w_j > 0] (d_j - m) / (sum relu(w) + eps), ReLU's derivative at 0 is 0;  softmax: w^_j (d_j - m)
    const double g = norm == 0 ? (w[k] > 0.0 ? (d[k] - m) / S : 0.0) : wh[k] * (d[k] - m);
    dweights[k] = (float)g;
  }
}

static int wfuse_terms(const char* what, const float* const* terms, const int32_t* shifts, float* const* dterms, int nterms,
                       int H, int W, WfTerms* a) {
  const int rc = check_terms(what, terms, shifts, nterms, 1, H, W);
  if (rc != EVK_OK) return rc;
  for (int k = 0; k < nterms; ++k) {
    a->t[k] = terms ? terms[k] : nullptr;
    a->d[k] = dterms ? dterms[k] : nullptr;
    a->shift[k] = shifts[k];
  }
  return EVK_OK;
}

}  // namespace evk

using namespace evk;

extern "C" int evk_wfuse_plan(int32_t N, int32_t H, int32_t W, int32_t C, int32_t nterms, int32_t* out) {
  EVK_REQUIRE(out, EVK_E_INVALID, "wfuse_plan: out is a null pointer");
  WfPlan pl;
  const int rc = wfuse_plan("wfuse_plan", N, H, W, C, nterms, &pl);
  if (rc != EVK_OK) return rc;
  EVK_REQUIRE(pl.ws_bytes < 0x7fffffffLL, EVK_E_UNSUPPORTED, "wfuse_plan: workspace of %lld bytes", (long long)pl.ws_bytes);
  out[0] = (int32_t)pl.grid; out[1] = kWfThreads; out[2] = kWfDepth; out[3] = (int32_t)pl.ws_bytes;
  out[4] = pl.quad; out[5] = pl.run; out[6] = (int32_t)(pl.grid * kWfMaxTerms); out[7] = 0;
  return EVK_OK;
}

extern "C" size_t evk_wfuse_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t nterms) {
  WfPlan pl;
  return wfuse_plan("wfuse_workspace_bytes", N, H, W, C, nterms, &pl) == EVK_OK ? (size_t)pl.ws_bytes : 0;
}

extern "C" int evk_wfuse_fwd(const float* const* terms, const int32_t* shifts, int32_t nterms, const float* weights,
                             int32_t norm, float eps, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
  EVK_REQUIRE(terms && shifts && y, EVK_E_INVALID, "wfuse_fwd: bad argument (null pointer or non-positive size)");
  WfPlan pl;
  int rc = wfuse_plan("wfuse_fwd", N, H, W, C, nterms, &pl);
  if (rc != EVK_OK) return rc;
  EVK_REQUIRE(norm == 0 || norm == 1, EVK_E_UNSUPPORTED, "wfuse_fwd: norm = %d (0 fast_normalize, 1 softmax)", norm);
  WfTerms a = {};
  rc = wfuse_terms("wfuse_fwd", terms, shifts, nullptr, nterms, H, W, &a);
  if (rc != EVK_OK) return rc;
  const uint32_t n4 = (uint32_t)((int64_t)N * H * W * (C / 4));
  const dim3 grid((n4 + kWfThreads - 1) / kWfThreads), block(kWfThreads);
  const FastDiv fc4 = make_fastdiv((uint32_t)(C / 4)), fW = make_fastdiv((uint32_t)W), fH = make_fastdiv((uint32_t)H);
  return pick<1, 2, 3, 4>(nterms, [&](auto NT) {
    hipLaunchKernelGGL(wfuse_fwd_kernel<NT()>, grid, block, 0, (hipStream_t)stream, a, weights, norm, eps, y, n4, fc4, fW, fH, C);
    return check_launch("wfuse_fwd");
  });
}

extern "C" int evk_wfuse_bwd(const float* dy, const float* const* terms, const int32_t* shifts, int32_t nterms,
                             const float* weights, int32_t norm, float eps, float* const* dterms, float* dweights,
                             void* workspace, int64_t workspace_bytes, int32_t N, int32_t H, int32_t W, int32_t C,
                             void* stream) {
  EVK_REQUIRE(dy && shifts && dterms && (!dweights || (terms && weights && workspace && ((uintptr_t)workspace & 15u) == 0)),
              EVK_E_INVALID,
              "wfuse_bwd: bad argument (null pointer or non-positive size)");
  WfPlan pl;
  int rc = wfuse_plan("wfuse_bwd", N, H, W, C, nterms, &pl);
  if (rc != EVK_OK) return rc;
  EVK_REQUIRE(norm == 0 || norm == 1, EVK_E_UNSUPPORTED, "wfuse_bwd: norm = %d (0 fast_normalize, 1 softmax)", norm);
  WfTerms a = {};
  rc = wfuse_terms("wfuse_bwd", dweights ? terms : nullptr, shifts, dterms, nterms, H, W, &a);
  if (rc != EVK_OK) return rc;
  bool any = dweights != nullptr;
  for (int k = 0; k < nterms; ++k) any = any || dterms[k];
  EVK_REQUIRE(any, EVK_E_INVALID, "wfuse_bwd: no output requested");
  EVK_REQUIRE(!dweights || workspace_bytes >= pl.ws_bytes, EVK_E_UNSUPPORTED,
              "wfuse_bwd: workspace of %lld bytes, %lld are needed (evk_wfuse_workspace_bytes)", (long long)workspace_bytes,
              (long long)pl.ws_bytes);
  const FastDiv fc4 = make_fastdiv((uint32_t)(C / 4)), fWq = make_fastdiv((uint32_t)(pl.quad ? W / 2 : W));
  float* records = (float*)workspace;
  const dim3 grid((unsigned)pl.grid);
  const uint32_t nitems = (uint32_t)pl.items;
  const bool dw = dweights != nullptr;
  hipStream_t st = (hipStream_t)stream;
  rc = pick<1, 2, 3, 4>(nterms, [&](auto NT) {
    return pick<1, 0>(pl.quad, [&](auto QUAD) {
      return pick<1, 0>(dw, [&](auto DW) {
        hipLaunchKernelGGL((wfuse_bwd_kernel<NT(), QUAD() != 0, DW() != 0>), grid, dim3(kWfThreads), 0, st, a, dy, weights, norm,
                           eps, records, nitems, fc4, fWq, W);
        return check_launch("wfuse_bwd");
      });
    });
  });
  if (rc != EVK_OK || !dw) return rc;
  hipLaunchKernelGGL(wfuse_dw_finalize_kernel, dim3(1), dim3(kWfThreads), 0, st, records, (uint32_t)pl.grid, nterms, weights, norm,
                     eps, records + pl.grid * kWfMaxTerms, dweights);
  return check_launch("wfuse_bwd (weights)");
}
