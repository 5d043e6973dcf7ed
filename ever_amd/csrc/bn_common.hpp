// What the BatchNorm translation units share — bn.hip: plain BatchNorm, eval, SyncBN stages; bn_pool.hip: the stem's BatchNorm +
// ReLU + MaxPool; bn_dot.hip: BatchNorm + ReLU + narrow classifier — and groupnorm.hip borrows (relu_mask): the reduce plan,
// the workspace layout, the argument check, the device helpers of the reduce / finalisation / apply passes.  Header only; a
// kernel template that another file needs is reached through the host launchers declared at the end, never included twice.
#pragma once
#include "x3_common.hpp"

namespace evk {

// Traversal direction of the streaming passes (round 5).  The apply passes, forward and backward, walk the map from
// its END: the pass in front of them (the convolution that wrote z; the reduce pass that has just read g and z) finished there,
// so the lines most recently touched come first, and what the pass writes is in turn met head-first by the next convolution.
// Same arithmetic, same bits.  Six interleaved rounds on one box: 538.49 -> 539.65 tiles/s (+0.22 %, ahead in every round);
// the forward alone +0.13 %, the reduce pass reversed as well +0.19 % (tools/ab_libs.sh, profiles/r05_experiments/ab_bn_rev*.txt).
// Bits: 1 bn_apply, 2 bn_bwd_apply, 4 bn_bwd_partial.
__device__ __forceinline__ unsigned bn_blk() { return gridDim.x - 1u - blockIdx.x; }

// Channel group of a FINALISATION workgroup (round 6).  Consecutive channel groups read neighbouring 4-byte .. 32-byte pieces of
// the same 64-byte lines of the partial records, and the hardware deals consecutive workgroups to the eight XCDs round-robin:
// with group = blockIdx every line of the records was fetched by up to eight L2s (bn_parts_final_kernel<1, 256>: 53.8 MB of HBM
// fetches for 6.3 MB of records, profiles/r06_experiments/traffic_by_kernel.txt).  xcd_remap hands the workgroups of ONE XCD
// consecutive groups instead.  Which workgroup finalises a channel changes, what it computes does not: the same bits.
__device__ __forceinline__ int bn_fin_group() { return xcd_remap((int)blockIdx.x, (int)gridDim.x); }

// streaming loads of the one-element-per-thread apply passes with the non-temporal hint (round 5): they are the LAST reader of
// what they stream for a long while (the forward apply of z until the backward; the backward apply of g and z for good), so the
// lines need not stay in L2 / the memory-side cache: 536.2 -> 539.6 tiles/s, three interleaved rounds on one box
// (tools/ab_lib.sh).  The reduce pass keeps plain loads: the apply pass re-reads its data.
__device__ __forceinline__ f32x4 bn_ld(const float* p, size_t i) {
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
}

constexpr int kMaxStatBlocks = 2048;

// the slots of an output's operand-scale buffer start empty (block_absmax below fills them)
__device__ __forceinline__ void zero_amax(uint32_t* __restrict__ amax) {   // by workgroup 0 of the finalisation kernels
  if (amax && blockIdx.x == 0 && threadIdx.x < kAmaxSlots) amax[threadIdx.x * kAmaxStride] = 0;
}

struct BnPlan {
  int nblk;
  int64_t rows_per_blk;
  int tpc, rl;
};
inline BnPlan bn_plan(int64_t rows, int C, int64_t per_override = 0, int64_t cap_override = 0) {
  BnPlan p;
  const int c4 = C / 4;
  p.tpc = c4 < 256 ? c4 : 256;
  p.rl = 256 / p.tpc;
  // ~32K elements per workgroup.  Round 5, three interleaved rounds on each of two boxes, tiles/s:
  // 65536 549.1 / 525.7, 49152 - / 526.6, 40960 - / 528.1, 32768 551.2 / 528.7 (+0.4 / +0.6 %), 24576 - / 526.8, 16384 545.9 / -:
  // twice the workgroups halve the latency-bound reduce passes on the small maps, four times cost more in the finalisation
  constexpr int64_t per = 32768;
  const int64_t per_e = per_override > 0 ? per_override : per;
  int64_t nb = (rows * (int64_t)C + per_e - 1) / per_e;
  // at most TWO workgroups per CU (<= kMaxStatBlocks): whole rounds of the chip and a quarter of the partials for
  // the finalisation of the large maps.  Three interleaved rounds, two boxes: 2048 542.9 / 546.4, 1024 543.1, 768 - / 547.4,
  // 640 - / 545.9, 512 546.1 / 550.0 (+0.6 / +0.65 %), 384 - / 547.4, 256 538.6
  constexpr int64_t cap = 512;
  if (nb > (cap_override > 0 ? cap_override : cap)) nb = cap_override > 0 ? cap_override : cap;
  if (nb > kMaxStatBlocks) nb = kMaxStatBlocks;
  if (nb < 1) nb = 1;
  int64_t rpb = (rows + nb - 1) / nb;
  rpb = ((rpb + p.rl - 1) / p.rl) * p.rl;
  p.rows_per_blk = rpb;
  p.nblk = (int)((rows + rpb - 1) / rpb);
  return p;
}

// the pool backward's split of an even map into quads: as many workgroups as its row plan
inline void bn_quad_split(int64_t rows, const BnPlan& pl, int& nblk, int& qpb) {
  const int quads = (int)(rows / 4);
  qpb = (quads + pl.nblk - 1) / pl.nblk;
  qpb = ((qpb + pl.rl - 1) / pl.rl) * pl.rl;
  nblk = (quads + qpb - 1) / qpb;
}

inline unsigned oneshot_grid(size_t n4) { return (unsigned)((n4 + 255) / 256); }

// The workspace of a [rows][C] map, one size per channel count: partial records [kMaxStatBlocks][2][C], 8 C floats of
// per-channel coefficients (the forward's scale / shift, the backward's coef), records of maxima [kMaxStatBlocks][2][C]
// (packed dx).
struct BnWorkspace {
  float *partial, *coef, *pmax;
  static size_t bytes(int C) { return ((size_t)kMaxStatBlocks * 4 * C + 8 * (size_t)C) * sizeof(float); }
  BnWorkspace(void* ws, int C)
      : partial((float*)ws), coef(partial + (size_t)kMaxStatBlocks * 2 * C), pmax(coef + 8 * (size_t)C) {}
};

// The argument check of every entry point that takes a [rows][C] map; need = bytes of workspace the entry point uses (0: none)
inline int bn_check(const char* what, int64_t rows, int32_t C, const void* ws, size_t ws_bytes, size_t need) {
  EVK_REQUIRE(rows > 0 && C > 0 && C % 4 == 0 && C <= 2048, EVK_E_UNSUPPORTED, "%s: rows=%lld C=%d", what, (long long)rows,
              C);
  EVK_REQUIRE(!need || (ws && ws_bytes >= need), EVK_E_WORKSPACE, "%s: workspace too small", what);
  return EVK_OK;
}

// kernel<true> when the output is written packed, else kernel<false>: one argument list
#define EVK_BN_LAUNCH_PK(kernel, pack, grid, lds, st, ...)                                   \
  do {                                                                                       \
    if (pack) hipLaunchKernelGGL((kernel<true>), grid, dim3(256), lds, st, __VA_ARGS__);     \
    else hipLaunchKernelGGL((kernel<false>), grid, dim3(256), lds, st, __VA_ARGS__);         \
  } while (0)

// g where the forward's output yy passed the ReLU, 0 elsewhere
__device__ __forceinline__ f32x4 relu_mask(f32x4 g, const f32x4 yy) {
  g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f;
  g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
  return g;
}

// End of a reduce pass's trip over channel chunk cb: fold the sums (s, q) over the chunk's rl row lanes through the kernel's
// red[2][256] (thread = tr * tpc + tc) and store workgroup blk's record rec[blk][0][C] = s, [1][C] = q.  Every thread of the
// workgroup arrives; red is free again on return.
// (Two neighbours keep their own text, because the split that introduced this header left every kernel's instructions as
// they were and these came out reordered, registers unchanged: gn_partial_kernel (groupnorm.hip) through this helper; the
// (mu, is, sc, sh) channel prologue of the reduce and pool passes as one helper, whose loads also moved across the gather in
// bn_pool_bwd_apply_kernel: 57 -> 63 VGPRs.  The fold of MAXIMA, fold_store_maxima below, is a function of its own for the
// same reason: written as a variant of this one — template flag, functor, reference or record-pointer parameters alike —
// it came out reordered.)
__device__ __forceinline__ void fold_store_record(f32x4 (*red)[256], f32x4 s, f32x4 q, float* rec, size_t blk, int C, int cb,
                                                  int tc, int tr, int tpc, int rl) {
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = q;
  __syncthreads();
  if (tr == 0) {
    for (int k = 1; k < rl; ++k) {
      s += red[0][k * tpc + tc];
      q += red[1][k * tpc + tc];
    }
    float* o = rec + blk * 2 * C;
    *reinterpret_cast<f32x4*>(o + cb * 4) = s;
    *reinterpret_cast<f32x4*>(o + C + cb * 4) = q;
  }
  __syncthreads();
}

// m = max(m, v) / max(m, |v|) per component
__device__ __forceinline__ void max4(f32x4& m, const f32x4 v) {
  m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
}
__device__ __forceinline__ void absmax4(f32x4& m, const f32x4 v) {
  m.x = fmaxf(m.x, fabsf(v.x)); m.y = fmaxf(m.y, fabsf(v.y)); m.z = fmaxf(m.z, fabsf(v.z)); m.w = fmaxf(m.w, fabsf(v.w));
}

// fold_store_record for a record of maxima (packed dx): rec[blk][0][C] = max |g|, [1][C] = max |xhat| over the chunk's rows
__device__ __forceinline__ void fold_store_maxima(f32x4 (*red)[256], f32x4 gm, f32x4 xm, float* rec, size_t blk, int C, int cb,
                                                  int tc, int tr, int tpc, int rl) {
  red[0][threadIdx.x] = gm;
  red[1][threadIdx.x] = xm;
  __syncthreads();
  if (tr == 0) {
    for (int k = 1; k < rl; ++k) {
      max4(gm, red[0][k * tpc + tc]);
      max4(xm, red[1][k * tpc + tc]);
    }
    float* o = rec + blk * 2 * C;
    *reinterpret_cast<f32x4*>(o + cb * 4) = gm;
    *reinterpret_cast<f32x4*>(o + C + cb * 4) = xm;
  }
  __syncthreads();
}

// Sum the per-workgroup partials of 8 channels with 32 lanes per channel in fp64 (four independent loads
// in flight per lane: the chain of up to 2048 partials per channel is latency bound, and a grid of C/8
// workgroups instead of C/32 spreads it over more CUs), then fold the 32 lanes through LDS in a fixed
// order.  Returns true on the lane that holds the totals.
constexpr int kFinCh = 8;
// Fold one value per thread over the FL lanes of a channel (thread = lane * FC + channel, FC * FL = 256): xor-shuffles
// inside a wave (a channel's lanes sit FC apart), then the four waves' results through LDS — a fixed tree, so the result
// is reproducible, and 4 + log2 steps where a serial fold by one thread took FL dependent LDS round trips (32 / 128 of
// them: 4 / 16 us of the 6 / 16 us these finalisation launches took).  Every thread gets the total of its channel.
template <int FC, typename T, typename Op>
__device__ __forceinline__ T fold_channel_lanes(T v, T (*lds)[FC], Op op) {
#pragma unroll
  for (int o = FC; o < 64; o <<= 1) v = op(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane < FC) lds[w][lane] = v;
  __syncthreads();
  const int tc = threadIdx.x % FC;
  const T r = op(op(lds[0][tc], lds[1][tc]), op(lds[2][tc], lds[3][tc]));
  __syncthreads();
  return r;
}
template <int FC = kFinCh>
__device__ __forceinline__ bool reduce_partials(const float* __restrict__ partial, int nblk, int C, int& c, double& s,
                                                double& q) {
  __shared__ double red[4][FC];
  const int tc = threadIdx.x % FC, tl = threadIdx.x / FC;
  c = bn_fin_group() * FC + tc;
  s = 0.0;
  q = 0.0;
  if (c < C) {
    const float* ps = partial + c;
    const size_t st = (size_t)2 * C;
    int b = tl;
    for (; b + 3 * (256 / FC) < nblk; b += 4 * (256 / FC)) {
      const float s0 = ps[b * st], s1 = ps[(b + (256 / FC)) * st], s2 = ps[(b + 2 * (256 / FC)) * st],
                  s3 = ps[(b + 3 * (256 / FC)) * st];
      const float q0 = ps[b * st + C], q1 = ps[(b + (256 / FC)) * st + C], q2 = ps[(b + 2 * (256 / FC)) * st + C],
                  q3 = ps[(b + 3 * (256 / FC)) * st + C];
      s += ((double)s0 + (double)s1) + ((double)s2 + (double)s3);
      q += ((double)q0 + (double)q1) + ((double)q2 + (double)q3);
    }
    for (; b < nblk; b += (256 / FC)) {
      s += (double)ps[b * st];
      q += (double)ps[b * st + C];
    }
  }
  auto add = [](double a, double b) { return a + b; };
  s = fold_channel_lanes<FC>(s, red, add);
  q = fold_channel_lanes<FC>(q, red, add);
  return tl == 0 && c < C;
}

// max|v| over a workgroup's 16-byte elements into the output's operand-scale buffer (bit image; the f16x2 convolution
// arithmetic's scale of the tensor being written, x3_common.hpp act_absmax): ONE atomic max per workgroup on slot
// (workgroup & 63), the slots a cache line apart and zeroed by the finalisation kernel launched just before.  Measured:
// free (BatchNorm family 4.16 -> 4.13 TB/s).  What was not: an atomic or a guarded read of ONE word from every wave, and
// a last-arriver fold with a device-scope fence per workgroup (0.4 TB/s each); per-workgroup words + a fold launch worked
// but cost 136 launches of 5.7 us per step.
__device__ __forceinline__ void block_absmax(const f32x4 v, bool valid, uint32_t* __restrict__ amax) {
  __shared__ uint32_t red[4];
  uint32_t m = 0;
  if (valid) {
    m = __builtin_bit_cast(uint32_t, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    if (v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w) m = 0x7fc00000u;   // fmaxf drops NaNs: keep them visible
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = max(max(red[0], red[1]), max(red[2], red[3]));
    if (t) atomicMax(&amax[(blockIdx.x & (kAmaxSlots - 1)) * kAmaxStride], t);
  }
}

// Host launchers of the kernels of bn.hip that the other files need (the caller checks the launch).
// Merge of `nparts` statistics records into (mean, invstd, scale, shift): bn_parts_final_kernel
void launch_parts_final(hipStream_t st, const float* parts, int nparts, int C, double rows, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                        float* save_mean, float* save_invstd, float* scale_shift, uint32_t* amax, int pack);
// Backward finalisation of nblk partial records (and their maxima pmax, or null) into dgamma, dbeta, coef:
// bn_bwd_final_kernel
void launch_bn_bwd_final(hipStream_t st, const float* partial, int nblk, int C, int64_t rows, const float* gamma,
                         const float* invstd, float* dgamma, float* dbeta, float* coef, int train, uint32_t* amax,
                         const float* pmax);

}  // namespace evk
