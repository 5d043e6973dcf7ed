/*
 * ever_hip.h — C-ABI of libever_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * EVer hot path  ResNet encoder -> FPN / FS-Relation / decoder -> per-pixel head -> pixel loss,
 * forward + backward.
 *
 * The reference (Z-Zheng/ever 0.5.6) has no FFI: its device boundary is the set of ATen ops its
 * torch.nn modules issue.  Every entry point below cites the reference
 * call site (file:line under the reference tree) whose ATen op it replaces.
 *
 * Conventions
 *   - All activations are dense fp32 **NHWC** (pixel-major, channel-minor) in HBM.  A logical
 *     [N,C,H,W] torch tensor with channels_last strides is exactly this layout.
 *   - Convolution weights are dense fp32 **OHWI** ([Cout][kh][kw][Cin]; an OIHW torch tensor with
 *     channels_last strides).  Gradients are produced in the same layout.
 *   - Pointers are raw device pointers (hipMalloc / torch caching allocator).  The library
 *     allocates nothing: scratch is caller-provided, sizes come from the *_workspace_bytes query.
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on that stream,
 *     is re-entrant across streams and never synchronises.
 *   - Return value: 0 = ok, <0 = error (EVK_E_*); evk_last_error() returns a thread-local text.
 *     No C++ exception crosses this boundary.
 */
#ifndef EVER_HIP_H_
#define EVER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVK_OK 0
#define EVK_E_INVALID (-1)     /* bad argument (null pointer, non-positive dim, misaligned channels) */
#define EVK_E_UNSUPPORTED (-2) /* shape outside what the kernels implement */
#define EVK_E_LAUNCH (-3)      /* hipLaunch / runtime failure; see evk_last_error() */
#define EVK_E_WORKSPACE (-4)   /* caller workspace too small */

const char* evk_last_error(void);
/* library ABI version (bumped on any signature change) and the gfx arch it was built for */
int evk_abi_version(void);
const char* evk_build_arch(void);

/* ------------------------------------------------------------------ convolution ------------ */
/* Geometry of one 2-D convolution, square kernel/stride/dilation not assumed.
 * Replaces nn.Conv2d at: _resnets.py:21-29 (3x3 / 1x1), _resnets.py:149 (7x7 stem),
 * fpn.py:23-37,72-73 (FPN lateral / output), fs_relation.py:23-53 (scene MLP, content /
 * re-encode 1x1 + bias), fpn.py:165 (decoder 3x3), fpn.py:179 (classifier + bias). */
typedef struct evk_conv_desc {
  int32_t N, H, W, Cin;   /* input  x: [N,H,W,Cin]   (Cin % 4 == 0; pad channels with evk_pad_channels) */
  int32_t Ho, Wo, Cout;   /* output y: [N,Ho,Wo,Cout] */
  int32_t kh, kw;
  int32_t stride_h, stride_w;
  int32_t pad_h, pad_w;
  int32_t dil_h, dil_w;
} evk_conv_desc;

/* flags for evk_conv2d_fwd */
#define EVK_CONV_RELU 1u /* y = max(y, 0) in the epilogue */
/* f16x2 entry points only: that activation operand is stored PACKED (evk_pack_f16x2: one 32-bit word per element) */
#define EVK_CONV_X_PACKED 2u
#define EVK_CONV_DY_PACKED 4u
/* PLANAR operands of the f16x2 arithmetic (round 3): the same (h, l) pair of value / s, stored as two fp16 planes —
 * H[M][C] followed by L[M][C] in one allocation of the fp32 tensor's size (evk_pack_planar_f16x2).  The weight gradient
 * then stages nothing: both operands go global -> LDS by DMA and the fragments come from transposing LDS reads
 * (csrc/conv_wgrad_tr.hip).  Needs both flags, Cin % 64 == 0, Cout % 64 == 0, Wo % 8 == 0, dbias == NULL. */
#define EVK_CONV_X_PLANAR 8u
#define EVK_CONV_DY_PLANAR 16u
/* evk_conv2d_wgrad_f16x2_ex only (round 5): the launch runs BESIDE other work on another stream (the weight-gradient side stream
 * of hip/functional.py).  The wide-tile kernels — one 8-wave workgroup per CU — are then split for half of the CUs, so that the
 * other stream's kernels find free CUs in every XCD instead of queueing behind a 700 us launch (+1.1 .. +2.1 % on the training
 * step).  Same result bits as without the flag only if the split count happens to coincide; the workspace size does not change. */
#define EVK_CONV_WGRAD_SHARED 32u

/* y = conv(x, w) (+ bias).  w: [Cout][kh][kw][Cin].  bias may be NULL.
 * Implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32), im2col rows gathered to LDS. */
int evk_conv2d_fwd(const evk_conv_desc* d, const float* x, const float* w, const float* bias,
                   float* y, uint32_t flags, void* stream);

/* dx = conv_transpose(dy, w)  (autograd of nn.Conv2d wrt input; aten::convolution_backward).
 * wt is the weight re-packed by evk_conv2d_pack_dgrad_weight: [Cin][kh][kw][Cout] (K = taps x Cout
 * contiguous per input channel).
 * dx is fully overwritten.  `accum` folds the sum with another gradient of the same tensor (the
 * residual branch of a ResNet block) into the epilogue instead of a separate add pass. */
int evk_conv2d_dgrad(const evk_conv_desc* d, const float* dy, const float* wt,
                     const float* accum /* NULL, or a tensor of dx's shape: dx = dgrad + accum */,
                     float* dx, void* stream);
int evk_conv2d_pack_dgrad_weight(const evk_conv_desc* d, const float* w, float* wt, void* stream);

/* The same two operations on the bf16 matrix pipe at fp32-grade accuracy ("x3": each fp32 operand is
 * split exactly into three bf16 terms; six of the nine partial products — everything above 2^-26 of
 * the product — are accumulated in fp32 by v_mfma_f32_32x32x16_bf16; 2.67x the MFMA rate of the exact
 * fp32 form).  Same reference call sites as evk_conv2d_fwd / _dgrad.  Requires Cin % 8 == 0 (fwd) /
 * Cout % 8 == 0 (dgrad).  The weight is pre-split once per optimiser step:
 *   for_dgrad = 0: planes [3][Cout][Kpad] bf16, K = (ky,kx,ci), Kpad = K rounded up to 32, zero padded;
 *   for_dgrad = 1: per residue class of the strided data gradient, planes [3][Cin][Kpad_c], K = (jy,jx,co),
 *                  produced straight from the OHWI parameter (no evk_conv2d_pack_dgrad_weight needed). */
size_t evk_conv2d_split_weight_bytes(const evk_conv_desc* d, int32_t for_dgrad);
int evk_conv2d_split_weight(const evk_conv_desc* d, const float* w, int32_t for_dgrad, void* wsplit,
                            void* stream);
/* All weights of a model in ONE launch (the planes change once per optimiser step; one launch per convolution
 * and direction was 164 launches per FarSeg-R50 step).  evk_conv2d_split_jobs fills (on the HOST) the 1..stride^2
 * jobs that evk_conv2d_split_weight(d, w, for_dgrad, wsplit) would launch — same layouts, chosen from the
 * descriptor — and returns their number (negative = error).  The caller sets job.arg[12] = workgroups it gives
 * the job (about evk_split_job_pairs(job) / 2048, at least 1), builds block_map[nblocks][2] = (job index, block
 * index inside the job), copies both tables to the device once, and calls evk_conv2d_split_multi after every
 * weight update.  Replaces nothing in the reference (operand preparation of the split arithmetic). */
typedef struct evk_split_job {
  const float* w;   /* OHWI parameter */
  void* out;        /* start of this job's planes inside the convolution's wsplit buffer */
  int32_t kind;     /* 0 forward, 1 data gradient (one residue class), 2 LDS-halo 3x3 (arg[3] != 0: under the f16x2
                     * arithmetic these planes are the Winograd F(2,3) kernel's, 12 transformed taps instead of 9) */
  int32_t arg[13];  /* layout parameters (opaque); arg[12] = workgroups assigned by the caller */
} evk_split_job;
int32_t evk_conv2d_split_job_count(const evk_conv_desc* d, int32_t for_dgrad);
int evk_conv2d_split_jobs(const evk_conv_desc* d, const float* w, int32_t for_dgrad, void* wsplit,
                          evk_split_job* jobs /* host */, int32_t max_jobs);
int64_t evk_split_job_pairs(const evk_split_job* job /* host */);
/* Host only (no launch, no device needed): which kernel a forward (cls < 0) or data-gradient residue class
 * (cls = cy * stride_w + cx) launch of this descriptor takes.  planes: 0 the fp32 kernels, 3 bf16x3, 1 bf16, 2 f16x2; flags:
 * EVK_CONV_X_PACKED (forward) / EVK_CONV_DY_PACKED (data gradient); with_accum: a residual / accumulate operand; with_stats:
 * the BatchNorm statistics epilogue is requested; cus_per_xcd: compute units per XCD of the device that will run it (32 on
 * a 256-CU MI355X).  Writes "kernel<template arguments>" as a kernel trace spells the instantiation (empty: the class has
 * no launch) and, if layout is not NULL, the weight-plane layout that kernel reads — 0 generic, 1 LDS-halo 3x3, 2 Winograd
 * F(2,3) — which is the layout evk_conv2d_split_weight* / evk_conv2d_split_jobs produce for the same descriptor. */
int evk_conv2d_route(const evk_conv_desc* d, int32_t cls, int32_t planes, uint32_t flags, int32_t with_accum,
                     int32_t with_stats, int32_t cus_per_xcd, char* buf, size_t buf_bytes, int32_t* layout);
/* Host only, the same for the third launch of a convolution, the weight gradient: which instantiation and which split-K plan
 * evk_conv2d_wgrad (planes 0), _bf16 (1), _f16x2 / _f16x2_ex (2) or _x3 (3) take for this descriptor.  flags: those of
 * evk_conv2d_wgrad_f16x2_ex (EVK_CONV_X/DY_PACKED, EVK_CONV_X/DY_PLANAR, EVK_CONV_WGRAD_SHARED; planes 2 only).  Writes the
 * kernel as a trace spells it ("conv_wgrad_x3ws_kernel<128, 256, 2, true, false, true>", "conv_wgrad_tr_kernel<9>") and, if
 * plan is not NULL, plan[6] = tile rows (output channels), tile columns (k = taps x Cin; nine-tap planar form: 9 taps x 64
 * channels), row tiles, column tiles, splits of the pixel reduction, pixels per split.  The grid is row tiles x column
 * tiles x splits; with more than one split the partial tiles go to the workspace ([splits][Cout][kh kw Cin] floats) and are
 * summed in a fixed order.  Returns the error the launch would for the same descriptor and flags (planar operands without
 * their pair, Cin % 64, Wo % 8, ...): the launch entry points take kernel, tile and operand form from the value this prints. */
int evk_conv2d_wgrad_route(const evk_conv_desc* d, int32_t planes, uint32_t flags, char* buf, size_t buf_bytes,
                           int32_t* plan /* NULL or int32[6] */);
int evk_conv2d_split_multi(const evk_split_job* jobs_dev, const int32_t* block_map_dev, int32_t nblocks,
                           void* stream);
int evk_conv2d_fwd_x3(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                      float* y, uint32_t flags, void* stream);
/* Forward convolution that also produces the BatchNorm statistics of its OUTPUT ("stats fusable into
 * conv epilogue"; reference call sites: every conv -> BatchNorm pair of _resnets.py:95-112, fs_relation.py:39-53,
 * fpn.py:163-167).  The epilogue parks each 32-row accumulator block in LDS, stores it as whole output rows and keeps
 * per-lane running (count, mean, M2) of its columns; one record per row-part goes to bn_parts[part][3][Cout].
 * *nparts (host) receives the number of parts written, 0 when this shape's kernel cannot do it (then the call was a
 * plain evk_conv2d_fwd_x3 and the caller runs evk_bn_fwd_train).  bn_capacity: parts the buffer holds
 * (evk_conv2d_stats_max_parts).  evk_bn_fwd_train_parts (below) consumes the records. */
int32_t evk_conv2d_stats_max_parts(const evk_conv_desc* d);
int evk_conv2d_fwd_x3_stats(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                            float* y, uint32_t flags, float* bn_parts, int32_t bn_capacity, int32_t* nparts /* host */,
                            void* stream);
/* The reference's optional `--mixed_precision bf16` (core/launcher.py:40-80: the model runs under torch.autocast):
 * the same three convolution directions with PLAIN bf16 operands — activations and weights rounded to bf16 once, one
 * v_mfma_f32_32x32x16_bf16 product per operand pair, fp32 accumulate, fp32 tensors in HBM.  Same arguments and the same
 * weight-plane buffers as the x3 forms (only plane 0, the bf16 rounding of the weight, is read).  evk_conv2d_fwd_bf16
 * also takes the statistics arguments of evk_conv2d_fwd_x3_stats (bn_parts may be NULL).  Accuracy is that of bf16
 * inputs (relative 2^-9 per operand): never the default, never the headline benchmark. */
int evk_conv2d_fwd_bf16(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias, float* y,
                        uint32_t flags, float* bn_parts, int32_t bn_capacity, int32_t* nparts /* host */, void* stream);
int evk_conv2d_dgrad_bf16(const evk_conv_desc* d, const float* dy, const void* wsplit_t, const float* accum, float* dx,
                          void* stream);
int evk_conv2d_wgrad_bf16(const evk_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                          void* workspace, size_t workspace_bytes, void* stream);
/* "f16x2" arithmetic — the default of the training step since round 2: every fp32 operand is divided by a per-tensor
 * power of two s and split into TWO fp16 terms x / s = h + l (11-bit significands, round-to-nearest-even; the largest
 * element lands in [2^13, 2^14), |x/s - h - l| <= 2^-22 |x/s|), the product is rebuilt from the three partial products
 * l*wh + h*wl + h*wh on v_mfma_f32_32x32x16_f16 (dropped: l*wl <= 2^-22 |x*w|), accumulated in fp32 and multiplied by
 * the two scales at the end.  Same call sites as the x3 forms (nn.Conv2d at _resnets.py:21-29,149, fpn.py:23-37,
 * fs_relation.py:23-53), same plane buffers (planes 0 and 1 are used), half the matrix work.
 *   An ACTIVATION's scale source is a device buffer of evk_absmax_words() uint32: 64 slots one cache line apart, each
 *   the bit image of a partial max|x| (a non-negative float read as uint32); consumers take the maximum of the slots.
 *   evk_absmax:        fills such a buffer from a tensor (slot 0 = max|x|, the others zero); `workspace` =
 *                      evk_absmax_workspace_bytes() bytes, ZERO before the first call, private to one stream
 *   the BatchNorm calls fill one for their output as a by-product (y_absmax / dx_absmax arguments)
 *   evk_absmax_multi:  ONE word per tensor for n tensors in one launch (the weights, once per optimiser step)
 *   x_absmax / dy_absmax arguments below are activation buffers, w_absmax a single word; the kernels derive
 *   s = 2^(exponent - 13) from them. */
size_t evk_absmax_words(void);
size_t evk_absmax_workspace_bytes(void);
int evk_absmax(const float* x, int64_t n, uint32_t* out_bits, void* workspace, void* stream);
int evk_absmax_multi(const float* const* ptrs_dev, const int64_t* sizes_dev, int32_t n_tensors, uint32_t* out_bits,
                     void* stream);
int evk_conv2d_split_weight_f16x2(const evk_conv_desc* d, const float* w, int32_t for_dgrad, void* wsplit,
                                  const uint32_t* w_absmax, void* stream);
/* job.arg[11] = index of the job's weight in absmax_dev */
int evk_conv2d_split_multi_f16x2(const evk_split_job* jobs_dev, const int32_t* block_map_dev, int32_t nblocks,
                                 const uint32_t* absmax_dev, void* stream);
/* residual, bn_parts (+ nparts) may be NULL; with bn_parts the epilogue also emits the BatchNorm records (fwd_x3_stats).
 * y_absmax / dx_absmax (may be NULL): an activation scale buffer whose slots are ZERO on entry; the epilogue raises them
 * to max|output| (the output is a later convolution's operand: saves its evk_absmax pass).  accum may alias dx. */
int evk_conv2d_fwd_f16x2(const evk_conv_desc* d, const float* x, const uint32_t* x_absmax, const void* wsplit,
                         const uint32_t* w_absmax, const float* bias, const float* residual, float* y, uint32_t flags,
                         float* bn_parts, int32_t bn_capacity, int32_t* nparts /* host */, uint32_t* y_absmax,
                         void* stream);
int evk_conv2d_dgrad_f16x2(const evk_conv_desc* d, const float* dy, const uint32_t* dy_absmax, const void* wsplit_t,
                           const uint32_t* w_absmax, const float* accum, float* dx, uint32_t* dx_absmax, void* stream);
int evk_conv2d_wgrad_f16x2(const evk_conv_desc* d, const float* x, const uint32_t* x_absmax, const float* dy,
                           const uint32_t* dy_absmax, float* dw, float* dbias, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Packed activation operands of the f16x2 arithmetic.  The kernels split every fp32 operand element into two fp16
 * (h, l) of x / s while staging it — the bound of the weight gradient.  A producer that knows the
 * scale can store the element already split: one 32-bit word, h in the low half, l in the high half, same shape and
 * strides as the fp32 tensor; the consumer's staging becomes a byte permute and its results are bit-identical to the
 * fp32 operand's under the same scale buffer.  evk_pack_f16x2 is the stand-alone producer (the BatchNorm passes are the
 * fused ones, EVK_BN_PACK_*), evk_unpack_f16x2 returns (h + l) * s (tests, debugging).  n % 4 == 0.
 * evk_conv2d_fwd_f16x2 takes EVK_CONV_X_PACKED in flags; the _ex forms of the two gradients take both flags
 * (dbias must be NULL with EVK_CONV_DY_PACKED). */
int evk_pack_f16x2(const float* x, int64_t n, const uint32_t* x_absmax, uint32_t* out, void* stream);
int evk_unpack_f16x2(const uint32_t* packed, int64_t n, const uint32_t* x_absmax, float* out, void* stream);
/* planar form (EVK_CONV_*_PLANAR): n % 8 == 0; `out` / `planar` hold n fp16 of h followed by n fp16 of l (4 n bytes).
 * Replaces nothing in the reference: operand preparation of this build's arithmetic, as evk_pack_f16x2. */
int evk_pack_planar_f16x2(const float* x, int64_t n, const uint32_t* x_absmax, void* out, void* stream);
int evk_unpack_planar_f16x2(const void* planar, int64_t n, const uint32_t* x_absmax, float* out, void* stream);
int evk_conv2d_dgrad_f16x2_ex(const evk_conv_desc* d, const void* dy, const uint32_t* dy_absmax, const void* wsplit_t,
                              const uint32_t* w_absmax, const float* accum, float* dx, uint32_t* dx_absmax,
                              uint32_t flags, void* stream);
/* dx = dgrad(dy) + (accum where its ReLU bit is set): the identity branch of a residual block hands its gradient over
 * UNMASKED together with the bits of the block's output (evk_bn_fwd_train_parts_bits / evk_bn_bwd_bits), and the mask is
 * applied here, in the epilogue that adds it.  Replaces the `out += identity; relu` backward of reference
 * ever/module/_resnets.py:95-112 as autograd would run it (a masked tensor written by the ReLU backward, read by the add). */
int evk_conv2d_dgrad_f16x2_masked(const evk_conv_desc* d, const void* dy, const uint32_t* dy_absmax, const void* wsplit_t,
                                  const uint32_t* w_absmax, const float* accum, const uint32_t* accum_bits, float* dx,
                                  uint32_t* dx_absmax, uint32_t flags, void* stream);
int evk_conv2d_wgrad_f16x2_ex(const evk_conv_desc* d, const void* x, const uint32_t* x_absmax, const void* dy,
                              const uint32_t* dy_absmax, float* dw, float* dbias, void* workspace,
                              size_t workspace_bytes, uint32_t flags, void* stream);
/* y = act(conv(x, w) + bias + residual): inference form of a residual block's last convolution with its
 * BatchNorm folded into (w, bias) — `out += identity; relu` of reference _resnets.py:95-112 in the epilogue. */
int evk_conv2d_fwd_res(const evk_conv_desc* d, const float* x, const float* w, const float* bias,
                       const float* residual, float* y, uint32_t flags, void* stream);
int evk_conv2d_fwd_x3_res(const evk_conv_desc* d, const float* x, const void* wsplit, const float* bias,
                          const float* residual, float* y, uint32_t flags, void* stream);
int evk_conv2d_dgrad_x3(const evk_conv_desc* d, const float* dy, const void* wsplit_t,
                        const float* accum, float* dx, void* stream);
/* weight / bias gradient in the same arithmetic: both operands (dy and im2col(x)) are split in registers
 * while they are transposed into the pixel-contiguous LDS image the bf16 MFMA needs. */
size_t evk_conv2d_wgrad_x3_workspace_bytes(const evk_conv_desc* d);
int evk_conv2d_wgrad_x3(const evk_conv_desc* d, const float* x, const float* dy, float* dw,
                        float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ transposed convolution -- */
/* nn.ConvTranspose2d (any kernel / stride / padding / output_padding / dilation, groups = 1).
 * NO reference call site: the reference's hot path contains no transposed convolution (SURVEY.md §2.3 note;
 * `grep -rn ConvTranspose /root/reference/ever` is empty).  BASELINE.json's north_star names the operator
 * ("conv3x3/1x1 and transposed-conv lowered to MFMA"), so it is exposed; parity is pinned against
 * torch.nn.ConvTranspose2d (tests/test_conv_transpose_gpu.py), the only available oracle.
 * A transposed convolution with weight wT[Cin_t][kh][kw][Cout_t] (a ConvTranspose2d parameter with channels_last
 * strides) is the ADJOINT of the convolution C: u[N,H,W,Cin] -> z[N,Ho,Wo,Cout] that reads the same memory as
 * OHWI with Cout = Cin_t, Cin = Cout_t.  `d` is the descriptor of C: (N,H,W,Cin) = this operator's OUTPUT,
 * (Ho,Wo,Cout) = its INPUT.  forward = evk_conv2d_dgrad's residue-class kernel (no MFMA on structurally-zero taps)
 * + bias; input gradient = evk_conv2d_fwd; weight gradient = evk_conv2d_wgrad with the operand roles swapped;
 * dbias = column sums of dy.  Weight operands are prepared exactly as for the convolution C:
 * evk_conv2d_pack_dgrad_weight / evk_conv2d_split_weight(for_dgrad = 1) for the forward, the plain parameter /
 * evk_conv2d_split_weight(for_dgrad = 0) for the input gradient. */
int evk_conv_transpose2d_fwd(const evk_conv_desc* d, const float* x, const float* wt, const float* bias, float* y,
                             void* stream);
int evk_conv_transpose2d_fwd_x3(const evk_conv_desc* d, const float* x, const void* wsplit_t, const float* bias,
                                float* y, void* stream);
int evk_conv_transpose2d_dgrad(const evk_conv_desc* d, const float* dy, const float* w, float* dx, void* stream);
int evk_conv_transpose2d_dgrad_x3(const evk_conv_desc* d, const float* dy, const void* wsplit, float* dx, void* stream);
size_t evk_conv_transpose2d_wgrad_workspace_bytes(const evk_conv_desc* d, int32_t x3);
/* x: the operator's input [N,Ho,Wo,Cout], dy: gradient of its output [N,H,W,Cin]; dw in the parameter's memory order
 * [Cout][kh][kw][Cin] of C; dbias[Cin] (either may be NULL) */
int evk_conv_transpose2d_wgrad(const evk_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                               void* workspace, size_t workspace_bytes, void* stream);
int evk_conv_transpose2d_wgrad_x3(const evk_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* dw[Cout][kh][kw][Cin] = sum_pixels dy (x) im2col(x); dbias[Cout] = sum_pixels dy (dbias may be
 * NULL).  Split over pixel ranges; partials go to `workspace` and are reduced deterministically. */
size_t evk_conv2d_wgrad_workspace_bytes(const evk_conv_desc* d);
int evk_conv2d_wgrad(const evk_conv_desc* d, const float* x, const float* dy, float* dw,
                     float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* [N,H,W,C] -> [N,H,W,Cp] zero padded (forward) and the adjoint / slice (backward). Also used for
 * OHWI weights with rows = Cout*kh*kw.  C, Cp arbitrary. */
/* The ResNet stem (conv 7x7 stride 2 padding 3 on a 3- or 4-band image; _resnets.py:149, resnet.py:100-117) as a
 * space-to-depth 4x4 stride-1 convolution with 16 input channels, so that it runs on the split-MFMA kernels
 * (evk_conv2d_fwd_x3 / _wgrad_x3 with desc N, H/2+3, W/2+3, 16 -> H/2, W/2, Cout, k 4, stride 1, pad 0):
 *   evk_stem_s2d:            image [N,H,W,C] (or [N,C,H,W] when src_is_nchw) -> [N][H/2+3][W/2+3][16], zero borders
 *   evk_stem_s2d_weight:     w7 [Cout][7][7][C] -> w4 [Cout][4][4][16]
 *   evk_stem_s2d_weight_bwd: dw4 -> dw7 (the adjoint gather)
 * Same products, same sum; C <= 4, H and W even. */
int evk_stem_s2d(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t src_is_nchw,
                 void* stream);
int evk_stem_s2d_weight(const float* w7, float* w4, int32_t Cout, int32_t C, void* stream);
int evk_stem_s2d_weight_bwd(const float* dw4, float* dw7, int32_t Cout, int32_t C, void* stream);
int evk_pad_channels(const float* src, float* dst, int64_t rows, int32_t C, int32_t Cp, void* stream);
int evk_unpad_channels(const float* src, float* dst, int64_t rows, int32_t Cp, int32_t C, void* stream);
/* NCHW <-> NHWC(+pad) transposes at the model boundary (image in, logits out). */
int evk_nchw_to_nhwc(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W,
                     int32_t Cp, void* stream);
int evk_nhwc_to_nchw(const float* src, float* dst, int32_t N, int32_t C, int32_t H, int32_t W,
                     int32_t Cp, void* stream);

/* ------------------------------------------------------------------ batch norm ------------- */
/* nn.BatchNorm2d (+ReLU, + residual add) — _resnets.py:95-112 (bn1/bn2/bn3, `out += identity`,
 * relu), fs_relation.py:39-53, fpn.py:163-167.  rows = N*H*W, C % 4 == 0, C <= 2048.
 * Training forward: batch statistics (biased var for normalisation, unbiased for running_var,
 * momentum update, as torch), y = act(gamma * (x-mean)*invstd + beta [+ residual]).
 * save_mean / save_invstd: [C] outputs kept for backward. */
#define EVK_BN_RELU 1u
/* evk_bn_bwd only: dx is written PACKED (evk_pack_f16x2's format) instead of fp32 — it is the producing convolution's dy
 * operand (EVK_CONV_DY_PACKED) and nothing else.  dx_absmax is required and its slots must be ZERO on entry: the
 * finalisation raises them to a per-channel bound of |dx| (from max|g|, max|xhat| gathered by the reduce pass) before the
 * apply pass writes dx under that scale; the bound is within ~2x of max|dx| (an upper bound is all a scale needs). */
#define EVK_BN_PACK_DX 2u
/* evk_bn_fwd_train_parts only, residual == NULL: y is written PACKED — it is the next convolution's operand
 * (EVK_CONV_X_PACKED in its forward and weight gradient) and nothing else.  y_absmax as for EVK_BN_PACK_DX: zero on entry,
 * slot 0 raised by the finalisation to a bound of |y| derived from the statistics records (2-3x the true maximum). */
#define EVK_BN_PACK_Y 4u
/* (ABI <= 19: EVK_BN_NO_FUSE = 8 asked evk_bn_bwd for its three-launch form instead of a one-launch form whose grid met at
 * device-wide barriers.  That form was removed in ABI 20 — measured level with the three launches on the default path — and
 * the bit is ignored.) */
#define EVK_BN_NO_FUSE 8u
size_t evk_bn_workspace_bytes(int64_t rows, int32_t C);
/* Host only, no launch: how the reduce passes split a [rows][C] map (tests pick their shapes with it).  kind 0: the plan of
 * evk_bn_fwd_train, evk_bn_bwd and the staged entry points; kind 1: the plan of evk_bn_relu_pool_bwd.
 * out[6] = { workgroups, rows per workgroup, threads per row (each walks C / 4 / tpc 16-byte chunks), rows in flight per
 * workgroup, and for kind 1 with rows % 4 == 0 the split an even map takes: workgroups, 2 x 2 quads per workgroup (else 0, 0) }.
 * kind 2: the merge of `rows` statistics records (evk_bn_fwd_train_parts, evk_bn_finalize_parts, the fused stem pass):
 * out = { workgroups, 0, channels per workgroup, record lanes per channel, 0, 0 }.
 * A workgroup's partial record is [2][C] floats; the workspace holds records, 8 C coefficients and, for packed dx, as many
 * records of maxima, in that order. */
int evk_bn_plan(int64_t rows, int32_t C, int32_t kind, int32_t* out);
int evk_bn_fwd_train(const float* x, const float* residual, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps,
                     float* y, float* save_mean, float* save_invstd, int64_t rows, int32_t C,
                     uint32_t flags, void* workspace, size_t workspace_bytes, uint32_t* y_absmax, void* stream);
/* y_absmax / dx_absmax (may be NULL) in the four calls of this section: an activation scale buffer of
 * evk_absmax_words() uint32 (see evk_absmax) that the apply pass fills with the bit images of max|output| as a
 * by-product — the tensor is the next convolution's operand and the f16x2 arithmetic needs its scale; producing it here
 * saves that tensor one read pass. */
/* Eval forward (running statistics): y = act((x-rm)/sqrt(rv+eps)*gamma+beta [+ residual]). */
/* evk_bn_fwd_train with the statistics pass replaced by the merge (Chan, fp64, fixed order) of the (count, mean, M2)
 * records a convolution epilogue wrote (evk_conv2d_fwd_x3_stats): one pass over x less per layer. */
int evk_bn_fwd_train_parts(const float* x, const float* residual, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* y,
                           float* save_mean, float* save_invstd, int64_t rows, int32_t C, uint32_t flags,
                           const float* parts, int32_t nparts, void* workspace, size_t workspace_bytes,
                           uint32_t* y_absmax, void* stream);
/* ... and with the ReLU bits of the output written beside it (relu_bits: evk_relu_bits_bytes(rows * C) bytes, one bit per
 * element, "y > 0"; layout in csrc/common.hpp).  For the BatchNorm + add + ReLU that ends a residual block (reference
 * _resnets.py:95-112): its backward (evk_bn_bwd_bits) then reads the bits instead of the whole output tensor. */
int evk_bn_fwd_train_parts_bits(const float* x, const float* residual, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, float momentum, float eps, float* y,
                                float* save_mean, float* save_invstd, int64_t rows, int32_t C, uint32_t flags,
                                const float* parts, int32_t nparts, void* workspace, size_t workspace_bytes,
                                uint32_t* y_absmax, uint32_t* relu_bits, void* stream);
size_t evk_relu_bits_bytes(int64_t n);
/* out = g where the bit is set, else 0 (n % 4 == 0): materialises a gradient that travels unmasked with its bits */
int evk_relu_bits_apply(const float* g, const uint32_t* bits, float* out, int64_t n, void* stream);
/* The stem: BatchNorm (batch statistics from the convolution epilogue's records, as evk_bn_fwd_train_parts) + ReLU +
 * MaxPool2d(3, 2, 1) in one pass each way — reference _resnets.py:150-153 (bn1, relu, maxpool).  x [N,H,W,C] ->
 * y [N,Ho,Wo,C] and code [N,Ho,Wo,C] uint8 (winning tap ky*3+kx of each window, first maximum in scan order, as
 * evk_maxpool3x3s2_fwd), Ho = (H-1)/2+1.  The backward rebuilds dz * (z > 0) from the pooled gradient dp and the
 * codes inside its two passes: the normalised full-resolution map and its gradient are never written. */
int evk_bn_relu_pool_fwd_train_parts(const float* x, const float* gamma, const float* beta, float* running_mean,
                                     float* running_var, float momentum, float eps, float* y, uint8_t* code,
                                     float* save_mean, float* save_invstd, int32_t N, int32_t H, int32_t W, int32_t C,
                                     const float* parts, int32_t nparts, void* workspace, size_t workspace_bytes,
                                     uint32_t* y_absmax, void* stream);
int evk_bn_relu_pool_bwd(const float* dp, const uint8_t* code, const float* x, const float* gamma, const float* beta,
                         const float* save_mean, const float* save_invstd, float* dx, float* dgamma, float* dbeta,
                         int32_t N, int32_t H, int32_t W, int32_t C, int32_t train, void* workspace,
                         size_t workspace_bytes, uint32_t* dx_absmax, void* stream);
int evk_bn_fwd_eval(const float* x, const float* residual, const float* gamma, const float* beta,
                    const float* running_mean, const float* running_var, float eps, float* y,
                    float* save_mean /* may be NULL */, float* save_invstd /* may be NULL */,
                    int64_t rows, int32_t C, uint32_t flags, void* workspace, size_t workspace_bytes,
                    uint32_t* y_absmax, void* stream);
/* Backward of the training forward.  ReLU mask: taken from the forward output y when y != NULL
 * (required when the forward had a residual), else recomputed from x, gamma, beta and the saved
 * statistics (one HBM read less per pass).  d_residual (may be NULL) receives the masked upstream
 * gradient.  `train`=0 differentiates the eval forward (statistics are constants). */
int evk_bn_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
               const float* save_mean, const float* save_invstd, float* dx, float* d_residual,
               float* dgamma, float* dbeta, int64_t rows, int32_t C, uint32_t flags, int32_t train,
               void* workspace, size_t workspace_bytes, uint32_t* dx_absmax, void* stream);
/* evk_bn_bwd with the mask of the incoming gradient given as bits (relu_bits != NULL; y is then not read):
 *  - with EVK_BN_RELU: the forward's own ReLU bits (evk_bn_fwd_train_parts_bits) — a residual block's last BatchNorm reads
 *    dy, x and 1/32 of a tensor instead of dy, x and y in both passes; with d_residual == NULL the masked gradient of the
 *    identity branch is not written either: the caller hands (dy, bits) on, and the consumer masks while it adds
 *    (evk_conv2d_dgrad_f16x2_masked), or another BatchNorm takes them as below — 5 tensor transfers instead of 7;
 *  - without EVK_BN_RELU: dy is such an unmasked gradient and relu_bits its mask (the down-sampling branch's BatchNorm
 *    behind a residual block's add). */
int evk_bn_bwd_bits(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                    const float* save_mean, const float* save_invstd, float* dx, float* d_residual,
                    float* dgamma, float* dbeta, int64_t rows, int32_t C, uint32_t flags, int32_t train,
                    void* workspace, size_t workspace_bytes, uint32_t* dx_absmax, const uint32_t* relu_bits, void* stream);

/* Both BatchNorms at the end of a residual block whose shortcut is a convolution (reference _resnets.py:108-112 with
 * `downsample`): y = relu(bn_a(za) + bn_b(zb)), za the main branch's last convolution output, zb the shortcut convolution's,
 * in passes that take both maps — bn_b(zb) is never stored.  Training mode, both statistics from epilogue records (as
 * evk_bn_fwd_train_parts).  Every output has the bits of evk_bn_fwd_train_parts on zb followed by
 * evk_bn_fwd_train_parts_bits on za with that result as the residual, and of evk_bn_bwd_bits on each map in the backward.
 * workspace: 2 * evk_bn_workspace_bytes(rows, C).  y_absmax as in evk_bn_fwd_train_parts (optional); relu_bits required. */
int evk_bn_fwd_train_parts_dual(const float* za, const float* zb, const float* gamma_a, const float* beta_a,
                                float* running_mean_a, float* running_var_a, float momentum_a, float eps_a,
                                const float* gamma_b, const float* beta_b, float* running_mean_b, float* running_var_b,
                                float momentum_b, float eps_b, float* y, float* save_mean_a, float* save_invstd_a,
                                float* save_mean_b, float* save_invstd_b, int64_t rows, int32_t C, const float* parts_a,
                                int32_t nparts_a, const float* parts_b, int32_t nparts_b, void* workspace,
                                size_t workspace_bytes, uint32_t* y_absmax, uint32_t* relu_bits, void* stream);
/* The backward of the pair: dy is the gradient of y (masked already if it arrived with bits of its own), relu_bits the
 * forward's.  flags_a / flags_b: EVK_BN_PACK_DX for that output (its absmax buffer then arrives zero), nothing else.
 * evk_bn_bwd_dual_fused (host only) tells whether a pair of flags runs the two-map passes (1) or, a form that was not
 * built, the two evk_bn_bwd_bits calls inside the entry point (0); the results are the same bits either way. */
int evk_bn_bwd_dual(const float* dy, const float* za, const float* zb, const float* gamma_a, const float* save_mean_a,
                    const float* save_invstd_a, const float* gamma_b, const float* save_mean_b, const float* save_invstd_b,
                    float* dza, float* dzb, float* dgamma_a, float* dbeta_a, float* dgamma_b, float* dbeta_b, int64_t rows,
                    int32_t C, uint32_t flags_a, uint32_t flags_b, void* workspace, size_t workspace_bytes,
                    uint32_t* dza_absmax, uint32_t* dzb_absmax, const uint32_t* relu_bits, void* stream);
int evk_bn_bwd_dual_fused(uint32_t flags_a, uint32_t flags_b);

/* `to` waits for everything enqueued on `from` so far (an event of a per-device ring recorded on `from`, waited for on
 * `to`): the fork of the weight-gradient side stream from the backward's stream, once per convolution layer
 * (ever_amd/hip/functional.py).  Not thread-safe per device (the backward of one device runs on one thread).
 * No reference counterpart (the reference runs its backward on one stream). */
int evk_stream_fork(void* from, void* to);

/* 1 when kernels of streams `a` and `b` run at the same time, 0 when the runtime serialises them (HIP multiplexes streams
 * onto a few hardware queues; two streams on one queue never overlap), -1 on error.  Measured: a single-workgroup kernel
 * spinning `us` microseconds on each stream, forked and joined by events; *elapsed_us (optional) receives what the pair
 * took.  Synchronises stream `a`; not to be called under a stream capture.  Used once per device to choose the
 * weight-gradient side stream (ever_amd/hip/functional.py).  No reference counterpart. */
int evk_streams_overlap(void* a, void* b, int32_t us, float* elapsed_us);

/* ------------------------------------------------------------------ pointwise / resampling - */
/* nn.ReLU (fs_relation.py:25) and its backward; elementwise add (fpn.py:105). */
int evk_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int evk_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);
int evk_add(const float* a, const float* b, float* out, int64_t n, void* stream);
int evk_scale(const float* a, float alpha, float* out, int64_t n, void* stream);
/* Grouped convolution (reference _resnets.py:21-24 `groups=groups`; the ResNeXt bodies :291-324) runs as a DENSE one: the
 * weight w [Cout][taps][Cin / groups] (OHWI memory) is expanded to the block-diagonal dense [Cout][taps][Cin] with exact zeros
 * outside an output channel's group, the dense kernels above take it, and the adjoint gathers the diagonal blocks of the
 * dense weight gradient.  Exact in every arithmetic; at 32 groups of 4..8 channels the dense form is what fills an MFMA
 * tile anyway. */
int evk_group_weight_expand(const float* w, float* dense, int32_t Cout, int32_t taps, int32_t Cin, int32_t groups, void* stream);
int evk_group_weight_gather(const float* ddense, float* dw, int32_t Cout, int32_t taps, int32_t Cin, int32_t groups, void* stream);
/* out = a * b * alpha — nn.Dropout(p) with a 0/1 keep mask (fpn.py:183,190 `self.dropout(out_feat)`), alpha = 1/(1-p) */
int evk_mul_scale(const float* a, const float* b, float alpha, float* out, int64_t n, void* stream);
/* nn.GELU() (exact, erf form) and its derivative: the decoder's activation when norm_fn is not BatchNorm2d — fpn.py:167 */
int evk_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int evk_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);

/* nn.MaxPool2d(3, 2, 1) — _resnets.py:153.  code: one byte per output element = winning tap
 * ky*3+kx (first maximum in scan order).  x: [N,H,W,C] -> y: [N,Ho,Wo,C], Ho = (H-1)/2+1. */
int evk_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* code, int32_t N, int32_t H, int32_t W,
                         int32_t C, void* stream);
int evk_maxpool3x3s2_bwd(const float* dy, const uint8_t* code, float* dx, int32_t N, int32_t H,
                         int32_t W, int32_t C, void* stream);

/* F.interpolate(scale_factor=2, mode="nearest") + lateral add — fpn.py:100-105.
 * out[n,y,x,:] = lateral[n,y,x,:] + top[n,y/2,x/2,:];  top is [N,H/2,W/2,C]. */
/* out_absmax (may be NULL) here and in evk_mean4_fwd: an activation scale buffer, zero on entry, raised to max|out| */
int evk_upsample_nearest2x_add_fwd(const float* top, const float* lateral, float* out, int32_t N,
                                   int32_t H, int32_t W, int32_t C, uint32_t* out_absmax, void* stream);
/* adjoint wrt `top`: dtop[n,y,x,:] = sum of the 2x2 block of dout. (d lateral = dout.) */
int evk_upsample_nearest2x_bwd(const float* dout, float* dtop, int32_t N, int32_t H, int32_t W,
                               int32_t C, void* stream);

/* F.max_pool2d(x, 1, 2, 0) of LastLevelMaxPool — fpn.py:118-120 (the FPN's optional `top_blocks`): a one-pixel window at
 * stride 2, y[n,yo,xo,:] = x[n,2yo,2xo,:] with Ho = (H-1)/2+1; _bwd is its adjoint (dx = dy at the even pixels, 0 elsewhere;
 * H, W are x's dims in both). */
int evk_subsample2_fwd(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int evk_subsample2_bwd(const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);

/* nn.UpsamplingBilinear2d(scale_factor=s) == bilinear, align_corners=True — fpn.py:168,180.
 * x: [N,Hi,Wi,C] -> y: [N,Ho,Wo,C]; src = dst*(in-1)/(out-1). Backward is the gather-form adjoint. */
int evk_upsample_bilinear_fwd(const float* x, float* y, int32_t N, int32_t Hi, int32_t Wi,
                              int32_t Ho, int32_t Wo, int32_t C, void* stream);
int evk_upsample_bilinear_bwd(const float* dy, float* dx, int32_t N, int32_t Hi, int32_t Wi,
                              int32_t Ho, int32_t Wo, int32_t C, void* stream);
/* Host only, no launch: the kernel a resampling call takes and what it is launched with (tests pick their shapes with it).
 * vec: 16-byte accesses are legal (C % 4 == 0, and for a slice c0 % 4 == 0 and Ctot % 4 == 0); backward: 0 = _fwd, 1 = _bwd.
 * out[8] = { kernel, patch rows, patch columns, patch bytes, bits of sy, sx, isy, isx }.  kernel: 0 element per thread,
 * scalar; 1 element per thread, 16-byte; 2 LDS tile, 32 lanes per pixel; 3 LDS tile, 64 lanes per pixel (forward only);
 * 4 wave per pixel (backward only).  The patch is the bound on the input rows / columns one 4 x 16 output tile reads, the
 * bytes its LDS (forward; 0 in the backward; saturated at INT32_MAX).  sy, sx = (in - 1) / (out - 1) in float (0 when
 * out == 1) and, for the backward, isy, isx = 1 / s (out when s == 0) as int32 bit images.  -1 on a bad argument. */
int evk_upsample_bilinear_plan(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t C, int32_t vec,
                               int32_t backward, int32_t* out);
/* The same resampling with y / dy the channel slice [c0, c0 + C) of a [N,Ho,Wo,Ctot] map (the same kernels, another pixel
 * stride: bit-identical to the dense calls) — hrnet_head.py:17-25 (SimpleFusion: `torch.cat` of the up-sampled branches):
 * every source is written straight into its place in the concat buffer, and its gradient read straight out of the buffer's.
 * Equal sizes copy.  The other channels of y are not touched.  -1 unless 0 <= c0 and c0 + C <= Ctot. */
int evk_upsample_bilinear_slice_fwd(const float* x, float* y, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                    int32_t Wo, int32_t C, int32_t c0, int32_t Ctot, void* stream);
int evk_upsample_bilinear_slice_bwd(const float* dy, float* dx, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                    int32_t Wo, int32_t C, int32_t c0, int32_t Ctot, void* stream);

/* The exchange that ends a HighResolutionModule — _hrnet.py:377-397: y = ReLU(((t0 + t1) + t2) + t3) over 1 to 4 terms
 * (csrc/hr_fuse.hip).  Term k is the map terms[k] = [N, H >> s, W >> s, C] with s = shifts[k] in 0..3, read at output pixel
 * (y, x) as v = terms[k][n, y >> s, x >> s, :] (nearest up-sampling by 2^s); with scale_shifts[k] != NULL ([2][C]: a BatchNorm
 * as evk_bn_finalize_parts leaves it) the term is fma(v, scale, shift), else v.  The three arrays are HOST arrays of nterms
 * entries read during the call.  relu_bits: evk_relu_bits_bytes(N * H * W * C) bytes, bit = (y > 0), layout in
 * csrc/common.hpp; y_absmax (may be NULL): as out_absmax of evk_upsample_nearest2x_add_fwd.
 * -1: null pointer or non-positive size.  -2 (with a text): C % 4 != 0, nterms outside 1..4, a shift outside 0..3, H or W
 * not a multiple of 2^(largest shift), 2^31 or more 16-byte elements. */
int evk_hr_fuse_fwd(const float* const* terms, const int32_t* shifts, const float* const* scale_shifts, int32_t nterms,
                    float* y, uint32_t* relu_bits, uint32_t* y_absmax, int32_t N, int32_t H, int32_t W, int32_t C,
                    void* stream);
/* Its backward, one read of dy [N,H,W,C] and the bits; every output may be NULL (not all): dmasked = dy where the bit is set
 * (the gradient of a same-resolution term: an identity term takes it as it is, a BatchNorm term runs evk_bn_bwd_bits
 * without EVK_BN_RELU on (dy, bits) and needs no dmasked), dpooled_s [N, H >> s, W >> s, C] = the sum of the masked dy over
 * each 2^s x 2^s block (the gradient of a term with shift s: a BatchNorm term runs evk_bn_bwd on it).  H and W must be
 * multiples of 2^(largest requested s).  One owner per output element and a fixed order of summation: no atomics, the same
 * bits every run.  Error codes as the forward. */
int evk_hr_fuse_bwd(const float* dy, const uint32_t* relu_bits, float* dmasked, float* dpooled1, float* dpooled2,
                    float* dpooled3, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);

/* The learned weighted fusion node of a BiFPN — fpn.py:196-224 (Fusion) with the UpsamplingNearest2d of fpn.py:264-269 as an
 * index shift (csrc/wfuse.hip):  y = ((w^0 t0 + w^1 t1) + w^2 t2) + w^3 t3 over 1 to 4 terms, NHWC fp32.  Term k is
 * terms[k] = [N, H >> s, W >> s, C] with s = shifts[k] in {0, 1}, read at output pixel (y, x) as its pixel (y >> s, x >> s).
 * terms and shifts are HOST arrays of nterms entries read during the call.  weights: the RAW [nterms] parameter ON THE
 * DEVICE, normalised inside the kernel: norm 0 = fast_normalize, r = max(w, 0), w^ = r / (sum r + eps); norm 1 = softmax
 * (max-subtracted; eps unused); weights == NULL = unit weights (one term with shift 1: plain nearest x2).  Every product
 * and sum is rounded on its own, and a term whose w^ is 0 is still read and multiplied (its infinities and NaNs propagate).
 * -1: null pointer or non-positive size.  -2 (with a text): C % 4 != 0, nterms outside 1..4, a shift outside {0, 1}, norm
 * outside {0, 1}, H or W odd with a shifted term, 2^31 or more 16-byte elements.  All before any launch. */
int evk_wfuse_fwd(const float* const* terms, const int32_t* shifts, int32_t nterms, const float* weights, int32_t norm,
                  float eps, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* Its backward: one read of dy [N,H,W,C], and of each term only when dweights != NULL (terms may be NULL otherwise).
 * dterms: HOST array of nterms device pointers, each may be NULL: shift 0 gives w^_k dy, shift 1 the sum over each 2 x 2 block
 * of w^_k dy, (p00 + p01) + (p10 + p11) by the block's one owner.  dweights [nterms] (may be NULL; needs weights): the
 * gradient with respect to the RAW weights: the dots d_k = sum dy up(t_k) over the whole map, then the Jacobian,
 * fast_normalize: [w_j > 0] (d_j - sum_k w^_k d_k) / (sum r + eps);  softmax: w^_j (d_j - sum_k w^_k d_k).  The dots use no
 * atomics: fp32 partials per thread over at most D products, a wave / LDS tree to one record per workgroup in the
 * workspace, a one-workgroup launch that adds the records in double in a fixed order: the same bits every run.
 * workspace (16-byte aligned, evk_wfuse_workspace_bytes; needed with dweights only) holds afterwards the records
 * [grid][4] fp32 and behind them the four dots, rounded to fp32 (float offset out[6] of evk_wfuse_plan).
 * Error codes as the forward; no output at all is -1, a workspace that is too small -2. */
int evk_wfuse_bwd(const float* dy, const float* const* terms, const int32_t* shifts, int32_t nterms, const float* weights,
                  int32_t norm, float eps, float* const* dterms, float* dweights, void* workspace, int64_t workspace_bytes,
                  int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* 0 for arguments evk_wfuse_plan refuses */
size_t evk_wfuse_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t nterms);
/* Host only, no launch: the geometry of evk_wfuse_bwd (tests take their error bound and grid-edge shapes from it).
 * out[8] = { grid (workgroups = records), threads per workgroup, D (products one thread adds serially into one fp32 partial),
 * workspace bytes, 1 if a thread owns a 2 x 2 quad (H and W even) else 0 (one 16-byte element), items (quads or elements)
 * per thread — a workgroup's share is threads x that many consecutive items —, float offset of the dots in the workspace, 0 }.
 * The grid has no cap: it grows with the map.  Return codes as evk_wfuse_fwd. */
int evk_wfuse_plan(int32_t N, int32_t H, int32_t W, int32_t C, int32_t nterms, int32_t* out);

/* The eight symmetries of the square on an NHWC map — magic/transform/segm.py (Rotate90k, HorizontalFlip, VerticalFlip,
 * Transpose) — and their fused mean — magic/transform/tta.py: `sum(outs) / len(outs)` (csrc/d4.hip).
 * op = swap | flip_rows << 1 | flip_cols << 2 acts on x: [N,Hi,Wi,C] and gives y: [N,Ho,Wo,C], (Ho, Wo) = swap ? (Wi, Hi) :
 * (Hi, Wi):  y[n,r,c,:] = x[n,a,b,:] with r' = flip_rows ? Ho-1-r : r, c' = flip_cols ? Wo-1-c : c, (a, b) = swap ? (c', r') :
 * (r', c') — transpose first, then flip.  In NCHW terms: flip(x, [2]) = 2, flip(x, [3]) = 4, transpose(2, 3) = 1,
 * rot90(x, 1, [2,3]) = 3, rot90(x, 2, [2,3]) = 6, rot90(x, 3, [2,3]) = 5, the anti-transpose = 7.  The inverse of 3 is 5 and
 * of 5 is 3; every other op is its own inverse.  A dense NCHW map is the same call with N' = N*C, C' = 1.
 * evk_d4_apply is a pure copy of 32-bit words (NaN payloads, infinities, -0.0 keep their bits); op 0 copies.  x and y may
 * not overlap.  Index arithmetic is 32-bit: all three entry points return -2 for N*Hi*Wi*C >= 2^31, before any launch;
 * -1: null pointer, non-positive size, op outside 0..7. */
int evk_d4_apply(const float* x, float* y, int32_t N, int32_t Hi, int32_t Wi, int32_t C, int32_t op, void* stream);
/* y[i] = s / (float)count (count > 0; a correctly rounded fp32 division) or s (count == 0), where
 * s = (acc ? acc[i] : 0.0f) + T_0(t_0)[i], then s += T_k(t_k)[i] for k = 1 .. nterms-1 in that order: bit for bit the
 * reference's `sum(outs) / len(outs)` (sequential fp32 adds from 0, so an all -0.0 sum is +0.0).  T_k is ops[k] as above and
 * terms[k] has the dims ops[k] implies for an [N,Ho,Wo,C] result: [N,Wo,Ho,C] for a swap op.  terms and ops are HOST arrays
 * of nterms entries read during the call, 1 <= nterms <= 16 (-2 otherwise); a longer list is chained through acc
 * [N,Ho,Wo,C] with count = 0 on all calls but the last, which keeps the order of additions.  y may alias acc, not a term
 * (-1).  One launch: every term takes the path evk_d4_plan names for its shape, a direct read or the LDS tile. */
int evk_d4_merge(const float* const* terms, const int32_t* ops, int32_t nterms, const float* acc, float* y, int32_t N,
                 int32_t Ho, int32_t Wo, int32_t C, int32_t count, void* stream);
/* Host only, no launch: the kernel a term x: [N,Hi,Wi,C] under `op` takes in evk_d4_apply and evk_d4_merge (both decide
 * through this function; tests pick their shapes with it).  out[6] = { kernel, tile rows, tile columns, LDS row stride in
 * floats, LDS bytes, elements per thread }.  kernel: 0 element per thread, scalar; 1 element per thread, 16-byte (C % 4 == 0;
 * the launchers fall back to 0 for a pointer off the 16-byte grid); 2 LDS tile (swap ops on narrow pixels; the last five
 * numbers are 0 otherwise).  Return codes as evk_d4_apply. */
int evk_d4_plan(int32_t N, int32_t Hi, int32_t Wi, int32_t C, int32_t op, int32_t* out);
/* For measurements and tests only (tools/bench_tta.py, tests/test_d4_gpu.py); the package never calls it.  From now on, in
 * this process, evk_d4_plan and both launchers name `kernel` (0, 1 or 2 as above) wherever that kernel is legal for the term
 * (1 needs C % 4 == 0, 2 a swap op and C <= 64) and follow their own rule elsewhere; any other value, -1 by custom, restores
 * the rule everywhere.  Returns the previous setting (-1: none). */
int evk_d4_force_kernel(int32_t kernel);

/* Augmentation and input preparation of a whole batch in one launch — preprocess/thsegm.py, thcomm.py: THRandomRotate90k ->
 * THRandomHorizontalFlip -> THRandomVerticalFlip -> THRandomCrop((crop_h, crop_w)) -> THChannelFirst2 -> THMeanStdNormalize2
 * -> THDivisiblePad per image, then torch.stack (csrc/augment.hip).  The random draws are the caller's: sample i comes with
 * one op (the 3 bits above) and one crop origin.
 * Sample i is a dense source S [Hs,Ws,C] (uint8, or fp32 when src_f32) at any byte address and, unless mask_mode is 0, a
 * dense label map [Hs,Ws].  T = d4(S, op) has (Ht, Wt) = swap ? (Ws, Hs) : (Hs, Ws).  For pixel (r, c) of the [Ho,Wo] output:
 *   r < crop_h and c < crop_w: (a, b) = (y0 + r, x0 + c); raw = a < Ht and b < Wt ? T[a,b,:] : 0 and the label likewise (the
 *     zero pad inside THRandomCrop); value = (float(raw) - mean[k]) / std[k] — one rounded subtraction, one correctly rounded
 *     division, no reciprocal, no fma — or float(raw) when mean and std are NULL
 *   else: value +0.0f, label mask_pad_value.
 * out: [N,Ho,Wo,C] (nchw == 0) or [N,C,Ho,Wo] fp32.  mask_mode 0: no labels (the mask words and out_mask are ignored);
 * 1: uint8 -> uint8; 2: uint8 -> int64 (zero-extended); 3: int64 -> int64; out_mask: [N,Ho,Wo].
 * `records` (HOST, read during the call) and `table` (DEVICE, read by the kernel; the caller uploads it in stream order)
 * hold the same N records of 8 int64: { image address, mask address, Hs, Ws, op, y0, x0, 0 }.  mean / std: C fp32 in DEVICE
 * memory, both or neither.  No atomics: every element has one writer, two runs give the same bits.
 * Refused before any launch: -1 for a null table, output or image, mean without std, a crop larger than the output, an op
 * outside 0..7, an origin outside 0 <= y0 <= max(Ht, crop_h) - crop_h (and the same for x0); -2 for C > 64, a source of
 * 2^31 elements or more, an output of 2^31 elements or more, N > 65535. */
int evk_augment_batch(const int64_t* records, const int64_t* table, int32_t N, int32_t C, int32_t crop_h, int32_t crop_w,
                      int32_t Ho, int32_t Wo, const float* mean, const float* std, int32_t mask_pad_value, int32_t nchw,
                      int32_t src_f32, int32_t mask_mode, float* out, void* out_mask, void* stream);
/* Host only, no launch: the checks evk_augment_batch makes on one sample (same return codes) and the kernel form its
 * (C, dtype, op, layout) takes.  out[6] = { kernel, tile edge T in pixels, LDS row stride in floats, LDS bytes, elements per
 * thread, 16-byte stores }.  kernel 0: direct, four consecutive output elements per thread and one 16-byte store when the last
 * number is 1 (Ho*Wo % 4 == 0; the launcher falls back to an element per thread for an output off the 16-byte grid); 1: LDS tile
 * (swap ops; numbers two to five are 0 otherwise).
 * A launch takes the tile kernel when the plan of any of its samples does; samples without a swap op read directly in it. */
int evk_augment_plan(int32_t Hs, int32_t Ws, int32_t C, int32_t op, int32_t y0, int32_t x0, int32_t crop_h, int32_t crop_w,
                     int32_t Ho, int32_t Wo, int32_t src_f32, int32_t nchw, int32_t* out);
/* For measurements and tests only (tools/bench_augment.py, tests/test_augment_gpu.py); the package never calls it.  From now
 * on, in this process, the plan names `kernel` (0, 1, or 2: direct with 4-byte stores only) wherever it is legal (1 needs a swap
 * op) and follows its own rule elsewhere; any other value, -1 by custom, restores the rule.  Returns the previous setting. */
int evk_augment_force_kernel(int32_t kernel);
/* evk_augment_batch with the reference's THRandomScale (bilinear align_corners=True for the image, nearest for the labels) in
 * front of the chain, inside the same single launch.  Sample i has a factor f > 0; the CALLER computes the scaled size
 * Hz = int(floor(double(Hs) * f)), Wz likewise (aten's output sizes) and s = float(1.0 / double(f)).  Z [Hz,Wz,C] is the
 * scaled image, and everything after Z is evk_augment_batch with Z for S: T = d4(Z, op), the window at (y0, x0) of T, raw 0
 * and label 0 inside the window where T ends, normalise, pad.
 * Image, fp32, every operation rounded on its own (no fma):
 *   ry = Hz > 1 ? float(Hs - 1) / float(Hz - 1) : 0;  sy = ry * float(a);  y0 = min(int(sy), Hs - 1);  y1 = y0 + (y0 < Hs - 1);
 *   ly = sy - float(y0);  hy = 1 - ly;  the same for x;  p** = float(S[y*, x*, k])
 *   Z[a,b,k] = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11)
 * A uint8 source is interpolated in fp32 and NOT rounded back to uint8 (aten's CPU kernel rounds back when handed a uint8
 * tensor): the pass is the chain applied to the image cast to fp32 first.  The min-clamps are there so that no record can
 * cause a read outside the source; aten has none.
 * Labels: Zm[a,b] = M[min(int(floorf(float(a) * s)), Hs - 1), min(int(floorf(float(b) * s)), Ws - 1)], for all three mask
 * modes (aten has no nearest kernel for int64).
 * A sample with Hz == Hs, Wz == Ws and s == 1.0f is not scaled: Z = S, one tap, the bits of evk_augment_batch (the formula
 * gives the same bits on finite values, but for the sign of a zero).
 * Relation to aten (tests/augment_scale_common.py is the definition, aten a second witness): the image is not bit-equal to
 * aten's CPU bilinear, which evaluates the same weights in another order; both make at most 9 roundings of non-negative
 * terms, so they differ by at most 8 * 2^-23 * max|source|.  The labels equal aten's CPU nearest wherever Hz is neither Hs nor
 * 2 Hs and Wz neither Ws nor 2 Ws; there aten takes a same-size / double-size shortcut its generic formula does not reproduce.
 * Records are 12 int64: { image address, mask address, Hs, Ws, op, y0, x0, 0, Hz, Wz, bit image of s in the low 32 bits, 0 }.
 * Return codes and refusals as evk_augment_batch, with the origin limits taken on d4 of (Hz, Wz), and further: -1 for Hz < 1,
 * Wz < 1, s not finite or not positive; -2 for Hz * Wz * C >= 2^31.  Every refusal comes before any launch. */
int evk_augment_scale_batch(const int64_t* records, const int64_t* table, int32_t N, int32_t C, int32_t crop_h, int32_t crop_w,
                            int32_t Ho, int32_t Wo, const float* mean, const float* std, int32_t mask_pad_value, int32_t nchw,
                            int32_t src_f32, int32_t mask_mode, float* out, void* out_mask, void* stream);
/* Host only, no launch: the checks evk_augment_scale_batch makes on one sample (same return codes).  out[5] = { kernel (0:
 * the scaled direct kernel, the only form), output elements per thread (4 C with 16-byte stores, else C: a thread owns whole
 * pixels), 16-byte stores (Ho*Wo % 4 == 0; the launcher falls back for an output off the 16-byte grid), bit image of ry, bit
 * image of rx }. */
int evk_augment_scale_plan(int32_t Hs, int32_t Ws, int32_t C, int32_t op, int32_t y0, int32_t x0, int32_t crop_h,
                           int32_t crop_w, int32_t Ho, int32_t Wo, int32_t src_f32, int32_t nchw, int32_t Hz, int32_t Wz,
                           int32_t s_bits, int32_t* out);

/* Whole-scene tiled inference, the stitching half (csrc/stitch.hip; magic/bigimage/scene.py) — per window the
 * `out[:, y0:y1, x0:x1] += s; count[y0:y1, x0:x1] += 1` of a sliding-window driver, per scene its `out / count`.
 * scores: M window maps of one size h x w, acc: the scene accumulator, both in the same dense layout: NHWC memory (nchw == 0:
 * scores [M,h,w,C], acc [H,W,C]) or NCHW-contiguous (scores [M,C,h,w], acc [C,H,W]); count: the coverage plane [H,W] fp32.
 * `records` (HOST, read during the call) and `table` (DEVICE, read by the kernels; the caller uploads it in stream order) hold
 * the same M records of 2 int64: { y0, x0 }, window m covers rows y0 .. y0+h-1 and columns x0 .. x0+w-1.
 * Every accumulator element has ONE owner, which adds the windows that cover it in table order: ((acc + s_a) + s_b) + ..., the
 * bits of the sequential loop; no atomics, two runs give the same bits.  The coverage of a pixel grows by 1 per covering window
 * (added as one (float)n: the same value while the count is below 2^24).  The grid covers the bounding box of the windows of a
 * launch; an element of the box that no window covers is neither read nor written.  64 windows per launch; a longer table is
 * chained in order inside the call.  Element offsets are 64-bit: the accumulator may hold 2^31 elements or more.
 * Refused before any launch: -1 for a null pointer, M < 1, a non-positive size, a window not inside the scene; -2 for
 * C > 65535 or a scene row of 2^31 floats or more. */
int evk_stitch_add(const int64_t* records, const int64_t* table, int32_t M, const float* scores, float* acc, float* count,
                   int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, int32_t nchw, void* stream);
/* One pass over acc and count (layouts as above).  mode 0, scores: out[i] = acc[i] / count[pixel of i], one correctly rounded
 * division (0/0 = NaN where nothing was added); out: fp32 in acc's layout, NULL or acc itself for in place.  mode 1, labels:
 * out [H,W] uint8 (label_i64 == 0) or int64; C >= 2: the index of the first maximal quotient acc / count — the quotients are
 * compared, not the sums, and a NaN is maximal, as in torch.argmax; C == 1: quotient > threshold ? 1 : 0 (threshold is
 * ignored otherwise); a pixel with coverage 0 gets fill_label.
 * Refused before any launch: -1 for a null acc or count, labels without an output, a mode outside 0..1, a non-positive size,
 * a fill_label outside 0..255 with uint8 labels; -2 for C > 256 with uint8 labels, C > 65535, a row of 2^31 floats or more. */
int evk_stitch_finalize(float* acc, const float* count, int32_t C, int32_t H, int32_t W, int32_t nchw, int32_t mode, void* out,
                        int32_t label_i64, float threshold, int32_t fill_label, void* stream);
/* Host only, no launch: the checks evk_stitch_add makes on a table (same return codes) and the forms the kernels take for
 * pointers on the 16-byte grid (the launchers fall back to the scalar forms otherwise).  out[12] = { stitch_add takes 16-byte
 * items (every row start and every window edge on the 4-float grid: W*cpp, w*cpp and every x0*cpp multiples of 4, cpp = 1 for
 * NCHW and C for NHWC), workgroups along a row of the bounding box (64 items each), workgroups down its rows (4 rows each),
 * grid.y (planes: C for NCHW, 1 for NHWC), launches (ceil(M / 64)), bounding box y0, x0, y1, x1 (end exclusive), scores
 * finalise takes 16-byte items (W*cpp % 4 == 0), labels finalise takes its wide form (4 pixels per thread: NCHW or C == 1 with
 * W % 4 == 0; 16-byte channel loads: NHWC with C % 4 == 0), 0 }.  Numbers one, two and five to eight are those of the first launch. */
int evk_stitch_plan(const int64_t* records, int32_t M, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, int32_t nchw,
                    int32_t* out);

/* Pyramid pooling (csrc/ppm.hip; reference ppm.py:8-35, ops.py:89-100) — `torch.cat([x] + [F.interpolate(block_k(
 * F.adaptive_avg_pool2d(x, b_k)), (H, W), mode='bilinear', align_corners=False) for k], dim=1)` as one read of x for all K
 * pools, one write of the concat map, and both backward halves in gather form.  fp32 on NHWC memory, plain fp32 under every
 * conv-math mode, no packed operands, no float atomics: two runs give the same bits.
 * x: [N,H,W,C]; bins: K sizes b_k (HOST array, read during the call, as are the per-bin pointer tables p, dp, z, dz);
 * p_k, dp_k: [N,b_k,b_k,C]; z_k, dz_k: [N,b_k,b_k,Cp]; cat, dcat: [N,H,W,C + K Cp].
 * Scope: 1 <= K <= 4, 1 <= b_k <= 8 (b_k > H is legal, as in aten), C % 4 == 0, Cp % 4 == 0, N H W (C + K Cp) < 2^31 and
 * fewer than 2^31 pooled elements, else EVK_E_UNSUPPORTED; null pointers, pointers off the 16-byte grid, non-positive sizes:
 * EVK_E_INVALID; a workspace smaller than its query: EVK_E_WORKSPACE.  Every refusal comes before any launch.
 *
 * Window i of an axis of L pixels under bin b is [ws, we) = [floor(i L / b), ceil((i + 1) L / b)) (aten's adaptive window;
 * the windows of one bin overlap where L % b != 0).
 * evk_ppm_pool_fwd:  p_k[n,i,j,c] = (sum of x[n,y,x,c] over the window) / float((ye - ys)(xe - xs)), ONE division.  Order of
 *   the sum: each axis is cut at the union of all bins' window edges (at most 63 cells per axis, a partition of the map).
 *   A cell row [y0, y1) is shared by four row groups, group g takes rows y0 + g, y0 + g + 4, ...; a group adds its rows in
 *   ascending y, each row of the cell in ascending x, from +0; the cell sum is ((g0 + g1) + g2) + g3.  A window's cells are
 *   then added row-major from +0.  The cell sums [N, cells_y, cells_x, C] go to the workspace.
 * evk_ppm_expand_fwd:  cat[n,y,x,0:C] = x[n,y,x,:] (copied bits);  cat[n,y,x,C + k Cp + c] = the bilinear
 *   align_corners=False sample of z_k.  Per axis (b sources, L outputs), in fp32, every operation rounded on its own, no fma:
 *     s = float(b) / float(L);  src = max(s * (float(y) + 0.5) - 0.5, 0);  i0 = min(int(src), b - 1);  i1 = i0 + (i0 < b - 1);
 *     l1 = src - float(i0);  l0 = 1 - l1
 *   value = l0y * (l0x * p00 + l1x * p01) + l1y * (l0x * p10 + l1x * p11); an axis whose taps coincide (i1 == i0)
 *   contributes the tap itself, without a blend, so a bin of 1 is an exact broadcast (evk_broadcast_hw's bits).
 *   C may be 0 here and in evk_ppm_expand_bwd (x NULL): the up-sampled maps alone.
 * evk_ppm_expand_bwd:  dz_k[n,i,j,c] = sum over (y, x) of wy(y,i) wx(x,j) dcat[n,y,x,C + k Cp + c], w(y,i) = l0 where
 *   i == i0 != i1, l1 where i == i1 != i0, 1 where i == i0 == i1, else 0.  Separable: t[n,y,j,c] = sum over x ascending of
 *   (wx * dcat), each product rounded, from +0 (workspace [N,H,sum b,Cp]); dz = sum over y ascending of (wy * t), from +0.
 *   One read of dcat's pooled slices for all K bins; the gradient of x through the concat is NOT written: it is dcat's
 *   channel slice [0, C), a strided view the caller hands to evk_ppm_pool_bwd.
 * evk_ppm_pool_bwd:  dx[n,y,x,c] = (dskip ? dskip[(n H W + y W + x) ld + c] : +0) + q_1 + q_2 + ..., q = dp_k[n,i,j,c] /
 *   float(count of window (i,j)), one division each, added in the order: bins k ascending, the windows of bin k that hold
 *   (y, x) row-major.  ld >= C, ld % 4 == 0 (EVK_E_INVALID otherwise).  One write of dx. */
size_t evk_ppm_pool_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, const int32_t* bins, int32_t K);
int evk_ppm_pool_fwd(const float* x, float* const* p, const int32_t* bins, int32_t K, int32_t N, int32_t H, int32_t W,
                     int32_t C, void* workspace, size_t workspace_bytes, void* stream);
int evk_ppm_pool_bwd(const float* const* dp, const int32_t* bins, int32_t K, const float* dskip, int32_t ld, float* dx,
                     int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int evk_ppm_expand_fwd(const float* x, const float* const* z, const int32_t* bins, int32_t K, float* cat, int32_t N, int32_t H,
                       int32_t W, int32_t C, int32_t Cp, void* stream);
size_t evk_ppm_expand_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cp, const int32_t* bins,
                                          int32_t K);
int evk_ppm_expand_bwd(const float* dcat, float* const* dz, const int32_t* bins, int32_t K, int32_t N, int32_t H, int32_t W,
                       int32_t C, int32_t Cp, void* workspace, size_t workspace_bytes, void* stream);
/* Host only, no launch: the checks the four launchers make on a case (same return codes; Cp may be 0: the pools alone, or C: the expand alone) and
 * the forms they take.  out[16] = { kernel form (0: cells + windows, the only one), bytes per load and store (16), cells per
 * axis y, x, pool forward stage 1 workgroups, of which per cell row (channel chunks of 256), stage 2 workgroups (N sum b^2),
 * workgroups of expand forward and of pool backward (one per pixel), expand backward stage 1 workgroups, of which per row
 * (chunks of 1024 pooled channels), stage 2 workgroups, threads per workgroup, pool workspace bytes, expand backward workspace
 * bytes, sum b, sum b^2 }.  A workspace of 2^31 bytes or more is refused here alone (EVK_E_UNSUPPORTED). */
int evk_ppm_plan(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cp, const int32_t* bins, int32_t K, int32_t* out);

/* F.adaptive_avg_pool2d(x, 1) — fs_relation.py:177. x: [N,HW,C] -> y: [N,C]. */
int evk_gap_fwd(const float* x, float* y, int32_t N, int32_t HW, int32_t C, void* stream);
int evk_gap_bwd(const float* dy, float* dx, int32_t N, int32_t HW, int32_t C, void* stream);

/* FS-Relation — fs_relation.py:61-71: r = sigmoid(sum_c scene[n,c]*content[n,p,c]); out = r*feat.
 * scene: [N,C], content/feat/out: [N,HW,C], r: [N,HW] (saved for backward). */
int evk_relation_fwd(const float* scene, const float* content, const float* feat, float* out,
                     float* r, int32_t N, int32_t HW, int32_t C, void* stream);
/* dscene must be zero-initialised by the caller? No: fully written (two-stage reduction inside,
 * workspace from evk_relation_workspace_bytes). */
size_t evk_relation_workspace_bytes(int32_t N, int32_t HW, int32_t C);
int evk_relation_bwd(const float* dout, const float* scene, const float* content, const float* feat,
                     const float* r, float* dscene, float* dcontent, float* dfeat, int32_t N,
                     int32_t HW, int32_t C, void* workspace, size_t workspace_bytes, void* stream);

/* The scene branch of FS-Relation — fs_relation.py:23-29,56-60: L scene encoders Conv2d(K, C, 1) -> ReLU -> Conv2d(C, C, 1)
 * (both with bias) on the pooled vector s [N][K], all levels in two launches forward and three backward, fp32, no atomics,
 * one fixed summation order (csrc/relation_scene.hip).  w1[l]: [C][K], w2[l]: [C][C], b1[l], b2[l]: [C] — HOST arrays of L
 * device pointers, the modules' own parameters; they travel in the kernel arguments (nothing is copied to the device, the
 * calls are capture-safe).  h, o, dh: [L][N][C].  The forward gives the bits of evk_conv2d_fwd on the same [N, K, 1, 1] input.
 * Backward: g[l] [N][C] = gradient of o[l] (a null entry counts as zeros) -> dh (gradient in front of the ReLU: zero where
 * h == 0), ds [N][K], dw1[l], db1[l], dw2[l], db2[l] in the parameters' layouts; workspace from
 * evk_relation_scene_bwd_workspace_bytes (the slice partials of ds).  L <= 8, N <= 32, K % 4 == 0, C % 4 == 0 and biases
 * present, else EVK_E_UNSUPPORTED; pointers 16-byte aligned, else EVK_E_INVALID; both before any launch. */
int evk_relation_scene_fwd(const float* s, const float* const* w1, const float* const* b1, const float* const* w2,
                           const float* const* b2, float* h, float* o, int32_t L, int32_t N, int32_t K, int32_t C,
                           void* stream);
size_t evk_relation_scene_bwd_workspace_bytes(int32_t L, int32_t N, int32_t K, int32_t C);
int evk_relation_scene_bwd(const float* s, const float* h, const float* const* g, const float* const* w1,
                           const float* const* w2, float* dh, float* ds, float* const* dw1, float* const* db1,
                           float* const* dw2, float* const* db2, int32_t L, int32_t N, int32_t K, int32_t C,
                           void* workspace, size_t workspace_bytes, void* stream);

/* `sum(list)/len(list)` over 4 decoder branches — fpn.py:189. */
int evk_mean4_fwd(const float* a, const float* b, const float* c, const float* d, float* out,
                  int64_t n, uint32_t* out_absmax, void* stream);

/* ------------------------------------------------------------------ pixel losses ----------- */
/* Labels are int64 [N*H*W]; ignore_index pixels are dropped from every sum (the reference
 * compacts with masked_select, loss.py:10-17,26-37).  logits: [N*H*W, C] (NHWC).
 * Each forward writes `stats` (doubles) that the matching backward consumes; loss is a device
 * float scalar.  grad_scale is the upstream dL/dloss (device float pointer, may be NULL = 1).
 * `stats` must hold evk_loss_stats_doubles(K) doubles (K finals followed by per-workgroup
 * partials); K = 2 (BCE), 2*C (dice), 3 (CE).  Only the first K are meaningful to the caller. */
int64_t evk_loss_stats_doubles(int32_t K);

/* binary_cross_entropy_with_logits(ignore) — loss.py:229-235; with label_smoothing > 0 it is
 * label_smoothing_binary_cross_entropy — loss.py:222-226 (target 0 -> eps, 1 -> 1-eps).
 * C == 1. stats: double[2]={sum,count} */
int evk_bce_fwd(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                float label_smoothing, float* loss, double* stats, void* stream);
int evk_bce_bwd(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                float label_smoothing, const double* stats, const float* grad_scale, float* dlogits,
                int32_t accumulate, void* stream);

/* the same with F.binary_cross_entropy_with_logits' `pos_weight` (one float: the path's heads have one logit channel)
 * and `reduction` (0 = 'mean', 1 = 'sum') — loss.py:229-235 passes both through */
int evk_bce_fwd_ex(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                   float label_smoothing, float pos_weight, int32_t reduction, float* loss, double* stats, void* stream);
int evk_bce_bwd_ex(const float* logits, const int64_t* labels, int64_t npix, int64_t ignore_index,
                   float label_smoothing, float pos_weight, int32_t reduction, const double* stats,
                   const float* grad_scale, float* dlogits, int32_t accumulate, void* stream);

/* dice_loss_with_logits — loss.py:40-75.  C==1: p=sigmoid; C>1: p=softmax, one-hot target.
 * 1 <= C <= 16: the softmax statistics keep 256 x 2C doubles in 64 KiB of LDS; evk_dice_stats refuses a larger C.
 * stats: double[2*C] = {inter[c], z[c]} (z = sum p + sum y, before smoothing).  In distributed
 * training the caller all-reduces `stats` between evk_dice_stats and evk_dice_finish
 * (loss.py:20-23,46-48). */
int evk_dice_stats(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
                   int64_t ignore_index, double* stats, void* stream);
int evk_dice_finish(const double* stats, int32_t C, float smooth, int32_t ignore_channel,
                    float* loss, void* stream);
int evk_dice_bwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
                 int64_t ignore_index, const double* stats, float smooth, int32_t ignore_channel,
                 const float* grad_scale, float* dlogits, int32_t accumulate, void* stream);

/* F.cross_entropy(ignore_index) (user model code; label-smoothing variant loss.py:207-219).
 * stats: double[3] = {sum nll, count, sum(-sum_c logp)} ; loss = (1-eps)*nll/count + eps/C*smooth/count */
int evk_ce_fwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
               int64_t ignore_index, float label_smoothing, float* loss, double* stats, void* stream);
int evk_ce_bwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
               int64_t ignore_index, float label_smoothing, const double* stats,
               const float* grad_scale, float* dlogits, int32_t accumulate, void* stream);

/* soft_cross_entropy(input, target) — loss.py:238-242: -(target*log_softmax(input,1)).mean((0,2,3)).sum().
 * target: float [N*H*W, C] (NHWC, same layout as logits).  stats: K = 1. */
int evk_soft_ce_fwd(const float* logits, const float* target, int64_t npix, int32_t C, float* loss,
                    double* stats, void* stream);
int evk_soft_ce_bwd(const float* logits, const float* target, int64_t npix, int32_t C,
                    const float* grad_scale, float* dlogits, void* stream);

/* ------------------------------------------------------------------ optimizer -------------- */
/* torch.optim.SGD step over a flat list of tensors (opt/optimizer.py:7) and
 * clip_grad_norm_ (interface/module.py:96-108).  ptr tables live in device memory. */
/* partial: double[evk_opt_blocks_per_tensor() * ntensors] scratch.  Writes the global L2 norm and
 * clip_coef = min(1, max_norm / (norm + 1e-6)) to device scalars (no host sync). */
int32_t evk_opt_blocks_per_tensor(void);
int evk_sqnorm_multi(const float* const* grads, const int64_t* sizes, int32_t ntensors,
                     double* partial, float max_norm, float* total_norm, float* clip_coef,
                     void* stream);
int evk_sgd_multi(float* const* params, const float* const* grads, float* const* momentum_bufs,
                  const int64_t* sizes, int32_t ntensors, float lr, float momentum, float dampening,
                  float weight_decay, int32_t nesterov, int32_t first_step,
                  const float* clip_coef /* device scalar or NULL */, void* stream);
/* ... with the learning rate read from a device word when lr_dev != NULL (lr is then ignored): a launch captured into a
 * hipGraph (ever_amd/core/graph.py) must follow the schedule on replay. */
int evk_sgd_multi_lr(float* const* params, const float* const* grads, float* const* momentum_bufs,
                     const int64_t* sizes, int32_t ntensors, float lr, const float* lr_dev, float momentum,
                     float dampening, float weight_decay, int32_t nesterov, int32_t first_step,
                     const float* clip_coef, void* stream);
/* torch.optim.Adam (decoupled = 0) / AdamW (decoupled = 1) step, no amsgrad — opt/optimizer.py:8-9 registers both.
 * bias_correction1 = 1 - beta1^step, sqrt_bias_correction2 = sqrt(1 - beta2^step) for the step being taken. */
int evk_adam_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   const int64_t* sizes, int32_t ntensors, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int32_t decoupled, float bias_correction1, float sqrt_bias_correction2,
                   const float* clip_coef /* device scalar or NULL */, void* stream);

/* ------------------------------------------------------------------ "next" rows ---- */
/* Class-probability statistics over the valid pixels: stats[0..C) = tp_c = sum p_c*y_c, [C..2C) = sum p_c,
 * [2C..3C) = sum y_c  (p = sigmoid for C == 1, softmax otherwise; y one-hot / the 0-1 label).  They are the
 * sufficient statistics of tversky_loss_with_logits (reference ever/module/loss.py:78-143; the caller
 * all-reduces them under sync_statistics and forms the ratio), and evk_prob_stats_bwd is their adjoint:
 * dlogits for any loss L(tp, sp) given g_tp[c] = dL/dtp_c, g_sp[c] = dL/dsp_c (device arrays).
 * `stats` needs evk_prob_stats_doubles(C) doubles. */
int64_t evk_prob_stats_doubles(int32_t C);
int evk_prob_stats(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
                   int64_t ignore_index, double* stats, void* stream);
int evk_prob_stats_bwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
                       int64_t ignore_index, const float* g_tp, const float* g_sp, float* dlogits,
                       int32_t accumulate, void* stream);
/* Focal losses on float targets of the logits' shape (any layout; n elements).
 * mode 0: focal_loss(normalize=False), loss.py:158-176 (modulating factor detached);
 * mode 1: sigmoid_focal_loss, loss.py:179-201 (alpha < 0 disables the alpha weighting);
 * mode 2: focal_loss(normalize=True) — the normalisation cancels identically: sum of BCE terms.
 * mean != 0 divides by n.  stats: 1 + 256 doubles. */
int evk_focal_fwd(const float* logits, const float* target, int64_t n, float gamma, float alpha,
                  int32_t mode, int32_t mean, float* loss, double* stats, void* stream);
int evk_focal_bwd(const float* logits, const float* target, int64_t n, float gamma, float alpha,
                  int32_t mode, int32_t mean, const float* grad_scale, float* dlogits, void* stream);
/* cm[t*C + p] += #{i : y_true[i] = t, y_pred[i] = p}; pairs with either index outside [0, C) are skipped
 * (ignore labels).  Replaces the host/scipy.sparse accumulation of ever/metric/confusion_matrix.py:11-24.
 * The _from_logits form fuses the prediction: threshold 0 for one logit channel (classes {0,1}), first
 * argmax otherwise; logits are [npix][C_logits] (NHWC). */
int evk_confusion_matrix(const int64_t* y_true, const int64_t* y_pred, int64_t n, int32_t num_classes,
                         int64_t* cm, void* stream);
int evk_confusion_from_logits(const float* logits, const int64_t* y_true, int64_t npix,
                              int32_t C_logits, int32_t num_classes, int64_t* cm, void* stream);

/* nn.GroupNorm(G, C) (+ReLU) on [N, HW, C] — reference fs_relation.py:88-116 (FSRelationV2 scene encoders).
 * flags bit 0: ReLU fused (backward then needs y).  save_mean / save_rstd: [N*G].  C % 4 == 0, C % G == 0. */
size_t evk_gn_workspace_bytes(int32_t N, int64_t HW, int32_t C, int32_t G);
/* Host only, no launch: the reduce plan evk_gn_fwd / evk_gn_bwd take for one sample's [HW][C] map (refuses what they
 * refuse).  out[4] = { row chunks (workgroups per sample), rows per chunk, threads per row (each walks C / 4 / tpc
 * 16-byte columns), rows in flight per workgroup }.  The workspace holds [N][chunks][2][C] partial sums and 2 N G
 * coefficients, as floats. */
int evk_gn_plan(int64_t HW, int32_t C, int32_t* out);
int evk_gn_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y,
               float* save_mean, float* save_rstd, int32_t N, int64_t HW, int32_t C, int32_t G,
               uint32_t flags, void* workspace, size_t workspace_bytes, void* stream);
int evk_gn_bwd(const float* dy, const float* x, const float* y, const float* gamma,
               const float* save_mean, const float* save_rstd, float* dx, float* dgamma, float* dbeta,
               int32_t N, int64_t HW, int32_t C, int32_t G, uint32_t flags, void* workspace,
               size_t workspace_bytes, void* stream);
/* torch.cat([a, b], dim=1) on NHWC rows and its adjoint (either output of the split may be NULL) —
 * fs_relation.py:155.  Ca, Cb multiples of 4. */
int evk_concat_channels(const float* a, const float* b, float* out, int64_t rows, int32_t Ca,
                        int32_t Cb, void* stream);
int evk_split_channels(const float* src, float* a, float* b, int64_t rows, int32_t Ca, int32_t Cb,
                       void* stream);
/* y[n][hw][c] = x[n][hw][c] * scale[n][c]: nn.Dropout2d with the caller's keep-mask/(1-p) — fs_relation.py:104,
 * 121; the same call is its backward. */
int evk_channel_scale(const float* x, const float* scale, float* y, int32_t N, int64_t HW, int32_t C,
                      void* stream);

/* FS-Relation with its two BatchNorm + ReLU passes inside (reference fs_relation.py:39-53: content / re-encoding =
 * ReLU(BN(conv1x1(p))); :61-71: out = sigmoid(<scene, content>) * re-encoded).  The stand-alone passes wrote both normalised
 * maps only for the relation kernel to read them back, and their backward read (g, z) of both once more just for the
 * per-channel sums.  Here:
 *  - evk_bn_finalize_parts merges the producing convolution's statistics records (evk_conv2d_fwd_f16x2: bn_parts) into
 *    save_mean / save_invstd / scale_shift [2][C] and updates the running statistics — no apply pass;
 *  - evk_relation_bn_fwd reads the convolution outputs zc, zf and applies scale / shift / ReLU on the fly; it raises the
 *    64 slots of out_absmax (zero on entry; may be NULL) with max|out|;
 *  - evk_relation_bn_bwd rebuilds both activations from z, writes the MASKED gradients gc, gf (w.r.t. the BatchNorm
 *    outputs, zero where the ReLU was off) and leaves, per workgroup, (sum g, sum g * xhat) and (max|g|, max|xhat|) of both
 *    BatchNorms in the workspace: floats [nb C] scene partials | content sums [nb][2][C] | content maxima [nb][2][C] |
 *    re-encoding sums | re-encoding maxima, nb = evk_relation_bn_parts(N, HW); mean_invstd = save_mean, save_invstd
 *    contiguous [2][C];
 *  - evk_bn_bwd_from_partials turns such records into dgamma, dbeta and dx = BatchNorm backward of the masked g (with
 *    EVK_BN_PACK_DX: packed, dx_absmax zero on entry); workspace 16 C floats. */
int evk_bn_finalize_parts(const float* parts, int32_t nparts, int32_t C, int64_t rows, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                          float* save_invstd, float* scale_shift, void* stream);
int evk_relation_bn_fwd(const float* scene, const float* zc, const float* scale_shift_c, const float* zf,
                        const float* scale_shift_f, float* out, float* r, int32_t N, int32_t HW, int32_t C,
                        uint32_t* out_absmax, void* stream);
int32_t evk_relation_bn_parts(int32_t N, int32_t HW);
size_t evk_relation_bn_workspace_bytes(int32_t N, int32_t HW, int32_t C);
int evk_relation_bn_bwd(const float* dout, const float* scene, const float* zc, const float* scale_shift_c,
                        const float* mean_invstd_c, const float* zf, const float* scale_shift_f, const float* mean_invstd_f,
                        const float* r, float* dscene, float* gc, float* gf, int32_t N, int32_t HW, int32_t C, void* workspace,
                        size_t workspace_bytes, void* stream);
int evk_bn_bwd_from_partials(const float* g, const float* x, const float* gamma, const float* save_mean,
                             const float* save_invstd, const float* partial, const float* maxima, int32_t nparts, float* dx,
                             float* dgamma, float* dbeta, int64_t rows, int32_t C, uint32_t flags, int32_t train,
                             void* workspace, size_t workspace_bytes, uint32_t* dx_absmax, void* stream);

/* BatchNorm + ReLU + a narrow 1x1 convolution as ONE consumer of a convolution output z (the decoder's classifier applied
 * per branch: reference fpn.py:163-170 `conv3x3 -> BN -> ReLU`, :179-193 the 1x1 classifier; ever_amd/module/fpn.py runs the
 * classifier before the last upsampling): out[pix][k] = sum_c relu(bn(z))[pix][c] * w[k][c] + bias[k], K <= 16.  The
 * normalised map is never written.  scale_shift / save_mean / save_invstd from evk_bn_finalize_parts.  Backward: dl
 * [rows][K] -> dz (gradient of z; EVK_BN_PACK_DX: packed, dx_absmax zero on entry), dgamma, dbeta, dw [K][C], dbias [K];
 * it reads z twice and never forms the C-channel gradient of the normalised map.
 * evk_bn_relu_dot_plan (host only, no launch) answers what both do with a [rows][C] map and K classes: out[5] = {workgroups,
 * pixels per workgroup, NCH, KT, dynamic LDS bytes of the backward} — a lane owns NCH (1, 2, 4) 16-byte channel chunks, KT
 * (1, 4, 16) classes are unrolled.  It returns what evk_bn_relu_dot_bwd returns for the same shape: EVK_E_UNSUPPORTED for a
 * C / K without an instantiation or beyond the LDS (16 (4 + K) C <= 65536), EVK_E_INVALID for a null `out`. */
int evk_bn_relu_dot_plan(int64_t rows, int32_t C, int32_t K, int32_t* out);
int evk_bn_relu_dot_fwd(const float* z, const float* scale_shift, const float* w, const float* bias, float* out, int64_t rows,
                        int32_t C, int32_t K, void* stream);
size_t evk_bn_relu_dot_workspace_bytes(int64_t rows, int32_t C, int32_t K);
int evk_bn_relu_dot_bwd(const float* dl, const float* z, const float* scale_shift, const float* gamma, const float* save_mean,
                        const float* save_invstd, const float* w, float* dz, float* dgamma, float* dbeta, float* dw,
                        float* dbias, int64_t rows, int32_t C, int32_t K, uint32_t flags, void* workspace,
                        size_t workspace_bytes, uint32_t* dx_absmax, void* stream);

/* Synchronized BatchNorm in stages (torch.nn.SyncBatchNorm under the trainer's `sync_bn`, reference
 * ever/trainer/th_ddp_trainer.py + SURVEY §8 C5): the exchange between the stages is the caller's
 * (torch.distributed over RCCL): forward all-gather of `stats` (local mean, local sum of squared deviations,
 * fp64 [2C]) + the row count; backward all-reduce of `sums` (sum g, sum g*xhat, fp64 [2C]).
 * Workspace: evk_bn_workspace_bytes(rows, C).  flags / y / d_residual as evk_bn_fwd_train / evk_bn_bwd. */
int evk_bn_local_stats(const float* x, double* stats, int64_t rows, int32_t C, void* workspace,
                       size_t workspace_bytes, void* stream);
int evk_bn_apply_stats(const float* x, const float* residual, const float* gamma, const float* beta,
                       const float* mean, const float* invstd, float* y, int64_t rows, int32_t C,
                       uint32_t flags, void* workspace, size_t workspace_bytes, void* stream);
int evk_bn_bwd_local_sums(const float* dy, const float* x, const float* y, const float* gamma,
                          const float* beta, const float* mean, const float* invstd, float* d_residual,
                          double* sums, int64_t rows, int32_t C, uint32_t flags, void* workspace,
                          size_t workspace_bytes, void* stream);
int evk_bn_bwd_apply_sums(const float* dy, const float* x, const float* y, const float* gamma,
                          const float* beta, const float* mean, const float* invstd, const float* mean_g,
                          const float* mean_gx, float* dx, int64_t rows, int32_t C, uint32_t flags,
                          void* workspace, size_t workspace_bytes, void* stream);

/* dst[offsets[t] + i] = srcs[t][i] * scale for t < ntensors (a NULL source packs zeros): one launch gathers the
 * gradients of a bucket into the flat RCCL all-reduce buffer, pre-divided by the world size — the gradient
 * exchange of the DDP trainer (reference ever/trainer/th_ddp_trainer.py: DistributedDataParallel's reducer).
 * srcs / sizes / offsets are device arrays.  A source may be EXACTLY its own destination slot (srcs[t] == dst +
 * offsets[t]: gradient accumulation over several backward passes without no_sync, reference core/launcher.py:196,317-321 —
 * the second pass accumulates into the bucket view and the pack scales it in place); partially overlapping ranges are not
 * allowed.  tests/world2_gpu_worker.py:case_forward_times_2 holds the in-place case at world size 2. */
int evk_pack_multi(const float* const* srcs, const int64_t* sizes, const int64_t* offsets,
                   int32_t ntensors, float scale, float* dst, void* stream);

/* F.cross_entropy(reduction='none', ignore_index) per pixel (0 on ignored pixels) and its backward with a per-pixel
 * upstream gradient — the input of online_hard_example_mining. */
int evk_ce_pixel_fwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
                     int64_t ignore_index, float* loss_pix, void* stream);
int evk_ce_pixel_bwd(const float* logits, const int64_t* labels, int64_t npix, int32_t C,
                     int64_t ignore_index, const float* grad_pix, float* dlogits, void* stream);
/* online_hard_example_mining (reference loss.py:146-155): loss = mean of the non-zero values among the `keep`
 * largest of losses[0..n); exact k-th value by a 3-pass radix select.  `state`: evk_ohem_state_bytes() bytes, kept
 * for the backward (dlosses = grad / #kept on the kept non-zero elements, 0 elsewhere). */
int64_t evk_ohem_state_bytes(void);
int evk_ohem_fwd(const float* losses, int64_t n, int64_t keep, float* loss, void* state, void* stream);
int evk_ohem_bwd(const float* losses, int64_t n, void* state, const float* grad_scale, float* dlosses,
                 void* stream);

/* ------------------------------------------------------------------ depthwise convolution --- */
/* nn.Conv2d(C, C, k, groups=C) — reference ops.py:25-31 (DepthwiseConv2d), :34-42 (SeparableConv2d's first
 * convolution; SeparableConvBlock in deeplabv3p_head.py:36-38).  Exact fp32 FMA on the vector ALUs in every arithmetic
 * mode (the convolution is HBM-bound).  Descriptor: Cin == Cout = C, C % 4 == 0, kh, kw in 1..7, stride 1 or 2 on each
 * axis, any dilation, any zero padding; anything else returns EVK_E_UNSUPPORTED before a launch.  w: the [C][1][kh][kw]
 * parameter ([C][kh][kw] memory); bias may be NULL; flags: EVK_CONV_RELU.  x / y NHWC. */
int evk_depthwise_fwd(const evk_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                      uint32_t flags, void* stream);
/* Host only: bytes of the per-tile weight / bias gradient records of evk_depthwise_bwd (0 for a descriptor out of scope). */
size_t evk_depthwise_bwd_workspace_bytes(const evk_conv_desc* d);
/* Host only (no launch): the kernel forms and tilings evk_depthwise_fwd / _bwd and the workspace size take for a descriptor,
 * from the function they take them from.  out = {forward <KW, SW, D1> (3), forward strips of 8 output pixels per row,
 * forward workgroups, backward <KW, S1D1> (2), channel lanes cl (a power of two <= 64, of 4 channels each), strips of 4
 * pixels per workgroup ps (cl * ps == 256), backward strips per row (over max(W, Wo)), strip groups, row tiles (4 rows, over
 * max(H, Ho)), channel blocks, tiles = N * row tiles * strip groups}; workspace bytes = tiles * (kh * kw + 1) * C * 4.
 * It refuses what the launches refuse, and a workgroup, tile or channel-block count that does not fit the grid; `out` is
 * untouched then. */
int evk_depthwise_plan(const evk_conv_desc* d, int32_t* out /*[14]*/);
/* Gradients of evk_depthwise_fwd: dx (may be NULL), dw [C][kh][kw] and db [C] (either may be NULL; then x may be NULL
 * too).  y: the forward's output when it fused the ReLU (the mask), else NULL.  One pass over dy and x writes dx and a
 * record of dw / db partial sums per tile; a second kernel sums the records in a fixed order (no atomics). */
int evk_depthwise_bwd(const evk_conv_desc* d, const float* dy, const float* x, const float* y, const float* w,
                      float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* dst[n][p][c] = src[n][c] for p < HW: F.interpolate of a 1x1 map to any size (bilinear, align_corners=False), which is
 * an exact broadcast — reference ops.py:96-100 (PoolBlock).  evk_sum_hw is its adjoint: dst[n][c] = sum over p of
 * src[n][p][c] in a fixed order.  C % 4 == 0. */
int evk_broadcast_hw(const float* src, float* dst, int32_t N, int64_t HW, int32_t C, void* stream);
int evk_sum_hw(const float* src, float* dst, int32_t N, int64_t HW, int32_t C, void* stream);

/* ------------------------------------------------------------------ row LayerNorm, layer-scale residual --- */
/* LayerNorm over the C floats of a row of a dense [R][C] fp32 matrix: ConvNeXt's LayerNorm in both data formats (a
 * logical-NCHW map is NHWC memory: one row per pixel) and nn.LayerNorm(C) on tokens — reference
 * dinov3/models/convnext.py:86-113,177,224.  y = (x - mean) * rstd * gamma + beta, biased variance,
 * rstd = 1 / sqrt(var + eps); the variance is the sum of squared residuals, never E[x^2] - mean^2.  gamma / beta may be
 * NULL (no affine), save_mean / save_rstd [R] may be NULL (inference).  Scope: C % 4 == 0, 4 <= C <= 2048, R >= 1, dense
 * rows, 16-byte aligned pointers; anything else returns EVK_E_INVALID / EVK_E_UNSUPPORTED before a launch.
 * evk_ln_plan (host only): out = {lanes per row L (a power of two <= 64), 16-byte columns per lane (L * columns >= C / 4 >
 * L * (columns - 1)), rows per workgroup per trip, workgroups (bounded whatever R is)}; it refuses what the launches refuse. */
int evk_ln_plan(int64_t R, int32_t C, int32_t* out /*[4]*/);
/* Host only: bytes of the per-workgroup dgamma / dbeta records of evk_ln_bwd, [workgroups][2][C] floats (0 out of scope). */
size_t evk_ln_bwd_workspace_bytes(int64_t R, int32_t C);
int evk_ln_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, float* save_mean,
               float* save_rstd, int64_t R, int32_t C, void* stream);
/* Gradients of evk_ln_fwd in one pass over dy and x: dx, dgamma [C], dbeta [C], each may be NULL (not all three).  The
 * workspace is needed for dgamma / dbeta only; its records are summed in a fixed order (no atomics: same bits every run). */
int evk_ln_bwd(const float* dy, const float* x, const float* save_mean, const float* save_rstd, const float* gamma,
               float* dx, float* dgamma, float* dbeta, int64_t R, int32_t C, void* workspace, size_t workspace_bytes,
               void* stream);
/* The tail of a ConvNeXt block, input + drop_path(gamma * x) (convnext.py:20-28,78-82), on [N][HW][C] fp32:
 * y = a + (s[n] * gamma[c]) * z with every product and the sum rounded on its own, in that order.  gamma [C] may be NULL
 * (no layer scale), sample_scale s [N] may be NULL (eval mode, rate 0); it holds floor(keep + u) / keep per sample.
 * Same scope and thread plan as evk_ln_* (evk_ln_plan(N * HW, C)). */
int evk_scale_residual_fwd(const float* a, const float* z, const float* gamma, const float* sample_scale, float* y,
                           int32_t N, int64_t HW, int32_t C, void* stream);
/* Host only: bytes of the per-workgroup dgamma records of evk_scale_residual_bwd, [workgroups][C] floats (0 out of scope). */
size_t evk_scale_residual_bwd_workspace_bytes(int32_t N, int64_t HW, int32_t C);
/* dz = (s[n] * gamma[c]) * dy (may be NULL), dgamma[c] = sum over n, p of s[n] * (dy * z) (may be NULL; then z and the
 * workspace may be NULL too), summed in a fixed order.  The gradient of a is dy itself. */
int evk_scale_residual_bwd(const float* dy, const float* z, const float* gamma, const float* sample_scale, float* dz,
                           float* dgamma, int32_t N, int64_t HW, int32_t C, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ------------------------------------------------------------------ RoPE self-attention, token prefix --- */
/* Multi-head self-attention with axial RoPE on Q and K — reference dinov3/layers/attention.py:16-27,66-85,106-118.
 * qkv [B][N][3][H][D] fp32 (the QKV Linear's output as it lies), o [B][N][H*D] (what the projection Linear takes), scale
 * 1/sqrt(D), softmax over all N keys, exact fp32 MFMA under every arithmetic mode.  The first `prefix` tokens are not
 * rotated; token n >= prefix takes row n - prefix of sin / cos [N - prefix][D]: y = x cos + rotate_half(x) sin,
 * rotate_half([x1, x2]) = [-x2, x1] over the halves of D.  sin == cos == NULL: no RoPE; prefix == N: no rotated token.
 * Scope: D in {32, 64} (else EVK_E_UNSUPPORTED), H * D % 4 == 0, B, H, N >= 1, 0 <= prefix <= N, 16-byte aligned pointers
 * (else EVK_E_INVALID); all refused before a launch.
 * evk_attn_plan (host only): out = {query tile Tq, key tile Tk, key trips ceil(N / Tk), workgroups of each tiled kernel,
 * LDS bytes of the forward and dQ kernels, LDS bytes of the dK / dV kernel}; it refuses what the launches refuse. */
int evk_attn_plan(int32_t B, int32_t N, int32_t H, int32_t D, int32_t prefix, int32_t* out /*[6]*/);
/* lse [B][H][N] (log-sum-exp of the scaled logits, what the backward recomputes P from) may be NULL: inference. */
int evk_attn_fwd(const float* qkv, const float* sin, const float* cos, float* o, float* lse, int32_t B, int32_t N, int32_t H,
                 int32_t D, int32_t prefix, void* stream);
/* Host only: bytes of delta [B][N][H] = rowsum(do * o), written by a pre-pass of evk_attn_bwd (0 out of scope). */
size_t evk_attn_bwd_workspace_bytes(int32_t B, int32_t N, int32_t H, int32_t D);
/* dqkv [B][N][3][H][D]: the gradient with respect to the UN-rotated q and k (the adjoint of the rotation is general: any
 * sin / cos) and v; every element is written.  One kernel owns a key tile for dK / dV, one a query tile for dQ; no float
 * atomics, the same bits every run.  dqkv == NULL: nothing to do. */
int evk_attn_bwd(const float* qkv, const float* sin, const float* cos, const float* o, const float* d_o, const float* lse,
                 float* dqkv, int32_t B, int32_t N, int32_t H, int32_t D, int32_t prefix, void* workspace,
                 size_t workspace_bytes, void* stream);
/* out [B][P + HW][C] = cat(prefix [P][C] broadcast over the batch, patch [B][HW][C]) — prepare_tokens_with_masks without
 * masks (dinov3/models/vision_transformer.py:201-231).  P >= 1, C % 4 == 0, 16-byte aligned pointers. */
int evk_tokens_prepend_fwd(const float* patch, const float* prefix, float* out, int32_t B, int64_t HW, int32_t P, int32_t C,
                           void* stream);
/* dpatch [B][HW][C] (may be NULL) and dprefix [P][C] = sum over b, in batch order, of dout[b][:P] (may be NULL). */
int evk_tokens_prepend_bwd(const float* dout, float* dpatch, float* dprefix, int32_t B, int64_t HW, int32_t P, int32_t C,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVER_HIP_H_ */
