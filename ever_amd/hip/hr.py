"""HRNet family of the host wrappers (include/ever_hip.h: evk_hr_fuse_*, evk_upsample_bilinear_slice_*): the multi-resolution
exchange that ends a HighResolutionModule (reference _hrnet.py:377-397) as one autograd node per output, and the head's
bilinear up-sampling straight into the concat buffer (hrnet_head.py:17-25).  Part of the hip/functional.py facade."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from . import weight_planes
from .workspace import workspace
from ._base import (
    HipPathError, _amax_out, _amax_zeroed, _f16x2, _is_packed, _mark_packed, _note_amax, _ptr, _refuse_packed, _require_cuda,
    _stream, _take_parts, _timed_call, as_nhwc, empty_nhwc, i32_array, materialize_lazy, ptr_array,
)

__all__ = ['hr_fuse', 'bilinear_concat', 'hr_fuse_stats']

_PLAIN, _BN_BATCH, _BN_RUNNING = 0, 1, 2     # how a term enters the sum
_Y_AMAX = [None]                             # scale buffer of the sum that has just been written, for hr_fuse() to note on it
hr_fuse_stats = {'nodes': 0, 'plain': 0, 'bn_batch': 0, 'bn_running': 0}   # how the terms entered (tests / tools)


class _HrFuseFn(Function):
    """y = ReLU(((t0 + t1) + t2) + t3): every term read at its own resolution (nearest x 2^shift), a BatchNorm term as
    scale / shift of the raw convolution output; y's ReLU bits are kept instead of y.  Backward: one read of dy and the bits
    gives the masked gradient and its 2^s x 2^s block sums; a BatchNorm term then runs the BatchNorm backward on its share.
    cfg[k] = (shift, mode, (parts, running_mean, running_var, momentum, eps)); tensors = the terms, then (gamma, beta) per term."""

    @staticmethod
    def forward(ctx, cfg, *ts):
        nt = len(cfg)
        terms, affine = ts[:nt], ts[nt:]
        n, c = terms[0].shape[0], terms[0].shape[1]
        h, w = terms[0].shape[2] << cfg[0][0], terms[0].shape[3] << cfg[0][0]
        dev, st = terms[0].device, _stream()
        stats = []
        for k, (shift, mode, bn_cfg) in enumerate(cfg):
            if mode == _PLAIN:
                stats.append(None)
                continue
            parts, rm, rv, mom, eps = bn_cfg
            gamma, beta = affine[2 * k], affine[2 * k + 1]
            s = torch.empty((4, c), device=dev, dtype=torch.float32)      # mean, invstd, scale, shift
            if mode == _BN_BATCH:
                _C.call('evk_bn_finalize_parts', parts[0].data_ptr(), parts[1], c, terms[k].numel() // c, _ptr(gamma), _ptr(beta),
                        _ptr(rm), _ptr(rv), float(mom), float(eps), s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), st)
            else:       # running statistics: a per-channel affine map with constant coefficients ([C]-sized host arithmetic)
                s[0] = rm
                s[1] = torch.rsqrt(rv + eps)
                s[2] = s[1] if gamma is None else gamma.detach() * s[1]
                s[3] = -rm * s[2] if beta is None else beta.detach() - rm * s[2]
            stats.append(s)
        y = empty_nhwc(n, c, h, w, dev)
        bits = torch.empty((_C.load().evk_relu_bits_bytes(y.numel()) // 4,), device=dev, dtype=torch.int32)
        abits = _amax_zeroed(dev)        # the sum is the operand of the next module's convolutions
        tp, sh = ptr_array(terms), i32_array([k[0] for k in cfg])
        sp = ptr_array([None if s is None else s[2] for s in stats])
        # algorithmic bytes: every term once at its own size, y and its bits
        nb = 4.0 * (sum(t.numel() for t in terms) + y.numel()) + 4.0 * bits.numel()
        _timed_call('hr_fuse', nb, 'evk_hr_fuse_fwd', tp, sh, sp, nt, y.data_ptr(), bits.data_ptr(), _ptr(abits), n, h, w, c, st)
        _Y_AMAX[0] = abits
        ctx.cfg = tuple((shift, mode, bool(mode == _BN_BATCH and len(bn_cfg[0]) > 2 and bn_cfg[0][2])) for shift, mode, bn_cfg in cfg)
        ctx.dims = (n, c, h, w)
        ctx.save_for_backward(bits, *[t if cfg[k][1] != _PLAIN else None for k, t in enumerate(terms)],
                              *[affine[2 * k] for k in range(nt)], *stats)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        nt = len(ctx.cfg)
        bits, zs, gammas, stats = saved[0], saved[1:1 + nt], saved[1 + nt:1 + 2 * nt], saved[1 + 2 * nt:]
        n, c, h, w = ctx.dims
        dev, st = dy.device, _stream()
        dy = as_nhwc(materialize_lazy(dy), 'hr_fuse.backward')
        need = ctx.needs_input_grad        # [cfg, terms..., (gamma, beta)...]
        wants = [need[1 + k] or (ctx.cfg[k][1] != _PLAIN and (need[1 + nt + 2 * k] or need[2 + nt + 2 * k])) for k in range(nt)]
        # one launch: the masked gradient for the plain same-resolution terms (a branch output feeds several sums and autograd
        # adds their gradients: it is written masked, never handed on with the bits) and a block sum per coarser resolution
        dmasked = torch.empty_like(dy) if any(wants[k] and s == 0 and m == _PLAIN for k, (s, m, _) in enumerate(ctx.cfg)) else None
        pooled = {s: empty_nhwc(n, c, h >> s, w >> s, dev) for s in {s for k, (s, _, _) in enumerate(ctx.cfg) if wants[k] and s}}
        if dmasked is not None or pooled:
            nb = 4.0 * (dy.numel() + (dy.numel() if dmasked is not None else 0) + sum(p.numel() for p in pooled.values()))
            _timed_call('hr_fuse', nb + 4.0 * bits.numel(), 'evk_hr_fuse_bwd', dy.data_ptr(), bits.data_ptr(), _ptr(dmasked),
                        _ptr(pooled.get(1)), _ptr(pooled.get(2)), _ptr(pooled.get(3)), n, h, w, c, st)
        lib = _C.load()
        gt, ga = [None] * nt, [None] * (2 * nt)
        for k, (shift, mode, pack) in enumerate(ctx.cfg):
            if not wants[k]:
                continue
            if mode == _PLAIN:
                gt[k] = dmasked if shift == 0 else pooled[shift]
                continue
            z, gamma, s = zs[k], gammas[k], stats[k]
            rows = z.numel() // c
            ws_bytes = lib.evk_bn_workspace_bytes(rows, c)
            ws = workspace(dev, ws_bytes)
            pack = pack and _f16x2()
            abits = _amax_zeroed(dev) if pack else _amax_out(dev)
            pack = pack and abits is not None
            dz = torch.empty_like(z)
            dgamma = torch.empty((c,), device=dev, dtype=torch.float32) if gamma is not None else None
            dbeta = torch.empty((c,), device=dev, dtype=torch.float32) if gamma is not None else None
            tail = (rows, c, 2 if pack else 0, 1 if mode == _BN_BATCH else 0, ws.data_ptr(), ws_bytes, _ptr(abits))
            if shift == 0:      # same resolution: the unmasked dy with y's bits as its mask
                _timed_call('bn', 20.0 * z.numel(), 'evk_bn_bwd_bits', dy.data_ptr(), z.data_ptr(), None, _ptr(gamma), None,
                            s[0].data_ptr(), s[1].data_ptr(), dz.data_ptr(), None, _ptr(dgamma), _ptr(dbeta), *tail,
                            bits.data_ptr(), st)
            else:               # coarser: the block sum of the masked dy
                _timed_call('bn', 20.0 * z.numel(), 'evk_bn_bwd', pooled[shift].data_ptr(), z.data_ptr(), None, _ptr(gamma), None,
                            s[0].data_ptr(), s[1].data_ptr(), dz.data_ptr(), None, _ptr(dgamma), _ptr(dbeta), *tail, st)
            if pack:
                _mark_packed(dz, abits)
            elif abits is not None:
                _note_amax(dz, abits)
            gt[k] = dz if need[1 + k] else None
            ga[2 * k] = dgamma if need[1 + nt + 2 * k] else None
            ga[2 * k + 1] = dbeta if need[2 + nt + 2 * k] else None
        return (None, *gt, *ga)


def _fusable_bn(bn):
    """a BatchNorm2d whose apply pass hr_fuse may absorb: not SyncBatchNorm (its statistics are exchanged across ranks first),
    momentum set, and no hook that expects to see its input or output"""
    return (isinstance(bn, torch.nn.BatchNorm2d) and not isinstance(bn, torch.nn.SyncBatchNorm) and bn.momentum is not None
            and not (bn._forward_hooks or bn._forward_pre_hooks))


def hr_fuse(terms):
    """`relu(sum_j T_j)` of a HighResolutionModule output (reference _hrnet.py:385-395) as one autograd node.  terms: up to four
    `(tensor, shift, bn_or_None)`, summed in order; a term is `[N, C, H >> shift, W >> shift]` and enters at output pixel
    (y, x) as its pixel (y >> shift, x >> shift) — nearest up-sampling by 2^shift.  With a BatchNorm2d the tensor is the RAW
    output of the convolution before it: in training mode with the convolution's statistics records on it
    (`conv(x, bn_stats=True)`), which are finalised here (running statistics updated); in eval mode the running statistics
    give scale and shift.  A BatchNorm this form cannot absorb (no records on the tensor, SyncBatchNorm or a foreign norm,
    hooks) is applied by its own forward and its output enters as a plain term."""
    if not 1 <= len(terms) <= 4:
        raise ValueError(f'hr_fuse: 1 to 4 terms, got {len(terms)}')
    ts, cfg, affine = [], [], []
    for t, shift, bn in terms:
        _require_cuda(t, 'hr_fuse')
        t = as_nhwc(t, 'hr_fuse')
        mode, bn_cfg = _PLAIN, None
        if bn is not None:
            batch = bn.training or getattr(bn, 'running_mean', None) is None
            parts = getattr(t, '_evk_bn_parts', None) if batch else None
            if not _fusable_bn(bn) or t.shape[1] % 4 or (batch and (parts is None or parts[1] <= 0)):
                t = as_nhwc(bn(t), 'hr_fuse')       # layer by layer: the module's own forward (and hooks)
            elif batch:
                _take_parts(t)
                track = bn.track_running_stats and bn.running_mean is not None
                if track:
                    weight_planes.note_running_stats_changed()
                    if bn.num_batches_tracked is not None:
                        bn._nbt_pending = getattr(bn, '_nbt_pending', 0) + 1
                mode = _BN_BATCH
                bn_cfg = (parts, bn.running_mean if track else None, bn.running_var if track else None, bn.momentum, bn.eps)
            else:
                mode, bn_cfg = _BN_RUNNING, (None, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
        _refuse_packed('hr_fuse', 'a term', t)
        ts.append(t)
        cfg.append((int(shift), mode, bn_cfg))
        affine += [bn.weight, bn.bias] if mode != _PLAIN else [None, None]
    n, c = ts[0].shape[0], ts[0].shape[1]
    h, w = ts[0].shape[2] << cfg[0][0], ts[0].shape[3] << cfg[0][0]
    for t, (shift, _, _) in zip(ts, cfg):
        if not 0 <= shift <= 3 or h % (1 << shift) or w % (1 << shift) or tuple(t.shape) != (n, c, h >> shift, w >> shift):
            raise ValueError(f'hr_fuse: a term of shape {tuple(t.shape)} with shift {shift} does not fit the output '
                             f'{(n, c, h, w)} (shift 0..3, H and W multiples of 2^shift)')
    hr_fuse_stats['nodes'] += 1
    for _, mode, _ in cfg:
        hr_fuse_stats[('plain', 'bn_batch', 'bn_running')[mode]] += 1
    _Y_AMAX[0] = None
    y = _HrFuseFn.apply(tuple(cfg), *ts, *affine)
    if _Y_AMAX[0] is not None:
        _note_amax(y, _Y_AMAX[0])
        _Y_AMAX[0] = None
    return y


class _BilinearConcatFn(Function):
    @staticmethod
    def forward(ctx, ho, wo, *feats):
        n, dev, st = feats[0].shape[0], feats[0].device, _stream()
        ctot = sum(f.shape[1] for f in feats)
        out = empty_nhwc(n, ctot, ho, wo, dev)
        c0 = 0
        for f in feats:
            _, c, h, w = f.shape
            _timed_call('resample_loss', 4.0 * (f.numel() + n * ho * wo * c), 'evk_upsample_bilinear_slice_fwd', f.data_ptr(),
                        out.data_ptr(), n, h, w, ho, wo, c, c0, ctot, st)
            c0 += c
        ctx.shapes = [tuple(f.shape) for f in feats]
        ctx.size = (ho, wo, ctot)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ho, wo, ctot = ctx.size
        dy = as_nhwc(materialize_lazy(dy), 'bilinear_concat.backward')
        st, grads, c0 = _stream(), [], 0
        for k, (n, c, h, w) in enumerate(ctx.shapes):
            dx = None
            if ctx.needs_input_grad[2 + k]:
                dx = empty_nhwc(n, c, h, w, dy.device)
                _timed_call('resample_loss', 4.0 * (dx.numel() + n * ho * wo * c), 'evk_upsample_bilinear_slice_bwd',
                            dy.data_ptr(), dx.data_ptr(), n, h, w, ho, wo, c, c0, ctot, st)
            grads.append(dx)
            c0 += c
        return (None, None, *grads)


def bilinear_concat(feats, size=None):
    """`torch.cat([F.interpolate(f, size, mode='bilinear', align_corners=True) for f in feats], dim=1)` (reference
    hrnet_head.py:17-23; a feature already of that size is copied): every source is written straight into its channel slice
    of the result, no up-sampled intermediate exists.  size defaults to the first feature's."""
    feats = [as_nhwc(f, 'bilinear_concat') for f in feats]
    ho, wo = (feats[0].shape[2], feats[0].shape[3]) if size is None else (int(size[0]), int(size[1]))
    if any(f.shape[0] != feats[0].shape[0] for f in feats):
        raise ValueError('bilinear_concat: batch sizes differ')
    if any(_is_packed(f) for f in feats):
        raise HipPathError('bilinear_concat: a packed activation cannot be resampled')
    return _BilinearConcatFn.apply(ho, wo, *feats)
